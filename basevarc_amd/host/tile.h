// tile.h -- one tile of positions of a phase-2 thread: what stage 1 put into it, the buffers of its library call, what came back.
// Included through tile_runner.h by main.cpp alone: PinnedBytes calls libbvc.
#ifndef BVC_HOST_TILE_H
#define BVC_HOST_TILE_H

#include <condition_variable>
#include <cstring>
#include <deque>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "pileup.h"
#include "../../include/bvc.h"

namespace bvchost {

// a reference letter as libbvc takes it
inline int8_t ref_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
inline void bvc_check(bvc_ctx *ctx, int rc) { if (rc != BVC_OK) throw std::runtime_error(std::string("libbvc: ") + bvc_last_error(ctx)); }

// What every feed of a thread's compute phase works on: the positions of the region with the reference's bases, the thread's share
// of them and the positions a tile holds at most.
struct Window {
    const std::vector<int32_t> &pv;
    const std::string &refseq;
    int32_t rg_s;
    size_t lo, hi;
    int64_t tile;
    int8_t ref_at(int32_t p) const { return ref_code(refseq[(size_t)(p - rg_s)]); }
};

// What stage 1 put into a tile: the columns the CPU parser built, or what the device parses -- the lines of its positions, or their
// binary records (bvc_pileup_begin / bvc_pileup_begin_bin), or its positions of the batches kept on the device (bvc_pileup_begin_store)
enum class TileForm { Sites, Text, Records, Stored };
// Where the VCF columns of a device-parsed tile's called positions come from: the entries of every position on the host (entry_off
// says where), the entries of the called positions alone (called_off), the columns' text from the device (vtext_off / vtext_len), or
// their finished BGZF blocks (vcomp_off).  TileRunner::finish_tile sets it.
enum class CalledFrom { HostEntries, HostCalledEntries, DeviceText, DeviceBlocks };

// Bytes in page-locked memory of the library's (bvc_host_alloc), which go over the link from where they lie: a tile's compressed blocks
// on their way up, gathered one after the other (append), or room for what the device sends down (reserve).
struct PinnedBytes {
    unsigned char *p = nullptr;
    size_t n = 0, cap = 0;
    PinnedBytes() = default;
    PinnedBytes(const PinnedBytes &) = delete;
    PinnedBytes &operator=(const PinnedBytes &) = delete;
    ~PinnedBytes() { bvc_host_free(p); }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    unsigned char *data() { return p; }
    void clear() { n = 0; }
    // room for `need` bytes (and a quarter more where it has to grow); what was there is gone
    void reserve(size_t need)
    {
        n = 0;
        if (need <= cap) return;
        bvc_host_free(p);
        p = nullptr; cap = 0;
        const size_t want = need + need / 4 + 4096;
        p = static_cast<unsigned char *>(bvc_host_alloc(want));
        if (!p) throw std::runtime_error("ERROR: page-locked host memory is not to be had (bvc_host_alloc)");
        cap = want;
    }
    void append(const unsigned char *src, size_t len)
    {
        const size_t need = ((n + len + 3) & ~(size_t)3) + 16;
        if (need > cap) {
            const size_t want = std::max(need + need / 2, (size_t)1 << 20);
            unsigned char *q = static_cast<unsigned char *>(bvc_host_alloc(want));
            if (!q) throw std::runtime_error("ERROR: page-locked host memory is not to be had (bvc_host_alloc)");
            if (n) std::memcpy(q, p, n);
            bvc_host_free(p);
            p = q; cap = want;
        }
        std::memcpy(p + n, src, len);
        n += len;
        while (n & 3) p[n++] = 0;                                // every payload from a 4-byte boundary
    }
};

// One tile of positions on its way through a runner: parsed (stage 1), handed to libbvc (stage 2), written out (stage 3).
struct Tile {
    TileForm form = TileForm::Sites;
    CalledFrom called_from = CalledFrom::HostEntries;
    // the tile's positions: slots [0, n_used) of `sites` (the slots and their vectors are reused from tile to tile)
    std::vector<SiteColumn> sites;
    size_t n_used = 0;
    size_t entries = 0;                  // observations held by the slots in use
    std::vector<int8_t> refs;
    SiteColumn &slot()
    {
        if (n_used == sites.size()) sites.emplace_back();
        return sites[n_used];
    }
    // buffers of the library call and its records: live as long as the tile, refilled, not reallocated
    std::vector<bvc_site_result> res;
    std::vector<bvc_group_result> gres;
    PackedTile in;
    // -- a tile whose text or records the DEVICE parses (bvc_pileup_begin[_bin] / bvc_pileup_finish): the inflated lines of its
    //    positions (the records: text = the records, line_start = where each begins), batch after batch, as they came out of the temp
    //    files; what comes back are the columns and tallies the CPU parser would have built
    size_t n_pos = 0;                    // positions of the tile (with or without entries)
    std::vector<int32_t> pos;            // their coordinates
    std::vector<char> text;
    std::vector<uint32_t> line_start;    // [n_batches][n_pos + 1]
    std::vector<int64_t> entry_off;
    std::vector<int64_t> called_off;     // where the entries of a CALLED position are in ent / samples (CalledFrom::HostCalledEntries)
    std::vector<int32_t> tally, samples;
    std::vector<bvc_pileup_entry> ent;
    std::vector<bvc_pileup_indel> indels;
    std::vector<bvc_site_stats> stats;   // per position, where the device computed them (empty: vcf_line tallies the entries itself)
    // the called positions' sample columns where the device formatted them (CalledFrom::DeviceText): position t's are vtext_len[t] bytes
    // at vout + vtext_off[t]; page-locked memory that grows on demand and lives as long as the tile.  (Both arrays are sized n_pos + 1 for
    // the calls that fill them; vtext_len's last slot means nothing.)
    PinnedBytes vout;
    std::vector<int64_t> vtext_off, vtext_len;
    // ... or deflated them too (CalledFrom::DeviceBlocks): position t's BGZF blocks are vout[vcomp_off[t] .. vcomp_off[t + 1]) instead;
    // vtext_len then says how long the text would have been
    std::vector<int64_t> vcomp_off;
    bool handed_back = false;            // a line was not regular: the tile went through the CPU parser and its columns are in `sites`
    void reset()
    {
        form = TileForm::Sites; called_from = CalledFrom::HostEntries; handed_back = false; n_used = 0; entries = 0; refs.clear(); n_pos = 0;
        pos.clear(); stats.clear();
    }
    bool empty() const { return form == TileForm::Sites ? n_used == 0 : n_pos == 0; }     // nothing for stage 2 to do
    bool device_parsed() const { return form != TileForm::Sites && !handed_back; }        // (once stage 2 is through with it)
    // the tile is the T positions from w.pv[ip] on: their coordinates and reference bases
    void set_positions(const Window &w, size_t ip, size_t T)
    {
        n_pos = T; pos.resize(T); refs.resize(T);
        for (size_t k = 0; k < T; ++k) { pos[k] = w.pv[ip + k]; refs[k] = w.ref_at(pos[k]); }
    }
    // position t's slice of the arrays the device returned: its entries and their samples (none of them here: slot 0, never read)
    SiteView view(size_t t) const
    {
        const int64_t a0 = called_from == CalledFrom::HostEntries ? entry_off[t] : called_from == CalledFrom::HostCalledEntries ? called_off[t] : 0;
        SiteView v;
        v.pos = pos[t];
        v.aiv = reinterpret_cast<const Entry *>(&ent[(size_t)a0]);
        v.sample = &samples[(size_t)a0];
        v.n = (size_t)(entry_off[t + 1] - entry_off[t]);
        v.stats = stats.empty() ? nullptr : &stats[t];
        return v;
    }
};
static_assert(sizeof(bvc_pileup_entry) == sizeof(Entry), "the device parser's entry is the host's");

// A runner's three stages on three threads with three tiles in flight: while libbvc works on tile i the thread that
// reads the temp batches parses tile i + 1 and the writer formats and compresses the lines of tile i - 1 (the
// reference does all of it position by position on one thread, src/BaseVarC.cpp:403-454, 548-666).  Tiles pass
// through in order, so the outputs are those of the one-thread loop byte for byte.
class TileQueue {
 public:
    void push(Tile *t) { { std::lock_guard<std::mutex> g(mu_); q_.push_back(t); } cv_.notify_one(); }
    // nullptr = the queue was closed and is empty
    Tile *pop()
    {
        std::unique_lock<std::mutex> g(mu_);
        cv_.wait(g, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return nullptr;
        Tile *t = q_.front();
        q_.pop_front();
        return t;
    }
    void close() { { std::lock_guard<std::mutex> g(mu_); closed_ = true; } cv_.notify_all(); }
 private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Tile *> q_;
    bool closed_ = false;
};

}  // namespace bvchost
#endif
