// feeds.h -- the feeds of the compute phase: each takes a thread's window through its runner, tile by tile.  Included by main.cpp
// alone: what is here calls libbvc.
#ifndef BVC_HOST_FEEDS_H
#define BVC_HOST_FEEDS_H

#include <array>
#include <cmath>
#include <iomanip>
#include <sstream>

#include "../../include/bvc_store.h"
#include "tile_runner.h"

namespace bvchost {

// At most BVC_HOST_DEVICE_SLOTS (default 8) threads per device are inside the device's part of a tile (bvc_pileup_begin_bgzf ..
// bvc_pileup_finish) at a time: past eight, the calls of more threads only get in each other's way (profiles/r05_host/README.txt: 4.9e4
// positions/s with 8 threads, 3.7e4 with 16, 2.4e4 with 32); the threads beyond them gather their next blocks and format their lines.
class DeviceSlots {
 public:
    explicit DeviceSlots(int limit) : limit_(limit) {}
    void acquire(int device)
    {
        std::unique_lock<std::mutex> g(mu_);
        if ((size_t)device >= used_.size()) used_.resize((size_t)device + 1, 0);
        cv_.wait(g, [&] { return used_[(size_t)device] < limit_; });
        used_[(size_t)device] += 1;
    }
    void release(int device)
    {
        { std::lock_guard<std::mutex> g(mu_); used_[(size_t)device] -= 1; }
        cv_.notify_all();
    }
 private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<int> used_;
    const int limit_;
};
// one of a device's slots, held for as long as this lives
struct DeviceSlot {
    DeviceSlots &slots;
    const int device;
    DeviceSlot(DeviceSlots &s, int d) : slots(s), device(d) { slots.acquire(d); }
    ~DeviceSlot() { slots.release(device); }
};

// The CPU parser, position by position (BVC_HOST_DEVICE_PARSE=0, the quality-shift hook, a mix of text and binary files): a line or
// record of every batch per position into the tile's next column.
inline void feed_cpu_parser(TileRunner &tr, const Window &w, BatchInputs &in, int qual_shift)
{
    std::string line;
    int32_t count = 0;
    for (size_t ip = w.lo; ip < w.hi; ++ip) {
        const int32_t p = w.pv[ip];
        SiteColumn &site = tr.slot();                                   // parsed in place: no copy into the tile
        site.clear();
        site.pos = p;
        int32_t j = 0;
        for (auto &fp : in) j += fp.next(j, site, line, tr.clk);
        if (qual_shift)                                                 // test hook (Knobs::qual_shift)
            for (auto &a : site.aiv)
                if (a.is_indel == 0) a.qual = (uint32_t)std::min(127, (int)a.qual + qual_shift);
        if (!site.aiv.empty()) {
            ++tr.cur->n_used;
            tr.cur->entries += site.aiv.size();
            tr.cur->refs.push_back(w.ref_at(p));
            // a tile is full at --tile positions or at 1M observations (16 MB of per-sample records held for the
            // CVG/VCF lines; three tiles are in flight per thread): at 1e5 samples that is a hundred positions, still far
            // more than the device needs, and short enough for the three stages to overlap within a thread's window
            if ((int64_t)tr.cur->n_used >= w.tile || tr.cur->entries >= ((size_t)1 << 20)) tr.flush();
            if (!(++count % 1000)) std::cerr << "basetype completed " << count << " sites -- thread" << tr.ithread << std::endl;
        }
    }
}

// Tiles staged on the host for the device parser: text inflated on the CPU (BVC_HOST_DEVICE_INFLATE=0), or binary records when every
// batch file is binary.  A tile: --tile positions at most, and about BVC_HOST_TILE_MB of text or records going by the tile before it
// (the first: 64 positions at most); every batch's share of it one after the other.
inline void feed_staged_tiles(TileRunner &tr, const Window &w, BatchInputs &in, TileForm form)
{
    const double target = 1048576.0 * tr.knobs.tile_mb_staged;
    double bytes_per_pos = 0;
    const size_t nb = in.size();
    for (size_t ip = w.lo; ip < w.hi;) {
        size_t T = (size_t)std::min<int64_t>(w.tile, (int64_t)(w.hi - ip));
        if (bytes_per_pos > 0) T = std::min(T, (size_t)std::max(1.0, target / bytes_per_pos));
        else T = std::min<size_t>(T, 64);
        Tile &tl = *tr.cur;
        tl.form = form;
        tl.text.clear();
        tl.line_start.resize(nb * (T + 1));
        const double t0 = StageClock::now();
        for (size_t b = 0; b < nb; ++b) {
            uint32_t *starts = &tl.line_start[b * (T + 1)];
            if (form == TileForm::Records) stage_records(in[b].rd, T, tl.text, starts);
            else stage_lines(in[b].rd, T, tl.text, starts);
        }
        tr.clk.read += StageClock::now() - t0;
        tl.set_positions(w, ip, T);
        bytes_per_pos = (double)tl.text.size() / (double)T;
        tr.flush();
        ip += T;
    }
}

// Tiles of the batches that phase 1 left on the device (--tmp-format mem): nothing is read, staged or uploaded.  A tile: --tile positions
// at most and BVC_HOST_TILE_MB of records (bvc_store_tile: host arithmetic on the store's cumulative sizes), gathered there from every
// kept batch by bvc_pileup_begin_store.  Like the BGZF feed this thread does stage 2's work itself, inside one of its device's slots,
// and finishes the tile by the knobs every device-parsed tile goes by; stage 3 runs beside it.  base: the store's position 0 is w.pv[base]
// (0 for a store of the whole region; a position window's first position, BVC_HOST_STORE_WINDOWS).
inline void feed_store_tiles(TileRunner &tr, const Window &w, const bvc_store *store, size_t base, DeviceSlots &slots, int device)
{
    const int64_t max_bytes = (int64_t)1048576 * tr.knobs.tile_mb_staged;
    for (size_t ip = w.lo; ip < w.hi;) {
        int32_t T = 0;
        int64_t bytes = 0, n_ent = 0, n_ind = 0, ind_bytes = 0;
        if (bvc_store_tile(store, (int32_t)(ip - base), (int32_t)std::min<int64_t>(w.tile, (int64_t)(w.hi - ip)), max_bytes, &T, &bytes) != BVC_OK)
            throw std::runtime_error("ERROR: the store of the batches does not hold the window's positions");
        Tile &tl = *tr.cur;
        tl.form = TileForm::Stored;
        tl.set_positions(w, ip, (size_t)T);
        {
            const double t1 = StageClock::now();
            DeviceSlot slot(slots, device);
            const int rc = bvc_pileup_begin_store(tr.ctx, store, (int32_t)(ip - base), T, &n_ent, &n_ind, &ind_bytes);
            if (rc == BVC_ERR_DATA) throw std::runtime_error(std::string("ERROR: malformed temp batch record (") + bvc_last_error(tr.ctx) + ")");
            bvc_check(tr.ctx, rc);
            tr.finish_tile(tl, n_ent, n_ind, ind_bytes, true);
            tr.clk_dev.gpu += StageClock::now() - t1;
        }
        ip += (size_t)T;
        // straight to stage 3 (this thread did stage 2's work itself)
        tr.rethrow_if_failed();
        tr.out_q.push(tr.cur);
        tr.cur = tr.free_q.pop();
    }
}

// The BGZF feed's arithmetic, without I/O: the blocks every batch gets next, going by what the calls report back of the lines they found.
struct BlockBudget {
    const double blocks_per_batch;      // the blocks of a batch that a tile of BVC_HOST_TILE_MB holds
    const int64_t tile;                 // --tile: the positions a tile holds at most
    std::vector<double> lines_per_block;                                // running estimate per batch
    std::vector<int64_t> blocks_sent, lines_seen;
    std::vector<int32_t> left_lines;                                    // whole lines of a batch the last tile left on the device
    int64_t target = 1;                 // positions the next tile should hold
    BlockBudget(size_t nb, int tile_mb, int64_t tile_)
        : blocks_per_batch(std::max(1.0, tile_mb * 1048576.0 / (65280.0 * (double)std::max<size_t>(1, nb)))), tile(tile_),
          lines_per_block(nb, 0.0), blocks_sent(nb, 0), lines_seen(nb, 0), left_lines(nb, 0) {}
    // batch b's new blocks: enough for `target` lines going by its lines per block so far; a batch found without a whole line gets one
    // block more than that
    int64_t want(size_t b) const
    {
        if (left_lines[b] >= target) return 0;
        const double lpb = lines_per_block[b] > 0 ? lines_per_block[b] : 1.0;
        return std::max<int64_t>(1, (int64_t)std::ceil((double)(target - left_lines[b]) / lpb));
    }
    // after a begin that made a tile of T positions (lines: the whole lines it found of every batch): the lines every batch has left
    // for the next tile and its lines per block so far; and the tile after this one: the positions that ~BVC_HOST_TILE_MB of blocks
    // hold, going by the batch with the fewest lines per block
    void note_lines(const int32_t *lines, int32_t T)
    {
        double lpb_min = 1e30;
        for (size_t b = 0; b < left_lines.size(); ++b) {
            lines_seen[b] += lines[b] - left_lines[b];
            if (blocks_sent[b] > 0) lines_per_block[b] = (double)lines_seen[b] / (double)blocks_sent[b];
            left_lines[b] = lines[b] - T;
            if (lines_per_block[b] > 0) lpb_min = std::min(lpb_min, lines_per_block[b]);
        }
        if (T > 0 && lpb_min < 1e30) target = std::max<int64_t>(1, std::min<int64_t>(tile, (int64_t)(blocks_per_batch * lpb_min)));
    }
};

// The blocks of one bvc_pileup_begin_bgzf call, gathered and not yet sent.
struct Staged {
    PinnedBytes comp;
    std::vector<bvc_bgzf_block> blocks;
    std::vector<int32_t> send;                                   // per batch: how many of them are its
    bool any_new = false, ready = false;
    double seconds = 0;                                          // what gathering them took
};

// Raw BGZF blocks, inflated and parsed on the device (text batches, the default).  The files go to the device as they are: this thread
// takes the raw blocks out of the mapped files, hands every batch's next blocks to bvc_pileup_begin_bgzf -- as many as its lines are
// short of the tile's target, counted from what the calls report back -- and the tile is the positions every batch has whole.  The
// thread does stage 2's work itself; stage 3 (CVG / VCF lines) runs beside it.
class BgzfFeed {
 public:
    // skip: per batch, the bytes of its names line (the BatchInputs that read them are closed by now: the files are mapped here)
    BgzfFeed(TileRunner &tr, const Window &w, const std::vector<std::string> &paths, const std::vector<int32_t> &skip, DeviceSlots &slots,
             int device)
        : tr_(tr), w_(w), skip_(skip), slots_(slots), device_(device), nb_(paths.size()), check_crc_(!tr.knobs.no_crc), feed_(paths),
          budget_(nb_, tr.knobs.tile_mb_bgzf, w.tile), lines_(nb_, 0), ended_(nb_, 0)
    {
        stg_[0].send.assign(nb_, 0); stg_[1].send.assign(nb_, 0);
    }

    void run()
    {
        // BVC_HOST_PROFILE=2: what every tile cost this thread (positions, compressed bytes, gathering its blocks, waiting for a device
        // slot, bvc_pileup_begin_bgzf, bvc_pileup_finish)
        const bool tile_log = tr_.knobs.profile_tiles;
        const bool overlap_gather = tr_.knobs.gather_ahead;
        std::vector<std::array<double, 6>> tile_times;
        int cur = 0;                                                    // of the two sets of blocks: the one this tile's call takes
        for (size_t ip = w_.lo; ip < w_.hi;) {
            Staged &S = stg_[cur];
            if (!S.ready) gather(S);
            const double t_wait = StageClock::now();
            DeviceSlot slot(slots_, device_);                                   // (held to the end of the loop's body)
            const double t1 = StageClock::now();
            Tile &tl = *tr_.cur;
            const int32_t max_pos = (int32_t)std::min<int64_t>((int64_t)(w_.hi - ip), std::max<int64_t>(2 * budget_.target, 64));
            int32_t T = 0;
            int64_t n_ent = 0, n_ind = 0, ind_bytes = 0;
            const int rc = bvc_pileup_begin_bgzf(tr_.ctx, S.comp.empty() ? nullptr : S.comp.data(), (int64_t)S.comp.size(), S.blocks.data(), S.send.data(),
                                                 first_ ? skip_.data() : nullptr, tr_.sample0.data(), tr_.n_in_batch.data(), (int32_t)nb_, max_pos,
                                                 first_ ? 1 : 0, &T, lines_.data(), &n_ent, &n_ind, &ind_bytes);
            first_ = false;
            S.ready = false;
            const double t_begun = StageClock::now();
            if (rc < 0) throw std::runtime_error(std::string("libbvc: ") + bvc_last_error(tr_.ctx) + " (BVC_HOST_DEVICE_INFLATE=0 inflates on the CPU)");
            budget_.note_lines(lines_.data(), T);
            if (T == 0) {
                // some batch has no whole line yet: it gets more blocks next time round (left_lines < target); nothing new and nothing
                // whole means its file has ended before the window has
                if (!S.any_new) throw std::runtime_error(kTruncatedBatch);
                continue;
            }
            tl.form = TileForm::Text;
            tl.set_positions(w_, ip, (size_t)T);
            if (rc == BVC_PILEUP_IRREGULAR) {
                int64_t need = 0;
                bvc_check(tr_.ctx, bvc_pileup_text(tr_.ctx, nullptr, 0, &need, nullptr));
                tl.text.resize((size_t)need + 1);
                tl.line_start.resize(nb_ * ((size_t)T + 1));
                bvc_check(tr_.ctx, bvc_pileup_text(tr_.ctx, tl.text.data(), need, &need, tl.line_start.data()));
                tr_.cpu_parse_tile(tl);
            } else if (overlap_gather && ip + (size_t)T < w_.hi) {
                // the blocks of the next tile are gathered (out of the mapped files into the other page-locked buffer) beside the call
                // that parses this one, runs its LRT and brings its records back: what the next call needs is known since the begin
                std::future<void> fin = std::async(std::launch::async, [&] { tr_.finish_tile(tl, n_ent, n_ind, ind_bytes, true); });
                gather(stg_[1 - cur]);                                  // (should it throw, fin's destructor waits for the call)
                fin.get();
                cur = 1 - cur;
            } else {
                tr_.finish_tile(tl, n_ent, n_ind, ind_bytes, true);
            }
            tr_.clk_dev.gpu += StageClock::now() - t1;
            if (tile_log) tile_times.push_back({(double)T, (double)S.comp.size(), S.seconds, t1 - t_wait, t_begun - t1, StageClock::now() - t_begun});
            ip += (size_t)T;
            // straight to stage 3 (this thread did stage 2's work itself)
            tr_.rethrow_if_failed();
            tr_.out_q.push(tr_.cur);
            tr_.cur = tr_.free_q.pop();
        }
        if (tile_log) {
            std::ostringstream os;
            os << "[profile] thread " << tr_.ithread << " tiles (positions, comp MB, gather ms, slot wait ms, begin ms, finish ms):";
            for (auto const &t : tile_times)
                os << " (" << t[0] << ", " << std::fixed << std::setprecision(1) << t[1] / 1048576.0 << ", " << t[2] * 1e3 << ", " << t[3] * 1e3 << ", "
                   << t[4] * 1e3 << ", " << t[5] * 1e3 << ")";
            std::cerr << os.str() << std::endl;
        }
    }

 private:
    // every batch's new blocks: what its budget says (the first call: the names line and one block of positions)
    void gather(Staged &S)
    {
        const double t0 = StageClock::now();
        S.comp.clear(); S.blocks.clear();
        S.any_new = false;
        for (size_t b = 0; b < nb_; ++b) {
            const int64_t want = first_ ? 1 + skip_[b] / 60000 : budget_.want(b);
            int32_t took = 0;
            RawBlock rb;
            while (took < want && !ended_[b]) {
                if (!feed_.pop(b, rb)) { ended_[b] = 1; break; }
                bvc_bgzf_block blk;
                blk.comp_off = (int64_t)S.comp.size(); blk.out_off = 0; blk.comp_len = (int32_t)rb.len; blk.isize = (int32_t)rb.isize;
                blk.crc32 = rb.crc32; blk.check_crc = check_crc_ ? 1u : 0u;
                S.comp.append(rb.payload, rb.len);
                S.blocks.push_back(blk);
                ++took;
            }
            S.send[b] = took;
            budget_.blocks_sent[b] += took;
            S.any_new = S.any_new || took > 0;
        }
        S.ready = true;
        S.seconds = StageClock::now() - t0;
        tr_.clk.read += S.seconds;
    }

    TileRunner &tr_;
    const Window &w_;
    const std::vector<int32_t> &skip_;
    DeviceSlots &slots_;
    const int device_;
    const size_t nb_;
    const bool check_crc_;
    MappedBlocks feed_;
    BlockBudget budget_;
    std::vector<int32_t> lines_;        // per batch: the whole lines the last begin found
    std::vector<char> ended_;
    Staged stg_[2];                     // two sets: the blocks of the tile after this one are gathered while bvc_pileup_finish works on this one
    bool first_ = true;
};

}  // namespace bvchost
#endif
