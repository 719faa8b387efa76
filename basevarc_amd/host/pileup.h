// pileup.h -- host-side data structures and text formats either side of the basetype hot path.
//
// Counterparts in the reference (paths under /root/reference):
//   AlleleInfo                      src/BamProcess.h:30-39
//   temp-batch pileup text writer   bt_r, src/BaseVarC.cpp:509-527
//   temp-batch pileup text parser   bt_s, src/BaseVarC.cpp:403-441
//   CVG line                        bt_f, src/BaseVarC.cpp:548-610, 617-663
//   VCF line                        WriteVcf, src/BaseType.cpp:141-234
//   headers                         src/BaseVarC.cpp:65-88, 364-382
#ifndef BVC_HOST_PILEUP_H
#define BVC_HOST_PILEUP_H

#include <cstdint>
#include <map>
#include <algorithm>
#include <string>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "../../include/bvc.h"
#include "../../include/bvc_site_acc_quals.h"

namespace bvchost {

struct AlleleInfo {                 // src/BamProcess.h:30-39
    uint8_t base = 4;               // 0 A, 1 C, 2 G, 3 T, 4 N, 5 indel marker
    uint8_t mapq = 0;
    uint8_t qual = 0;
    uint8_t rpr = 0;
    uint8_t strand = 0;             // 0 '-', 1 '+'
    uint8_t is_indel = 0;
    std::string indel;
};

// What the position loop keeps of one entry: eight bytes.  (The indel text of an entry, which only the CVG line's
// "Indels" column reads, is kept once per indel entry in SiteColumn::indels -- an AlleleInfo per entry would be 40 bytes
// of which 32 are an empty string for all but a few entries per thousand, and the loops over a position's entries
// are memory-bound at 1e5 samples.)
struct Entry {
    uint8_t base, mapq, qual, rpr, strand, is_indel;
    uint16_t pad;
};

// One position: the entries of the samples that have data, in sample order (aiv), and which sample each
// entry belongs to (the inverse of the reference's `idx` map, src/BaseVarC.cpp:428-429).  The tallies of the CVG line
// (src/BaseVarC.cpp:560-590: depth per base over the non-indel entries, forward / reverse counts per base value over
// ALL entries) are taken as the entries are appended, while each is in registers: cvg_line does not walk them again.
// std::allocator whose value-less construct() default-initialises: resize() of a vector of trivial elements then leaves the new
// elements unwritten instead of zero-filling them.  The parsers size a position's arrays for the most entries its line could hold
// and write the real ones in place; at N = 1e5 samples the zero fill alone was 1.2 MB of stores per position.
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { typedef NoInitAlloc<U> other; };
    NoInitAlloc() = default;
    template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
    template <class U> void construct(U *p) { ::new (static_cast<void *>(p)) U; }
    template <class U, class... A> void construct(U *p, A &&... a) { ::new (static_cast<void *>(p)) U(std::forward<A>(a)...); }
};

struct SiteColumn {
    int32_t pos = 0;
    std::vector<Entry, NoInitAlloc<Entry>> aiv;
    std::vector<int32_t, NoInitAlloc<int32_t>> sample;
    std::vector<std::string> indels;   // indel text of the entries with is_indel = 1, in entry order
    int32_t cnt[4] = {0, 0, 0, 0};
    int32_t fwd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void clear()
    {
        aiv.clear(); sample.clear(); indels.clear();
        for (int i = 0; i < 4; ++i) cnt[i] = 0;
        for (int i = 0; i < 8; ++i) { fwd[i] = 0; rev[i] = 0; }
    }
    void add(const AlleleInfo &a, int32_t j)
    {
        aiv.push_back(Entry{a.base, a.mapq, a.qual, a.rpr, a.strand, a.is_indel, 0});
        sample.push_back(j);
        if (a.is_indel) indels.push_back(a.indel);
        else if (a.base < 4) cnt[a.base] += 1;
        if (a.base < 8u) (a.strand == 1 ? fwd : rev)[a.base] += 1;
    }
};

// What the emitters read of a position, wherever it lives: a SiteColumn the CPU parser filled, or a position's slice of the arrays
// the device parser returned (bvc_pileup_finish).
struct SiteView {
    int32_t pos = 0;
    const Entry *aiv = nullptr;
    const int32_t *sample = nullptr;
    size_t n = 0;                       // entries
    const int32_t *cnt = nullptr, *fwd = nullptr, *rev = nullptr;   // [4], [8], [8]
    const std::string *indels = nullptr;    // indel text of the entries with is_indel = 1, in entry order
    size_t n_indels = 0;
    // the position's rank sums and strand counts where the device computed them (bvc_pileup_finish_called_stats): vcf_line then takes
    // them from the record and walks the entries for the sample columns alone.  nullptr: it tallies them itself
    const bvc_site_stats *stats = nullptr;
};
inline SiteView view_of(const SiteColumn &c)
{
    SiteView v;
    v.pos = c.pos; v.aiv = c.aiv.data(); v.sample = c.sample.data(); v.n = c.aiv.size();
    v.cnt = c.cnt; v.fwd = c.fwd; v.rev = c.rev; v.indels = c.indels.data(); v.n_indels = c.indels.size();
    return v;
}

// Population groups: name-sorted (std::map order in the reference, src/BaseVarC.cpp:98, 358-362).
struct Groups {
    std::vector<std::string> names;
    std::vector<uint8_t> of_sample;     // group index per sample, 255 = in no group
    // Column order of the dense tiles handed to libbvc: samples ordered by group (ungrouped last), so that every
    // group is a contiguous run of columns and the library's column-range histogram kernel takes the call.
    std::vector<int32_t> column_of;     // sample -> column
    std::vector<uint8_t> of_column;     // group index per column (non-decreasing, 255 last)
    void order_columns()
    {
        const size_t n = of_sample.size();
        std::vector<int32_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return of_sample[(size_t)x] < of_sample[(size_t)y]; });
        column_of.assign(n, 0);
        of_column.assign(n, 255);
        for (size_t c = 0; c < n; ++c) { column_of[(size_t)order[c]] = (int32_t)c; of_column[c] = of_sample[(size_t)order[c]]; }
    }
    bool empty() const { return names.empty(); }
};

// ---- a tile of positions in the form libbvc takes -------------------------------------------------------
// ONE byte per observation (base << 6 | qual: half the bytes over the host link) while every base quality of the tile is below 63,
// else two (bases, quals).  Indel entries are no observations.  The vectors live as long as their tile: refilled, not reallocated.
struct PackedTile {
    std::vector<int64_t> offsets;
    std::vector<uint8_t> packed;
    std::vector<int8_t> bases, quals;
};
// Ragged form, exactly the vectors bt_f builds (src/BaseVarC.cpp:550-559): site i's observations are [offsets[i], offsets[i + 1]) of
// `packed` (returns true; a base that is not A/C/G/T is 0xFF) or of `bases` and `quals` (false; base and quality as they are).
inline bool pack_ragged(const SiteColumn *sites, size_t n_sites, bool two_byte_only, PackedTile &o)
{
    o.offsets.assign(1, 0);
    o.packed.clear();
    bool fits = !two_byte_only;
    for (size_t i = 0; i < n_sites && fits; ++i) {
        for (auto const &a : sites[i].aiv)
            if (a.is_indel == 0) {
                if (a.qual > 62u) { fits = false; break; }
                o.packed.push_back(a.base > 3u ? (uint8_t)0xFF : (uint8_t)((a.base << 6) | a.qual));
            }
        o.offsets.push_back((int64_t)o.packed.size());
    }
    if (fits) return true;
    o.offsets.assign(1, 0);
    o.bases.clear(); o.quals.clear();
    for (size_t i = 0; i < n_sites; ++i) {
        for (auto const &a : sites[i].aiv)
            if (a.is_indel == 0) { o.bases.push_back((int8_t)a.base); o.quals.push_back((int8_t)a.qual); }
        o.offsets.push_back((int64_t)o.bases.size());
    }
    return false;
}
// Dense [site][column] form of `stride` bytes a site; column_of: sample -> column (Groups::order_columns).  `packed` with 0xFF for
// "no observation", which a base that is not A/C/G/T is too (returns true), or `bases` / `quals` with -1 / 0 for it and base and
// quality as they are elsewhere (false).
inline bool pack_dense(const SiteColumn *sites, size_t n_sites, int64_t stride, const int32_t *column_of, bool two_byte_only, PackedTile &o)
{
    bool fits = !two_byte_only;
    if (fits) o.packed.assign(n_sites * (size_t)stride, (uint8_t)0xFF);
    for (size_t s = 0; s < n_sites && fits; ++s)
        for (size_t k = 0; k < sites[s].aiv.size(); ++k) {
            const Entry &a = sites[s].aiv[k];
            if (a.is_indel != 0 || a.base > 3u) continue;             // not A/C/G/T: no observation, as in the two-byte tile
            if (a.qual > 62u) { fits = false; break; }
            o.packed[s * (size_t)stride + (size_t)column_of[sites[s].sample[k]]] = (uint8_t)((a.base << 6) | a.qual);
        }
    if (fits) return true;
    o.bases.assign(n_sites * (size_t)stride, (int8_t)-1);
    o.quals.assign(n_sites * (size_t)stride, (int8_t)0);
    for (size_t s = 0; s < n_sites; ++s)
        for (size_t k = 0; k < sites[s].aiv.size(); ++k) {
            const Entry &a = sites[s].aiv[k];
            if (a.is_indel != 0) continue;
            const size_t at = s * (size_t)stride + (size_t)column_of[sites[s].sample[k]];
            o.bases[at] = (int8_t)a.base;
            o.quals[at] = (int8_t)a.qual;
        }
    return false;
}

// ---- temp-batch pileup text (f1) -----------------------------------------------------------------------
// One line per position; per sample one space-terminated token: "." | "base,mapq,qual,rpr,strand" | indel.
void format_pileup_token(const AlleleInfo *a, std::string &out);           // a == nullptr -> ". "
// Parses the tokens of one batch's line; sample indices start at j0.  Returns the number of tokens seen
// (= samples in that batch).  N bases are dropped, indel tokens kept (src/BaseVarC.cpp:427-436).
int parse_pileup_line(const char *line, size_t len, int32_t j0, SiteColumn &site);
// The parser carries one AlleleInfo across calls within a thread, as bt_s does; call this at thread start.
void reset_parser_carry();
// base, mapq, qual, rpr, strand of that AlleleInfo: tiles parsed on the device and tiles parsed here hand it back and forth
void get_parser_carry(uint8_t out[5]);
void set_parser_carry(const uint8_t in[5]);

// ---- temp-batch binary form (additive: `--tmp-format bin`; the text form above stays the default) ----------------
// Same content as the text form, without the tokenising: a BGZF stream of
//   magic "BVCBAT1\n" | u32 samples in this batch | u32 length + the text form's first line (tab-terminated names)
// and then, per position of the thread's window, one record
//   u32 payload bytes | entries...      entry = u32 sample-in-batch | u8 base mapq qual rpr flags | [u16 n + indel text]
// (flags: bit 0 strand, bit 1 indel).  Only samples WITH data take space: at low coverage the text form spends two
// bytes (". ") on every absent sample and the parser a branch, this form nothing.  Little-endian.
extern const char kBinBatchMagic[8];
void bin_batch_header(uint32_t n_samples_in_batch, const std::string &names_line, std::string &out);
// Appends sample `j`'s entry to a position record under construction (payload only).
void bin_batch_entry(const AlleleInfo &a, uint32_t j, std::string &payload);
// Decodes one position record's payload; sample indices are offset by j0.  Reproduces the text parser's observable
// quirks: N bases dropped, and the one long-lived AlleleInfo whose fields an indel entry inherits
// (src/BaseVarC.cpp:392, 407-440) -- so both forms give identical SiteColumns.  Returns false on a malformed record.
bool parse_pileup_bin(const unsigned char *payload, size_t len, int32_t j0, SiteColumn &site);

// ---- emission (f2) -------------------------------------------------------------------------------------
extern const char *const kCvgHeader;
extern const char *const kVcfHeader;
std::string cvg_header(const Groups &g);
std::string vcf_header(const Groups &g, const std::string &reference, const std::vector<std::string> &sample_names);

// CVG line without the trailing newline handling of groups: pass grp (n_groups records) or nullptr.
std::string cvg_line(const std::string &chr, int8_t ref_base, const SiteView &site, const bvc_group_result *grp, int n_groups);
inline std::string cvg_line(const std::string &chr, int32_t pos, int8_t ref_base, const SiteColumn &site,
                            const bvc_group_result *grp, int n_groups)
{
    SiteView v = view_of(site);
    v.pos = pos;
    return cvg_line(chr, ref_base, v, grp, n_groups);
}
// VCF line for a called site.  info carries the "<group>_AF" entries; the rest is filled here.
std::string vcf_line(const bvc_site_result &bt, const std::string &chr, int8_t ref_base, const SiteView &site,
                     std::map<std::string, std::string> &info, int32_t n_samples);
inline std::string vcf_line(const bvc_site_result &bt, const std::string &chr, int32_t pos, int8_t ref_base,
                            const SiteColumn &site, std::map<std::string, std::string> &info, int32_t n_samples)
{
    SiteView v = view_of(site);
    v.pos = pos;
    return vcf_line(bt, chr, ref_base, v, info, n_samples);
}
// The sample columns of that line alone: one GT:AB:SO:BP field per sample, tab separated (what libbvc's bvc_vcf_samples_csr formats
// on the device, byte for byte).
std::string vcf_samples(const bvc_site_result &bt, int8_t ref_base, const SiteView &site, int32_t n_samples);
// The VCF line around sample columns that exist already (samples_len bytes, no tab behind the last field) and the statistics the
// device computed: reads no entries.
std::string vcf_line(const bvc_site_result &bt, const std::string &chr, int32_t pos, int8_t ref_base, const bvc_site_stats &stats,
                     std::map<std::string, std::string> &info, const char *samples_text, size_t samples_len);
// "<group>_AF" values from the group records (src/BaseVarC.cpp:646-658).
void group_af_info(const bvc_site_result &bt, const bvc_group_result *grp, const Groups &g,
                   std::map<std::string, std::string> &info);

std::string fmt_fixed(double v, int prec);          // fmt's {:.Nf}

// ---- orchestration (f3): who works on which positions, on which device, and how the pieces come together again ----------
// Per-thread window of positions (src/BaseVarC.cpp:399-403, 497, 523): thread i takes [lo, hi) of the region's position list.
// The reference's arithmetic (window = psize % T + psize / T) can run a non-last thread past the end when psize % T is
// large; the range is clamped here.  The windows of threads 0..T-1 are disjoint, ascending and cover [0, psize).
void thread_window(size_t psize, int thread, int ithread, size_t &lo, size_t &hi);
// Position windows of --tmp-format mem (BVC_HOST_STORE_WINDOWS, additive): with `thread` threads and `windows` windows the region's
// position list is cut as a run with n = thread * windows threads cuts it, and window w is the ranges of threads w * thread ..
// w * thread + thread - 1 of n taken together: [a[w], b[w]).  Contiguous, ascending, disjoint, covering [0, psize); empty windows come
// last only.  Compute thread i of window w then works as thread w * thread + i of n, so the outputs are those of a -t n run.
void store_windows(size_t psize, int thread, int windows, size_t *a, size_t *b);
// The ranges [wbeg[w], wend[w]) the windows' blocks are gathered for (0-based, as BamFile::fetch takes them): they tile the region's
// [beg0, end0).  Window 0 begins at beg0, the last window that has positions ends at end0, and the cut between a window and the next one
// that has positions is the coordinate just behind the earlier window's last position (pv holds 1-based positions, so that coordinate is
// pv[b[w] - 1]): a read that starts there or later covers nothing of the earlier window.  wbeg[w] says where the index is asked for the
// window's first block and nothing else: the reads of the gathered blocks are filtered by the REGION's beg0 (main.cpp, MemBatches::
// keep_from), so the window's list is the whole-region fetch's list from some read at or in front of the first one that covers a
// position of the window -- the rule never looks in front of that read, and behind it the two lists are the same read for read.  A
// window without positions gets an empty range (nothing is gathered for it).
void store_window_ranges(const int32_t *pv, int windows, const size_t *a, const size_t *b, int32_t beg0, int32_t end0, int32_t *wbeg,
                         int32_t *wend);
// The positions whose per-sample entries a run that piled phase 1 into class counts (bvc_bam_counts.h) must read after all, from the
// counts pass's tallies and `called` flags alone.  Per thread window of `thread` threads, position t is in the set when
//   kRevisitCalled   it is called (VCF sample columns, rank sums);
//   kRevisitIndel    it has indel entries (the CVG line's indel column, and the strand counts those entries inherit);
//   kRevisitCarry    it is the nearest earlier position OF THE SAME WINDOW that holds a base token (class 4 counts) in front of a position
//                    with indel entries: an indel entry shows the fields of the last base token parsed before it (pileup.cpp's g_carry),
//                    positions in between hold none and cannot change it, and a window that starts without one starts from zeros in
//                    every run (reset_parser_carry).
// flags [psize]: the bits above; 0 = the position's CVG line is made from its tally.
enum : uint8_t { kRevisitCalled = 1, kRevisitIndel = 2, kRevisitCarry = 4 };
inline void counts_revisit(const bvc_bam_site_tally *tally, const uint8_t *called, size_t psize, int thread, uint8_t *flags)
{
    for (int i = 0; i < thread; ++i) {
        size_t lo, hi;
        thread_window(psize, thread, i, lo, hi);
        size_t last_base = psize;                    // the window's latest position so far that holds a base token; psize: none
        for (size_t t = lo; t < hi; ++t) {
            const bvc_bam_site_tally &y = tally[t];
            flags[t] = (uint8_t)((called[t] ? kRevisitCalled : 0) | (y.n_indel > 0 ? kRevisitIndel : 0));
            if (y.n_indel > 0 && last_base != psize) flags[last_base] |= kRevisitCarry;
            uint64_t bases = y.n_other;
            for (int k = 0; k < 8; ++k) bases += y.strand_base[k];
            if (bases > 0) last_base = t;
        }
    }
}

// --tmp-format counts with --group (BVC_HOST_COUNTS_GROUPS): the counts pass labels a sample for the groups' depths (bvc_bam_group_depth.h)
// before the cohort's sample names are all known, which is what Groups' indices go by (read_groups: only groups that HAVE a sample count,
// name-sorted).  So the pass labels by the group file alone: the file's distinct group names, sorted, are `names`, and a sample's label is
// the index of its group among them, 255 when the file does not list it (or the index does not fit a label; more than BVC_MAX_GROUPS names
// are refused before anything is labelled).  The groups that have a sample among `samples` are a subsequence of `names` in the same order:
// column_file_index[c] is the index in `names` of the c-th of them -- column c of the CVG line reads depth row column_file_index[c].
// ids[i], groups[i]: the file's lines in order; a sample listed twice keeps its first line (read_groups' insert).
inline void counts_group_map(const std::vector<std::string> &ids, const std::vector<std::string> &groups, const std::vector<std::string> &samples,
                             std::vector<std::string> &names, std::vector<uint8_t> &label, std::vector<int32_t> &column_file_index)
{
    names = groups;
    std::sort(names.begin(), names.end());
    names.erase(std::unique(names.begin(), names.end()), names.end());
    std::map<std::string, size_t> group_of_id;
    for (size_t i = 0; i < ids.size() && i < groups.size(); ++i)
        group_of_id.insert({ids[i], (size_t)(std::lower_bound(names.begin(), names.end(), groups[i]) - names.begin())});
    label.assign(samples.size(), 255);
    std::vector<char> present(names.size(), 0);
    for (size_t s = 0; s < samples.size(); ++s) {
        auto it = group_of_id.find(samples[s]);
        if (it == group_of_id.end()) continue;
        present[it->second] = 1;
        if (it->second < 255) label[s] = (uint8_t)it->second;
    }
    column_file_index.clear();
    for (size_t g = 0; g < names.size(); ++g)
        if (present[g]) column_file_index.push_back((int32_t)g);
}

// Device of a phase-2 thread (additive: the reference has one CPU path): thread i works on device i mod G, G = the devices present,
// or --gpus when that is given and smaller.  Sites shard by position window, no device ever needs another's data.
int device_of_thread(int ithread, int devices_present, int gpus_option);
// Merge of the per-thread sub-files <out>.<i><suffix>, i = 0..T-1, into `dst` in thread order -- which is position order, since
// the windows ascend with the thread index (src/BaseVarC.cpp:268-296) -- removing each after it is appended.
class BgzfWriter;
bool merge_subfiles(const std::string &out_prefix, const std::string &suffix, int thread, BgzfWriter &dst);

}  // namespace bvchost
#endif
