// knobs.h -- the compute phase's knobs in the environment: every name, default and meaning once (none changes an output).  Read once,
// in run_basetype before any thread starts, and passed on by const reference.
#ifndef BVC_HOST_KNOBS_H
#define BVC_HOST_KNOBS_H

#include <sched.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "pileup.h"

namespace bvchost {

// CPUs this process may use: the cgroup's quota when it has one (cpu.max: "<quota> <period>"), else the CPUs of its affinity mask.
inline double process_cpus()
{
    double c = (double)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) c = (double)CPU_COUNT(&set);
    std::ifstream f("/sys/fs/cgroup/cpu.max");
    std::string q; double period = 0;
    if (f >> q >> period && q != "max" && period > 0) c = std::min(c, std::max(1.0, atof(q.c_str()) / period));
    return c;
}

// BVC_HOST_STORE_WINDOWS as text: an integer K >= 1 in plain digits, or "auto" (0).  nullptr (unset) is 1.  -1: none of these.
inline int parse_store_windows(const char *v)
{
    if (!v) return 1;
    const std::string s(v);
    if (s == "auto") return 0;
    if (s.empty() || s.size() > 9) return -1;
    for (char c : s) if (c < '0' || c > '9') return -1;
    const int k = atoi(s.c_str());
    return k >= 1 ? k : -1;
}
// K windows of `thread` threads are the ranges of a run with thread * K threads: that many sub-files, 65536 at the most
const int kStoreWindowsMaxThreads = 65536;
inline bool store_windows_refused(int windows, int thread)
{
    return windows < 1 || thread < 1 || (int64_t)windows * (int64_t)thread > (int64_t)kStoreWindowsMaxThreads;
}
// "auto" sizes the windows from ONE batch's bytes per position scaled to the cohort: the other batches' samples may be covered more
// deeply than batch 0's, and where they are, by how much is not known before they are piled up.  Half as much again is allowed for.
const double kStoreWindowsSafety = 1.5;
// "auto": the smallest K (at most max_k) whose largest window, estimated and times kStoreWindowsSafety, fits `budget` bytes; max_k where
// none does.  rec_start [psize + 1]: batch 0's record offsets over the whole region; scale: the cohort's samples over batch 0's;
// n_batches rows of (positions + 1) 32-bit offsets are a window's fixed cost.
inline int auto_store_windows(const uint32_t *rec_start, size_t psize, int thread, int max_k, double scale, int n_batches, double budget)
{
    auto estimate = [&](size_t a, size_t b) {
        return kStoreWindowsSafety * (scale * (double)(rec_start[b] - rec_start[a]) + 4.0 * (double)n_batches * (double)(b - a + 1));
    };
    // (the largest window is at least the average one: no K below whole / budget can fit)
    int k = (int)std::min<double>((double)max_k, std::max(1.0, estimate(0, psize) / std::max(1.0, budget)));
    std::vector<size_t> a, b;
    for (size_t t = 0; t < psize; ++t)
        if (estimate(t, t + 1) > budget) return max_k;                   // (a position that fits no budget: no K does)
    for (; k < max_k; ++k) {
        a.assign((size_t)k, 0); b.assign((size_t)k, 0);
        store_windows(psize, thread, k, a.data(), b.data());
        double largest = 0;
        for (int w = 0; w < k; ++w) largest = std::max(largest, a[(size_t)w] == b[(size_t)w] ? 0.0 : estimate(a[(size_t)w], b[(size_t)w]));
        if (largest <= budget) break;
    }
    return k;
}

// BVC_HOST_COUNTS_QUALS as text: the quality columns --tmp-format counts keeps for each base, a multiple of 4 in 4..128 in plain digits.
// nullptr (unset) is 128.  -1: none of these.
inline int parse_counts_quals(const char *v)
{
    if (!v) return 128;
    const std::string s(v);
    if (s.empty() || s.size() > 3) return -1;
    for (char c : s) if (c < '0' || c > '9') return -1;
    const int q = atoi(s.c_str());
    return q >= 4 && q <= 128 && q % 4 == 0 ? q : -1;
}

// BVC_HOST_COUNTS_LOAD as text: FILE[:FILE...], the counts files (counts_file.h) a --tmp-format counts run adds into its accumulator before
// pass 1.  nullptr (unset): no file, true.  false: an empty value or an empty name between, in front of or behind the colons.
inline bool parse_counts_load(const char *v, std::vector<std::string> &files)
{
    files.clear();
    if (!v) return true;
    const std::string s(v);
    for (size_t a = 0;;) {
        const size_t e = s.find(':', a);
        const std::string f = s.substr(a, e == std::string::npos ? std::string::npos : e - a);
        if (f.empty()) { files.clear(); return false; }
        files.push_back(f);
        if (e == std::string::npos) return true;
        a = e + 1;
    }
}
// BVC_HOST_COUNTS_SAVE as text: the one counts file the run writes after pass 1 (a colon is part of the name).  0: unset; 1: a name;
// -1: an empty value
inline int parse_counts_save(const char *v) { return !v ? 0 : *v ? 1 : -1; }

struct Knobs {
    static bool set(const char *name) { return getenv(name) != nullptr; }
    static int num(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
    static double real(const char *name, double dflt) { const char *v = getenv(name); return v ? atof(v) : dflt; }
    explicit Knobs(int threads) : cpus_per_loop(process_cpus() / (double)std::max(1, threads)) {}
    // A position loop runs helper threads beside its own (the tile formatter, the deflaters of its two outputs, the call that finishes
    // a tile while the next one's blocks are gathered); how many it starts goes by the CPUs per loop -- past the quota they only get the
    // whole process throttled (round 5, 16 CPUs: three VCF deflaters per loop +50 % with one loop, +18 % with four, -15 % with eight).
    const double cpus_per_loop;
    const bool profile = set("BVC_HOST_PROFILE");                            // set: the stage clocks of every thread and of main
    const bool profile_tiles = num("BVC_HOST_PROFILE", 0) >= 2;              // 2: and what every tile of the BGZF feed cost its thread
    const bool device_parse = num("BVC_HOST_DEVICE_PARSE", 1) != 0;          // 0: the CPU parser, not the device's (A/B runs)
    const bool device_inflate = num("BVC_HOST_DEVICE_INFLATE", 1) != 0;      // 0: the text batches are inflated on the CPU
    // 0: a device-parsed tile's entries come back for every position, not for the called ones only (WriteVcf is their one reader,
    // src/BaseVarC.cpp:664; as up to round 5's first form of this feed)
    const bool called_only = num("BVC_HOST_CALLED_ONLY", 1) != 0;
    // 1: the rank sums and strand counts of a called position's VCF line are computed on the device, where the tile's entries lie
    // (bvc_pileup_finish_called_stats), not from its entries on this CPU (three sorts per called position); needs called_only.  On since the
    // eight-thread comparison of profiles/site_stats/README.txt item 3; 0: the CPU's own tallies (A/B runs)
    const bool device_stats = num("BVC_HOST_DEVICE_STATS", 1) != 0;
    // 1: the sample columns of a called position's VCF line -- one GT:AB:SO:BP field per sample -- are formatted on the device too
    // (bvc_pileup_finish_called_text + bvc_pileup_sample_text) and no entry of a device-parsed tile comes to this CPU at all; implies the
    // device's statistics for those tiles -- BVC_HOST_DEVICE_STATS=0 therefore turns this off as well; needs called_only.  On since the
    // eight-thread comparison of profiles/vcf_samples/README.txt; 0: vcf_line's sample loop on the CPU (A/B runs)
    const bool device_samples = num("BVC_HOST_DEVICE_SAMPLES", 1) != 0 && device_stats;
    // 1: those sample columns are also deflated on the device (bvc_pileup_sample_bgzf): their text never comes to this CPU, and a called
    // position's line is written as the text in front of the columns, the columns' finished BGZF blocks (BgzfWriter::write_blocks) and the
    // newline.  The .vcf.gz inflates to the same bytes; it is larger than zlib's level 6 makes it (profiles/vcf_deflate/README.txt).  Needs
    // device_samples; acts on device-parsed tiles only.  Off by default
    const bool device_deflate = num("BVC_HOST_DEVICE_DEFLATE", 0) != 0 && device_samples;
    // 1: those blocks take a Huffman code of their own where that is smaller (tuning key "bgzf_codes" of the contexts, include/bvc.h):
    // a smaller .vcf.gz that inflates to the same bytes.  Acts only with device_deflate.  Off by default
    const bool device_deflate_codes = num("BVC_HOST_DEVICE_DEFLATE_CODES", 0) != 0 && device_deflate;
    // 1: those blocks are parsed as fields ended by tabs and colons -- what the sample columns are -- instead of searched position by
    // position (tuning key "bgzf_parse" of the contexts, include/bvc.h, docs/BGZF_FIELDS.md): other bytes that inflate to the same text.
    // Acts only with device_deflate; independent of the knob above.  Off by default (profiles/vcf_deflate_fields/README.txt)
    const bool device_deflate_fields = num("BVC_HOST_DEVICE_DEFLATE_FIELDS", 0) != 0 && device_deflate;
    // 1: phase 1 (bt_r) on the device -- the batch's BAM blocks are gathered, inflated and piled up there (bvc_bam_pileup_bgzf) and the
    // temp batches written from the records that come back; acts with --tmp-format bin|raw, ignored with text.  The batch files inflate
    // to the same bytes.  Off by default (profiles/bam_pileup/README.txt)
    const bool device_pileup = num("BVC_HOST_DEVICE_PILEUP", 0) != 0;
    // 1: the same with --tmp-format text (bvc_bam_pileup_text_bgzf): the batch's lines come back and are written behind the names line; a
    // knob of its own because the one above is documented and tested as ignored with text; ignored with bin|raw.  A batch whose lines
    // cannot fit 0xFFFFFF00 bytes takes the CPU path, said once.  The batch files inflate to the same bytes.  Off by default
    // (profiles/bam_pileup_text/README.txt)
    const bool device_pileup_text = num("BVC_HOST_DEVICE_PILEUP_TEXT", 0) != 0;
    // 1: the batch is also deflated on the device (bvc_bam_pileup_bgzf_deflate / bvc_bam_pileup_text_bgzf_deflate, include/bvc_bam_deflate.h):
    // only finished BGZF blocks come back, cut at the threads' windows, and each batch file is its names line (or binary header) through the
    // writer, then its window's blocks (BgzfWriter::write_blocks).  Acts with device_pileup on --tmp-format bin, or with device_pileup_text
    // on text; ignored with raw (stored blocks are that form's point) and mem (no files).  The batch files inflate to the same bytes; they are
    // larger than zlib's level 6 makes them.  Off by default (profiles/bam_pileup_deflate/README.txt)
    const bool device_pileup_deflate = num("BVC_HOST_DEVICE_PILEUP_DEFLATE", 0) != 0 && (device_pileup || device_pileup_text);
    // 1: those blocks take a Huffman code of their own where that is smaller (tuning key "bgzf_codes" of the load contexts).  Acts only
    // with device_pileup_deflate.  Off by default
    const bool device_pileup_deflate_codes = num("BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES", 0) != 0 && device_pileup_deflate;
    // 1, text only: those blocks are parsed as tokens ended by a space or a newline -- what a text batch's lines are -- instead of searched
    // position by position (tuning keys "bgzf_parse" = 1 and "bgzf_cuts" = 1 of the load contexts, docs/BGZF_FIELDS.md).  Acts only with
    // device_pileup_deflate and device_pileup_text; independent of the knob above.  Off by default
    const bool device_pileup_deflate_tokens = num("BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS", 0) != 0 && device_pileup_deflate && device_pileup_text;
    // 1: `BaseVarC popmatrix` makes the matrix's rows on the device -- per batch of -b samples (default 100) the region's BAM blocks are
    // gathered, inflated and resolved there (bvc_bam_popmatrix_bgzf); taken only when the position file's positions do not descend, else
    // the CPU path runs and says so.  The matrix inflates to the same bytes.  Off by default (profiles/popmatrix/README.txt)
    const bool device_popmatrix = num("BVC_HOST_DEVICE_POPMATRIX", 0) != 0;
    // --tmp-format mem: GB (a fraction will do) of device memory the batches kept there may take together (bvc_store_create's byte_budget);
    // a batch past it ends the run with a line that names --tmp-format bin.  0: no cap but the device's
    const double store_gb = std::max(0.0, real("BVC_HOST_STORE_GB", 0));
    // --tmp-format mem only (the other forms ignore it): the region is cut into K windows of positions, and per window a store is filled,
    // its positions are called and the store is dropped, so that BVC_HOST_STORE_GB is the budget of ONE window's store and a cohort of any
    // size fits.  The windows are the ranges of a run with -t T*K taken T at a time (store_windows, pileup.h), compute thread i of window w
    // works as thread w*T+i of T*K, and the outputs inflate to the bytes of --tmp-format bin -t T*K.  Unset or 1: one window, the whole
    // region.  "auto" (0 here): the smallest K whose largest window fits the budget, going by batch 0's bytes per position scaled to the
    // cohort and kStoreWindowsSafety; the K chosen is printed on a [profile] line, and an estimate that was too small ends the run with
    // the overflow line.  0, a negative number, anything that is no number and K*T above 65536 end the run before anything is written
    // (run_basetype).  Default 1 (profiles/store_windows/README.txt)
    const int store_windows = parse_store_windows(getenv("BVC_HOST_STORE_WINDOWS"));
    // 1, with K > 1 only: window w+1 is loaded while window w is computed, in lock-step (both are joined before the next pair starts); two
    // stores are alive at a time, each with half of BVC_HOST_STORE_GB.  The outputs are those of 0.  Default 0
    const bool store_overlap = num("BVC_HOST_STORE_OVERLAP", 0) != 0;
    // 1: --tmp-format counts takes --group -- the counts pass keeps the groups' depths per base beside ONE slot of class counts
    // (bvc_site_acc_create_depth, include/bvc_bam_group_depth.h: 16 bytes a group and position more) for the CVG lines' group columns, and
    // the "<group>_AF" values come from the second pile-up's store as with mem; more than 32 distinct group names in the file end the run.
    // The outputs inflate to the bytes of --tmp-format bin --group.  0: counts refuses --group.  Without --group it changes nothing.  Default 0
    // (run_basetype asks counts_groups_on() where its refusals stand, before this object is made: the refusal opens nothing)
    static bool counts_groups_on() { return num("BVC_HOST_COUNTS_GROUPS", 0) != 0; }
    const bool counts_groups = counts_groups_on();
    // --tmp-format counts only (every other format ignores it): the quality columns the counts pass keeps for each base, a multiple of 4 in
    // 4..128 (bvc_site_acc_create_quals, include/bvc_site_acc_quals.h).  A position then takes 16 x Q + 48 bytes (and 16 a group) where it
    // takes 2 KB + 48 at 128, so a region 2048 / (16 x Q) times as long fits the device; a batch that holds a counted base quality of Q or
    // more ends the run with a line that names the BAM and BVC_HOST_COUNTS_QUALS=128.  The outputs are those of 128.  Any other value ends
    // the run before anything is opened (run_basetype asks parse_counts_quals where its refusals stand; -1 here).  Default 128: the
    // accumulators of bvc_site_acc_create / _create_depth, as before the knob
    const int counts_quals = parse_counts_quals(getenv("BVC_HOST_COUNTS_QUALS"));
    // --tmp-format counts only (every other format ignores them; unset, nothing changes): counts files (counts_file.h,
    // docs/COUNTS_FILES.md).  BVC_HOST_COUNTS_LOAD=FILE[:FILE...]: before pass 1 every file's pieces are added into the accumulator
    // (bvc_site_acc_add_packed) and every BAM a file records as counted is skipped in pass 1.  BVC_HOST_COUNTS_SAVE=FILE: after pass 1 the
    // accumulator is packed in pieces of rows (bvc_site_acc_pack) and written to FILE with the list of every BAM counted, loaded ones
    // included; the run then ends with status 0 and writes no .vcf.gz or .cvg.gz -- the counts analogue of --load.  An empty value or an
    // empty name in the list ends the run before anything is opened (run_basetype asks the parse rules where its refusals stand)
    const std::string counts_save = getenv("BVC_HOST_COUNTS_SAVE") ? getenv("BVC_HOST_COUNTS_SAVE") : "";
    const std::vector<std::string> counts_load = [] { std::vector<std::string> f; parse_counts_load(getenv("BVC_HOST_COUNTS_LOAD"), f); return f; }();
    const bool two_byte_tiles =set("BVC_HOST_TWO_BYTE_TILES");              // set: never one byte per observation in the CPU parser's tiles
    const bool no_crc = set("BVC_HOST_NO_CRC");                              // set: the device does not check the CRC32 of the blocks it inflates
    // tests only: added to every base quality as it is read, so that data whose qualities stop at 41 can exercise the tiles that do not
    // fit one byte per observation (quality >= 63)
    const int qual_shift = num("BVC_HOST_QUAL_SHIFT", 0);
    // threads that inflate the blocks of the temp batches ahead of a position loop that reads them on the CPU (the loop takes a line of
    // every batch per position; inflating was 70 % of it with the text form); 0 = none
    const int inflate_threads = num("BVC_HOST_INFLATE_THREADS", 2);
    // MB a tile should hold: of text or records in the tiles staged on the host, of compressed blocks in the BGZF feed
    const int tile_mb_staged = std::max(1, num("BVC_HOST_TILE_MB", 32)), tile_mb_bgzf = std::max(1, num("BVC_HOST_TILE_MB", 128));
    const int device_slots = std::max(1, num("BVC_HOST_DEVICE_SLOTS", 8));   // threads per device inside its part of a tile at a time
    // the BGZF feed gathers the next tile's blocks beside the call that finishes this one; threads that deflate a loop's VCF text
    const bool gather_ahead = num("BVC_HOST_GATHER_AHEAD", cpus_per_loop >= 3 ? 1 : 0) != 0;
    const int vcf_deflaters = std::max(1, num("BVC_HOST_VCF_DEFLATERS", cpus_per_loop >= 4 ? 3 : (cpus_per_loop >= 3 ? 2 : 1)));
};

}  // namespace bvchost
#endif
