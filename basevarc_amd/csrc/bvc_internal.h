// bvc_internal.h -- launcher prototypes shared by the translation units of libbvc (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/bvc.h"
#include "counts_layout.h"

struct bvc_bam_site_tally;              // include/bvc_bam_counts.h

namespace bvc {

// Launch policy and one-time kernel setup of ONE context (bvc_ctx owns it; nothing here is process-wide, so
// contexts on the same or different devices are independent, include/bvc.h "Threading").
struct LaunchState {
    int n_cu = 256;
    int em_waves_per_cu = 0;   // 0 = default policy (em_kernel.hip); 1..32 resident EM wavefronts per CU
    int em_wpb = 4;            // waves per EM workgroup: 4, or 1 (A/B runs)
    int hist_split = 0;        // 0 = by tile shape; 1..64 workgroups sharing a site in the dense histogram pass
    int host_chunk_kib = 1 << 19;  // BVC_PTR_HOST calls: KiB per array and staging chunk
    int em_streams = 0;        // overlap mode: side streams stage 2 alternates between: 0 = by call shape, 1..3
    int group_pipe = 1;        // any-order group histogram: issue the next chunk's loads before counting the current one
    int group_log2c = -1;      // any-order group histograms: -1 = as many LDS copies per histogram as fit 64 KiB; 0..5 = at most
                               // 2^n copies (A/B runs: fewer copies = smaller workgroups' LDS = more resident wavefronts)
    int group_big_lds = 1;     // any-order group histograms, 4 groups and more: 1 = one 1024-thread workgroup per CU with 256 slots x
                               // 16 / 8 / 4 copies per histogram (up to 9 / 18 / 36 histograms in 144 KiB of LDS; two-byte rows packed in
                               // registers), 0 = 512-thread workgroups of <= 64 KiB
    int group_h16 = 0;         // any-order group histograms on packed rows / packed-in-registers rows: 1 = 32 conflict-free copies of
                               // 16-bit counter pairs (hist_kernel.hip "H16"), 0 = 16 copies of 32-bit counters
    int em_engine = 0;         // stage 2: 0 = item engine (em_items.hip; em_kernel.hip takes the sites it leaves),
                               // 1 = one wavefront per site for every site (em_kernel.hip): A/B runs.  The two agree to
                               // rounding (1e-15 on AF), not bit for bit: a call's records never depend on the call's
                               // size or neighbours with either, but they depend on this choice
    int em_tiny_regions = 0;       // 1: regions whose sites all have <= 8 quality values per allele take the one-lane-per-allele
                               // kernel (binned qualities: 0.23 -> 0.17 ms per 4000 sites).  Off by default: that kernel adds in a
                               // different order, so a site's last bits would depend on whether its five region neighbours are binned too
    int csr_scatter_max = 64;      // bvc_counts_add_csr*: a site with at most this many observations in the call takes one atomic per
                                   // observation (hist_csr_scatter_kernel, counts_kernel.hip) instead of a histogram in LDS; 0 = never
    int em_prune = 1;              // item engine: 1 = a level does not run the subset without the deepest candidate when a bound on its
                                   // log-likelihood shows that it cannot be the level's first minimum (em_items.hip, site_decide); 0 = it always runs
    int stats_log2c = 2;           // site_stats_kernel: 2^n LDS copies of its 1536 counters (0..4; 2 = 30 KiB with the folded counters: four
                                   // 512-thread workgroups a CU, as many as its 32 wavefronts hold; measured, profiles/site_stats/README.txt)
    int bgzf_codes = 0;            // device deflate: 0 = fixed code or stored (bd_fixed_block), 1 = the smallest of stored, fixed and a code of
                                   // the block's own (bd_dynamic_block).  Not a launch policy: it changes the bytes
    int bgzf_parse = 0;            // device deflate: 0 = the general parse (a search at every position, bd_matches), 1 = the field parse for
                                   // tab-separated text (bd_field_matches, bgzf_fields_device.h).  Independent of bgzf_codes; it changes the bytes
    int bgzf_cuts = 0;             // the field parse (bgzf_parse = 1; nothing otherwise): what ends a field -- 0 = a tab or a colon, 1 = a space or a
                                   // newline (the text temp batches' lines).  It changes the bytes
    int dbg_levels = 0;            // BVC_DBG_LEVELS (timing only, records wrong): cut region_kernel short after a phase; 0 = run all
    mutable uint32_t em_epoch = 0; // stage-2 launches of this context so far (em_items.hip: the narrow launch tells the wide one)
    struct RaisedLds { const void *kernel; size_t bytes; };
    mutable std::vector<RaisedLds> lds_raised;     // kernels whose dynamic-LDS attribute has been raised on this context's device, and to what
};

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

// Slices of a device buffer, each starting on a 256-byte boundary: take<T>(count, pad) hands out count elements + pad bytes.
// A list of take() calls written once as a function of a Layout & both sizes a buffer (base 0: `at` ends as the byte count)
// and hands out its pointers, so the two cannot disagree (bvc_ctx.h carve(); the stage-2 scratch of em_kernel.hip and
// em_items.hip).
struct Layout {
    uintptr_t base = 0;
    size_t at = 0;
    template <class T> T *take(size_t count, size_t pad = 0)
    {
        T *p = reinterpret_cast<T *>(base + at);
        at += round256(count * sizeof(T) + pad);
        return p;
    }
};

// Kernels with more than 48 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised before their first
// launch: done once per kernel and context (hist_kernel.hip).
hipError_t raise_lds(const LaunchState &st, const void *kernel, size_t bytes);

// Base-quality -> likelihood table, built on the HOST with the same libm exp() the CPU path uses
// (src/BaseType.cpp:13,15) and uploaded once per context:
//   a[q] = 1 - eps   likelihood of the observed base given the matching allele
//   e[q] = eps / 3   likelihood given any other allele
struct QualLut {
    double a[128];
    double e[128];
    double e_empty;            // e[128]: the "empty class place" of the item engine (em_items.hip), 1/4
    double log_e[128];         // log(e[q]) (libm, on the host): what a class of an allele outside the fitted subset adds to the
                               // log-likelihood per observation (em_items.hip, site_classes)
    double log_a[128];         // log(a[q]): what a class of THE allele of a one-allele model adds per observation (its marginal is a)
};

// Stage 1: dense pileup rows -> per-site class counts.  counts must be zeroed by the caller when split > 1.
hipError_t launch_hist_dense(LaunchState &st, hipStream_t stream, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                             const int8_t *bases, const int8_t *quals, const uint8_t *group_of_sample,
                             int n_groups, uint32_t *counts, int split, int64_t *group_scratch = nullptr,
                             uint8_t *hist_of_sample = nullptr);
constexpr int kGroupScratchWords = BVC_MAX_GROUPS + 4;
// The label buffer of a group call (hist_of_sample): the labels clamped to 0..n_groups, then one flag per site ("redo with
// the general kernel", hist_dense_groups_slots_kernel).
inline size_t group_redo_offset(int64_t n_samples) { return ((size_t)n_samples + 255) & ~(size_t)255; }
inline size_t group_labels_bytes(int64_t n_samples, int64_t n_sites) { return group_redo_offset(n_samples) + (size_t)n_sites + 256; }
// Group mode needs group_scratch (kGroupScratchWords int64 of device memory) and hist_of_sample (group_labels_bytes(),
// 256-byte aligned): calls whose samples are ordered by group take the column-range kernel (decided on the device),
// the others index their histograms with the clamped labels written to hist_of_sample.
// Number of sample-range splits per site launch_hist_dense should use for this shape (1 = none).
int choose_hist_split(const LaunchState &st, int64_t n_sites, int64_t n_samples);

// Stage 1 on packed rows (one byte per sample: base << 6 | qual, qual <= 62; 0xFF = no observation).
hipError_t launch_hist_packed(LaunchState &st, hipStream_t stream, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                              const uint8_t *packed, uint32_t *counts, int split);
// Group mode on packed rows: counts = [site][n_groups + 1][512]; scratch and labels as for launch_hist_dense.
hipError_t launch_hist_packed_groups(LaunchState &st, hipStream_t stream, int64_t n_sites, int64_t n_samples,
                                     int64_t row_stride, const uint8_t *packed, const uint8_t *group_of_sample, int n_groups,
                                     uint32_t *counts, int64_t *group_scratch, uint8_t *hist_of_sample);
hipError_t launch_pack_dense(hipStream_t stream, int64_t n_sites, int64_t n_samples, int64_t stride_in, const int8_t *bases,
                             const int8_t *quals, int64_t stride_out, uint8_t *packed, unsigned long long *bad);

hipError_t launch_stream_read(hipStream_t stream, const void *src, int64_t bytes, uint32_t *sink);

hipError_t launch_hist_csr(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets,
                           const int8_t *bases, const int8_t *quals, uint32_t *counts);

// Stage 2: EM + LRT, one wavefront per (site, histogram).
//   hist_stride: uint32 elements between consecutive sites' histograms.
//   comb/n_comb: optional per-site candidate list (SetBase).
//   shared: the launch runs underneath a streaming histogram kernel (overlap mode) and keeps to a few wave slots.
//   scratch: em_items_scratch_bytes(n_sites) of device memory for the item engine (em_items.hip), or null: every
//            site then takes the one-wavefront-per-site kernels.
// Does a stage 2 with this min_af go through the item engine (when it is given scratch)?  em_engine = 1 is the A/B switch;
// min_af <= 0 lets zero-depth alleles through the filter and UpdateF skip subsets (src/BaseType.cpp:54), which is left to
// the one-wavefront-per-site kernels.  The scratch is allocated, and the engine launched, by this one rule.
inline bool uses_item_engine(const LaunchState &st, double min_af) { return st.em_engine != 1 && min_af > 0.0; }
hipError_t launch_lrt(const LaunchState &st, hipStream_t stream, int64_t n_sites, const uint32_t *counts,
                      int64_t hist_stride, const int8_t *ref_base, double min_af, const QualLut *lut,
                      const int8_t *comb, const uint8_t *n_comb, bvc_site_result *results, bool shared = false,
                      int shared_waves_per_cu = 0,   // 0 = default cap when shared
                      void *scratch = nullptr);

// Item engine (em_items.hip): the EM fits of the call as work items, 8 or 16 to a wavefront.  Writes the records of
// the sites it takes and flags them in *taken_out ([n_sites] bytes inside scratch) for the kernels of em_kernel.hip.
// n_groups > 0: pseudo-site p = (site, group) on the per-group histograms [site][n_groups + 1][512].
size_t em_items_scratch_bytes(int64_t n_sites);
hipError_t launch_lrt_items(const LaunchState &st, hipStream_t stream, int64_t n_sites, int n_groups,
                            const uint32_t *counts, int64_t hist_stride, const int8_t *ref_base, double min_af,
                            const QualLut *lut, const int8_t *comb, const uint8_t *n_comb, bvc_site_result *results,
                            void *scratch, const uint8_t **taken_out, bool shared = false);

hipError_t launch_lrt_groups(const LaunchState &st, hipStream_t stream, int64_t n_sites, int n_groups,
                             const uint32_t *grp_counts, const int8_t *ref_base, double min_af, const QualLut *lut,
                             const bvc_site_result *overall, bvc_group_result *grp_results, bool shared = false,
                             int shared_waves_per_cu = 0, void *scratch = nullptr);
// scratch: em_group_scratch_bytes(n_sites, n_groups) for the item engine on the (site, group) pseudo-sites, or null
size_t em_group_scratch_bytes(int64_t n_sites, int n_groups);
// EM wavefronts per CU the stage-2 launches of group calls keep in flight underneath a long histogram pass, summed
// over the stage-2 streams in use (em_kernel.hip, em_grid_cap).
constexpr int kGroupSharedWavesPerCu = 8;

// Sum the per-group histograms (+ the "no group" one) into the overall histogram of each site.
hipError_t launch_sum_groups(hipStream_t stream, int64_t n_sites, int n_hist, const uint32_t *grp_counts,
                             uint32_t *counts);

hipError_t launch_synth_dense(hipStream_t stream, uint64_t seed, int64_t site0, int64_t n_sites,
                              int64_t n_samples, int64_t row_stride, uint32_t cov_thr16,
                              int8_t *bases, int8_t *quals, int8_t *ref_base);

// ---- pileup_kernel.hip: temp-batch pileup text -> ragged columns; per-group histograms of ragged columns -----------------
// Device buffers of one tile between bvc_pileup_begin and bvc_pileup_finish (all owned by the context).
struct PileupTile {
    const uint8_t *text = nullptr;
    bool bin = false;                        // the tile is binary records (bvc_pileup_begin_bin): text = the records, line_start = where each
                                             // begins; the count and write passes launch pileup_bin_kernel
    const uint32_t *line_start = nullptr;    // [n_batches][line_stride]
    const int32_t *sample0 = nullptr, *n_in_batch = nullptr;
    int32_t n_batches = 0, n_pos = 0;        // n_pos: the tile's positions (an upper bound while n_pos_dev decides)
    int32_t line_stride = 0;                 // elements of line_start per batch
    const int32_t *n_pos_dev = nullptr;      // tiles inflated on the device: the positions, decided there
    int64_t n_lines_cap = 0;                 // lines the per-line arrays are laid out for
    uint32_t *line_words = nullptr;          // 4 arrays of n_lines_cap words: entries, observations, last base token, inherited indels
    uint32_t *status = nullptr;              // [0] irregular lines [1] indel entries [2] indel records written [3] carry out
                                             // [4] bytes of indel tokens [5] bytes of indel text gathered
    int64_t *entry_off = nullptr, *obs_off = nullptr, *totals = nullptr;    // [n_pos + 1], [n_pos + 1], [2]
    bvc_pileup_entry *entries = nullptr;
    int32_t *samples = nullptr;
    int8_t *obs_base = nullptr, *obs_qual = nullptr;
    // tiles finished with n_groups > 0: the write pass stores each observation's group (min(group_of_sample[sample], n_groups);
    // n_groups for a sample outside the label vector) in obs_label, the third column launch_hist_csr_labels reads
    const uint8_t *group_of_sample = nullptr;
    int64_t n_samples = 0;
    int32_t n_groups = 0;
    uint8_t *obs_label = nullptr;
    int32_t *tally = nullptr;                // [n_pos][32]
    bvc_pileup_indel *indels = nullptr;
    uint32_t indel_cap = 0;
};
// A batch's region of the text buffer of a tile inflated on the device: [start, start + len) = left_len bytes the tile before left
// (at left_src of the other text buffer) + the output of the batch's new blocks.
struct bvc_pileup_region { uint32_t start, len, left_src, left_len; };
hipError_t launch_region_carry(hipStream_t stream, const uint8_t *old_text, uint8_t *text, const bvc_pileup_region *regions, int32_t n_batches);
// newlines of every region -> lines[b], the tile's positions (*P.n_pos_dev = min(lines, max_pos)), line_start of those positions
hipError_t launch_region_index(hipStream_t stream, const PileupTile &P, const bvc_pileup_region *regions, const uint32_t *seg_base,
                               int64_t n_segments, uint32_t *seg_nl, int32_t *lines, int32_t max_pos);
hipError_t launch_region_ends(hipStream_t stream, const PileupTile &P, uint32_t *ends);
// the text of the indel tokens gathered into dst (records' text_off become offsets into it); *used = bytes
hipError_t launch_indel_text(hipStream_t stream, const PileupTile &P, uint8_t *dst, uint32_t dst_cap, uint32_t *used);
// the entries of the called positions, compacted: called_off [n_pos + 1] (exclusive prefix; the last word is the total)
hipError_t launch_called_scan(hipStream_t stream, const PileupTile &P, const bvc_site_result *results, int64_t *called_off);
hipError_t launch_called_gather(hipStream_t stream, const PileupTile &P, const int64_t *called_off, bvc_pileup_entry *out_entries,
                                int32_t *out_samples);
// count pass + prefix sums (fills line_words, entry_off, obs_off, totals, status[0..1])
hipError_t launch_pileup_count(hipStream_t stream, const PileupTile &P);
// write pass + the entries that inherit across lines (status[2] and tally must be zero; leaves the carry in status[3])
hipError_t launch_pileup_write(hipStream_t stream, const PileupTile &P, uint32_t carry_in);
// counts = [site][n_groups + 1][512] from ragged observations with their sample indices
hipError_t launch_hist_csr_groups(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const int8_t *bases,
                                  const int8_t *quals, const int32_t *sample_of_obs, const uint8_t *group_of_sample, int64_t n_samples,
                                  int n_groups, uint32_t *counts);
// the same counts from one label byte per observation (group_of_obs[i] >= n_groups: in no group); quals == nullptr: obs is the
// packed byte base << 6 | qual.  Any byte alignment of the three arrays
hipError_t launch_hist_csr_labels(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const uint8_t *obs,
                                  const uint8_t *quals, const uint8_t *group_of_obs, int n_groups, uint32_t *counts);

// ---- counts accumulated over chunks of a cohort's samples (counts_kernel.hip; hist_csr_add_kernel in pileup_kernel.hip) ------
// dst[i] += src[i], i < n_words (mod 2^32): the fold of a chunk's scratch histograms into the caller's counts, and bvc_counts_merge
hipError_t launch_counts_add(hipStream_t stream, int64_t n_words, uint32_t *dst, const uint32_t *src);
// Ragged stage 1 ADDED to the caller's counts -- [site][512], or with group_of_obs [site][n_groups + 1][512]; quals == nullptr: obs is the
// packed byte.  The two launches share a call's sites: the scatter kernel takes those of at most max_len observations (max_len <= 0:
// none), the histogram kernel those of more than min_len.  Any byte alignment of the arrays.
hipError_t launch_hist_csr_scatter(const LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const uint8_t *obs,
                                   const uint8_t *quals, const uint8_t *group_of_obs, int n_groups, int64_t max_len, uint32_t *counts);
hipError_t launch_hist_csr_add(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const uint8_t *obs,
                               const uint8_t *quals, const uint8_t *group_of_obs, int n_groups, int64_t min_len, uint32_t *counts);

// site_stats_kernel.hip: the rank sums and strand counts of the called sites' entries (include/bvc.h, bvc_site_stats); a site that is not
// called gets a zeroed record.  A workgroup takes one site at a time, called or not; st.stats_log2c LDS copies of the counters.
constexpr int kStatsMaxLog2c = 4;
constexpr int kSiteStatsTrip = 4096;     // entries a workgroup takes per trip of its streaming loop (the sizes the tests straddle)
hipError_t launch_site_stats(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                             const int8_t *ref_base, const bvc_site_result *results, bvc_site_stats *stats);

// vcf_samples_kernel.hip: the sample columns of the called sites' VCF lines (include/bvc.h, bvc_vcf_samples_csr).  The plan launches fill
// text_off [n_sites + 1], text_len [n_sites] and the scratch (vcf_samples_scratch_bytes of device memory: head[0] = called sites, head[1] =
// the sum of the slots, the called sites' list, every site's valid prefix); launch_vcf_samples then formats into `text` (16-byte aligned) and
// writes nothing when head[1] > text_cap.  bp_lut: the 2048 bytes of bvc_vcf_bp_lut in device memory.
constexpr int kVcfSamplesTile = 508;     // samples a workgroup formats per trip of its loop (the sizes the tests straddle)
struct VcfSamplesScratch { int64_t *head; int32_t *called_list; uint32_t *n_valid; };
size_t vcf_samples_scratch_bytes(int64_t n_sites);
VcfSamplesScratch vcf_samples_scratch(void *buf, int64_t n_sites);
hipError_t launch_vcf_samples_plan(hipStream_t stream, int64_t n_sites, const int64_t *offsets, const int32_t *samples,
                                   const bvc_site_result *results, int64_t n_samples, int64_t *text_off, int64_t *text_len,
                                   const VcfSamplesScratch &s);
hipError_t launch_vcf_samples(hipStream_t stream, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                              const int32_t *samples, const int8_t *ref_base, const bvc_site_result *results, int64_t n_samples,
                              const int64_t *text_off, const VcfSamplesScratch &s, const char *bp_lut, char *text, int64_t text_cap);

// bgzf_deflate_kernel.hip: pieces of device memory deflated into BGZF blocks (include/bvc.h, bvc_bgzf_deflate).  Piece i holds the
// blocks first_block[i] .. first_block[i + 1] of the call (first_block [n_pieces + 1] in the scratch, filled by the caller: from the
// pieces' lengths or from upper bounds of them -- a block behind a piece's real length is empty and takes no byte); comp_off
// [n_pieces + 1] and the packed blocks are written on the stream.  Nothing is packed when the blocks do not fit comp_cap.
constexpr int kBgzfDeflateGrid = 256;    // workgroups of bgzf_block_kernel: a call of more blocks sends each round its loop again
struct BlockDesc { int64_t src; uint32_t len; uint32_t pad; };               // a block of the call: where its input starts in `data`, its bytes
struct BgzfDeflateScratch { int64_t *first_block, *block_off; BlockDesc *desc; uint32_t *bsize, *match_rows; uint8_t *staging; };
// Which instantiation of bgzf_block_kernel (bgzf_block_kernel.h) a call launches -- fields: the field parse, dynamic: a code of the block's own
// as well -- and the two bytes that end a field, as the field parse takes them.  bgzf_mode makes it from the
// tuning keys "bgzf_parse", "bgzf_codes" and "bgzf_cuts".
struct BgzfMode { bool fields, dynamic; uint32_t delims; };
BgzfMode bgzf_mode(const LaunchState &ls);
size_t bgzf_deflate_scratch_bytes(int64_t n_pieces, int64_t n_blocks);
BgzfDeflateScratch bgzf_deflate_scratch(void *buf, int64_t n_pieces, int64_t n_blocks, Layout *sized = nullptr);
hipError_t launch_bgzf_deflate(hipStream_t stream, int64_t n_pieces, const uint8_t *data, const int64_t *piece_off, const int64_t *piece_len,
                               int64_t n_blocks, const BgzfDeflateScratch &s, uint8_t *comp, int64_t comp_cap, int64_t *comp_off, const BgzfMode &mode);
// bgzf_dynamic_kernel.hip: the code-length builder on counts of the caller's: lengths[set][s] from counts[set][s], device pointers
hipError_t launch_bgzf_code_lengths(hipStream_t stream, int64_t n_sets, const uint32_t *counts, int32_t n_symbols, int32_t limit, uint8_t *lengths);

// inflate_kernel.hip: raw deflate of whole BGZF blocks, one wavefront per block; status[i] != 0: block i is not valid deflate of isize bytes
hipError_t launch_inflate(hipStream_t stream, const uint8_t *comp, const bvc_bgzf_block *blocks, int64_t n_blocks, uint8_t *out, uint32_t *status);

// bam_pileup_kernel.hip: inflated BAM alignment records of a batch of samples -> the batch's position records in the binary temp-batch
// form (include/bvc_bam.h, bvc_bam_pileup).  launch_bam_index fills the read table (the kept reads of sample s from slot
// sample_off[s] / kBamMinRecord on: a record takes at least that many bytes, so the slices cannot meet) and sample_status 0..3;
// launch_bam_tile(place = false) leaves rec_len of the tile's positions (and status 4); launch_bam_scan leaves rec_start and head (the
// total, the first sample of status 2, 3, 4 or 0x7FFFFFFF); launch_bam_tile(place = true) writes the tile's records.  The scratch is the
// read table + a size matrix of one tile of positions + O(n_positions + n_samples).
constexpr int64_t kBamMinRecord = 36;    // block_size word + the 32 fixed bytes read_record insists on
struct BamRead { int64_t off; int32_t pos, end; };      // the record's block_size word in bam; 0-based start; end_pos
// positions per tile: 1024, fewer for wide batches (about 4 Mi cells), never below a wavefront's 64
inline int32_t bam_pileup_tile(int32_t n_samples)
{
    const int64_t t = (((int64_t)1 << 22) / (n_samples > 0 ? n_samples : 1)) / 64 * 64;
    return (int32_t)(t < 64 ? 64 : t > 1024 ? 1024 : t);
}
struct BamPileupScratch {
    int32_t tile = 0;
    BamRead *reads = nullptr; int32_t *runmax = nullptr; uint32_t *n_reads = nullptr; uint8_t *carry = nullptr; uint32_t *cell = nullptr;
    uint64_t *rec_len = nullptr; uint32_t *rec_start = nullptr; int64_t *head = nullptr;
};
BamPileupScratch bam_pileup_scratch(Layout &L, int64_t bam_bytes, int32_t n_samples, int32_t n_positions);
hipError_t launch_bam_index(hipStream_t stream, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                            const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                            const BamPileupScratch &s, uint32_t *sample_status);
hipError_t launch_bam_tile(hipStream_t stream, bool place, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                           const int64_t *sample_end, const int32_t *positions, int32_t t0, int32_t tile_n, int32_t rg_s, const uint8_t *refseq, int64_t refseq_len,
                           const BamPileupScratch &s, uint32_t *sample_status, uint8_t *records);
hipError_t launch_bam_scan(hipStream_t stream, int32_t n_positions, int32_t n_samples, const BamPileupScratch &s, const uint32_t *sample_status);

// bam_text_kernel.hip: the same call with the batch's lines in the text temp-batch form as its output (include/bvc_bam_text.h,
// bvc_bam_pileup_text).  launch_bam_index, launch_bam_scan and the scratch are the ones above (carry stays unused; rec_len holds a line's
// bytes less the 4 the scan adds, rec_start is line_start); launch_bam_text_tile is launch_bam_tile's twin, `text` the lines' bytes.
hipError_t launch_bam_text_tile(hipStream_t stream, bool place, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                                const int64_t *sample_end, const int32_t *positions, int32_t t0, int32_t tile_n, int32_t rg_s, const uint8_t *refseq,
                                int64_t refseq_len, const BamPileupScratch &s, uint32_t *sample_status, uint8_t *text);

// bam_popmatrix_kernel.hip: the same records and a list of (position, REF, ALT) -> one row of '0' / '1' / '.' per sample
// (include/bvc_popmatrix.h, bvc_bam_popmatrix).  launch_bam_index as above; launch_bam_popmatrix writes matrix[s * row_stride + t] for every
// sample and position (and status 4); launch_bam_scan with n_positions = 0 leaves head[1..3].  The scratch is the read table + O(n_samples):
// of a BamPileupScratch only reads, runmax, n_reads, one word of rec_start and head are set.
BamPileupScratch bam_popmatrix_scratch(Layout &L, int64_t bam_bytes, int32_t n_samples);
hipError_t launch_bam_popmatrix(hipStream_t stream, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                                const int64_t *sample_end, int32_t n_positions, const int32_t *positions, const uint8_t *ref, const uint8_t *alt,
                                int32_t rg_s, int64_t refseq_len, const BamPileupScratch &s, uint8_t *matrix, int64_t row_stride, uint32_t *sample_status);

// A call over a batch's inflated BAM records: its inputs where the kernels read them (device memory; in the host-pointer forms the caller's
// arrays until they are staged) and its sizes
struct BamCall {
    int32_t n_samples = 0, n_positions = 0, beg0 = 0, end0 = 0, min_mapq = 0, rg_s = 0;
    const uint8_t *bam = nullptr, *eof = nullptr, *ref = nullptr;   // ref: the reference's text (the pileup only)
    const uint8_t *pref = nullptr, *palt = nullptr;                 // the positions' REF and ALT characters (the matrix only)
    const int64_t *off = nullptr, *end = nullptr;
    const int32_t *rid = nullptr, *pos = nullptr;
    int64_t bam_bytes = 0, refseq_len = 0;
};

// bam_counts_kernel.hip: the same records added into class counts and tallies [position] of any CountsLayout (counts_layout.h;
// include/bvc_bam_counts.h, bvc_bam_group_depth.h, bvc_site_acc_quals.h).  launch_bam_index as above, the scratch is bam_popmatrix_scratch.
// add = false: the dry pass, which raises status 4 and on narrow rows status 5 (4 where both hold) and reads nothing of the arrays;
// add = true: the adds -- counts [slots][512] or [4][n_quals] a position (none for a quality >= n_quals), the tally, and depth
// [depth_groups][4] where the layout has groups' depths; group_of_sample is read where label_groups() > 0, a label >= that adds to the last
// slot or to no depth.  launch_bam_scan with n_positions = 0 leaves head[1..3]; launch_first_status leaves in out[0] the first sample of
// status `which` (0x7FFFFFFF: none); launch_acc_expand turns rows [n_rows][4][n_quals] into [n_rows][512] with zeros in the columns
// >= n_quals (both 16-byte aligned).
struct CountsArrays { uint32_t *counts; ::bvc_bam_site_tally *tally; uint32_t *depth; const uint8_t *group_of_sample; };
hipError_t launch_bam_counts(hipStream_t stream, bool add, const BamCall &c, const CountsLayout &layout, const BamPileupScratch &s, CountsArrays a,
                             uint32_t *sample_status);
hipError_t launch_first_status(hipStream_t stream, int32_t n_samples, const uint32_t *sample_status, uint32_t which, int64_t *out);
hipError_t launch_acc_expand(hipStream_t stream, int64_t n_rows, int32_t n_quals, const uint32_t *narrow, uint32_t *wide);

// acc_pack_kernel.hip: an accumulator's rows <-> (row_start, cell, count) entries of their logical rows (include/bvc_site_acc_pack.h).  The
// rows a launch works on are an AccRowShape (counts_layout.h, CountsLayout::row_shape).
enum : uint32_t { kAccFaultRowStart = 1, kAccFaultCell = 2, kAccFaultOrder = 3, kAccFaultQual = 4 };   // a row's fault in row_fault
// place = false: row_n [n_rows] (nothing of row_start, cell or count is touched); place = true: cell and count through row_start [n_rows + 1]
hipError_t launch_acc_pack(hipStream_t stream, bool place, int64_t n_rows, const AccRowShape &s, const uint32_t *counts, const ::bvc_bam_site_tally *tally,
                           const uint32_t *depth, uint32_t *row_n, const int64_t *row_start, uint16_t *cell, uint32_t *count);
hipError_t launch_acc_pack_scan(hipStream_t stream, int64_t n_rows, const uint32_t *row_n, int64_t *row_start);
// add = false: row_fault [n_rows] (nothing is added); add = true: the adds (row_fault unused)
hipError_t launch_acc_add_packed(hipStream_t stream, bool add, int64_t n_rows, const AccRowShape &s, const int64_t *row_start,
                                 const uint16_t *cell, const uint32_t *count, int64_t n_entries, uint32_t *counts, ::bvc_bam_site_tally *tally,
                                 uint32_t *depth, uint32_t *row_fault);
// out[0] = the first row whose fault is not 0 (0x7FFFFFFFFFFFFFFF: none), out[1] = that fault
hipError_t launch_acc_first_fault(hipStream_t stream, int64_t n_rows, const uint32_t *row_fault, int64_t *out);

// store_kernel.hip: temp batches kept on the device (include/bvc_store.h).  A kept batch as the kernels see it: the device addresses of its
// rec_start row and of its records, and the records' bytes (what every word of the row is clamped with).
constexpr int kStoreGrid = 1024;         // workgroups of store_gather_kernel at most: a tile of more items sends each round its loop again
struct StoreBatch { uint64_t rec_start, records, bytes; };
// What one bvc_pileup_begin_store call plans (the context's memory): per batch its slice's start in its records, the slice's bytes, its place
// in the tile buffer and its first work item ([n_batches + 1]: the last word is the items' number); *used: the tile buffer's bytes in use
struct StorePlan { uint32_t *lo, *len, *dst, *first_item; unsigned long long *used; };
// cum[i] += rec_start[i], i < n_words
hipError_t launch_store_cum(hipStream_t stream, const uint32_t *rec_start, int32_t n_words, unsigned long long *cum);
// positions [t0, t0 + T] of every batch -> tile (16-byte aligned, tile_cap bytes: the slices' bytes and 16 a batch) and rows [n_batches][T + 1]
hipError_t launch_store_gather(hipStream_t stream, const StoreBatch *batches, int32_t n_batches, int32_t t0, int32_t T, const StorePlan &plan,
                               uint8_t *tile, int64_t tile_cap, uint32_t *rows);

#ifdef BVC_CHECK_LDS
hipError_t debug_read_inflate(uint32_t *out8, bool reset);
hipError_t debug_read_pileup(uint32_t *out8, bool reset);
hipError_t debug_read_site_stats(uint32_t *out8, bool reset);
hipError_t debug_read_vcf_samples(uint32_t *out8, bool reset);
hipError_t debug_read_bgzf_deflate(uint32_t *out8, bool reset);
hipError_t debug_read_bgzf_dynamic(uint32_t *out8, bool reset);
hipError_t debug_read_bgzf_fields(uint32_t *out8, bool reset);
// diagnostic builds: each translation unit's violation record (bvc_device.h)
hipError_t debug_read_hist(uint32_t *out8, bool reset);
hipError_t debug_read_wave_engine(uint32_t *out8, bool reset);
hipError_t debug_read_items(uint32_t *out8, bool reset);
#endif

}  // namespace bvc
