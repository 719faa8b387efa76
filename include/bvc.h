/*
 * bvc.h -- C ABI of libbvc, the MI355X (gfx950) implementation of BaseVarC's per-site
 * basetype hot path.
 *
 * What it replaces in the reference (paths under /root/reference):
 *   - class BaseType: constructor, SetBase, LRT and the public result fields
 *       src/BaseType.h:59-74, src/BaseType.cpp:5-139, 237-255
 *   - EM / singleEM / delta_bylog and chisf
 *       src/Algorithm.cpp:3-7, 69-130
 *   - the per-site call sites in bt_f
 *       src/BaseVarC.cpp:612-615 (overall call), :617-661 (per-group calls)
 *
 * The reference has no FFI: BaseType is a C++ object built and consumed once per site on the caller's
 * stack.  Launching device work per site is not viable, so the ABI is batched: the caller hands over a
 * TILE of sites in site-major layout and receives one fixed-size record per site holding exactly the
 * fields bt_f and WriteVcf read from a BaseType (var_qual, depth_total, alt_bases, depth, af_lrt;
 * src/BaseType.cpp:145-147, 200-212, 221, 226) plus a few diagnostics used for parity pinning.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every entry point returns BVC_OK (0) or a negative code
 *     and bvc_last_error(ctx) gives the text.  "No call" (LRT() == false) is called = 0, not an error.
 *   - the caller owns all input/output buffers; the library owns only device scratch inside the context.
 *   - one context = one device + one HIP stream; contexts are independent (one per host thread, as
 *     bt_f runs on T std::threads in the reference, src/BaseVarC.cpp:263-266); the library keeps no
 *     process-wide mutable state.
 *   - there is NO CPU fallback: without a usable gfx950 device bvc_create fails.
 */
#ifndef BVC_H
#define BVC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVC_OK               0
#define BVC_ERR_ARG         -1   /* bad argument (null pointer, negative size, base_comb out of range ...) */
#define BVC_ERR_DEVICE      -2   /* HIP runtime error; text in bvc_last_error */
#define BVC_ERR_NO_DEVICE   -3   /* no gfx950 device / device index out of range */
#define BVC_ERR_ALLOC       -4   /* device or host allocation failed */
#define BVC_ERR_DATA        -5   /* bvc_pileup_begin_bgzf: a BGZF block is not valid deflate of its ISIZE bytes;
                                    bvc_pileup_begin_bin: a binary record is malformed.  The context stays usable */
#define BVC_PILEUP_IRREGULAR 1   /* bvc_pileup_begin only, not an error: a line of the tile is not of the shape the reference's
                                    writer produces; nothing was computed, parse this tile with the reference's own rules */
#define BVC_BAM_MORE         2   /* bvc_bam_pileup only (bvc_bam.h), not an error: a sample's bytes ran out before its stop record, or
                                    records_cap is below *records_needed; nothing was written, supply more and call again */

/* flags for the compute entry points */
#define BVC_PTR_HOST    0u       /* every data pointer is host memory; the call is synchronous */
#define BVC_PTR_DEVICE  1u       /* every data pointer is device memory; the call is asynchronous on the
                                    context's stream (bvc_synchronize or a stream sync completes it) */

#define BVC_NCLASS 512           /* (base, qual) classes per site: base * 128 + qual */
#define BVC_MAX_GROUPS 32

typedef struct bvc_ctx bvc_ctx;

/* One record per site: what a BaseType holds after LRT() (src/BaseType.h:70-74). 120 bytes. */
typedef struct bvc_site_result {
    double  var_qual;       /* BaseType::var_qual */
    double  chi;            /* chi_sqrt_t when LRT() left its loop (src/BaseType.cpp:101) -- diagnostic */
    double  depth_total;    /* BaseType::depth_total */
    double  af[3];          /* af_lrt[alt_base[i]], i < n_alt */
    double  lr_alt;         /* lr_alt_t at exit -- diagnostic */
    double  base_frq[4];    /* fitted frequencies of the accepted model, indexed by base -- diagnostic */
    int32_t depth[4];       /* BaseType::depth[A,C,G,T] */
    int32_t n_passes;       /* number of E+M passes run (singleEM calls) -- diagnostic; see "em_prune" */
    int8_t  alt_base[3];    /* BaseType::alt_bases, in the reference's order */
    uint8_t n_alt;
    uint8_t called;         /* return value of LRT() */
    uint8_t n_kept;         /* size of the accepted model */
    int8_t  kept[4];        /* bases of the accepted model (`bases` at exit) */
    uint8_t status;         /* 0 ok; 1 = the reference's behaviour is undefined for this input
                               (bp[0] / min_element on an empty vector, only reachable with min_af <= 0) */
    uint8_t n_fits;         /* EM() calls run -- diagnostic; see "em_prune" */
} bvc_site_result;

/* Per (site, group) record for the caller's --group loop (src/BaseVarC.cpp:617-661). 48 bytes. */
typedef struct bvc_group_result {
    double  af[3];          /* <group>_AF for overall alt i: gr_bt.af_lrt[alt] or 0 when absent (:646-652) */
    int32_t depth[4];       /* na:nc:ng:nt of the group's covered samples (:640) */
    uint8_t ran;            /* 1 when the group's BaseType was built and LRT() run (:641-644) */
    uint8_t present;        /* bit i set: overall alt i is among the group's alt_bases (af_lrt.count(b), :647);
                               a clear bit is the literal "0" of :650, not an estimated frequency of zero */
    uint8_t pad[6];
} bvc_group_result;

typedef struct bvc_profile {
    double  hist_ms;        /* summed HIP-event time of the pileup->histogram kernel since the last reset */
    double  em_ms;          /* summed HIP-event time of the EM/LRT kernel */
    int64_t hist_launches;
    int64_t em_launches;
    int64_t sites;
} bvc_profile;

/* ---- context -------------------------------------------------------------------------------------- */
const char *bvc_version(void);
/* Number of usable gfx950 devices (0 when there is none or the HIP runtime cannot start). */
int  bvc_device_count(void);
int  bvc_create(bvc_ctx **out, int device);
void bvc_destroy(bvc_ctx *ctx);

/*
 * Additive: page-locked host memory for the buffers a caller hands to the calls that take HOST pointers.  A transfer from or to a
 * buffer that lies inside such an allocation goes straight over the link; any other host buffer goes through the context's own
 * page-locked bounce buffer (one memcpy of the bytes more).  The host program assembles the compressed blocks of a tile there
 * (bvc_pileup_begin_bgzf: a fifth of a tile's bytes, and the largest transfer of the feed).  Any thread, any device; NULL when the
 * allocation fails.  bvc_host_free(NULL) is a no-op.
 */
void *bvc_host_alloc(size_t bytes);
void bvc_host_free(void *p);
const char *bvc_last_error(const bvc_ctx *ctx);
/* Run on the caller's HIP stream (hipStream_t passed as void*; NULL = the device's default stream).  A new context works on a
 * stream of its own (a blocking stream: ordered against the device's default stream, concurrent with other contexts' streams). */
int  bvc_set_stream(bvc_ctx *ctx, void *hip_stream);
int  bvc_synchronize(bvc_ctx *ctx);
/*
 * Overlap mode (off by default).  With it on, every entry point that takes device pointers (bvc_lrt_dense,
 * bvc_lrt_dense_groups, bvc_lrt_csr[_comb]) runs its second stage (EM/LRT, FP64-bound) on internal side streams,
 * so that it executes underneath the first stage (histogram, HBM-bound) of the NEXT call.  Results of a call are
 * then complete only after bvc_join (makes the context's stream wait for all side work) or bvc_synchronize; the
 * caller must keep the ref_base and results buffers of a call alive and untouched until then, and give calls
 * that may be in flight together DIFFERENT results buffers: the second stages of consecutive calls may run
 * side by side (two side streams), so which of two writers of one buffer comes last is not defined.
 */
int  bvc_set_overlap(bvc_ctx *ctx, int on);
int  bvc_join(bvc_ctx *ctx);
/* HIP-event timing of each kernel (adds two event records per launch). */
int  bvc_set_profiling(bvc_ctx *ctx, int on);
int  bvc_get_profile(bvc_ctx *ctx, bvc_profile *out, int reset);

/* ---- the hot path --------------------------------------------------------------------------------- */
/*
 * Dense tile: bases[s * row_stride + i], quals[...] for site s < n_sites, sample i < n_samples.
 * A sample is covered iff its base byte is 0..3 (A,C,G,T) and its qual byte is 0..127; anything else
 * (the caller's "no read / N / indel" cases, src/BaseVarC.cpp:427, 551-559) is skipped.
 * Equivalent per site to:  BaseType bt(bases, quals, ref_base[s], min_af); bt.LRT();
 * (src/BaseVarC.cpp:612-613).  min_af is the caller's value (src/BaseVarC.cpp:541-543).
 * ref_base[s] is 0..3 (A,C,G,T).  Any other value (the caller's -1 for a non-ACGT reference letter) means "no
 * base equals the reference": every kept base is then an ALT, as `b != ref_base` decides in src/BaseType.cpp:112,
 * and in group mode it contributes no candidate to {ref} + alt_bases (its depth is 0 in the reference, so the
 * min_af filter of src/BaseType.cpp:79 drops it).  The reference's caller never produces such a site
 * (src/BaseVarC.cpp:199-203).
 */
int bvc_lrt_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                  const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                  double min_af, bvc_site_result *results, uint32_t flags);

/*
 * Dense tile with population groups: additionally, for every group g < n_groups, the depth counts and --
 * when the overall call succeeded -- BaseType gr(bases_g, quals_g, ref, min_af);
 * gr.SetBase({ref} + alt_bases); gr.LRT()  (src/BaseVarC.cpp:617-661).
 * group_of_sample[i] >= n_groups means "in no group" (src/BaseVarC.cpp:352-356).
 * grp_results is [n_sites][n_groups].
 * Any column order gives the same records; when group_of_sample is non-decreasing (each group a contiguous run
 * of columns, ungrouped samples last) the call takes a faster histogram kernel.
 */
int bvc_lrt_dense_groups(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                         const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                         double min_af, const uint8_t *group_of_sample, int32_t n_groups,
                         bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);

/*
 * Ragged (CSR) pileup: site s owns bases[offsets[s] .. offsets[s+1]) -- exactly the vectors bt_f builds
 * (src/BaseVarC.cpp:550-559).  Every element must be a covered observation or it is skipped as above.
 */
int bvc_lrt_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets,
                const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                double min_af, bvc_site_result *results, uint32_t flags);
/*
 * The same with BaseType::SetBase (src/BaseType.h:67): base_comb[s * 4 + c], c < n_comb[s] <= 4, are the candidate
 * bases of site s in SetBase order; both NULL means the default {A,C,G,T} (src/BaseType.h:79).  This is the whole
 * of  BaseType bt(bases, quals, ref, min_af); bt.SetBase(v); bt.LRT();  in one call (src/BaseVarC.cpp:642-644).
 */
int bvc_lrt_csr_comb(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets,
                     const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                     double min_af, const int8_t *base_comb, const uint8_t *n_comb,
                     bvc_site_result *results, uint32_t flags);

/*
 * Additive: the ragged form at ONE byte per observation (the packed byte of bvc_lrt_dense_packed below:
 * base << 6 | qual, qual 0..62; a byte whose qual bits are 63 is skipped).  Site s owns packed[offsets[s] .. offsets[s+1]).
 * Same records as bvc_lrt_csr on the same observations, bit for bit.  For host callers this halves what crosses
 * the host link, which is what bounds them (src/BaseVarC.cpp:550-559 builds the two vectors this replaces; the
 * successor of bt_s writes the byte directly).  Observations with base quality >= 63 cannot be packed: such tiles
 * stay on bvc_lrt_csr.
 */
int bvc_lrt_csr_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed,
                       const int8_t *ref_base, double min_af, bvc_site_result *results, uint32_t flags);

/*
 * Additive: packed dense tiles, ONE byte per (site, sample) instead of two.  The path is bound by the bytes it reads,
 * and (base 0..3, qual 0..62) fits a byte:
 *     packed[s * row_stride + i] = base << 6 | qual        0xFF (any byte whose qual bits are 63) = no observation
 * Results are those of bvc_lrt_dense on the same observations, bit for bit (the histogram is the same).  Base
 * qualities of 63 and more cannot be packed: keep such tiles on bvc_lrt_dense.  A producer (the successor of bt_s,
 * src/BaseVarC.cpp:403-441, which builds the vectors of :550-559) writes the bytes itself; bvc_pack_dense converts a
 * two-byte tile on the device and reports in *n_unrepresentable how many covered samples did not fit (they are
 * written as "no observation": a tile with n_unrepresentable != 0 must not be used).
 */
int bvc_lrt_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                         const uint8_t *packed, const int8_t *ref_base, double min_af,
                         bvc_site_result *results, uint32_t flags);
/* Group mode on a packed tile: bvc_lrt_dense_groups with the one-byte layout (same records, bit for bit). */
int bvc_lrt_dense_groups_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                                const uint8_t *packed, const int8_t *ref_base, double min_af,
                                const uint8_t *group_of_sample, int32_t n_groups,
                                bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);
/* Device pointers only (BVC_PTR_DEVICE); synchronises the context's stream. */
int bvc_pack_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                   const int8_t *bases, const int8_t *quals, int64_t packed_stride, uint8_t *packed,
                   int64_t *n_unrepresentable, uint32_t flags);

/*
 * Additive: the caller's --group loop on RAGGED columns (src/BaseVarC.cpp:617-661 works on each site's COVERED samples: the
 * vectors of :550-559 plus, per entry, which sample it came from, :633-636).  bvc_lrt_csr with, per observation, the index of
 * its sample: sample_of_obs[i] in 0..n_samples-1 (anything else: in no group); group_of_sample[n_samples] as in
 * bvc_lrt_dense_groups.  grp_results is [n_sites][n_groups].  Same records as bvc_lrt_dense_groups on the dense tile that holds
 * the same observations, bit for bit (the per-group histograms are the same counts), without building, uploading or reading
 * n_samples bytes per site: at the coverage of the cohorts this tool is for (6-10 %) that is 10-16 x fewer bytes.
 */
int bvc_lrt_csr_groups(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                       const int32_t *sample_of_obs, const int8_t *ref_base, double min_af,
                       const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                       bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);

/*
 * Additive: bvc_lrt_csr_groups for a caller who knows each entry's GROUP when it builds the vectors (src/BaseVarC.cpp:633-636 looks
 * it up per entry): group_of_obs[i] is the group of observation i, one byte in place of the 4-byte sample index and the label
 * vector.  Any value >= n_groups: in no group, as in bvc_lrt_dense_groups (the observation still counts in the overall record);
 * no byte value is an error.  Skips what bvc_lrt_csr skips (a base outside 0..3, a quality byte outside 0..127).  Same records as
 * bvc_lrt_csr_groups on the same observations with group_of_obs[i] = group_of_sample[sample_of_obs[i]] (an index outside the label
 * vector: any byte >= n_groups), byte for byte.  3 bytes per observation instead of 6 over the host link and out of device memory,
 * and no gather.  Host or device pointers (flags); device arrays may start at any byte.  n_groups outside 1..32, a null
 * grp_results, null data or label pointers with observations present, offsets that do not start at 0 or that decrease:
 * BVC_ERR_ARG.
 */
int bvc_lrt_csr_group_labels(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                             const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                             bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);
/* The same at TWO bytes per observation: packed[i] = base << 6 | qual as in bvc_lrt_csr_packed (quality bits 63: skipped). */
int bvc_lrt_csr_group_labels_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed,
                                    const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                                    bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);

/*
 * Additive: BGZF blocks inflated on the device.  The reference reads its temp batches through htslib's bgzf_getline
 * (src/BaseVarC.cpp:406; written with bgzf_write, :509-527): one raw-deflate stream (RFC 1951) of at most 64 KiB of output per
 * block, blocks independent of each other.  blocks[i] names the deflate payload of a block inside `comp` (the bytes between the
 * 18-byte BGZF header and the 8-byte CRC32 / ISIZE trailer), its ISIZE and where its output goes in `out`; status[i] = 0 when the
 * block inflated to exactly ISIZE bytes, else a non-zero code (the block's output is then undefined; zlib refuses the same streams).
 * With check_crc the CRC32 of the output is computed on the device too and compared.  Host or device pointers (flags).
 */
typedef struct bvc_bgzf_block {
    int64_t comp_off;      /* offset of the deflate payload in comp */
    int64_t out_off;       /* offset of the block's output in out */
    int32_t comp_len;      /* bytes of deflate payload */
    int32_t isize;         /* bytes the block inflates to (<= 65536) */
    uint32_t crc32;        /* CRC32 of the inflated bytes (the block's trailer, RFC 1952) */
    uint32_t check_crc;    /* non-zero: compare (htslib does for every block it reads); a mismatch is status 10 */
} bvc_bgzf_block;
int bvc_inflate_blocks(bvc_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                       uint8_t *out, int64_t out_bytes, uint32_t *status, uint32_t flags);

/* ---- the producer of the hot path's input on the device (additive) ------------------------------------------------------ */
/*
 * The reference's position loop (bt_s, src/BaseVarC.cpp:403-441) reads one line of every temp-batch file per position and
 * tokenises it with strtok_r / atoi into the position's entries; bt_f then tallies depths and strands (:548-590), builds the
 * (base, qual) vectors (:550-559) and calls BaseType on them (:612-613; per group :617-661).  These two calls do all of that for
 * a TILE of positions from the inflated TEXT of the temp batches (format: writer :509-527): the text goes to the device as it is,
 * the parsed columns feed the LRT there, and what bt_f and WriteVcf read afterwards comes back.  (bvc_pileup_begin_bin below takes
 * the tile as binary records instead; bvc_pileup_begin_bgzf takes the text still compressed.)
 *
 *   text         the tile's text: for every temp batch the lines of the tile's positions ('\n' after each), anywhere in the buffer
 *   line_start   [n_batches][n_positions + 1] offsets into text: line t of batch b starts at line_start[b * (n_positions + 1) + t];
 *                entry n_positions of a batch = one past the '\n' of its last line (lines of a batch are consecutive)
 *   sample0      [n_batches] index of the batch's first sample (the running j of :407); n_in_batch: samples (= tokens per line)
 *
 * bvc_pileup_begin uploads and counts; it returns BVC_OK and the sizes of what bvc_pileup_finish will deliver, or
 * BVC_PILEUP_IRREGULAR when some line is not what the reference's writer produces (tokens ". ", "b,m,q,r,s " with 1-3 digits a
 * field, or an indel token starting '+', '-' or 'N'; ONE space after every token; as many tokens as the batch has samples): the
 * reference's parser gives such lines a meaning too (strtok_r, atoi), which the caller then applies itself (host/pileup.cpp).
 * bvc_pileup_finish (only after a begin that returned BVC_OK, same context) parses, runs the LRT of every position on the device
 * (bvc_lrt_csr on the non-indel entries; bvc_lrt_csr_groups when n_groups > 0) and returns
 *   entry_off  [n_positions + 1]  entries of position t = entries[entry_off[t] .. entry_off[t + 1]), in sample order
 *   tally      [n_positions][32]  [strand << 3 | base] counts of the base entries, + 16 for the indel entries (:560-590)
 *   entries / samples             the entry and the sample it belongs to (aiv and the inverse of idx, :428-429)
 *   indels     [n_indels]         which entries are indel tokens and where their text is (any order)
 *   results / grp_results         as bvc_lrt_csr / bvc_lrt_csr_groups
 * carry: base, mapq, qual, rpr, strand of the last base token parsed before the tile / after it -- the reference keeps ONE
 * AlleleInfo alive across tokens, lines and positions and an indel token only sets is_indel / indel (:392, 407-440), so an indel
 * entry shows the fields of the last base token before it.
 * Host pointers only; both calls synchronise the context's stream.
 */
typedef struct bvc_pileup_entry {       /* AlleleInfo without its string, src/BamProcess.h:30-39 */
    uint8_t  base, mapq, qual, rpr, strand, is_indel;
    uint16_t pad;
} bvc_pileup_entry;
typedef struct bvc_pileup_indel {
    int64_t entry;                      /* index into entries */
    int64_t text_off;                   /* the token's text in the caller's buffer */
    int32_t len;
    int32_t pad;
} bvc_pileup_indel;
int bvc_pileup_begin(bvc_ctx *ctx, const char *text, int64_t text_bytes, const uint32_t *line_start,
                     const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                     int64_t *n_entries, int64_t *n_indels);
int bvc_pileup_finish(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                      const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                      int64_t *entry_off, int32_t *tally, bvc_pileup_entry *entries, int32_t *samples,
                      bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results, bvc_group_result *grp_results);
/*
 * The same from the BINARY form of the temp batches (additive; the host program's `--tmp-format bin` and `raw`): per position and
 * batch one record
 *   record  = u32 payload bytes | payload                                                        (little-endian)
 *   payload = entries; entry = u32 sample-in-batch | u8 base mapq qual rpr flags | [u16 n | n bytes of indel text]
 *             flags: bit 0 strand, bit 1 "indel entry" (only then the u16 and the text follow)
 * with the meaning the text form has: base = byte & 7, strand = flags & 1, a base entry with base 4 (N) is dropped but remains the
 * "last base token", an indel entry shows the fields of the last base entry before it (carry, above).
 *   records      the tile's records: for every temp batch the records of the tile's positions, one after the other, anywhere in the buffer
 *   rec_start    [n_batches][n_positions + 1] offsets into records, the twin of line_start: record t of batch b begins -- at its
 *                length word -- at rec_start[b * (n_positions + 1) + t]; entry n_positions of a batch = one past its last record
 *   sample0, n_in_batch   as above; a sample-in-batch index must be below n_in_batch[b]
 * The call checks on the host that every rec_start[t + 1] - rec_start[t] equals 4 + the record's length word and that all of it lies
 * inside records_bytes (<= 0xFFFFFF00): BVC_ERR_ARG otherwise.  It returns BVC_OK and the sizes, or BVC_ERR_DATA when some record is
 * malformed: fewer than 9 bytes left for an entry, fewer than 11 for an indel entry, an indel text that runs past the payload's
 * end -- what the host program's CPU parser refuses too -- or a sample-in-batch index >= n_in_batch[b], which that parser does
 * not check and this call must, because the index feeds the group lookup on the device.  The kernel bounds every load by the
 * record's end whatever the bytes say; a malformed record is counted (bvc_last_error says how many), never followed; the tile is
 * not begun and the context stays usable.  There is no BVC_PILEUP_IRREGULAR here: binary records have no second meaning.
 * bvc_pileup_finish / bvc_pileup_finish_called then serve the tile as they serve text: indel_text NULL leaves the indel records'
 * text_off as offsets into `records` (at the text bytes, len = n); given, it receives the texts gathered on the device and
 * text_off become offsets into it (room for the sum of the records' len is needed; records_bytes always suffices).
 * Host pointers only; synchronises the context's stream.
 */
int bvc_pileup_begin_bin(bvc_ctx *ctx, const uint8_t *records, int64_t records_bytes, const uint32_t *rec_start,
                         const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                         int64_t *n_entries, int64_t *n_indels);
/*
 * bvc_pileup_finish with the entries of the CALLED positions only (results[t].called != 0).  Of a position that is not called the
 * reference reads the tallies and the indel strings alone (the CVG line, src/BaseVarC.cpp:560-610); the entries themselves are read
 * by WriteVcf (:664), i.e. for the few per cent of the positions that are called -- at 1e5 samples and 10 % coverage the entries are
 * 120 KB per position that a caller otherwise receives and never looks at.
 *   called_off [n_positions + 1]  entries / samples of position t = [called_off[t] .. called_off[t + 1]) (empty unless called);
 *                                 gathered on the device, in position order
 *   called_cap                    room in entries / samples, in entries (n_entries of the begin call always suffices; BVC_ERR_ARG when
 *                                 the called positions hold more)
 * entry_off, indels (records' entry = index among ALL entries, as before) and everything else as bvc_pileup_finish.
 */
int bvc_pileup_finish_called(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                             const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                             int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                             int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                             bvc_group_result *grp_results);
/*
 * Additive: what WriteVcf (src/BaseType.cpp:141-234) computes from a CALLED position's entries besides the sample columns -- the
 * inputs of MQRankSum / BaseQRankSum / ReadPosRankSum (RankSumTest, src/Algorithm.cpp:55-67) and of FS / SOR / SB_REF / SB_ALT (Stat,
 * src/BaseType.cpp:174-186) -- as integers, computed on the device from the entries.
 *
 * An entry counts iff is_indel != 1 and base <= 3.  It is a REF observation iff base == ref_base[s] (a ref_base outside 0..3 matches
 * nothing), otherwise an ALT observation iff base is one of results[s].alt_base[0 .. n_alt) (n_alt > 3 is read as 3), otherwise it is
 * ignored; forward iff strand == 1 (WriteVcf:164-186).
 *
 * rankR1 (src/Algorithm.cpp:27-53) ranks the pooled ref + alt values in DESCENDING order, a run of equal values sharing the mean of its
 * ranks, and sums the ranks of the ref observations.  All three fields are bytes (src/BamProcess.h:32-37), so with r[v] / a[v] the
 * ref / alt observations of value v and lo the pooled observations of a value larger than v, the run of v occupies the ranks
 * lo + 1 .. lo + r[v] + a[v] and
 *     rank2 = 2 * r1 = sum over v of r[v] * (2 * lo + r[v] + a[v] + 1)
 * an integer; rank2 / 2.0 is exact (below 2^53) and is the double the host's rank_r1 returns (host/stats.cpp), so z, the phred value and
 * the printed text follow from (rank2, n_ref, n_alt) unchanged: bvchost_ranksum_from_rank2 / RankSumFromR1 (host/stats.h).  The
 * reference's rankR1 itself keeps a run's rank sum in an int32_t, which overflows once a run of equal values is longer than about 65,536
 * observations; this statistic is the host program's, which does not (host/stats.cpp).
 */
typedef struct bvc_site_stats {          /* 64 bytes */
    int64_t rank2[3];                    /* 2 x rankR1 of the REF observations in the pooled ref + alt values: [0] mapq, [1] qual, [2] rpr */
    int32_t n_ref, n_alt;                /* sizes of the two samples (RankSumTest's n1, n2) */
    int32_t ref_fwd, ref_rev, alt_fwd, alt_rev;   /* Stat, src/BaseType.cpp:174-186 */
    uint8_t valid;                       /* 1 where results[s].called != 0, else the whole record is 0 */
    uint8_t pad[15];
} bvc_site_stats;
/*
 * stats[s] for site s < n_sites from its entries[offsets[s] .. offsets[s + 1]); a site with results[s].called == 0 gets a zeroed record and
 * its entries are not read.  Host or device pointers (flags); device `entries` may start at any entry; device `stats` must start on a
 * 16-byte boundary (the records are written with 16-byte stores).  With host pointers the small arrays are staged through the context's page-locked buffer; the entries, the bulk, are copied
 * from the caller's memory as it is -- a DMA the call sleeps behind when they lie in bvc_host_alloc memory, a pageable copy otherwise.  Of `results`
 * only called, n_alt and alt_base are read, and they must be COMPLETE: in overlap mode call bvc_join after the bvc_lrt_* call that
 * writes them -- this call is ordered on the context's stream behind that join, it does not join by itself.  BVC_ERR_ARG: null pointers
 * with work present, a negative n_sites, host offsets that do not start at 0 or that decrease.
 */
int bvc_site_stats_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                       const int8_t *ref_base, const bvc_site_result *results, bvc_site_stats *stats, uint32_t flags);
/*
 * bvc_pileup_finish_called with the statistics of every position of the tile: stats [n_positions], computed on the tile's entries where
 * they lie on the device and delivered with the records (no further transfer or wait).  stats == NULL: bvc_pileup_finish_called itself.
 */
int bvc_pileup_finish_called_stats(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                                   const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                                   int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                                   int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                                   bvc_group_result *grp_results, bvc_site_stats *stats);
/* The called positions' VCF sample columns formatted on the device -- bvc_vcf_samples_csr, bvc_pileup_finish_called_text,
 * bvc_pileup_sample_text -- are declared in their own section below. */
/*
 * The same from the COMPRESSED temp batches: the BGZF blocks go to the device as they are in the files (a fifth of the bytes of
 * their text), are inflated there (bvc_inflate_blocks) and the text never exists on the host.  The caller no longer knows where the
 * lines are, so the call decides the tile's positions itself: every batch's text so far = what the previous call left of it (kept
 * on the device) + its new blocks; the tile = the lines EVERY batch has whole, at most max_positions.
 *   blocks            the new blocks of all batches, batch after batch (out_off is ignored); blocks_of_batch[b] = how many are b's
 *   skip_bytes        NULL, or per batch the bytes at the start of its FIRST block that are not position lines (the sample-names
 *                     line, src/BaseVarC.cpp:495, 503); only read where the batch has nothing left over
 *   reset             non-zero: forget what earlier calls left (a new window of positions)
 *   n_positions       out: the tile's positions T (0: some batch has no whole line yet -- send more of its blocks; lines_of_batch
 *                     says which); lines_of_batch[b]: whole lines batch b had (before the T of this tile are taken away)
 *   indel_text_bytes  out: size of the buffer bvc_pileup_finish's indel_text needs (the indel tokens' text: records' text_off are
 *                     then offsets into it; with bvc_pileup_begin indel_text may be NULL and text_off stays an offset into text)
 * Returns BVC_OK, BVC_PILEUP_IRREGULAR (the tile's T positions are decided and consumed, but some line is not regular: fetch the text
 * with bvc_pileup_text and parse it with the reference's rules), BVC_ERR_DATA (a block is not valid deflate of its ISIZE bytes, or -- check_crc -- fails its CRC32)
 * or another error.
 */
int bvc_pileup_begin_bgzf(bvc_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                          const int32_t *blocks_of_batch, const int32_t *skip_bytes, const int32_t *sample0, const int32_t *n_in_batch,
                          int32_t n_batches, int32_t max_positions, int32_t reset, int32_t *n_positions, int32_t *lines_of_batch,
                          int64_t *n_entries, int64_t *n_indels, int64_t *indel_text_bytes);
/* After bvc_pileup_begin_bgzf: the tile's text (text_bytes from *text_bytes_needed: call with text = NULL first) and its line table
 * [n_batches][n_positions + 1] as bvc_pileup_begin takes it. */
int bvc_pileup_text(bvc_ctx *ctx, char *text, int64_t text_cap, int64_t *text_bytes_needed, uint32_t *line_start);

/* ---- the two stages on their own (used by the parity tests; also valid entry points) -------------- */
/* Stage 1: counts[s * 512 + base * 128 + qual] = number of covered samples of that class (exact). */
int bvc_hist_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                   const int8_t *bases, const int8_t *quals, uint32_t *counts, uint32_t flags);
/* Stage 1 on a packed tile (device pointers only): the same counts[s * 512 + base * 128 + qual]. */
int bvc_hist_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                          const uint8_t *packed, uint32_t *counts, uint32_t flags);
/* Stage 2: EM + LRT on per-site class counts.  base_comb (optional): [n_sites][4] candidate bases in
 * SetBase order with n_comb[s] entries used; NULL means the default {A,C,G,T} (src/BaseType.h:79).
 * base_comb / n_comb contract (also bvc_lrt_csr_comb): with BVC_PTR_HOST an entry outside 0..3 or n_comb[s] > 4 is
 * rejected with BVC_ERR_ARG before anything runs.  With BVC_PTR_DEVICE the library cannot look at the arrays without
 * a round trip, so the kernels apply the reference's own rule instead: a candidate that is not A, C, G or T has
 * depth 0 in BaseType (src/BaseType.cpp:79 reads depth[b]) and falls to the min_af filter, i.e. the entry is
 * ignored (the record equals the one for the list without it), and n_comb[s] > 4 is read as 4.
 * A list may repeat a base (the reference then divides the starting frequencies by a depth sum that counts it twice,
 * src/BaseType.cpp:27-37; the record is the reference's).
 * Counts: a site's observations must sum to at most 2^31 - 1 (depth[] is int32_t, as BaseType::depth is); larger sums are not
 * checked and wrap the depths. */
int bvc_lrt_hist(bvc_ctx *ctx, int64_t n_sites, const uint32_t *counts, const int8_t *ref_base,
                 double min_af, const int8_t *base_comb, const uint8_t *n_comb,
                 bvc_site_result *results, uint32_t flags);

/* ---- a cohort in SAMPLE chunks: counts that accumulate (additive) ------------------------------------------------------------ */
/*
 * A site's record depends on its samples only through its 512 class counts, and counts add over samples.  So a cohort need not arrive
 * site by site with all its samples: zero counts[n_sites][512] once, ADD every chunk of samples to it (a temp batch of 500 samples, a
 * node's share of the cohort) with the calls below, then run stage 2 on the sum -- bvc_lrt_hist, or with groups bvc_lrt_hist_groups.
 * The records are those of the one-piece call on all samples, byte for byte (the counts are the same integers).
 *
 *   counts[s * 512 + c] += the chunk's covered observations of class c = base * 128 + qual at site s        (exact)
 * in unsigned 32-bit arithmetic: a class of more than 2^32 - 1 observations wraps, which is NOT checked.  `counts` follows `flags` like
 * every other pointer.  BVC_PTR_DEVICE: asynchronous on the context's stream (in overlap mode too: these calls are ordered like
 * bvc_hist_dense).  BVC_PTR_HOST: the convenience form -- the inputs AND the counts are staged up, added to on the device and brought
 * back, in one piece and synchronously; a caller with many chunks keeps the counts on the device.
 * What counts as a covered observation is what the bvc_lrt_* call of the same layout says.  BVC_ERR_ARG: null pointers with work
 * present, negative sizes, n_groups outside 1..32, host offsets that do not start at 0 or that decrease.
 */
/* Dense chunk: the tile of bvc_hist_dense[_packed], its n_samples columns a chunk of the cohort's. */
int bvc_counts_add_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                         const int8_t *bases, const int8_t *quals, uint32_t *counts, uint32_t flags);
int bvc_counts_add_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                                const uint8_t *packed, uint32_t *counts, uint32_t flags);
/* Ragged chunk: offsets and columns as bvc_lrt_csr[_packed] take them; site s of the chunk adds into row s.  A site without an
 * observation in the chunk (offsets[s] == offsets[s + 1]) is legal and costs nothing.  Device arrays may start at any byte. */
int bvc_counts_add_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                       uint32_t *counts, uint32_t flags);
int bvc_counts_add_csr_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed,
                              uint32_t *counts, uint32_t flags);
/*
 * With groups: grp_counts[n_sites][n_groups + 1][512], the layout the group calls use between their stages.  Slot g < n_groups holds
 * the observations of group g; the LAST slot, n_groups, holds those in no group (a label >= n_groups).  The overall counts of a site
 * are the sum of its n_groups + 1 slots.
 *   bvc_counts_add_dense_groups       two-byte tile; group_of_sample[n_samples] are the labels of the CHUNK's columns
 *   bvc_counts_add_csr_group_labels   two-byte ragged columns with one label byte per observation (bvc_lrt_csr_group_labels)
 */
int bvc_counts_add_dense_groups(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                                const int8_t *bases, const int8_t *quals, const uint8_t *group_of_sample, int32_t n_groups,
                                uint32_t *grp_counts, uint32_t flags);
int bvc_counts_add_csr_group_labels(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                                    const uint8_t *group_of_obs, int32_t n_groups, uint32_t *grp_counts, uint32_t flags);
/*
 * Stage 2 of the group calls on accumulated group histograms: the site records and the [n_sites][n_groups] group records of
 * bvc_lrt_dense_groups / bvc_lrt_csr_group_labels on the same observations, byte for byte.  The overall counts are summed into the
 * context's own scratch; grp_counts is only read.  In overlap mode stage 2 runs on a side stream like that of every bvc_lrt_* call:
 * grp_counts, ref_base and the record buffers stay untouched until bvc_join.
 */
int bvc_lrt_hist_groups(bvc_ctx *ctx, int64_t n_sites, const uint32_t *grp_counts, const int8_t *ref_base, double min_af,
                        int32_t n_groups, bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags);
/* dst[i] += src[i] for i < n_words (mod 2^32): partial counts of another context, device or rank (either layout) added to this one's. */
int bvc_counts_merge(bvc_ctx *ctx, int64_t n_words, uint32_t *dst, const uint32_t *src, uint32_t flags);

/* ---- synthetic pileup generator (benchmark / test input); device pointers only ------ */
/* Fills sites site0 .. site0+n_sites-1.  cov_thr16 = 65536 gives dense coverage; smaller values leave
 * a sample uncovered (base = -1) with probability 1 - cov_thr16/65536.  Integer arithmetic only. */
int bvc_synth_dense(bvc_ctx *ctx, uint64_t seed, int64_t site0, int64_t n_sites, int64_t n_samples,
                    int64_t row_stride, uint32_t cov_thr16, int8_t *bases, int8_t *quals,
                    int8_t *ref_base);

/* ---- tuning (per context; additive, no counterpart in the reference) -------------------------------- */
/* Launch policy of THIS context; results never depend on it.  Keys:
 *   "em_waves_per_cu"  0 = default policy, 1..32 = stage-2 wavefronts per CU and launch: a call's stage 2 then runs as a
 *                      SEQUENCE of launches of at most that many wavefronts per CU (a region of eight sites belongs to a team
 *                      of two wavefronts; a workgroup holds up to two teams).  Default: unbounded when stage 2 has the chip to
 *                      itself, 4 underneath a streaming histogram pass (overlap mode, rows of 200,000 samples and more)
 *   "em_wpb"           waves per EM workgroup: 4 (default) or 1
 *   "hist_split"       0 = by tile shape, 1..64 workgroups sharing a site in the dense histogram pass
 *   "em_streams"       overlap mode: stage 2 of consecutive calls on one side stream (1), on two alternating ones (2: the
 *                      next EM launch fills the previous one's tail), or chosen by row length (0, default)
 *   "group_pipe"       any-order group histogram: 1 (default) issues the next chunk's loads before counting the
 *                      current one, 0 loads two chunks then counts both
 *   "group_copies_log2"  any-order group histograms: -1 (default) = as many LDS copies of each histogram as fit 64 KiB,
 *                      0..5 = at most 2^n copies (smaller workgroups, more of them resident; A/B runs)
 *   "group_big_lds"    any-order group histograms, 4 groups and more: 1 (default) = one 1024-thread workgroup per CU with 256
 *                      slots x 16 / 8 / 4 copies per histogram in up to 144 KiB of LDS (two-byte rows are packed in registers for
 *                      it; sites with a covered quality of 63 or more are redone by the general kernel), 0 = 512-thread
 *                      workgroups of 64 KiB
 *   "group_h16"        any-order group histograms on packed rows: 0 (default) = 16 LDS copies of 32-bit counters, 1 = 32
 *                      conflict-free copies of 16-bit counter pairs (A/B runs)
 *   "csr_scatter_max"  bvc_counts_add_csr*: a site with at most this many observations IN THE CALL is counted with one global atomic per
 *                      observation, lanes running over the observations across site boundaries; a longer one through a histogram in
 *                      LDS that one workgroup adds to the counts.  0 = never scatter, up to 1 << 30 (= always: the scatter kernel alone, sites of any length).  Default 64
 *                      (measured: DESIGN.md section 3.10).  Environment: BVC_CSR_SCATTER_MAX
 *   "stats_copies_log2"  bvc_site_stats_csr / bvc_pileup_finish_called_stats: 2^n copies (0..4, default 2) of the 1536 counters a
 *                      workgroup keeps in LDS, copy = lane mod 2^n (A/B runs).  Environment: BVC_STATS_LOG2C
 *   "host_chunk_kib"   BVC_PTR_HOST calls stage the tile through device memory in chunks of sites of at most this
 *                      many KiB per array (default 524288 = 512 MiB); the upload of chunk i+1 runs under the kernels
 *                      of chunk i
 * A new context starts from the environment variables BVC_EM_WAVES_PER_CU, BVC_EM_WPB, BVC_HIST_SPLIT, BVC_EM_STREAMS,
 * BVC_GROUP_PIPE, BVC_GROUP_LOG2C (for "group_copies_log2"), BVC_GROUP_BIG_LDS, BVC_GROUP_H16 when they are set to a value their
 * key accepts ("host_chunk_kib" has no variable).
 *
 * One key is NOT a launch policy:
 *   "em_engine"        0 (default) = the item engine of stage 2 (fits as work items, csrc/em_items.hip), 1 = one
 *                      wavefront per site for every site (csrc/em_kernel.hip, the engine of rounds 1-2, which otherwise
 *                      only takes the sites the item engine leaves).  The two evaluate the same sums in different
 *                      orders: calls, depths, pass counts and every integer field agree (except where two subsets tie
 *                      to rounding), AF / chi / var_qual agree to ~1e-15 relative, not bit for
 *                      bit.  With either engine a site's record never depends on the call's size or on its neighbours.
 *                      Environment: BVC_EM_ENGINE.
 *   "em_tiny_regions"  0 (default) / 1: with 1, regions of eight sites that all have at most 8 quality values per allele
 *                      (binned qualities) take a kernel with one lane per allele (stage 2 1.36 x faster on such data).  That
 *                      kernel adds in a different order, so a site's AF / chi could differ in the last bits with the
 *                      binning of its seven region neighbours: off by default.  Environment: BVC_EM_TINY_REGIONS.
 *   "em_prune"         1 (default) / 0.  A level of the likelihood-ratio test goes on with the FIRST MINIMUM of chi over its
 *                      subsets and reads nothing else of the others (src/BaseType.cpp:97-105).  With 1 the item engine runs the
 *                      subsets that keep the deepest allele first and does not run the one without it when an upper bound on
 *                      that subset's log-likelihood (every class marginal <= 1; the left-out allele's observations have
 *                      marginal e exactly) puts its chi above the minimum of the others: the decision, and every field of the
 *                      record the reference defines, is unchanged, the diagnostics n_fits / n_passes count what was run.  0 =
 *                      the subset is always run (n_fits / n_passes then equal the reference's counts).  Environment: BVC_EM_PRUNE.
 *   "bgzf_codes"       0 (default) / 1.  bvc_bgzf_deflate (host and device pointers) and bvc_pileup_sample_bgzf: with 0 every block is
 *                      written in the fixed Huffman code, or stored; with 1 each block takes the smallest of stored, fixed and a
 *                      Huffman code of its own (RFC 1951 BTYPE = 10; the rule is with bvc_bgzf_deflate below).  It changes the BYTES of
 *                      the blocks, never what they inflate to, their number, their framing or the waits of the calls.  With 0
 *                      nothing differs by a byte from a library without the key.  Environment: BVC_BGZF_CODES.
 *   "bgzf_parse"       0 (default) / 1.  The same calls: with 0 a block's matches come from a search at every position; with 1 from the
 *                      FIELD PARSE for tab-separated text (the rule is with bvc_bgzf_deflate below and in docs/BGZF_FIELDS.md): a field that
 *                      repeats the field in front of it is a match at the distance of one field, the others look a hash of their bytes
 *                      up, no other position has a match.  Independent of "bgzf_codes": all four combinations are valid.  It changes
 *                      the BYTES of the blocks, never what they inflate to, their number, their framing or the waits of the calls;
 *                      text without tabs or colons becomes literals, hence mostly stored blocks.  With 0 nothing differs by a byte
 *                      from a library without the key.  Environment: BVC_BGZF_PARSE.
 *   "bgzf_cuts"        0 (default) / 1.  Acts only with "bgzf_parse" = 1 (with 0 it changes nothing): the two bytes that end a field of the
 *                      field parse.  0: a tab or a colon (VCF sample columns).  1: a space or a newline -- the text temp batches' lines
 *                      (bvc_bam_text.h), where ". " is a two-byte field whose runs become matches at the distance of one field and a
 *                      "b,m,q,r,s " token is a head with a key.  Everything else of the rule is unchanged; it changes the BYTES of the
 *                      blocks, never what they inflate to.  Environment: BVC_BGZF_CUTS. */
int bvc_set_tuning(bvc_ctx *ctx, const char *key, int value);

/* ---- measurement aid ------------------------------------------------------------------------------- */
/* Streams `bytes` of device memory once with 16-byte loads per lane and nothing else; HIP-event time in ms.
 * The empirical HBM read ceiling to hold next to the spec peak when judging the histogram kernel. */
int bvc_stream_read_ms(bvc_ctx *ctx, const void *device_ptr, int64_t bytes, int repeats, double *ms_per_pass);

/* ---- the called positions' VCF sample columns formatted on the device (additive) ------------------- */
/*
 * Additive: the SAMPLE COLUMNS of a called position's VCF line (WriteVcf, src/BaseType.cpp:187-212: one GT:AB:SO:BP field per sample,
 * 400 KB per position at 1e5 samples) formatted on the device from the position's entries and the sample each belongs to.  The text is,
 * byte for byte, what the host program's vcf_line puts behind "GT:AB:SO:BP\t" (host/pileup.cpp):
 *   - the entries count up to the first k with samples[k] < (one past the previous entry's sample, 0 at the start) or samples[k] outside
 *     0 .. n_samples - 1; that entry and all behind it are ignored.  Indel entries and N bases are formatted like any other entry
 *   - a sample without an entry is "./."; a sample with one is "g:B:S:d.dddddd": g = "0/." where base == ref_base[s] (as ints: a
 *     negative ref_base matches nothing), else "./i" with i - 1 the LAST index below n_alt (n_alt > 3 is read as 3) whose
 *     alt_base & 7 equals the base, else "./."; B = "ACGTNN"[min(base, 5)]; S = "-+"[strand & 1]; d.dddddd = 1 - 10^(-qual / 10) as %.6f
 *     (the 256 strings of bvc_vcf_bp_lut).  The base is read & 7
 *   - fields are separated by tabs: n_samples fields, text_len = max(0, 4 * n_samples + 13 * (entries that count) - 1) bytes
 * Layout: site s has a slot iff results[s].called != 0, of bvc_vcf_samples_slot(n_samples, offsets[s + 1] - offsets[s]) bytes, the slots
 * one after the other in site order from byte 0 of `text`: text_off [n_sites + 1] are their starts (text_off[n_sites] = their sum, which
 * text_cap must reach), text_len [n_sites] the bytes of text in each (0 for a site that is not called).  The bytes of a slot behind its
 * text are unspecified; nothing outside the slots is written.
 * Host or device pointers (flags), as bvc_site_stats_csr: of `results` called, n_alt and alt_base are read and must be complete (overlap
 * mode: bvc_join first).  Device `entries` / `samples` may start at any element, device `text` must start on a 16-byte boundary (the text
 * is written with 16-byte stores); the device form waits once, for the sum of the slots, before it formats (asynchronously).  With host
 * pointers the small arrays are staged through the context's page-locked buffer, the entries and samples go up from the caller's memory
 * as it is and the text comes down straight into it (a DMA where that is bvc_host_alloc memory).  BVC_ERR_ARG: null pointers with work
 * present, a negative n_sites, n_samples or text_cap, host offsets that do not start at 0 or that decrease, a text_cap smaller than the sum
 * of the slots (bvc_last_error names the need; with host pointers nothing has been launched, with either the context stays usable).
 */
/* Bytes of a called site's slot, for callers to size `text`: 4 * n_samples + 13 * n_entries rounded up to 16. */
static inline int64_t bvc_vcf_samples_slot(int64_t n_samples, int64_t n_entries)
{
    return (4 * n_samples + 13 * n_entries + 15) / 16 * 16;
}
/* The eight characters d.dddddd for quality q at out[8 * q], q = 0..255.  Needs no context and no device. */
void bvc_vcf_bp_lut(char out[2048]);
int bvc_vcf_samples_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                        const int32_t *samples, const int8_t *ref_base, const bvc_site_result *results, int64_t n_samples,
                        char *text, int64_t text_cap, int64_t *text_off, int64_t *text_len, uint32_t flags);
/*
 * The same behind the producer calls.  bvc_pileup_finish_called_text is bvc_pileup_finish_called_stats without the gather and the
 * download of the called positions' entries and samples (stats is required): one wait.  It leaves the tile's columns and records on
 * the device, and until the next bvc_pileup_begin* on the context bvc_pileup_sample_text formats the called positions' sample columns
 * from them: text / text_off / text_len as above (host pointers), n_positions sites.  The caller sizes `text` from entry_off, results
 * and bvc_vcf_samples_slot; a text_cap that is too small is BVC_ERR_ARG (bvc_last_error names the need) and consumes nothing: the call
 * may be repeated with a larger buffer -- as it may be repeated anyway.  bvc_pileup_sample_text without a preceding
 * bvc_pileup_finish_called_text, or after the next begin: BVC_ERR_ARG.  One wait; the text comes straight into the caller's memory.
 */
int bvc_pileup_finish_called_text(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                                  const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                                  int64_t *entry_off, int32_t *tally, bvc_pileup_indel *indels, char *indel_text,
                                  bvc_site_result *results, bvc_group_result *grp_results, bvc_site_stats *stats);
int bvc_pileup_sample_text(bvc_ctx *ctx, int64_t n_samples, char *text, int64_t text_cap, int64_t *text_off, int64_t *text_len);

/* ---- byte ranges in device memory deflated into finished BGZF blocks (additive) --------------------- */
/*
 * Additive: a device deflate encoder (RFC 1951) for BGZF (SAM specification 4.1), the format of the host program's .vcf.gz.  A "piece"
 * is a range of bytes; a piece of len bytes becomes bvc_bgzf_blocks(len) blocks, each but the last of exactly BVC_BGZF_BLOCK_INPUT
 * input bytes (htslib's block size: a stored block always fits 64 KiB); a piece of 0 bytes yields no block (an empty block is the
 * end-of-file marker and never appears).  Every block is a complete, independent gzip member of at most 65536 bytes: the 18-byte
 * header with the BC extra field (BSIZE - 1) as the host program's BgzfWriter writes it, one deflate block with BFINAL set (fixed
 * Huffman codes, or stored where that is smaller) padded to a byte, CRC32 of the input bytes and ISIZE.  Matches stay inside the
 * block's own input (distances 1..32768, lengths 4..258).  The output is a pure function of the input bytes: the same pieces give the
 * same bytes on every run.  Concatenated in any order with other BGZF blocks and closed with the end-of-file marker they are a BGZF file.
 *
 * Tuning key "bgzf_codes" = 1 (bvc_set_tuning; default 0): the parse of a block -- its literals, lengths and distances -- stays the one
 * above, and the block is written in a Huffman code of its own (BTYPE = 10) iff its deflate data is then SMALLER, in bytes, than in the
 * form above (fixed, or stored); otherwise it is exactly the block key 0 writes.  Still one deflate block with BFINAL a BGZF block,
 * still a pure function of the input bytes.  The code is a function of the block's symbol counts alone (docs/BGZF_DYNAMIC.md, in short):
 *   (a) lengths of the literal/length alphabet (286 symbols, end of block counted once) and of the distance alphabet (30), limit 15:
 *       the used symbols in the order of (count, symbol); a Huffman tree by two queues, a leaf before an internal node of the same weight,
 *       internal nodes in the order they were made; leaves deeper than the limit are set to it and the Kraft sum is repaired by zlib's
 *       move (the deepest leaf above the limit's level one level down, a leaf of the limit's level made its sibling) once per unit of
 *       2^-limit; the multiset of lengths is then handed out longest first in the order of (count, symbol).  With fewer than two used
 *       symbols the used one (if any) and the smallest unused symbols of 0 and 1, two in all, get length 1
 *   (b) HLIT + HDIST lengths as ONE row (runs cross from the first alphabet into the second), greedily from the front: 11 or more zeros ->
 *       symbol 18 (at most 138), 3..10 zeros -> 17, 3 or more repeats of the length just written -> 16 (at most 6), else the length itself
 *   (c) HLIT, HDIST and HCLEN trimmed to the last used symbol (at least 257, 1 and 4)
 *   (d) the code-length code (19 symbols, limit 7) by rule (a)    (e) canonical codes, RFC 1951 3.2.2
 * bvc_bgzf_code_lengths (bvc_bgzf_codes.h) runs rule (a) on counts of the caller's.
 *
 * Tuning key "bgzf_parse" = 1 (default 0): another parse, for text made of short fields ended by tabs, with colons inside; whatever
 * "bgzf_codes" says is then done with ITS literals, lengths and distances.  A pure function of a block's input bytes x[0 .. n)
 * (docs/BGZF_FIELDS.md, in short): position p is a CUT iff p = 0 or x[p - 1] is a tab or a colon; a FIELD runs from a cut to the next, or
 * to n.  A field is a REPEAT iff the field in front of it has the same length L and the same bytes, else a HEAD.  A repeat's match has
 * distance L and the length min(e - p, 258) rounded down to a multiple of L, e the next head's start or n.  A head of 4..32 bytes looks
 * for earlier heads with the same hash of (L, bytes) -- seventeen candidates at the most, a function of the bytes -- extends each up to
 * 258 bytes, drops those that hold fewer than L, cuts the others back to the last cut (or n) they reach and keeps the longest, the
 * nearest among equals.  No other position has a match, a match is used from 4 bytes on, and the path is the greedy walk of key 0.
 * Tuning key "bgzf_cuts" = 1 (default 0) reads "a space or a newline" for "a tab or a colon" in the rule above, and changes nothing else.
 */
#define BVC_BGZF_BLOCK_INPUT 65280
/* Blocks of a piece: ceil(len / 65280), 0 for len <= 0. */
static inline int64_t bvc_bgzf_blocks(int64_t len)
{
    return len <= 0 ? 0 : (len + BVC_BGZF_BLOCK_INPUT - 1) / BVC_BGZF_BLOCK_INPUT;
}
/* The most bytes the blocks of a piece take (every block stored: 18 + 5 + 8 bytes around its input), for callers to size `comp`. */
static inline int64_t bvc_bgzf_bound(int64_t len)
{
    return len <= 0 ? 0 : len + (len + BVC_BGZF_BLOCK_INPUT - 1) / BVC_BGZF_BLOCK_INPUT * 31;
}
/*
 * Piece i is data[piece_off[i] .. piece_off[i] + piece_len[i]); pieces may start at any byte and need not be adjacent or ordered.  Its
 * blocks are comp[comp_off[i] .. comp_off[i + 1]): comp_off [n_pieces + 1], comp_off[0] = 0, the blocks of all pieces one after the
 * other in piece order without gaps.  Nothing beyond comp_off[n_pieces] is written.  comp_cap must reach the sum of
 * bvc_bgzf_bound(piece_len[i]).
 * Host or device pointers (flags).  With host pointers the bytes of the pieces go up through the context's page-locked buffer, nothing
 * is launched before the arguments have been checked, and the call waits twice: for comp_off, then for the packed bytes (only they come
 * down, never a bound-sized buffer).  With device pointers the call waits for piece_off and piece_len (the launches are sized from the lengths)
 * and, briefly, for its table of (n_pieces + 1) * 8 bytes to have gone up; the blocks and comp_off are then written asynchronously on the
 * context's stream.
 * BVC_ERR_ARG: null pointers with work present, a negative n_pieces, piece_off, piece_len or comp_cap, a comp_cap smaller than the sum
 * of the bounds (bvc_last_error names the need); the context stays usable.
 */
int bvc_bgzf_deflate(bvc_ctx *ctx, int64_t n_pieces, const uint8_t *data, const int64_t *piece_off, const int64_t *piece_len,
                     uint8_t *comp, int64_t comp_cap, int64_t *comp_off, uint32_t flags);
/*
 * bvc_pileup_sample_text's twin: after bvc_pileup_finish_called_text and until the next bvc_pileup_begin* on the context it
 * formats the called positions' sample columns into device memory of the context's and delivers each position's text as BGZF blocks;
 * the text never comes to the host.  Host pointers: comp_off [n_positions + 1] (an empty range for a position that is not called),
 * text_len [n_positions] as bvc_pileup_sample_text reports it.  The caller sizes `comp` from entry_off, the results,
 * bvc_vcf_samples_slot and bvc_bgzf_bound: comp_cap must reach the sum of bvc_bgzf_bound(bvc_vcf_samples_slot(n_samples, entries of
 * the position)) over the called positions; a comp_cap that is too small is BVC_ERR_ARG (bvc_last_error names the need) and consumes
 * nothing.  The call may be repeated, and made beside bvc_pileup_sample_text in either order; out of sequence it is BVC_ERR_ARG as its
 * twin.  Two waits, one more than its twin: for comp_off and text_len, then for the packed bytes, which come straight into the caller's
 * memory.
 */
int bvc_pileup_sample_bgzf(bvc_ctx *ctx, int64_t n_samples, uint8_t *comp, int64_t comp_cap, int64_t *comp_off, int64_t *text_len);
/* Rule (a) of "bgzf_codes" on counts of the caller's -- bvc_bgzf_code_lengths -- is declared in bvc_bgzf_codes.h beside this header. */
/* Phase 1 on the device -- bvc_bam_pileup: inflated BAM records of a batch of samples -> the batch's binary position records -- is declared
 * in bvc_bam.h beside this header; its twin for the text temp batches -- bvc_bam_pileup_text: the same records -> the batch's lines -- in
 * bvc_bam_text.h. */
/* `BaseVarC popmatrix` on the device -- bvc_bam_popmatrix: the same records and a position file's lines -> one row of '0' / '1' / '.' per
 * sample (BVC_BAM_MORE there: some sample's bytes ran out) -- is declared in bvc_popmatrix.h beside this header. */
/* Temp batches that stay on the device -- bvc_store_*: a batch's records kept in device memory, bvc_pileup_begin_store: a tile of positions
 * gathered from all kept batches -- are declared in bvc_store.h beside this header. */
/* Phase 1's temp batches deflated where they are made -- bvc_bam_pileup_bgzf_deflate, bvc_bam_pileup_text_bgzf_deflate: BAM blocks in, the
 * batch's finished BGZF blocks out -- are declared in bvc_bam_deflate.h beside this header. */
/* Phase 1 straight into class counts -- bvc_bam_counts: the same BAM records added into per-position class counts and tallies, bvc_site_acc_*:
 * such counts kept on the device and called from there -- are declared in bvc_bam_counts.h beside this header. */
/* The same into ONE slot of class counts with the groups' depths per base beside it -- bvc_bam_counts_depth, bvc_site_acc_create_depth,
 * bvc_site_acc_get_depth: 16 bytes a group and position where bvc_bam_counts takes 2 KB -- is declared in bvc_bam_group_depth.h beside this
 * header. */
/* Such counts in narrow quality rows -- bvc_bam_counts_quals, bvc_site_acc_create_quals, bvc_site_acc_quals: 16 x n_quals bytes a position
 * where a row of 128 quality columns takes 2 KB, and a batch that needs a higher quality is refused -- are declared in bvc_site_acc_quals.h
 * beside this header. */

#ifdef __cplusplus
}
#endif
#endif /* BVC_H */
