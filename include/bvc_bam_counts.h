/*
 * bvc_bam_counts.h -- C ABI of libbvc, eighth header: phase 1 of `BaseVarC basetype` added straight into per-position class counts.  A
 * position's call depends on its samples only through 512 class counts, and the coverage line of a position without indel entries only
 * through eight strand x base counts: this is the link BAM -> counts in front of bvc_counts_add_* / bvc_lrt_hist[_groups], at 2 KB + 48
 * bytes per position whatever the number of samples.  Everything of bvc.h (conventions, contexts, return codes) holds here; the entry
 * points below are exported by the same library.  A header of its own because bvc.h's list of entry points is closed (bvc_bam.h's
 * opening comment).
 */
#ifndef BVC_BAM_COUNTS_H
#define BVC_BAM_COUNTS_H

#include "bvc_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a position's entries amount to beside its class counts: enough for the coverage line of a position that has no indel entry, and to
 * tell which positions need their entries after all (those with n_indel > 0, and their predecessor that holds a base token). */
typedef struct bvc_bam_site_tally {      /* 48 bytes */
    uint32_t strand_base[8];             /* [strand << 2 | base], base 0..3: base entries, whatever their quality byte */
    uint32_t n_other;                    /* base entries of class 4: dropped by phase 2, but still "the last base token" */
    uint32_t n_indel;                    /* indel entries */
    uint32_t pad[2];
} bvc_bam_site_tally;
/* counts [n_positions][slots][512] + tally [n_positions] on ONE device, zeroed at creation; slots = 1, or n_groups + 1 with groups */
typedef struct bvc_site_acc bvc_site_acc;

/*
 * bvc_bam_pileup's inputs (bvc_bam.h: the arguments up to rg_s mean what they mean there, the record filter and the per-position rule are
 * that call's word for word) ADDED into counts and tally instead of written out as records.  There is no refseq pointer: only refseq_len
 * and rg_s decide whether a deletion's text starts inside the reference (status 4).  For every (sample, position) that has an entry:
 *   a base entry of base 0..3   tally[t].strand_base[strand << 2 | base] += 1, whatever its quality byte; and with a quality byte of
 *                               0..127 (bvc.h's rule for a covered observation) counts[(t * slots + slot) * 512 + base * 128 + qual] += 1
 *   a base entry of class 4     tally[t].n_other += 1
 *   an indel entry              tally[t].n_indel += 1
 * n_groups == 0: slots = 1, slot = 0 -- the layout of bvc_counts_add_csr / bvc_lrt_hist.  n_groups 1..32: slots = n_groups + 1 and sample
 * s adds to slot group_of_sample[s], or to slot n_groups when its label is >= n_groups -- the layout of bvc_counts_add_dense_groups /
 * bvc_lrt_hist_groups.  All adds are modulo 2^32; nothing is ever stored, so several calls (of several contexts and threads of the device)
 * may add into the same arrays at the same time.
 *
 * sample_status and the return codes are exactly bvc_bam_pileup's for the same inputs, except that there is no records_cap: BVC_BAM_MORE
 * only ever means a sample of status 2.  After every return other than BVC_OK counts and tally hold what they held: the call resolves
 * every cell once without adding (which finds the samples of status 4), waits for the verdict, and only then adds.  BVC_ERR_ARG as there,
 * plus n_groups outside 0..32 and a null group_of_sample with n_groups > 0 and samples present.
 *
 * BVC_PTR_DEVICE: every array is device memory; ONE wait in the middle of the call, the adds are enqueued on the context's stream when it
 * returns.  BVC_PTR_HOST: the convenience form, as of bvc_counts_add_*: counts and tally go up, are added to and come back (a second
 * wait).  Scratch is bvc_bam_popmatrix's: the read table and O(n_samples); a second call of the same shape allocates nothing.
 */
int bvc_bam_counts(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                   const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                   const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                   uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *sample_status, uint32_t flags);

/*
 * An accumulator: counts and tallies of n_positions positions on `device`, zeroed.  It belongs to no context; adds through several contexts
 * and threads of its device may run at the same time (they are atomic adds).  It must outlive every call that names it.  byte_budget: the
 * most device memory it may take (what bvc_site_acc_bytes reports as used); <= 0: no cap but the device's.  BVC_ERR_ARG: null out, negative
 * n_positions, n_groups outside 0..32.  BVC_ERR_ALLOC: over the budget, or the device has no room.  BVC_ERR_DEVICE: the device cannot be
 * used.
 */
int bvc_site_acc_create(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget);
/* frees the arrays; null is ignored.  No call that names the accumulator may be running */
void bvc_site_acc_destroy(bvc_site_acc *acc);
/* *used: device bytes of the counts and tallies; *budget: byte_budget as given.  Either may be null */
int bvc_site_acc_bytes(const bvc_site_acc *acc, int64_t *used, int64_t *budget);

/*
 * bvc_bam_counts from the samples' BGZF blocks, still compressed (bvc_bam_pileup_bgzf's input arguments, without refseq), added into acc
 * with its n_groups.  Host pointers; synchronises the context's stream.  n_positions must be the accumulator's and the context one of its
 * device (BVC_ERR_ARG).  A block that is not valid deflate of its ISIZE bytes or fails its CRC32 is BVC_ERR_DATA, found at the call's
 * first wait: nothing is added.  Only BVC_OK adds.
 */
int bvc_bam_counts_bgzf_acc(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                            int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                            int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                            int64_t refseq_len, const uint8_t *group_of_sample, bvc_site_acc *acc, uint32_t *sample_status);

/* Rows [t0, t0 + n) to the host: counts [n][slots][512] (may be NULL: the tallies alone) and tally [n].  Waits for the context's stream;
 * adds of other contexts must have returned.  BVC_ERR_ARG: rows outside the accumulator, a context of another device, null tally with n > 0. */
int bvc_site_acc_get(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, uint32_t *counts, bvc_bam_site_tally *tally);

/*
 * Stage 2 on rows [t0, t0 + n) where they lie: bvc_lrt_hist, or bvc_lrt_hist_groups when the accumulator has groups (grp_results
 * [n][n_groups] is then required, else ignored).  ref_base [n], results [n] and grp_results are HOST memory; the records are byte for byte
 * those calls' on the counts bvc_site_acc_get delivers.  Waits for the context's stream.
 */
int bvc_site_acc_lrt(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, const int8_t *ref_base, double min_af,
                     bvc_site_result *results, bvc_group_result *grp_results);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BAM_COUNTS_H */
