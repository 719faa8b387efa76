/*
 * bvc_site_acc_quals.h -- C ABI of libbvc, tenth header: class counts kept in NARROW quality rows.  A row of bvc_bam_counts (bvc_bam_counts.h)
 * holds 128 quality columns for each of the four bases, 2 KB a position, and base qualities stop far below 128: most of a row is zeros.
 * The calls below keep only the first n_quals quality columns of each base, counts [position][4][n_quals], 16 x n_quals bytes a position
 * beside the tally and the optional depth rows of the groups (bvc_bam_group_depth.h): n_positions x (16 x n_quals + 48 + 16 x n_groups)
 * bytes whatever the number of samples.  With n_quals = 48 that is 816 bytes a position where the wide row with its tally takes 2,096.
 * The price is a promise the caller makes about the data: a batch that holds a counted observation of quality n_quals or more is REFUSED,
 * before anything is added (sample status 5 below), and the caller starts again with a larger n_quals.  Everything of bvc.h,
 * bvc_bam_counts.h and bvc_bam_group_depth.h (conventions, contexts, return codes, the tally, the depth rows, the accumulator's calls) holds
 * here; the entry points below are exported by the same library.  A header of its own because the ninth header's list of entry points is
 * closed.
 */
#ifndef BVC_SITE_ACC_QUALS_H
#define BVC_SITE_ACC_QUALS_H

#include "bvc_bam_group_depth.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bvc_bam_counts_depth (the arguments up to n_groups, the record filter, the per-position rule, tally [n_positions] and group_depth
 * [n_positions][n_groups][4] are that call's word for word) with n_quals in front of the arrays and counts [n_positions][4][n_quals].
 * n_quals is a multiple of 4 in 4..128 (BVC_ERR_ARG otherwise): a position's counts are a multiple of 64 bytes.  n_groups is 0..32; with
 * n_groups == 0 nothing is read of group_of_sample or group_depth, which may be null.  What a call that returns BVC_OK adds:
 *   the tally                   exactly as bvc_bam_counts adds it
 *   a base entry of base 0..3   with a quality byte q < n_quals: counts[(t * 4 + base) * n_quals + q] += 1, and under the same condition
 *                               the depth of the sample's group, as bvc_bam_counts_depth adds it
 *   a quality byte 128..255     is tallied and never counted, as there; it is never a reason to refuse
 * So with the same inputs counts[t][base][q] is the wide call's counts[t][base * 128 + q] for every q < n_quals, and with n_quals = 128
 * the two arrays are the same bytes.
 *
 * sample_status 5: a sample that has, at one of the call's positions, a base entry of base 0..3 whose quality byte q is n_quals <= q <= 127
 * -- an observation the wide call counts and this one has no column for.  Statuses 0..4 are bvc_bam_counts's.  A sample gets ONE status:
 * where the out-of-range rule (status 4) holds at one position and such a quality lies at another, the sample's status is 4 -- the
 * record is at fault, not the choice of n_quals -- whichever position a lane reaches first.  The verdict of bvc_bam_counts runs first, on
 * the statuses 2, 3 and 4, with its return codes and messages; a call it would pass returns BVC_ERR_DATA when some sample has status 5,
 * and bvc_last_error names the first such sample and n_quals.  The promise holds: after every return other than BVC_OK all three arrays
 * hold what they held.  The BVC_PTR_HOST / BVC_PTR_DEVICE forms, the one wait in the middle and the scratch are bvc_bam_counts's.
 */
int bvc_bam_counts_quals(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups, int32_t n_quals,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags);

/*
 * An accumulator of the third kind: ONE slot of counts [n_positions][4][n_quals], the tallies and group_depth [n_positions][n_groups][4]
 * (n_groups 0..32; 0: no depth rows), all zeroed.  byte_budget, the return codes and the refusals are bvc_site_acc_create_depth's, plus
 * BVC_ERR_ARG for an n_quals that is no multiple of 4 in 4..128.  With n_quals = 128 the stored bytes are those of the first kind
 * (n_groups 0) or the second.  The calls of bvc_bam_counts.h and bvc_bam_group_depth.h take it as follows:
 *   bvc_site_acc_bytes        *used is exactly n_positions x (16 x n_quals + 48 + 16 x n_groups)
 *   bvc_bam_counts_bgzf_acc   adds as bvc_bam_counts_quals does with the accumulator's n_quals and n_groups (a null group_of_sample with
 *                             n_groups > 0 and samples present is BVC_ERR_ARG); a batch with a sample of status 5 is BVC_ERR_DATA and
 *                             adds nothing
 *   bvc_site_acc_get          counts [n][1][512], EXPANDED: the wide layout with zeros in the columns >= n_quals, and tally [n]
 *   bvc_site_acc_get_depth    unchanged; refuses an accumulator with n_groups 0
 *   bvc_site_acc_lrt          bvc_lrt_hist on the expanded rows, a bounded piece of them at a time in the context's scratch; grp_results
 *                             is ignored.  The records are byte for byte those of a wide accumulator that was given the same batches
 *   bvc_site_acc_destroy      frees it
 * Every call on an accumulator of the first two kinds is what it was.
 */
int bvc_site_acc_create_quals(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int32_t n_quals, int64_t byte_budget);

/* *n_quals: the quality columns the accumulator stores for each base -- what it was made with, 128 for the first two kinds.
 * BVC_ERR_ARG: a null pointer. */
int bvc_site_acc_quals(const bvc_site_acc *acc, int32_t *n_quals);

#ifdef __cplusplus
}
#endif
#endif /* BVC_SITE_ACC_QUALS_H */
