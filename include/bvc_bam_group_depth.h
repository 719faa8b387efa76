/*
 * bvc_bam_group_depth.h -- C ABI of libbvc, ninth header: phase 1 added into ONE slot of class counts with the groups' depths beside it.
 * bvc_bam_counts (bvc_bam_counts.h) with groups keeps a 512-class slot for every group, 2 KB x (n_groups + 1) a position, because
 * bvc_lrt_hist_groups fits every group from its own counts.  A caller that fits the groups elsewhere -- the host program fits them at the
 * called positions only, from records it piles up a second time -- needs of the groups in this pass only what the coverage line of EVERY
 * position prints: the covered observations of each group per base.  That is 16 bytes a group and position beside one slot of counts and
 * the tally: 2 KB + 48 B + 16 x n_groups B a position whatever the number of samples.  Everything of bvc.h and bvc_bam_counts.h
 * (conventions, contexts, return codes, the tally, the accumulator's calls) holds here; the entry points below are exported by the same
 * library.  A header of its own because the eighth header's list of entry points is closed.
 */
#ifndef BVC_BAM_GROUP_DEPTH_H
#define BVC_BAM_GROUP_DEPTH_H

#include "bvc_bam_counts.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bvc_bam_counts with n_groups == 0 (the arguments up to refseq_len, the record filter, the per-position rule, counts [n_positions][512]
 * and tally [n_positions] are that call's word for word) and one array more, group_depth [n_positions][n_groups][4].  For every
 * (sample, position) that has a base entry of base 0..3 with a quality byte of 0..127 -- exactly the entries that add a class count --
 * and whose sample's label g = group_of_sample[s] is < n_groups:
 *     group_depth[(t * n_groups + g) * 4 + base] += 1
 * A label >= n_groups (in no group) adds no depth; its counts and tally are added as every sample's.  So group_depth[t][g][b] is the sum
 * over the 128 quality classes of base b of slot g of what bvc_bam_counts adds with the same labels (bvc_group_result.depth of that
 * slot), and counts is the sum of that call's slots.  All adds are modulo 2^32 and atomic, as there.
 *
 * n_groups is 1..32 and group_of_sample must not be null with samples present (BVC_ERR_ARG).  The call sequence (index, a pass that
 * resolves every cell without adding, the verdict, then the adds), sample_status, the return codes and the BVC_PTR_HOST / BVC_PTR_DEVICE
 * forms are bvc_bam_counts's, and so is the promise: after every return other than BVC_OK all three arrays hold what they held.
 */
int bvc_bam_counts_depth(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags);

/*
 * An accumulator of the second kind: ONE slot of counts [n_positions][512], the tallies and group_depth [n_positions][n_groups][4], all
 * zeroed.  byte_budget, the return codes and the refusals are bvc_site_acc_create's, except that n_groups is 1..32.  The calls of
 * bvc_bam_counts.h take it as follows:
 *   bvc_site_acc_bytes        *used counts all three arrays: n_positions x (2048 + 48 + 16 x n_groups)
 *   bvc_bam_counts_bgzf_acc   adds as bvc_bam_counts_depth does; a null group_of_sample with samples present is BVC_ERR_ARG
 *   bvc_site_acc_get          counts [n][1][512] and tally [n]
 *   bvc_site_acc_lrt          bvc_lrt_hist on the one slot; grp_results is ignored
 *   bvc_site_acc_destroy      frees it
 * Every call on an accumulator made by bvc_site_acc_create is what it was.
 */
int bvc_site_acc_create_depth(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget);

/* Rows [t0, t0 + n) of the depths to the host: group_depth [n][n_groups][4].  Waits for the context's stream; adds of other contexts must
 * have returned.  BVC_ERR_ARG: rows outside the accumulator, a context of another device, null group_depth with n > 0, an accumulator made
 * by bvc_site_acc_create (it has no depths: they are sums over its slots). */
int bvc_site_acc_get_depth(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, uint32_t *group_depth);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BAM_GROUP_DEPTH_H */
