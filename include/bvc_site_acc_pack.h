/*
 * bvc_site_acc_pack.h -- C ABI of libbvc, eleventh header: an accumulator's rows in a SPARSE form.  An accumulator (bvc_bam_counts.h,
 * bvc_bam_group_depth.h, bvc_site_acc_quals.h) comes off the device only as [n][slots][512] rows, 2 KB a position whatever the row holds,
 * and the only way into one is a batch of BAM records.  Almost all of a row is zeros, and class counts are sums: the calls below turn rows
 * into the list of their non-zero words (pack) and ADD such a list into rows (add_packed), so that partial counts can be kept, moved and
 * summed.  Everything of bvc.h and the three headers named above (conventions, contexts, return codes, the tally, the depth rows, the
 * accumulator's calls) holds here; the entry points below are exported by the same library.  A header of its own because the tenth
 * header's list of entry points is closed.
 *
 * THE LOGICAL ROW.  An accumulator of any of the three kinds has, per position, one logical row of
 *     W = slots * 512 + 10 + 4 * depth_groups        words (slots = n_groups + 1 for the first kind with groups, else 1):
 *   cells 0 .. slots * 512     the class counts in the WIDE layout, slot * 512 + base * 128 + qual; a narrow accumulator's column q of
 *                              base b is cell b * 128 + q
 *   the next 10                the tally's words 0..9: strand_base[8], n_other, n_indel (its two pad words are no part of the row)
 *   the next 4 * depth_groups  the depth row, g * 4 + base
 * W is at most 33 * 512 + 10 + 128 = 17,034: a cell index fits 16 bits.
 *
 * A PACKED PIECE of rows [t0, t0 + n) is three arrays; the entries are in rows ascending, and within a row cells strictly ascending:
 *   int64_t  row_start[n + 1]      entry offsets, row_start[0] = 0
 *   uint16_t cell[n_entries]       the logical cell of each entry
 *   uint32_t count[n_entries]      the cell's count
 * A cell is an entry of what bvc_site_acc_pack delivers if and only if its word is not zero.  Because cells are logical, the same piece
 * comes from a wide and a narrow accumulator that hold the same counts, and it goes into either.
 */
#ifndef BVC_SITE_ACC_PACK_H
#define BVC_SITE_ACC_PACK_H

#include "bvc_site_acc_quals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BVC_ACC_MORE 2   /* bvc_site_acc_pack: entries_cap is too small; *n_entries says what is needed (positive, like BVC_BAM_MORE) */

/* The shape of the accumulator's logical row: *row_words = W, *slots, *depth_groups (each may be null).  BVC_ERR_ARG: a null accumulator. */
int bvc_site_acc_row_words(const bvc_site_acc *acc, int32_t *row_words, int32_t *slots, int32_t *depth_groups);

/*
 * Rows [t0, t0 + n) as a packed piece.  Two steps, like bvc_bam_pileup's records_cap: *n_entries is always the number of entries the rows
 * hold; where entries_cap is smaller the call returns BVC_ACC_MORE and has written row_start in full and nothing of cell and count (they
 * may then be null), and the caller comes again with room.  BVC_PTR_HOST: the three arrays are host memory; the call returns with them
 * complete.  BVC_PTR_DEVICE: they are device memory; ONE wait in the middle of the call, for the total, and the place pass is enqueued on
 * the context's stream when it returns.  n_entries is host memory in both forms.  n == 0: row_start[0] = 0, *n_entries = 0.
 * BVC_ERR_ARG: rows outside the accumulator, a context of another device, a negative entries_cap, null row_start or n_entries, null cell or
 * count with room for an entry that exists.  Adds of other contexts must have returned, as for bvc_site_acc_get.  Scratch is the
 * context's, 4 bytes a row (and in the host form the piece itself); a second call of the same shape allocates nothing.
 * COST: the size and place passes run across the whole device, but row_start is made by ONE wavefront that walks the n rows 256 at a
 * time, in front of the call's wait (and bvc_site_acc_add_packed's search for the first row at fault is one wavefront over n rows, 64 at
 * a time): a serial part that is small for pieces of 1e4 - 1e5 rows and grows with n.  Callers with millions of rows get the device's
 * rate by packing them in pieces, as the host program does with 65,536 rows a piece.
 */
int bvc_site_acc_pack(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, int64_t *row_start, uint16_t *cell, uint32_t *count,
                      int64_t entries_cap, int64_t *n_entries, uint32_t flags);

/*
 * ADDS a packed piece into rows [t0, t0 + n): for every entry, the word of its cell += count, modulo 2^32, with atomic adds that return
 * nothing -- several contexts and threads of the device may add pieces and batches (bvc_bam_counts_bgzf_acc) into one accumulator at
 * once.  An entry with count 0 is legal and adds nothing.  The promise of bvc_bam_counts holds here: a dry pass validates the piece, one
 * wait brings the verdict, and only then the add pass runs; after every return other than BVC_OK the accumulator holds what it held.
 * BVC_ERR_DATA, with bvc_last_error naming the first row at fault ("row <t>: ...", t counted from the piece's first row), covers
 *   row_start                  not starting at 0, decreasing, or not ending at n_entries (a word outside 0..n_entries is the fault of
 *                              the row it ends, which is then the first at fault)
 *   a cell >= W
 *   cells of a row             not strictly ascending
 *   on a narrow accumulator    a count cell whose quality is >= n_quals: bvc_site_acc_quals.h's status 5 rule, and the message names n_quals
 * A row's fault is that of its first entry at fault, in the order above.  The add pass compares every cell with the accumulator's bounds
 * again before it makes an address of it, whatever the dry pass found.  BVC_PTR_HOST: the arrays are host memory; the call returns when
 * the adds are done.  BVC_PTR_DEVICE: device memory; ONE wait in the middle, the adds are enqueued on the context's stream when it returns.
 * BVC_ERR_ARG: rows outside the accumulator, a context of another device, a negative n_entries, null row_start, null cell or count with
 * n_entries > 0.  n == 0 with n_entries != 0 is BVC_ERR_DATA (row 0).  Scratch as above.
 */
int bvc_site_acc_add_packed(bvc_ctx *ctx, bvc_site_acc *acc, int32_t t0, int32_t n, const int64_t *row_start, const uint16_t *cell,
                            const uint32_t *count, int64_t n_entries, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* BVC_SITE_ACC_PACK_H */
