/*
 * bvc_bam_text.h -- C ABI of libbvc, fifth header: phase 1 of `BaseVarC basetype` on the device for the TEXT temp batches, the form the
 * reference writes and reads and the default of --tmp-format.  Everything of bvc.h (conventions, contexts, return codes) holds here; the
 * entry points below are exported by the same library.  They have a header of their own because bvc.h's list of entry points is closed
 * and bvc_bam.h is held to its own table (tests/test_bam_pileup_abi.py).
 */
#ifndef BVC_BAM_TEXT_H
#define BVC_BAM_TEXT_H

#include "bvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Additive: bvc_bam_pileup (bvc_bam.h) with the batch's LINES as its output, byte for byte what the host program's bt_r writes per
 * position with `--tmp-format text` behind the names line (the reference's src/BaseVarC.cpp:509-527):
 *   line   = token of sample 0 | token of sample 1 | ... | "\n"
 *   token  = ". "                                   the sample has no entry at the position
 *          | "base,mapq,qual,rpr,strand "           a base entry: five unsigned decimals (base 0..4, the others bytes, strand 0 / 1)
 *          | indel text " "                         an indel entry: "-" + the reference bases (clamped at refseq's end: "- " when none is
 *                                                   left) or "+" + the read's bases
 * one line per position, in position order.  With n_samples == 0 every line is "\n"; with n_positions == 0 nothing is written and
 * *text_needed is 0.
 *
 * Every input, the record filter, the per-position rule, sample_status 0..4, the return codes and their rules are bvc_bam_pileup's, word
 * for word, with text / text_cap / text_needed / line_start in the places of records / records_cap / records_needed / rec_start:
 * BVC_BAM_MORE for a sample of status 2 or text_cap < *text_needed; BVC_ERR_DATA names the first sample of status 3 or 4; only BVC_OK
 * writes text and line_start; *text_needed (a HOST pointer with either flag) is always set, 0 when a sample has status 2, 3 or 4;
 * *text_needed > 0xFFFFFF00 is BVC_ERR_ARG (line_start is 32-bit).  Two differences, both of the form and not of the rule: an indel text
 * is WHOLE (the binary entry's bound of 0xffff bytes belongs to that entry's 16-bit length field), and an indel token shows no fields,
 * so the mapq an indel entry inherits there has no counterpart here.
 *
 *   text         out: the lines, *text_needed bytes.  text_cap: room in it
 *   line_start   out: [n_positions + 1]: position t's line begins at line_start[t]; line_start[n_positions] = one past the last newline
 *
 * BVC_PTR_HOST / BVC_PTR_DEVICE as bvc_bam_pileup: with device pointers ONE wait in the middle of the call.  The scratch is that call's
 * (the read table, a size matrix of one tile of at most 1024 positions x n_samples, O(n_positions + n_samples)); a second call of the same
 * shape allocates nothing.
 */
int bvc_bam_pileup_text(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                        const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                        int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                        uint8_t *text, int64_t text_cap, int64_t *text_needed, uint32_t *line_start, uint32_t *sample_status, uint32_t flags);
/*
 * The same from the samples' BGZF blocks, still compressed: what the host program's phase 1 calls per batch with --tmp-format text
 * (BVC_HOST_DEVICE_PILEUP_TEXT).  comp / blocks / bam_bytes and every rule as bvc_bam_pileup_bgzf: host pointers only, synchronises the
 * context's stream, and a block that is not valid deflate of its ISIZE bytes or fails its CRC32 is BVC_ERR_DATA whatever the kernels made
 * of its bytes.
 */
int bvc_bam_pileup_text_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                             int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                             int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                             const char *refseq, int64_t refseq_len, uint8_t *text, int64_t text_cap, int64_t *text_needed,
                             uint32_t *line_start, uint32_t *sample_status);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BAM_TEXT_H */
