/*
 * bvc_bam_deflate.h -- C ABI of libbvc, seventh header: phase 1 of `BaseVarC basetype` with the temp batches deflated where they are made.
 * The BAM blocks of a batch of samples go in, the batch's finished BGZF blocks come out; the records (or lines) between the two never
 * reach the host.  Everything of bvc.h (conventions, contexts, return codes) holds here; the entry points below are exported by the same
 * library.  A header of its own because bvc.h's list of entry points is closed (bvc_bam.h's opening comment).
 */
#ifndef BVC_BAM_DEFLATE_H
#define BVC_BAM_DEFLATE_H

#include "bvc_bam.h"
#include "bvc_bam_text.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * bvc_bam_pileup_bgzf (bvc_bam.h) and bvc_bam_pileup_text_bgzf (bvc_bam_text.h) with bvc_bgzf_deflate (bvc.h) behind them on the device.
 * Every argument up to refseq_len is that call's, unchanged; so are sample_status, the statuses 0..4, BVC_BAM_MORE for a sample of status
 * 2, BVC_ERR_DATA (a sample of status 3 or 4, a block that is not valid deflate of its ISIZE bytes or fails its CRC32) and BVC_ERR_ARG
 * for records (or text) of more than 0xFFFFFF00 bytes.  Host pointers only; comp is best placed in bvc_host_alloc memory.
 *
 * The PIECES: piece_pos [n_pieces + 1] are indices into `positions`, non-decreasing, piece_pos[0] = 0 and piece_pos[n_pieces] =
 * n_positions (anything else, or n_pieces < 0, is BVC_ERR_ARG before anything is launched).  Piece i is the records (lines) of positions
 * [piece_pos[i], piece_pos[i + 1]): the bytes [rec_start[piece_pos[i]], rec_start[piece_pos[i + 1]]) of what the call above would have
 * returned; piece_bytes[i] is that length.  A piece without a position yields no block.
 *
 * The BLOCKS of piece i are out[out_off[i] .. out_off[i + 1]), out_off[0] = 0, all pieces one behind the other without gaps.  They are
 * exactly the bytes bvc_bgzf_deflate writes for the same pieces under the context's tuning keys ("bgzf_codes", "bgzf_parse",
 * "bgzf_cuts"): every block a complete BGZF block of at most BVC_BGZF_BLOCK_INPUT input bytes.
 *
 * *out_needed (a host pointer) is always set: 0 when a sample has status 2, 3 or 4 or the call fails, else the packed size
 * out_off[n_pieces].  (One failure reports a size, as the calls above do: BVC_ERR_ARG for more than 0xFFFFFF00 bytes of records or text
 * sets it to that UNCOMPRESSED size.)  out_cap < *out_needed is BVC_BAM_MORE too: out_off and piece_bytes are written, `out` is not, and
 * the finished blocks stay in the context until the next of these two calls on it, from where bvc_bam_pileup_deflate_fetch delivers them
 * without computing anything again (so a call with out_cap 0 and a fetch sized from *out_needed is the two-step form).  Only BVC_OK and
 * that BVC_BAM_MORE write out_off and piece_bytes; only BVC_OK writes `out`, and nothing beyond *out_needed bytes of it.
 *
 * Nothing uncompressed comes down.  Three waits at the most: for the sizes and the statuses, for out_off, for the packed bytes (which come
 * straight into the caller's memory).  The scratch is the two calls' together with the uncompressed batch and the bound of its blocks; a
 * second call of the same shape allocates nothing.
 */
int bvc_bam_pileup_bgzf_deflate(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                                int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                                const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                                int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                                int32_t n_pieces, const int32_t *piece_pos, uint8_t *out, int64_t out_cap, int64_t *out_needed,
                                int64_t *out_off, int64_t *piece_bytes, uint32_t *sample_status);
/* The same with the batch's lines (the text temp-batch form of bvc_bam_text.h) in the records' place. */
int bvc_bam_pileup_text_bgzf_deflate(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                                     int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                                     const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                                     int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                                     int32_t n_pieces, const int32_t *piece_pos, uint8_t *out, int64_t out_cap, int64_t *out_needed,
                                     int64_t *out_off, int64_t *piece_bytes, uint32_t *sample_status);
/*
 * The blocks the last of the two calls above left in the context when it returned BVC_BAM_MORE for out_cap: the *out_needed bytes it
 * reported, into out.  One wait.  BVC_ERR_ARG, with what is kept still kept: nothing is kept (no such call yet, or the last one returned
 * anything else), out_cap below the kept size, a null out with bytes to deliver.  The fetch may be repeated.
 */
int bvc_bam_pileup_deflate_fetch(bvc_ctx *ctx, uint8_t *out, int64_t out_cap);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BAM_DEFLATE_H */
