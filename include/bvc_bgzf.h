/*
 * bvc_bgzf.h -- C ABI of libbvc, third header: byte ranges in device memory deflated into finished BGZF blocks on the device.
 * Everything of bvc.h (conventions, records, contexts, flags) holds here; the entry points below are exported by the same library.
 * They have a header of their own because the lists of entry points of bvc.h and bvc_vcf.h are closed: their bindings are generated
 * from, and checked against, those lists.
 */
#ifndef BVC_BGZF_H
#define BVC_BGZF_H

#include "bvc_vcf.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Additive: a device deflate encoder (RFC 1951) for BGZF (SAM specification 4.1), the format of the host program's .vcf.gz.  A "piece"
 * is a range of bytes; a piece of len bytes becomes bvc_bgzf_blocks(len) blocks, each but the last of exactly BVC_BGZF_BLOCK_INPUT
 * input bytes (htslib's block size: a stored block always fits 64 KiB); a piece of 0 bytes yields no block (an empty block is the
 * end-of-file marker and never appears).  Every block is a complete, independent gzip member of at most 65536 bytes: the 18-byte
 * header with the BC extra field (BSIZE - 1) as the host program's BgzfWriter writes it, one deflate block with BFINAL set (fixed
 * Huffman codes, or stored where that is smaller) padded to a byte, CRC32 of the input bytes and ISIZE.  Matches stay inside the
 * block's own input (distances 1..32768, lengths 4..258).  The output is a pure function of the input bytes: the same pieces give the
 * same bytes on every run.  Concatenated in any order with other BGZF blocks and closed with the end-of-file marker they are a BGZF file.
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
 * bvc_pileup_sample_text's twin (bvc_vcf.h): after bvc_pileup_finish_called_text and until the next bvc_pileup_begin* on the context it
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

#ifdef __cplusplus
}
#endif
#endif /* BVC_BGZF_H */
