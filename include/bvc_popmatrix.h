/*
 * bvc_popmatrix.h -- C ABI of libbvc, fourth header: `BaseVarC popmatrix` (the population matrix's rows) on the device.
 * Everything of bvc.h (conventions, contexts, return codes) holds here; the entry points below are exported by the same library.  They
 * have a header of their own because bvc.h's list of entry points is closed and bvc_bam.h is held to its own table
 * (tests/test_binding_abi.py, tests/test_bam_pileup_abi.py).
 */
#ifndef BVC_POPMATRIX_H
#define BVC_POPMATRIX_H

#include "bvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Additive.  The reference's runPopMatrix (src/BaseVarC.cpp:671-729) calls BamProcess::FetchAlleleType (src/BamProcess.cpp:96-198) once
 * per BAM: the region's alignments (GetBRV), then per line of the position file one character -- '0' when the first usable read's base
 * is the line's REF character, '1' when it is the ALT character, '.' otherwise (no coverage, an indel token, another base).  This call
 * does the same for a batch of samples from their INFLATED alignment records and writes one row of n_positions characters per sample.
 *
 *   bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq
 *                    bvc_bam_pileup's (bvc_bam.h), word for word: the samples' byte ranges, the record filter and its order
 *   positions        [n_positions], 1-based, NOT DESCENDING; a position may repeat (a multi-allelic site is two lines of a position file)
 *   ref, alt         [n_positions] each: the line's REF and ALT characters, compared as they are with the read's base character out of
 *                    "=ACMGRSVTWYHKDBN" (a REF of 'N' matches a read's N; a lowercase character matches nothing; REF is tried first)
 *   rg_s, refseq_len the region's 1-based start and the length of its reference string: the string itself is never read, but a deletion
 *                    whose text would start past it is one of the out-of-range cases below
 *   matrix           out: n_samples rows, row_stride >= n_positions bytes apart; row s = matrix[s * row_stride ...], n_positions characters
 *   sample_status    out: [n_samples], written by every call that gets past its argument checks
 *
 * Per position the rule is bvc_bam_pileup's (the first read that has not ended in front of the position; the indel token; the next read
 * on D or N), which for positions that do not descend is what FetchAlleleType's stateful loop computes (host/bam.cpp,
 * fetch_allele_type; tests/test_popmatrix_model.py).  For a list that descends the two differ: host positions that descend are refused.
 *
 * sample_status: bvc_bam_pileup's 0..4 -- 0 = a row from at least one read; 1 = no read passed the filter: a row of '.' (not an error);
 * 2 = the bytes ran out before a stop record and sample_eof is 0: supply more; 3 = a malformed record in front of the stop; 4 = the
 * rule's out-of-range cases (query offset past the sequence, empty sequence, an insertion or deletion text that starts past its source:
 * the reference builds the token before it discards it, so it throws there too).
 *
 * Returns BVC_OK; BVC_BAM_MORE (positive, not an error) when some sample has status 2; BVC_ERR_DATA when some sample has status 3 or 4
 * (bvc_last_error names the first); BVC_ERR_ARG for null pointers with work present, negative sizes, row_stride < n_positions, host
 * sample ranges that do not lie inside the buffer one behind the other and host positions that descend.  Rows of samples with status 0
 * or 1 are defined whatever the return value; rows of samples with status 2, 3 or 4 are unspecified.  Nothing outside
 * matrix[0 .. n_samples * row_stride) is ever written, and bytes n_positions .. row_stride of a row are never written.
 *
 * BVC_PTR_HOST: synchronises the context's stream.  BVC_PTR_DEVICE: bam, sample_off, sample_end, sample_eof, rid, positions, ref, alt,
 * matrix and sample_status are device memory (positions are not checked) and the call is asynchronous on the context's stream apart
 * from ONE wait at its end, which reads the statuses that decide the return value.  Scratch lives in the context and grows on demand:
 * the read table (16 + 4 bytes per 36 bytes of bam) and O(n_samples); a second call of the same shape allocates nothing.
 */
int bvc_bam_popmatrix(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                      const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                      int32_t n_positions, const int32_t *positions, const uint8_t *ref, const uint8_t *alt, int32_t rg_s, int64_t refseq_len,
                      uint8_t *matrix, int64_t row_stride, uint32_t *sample_status, uint32_t flags);
/*
 * The same from the samples' BGZF blocks, still compressed: what the host program's popmatrix calls per batch
 * (BVC_HOST_DEVICE_POPMATRIX).  comp / blocks / bam_bytes as bvc_bam_pileup_bgzf takes them (blocks[i].out_off: where the block's output
 * lies among the bam_bytes inflated bytes, which stay on the device; the CRC32 is checked where the block asks for it); sample_off /
 * sample_end are offsets into those inflated bytes; everything else is bvc_bam_popmatrix's.  Host pointers only; synchronises the
 * context's stream.  A block that is not valid deflate of its ISIZE bytes or fails its CRC32 is BVC_ERR_DATA (bvc_last_error names the
 * first), whatever the kernels made of its bytes.
 */
int bvc_bam_popmatrix_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                           int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                           int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, const uint8_t *ref,
                           const uint8_t *alt, int32_t rg_s, int64_t refseq_len, uint8_t *matrix, int64_t row_stride, uint32_t *sample_status);

#ifdef __cplusplus
}
#endif
#endif /* BVC_POPMATRIX_H */
