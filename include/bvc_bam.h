/*
 * bvc_bam.h -- C ABI of libbvc, third header: phase 1 of `BaseVarC basetype` (the per-sample BAM pileup) on the device.
 * Everything of bvc.h (conventions, contexts, return codes) holds here; the entry point below is exported by the same library.  It has
 * a header of its own because bvc.h's list of entry points is closed: the binding's first table is checked against that list, name by
 * name and by their number (tests/test_binding_abi.py).
 */
#ifndef BVC_BAM_H
#define BVC_BAM_H

#include "bvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Additive: the stage in front of the temp batches.  The reference's bt_r (src/BaseVarC.cpp:444-530) reads, per sample of a batch, the
 * region's alignments (BamProcess::GetBRV, src/BamProcess.cpp:264-304), applies the per-position rule (FindSnpAtPos, :4-94) and writes
 * one temp-batch record per position.  This call does the same from the INFLATED alignment records of the batch's samples (what
 * bvc_inflate_blocks leaves of their BGZF blocks) and returns the batch's records in the binary temp-batch form of
 * bvc_pileup_begin_bin, byte for byte what the host program writes per position with `--tmp-format bin|raw`:
 *   record  = u32 payload bytes | entries          entry = u32 sample-in-batch | u8 base mapq qual rpr flags | [u16 n | n bytes of indel text]
 * one record per position, in position order, a record's entries in sample order.
 *
 *   bam, bam_bytes   the inflated record bytes of all samples
 *   sample_off, sample_end   [n_samples] each: sample s = bam[sample_off[s] .. sample_end[s]), starting AT a record's block_size word (any
 *                    byte address); the ranges lie one behind the other and may leave bytes between them (a file's header, the records in
 *                    front of the one the index names: a sample's blocks are inflated whole).  The kernels clamp a range into the buffer
 *                    whatever the arrays say
 *   sample_eof       [n_samples]: non-zero = the range ends at the file's end
 *   rid              [n_samples]: index of the region's reference in that BAM's header
 *   beg0, end0, min_mapq   BamFile::fetch's [beg, end) (0-based) and mapping-quality floor
 *   positions        [n_positions], 1-based, strictly ascending
 *   rg_s, refseq     the region's 1-based start and reference string (deletion tokens are cut from it: refseq[pos - rg_s + 1 ...])
 *   records          out: the records, *records_needed bytes.  records_cap: room in it
 *   rec_start        out: [n_positions + 1], the twin of bvc_pileup_begin_bin's: record t begins -- at its length word -- at rec_start[t];
 *                    rec_start[n_positions] = one past the last record
 *   sample_status    out: [n_samples], always written (below)
 *
 * The semantics are the host program's (host/bam.cpp: BamFile::fetch, find_snp_at_pos; host/pileup.cpp: bin_batch_entry), quirks included.
 * Record filter, in order: ref_id < 0 and ref_id < rid are skipped; the first record with ref_id > rid or pos >= end0 ends the sample for
 * good (no byte behind it is interpreted); unmapped reads, n_cigar == 0 (the 16-bit field only), end_pos <= beg0, duplicates and
 * mapq < min_mapq are skipped.  Per position: the first read that has not ended in front of it (sticking at the last read) -- if that one
 * does not cover it, nobody does; the indel token when the position is the last reference base of its operation and the next operation
 * is I or D of non-zero length (a pad next never gives one); on D or N at the position the next read, while it covers the position.  The
 * four CIGAR coordinates and the unsigned 32-bit query offset are those of host/bam.cpp.  A base entry: base 0..3, 4 for anything else,
 * rpr = (uint8_t)(offset + 1), strand = !(reverse || mate_reverse).  An indel entry: base 5, qual = the read's mapq, rpr 0, mapq = that of
 * the last base entry this sample produced earlier in the call (0: none); text "-" + the reference bases (clamped at refseq's end) or "+" +
 * the read's bases, at most 0xffff bytes.
 *
 * sample_status: 0 = entries may have been written; 1 = no read passed the filter (the caller prints the reference's "region is empty"
 * warning; not an error); 2 = the bytes ran out before a stop record and sample_eof is 0 (a clean end or a record cut short): supply
 * more; 3 = a malformed record in front of the stop (block_size < 32 or > 1 << 28, fields that do not fit their block, a record cut short
 * although sample_eof is set: read_record's `bad`); 4 = the rule's out-of-range cases (query offset past the sequence, empty sequence, an
 * insertion or deletion text that starts past its source: the host program throws std::out_of_range).
 *
 * Returns BVC_OK; BVC_BAM_MORE (positive, not an error) when some sample has status 2, or when records_cap < *records_needed -- the
 * caller retries with more bytes / the reported size; BVC_ERR_DATA when some sample has status 3 or 4 (bvc_last_error names the first);
 * BVC_ERR_ARG for null pointers with work present, negative sizes, host sample ranges that do not lie inside the buffer one behind the other,
 * host positions that do not strictly ascend, and *records_needed > 0xFFFFFF00 (rec_start is 32-bit like its twin).  Only BVC_OK writes
 * records and rec_start: every other return leaves both untouched.  *records_needed (a HOST pointer with either flag) is always set: the
 * size of the records, 0 when a sample has status 2, 3 or 4.
 *
 * BVC_PTR_HOST: synchronises the context's stream.  BVC_PTR_DEVICE: bam, sample_off, sample_end, sample_eof, rid, positions, refseq, records,
 * rec_start and sample_status are device memory and the kernels are asynchronous on the context's stream, apart from ONE wait in the middle
 * of the call -- for the size and the statuses, which decide the return value -- so the inputs must be complete on that stream when
 * the call is made.  Scratch lives in the context and grows on demand: the read table (16 + 4 bytes per 36 bytes of bam), a size matrix of
 * one tile of at most 1024 positions x n_samples, and O(n_positions + n_samples); a second call of the same shape allocates nothing.
 */
int bvc_bam_pileup(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                   const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                   int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                   uint8_t *records, int64_t records_cap, int64_t *records_needed, uint32_t *rec_start, uint32_t *sample_status,
                   uint32_t flags);
/*
 * The same from the samples' BGZF blocks, still compressed: what the host program's phase 1 calls per batch (BVC_HOST_DEVICE_PILEUP).
 * comp / blocks as bvc_inflate_blocks takes them (blocks[i].out_off: where the block's output lies among the bam_bytes inflated bytes,
 * which stay on the device; check_crc as there); sample_off / sample_end are offsets into those inflated bytes -- a sample's first block
 * is inflated whole, so sample_off[s] names the first record inside it -- and everything else is bvc_bam_pileup's.  Host pointers only
 * (comp best in bvc_host_alloc memory: it is the bulk and goes up by DMA); synchronises the context's stream.  A block that is not valid
 * deflate of its ISIZE bytes or fails its CRC32 is BVC_ERR_DATA (bvc_last_error names the first), whatever the kernels made of its
 * bytes; what records then holds is undefined.
 */
int bvc_bam_pileup_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                        int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                        int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                        const char *refseq, int64_t refseq_len, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                        uint32_t *rec_start, uint32_t *sample_status);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BAM_H */
