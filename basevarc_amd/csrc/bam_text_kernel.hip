// bam_text_kernel.hip -- phase 1 of `BaseVarC basetype` on the device for the TEXT temp batches: the inflated alignment records of a
// batch of samples -> the batch's lines as bt_r writes them (include/bvc_bam_text.h, bvc_bam_pileup_text).  A line is
// format_pileup_token (host/pileup.cpp) of every sample in sample order and "\n"; the read table, resolve() and the scan are those of
// bam_pileup_kernel.hip (launch_bam_index, launch_bam_scan) and the plan is the same: sizes into the tile's matrix [position][sample],
// row sums, one scan to line_start, then the bytes.
//
//   bam_text_token_kernel   one wavefront per sample, one position a lane, a tile's chunks of 64 positions spread over blockIdx.y (no
//                           carry runs through them: a text indel token shows no fields).  SIZE: the token's byte size into the
//                           matrix -- 2 for ". ", 7 + the digits of mapq, qual and rpr for a base token, the whole text + 1 for an
//                           indel token.  PLACE: the same resolution again and the token written at the line's start + the row's
//                           exclusive prefix; a sample without an entry writes nothing here.
//   bam_text_rows_kernel    one wavefront per position of the tile, lanes along samples.  SIZE: the row's sum + the newline.  PLACE: the
//                           row becomes its exclusive prefix, every cell of size 2 gets its ". " (nine cells in ten at the coverage this
//                           is for: neighbouring lanes write neighbouring bytes, where the per-sample pass would write 2 bytes at a
//                           stride of a whole line) and the line its "\n".  The one real token of 2 bytes, "- " (a deletion cut at
//                           refseq's end), is written over its filler by the token pass, which runs behind this one on the stream.
// Nothing is placed by an atomic cursor: every byte's address is a function of the input alone.  Decimal digits are computed, never
// looked up in a lane's own array.
#include "bam_resolve_device.h"

namespace bvc {

namespace {

__device__ __forceinline__ uint32_t dec_len(uint32_t v) { return v >= 100u ? 3u : v >= 10u ? 2u : 1u; }   // v < 1000

// v < 1000 in decimal and `sep` behind it; returns the byte behind sep
__device__ __forceinline__ uint8_t *put_dec(uint8_t *__restrict__ p, uint32_t v, uint8_t sep)
{
    const uint32_t h = v / 100u, r = v - h * 100u, t = r / 10u;
    if (v >= 100u) *p++ = (uint8_t)('0' + h);
    if (v >= 10u) *p++ = (uint8_t)('0' + t);
    *p++ = (uint8_t)('0' + (r - t * 10u));
    *p++ = sep;
    return p;
}

// bytes of format_pileup_token for what resolve() found
__device__ __forceinline__ uint32_t token_size(const Hit &h)
{
    if (h.size == 0u) return 2u;
    if (h.flags & 2u) return h.text_full + 1u;
    return 7u + dec_len((h.fields >> 8) & 0xFFu) + dec_len((h.fields >> 16) & 0xFFu) + dec_len(h.fields >> 24);
}

}  // namespace

// positions / line_start: the tile's; cell: [tile_n][n_samples], sizes (SIZE, written) or exclusive row prefixes (PLACE, read).
template <bool PLACE>
__global__ __launch_bounds__(kBamThreads) void bam_text_token_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax, const uint32_t *__restrict__ n_reads,
    const int32_t *__restrict__ positions, int32_t tile_n, int32_t rg_s, const uint8_t *__restrict__ refseq, int64_t refseq_len,
    uint32_t *__restrict__ cell, uint32_t *__restrict__ sample_status, const uint32_t *__restrict__ line_start, uint8_t *__restrict__ text)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    const int64_t slot0 = uniform64(lo) / kBamMinRecord;
    const uint32_t n = uniform(n_reads[s]);
    if (PLACE && n == 0u) return;                   // all filler: the row pass wrote it
    for (int32_t t0 = (int32_t)blockIdx.y * kWave; t0 < tile_n; t0 += (int32_t)gridDim.y * kWave) {
        const int32_t t = t0 + lane;
        if (t >= tile_n) continue;
        Hit h;
        if (n > 0u) h = resolve(bam, reads + slot0, runmax + slot0, n, positions[t], rg_s, refseq_len);
        if (!PLACE) {
            cell[(int64_t)t * n_samples + s] = token_size(h);
            if (h.out_of_range) sample_status[s] = 4u;
            continue;
        }
        if (h.size == 0u) continue;
        uint8_t *dst = text + (int64_t)line_start[t] + (int64_t)cell[(int64_t)t * n_samples + s];
        if (!(h.flags & 2u)) {                      // "%u,%u,%u,%u,%u " of base, mapq, qual, rpr, strand
            dst = put_dec(dst, h.fields & 0xFFu, ',');
            dst = put_dec(dst, (h.fields >> 8) & 0xFFu, ',');
            dst = put_dec(dst, (h.fields >> 16) & 0xFFu, ',');
            dst = put_dec(dst, h.fields >> 24, ',');
            put_dec(dst, h.flags & 1u, ' ');
            continue;
        }
        const uint32_t len = h.text_full;           // the sign included; whole, whatever the binary entry's length field holds
        dst[0] = h.deletion ? '-' : '+';
        if (h.deletion) {
            for (uint32_t i = 1; i < len; ++i) dst[i] = refseq[h.text_src + (i - 1u)];
        } else {
            for (uint32_t i = 1; i < len; ++i) {
                const uint32_t at = h.text_at + (i - 1u);
                dst[i] = nt16_char((bam[h.text_src + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 15u);
            }
        }
        dst[len] = ' ';
    }
}

// One wavefront per position of the tile.  SIZE: rec_len[t] = the line's bytes (the row's sum + 1) LESS the 4 that bam_scan_kernel adds
// to every position for the binary record's length word -- unsigned arithmetic, so a line of 1 byte is right too.  PLACE: the row becomes
// its exclusive prefix (every prefix fits 32 bits: the call's text does), the filler and the newline are written.
template <bool PLACE>
__global__ __launch_bounds__(kBamThreads) void bam_text_rows_kernel(int32_t tile_n, int32_t n_samples, uint32_t *__restrict__ cell,
                                                                    uint64_t *__restrict__ rec_len, const uint32_t *__restrict__ line_start,
                                                                    uint8_t *__restrict__ text)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t t = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (t >= tile_n) return;
    uint32_t *const row = cell + (int64_t)t * n_samples;
    if (!PLACE) {
        uint64_t sum = 0;
        for (int32_t s = lane; s < n_samples; s += kWave) sum += row[s];
        for (int d = kWave / 2; d > 0; d >>= 1) sum += from_lane64(sum, lane + d);   // (lane 0's sum takes in lanes 0..63 only)
        if (lane == 0) rec_len[t] = sum + 1u - 4u;
        return;
    }
    uint8_t *const line = text + (int64_t)line_start[t];
    uint32_t run = 0;
    for (int32_t s0 = 0; s0 < n_samples; s0 += kWave) {
        const int32_t s = s0 + lane;
        const uint32_t v = s < n_samples ? row[s] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t x = from_lane(incl, lane - d);
            if (lane >= d) incl += x;
        }
        const uint32_t at = run + incl - v;
        if (s < n_samples) row[s] = at;
        if (v == 2u) { line[at] = '.'; line[at + 1u] = ' '; }
        run += from_lane(incl, kWave - 1);
    }
    if (lane == 0) line[run] = '\n';
}

hipError_t launch_bam_text_tile(hipStream_t stream, bool place, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                                const int64_t *sample_end, const int32_t *positions, int32_t t0, int32_t tile_n, int32_t rg_s, const uint8_t *refseq,
                                int64_t refseq_len, const BamPileupScratch &s, uint32_t *sample_status, uint8_t *text)
{
    if (tile_n <= 0) return hipSuccess;
    const dim3 rows((unsigned)((tile_n + kBamWaves - 1) / kBamWaves)),
        chunks((unsigned)((n_samples + kBamWaves - 1) / kBamWaves), (unsigned)((tile_n + kWave - 1) / kWave));
    // the sizes first, in both passes: the matrix is the tile's, not the call's
    if (n_samples > 0)
        hipLaunchKernelGGL(bam_text_token_kernel<false>, chunks, dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off, sample_end, s.reads,
                           s.runmax, s.n_reads, positions + t0, tile_n, rg_s, refseq, refseq_len, s.cell, sample_status, s.rec_start + t0, text);
    if (!place) {
        hipLaunchKernelGGL(bam_text_rows_kernel<false>, rows, dim3(kBamThreads), 0, stream, tile_n, n_samples, s.cell, s.rec_len + t0, s.rec_start + t0, text);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(bam_text_rows_kernel<true>, rows, dim3(kBamThreads), 0, stream, tile_n, n_samples, s.cell, s.rec_len + t0, s.rec_start + t0, text);
    if (n_samples > 0)
        hipLaunchKernelGGL(bam_text_token_kernel<true>, chunks, dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off, sample_end, s.reads,
                           s.runmax, s.n_reads, positions + t0, tile_n, rg_s, refseq, refseq_len, s.cell, sample_status, s.rec_start + t0, text);
    return hipGetLastError();
}

}  // namespace bvc
