// bam_pileup_kernel.hip -- phase 1 of `BaseVarC basetype` on the device: the inflated alignment records of a batch of samples -> the
// batch's position records in the binary temp-batch form (include/bvc_bam.h, bvc_bam_pileup).  What has to come out is fixed by
// BamFile::fetch + find_snp_at_pos + bin_batch_entry (host/bam.cpp, host/pileup.cpp); how it is computed is different.
//
//   bam_index_kernel     one wavefront per sample.  The block_size chain is a dependent chain: every lane walks the same 64 records
//                        (one address for the wavefront), lane i keeps record i.  The field checks, the filter and end_pos then run one
//                        record a lane; a ballot finds the first stop / malformed record, the kept reads go -- compacted, in order -- to
//                        the sample's slice of the read table with the running maximum of their end_pos (an inclusive max scan).
//   bam_pileup_kernel    one wavefront per sample, one position a lane.  first(pos) of the rule is "the first read whose running maximum
//                        of end_pos reaches pos, else the last read": a binary search of that monotone column.  The lane then rescans its
//                        read's CIGAR from the record's bytes (no per-read tables: n_cigar goes up to 65535) in the rule's four coordinates
//                        and falls through to the next read on D / N.  SIZE pass: the entry's byte size into the tile's size matrix
//                        [position][sample].  PLACE pass: the same resolution again, and the entry written at the record's start + 4 + the
//                        row's exclusive prefix; the mapq an indel entry shows (the last base entry's of this sample) is a lane scan with a
//                        per-sample carry across chunks and tiles.
//   bam_rows_kernel      one wavefront per position of the tile: the row's sum (SIZE), or its exclusive prefix in place and the record's
//                        length word (PLACE).
//   bam_scan_kernel      one wavefront: rec_start = exclusive scan of 4 + row sum over all positions, the total, and the first sample of
//                        each failing status.
// Nothing is placed by an atomic cursor: every byte's address is a function of the input alone.
//
// resolve() and the byte / lane helpers live in bam_resolve_device.h, which bam_popmatrix_kernel.hip shares.
//
// Untrusted input: the chain walk bounds every record by the sample's range, the field check bounds CIGAR, bases and qualities by the
// record, and the pileup pass only reads records that passed both.  Records lie at any byte address: every field is built from bytes.
#include "bam_resolve_device.h"

namespace bvc {

namespace {

constexpr uint32_t kBamMaxRecord = 1u << 28;        // read_record's kMaxRecord
constexpr int32_t kNoEnd = -2147483647 - 1;

__device__ __forceinline__ void st16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ __forceinline__ void st32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

}  // namespace

__global__ __launch_bounds__(kBamThreads) void bam_index_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const uint8_t *__restrict__ sample_eof, const int32_t *__restrict__ rid, int32_t beg0, int32_t end0, int32_t min_mapq,
    BamRead *__restrict__ reads, int32_t *__restrict__ runmax, uint32_t *__restrict__ n_reads, uint32_t *__restrict__ sample_status)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    lo = uniform64(lo); hi = uniform64(hi);
    const int32_t want = rid[s];
    const bool eof = sample_eof[s] != 0;
    const int64_t slot0 = lo / kBamMinRecord;
    int64_t cur = lo;
    uint32_t kept = 0, status = 0;
    int32_t mx = kNoEnd;
    for (bool done = false; !done;) {
        // the chain: 64 records, walked by every lane alike; tail: 0 = all 64 are there, 1 = the bytes end cleanly, 2 = they end
        // inside a record, 3 = a block_size read_record refuses
        int64_t mine = 0;
        uint32_t my_bs = 0;
        int n = 0, tail = 0;
        for (int i = 0; i < kWave; ++i) {
            const int64_t left = hi - cur;
            if (left == 0) { tail = 1; break; }
            if (left < 4) { tail = 2; break; }
            const uint32_t bs = uniform(ld32(bam, cur));
            if (bs < 32u || bs > kBamMaxRecord) { tail = 3; break; }
            if (left - 4 < (int64_t)bs) { tail = 2; break; }
            if (lane == i) { mine = cur; my_bs = bs; }
            cur += 4 + (int64_t)bs;
            n = i + 1;
        }
        int cls = 0;                                // 0 skip, 1 keep, 2 stop, 3 malformed
        int32_t rpos = 0, rend = 0;
        if (lane < n) {
            const int64_t q = mine + 4;
            const int32_t ref_id = (int32_t)ld32(bam, q), pos = (int32_t)ld32(bam, q + 4);
            const uint32_t l_rn = bam[q + 8], mapq = bam[q + 9], n_cig = ld16(bam, q + 12), flag = ld16(bam, q + 14);
            const int32_t l_seq = (int32_t)ld32(bam, q + 16);
            if (l_seq < 0 || 32 + (int64_t)l_rn + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq > (int64_t)my_bs) cls = 3;
            else if (ref_id < 0 || ref_id < want) cls = 0;
            else if (ref_id > want || pos >= end0) cls = 2;
            else if ((flag & 0x4u) || n_cig == 0u) cls = 0;
            else {
                uint32_t e = (uint32_t)pos;
                const int64_t c0 = q + 32 + l_rn;
                for (uint32_t k = 0; k < n_cig; ++k) {
                    const uint32_t c = ld32(bam, c0 + 4 * (int64_t)k), op = cigar_op(c);
                    if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) e += c >> 4;
                }
                rpos = pos; rend = (int32_t)e;
                cls = (rend <= beg0 || (flag & 0x400u) || (int32_t)mapq < min_mapq) ? 0 : 1;
            }
        }
        const uint64_t stops = __ballot(cls >= 2);
        const int term = stops ? __ffsll((unsigned long long)stops) - 1 : kWave;
        const bool keep = cls == 1 && lane < term;
        const uint64_t keeps = __ballot(keep);
        int32_t v = keep ? rend : kNoEnd;           // running maximum of end_pos over the kept reads, in order
        for (int d = 1; d < kWave; d <<= 1) {
            const int32_t t = (int32_t)from_lane((uint32_t)v, lane - d);
            if (lane >= d && t > v) v = t;
        }
        if (mx > v) v = mx;
        if (keep) {
            const int64_t at = slot0 + kept + (uint32_t)__popcll(keeps & ((1ull << lane) - 1ull));
            reads[at] = BamRead{mine, rpos, rend};
            runmax[at] = v;
        }
        mx = (int32_t)from_lane((uint32_t)v, kWave - 1);
        kept += (uint32_t)__popcll(keeps);
        if (term < kWave) {
            status = from_lane((uint32_t)cls, term) == 3u ? 3u : 0u;
            done = true;
        } else if (tail != 0) {
            status = tail == 1 ? (eof ? 0u : 2u) : tail == 2 ? (eof ? 3u : 2u) : 3u;
            done = true;
        }
    }
    if (status == 0u && kept == 0u) status = 1u;
    if (lane == 0) {
        sample_status[s] = status;
        n_reads[s] = status >= 2u ? 0u : kept;
    }
}

// positions / rec_start: the tile's; cell: [tile_n][n_samples].  PLACE: one block row (the carry runs through the chunks in order).
template <bool PLACE>
__global__ __launch_bounds__(kBamThreads) void bam_pileup_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax, const uint32_t *__restrict__ n_reads,
    const int32_t *__restrict__ positions, int32_t tile_n, int32_t rg_s, const uint8_t *__restrict__ refseq, int64_t refseq_len,
    uint32_t *__restrict__ cell, uint32_t *__restrict__ sample_status, const uint32_t *__restrict__ rec_start, uint8_t *__restrict__ records,
    uint8_t *__restrict__ carry)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    const int64_t slot0 = uniform64(lo) / kBamMinRecord;
    const uint32_t n = uniform(n_reads[s]);
    uint32_t last_mapq = PLACE ? uniform(carry[s]) : 0u;
    for (int32_t t0 = (int32_t)blockIdx.y * kWave; t0 < tile_n; t0 += (int32_t)gridDim.y * kWave) {
        const int32_t t = t0 + lane;
        Hit h;
        if (t < tile_n && n > 0u) h = resolve(bam, reads + slot0, runmax + slot0, n, positions[t], rg_s, refseq_len);
        if (!PLACE) {
            if (t < tile_n) cell[(int64_t)t * n_samples + s] = h.size;
            if (h.out_of_range) sample_status[s] = 4u;
            continue;
        }
        // an indel entry shows the mapq of the last base entry this sample produced before it
        const bool is_base = h.size == 9u;
        const uint64_t bases = __ballot(is_base);
        const uint64_t below = bases & ((1ull << lane) - 1ull);
        const uint32_t m = from_lane((h.fields >> 8) & 0xFFu, below ? 63 - __clzll((long long)below) : 0);
        const uint32_t shown = below ? m : last_mapq;
        if (bases) last_mapq = uniform(from_lane((h.fields >> 8) & 0xFFu, 63 - __clzll((long long)bases)));
        if (h.size == 0u) continue;
        uint8_t *dst = records + (int64_t)rec_start[t] + 4 + (int64_t)cell[(int64_t)t * n_samples + s];
        st32(dst, (uint32_t)s);
        dst[4] = (uint8_t)h.fields;
        dst[5] = (uint8_t)(is_base ? h.fields >> 8 : shown);
        dst[6] = (uint8_t)(h.fields >> 16);
        dst[7] = (uint8_t)(h.fields >> 24);
        dst[8] = (uint8_t)h.flags;
        if (is_base) continue;
        st16(dst + 9, h.text_len);
        dst[11] = h.deletion ? '-' : '+';
        if (h.deletion) {
            for (uint32_t i = 1; i < h.text_len; ++i) dst[11 + i] = refseq[h.text_src + (i - 1u)];
        } else {
            for (uint32_t i = 1; i < h.text_len; ++i) {
                const uint32_t at = h.text_at + (i - 1u);
                const uint32_t nib = (bam[h.text_src + (at >> 1)] >> ((at & 1u) ? 0 : 4)) & 15u;
                dst[11 + i] = nt16_char(nib);
            }
        }
    }
    if (PLACE && lane == 0) carry[s] = (uint8_t)last_mapq;
}

// One wavefront per position of the tile.  SIZE: rec_len[t] = the row's sum.  PLACE: the row becomes its exclusive prefix (every
// prefix fits 32 bits: the call's records do) and the record's length word is written.
template <bool PLACE>
__global__ __launch_bounds__(kBamThreads) void bam_rows_kernel(int32_t tile_n, int32_t n_samples, uint32_t *__restrict__ cell,
                                                               uint64_t *__restrict__ rec_len, const uint32_t *__restrict__ rec_start,
                                                               uint8_t *__restrict__ records)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t t = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (t >= tile_n) return;
    uint32_t *const row = cell + (int64_t)t * n_samples;
    if (!PLACE) {
        uint64_t sum = 0;
        for (int32_t s = lane; s < n_samples; s += kWave) sum += row[s];
        for (int d = kWave / 2; d > 0; d >>= 1) sum += from_lane64(sum, lane + d);   // (lane 0's sum takes in lanes 0..63 only)
        if (lane == 0) rec_len[t] = sum;
        return;
    }
    uint32_t run = 0;
    for (int32_t s0 = 0; s0 < n_samples; s0 += kWave) {
        const int32_t s = s0 + lane;
        const uint32_t v = s < n_samples ? row[s] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t x = from_lane(incl, lane - d);
            if (lane >= d) incl += x;
        }
        if (s < n_samples) row[s] = run + incl - v;
        run += from_lane(incl, kWave - 1);
    }
    if (lane == 0) st32(records + rec_start[t], run);
}

// One wavefront: rec_start [n_positions + 1] (the low 32 bits: a call whose total does not fit them is refused), head[0] = the total,
// head[1..3] = the first sample of status 2, 3, 4 (0x7FFFFFFF: none).
__global__ __launch_bounds__(kWave) void bam_scan_kernel(int32_t n_positions, const uint64_t *__restrict__ rec_len, uint32_t *__restrict__ rec_start,
                                                         int32_t n_samples, const uint32_t *__restrict__ sample_status, int64_t *__restrict__ head)
{
    const int lane = threadIdx.x;
    uint64_t run = 0;
    for (int32_t t0 = 0; t0 < n_positions; t0 += kWave) {
        const int32_t t = t0 + lane;
        const uint64_t v = t < n_positions ? rec_len[t] + 4u : 0u;
        uint64_t incl = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint64_t x = from_lane64(incl, lane - d);
            if (lane >= d) incl += x;
        }
        if (t < n_positions) rec_start[t] = (uint32_t)(run + incl - v);
        run += from_lane64(incl, kWave - 1);
    }
    int32_t first[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF};
    for (int32_t s0 = 0; s0 < n_samples; s0 += kWave) {
        const int32_t s = s0 + lane;
        const uint32_t st = s < n_samples ? sample_status[s] : 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint64_t m = __ballot(st == (uint32_t)(k + 2));
            if (m && first[k] == 0x7FFFFFFF) first[k] = s0 + __ffsll((unsigned long long)m) - 1;
        }
    }
    if (lane == 0) {
        rec_start[n_positions] = (uint32_t)run;
        head[0] = (int64_t)run;
        head[1] = first[0]; head[2] = first[1]; head[3] = first[2];
    }
}

BamPileupScratch bam_pileup_scratch(Layout &L, int64_t bam_bytes, int32_t n_samples, int32_t n_positions)
{
    BamPileupScratch s;
    const size_t cap = (size_t)(bam_bytes / kBamMinRecord) + 1, ns = (size_t)n_samples, np = (size_t)n_positions;
    s.tile = bam_pileup_tile(n_samples);
    s.reads = L.take<BamRead>(cap);
    s.runmax = L.take<int32_t>(cap);
    s.n_reads = L.take<uint32_t>(ns);
    s.carry = L.take<uint8_t>(ns);
    s.cell = L.take<uint32_t>((size_t)s.tile * ns);
    s.rec_len = L.take<uint64_t>(np);
    s.rec_start = L.take<uint32_t>(np + 1);
    s.head = L.take<int64_t>(4);
    return s;
}

hipError_t launch_bam_index(hipStream_t stream, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                            const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                            const BamPileupScratch &s, uint32_t *sample_status)
{
    if (n_samples <= 0) return hipSuccess;
    hipLaunchKernelGGL(bam_index_kernel, dim3((unsigned)((n_samples + kBamWaves - 1) / kBamWaves)), dim3(kBamThreads), 0, stream, n_samples, bam,
                       bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, s.reads, s.runmax, s.n_reads, sample_status);
    return hipGetLastError();
}

hipError_t launch_bam_tile(hipStream_t stream, bool place, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                           const int64_t *sample_end, const int32_t *positions, int32_t t0, int32_t tile_n, int32_t rg_s, const uint8_t *refseq, int64_t refseq_len,
                           const BamPileupScratch &s, uint32_t *sample_status, uint8_t *records)
{
    if (tile_n <= 0) return hipSuccess;
    const dim3 rows((unsigned)((tile_n + kBamWaves - 1) / kBamWaves)), samples((unsigned)((n_samples + kBamWaves - 1) / kBamWaves)),
        chunks(samples.x, (unsigned)((tile_n + kWave - 1) / kWave));
    // the sizes first, in both passes: the matrix is the tile's, not the call's
    if (n_samples > 0)
        hipLaunchKernelGGL(bam_pileup_kernel<false>, chunks, dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off, sample_end, s.reads,
                           s.runmax, s.n_reads, positions + t0, tile_n, rg_s, refseq, refseq_len, s.cell, sample_status, s.rec_start + t0, records, s.carry);
    if (!place) {
        hipLaunchKernelGGL(bam_rows_kernel<false>, rows, dim3(kBamThreads), 0, stream, tile_n, n_samples, s.cell, s.rec_len + t0, s.rec_start + t0,
                           records);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(bam_rows_kernel<true>, rows, dim3(kBamThreads), 0, stream, tile_n, n_samples, s.cell, s.rec_len + t0, s.rec_start + t0, records);
    if (n_samples > 0)
        hipLaunchKernelGGL(bam_pileup_kernel<true>, samples, dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off, sample_end, s.reads,
                           s.runmax, s.n_reads, positions + t0, tile_n, rg_s, refseq, refseq_len, s.cell, sample_status, s.rec_start + t0, records, s.carry);
    return hipGetLastError();
}

hipError_t launch_bam_scan(hipStream_t stream, int32_t n_positions, int32_t n_samples, const BamPileupScratch &s, const uint32_t *sample_status)
{
    hipLaunchKernelGGL(bam_scan_kernel, dim3(1), dim3(kWave), 0, stream, n_positions, s.rec_len, s.rec_start, n_samples, sample_status, s.head);
    return hipGetLastError();
}

static_assert(sizeof(BamRead) == 16, "one 16-byte store a kept read");

}  // namespace bvc
