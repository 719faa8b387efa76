// bam_popmatrix_kernel.hip -- `BaseVarC popmatrix` on the device: the inflated alignment records of a batch of samples and a list of
// (position, REF, ALT) -> one row of '0' / '1' / '.' per sample (include/bvc_popmatrix.h, bvc_bam_popmatrix).  What has to come out is
// fixed by BamFile::fetch + fetch_allele_type (host/bam.cpp), the reference's BamProcess::FetchAlleleType; for positions that do not
// descend that is find_snp_at_pos's walk with another ending, so the read table (bam_index_kernel) and resolve() (bam_resolve_device.h)
// are bam_pileup_kernel.hip's.
//
//   bam_popmatrix_kernel   one wavefront per sample, one position a lane: resolve() once, the character of the read's base against the
//                          position's REF and ALT characters, one byte stored at matrix[s * row_stride + t] -- 64 consecutive bytes a
//                          wavefront a step.  No size matrix, no second pass, no scan of a row: the output is sample-major.
// The statuses' scan is bam_scan_kernel with no positions.  The reference's text never reaches this kernel: only refseq_len and rg_s
// decide whether a deletion's text starts inside it.
#include "bam_resolve_device.h"

namespace bvc {

__global__ __launch_bounds__(kBamThreads) void bam_popmatrix_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax, const uint32_t *__restrict__ n_reads,
    int32_t n_positions, const int32_t *__restrict__ positions, const uint8_t *__restrict__ ref, const uint8_t *__restrict__ alt, int32_t rg_s,
    int64_t refseq_len, uint8_t *__restrict__ matrix, int64_t row_stride, uint32_t *__restrict__ sample_status)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    const int64_t slot0 = uniform64(lo) / kBamMinRecord;
    const uint32_t n = uniform(n_reads[s]);         // 0: no kept read (status 1), or a status that leaves the row unspecified: dots
    uint8_t *const row = matrix + (int64_t)s * row_stride;
    for (int64_t t0 = (int64_t)blockIdx.y * kWave; t0 < n_positions; t0 += (int64_t)gridDim.y * kWave) {
        const int64_t t = t0 + lane;
        if (t >= n_positions) continue;
        uint8_t out = '.';
        if (n > 0u) {
            const Hit h = resolve<true>(bam, reads + slot0, runmax + slot0, n, positions[t], rg_s, refseq_len);
            if (h.out_of_range) sample_status[s] = 4u;
            else if (h.size == 9u) {                // a base of a read: its character, not its 0..4 class (REF 'N' matches a read's N)
                const uint8_t c = nt16_char(h.nib);
                out = c == ref[t] ? '0' : c == alt[t] ? '1' : '.';
            }
        }
        row[t] = out;
    }
}

BamPileupScratch bam_popmatrix_scratch(Layout &L, int64_t bam_bytes, int32_t n_samples)
{
    BamPileupScratch s;                             // the read table, the counts and the scan's two outputs: nothing per position
    const size_t cap = (size_t)(bam_bytes / kBamMinRecord) + 1;
    s.reads = L.take<BamRead>(cap);
    s.runmax = L.take<int32_t>(cap);
    s.n_reads = L.take<uint32_t>((size_t)n_samples);
    s.rec_start = L.take<uint32_t>(1);
    s.head = L.take<int64_t>(4);
    return s;
}

hipError_t launch_bam_popmatrix(hipStream_t stream, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                                const int64_t *sample_end, int32_t n_positions, const int32_t *positions, const uint8_t *ref, const uint8_t *alt,
                                int32_t rg_s, int64_t refseq_len, const BamPileupScratch &s, uint8_t *matrix, int64_t row_stride, uint32_t *sample_status)
{
    if (n_samples <= 0 || n_positions <= 0) return hipSuccess;
    hipLaunchKernelGGL(bam_popmatrix_kernel, bam_sample_grid(n_samples, n_positions), dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off,
                       sample_end, s.reads, s.runmax, s.n_reads, n_positions, positions, ref, alt, rg_s, refseq_len, matrix, row_stride, sample_status);
    return hipGetLastError();
}

}  // namespace bvc
