// bam_group_depth_kernel.hip -- the add pass of bvc_bam_counts_depth (include/bvc_bam_group_depth.h): the inflated alignment records of a batch
// of samples -> ONE slot of class counts [position][512], tally [position] and the groups' depths per base [position][group][4].  Shaped
// like bam_counts_kernel<true> (bam_counts_kernel.hip) with slots = 1: the read table (bam_index_kernel), resolve() (bam_resolve_device.h)
// and the per-cell rule are that kernel's word for word; the dry pass in front of it is bam_counts_kernel<false> itself.
//
//   bam_counts_depth_kernel   one wavefront per sample, one position a lane: resolve<false>() once, the tally add, the class-count add for
//                             a base 0..3 of quality 0..127, and under the same condition one add into the depth of the sample's group --
//                             none for a label >= n_groups.
// No LDS: every lane adds into another position's rows.  The adds are 32-bit integer atomics on global memory that return nothing; several
// launches (of several contexts) may add into the same arrays at once.
#include "bam_resolve_device.h"
#include "../../include/bvc_bam_group_depth.h"

namespace bvc {

__global__ __launch_bounds__(kBamThreads) void bam_counts_depth_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax, const uint32_t *__restrict__ n_reads,
    int32_t n_positions, const int32_t *__restrict__ positions, int32_t rg_s, int64_t refseq_len, const uint8_t *__restrict__ group_of_sample,
    int32_t n_groups, uint32_t *__restrict__ counts, uint32_t *__restrict__ tally, uint32_t *__restrict__ group_depth)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    const uint32_t n = uniform(n_reads[s]);         // 0: no kept read (status 1)
    if (n == 0u) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    const int64_t slot0 = uniform64(lo) / kBamMinRecord;
    const uint32_t g = uniform(group_of_sample[s]);
    const bool grouped = g < (uint32_t)n_groups;    // (the program's 255: in no group)
    for (int64_t t0 = (int64_t)blockIdx.y * kWave; t0 < n_positions; t0 += (int64_t)gridDim.y * kWave) {
        const int64_t t = t0 + lane;
        if (t >= n_positions) continue;
        const Hit h = resolve<false>(bam, reads + slot0, runmax + slot0, n, positions[t], rg_s, refseq_len);
        if (h.out_of_range || h.size == 0u) continue;
        uint32_t *const tw = tally + t * (int64_t)(sizeof(bvc_bam_site_tally) / 4);
        if (h.flags & 2u) { atomicAdd(tw + 9, 1u); continue; }          // an indel entry
        const uint32_t base = h.fields & 0xFFu, qual = (h.fields >> 16) & 0xFFu;
        if (base > 3u) { atomicAdd(tw + 8, 1u); continue; }             // class 4
        atomicAdd(tw + (((h.flags & 1u) << 2) | base), 1u);
        if (qual < 128u) {
            atomicAdd(counts + t * 512 + base * 128u + qual, 1u);
            if (grouped) atomicAdd(group_depth + ((t * n_groups + g) * 4 + base), 1u);
        }
    }
}

hipError_t launch_bam_counts_depth(hipStream_t stream, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                                   const int64_t *sample_end, int32_t n_positions, const int32_t *positions, int32_t rg_s, int64_t refseq_len,
                                   const uint8_t *group_of_sample, int32_t n_groups, const BamPileupScratch &s, uint32_t *counts,
                                   bvc_bam_site_tally *tally, uint32_t *group_depth)
{
    if (n_samples <= 0 || n_positions <= 0) return hipSuccess;
    const int64_t chunks = ((int64_t)n_positions + kWave - 1) / kWave;
    const dim3 grid((unsigned)((n_samples + kBamWaves - 1) / kBamWaves), (unsigned)(chunks < 1024 ? chunks : 1024));
    hipLaunchKernelGGL(bam_counts_depth_kernel, grid, dim3(kBamThreads), 0, stream, n_samples, bam, bam_bytes, sample_off, sample_end, s.reads, s.runmax,
                       s.n_reads, n_positions, positions, rg_s, refseq_len, group_of_sample, n_groups, counts, reinterpret_cast<uint32_t *>(tally),
                       group_depth);
    return hipGetLastError();
}

}  // namespace bvc
