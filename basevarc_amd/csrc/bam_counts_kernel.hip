// bam_counts_kernel.hip -- phase 1 of `BaseVarC basetype` added straight into per-position class counts: the inflated alignment records of
// a batch of samples -> counts and tally [position] of any CountsLayout (counts_layout.h; include/bvc_bam_counts.h, bvc_bam_group_depth.h,
// bvc_site_acc_quals.h).  The cheap sibling of bam_pileup_kernel.hip, shaped like bam_popmatrix_kernel.hip: the read table
// (bam_index_kernel) and resolve() (bam_resolve_device.h) are theirs, so which (sample, position) has which entry -- and which sample is
// out of range -- is bvc_bam_pileup's word for word.
//
//   bam_counts_kernel<ADD, K>   one wavefront per sample, one position a lane: one resolve() without text.  ADD = false: the dry pass -- it lets
//                               the call promise that nothing is added unless it returns BVC_OK.  ADD = true: one atomic add into the
//                               position's tally, and for a base 0..3 whose quality has a column one into its class count.  K:
//                                 Slots    counts [slots][512], the sample's label names the slot.  Its dry pass only raises status 4 and
//                                          loads no quality; it is Depth's dry pass too
//                                 Depth    one slot, and under the count add's condition one add into the depth of the sample's group
//                                 Narrow   counts [4][n_quals], the depth add with groups.  Its dry pass also raises status 5 for a base
//                                          0..3 whose quality byte q is n_quals <= q <= 127; a sample ends with 4 where both were raised,
//                                          whatever the order (an exchange writes 4 over anything, a compare-and-swap writes 5 over 0 only)
//                               Every quality is compared with the columns before an address is made of it, whatever the dry pass found.
//   first_status_kernel         one wavefront: the first sample of one status (0x7FFFFFFF: none), as bam_scan_kernel finds 2, 3 and 4
//   acc_expand_kernel           rows [n][4][n_quals] -> [n][512], zeros in the columns >= n_quals: 16 bytes a lane, streaming
// No size matrix, no row scan, no LDS: every lane adds into another position's rows.  The adds are 32-bit integer atomics on global
// memory that return nothing; several launches (of several contexts) may add into the same arrays at once.  All index arithmetic is
// 64-bit: 2.5e8 positions x 192 words pass 2^32.
#include "bam_resolve_device.h"
#include "../../include/bvc_site_acc_quals.h"

namespace bvc {

template <bool ADD, CountsKind K>
__global__ __launch_bounds__(kBamThreads) void bam_counts_kernel(
    int32_t n_samples, const uint8_t *__restrict__ bam, int64_t bam_bytes, const int64_t *__restrict__ sample_off,
    const int64_t *__restrict__ sample_end, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax, const uint32_t *__restrict__ n_reads,
    int32_t n_positions, const int32_t *__restrict__ positions, int32_t rg_s, int64_t refseq_len, const uint8_t *__restrict__ group_of_sample,
    int32_t n_groups, uint32_t n_quals, uint32_t *__restrict__ counts, uint32_t *__restrict__ tally, uint32_t *__restrict__ group_depth,
    uint32_t *__restrict__ sample_status)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t s = (int32_t)uniform(blockIdx.x * kBamWaves + (threadIdx.x >> 6));
    if (s >= n_samples) return;
    const uint32_t n = uniform(n_reads[s]);         // 0: no kept read (status 1), or a status that fails the call
    if (n == 0u) return;
    int64_t lo, hi;
    sample_range(sample_off, sample_end, s, bam_bytes, lo, hi);
    const int64_t slot0 = uniform64(lo) / kBamMinRecord;
    // the sample's label: its slot of counts (a label outside the groups: the last one), or whether it adds a depth
    uint32_t g = 0u, slots = 1u, slot = 0u;
    bool grouped = false;
    if (ADD && (K == CountsKind::Depth || n_groups > 0)) {
        g = uniform(group_of_sample[s]);
        if (K == CountsKind::Slots) {
            slots = (uint32_t)n_groups + 1u;
            slot = g < (uint32_t)n_groups ? g : (uint32_t)n_groups;
        } else
            grouped = g < (uint32_t)n_groups;       // (the program's 255: in no group)
    }
    for (int64_t t0 = (int64_t)blockIdx.y * kWave; t0 < n_positions; t0 += (int64_t)gridDim.y * kWave) {
        const int64_t t = t0 + lane;
        if (t >= n_positions) continue;
        const Hit h = resolve<false>(bam, reads + slot0, runmax + slot0, n, positions[t], rg_s, refseq_len);
        const uint32_t base = h.fields & 0xFFu, qual = (h.fields >> 16) & 0xFFu;
        if (!ADD) {
            if (K != CountsKind::Narrow) {
                if (h.out_of_range) sample_status[s] = 4u;
            } else if (h.out_of_range)
                (void)atomicExch(sample_status + s, 4u);
            else if (h.size != 0u && !(h.flags & 2u) && base <= 3u && qual >= n_quals && qual < 128u)
                (void)atomicCAS(sample_status + s, 0u, 5u);
            continue;
        }
        if (h.out_of_range || h.size == 0u) continue;
        uint32_t *const tw = tally + t * (int64_t)(sizeof(bvc_bam_site_tally) / 4);
        if (h.flags & 2u) { atomicAdd(tw + 9, 1u); continue; }          // an indel entry
        if (base > 3u) { atomicAdd(tw + 8, 1u); continue; }             // class 4
        atomicAdd(tw + (((h.flags & 1u) << 2) | base), 1u);
        if (qual < (K == CountsKind::Narrow ? n_quals : 128u)) {        // (n_quals <= 128: a covered observation that has a column)
            if (K == CountsKind::Narrow) atomicAdd(counts + ((t * 4 + (int64_t)base) * (int64_t)n_quals + (int64_t)qual), 1u);
            else atomicAdd(counts + (t * slots + slot) * 512 + base * 128u + qual, 1u);
            if (grouped) atomicAdd(group_depth + ((t * n_groups + (int64_t)g) * 4 + (int64_t)base), 1u);
        }
    }
}

// out[0] = the first sample whose status is `which`, 0x7FFFFFFF: none
__global__ __launch_bounds__(kWave) void first_status_kernel(int32_t n_samples, const uint32_t *__restrict__ sample_status, uint32_t which,
                                                             int64_t *__restrict__ out)
{
    const int lane = threadIdx.x;
    int32_t first = 0x7FFFFFFF;
    for (int32_t s0 = 0; s0 < n_samples && first == 0x7FFFFFFF; s0 += kWave) {
        const int32_t s = s0 + lane;
        const uint64_t m = __ballot(s < n_samples && sample_status[s] == which);
        if (m) first = s0 + (int32_t)__builtin_ctzll(m);
    }
    if (lane == 0) out[0] = first;
}

// One lane a 16-byte piece of an output row: piece j of row r is the qualities 4 * (j % 32) .. + 3 of base j / 32.
constexpr int kExpandThreads = 256;
constexpr int kExpandGrid = 2048;                   // workgroups at most: more pieces go round the loop again
__global__ __launch_bounds__(kExpandThreads) void acc_expand_kernel(int64_t n_rows, uint32_t n_quals, const uint4 *__restrict__ narrow,
                                                                    uint4 *__restrict__ wide)
{
    const int64_t pieces = n_rows * 128, q4 = n_quals >> 2;
    for (int64_t i = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * kExpandThreads) {
        const int64_t row = i >> 7;
        const uint32_t j = (uint32_t)i & 127u, base = j >> 5, q = j & 31u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((int64_t)q < q4) v = narrow[(row * 4 + (int64_t)base) * q4 + (int64_t)q];
        wide[i] = v;
    }
}

hipError_t launch_bam_counts(hipStream_t stream, bool add, const BamCall &c, const CountsLayout &layout, const BamPileupScratch &s, CountsArrays a,
                             uint32_t *sample_status)
{
    if (!layout.quals_ok()) return hipErrorInvalidValue;
    if (c.n_samples <= 0 || c.n_positions <= 0) return hipSuccess;
    if (add && layout.label_groups() > 0u && (!a.group_of_sample || (layout.depth_groups > 0u && !a.depth))) return hipErrorInvalidValue;
    const CountsKind k = layout.kind();
    // (the five instantiations have one type: the wide dry pass serves Slots and Depth)
    auto *const kernel = !add ? (k == CountsKind::Narrow ? bam_counts_kernel<false, CountsKind::Narrow> : bam_counts_kernel<false, CountsKind::Slots>)
                         : k == CountsKind::Narrow ? bam_counts_kernel<true, CountsKind::Narrow>
                         : k == CountsKind::Depth  ? bam_counts_kernel<true, CountsKind::Depth>
                                                   : bam_counts_kernel<true, CountsKind::Slots>;
    hipLaunchKernelGGL(kernel, bam_sample_grid(c.n_samples, c.n_positions), dim3(kBamThreads), 0, stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end,
                       s.reads, s.runmax, s.n_reads, c.n_positions, c.pos, c.rg_s, c.refseq_len, a.group_of_sample, (int32_t)layout.label_groups(),
                       layout.n_quals, a.counts, reinterpret_cast<uint32_t *>(a.tally), a.depth, sample_status);
    return hipGetLastError();
}

hipError_t launch_first_status(hipStream_t stream, int32_t n_samples, const uint32_t *sample_status, uint32_t which, int64_t *out)
{
    hipLaunchKernelGGL(first_status_kernel, dim3(1), dim3(kWave), 0, stream, n_samples, sample_status, which, out);
    return hipGetLastError();
}

hipError_t launch_acc_expand(hipStream_t stream, int64_t n_rows, int32_t n_quals, const uint32_t *narrow, uint32_t *wide)
{
    if (!CountsLayout::quals_ok(n_quals) || n_rows < 0) return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    const int64_t blocks = (n_rows * 128 + kExpandThreads - 1) / kExpandThreads;
    hipLaunchKernelGGL(acc_expand_kernel, dim3((unsigned)(blocks < kExpandGrid ? blocks : kExpandGrid)), dim3(kExpandThreads), 0, stream, n_rows,
                       (uint32_t)n_quals, reinterpret_cast<const uint4 *>(narrow), reinterpret_cast<uint4 *>(wide));
    return hipGetLastError();
}

static_assert(sizeof(bvc_bam_site_tally) == 48, "twelve words a position");

}  // namespace bvc
