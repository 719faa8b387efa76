// bgzf_dynamic_kernel.hip -- the instantiation <false, true> of the device deflate encoder's block kernel (bgzf_block_kernel.h; tuning key
// "bgzf_codes" = 1 with the general parse), and the launch of the three instantiations that the tuning keys choose.  It lives here, not beside
// <false, false> in bgzf_deflate_kernel.hip, because this file is built without the compiler's machine LICM pass (build.py): with it the
// block kernel with the code builder inlined has 128 VGPRs and 3 of them spilled, without it 77 and none.  The plan, CRC, scan and pack
// kernels of bgzf_deflate_kernel.hip, where the passes are described, run unchanged around all four.
//
// What "bgzf_codes" = 1 runs behind passes A and B (RFC 1951, BTYPE = 10; bgzf_dynamic_device.h) -- the parse is the one the fixed code gets:
//   COUNTS   thread t counts the symbols of positions 64 t .. 64 t + 63 into 316 LDS counters (atomicAdd), end of block once
//   LENGTHS  wavefront 0 builds both alphabets' lengths, the code-length sequence, its code and all canonical codes by the rule of
//            docs/BGZF_DYNAMIC.md (bgzf_codes_device.h), and the block's size in the dynamic (D) and in the fixed code; the other fifteen
//            wavefronts wait at the barrier
//   CHOICE   F = what the fixed code's pass C writes (fixed, or stored where that is smaller).  The block is dynamic iff D < F, else exactly
//            that block.  (workgroup-uniform: read from LDS behind a barrier)
//   BITS     as pass C, the codes from the LDS table; thread 0 writes the header in front of its symbols, every thread's first bit is
//            offset by the header's; a match is two puts (length half, distance half: up to 20 + 28 bits) with a flush between;
//            the end-of-block code behind the last symbol
// bgzf_code_lengths_kernel runs the same length builder on counts of the caller's, one wavefront a set (bvc_bgzf_code_lengths).
#include "bgzf_block_kernel.h"

namespace bvc {

template __global__ void bgzf_block_kernel<false, true>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);
// (bgzf_fields_kernel.hip holds the field parse's two: with both dynamic instantiations in one source the compiler gives each a few other
// instructions than it has alone)
extern template __global__ void bgzf_block_kernel<true, false>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);
extern template __global__ void bgzf_block_kernel<true, true>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);

// lengths[set][0 .. n_symbols) from counts[set][0 .. n_symbols): the builder of the block kernel, one wavefront a set.
__global__ __launch_bounds__(kWave) void bgzf_code_lengths_kernel(int64_t n_sets, const uint32_t *__restrict__ counts, uint32_t n_symbols,
                                                                  uint32_t limit, uint8_t *__restrict__ lengths)
{
    BVC_POISON_LDS();
    __shared__ CodeTables t;
    const uint32_t lane = threadIdx.x;
    const uint32_t n = n_symbols < kDcMaxSyms ? n_symbols : kDcMaxSyms;
    for (int64_t set = blockIdx.x; set < n_sets; set += gridDim.x) {
        for (uint32_t s = lane; s < n; s += kWave) t.counts[s] = counts[set * (int64_t)n_symbols + s];
        __syncthreads();
        dc_build_lengths(t.counts, n, limit, t.len, t, lane, kWave);
        __syncthreads();
        for (uint32_t s = lane; s < n; s += kWave) lengths[set * (int64_t)n_symbols + s] = t.len[s];
        __syncthreads();
    }
}

// mode.fields || mode.dynamic: launch_bgzf_deflate launches the fourth instantiation itself
void launch_bgzf_blocks_other(hipStream_t stream, unsigned grid, const BgzfMode &mode, const uint8_t *data, const BlockDesc *desc, int64_t n_blocks,
                              uint8_t *staging, uint32_t *bsize, uint32_t *match_rows)
{
    auto *const kernel = !mode.fields ? bgzf_block_kernel<false, true> : mode.dynamic ? bgzf_block_kernel<true, true> : bgzf_block_kernel<true, false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBdThreads), 0, stream, data, desc, n_blocks, staging, bsize, match_rows, mode.delims);
}

hipError_t launch_bgzf_code_lengths(hipStream_t stream, int64_t n_sets, const uint32_t *counts, int32_t n_symbols, int32_t limit, uint8_t *lengths)
{
    if (n_sets > 0)
        hipLaunchKernelGGL(bgzf_code_lengths_kernel, dim3((unsigned)(n_sets < 4096 ? n_sets : 4096)), dim3(kWave), 0, stream, n_sets, counts,
                           (uint32_t)n_symbols, (uint32_t)limit, lengths);
    return hipGetLastError();
}

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_bgzf_dynamic)
#endif

}  // namespace bvc
