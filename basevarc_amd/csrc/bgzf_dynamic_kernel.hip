// bgzf_dynamic_kernel.hip -- the device deflate encoder with a Huffman code of the block's own (RFC 1951, BTYPE = 10): what tuning key
// "bgzf_codes" = 1 launches in place of bgzf_deflate_kernel (bgzf_deflate_kernel.hip, where the passes are described).  Same grid,
// same 1024 threads a block, same staging slot and bsize; the plan, CRC, scan and pack kernels run unchanged around it.
//
// Passes A and B are the shared ones (bgzf_deflate_device.h): the parse -- literals, lengths, distances -- is the one the fixed code gets.
// Behind them (bgzf_dynamic_device.h: the field parse's kernel of bgzf_fields_kernel.hip runs the same):
//   COUNTS   thread t counts the symbols of positions 64 t .. 64 t + 63 into 316 LDS counters (atomicAdd), end of block once
//   LENGTHS  wavefront 0 builds both alphabets' lengths, the code-length sequence, its code and all canonical codes by the rule of
//            docs/BGZF_DYNAMIC.md (bgzf_codes_device.h), and the block's size in the dynamic (D) and in the fixed code; the other fifteen
//            wavefronts wait at the barrier
//   CHOICE   F = what bgzf_deflate_kernel writes (fixed, or stored where that is smaller).  The block is dynamic iff D < F, else exactly
//            that block.  (workgroup-uniform: read from LDS behind a barrier)
//   BITS     as pass C, the codes from the LDS table; thread 0 writes the header in front of its symbols, every thread's first bit is
//            offset by the header's; a match is two puts (length half, distance half: up to 20 + 28 bits) with a flush between;
//            the end-of-block code behind the last symbol
// bgzf_code_lengths_kernel runs the same length builder on counts of the caller's, one wavefront a set (bvc_bgzf_code_lengths).
#include "bgzf_deflate_device.h"
#include "bgzf_codes_device.h"
#include "bgzf_dynamic_device.h"

namespace bvc {

__global__ __launch_bounds__(kBdThreads) void bgzf_deflate_dynamic_kernel(
    const uint8_t *__restrict__ data, const BlockDesc *__restrict__ desc, int64_t n_blocks, uint8_t *__restrict__ staging,
    uint32_t *__restrict__ bsize, uint32_t *__restrict__ match_rows)
{
    BVC_POISON_LDS();
    __shared__ __attribute__((aligned(16))) uint32_t s_in[kBdInWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kBdTabWords];
    __shared__ uint32_t s_first[kBdBitWords];
    __shared__ uint32_t s_path[kBdBitWords];
    __shared__ uint32_t s_scan[32];
    __shared__ CodeTables s_codes;
    const uint32_t tid = threadIdx.x;
    uint32_t *const match = match_rows + (size_t)blockIdx.x * kBdIn;
    // (behind pass B the image of the output lies in s_in, and the bytes of s_tab are the literal, or length - 3)
    uint32_t *const s_ism = s_first;                                          // behind pass B: bit p = position p holds a match

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {       // (workgroup-uniform)
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        uint8_t *const slot = staging + (size_t)blk * kBdSlot;
        if (n == 0u) {
            if (tid == 0u) bsize[blk] = 0u;
            continue;
        }
        bd_load(s_in, s_tab, s_first, data + desc[blk].src, n, tid);
        bd_matches(s_in, s_tab, s_first, match, n, tid);
        bd_path(s_in, s_tab, s_ism, s_path, match, n, tid);

        const uint32_t bs = bd_dynamic_block(slot, s_in, s_tab, s_ism, s_path, s_scan, s_codes, match, n, tid);
        if (tid == 0u) bsize[blk] = bs;
        __syncthreads();                                                      // the LDS belongs to the next block from here
    }
}

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

void launch_bgzf_deflate_dynamic_blocks(hipStream_t stream, unsigned grid, const uint8_t *data, const char *desc, int64_t n_blocks, uint8_t *staging,
                                        uint32_t *bsize, uint32_t *match_rows)
{
    hipLaunchKernelGGL(bgzf_deflate_dynamic_kernel, dim3(grid), dim3(kBdThreads), 0, stream, data, reinterpret_cast<const BlockDesc *>(desc), n_blocks,
                       staging, bsize, match_rows);
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
