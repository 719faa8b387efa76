// bgzf_fields_kernel.hip -- the device deflate encoder with the field parse (docs/BGZF_FIELDS.md): what tuning key "bgzf_parse" = 1 launches
// in place of bgzf_deflate_kernel ("bgzf_codes" = 0: bgzf_deflate_fields_kernel) and of bgzf_deflate_dynamic_kernel ("bgzf_codes" = 1:
// bgzf_deflate_fields_dynamic_kernel).  Same grid, same 1024 threads a block, same staging slot and bsize; the plan, CRC, scan and pack
// kernels of bgzf_deflate_kernel.hip run unchanged around them.
//
// Only pass A differs: bd_field_matches (bgzf_fields_device.h) fills the match row from two bitmaps of the block -- where fields start (behind
// a tab or a colon; with tuning key "bgzf_cuts" = 1 behind a space or a newline: the pair of bytes is the kernels' last argument),
// which fields repeat the field in front of them -- and a table look-up for the others, where bd_matches searches at every position.
// The row's format is the same, so pass B (the path) and what follows it are the shared ones: bd_fixed_block of bgzf_deflate_device.h,
// bd_dynamic_block of bgzf_dynamic_device.h.  The cuts' bitmap lies where pass B keeps the path bits; the heads' bitmap and a round's best
// matches are 9 KiB more LDS.
#include "bgzf_deflate_device.h"
#include "bgzf_codes_device.h"
#include "bgzf_dynamic_device.h"
#include "bgzf_fields_device.h"

namespace bvc {

static_assert((kBdInWords + kBdTabWords + 3 * kBdBitWords + kBdRound + 32) * 4 + sizeof(CodeTables) <= 160 * 1024, "one workgroup's LDS");

__global__ __launch_bounds__(kBdThreads) void bgzf_deflate_fields_kernel(
    const uint8_t *__restrict__ data, const BlockDesc *__restrict__ desc, int64_t n_blocks, uint8_t *__restrict__ staging,
    uint32_t *__restrict__ bsize, uint32_t *__restrict__ match_rows, uint32_t delims)
{
    BVC_POISON_LDS();
    __shared__ __attribute__((aligned(16))) uint32_t s_in[kBdInWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kBdTabWords];
    __shared__ uint32_t s_first[kBdBitWords];
    __shared__ uint32_t s_path[kBdBitWords];
    __shared__ uint32_t s_head[kBdBitWords];
    __shared__ uint32_t s_best[kBdRound];
    __shared__ uint32_t s_scan[32];
    const uint32_t tid = threadIdx.x;
    uint32_t *const match = match_rows + (size_t)blockIdx.x * kBdIn;
    uint32_t *const s_ism = s_first;                                          // passes B and C: bit p = position p holds a match

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {       // (workgroup-uniform)
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        uint8_t *const slot = staging + (size_t)blk * kBdSlot;
        if (n == 0u) {
            if (tid == 0u) bsize[blk] = 0u;
            continue;
        }
        bd_load(s_in, s_tab, s_first, data + desc[blk].src, n, tid);
        bd_field_matches(s_in, s_tab, s_first, s_path, s_head, s_best, match, n, tid, delims);
        bd_path(s_in, s_tab, s_ism, s_path, match, n, tid);
        const uint32_t bs = bd_fixed_block(slot, s_in, s_tab, s_ism, s_path, s_scan, match, n, tid);
        if (tid == 0u) bsize[blk] = bs;
        __syncthreads();                                                      // the LDS belongs to the next block from here
    }
}

__global__ __launch_bounds__(kBdThreads) void bgzf_deflate_fields_dynamic_kernel(
    const uint8_t *__restrict__ data, const BlockDesc *__restrict__ desc, int64_t n_blocks, uint8_t *__restrict__ staging,
    uint32_t *__restrict__ bsize, uint32_t *__restrict__ match_rows, uint32_t delims)
{
    BVC_POISON_LDS();
    __shared__ __attribute__((aligned(16))) uint32_t s_in[kBdInWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kBdTabWords];
    __shared__ uint32_t s_first[kBdBitWords];
    __shared__ uint32_t s_path[kBdBitWords];
    __shared__ uint32_t s_head[kBdBitWords];
    __shared__ uint32_t s_best[kBdRound];
    __shared__ uint32_t s_scan[32];
    __shared__ CodeTables s_codes;
    const uint32_t tid = threadIdx.x;
    uint32_t *const match = match_rows + (size_t)blockIdx.x * kBdIn;
    uint32_t *const s_ism = s_first;                                          // behind pass B: bit p = position p holds a match

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {       // (workgroup-uniform)
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        uint8_t *const slot = staging + (size_t)blk * kBdSlot;
        if (n == 0u) {
            if (tid == 0u) bsize[blk] = 0u;
            continue;
        }
        bd_load(s_in, s_tab, s_first, data + desc[blk].src, n, tid);
        bd_field_matches(s_in, s_tab, s_first, s_path, s_head, s_best, match, n, tid, delims);
        bd_path(s_in, s_tab, s_ism, s_path, match, n, tid);
        const uint32_t bs = bd_dynamic_block(slot, s_in, s_tab, s_ism, s_path, s_scan, s_codes, match, n, tid);
        if (tid == 0u) bsize[blk] = bs;
        __syncthreads();                                                      // the LDS belongs to the next block from here
    }
}

void launch_bgzf_deflate_field_blocks(hipStream_t stream, unsigned grid, int codes, int cuts, const uint8_t *data, const char *desc, int64_t n_blocks,
                                      uint8_t *staging, uint32_t *bsize, uint32_t *match_rows)
{
    const BlockDesc *const d = reinterpret_cast<const BlockDesc *>(desc);
    const uint32_t delims = cuts == 1 ? kBfDelimsSpaceNewline : kBfDelimsTabColon;   // tuning key "bgzf_cuts"
    if (codes == 1)
        hipLaunchKernelGGL(bgzf_deflate_fields_dynamic_kernel, dim3(grid), dim3(kBdThreads), 0, stream, data, d, n_blocks, staging, bsize, match_rows, delims);
    else
        hipLaunchKernelGGL(bgzf_deflate_fields_kernel, dim3(grid), dim3(kBdThreads), 0, stream, data, d, n_blocks, staging, bsize, match_rows, delims);
}

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_bgzf_fields)
#endif

}  // namespace bvc
