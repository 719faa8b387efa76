// bgzf_block_kernel.h -- the block kernel of the device deflate encoder, once: a block's way through passes A, B and C (described at the top of
// bgzf_deflate_kernel.hip) for both parses and both codes.  FIELDS: pass A is the field parse (bd_field_matches, bgzf_fields_device.h;
// tuning key "bgzf_parse" = 1) instead of the search at every position (bd_matches); DYNAMIC: pass C may give the block a Huffman code of
// its own (bd_dynamic_block, bgzf_dynamic_device.h; "bgzf_codes" = 1) instead of the fixed code or the stored form (bd_fixed_block).  Same
// grid, same 1024 threads a block, same staging slot and bsize for all four; an instantiation holds the LDS of the passes it runs only.
// bgzf_deflate_kernel.hip instantiates <false, false>, bgzf_dynamic_kernel.hip <false, true>, bgzf_fields_kernel.hip <true, false> and <true, true>.
#pragma once
#include "bgzf_deflate_device.h"
#include "bgzf_codes_device.h"
#include "bgzf_dynamic_device.h"
#include "bgzf_fields_device.h"

namespace bvc {

// delims: the two bytes that end a field (kBfDelimsTabColon, kBfDelimsSpaceNewline); only the field parse reads them
template <bool FIELDS, bool DYNAMIC>
__global__ __launch_bounds__(kBdThreads) void bgzf_block_kernel(
    const uint8_t *__restrict__ data, const BlockDesc *__restrict__ desc, int64_t n_blocks, uint8_t *__restrict__ staging,
    uint32_t *__restrict__ bsize, uint32_t *__restrict__ match_rows, uint32_t delims)
{
    BVC_POISON_LDS();
    // the field parse's bitmap of heads and a round's best matches are 9 KiB more, the code tables 6.6 KiB more: one workgroup a CU either way
    static_assert((kBdInWords + kBdTabWords + (FIELDS ? 3 : 2) * kBdBitWords + (FIELDS ? kBdRound : 0) + 32) * 4 + (DYNAMIC ? sizeof(CodeTables) : 0)
                      <= 160 * 1024, "one workgroup's LDS");
    __shared__ __attribute__((aligned(16))) uint32_t s_in[kBdInWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kBdTabWords];
    __shared__ uint32_t s_first[kBdBitWords];
    __shared__ uint32_t s_path[kBdBitWords];                                  // (the field parse keeps its bitmap of cuts here until pass B)
    __shared__ uint32_t s_scan[32];
    uint32_t *heads = nullptr, *best = nullptr;                               // the field parse's bitmap of heads and a round's best matches
    CodeTables *codes = nullptr;                                              // the dynamic code's tables
    if constexpr (FIELDS) {
        __shared__ uint32_t s_head[kBdBitWords];
        __shared__ uint32_t s_best[kBdRound];
        heads = s_head;
        best = s_best;
    }
    if constexpr (DYNAMIC) {
        __shared__ CodeTables s_codes;
        codes = &s_codes;
    }
    const uint32_t tid = threadIdx.x;
    uint32_t *const match = match_rows + (size_t)blockIdx.x * kBdIn;
    // (behind pass B the image of the output lies in s_in, and the bytes of s_tab are the literal, or length - 3)
    uint32_t *const s_ism = s_first;                                          // passes B and C: bit p = position p holds a match

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {       // (workgroup-uniform)
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        uint8_t *const slot = staging + (size_t)blk * kBdSlot;
        if (n == 0u) {
            if (tid == 0u) bsize[blk] = 0u;
            continue;
        }
        bd_load(s_in, s_tab, s_first, data + desc[blk].src, n, tid);
        if constexpr (FIELDS) bd_field_matches(s_in, s_tab, s_first, s_path, heads, best, match, n, tid, delims);     // ---- A: matches
        else bd_matches(s_in, s_tab, s_first, match, n, tid);
        bd_path(s_in, s_tab, s_ism, s_path, match, n, tid);                                                               // ---- B: path

        uint32_t bs;                                                                                                      // ---- C: bits
        if constexpr (DYNAMIC) bs = bd_dynamic_block(slot, s_in, s_tab, s_ism, s_path, s_scan, *codes, match, n, tid);
        else bs = bd_fixed_block(slot, s_in, s_tab, s_ism, s_path, s_scan, match, n, tid);
        if (tid == 0u) bsize[blk] = bs;
        __syncthreads();                                                      // the LDS belongs to the next block from here
    }
}

// bgzf_dynamic_kernel.hip: the launch of every mode but <false, false>, which launch_bgzf_deflate (bgzf_deflate_kernel.hip) launches itself
void launch_bgzf_blocks_other(hipStream_t stream, unsigned grid, const BgzfMode &mode, const uint8_t *data, const BlockDesc *desc, int64_t n_blocks,
                              uint8_t *staging, uint32_t *bsize, uint32_t *match_rows);

}  // namespace bvc
