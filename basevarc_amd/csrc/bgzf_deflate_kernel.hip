// bgzf_deflate_kernel.hip -- DEFLATE (RFC 1951) of byte ranges in device memory into finished BGZF blocks (include/bvc.h): what
// the host program's BgzfWriter does with zlib, done where the VCF sample columns are made (vcf_samples_kernel.hip).
//
// A block is at most 65280 input bytes and static: every position can look for its match at once.  One WORKGROUP of 1024 threads per
// block, the block's input and its match tables in LDS (144 KiB: one workgroup a CU).  Five launches:
//   bgzf_plan_kernel     block b of the call -> (source, length): piece i holds blocks first_block[i] .. first_block[i + 1], of which
//                        those behind the piece's real length are empty (the host may know an upper bound of a length only)
//   bgzf_block_kernel    the block, written to its own 64 KiB slot of a staging buffer, and its size (bgzf_block_kernel.h: one template
//                        for both parses and both codes.  <false, false>, the default, is instantiated here; tuning keys "bgzf_codes" = 1
//                        and "bgzf_parse" = 1 choose among the other three, which bgzf_dynamic_kernel.hip and bgzf_fields_kernel.hip hold)
//   bgzf_crc_kernel      CRC32 of the block's input into its trailer: one wavefront a block, crc32_device.h
//   bgzf_scan_kernel     exclusive prefix sums of the sizes: where each block goes, comp_off of every piece
//   bgzf_pack_kernel     the blocks laid down one after the other, no gaps
//
// The block kernel, per block (pass A as the general parse has it; the field parse's is described in bgzf_fields_device.h):
//   A  MATCHES.  The positions are taken in rounds of 256, in order, four lanes a position.  Candidates for position p come from
//      - a table of 16 ways x 2048 hash values (hash of the four bytes at p): way (r mod 16) holds the LARGEST position of round r' = r
//        (mod 16), r' < current, with that hash -- written with atomicMax after the round's look-ups, so a cell never depends on the
//        order in which wavefronts arrive.  Sixteen bits a cell (position + 1); ways w and w + 8 share a word, and as only one way is
//        written in a round the other half of the word is constant while atomicMax works on it;
//      - the FIRST position of the current round with the hash (atomicMax of (round + 1) << 8 | 255 - offset, written before the
//        look-ups), for the matches a round would otherwise not see in itself: the text's fields are 4 and 17 bytes apart.
//      Each lane extends four ways (lane 0 also the round's own candidate) eight bytes of LDS a step and keeps the longest: a later
//      candidate replaces the lane's best only if it is strictly longer (it is skipped unless it matches where the best so far ends,
//      and nothing is tried behind a match of full length).  The quad then keeps the longest of its four, the nearest among equals;
//      a match is used from 4 bytes on.  (match - 3) << 16 | (distance - 1) | 1 << 31 goes to a
//      scratch row in global memory: the tables and the input fill the LDS.
//   B  PATH.  The tables' space takes one byte a position (the literal, or length - 3) and a bit a position says which; ONE lane walks
//      the greedy parse -- the dependent chain of a block, one LDS read a match, literals by the bit mask 32 positions a step -- and
//      marks the positions where a symbol starts.
//   C  BITS.  Thread t owns positions 64 t .. 64 t + 63: it adds up its symbols' bits in the fixed code, a workgroup scan gives its
//      first bit, and it writes its symbols into an LDS image of the output, whole words with one atomicOr each (its first and last
//      word are shared with its neighbours; OR does not depend on order).  If the image would be larger than the stored form the block
//      is stored instead.  The workgroup copies header, image and ISIZE to the staging slot.
// Every LDS index that comes from data (hash values, candidate positions, bit offsets) is bounded before use.
#include "bgzf_block_kernel.h"
#include "crc32_device.h"

namespace bvc {

template __global__ void bgzf_block_kernel<false, false>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);

// desc[b] of every block of the call: piece i = the one with first_block[i] <= b < first_block[i + 1].
__global__ __launch_bounds__(256) void bgzf_plan_kernel(
    int64_t n_pieces, const int64_t *__restrict__ piece_off, const int64_t *__restrict__ piece_len, const int64_t *__restrict__ first_block,
    int64_t n_blocks, BlockDesc *__restrict__ desc)
{
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < n_blocks; b += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n_pieces - 1;                                    // the last piece with first_block[i] <= b
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (first_block[mid] <= b) lo = mid; else hi = mid - 1;
        }
        const int64_t at = (b - first_block[lo]) * (int64_t)kBdIn, left = piece_len[lo] - at;
        BlockDesc d;
        d.src = piece_off[lo] + at;
        d.len = left <= 0 ? 0u : (left < (int64_t)kBdIn ? (uint32_t)left : kBdIn);
        d.pad = 0u;
        desc[b] = d;
    }
}

// CRC32 of every block's input into bytes bsize - 8 .. bsize - 5 of its slot.  data16 = `data` rounded down to 16 bytes, shift = what
// was cut off: the slices of crc32_wave are cut at absolute 16-byte boundaries.
__global__ __launch_bounds__(kWave) void bgzf_crc_kernel(const uint8_t *__restrict__ data16, uint32_t shift, const BlockDesc *__restrict__ desc,
                                                         int64_t n_blocks, const uint32_t *__restrict__ bsize, uint8_t *__restrict__ staging)
{
    BVC_POISON_LDS();
    __shared__ uint32_t tab[256];
    const int lane = threadIdx.x;
    crc_table_fill(tab, lane);
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        if (n == 0u) continue;
        const uint32_t crc = crc32_wave(data16, (uint64_t)desc[blk].src + shift, n, tab, lane);
        const uint32_t bs = bsize[blk] <= kBdSlot ? bsize[blk] : kBdSlot;
        if (lane < 4 && bs >= 26u) staging[(size_t)blk * kBdSlot + bs - 8u + (uint32_t)lane] = (uint8_t)(crc >> (8 * lane));
    }
}

// block_off[0 .. n_blocks] = exclusive prefix sums of the sizes; comp_off[i] = block_off[first_block[i]], i <= n_pieces.  One workgroup.
__global__ __launch_bounds__(1024) void bgzf_scan_kernel(int64_t n_blocks, const uint32_t *__restrict__ bsize, int64_t *__restrict__ block_off,
                                                         int64_t n_pieces, const int64_t *__restrict__ first_block, int64_t *__restrict__ comp_off)
{
    BVC_POISON_LDS();
    __shared__ int64_t s_sz[1024];
    const int tid = threadIdx.x;
    int64_t base = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const int64_t b = b0 + tid;
        const int64_t sz = b < n_blocks ? (int64_t)bsize[b] : 0;
        s_sz[tid] = sz;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t v = tid >= d ? s_sz[tid - d] : 0;
            __syncthreads();
            s_sz[tid] += v;
            __syncthreads();
        }
        if (b < n_blocks) block_off[b] = base + s_sz[tid] - sz;
        const int64_t tot = s_sz[1023];
        __syncthreads();
        base += tot;
    }
    if (tid == 0) block_off[n_blocks] = base;
    __threadfence();
    __syncthreads();
    for (int64_t i = tid; i <= n_pieces; i += 1024) comp_off[i] = block_off[first_block[i]];
}

__global__ __launch_bounds__(256) void bgzf_pack_kernel(int64_t n_blocks, const uint32_t *__restrict__ bsize, const int64_t *__restrict__ block_off,
                                                        const uint8_t *__restrict__ staging, uint8_t *__restrict__ comp, int64_t comp_cap)
{
    if (block_off[n_blocks] > comp_cap) return;                               // (the host side has compared the bound with it)
    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t bs = bsize[blk] <= kBdSlot - 8u ? bsize[blk] : kBdSlot - 8u;       // (a block is at most 65280 + 31 bytes)
        // aligned words of `comp` from the two aligned words of the slot that hold them (the slot is aligned, the destination starts at
        // any byte); up to three bytes each in front of and behind them
        const uint32_t *__restrict__ from = reinterpret_cast<const uint32_t *>(staging + (size_t)blk * kBdSlot);
        uint8_t *__restrict__ to = comp + block_off[blk];
        const uint32_t lead = (uint32_t)(-reinterpret_cast<uintptr_t>(to) & 3u);
        const uint32_t head = lead < bs ? lead : bs, words = (bs - head) >> 2, tail = head + 4u * words;
        if (threadIdx.x < head) to[threadIdx.x] = (uint8_t)(from[0] >> (8u * threadIdx.x));
        uint32_t *__restrict__ to32 = reinterpret_cast<uint32_t *>(to + head);
        for (uint32_t j = threadIdx.x; j < words; j += 256) {
            const uint32_t at = head + 4u * j;                                // (at + 7 < bs + 4 <= the slot's 64 KiB: bs <= 65280 + 31)
            const uint64_t v = (uint64_t)from[at >> 2] | ((uint64_t)from[(at >> 2) + 1u] << 32);
            to32[j] = (uint32_t)(v >> (8u * (at & 3u)));
        }
        if (threadIdx.x < bs - tail) {
            const uint32_t at = tail + threadIdx.x;
            to[at] = (uint8_t)(from[at >> 2] >> (8u * (at & 3u)));
        }
    }
}

size_t bgzf_deflate_scratch_bytes(int64_t n_pieces, int64_t n_blocks)
{
    Layout L;
    (void)bgzf_deflate_scratch(nullptr, n_pieces, n_blocks, &L);
    return L.at;
}

BgzfDeflateScratch bgzf_deflate_scratch(void *buf, int64_t n_pieces, int64_t n_blocks, Layout *sized)
{
    Layout L{reinterpret_cast<uintptr_t>(buf)};
    const size_t nb = (size_t)n_blocks, grid = nb < (size_t)kBgzfDeflateGrid ? nb : (size_t)kBgzfDeflateGrid;
    BgzfDeflateScratch s;
    s.first_block = L.take<int64_t>((size_t)n_pieces + 1);
    s.block_off = L.take<int64_t>(nb + 1);
    s.desc = L.take<BlockDesc>(nb);
    s.bsize = L.take<uint32_t>(nb);
    s.match_rows = L.take<uint32_t>(grid * kBdIn);
    s.staging = L.take<uint8_t>(nb * kBdSlot);
    if (sized) *sized = L;
    return s;
}

// The tuning keys as the launches read them: the one place where they become a mode.
BgzfMode bgzf_mode(const LaunchState &ls)
{
    return {ls.bgzf_parse == 1, ls.bgzf_codes == 1, ls.bgzf_cuts == 1 ? kBfDelimsSpaceNewline : kBfDelimsTabColon};
}

hipError_t launch_bgzf_deflate(hipStream_t stream, int64_t n_pieces, const uint8_t *data, const int64_t *piece_off, const int64_t *piece_len,
                               int64_t n_blocks, const BgzfDeflateScratch &s, uint8_t *comp, int64_t comp_cap, int64_t *comp_off, const BgzfMode &mode)
{
    if (n_blocks > 0) {
        const unsigned grid = (unsigned)(n_blocks < kBgzfDeflateGrid ? n_blocks : kBgzfDeflateGrid);
        hipLaunchKernelGGL(bgzf_plan_kernel, dim3((unsigned)((n_blocks + 255) / 256 < 1024 ? (n_blocks + 255) / 256 : 1024)), dim3(256), 0, stream,
                           n_pieces, piece_off, piece_len, s.first_block, n_blocks, s.desc);
        if (mode.fields || mode.dynamic) launch_bgzf_blocks_other(stream, grid, mode, data, s.desc, n_blocks, s.staging, s.bsize, s.match_rows);
        else hipLaunchKernelGGL((bgzf_block_kernel<false, false>), dim3(grid), dim3(kBdThreads), 0, stream, data, s.desc, n_blocks, s.staging, s.bsize,
                                s.match_rows, mode.delims);
        const uintptr_t a = reinterpret_cast<uintptr_t>(data);
        hipLaunchKernelGGL(bgzf_crc_kernel, dim3((unsigned)(n_blocks < 65536 ? n_blocks : 65536)), dim3(kWave), 0, stream,
                           reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)15), (uint32_t)(a & 15u), s.desc, n_blocks, s.bsize, s.staging);
    }
    // (with no block at all it still writes comp_off: all zero)
    hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(1024), 0, stream, n_blocks, s.bsize, s.block_off, n_pieces, s.first_block, comp_off);
    if (n_blocks > 0)
        hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)(n_blocks < 2048 ? n_blocks : 2048)), dim3(256), 0, stream, n_blocks, s.bsize,
                           s.block_off, s.staging, comp, comp_cap);
    return hipGetLastError();
}

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_bgzf_deflate)
#endif

}  // namespace bvc
