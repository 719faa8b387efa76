// bgzf_deflate_kernel.hip -- DEFLATE (RFC 1951) of byte ranges in device memory into finished BGZF blocks (include/bvc.h): what
// the host program's BgzfWriter does with zlib, done where the VCF sample columns are made (vcf_samples_kernel.hip).
//
// A block is at most 65280 input bytes and static: every position can look for its match at once.  One WORKGROUP of 1024 threads per
// block, the block's input and its match tables in LDS (144 KiB: one workgroup a CU).  Five launches:
//   bgzf_plan_kernel     block b of the call -> (source, length): piece i holds blocks first_block[i] .. first_block[i + 1], of which
//                        those behind the piece's real length are empty (the host may know an upper bound of a length only)
//   bgzf_deflate_kernel  the block, written to its own 64 KiB slot of a staging buffer, and its size
//   bgzf_crc_kernel      CRC32 of the block's input into its trailer: one wavefront a block, crc32_device.h
//   bgzf_scan_kernel     exclusive prefix sums of the sizes: where each block goes, comp_off of every piece
//   bgzf_pack_kernel     the blocks laid down one after the other, no gaps
//
// The deflate kernel, per block:
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
#include "bvc_device.h"
#include "bvc_internal.h"
#include "crc32_device.h"

namespace bvc {

namespace {

constexpr int kBdThreads = 1024;
constexpr int kBdRound = 256;                           // positions a round
constexpr int kBdLanes = kBdThreads / kBdRound;         // lanes a position
constexpr int kBdWays = 16, kBdHashBits = 11, kBdHash = 1 << kBdHashBits;
constexpr int kBdWaysPerLane = kBdWays / kBdLanes;
constexpr uint32_t kBdIn = BVC_BGZF_BLOCK_INPUT;
constexpr uint32_t kBdSlot = 65536;                     // bytes of a block's staging slot
constexpr uint32_t kBdMinMatch = 4, kBdMaxMatch = 258, kBdMaxDist = 32768;
constexpr uint32_t kBdMatchBit = 0x80000000u;
// LDS, in words: the input (+ the words a read of eight bytes at the last position touches), then the image of the output in its place;
// the table, then a byte a position in its place; the round's first positions, then the "is a match" bits; the path bits; the scan
constexpr int kBdInWords = kBdSlot / 4 + 4;
constexpr int kBdTabWords = kBdWays / 2 * kBdHash;
constexpr int kBdBitWords = kBdHash;                    // 65536 bits: one a position
static_assert(kBdTabWords * 4 >= (int)kBdIn && kBdBitWords * 32 >= (int)kBdIn && kBdHash == 2048, "what takes the tables' place fits");
static_assert((kBdInWords + kBdTabWords + 2 * kBdBitWords + 32) * 4 <= 160 * 1024, "one workgroup's LDS");
static_assert(kBdIn % 64 == 0 && kBdIn / 64 <= kBdThreads, "64 positions a thread in pass C");
static_assert(kBdWays == 16 && kBdRound == 256, "the packing of the table's and the round's cells");

struct BlockDesc { int64_t src; uint32_t len; uint32_t pad; };

// the four bytes at byte address a of an LDS word array (any alignment)
__device__ __forceinline__ uint32_t ld32(const uint32_t *w, uint32_t a)
{
    const uint32_t i = a >> 2;
    const uint64_t v = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
    return (uint32_t)(v >> ((a & 3u) * 8u));
}

__device__ __forceinline__ uint32_t hash_of(uint32_t four) { return (four * 2654435761u) >> (32 - kBdHashBits); }

__device__ __forceinline__ uint32_t rev_bits(uint32_t x, uint32_t n) { return __brev(x) >> (32u - n); }

// A symbol's bits in the fixed code, first bit lowest (Huffman codes are packed from their most significant bit: reversed here; extra
// bits from their least significant).  Returns the number of bits: 8-9 for a literal, 12-31 for a match.
__device__ __forceinline__ uint32_t literal_bits(uint32_t b, uint32_t &bits)
{
    if (b < 144u) { bits = rev_bits(0x30u + b, 8u); return 8u; }
    bits = rev_bits(0x190u + (b - 144u), 9u);
    return 9u;
}
__device__ __forceinline__ uint32_t match_bits(uint32_t len, uint32_t dist, uint32_t &bits)
{
    // length 3..258 -> symbol 257..285 and its extra bits
    const uint32_t l = len - 3u;
    uint32_t sym, le = 0u, lx = 0u;
    if (len == 258u) sym = 285u;
    else if (l < 8u) sym = 257u + l;
    else { le = (31u - (uint32_t)__clz((int)l)) - 2u; sym = 261u + 4u * le + ((l >> le) & 3u); lx = l & ((1u << le) - 1u); }
    uint32_t n;
    if (sym <= 279u) { bits = rev_bits(sym - 256u, 7u); n = 7u; } else { bits = rev_bits(0xC0u + (sym - 280u), 8u); n = 8u; }
    bits |= lx << n; n += le;
    // distance 1..32768 -> symbol 0..29 (five bits) and its extra bits
    const uint32_t d = dist - 1u;
    uint32_t ds, de = 0u, dx = 0u;
    if (d < 4u) ds = d;
    else { de = (31u - (uint32_t)__clz((int)d)) - 1u; ds = 2u * de + 2u + ((d >> de) & 1u); dx = d & ((1u << de) - 1u); }
    bits |= rev_bits(ds, 5u) << n; n += 5u;
    bits |= dx << n; n += de;
    return n;
}

}  // namespace

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

__global__ __launch_bounds__(kBdThreads) void bgzf_deflate_kernel(
    const uint8_t *__restrict__ data, const BlockDesc *__restrict__ desc, int64_t n_blocks, uint8_t *__restrict__ staging,
    uint32_t *__restrict__ bsize, uint32_t *__restrict__ match_rows)
{
    BVC_POISON_LDS();
    __shared__ __attribute__((aligned(16))) uint32_t s_in[kBdInWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kBdTabWords];
    __shared__ uint32_t s_first[kBdBitWords];
    __shared__ uint32_t s_path[kBdBitWords];
    __shared__ uint32_t s_scan[32];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t *const match = match_rows + (size_t)blockIdx.x * kBdIn;
    uint32_t *const s_out = s_in;                                             // pass C
    uint8_t *const s_sym = reinterpret_cast<uint8_t *>(s_tab);               // passes B and C: the literal, or length - 3
    uint32_t *const s_ism = s_first;                                          // passes B and C: bit p = position p holds a match

    for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {       // (workgroup-uniform)
        const uint32_t n = desc[blk].len < kBdIn ? desc[blk].len : kBdIn;
        uint8_t *const slot = staging + (size_t)blk * kBdSlot;
        if (n == 0u) {
            if (tid == 0u) bsize[blk] = 0u;
            continue;
        }
        const uint8_t *__restrict__ src = data + desc[blk].src;
        // ---- the input (bytes behind it read as zero), empty tables.  LDS word w = the block's bytes 4 w .. 4 w + 3, from the two aligned
        // words of global memory that hold them: the source starts at any byte, and an aligned word is read only where it holds a byte
        // of the block (it then lies in the block's page)
        {
            const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u);
            const uint32_t *__restrict__ g = reinterpret_cast<const uint32_t *>(src - head);      // word j: the block's bytes 4 j - head ..
            for (uint32_t w = tid; w < (uint32_t)kBdInWords; w += kBdThreads) {
                uint32_t v = 0u;
                if (4u * w < n) {
                    const uint32_t lo = g[w];                                                     // (holds byte 4 w of the block)
                    const uint32_t hi = head != 0u && 4u * (w + 1u) < n + head ? g[w + 1u] : 0u;   // (its first byte is byte 4 w + 4 - head)
                    v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * head));
                    const uint32_t left = n - 4u * w;
                    if (left < 4u) v &= (1u << (8u * left)) - 1u;
                }
                s_in[w] = v;
            }
        }
        for (uint32_t w = tid; w < (uint32_t)kBdTabWords; w += kBdThreads) s_tab[w] = 0u;
        for (uint32_t w = tid; w < (uint32_t)kBdBitWords; w += kBdThreads) s_first[w] = 0u;
        __syncthreads();

        // ---- A: matches
        const uint32_t sub = tid & (kBdLanes - 1), slotpos = tid / kBdLanes;
        const uint32_t rounds = (n + kBdRound - 1) / kBdRound;
        uint32_t prev_h = 0u, prev_p = 0u;
        bool prev_ok = false;
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t p = r * kBdRound + slotpos;
            const bool ok = p + 4u <= n;                                      // four bytes to hash
            const uint32_t four = ok ? ld32(s_in, p) : 0u;
            const uint32_t h = hash_of(four);                                // (below kBdHash by the shift)
            if (sub == 0u) {
                // the round before into its way, this round's first positions
                if (prev_ok && BVC_LDS_OK(0x901, prev_h, kBdHash)) {
                    const uint32_t way = (r - 1u) & (kBdWays - 1u);
                    uint32_t *const cell = &s_tab[(way & 7u) * kBdHash + prev_h];
                    const uint32_t cur = *cell;
                    atomicMax(cell, way >> 3 ? (cur & 0xFFFFu) | ((prev_p + 1u) << 16) : (cur & 0xFFFF0000u) | (prev_p + 1u));
                }
                if (ok && BVC_LDS_OK(0x902, h, kBdHash)) atomicMax(&s_first[h], ((r + 1u) << 8) | (255u - slotpos));
            }
            __syncthreads();
            uint32_t best = 0u, best_d = 0u;
            if (ok) {
                const uint32_t mx = n - p < kBdMaxMatch ? n - p : kBdMaxMatch;
                auto consider = [&](uint32_t q) {                             // q < p: a candidate's position
                    const uint32_t d = p - q;
                    if (d > kBdMaxDist || best == mx) return;
                    // it can only win if it also matches where the best so far ends
                    if (best >= kBdMinMatch && ld32(s_in, q + best - 3u) != ld32(s_in, p + best - 3u)) return;
                    uint32_t l = 0u;
                    while (l < mx) {
                        const uint32_t x = ld32(s_in, q + l) ^ ld32(s_in, p + l);
                        if (x != 0u) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
                        l += 4u;
                    }
                    l = l < mx ? l : mx;
                    if (l > best) { best = l; best_d = d; }
                };
#pragma unroll
                for (uint32_t k = 0; k < (uint32_t)kBdWaysPerLane; ++k) {
                    const uint32_t way = sub * kBdWaysPerLane + k;
                    const uint32_t cell = s_tab[(way & 7u) * kBdHash + h];
                    const uint32_t q1 = way >> 3 ? cell >> 16 : cell & 0xFFFFu;      // position + 1; 0 = none
                    if (q1 != 0u && q1 - 1u < p && BVC_LDS_OK(0x903, q1 - 1u, kBdIn)) consider(q1 - 1u);
                }
                if (sub == 0u) {
                    const uint32_t f = s_first[h];
                    const uint32_t q = r * kBdRound + 255u - (f & 255u);
                    if ((f >> 8) == r + 1u && q < p && BVC_LDS_OK(0x904, q, kBdIn)) consider(q);
                }
            }
            // the quad's longest match, the nearest among equals
            uint32_t key = best >= kBdMinMatch ? (best << 16) | (kBdMaxDist - best_d) : 0u;
#pragma unroll
            for (int d = 1; d < kBdLanes; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)key, d);
                key = o > key ? o : key;
            }
            if (sub == 0u && p < n)
                match[p] = key != 0u ? kBdMatchBit | (((key >> 16) - 3u) << 16) | (kBdMaxDist - (key & 0xFFFFu) - 1u) : 0u;
            prev_h = h; prev_p = p; prev_ok = ok;
            __syncthreads();                                                  // the tables belong to the next round's writers from here
        }
        __threadfence();                                                      // the match row: written here, read below by other wavefronts
        __syncthreads();

        // ---- B: a byte and a bit a position in the tables' place (32 positions a thread and trip), then the path
        for (uint32_t g = tid; g < kBdIn / 32u; g += kBdThreads) {
            uint32_t ism = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j) {
                const uint32_t p0 = 32u * g + 4u * j;
                uint32_t packed = 0u;
                if (p0 < n) {
                    const uint4 m4 = *reinterpret_cast<const uint4 *>(match + p0);     // (the row is 16-byte aligned, p0 a multiple of 4)
                    const uint32_t m[4] = {m4.x, m4.y, m4.z, m4.w};
                    const uint32_t lit = s_in[p0 >> 2];
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) {
                        const bool is = p0 + k < n && (m[k] & kBdMatchBit) != 0u;
                        ism |= is ? 1u << (4u * j + k) : 0u;
                        packed |= (is ? (m[k] >> 16) & 0xFFu : (lit >> (8u * k)) & 0xFFu) << (8u * k);
                    }
                }
                s_tab[8u * g + j] = packed;                                   // (reads of s_tab ended with pass A)
            }
            s_ism[g] = ism;
            s_path[g] = 0u;
        }
        __syncthreads();
        if (tid == 0u) {
            // the greedy parse: literals up to the window's next match in one step, a match by its length
            uint32_t p = 0u;
            while (p < n) {
                const uint32_t w = p >> 5, b = p & 31u;
                const uint32_t m = s_ism[w] >> b;                             // (w < kBdIn / 32: p < n)
                if (m == 0u) { s_path[w] |= ~0u << b; p = (w + 1u) << 5; continue; }
                const uint32_t k = (uint32_t)__builtin_ctz(m);               // literals p .. p + k - 1, then the match
                s_path[w] |= (((1u << k) - 1u) | (1u << k)) << b;
                p += k;
                p += (uint32_t)s_sym[p] + 3u;
            }
        }
        __syncthreads();

        // ---- C: bits.  Thread t: positions 64 t .. 64 t + 63 (path bits behind n may be set by the last window: masked here)
        uint32_t my_bits = 0u;
        uint64_t mask = 0u;
        const uint32_t base = 64u * tid;
        if (base < n) {
            mask = (uint64_t)s_path[2u * tid] | ((uint64_t)s_path[2u * tid + 1u] << 32);
            if (n - base < 64u) mask &= (1ull << (n - base)) - 1ull;
            const uint64_t ism = (uint64_t)s_ism[2u * tid] | ((uint64_t)s_ism[2u * tid + 1u] << 32);
            for (uint64_t left = mask; left != 0u; left &= left - 1u) {
                const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
                uint32_t bits;
                my_bits += (ism >> (p - base)) & 1u ? match_bits((uint32_t)s_sym[p] + 3u, (match[p] & 0x7FFFu) + 1u, bits)
                                                   : literal_bits(s_sym[p], bits);
            }
        }
        // exclusive scan over the workgroup
        uint32_t incl = my_bits;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
            incl += lane >= (uint32_t)d ? o : 0u;
        }
        if (lane == kWave - 1) s_scan[wave] = incl;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t v = 0; v < kBdThreads / kWave; ++v) {
            const uint32_t s = s_scan[v];
            before += v < wave ? s : 0u;
            all += s;
        }
        const uint32_t total_bits = 3u + all + 7u;                           // block header, symbols, end of block
        const uint32_t coded = (total_bits + 7u) >> 3;
        const bool stored = coded > n + 5u;                                   // (workgroup-uniform)
        const uint32_t csize = stored ? n + 5u : coded;
        const uint32_t out_words = (csize + 3u) >> 2;                         // <= (65280 + 5 + 3) / 4 < kBdInWords
        if (!stored) {
            // (the input's last readers were pass B's: its place takes the image)
            for (uint32_t w = tid; w < out_words; w += kBdThreads) s_out[w] = 0u;
            __syncthreads();
            if (base < n) {
                uint32_t at = 3u + before + incl - my_bits;                   // this thread's first bit
                uint32_t word = at >> 5, fill = at & 31u;
                uint64_t acc = tid == 0u ? 3u : 0u;                           // BFINAL = 1, BTYPE = 01 in front of thread 0's symbols
                const uint64_t ism = (uint64_t)s_ism[2u * tid] | ((uint64_t)s_ism[2u * tid + 1u] << 32);
                for (uint64_t left = mask; left != 0u; left &= left - 1u) {
                    const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
                    uint32_t bits;
                    const uint32_t nb = (ism >> (p - base)) & 1u ? match_bits((uint32_t)s_sym[p] + 3u, (match[p] & 0x7FFFu) + 1u, bits)
                                                                : literal_bits(s_sym[p], bits);
                    acc |= (uint64_t)bits << fill;
                    fill += nb;
                    if (fill >= 32u) {
                        if (BVC_LDS_OK(0x905, word, out_words)) atomicOr(&s_out[word], (uint32_t)acc);
                        acc >>= 32; fill -= 32u; ++word;
                    }
                }
                if (acc != 0u && BVC_LDS_OK(0x906, word, out_words)) atomicOr(&s_out[word], (uint32_t)acc);
                // (the end-of-block symbol is seven zero bits: already there)
            }
            __syncthreads();
        }
        // ---- the block: header, deflate data, CRC32 (zero here: bgzf_crc_kernel), ISIZE -- in aligned words (the slot is 64 KiB aligned;
        // the bytes behind the block up to its last word's end are written too).  A word inside the deflate data is four bytes of the
        // image (or of the input, five bytes behind the stored block's own header) at an odd offset; the others are put together byte by byte
        const uint32_t bs = csize + 26u;
        {
            auto byte_at = [&](uint32_t x) -> uint32_t {                      // byte x of the block
                if (x < 18u) {
                    // 1f 8b 08 04 | mtime 0 | xfl 0, os ff, xlen 6 | 'B' 'C', 2 | BSIZE - 1
                    const uint32_t word = x < 4u ? 0x04088b1fu : x < 8u ? 0u : x < 12u ? 0x0006ff00u : x < 16u ? 0x00024342u : (bs - 1u) & 0xFFFFu;
                    return (word >> (8u * (x & 3u))) & 0xFFu;
                }
                const uint32_t i = x - 18u;
                if (i < csize) {
                    if (!stored) return (s_out[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
                    // BFINAL = 1, BTYPE = 00 | LEN | NLEN, then the input
                    if (i < 5u) return ((i < 4u ? 0x01u | (n << 8) | ((~n & 0xFFu) << 24) : (~n >> 8) & 0xFFu) >> (8u * (i & 3u))) & 0xFFu;
                    return (s_in[(i - 5u) >> 2] >> (8u * ((i - 5u) & 3u))) & 0xFFu;
                }
                const uint32_t t = i - csize;                                 // the trailer
                return t >= 4u && t < 8u ? (n >> (8u * (t - 4u))) & 0xFFu : 0u;
            };
            uint32_t *const slot32 = reinterpret_cast<uint32_t *>(slot);
            const uint32_t first = stored ? 23u : 18u;                        // where the bytes of s_in / s_out begin
            for (uint32_t k = tid; 4u * k < bs; k += kBdThreads) {
                uint32_t v;
                if (4u * k >= first && 4u * k + 4u <= 18u + csize) v = ld32(stored ? s_in : s_out, 4u * k - first);
                else v = byte_at(4u * k) | (byte_at(4u * k + 1u) << 8) | (byte_at(4u * k + 2u) << 16) | (byte_at(4u * k + 3u) << 24);
                slot32[k] = v;
            }
        }
        if (tid == 0u) bsize[blk] = bs;
        __syncthreads();                                                      // the LDS belongs to the next block from here
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
    s.desc = L.take<char>(nb * sizeof(BlockDesc));
    s.bsize = L.take<uint32_t>(nb);
    s.match_rows = L.take<uint32_t>(grid * kBdIn);
    s.staging = L.take<uint8_t>(nb * kBdSlot);
    if (sized) *sized = L;
    return s;
}

hipError_t launch_bgzf_deflate(hipStream_t stream, int64_t n_pieces, const uint8_t *data, const int64_t *piece_off, const int64_t *piece_len,
                               int64_t n_blocks, const BgzfDeflateScratch &s, uint8_t *comp, int64_t comp_cap, int64_t *comp_off)
{
    BlockDesc *const desc = reinterpret_cast<BlockDesc *>(s.desc);
    if (n_blocks > 0) {
        const unsigned grid = (unsigned)(n_blocks < kBgzfDeflateGrid ? n_blocks : kBgzfDeflateGrid);
        hipLaunchKernelGGL(bgzf_plan_kernel, dim3((unsigned)((n_blocks + 255) / 256 < 1024 ? (n_blocks + 255) / 256 : 1024)), dim3(256), 0, stream,
                           n_pieces, piece_off, piece_len, s.first_block, n_blocks, desc);
        hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid), dim3(kBdThreads), 0, stream, data, desc, n_blocks, s.staging, s.bsize, s.match_rows);
        const uintptr_t a = reinterpret_cast<uintptr_t>(data);
        hipLaunchKernelGGL(bgzf_crc_kernel, dim3((unsigned)(n_blocks < 65536 ? n_blocks : 65536)), dim3(kWave), 0, stream,
                           reinterpret_cast<const uint8_t *>(a & ~(uintptr_t)15), (uint32_t)(a & 15u), desc, n_blocks, s.bsize, s.staging);
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
