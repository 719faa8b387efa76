// bgzf_deflate_device.h -- what every instantiation of the device deflate encoder's block kernel runs (bgzf_block_kernel.h): the layout of a
// workgroup's LDS, the input's way into it, passes A (matches) and B (path), the fixed code, the workgroup scan of pass C and the
// block's way out to its staging slot.  The passes are described at the top of bgzf_deflate_kernel.hip.  Every function is inlined into its kernel; all of a workgroup's 1024 threads call each of them.
#pragma once
#include "bvc_device.h"
#include "bvc_internal.h"

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

// the four bytes at byte address a of an LDS word array (any alignment)
__device__ __forceinline__ uint32_t ld32(const uint32_t *w, uint32_t a)
{
    const uint32_t i = a >> 2;
    const uint64_t v = (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
    return (uint32_t)(v >> ((a & 3u) * 8u));
}

__device__ __forceinline__ uint32_t hash_of(uint32_t four) { return (four * 2654435761u) >> (32 - kBdHashBits); }

__device__ __forceinline__ uint32_t rev_bits(uint32_t x, uint32_t n) { return __brev(x) >> (32u - n); }

// length 3..258 -> symbol 257..285, the number of its extra bits and their value; distance 1..32768 -> symbol 0..29 likewise
__device__ __forceinline__ uint32_t length_symbol(uint32_t len, uint32_t &le, uint32_t &lx)
{
    const uint32_t l = len - 3u;
    uint32_t sym;
    le = 0u; lx = 0u;
    if (len == 258u) sym = 285u;
    else if (l < 8u) sym = 257u + l;
    else { le = (31u - (uint32_t)__clz((int)l)) - 2u; sym = 261u + 4u * le + ((l >> le) & 3u); lx = l & ((1u << le) - 1u); }
    return sym;
}
__device__ __forceinline__ uint32_t distance_symbol(uint32_t dist, uint32_t &de, uint32_t &dx)
{
    const uint32_t d = dist - 1u;
    uint32_t ds;
    de = 0u; dx = 0u;
    if (d < 4u) ds = d;
    else { de = (31u - (uint32_t)__clz((int)d)) - 1u; ds = 2u * de + 2u + ((d >> de) & 1u); dx = d & ((1u << de) - 1u); }
    return ds;
}

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
    uint32_t le, lx;
    const uint32_t sym = length_symbol(len, le, lx);
    uint32_t n;
    if (sym <= 279u) { bits = rev_bits(sym - 256u, 7u); n = 7u; } else { bits = rev_bits(0xC0u + (sym - 280u), 8u); n = 8u; }
    bits |= lx << n; n += le;
    uint32_t de, dx;
    const uint32_t ds = distance_symbol(dist, de, dx);                       // five bits
    bits |= rev_bits(ds, 5u) << n; n += 5u;
    bits |= dx << n; n += de;
    return n;
}

// ---- the input (bytes behind it read as zero), empty tables.  LDS word w = the block's bytes 4 w .. 4 w + 3, from the two aligned
// words of global memory that hold them: the source starts at any byte, and an aligned word is read only where it holds a byte
// of the block (it then lies in the block's page)
__device__ __forceinline__ void bd_load(uint32_t *s_in, uint32_t *s_tab, uint32_t *s_first, const uint8_t *__restrict__ src, uint32_t n, uint32_t tid)
{
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
}

// ---- A: matches
__device__ __forceinline__ void bd_matches(const uint32_t *s_in, uint32_t *s_tab, uint32_t *s_first, uint32_t *match, uint32_t n, uint32_t tid)
{
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
}

// ---- B: a byte and a bit a position in the tables' place (32 positions a thread and trip), then the path
__device__ __forceinline__ void bd_path(const uint32_t *s_in, uint32_t *s_tab, uint32_t *s_ism, uint32_t *s_path, const uint32_t *match, uint32_t n,
                                        uint32_t tid)
{
    const uint8_t *const s_sym = reinterpret_cast<const uint8_t *>(s_tab);
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
}

// ---- C, shared parts.  Thread t: positions 64 t .. 64 t + 63 (path bits behind n may be set by the last window: masked here)
__device__ __forceinline__ uint64_t bd_my_symbols(const uint32_t *s_path, uint32_t n, uint32_t tid)
{
    uint64_t mask = 0u;
    const uint32_t base = 64u * tid;
    if (base < n) {
        mask = (uint64_t)s_path[2u * tid] | ((uint64_t)s_path[2u * tid + 1u] << 32);
        if (n - base < 64u) mask &= (1ull << (n - base)) - 1ull;
    }
    return mask;
}

// the bits of this thread's symbols in the fixed code
__device__ __forceinline__ uint32_t bd_fixed_bits(const uint8_t *s_sym, const uint32_t *s_ism, const uint32_t *match, uint64_t mask, uint32_t n,
                                                  uint32_t tid)
{
    uint32_t my_bits = 0u;
    const uint32_t base = 64u * tid;
    if (base < n) {
        const uint64_t ism = (uint64_t)s_ism[2u * tid] | ((uint64_t)s_ism[2u * tid + 1u] << 32);
        for (uint64_t left = mask; left != 0u; left &= left - 1u) {
            const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
            uint32_t bits;
            my_bits += (ism >> (p - base)) & 1u ? match_bits((uint32_t)s_sym[p] + 3u, (match[p] & 0x7FFFu) + 1u, bits)
                                               : literal_bits(s_sym[p], bits);
        }
    }
    return my_bits;
}

// exclusive scan over the workgroup: the sum over the threads in front of this one, and the sum over all
__device__ __forceinline__ uint32_t bd_scan(uint32_t my_bits, uint32_t *s_scan, uint32_t lane, uint32_t wave, uint32_t &all)
{
    uint32_t incl = my_bits;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d);
        incl += lane >= (uint32_t)d ? o : 0u;
    }
    if (lane == kWave - 1) s_scan[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
    all = 0u;
#pragma unroll
    for (uint32_t v = 0; v < kBdThreads / kWave; ++v) {
        const uint32_t s = s_scan[v];
        before += v < wave ? s : 0u;
        all += s;
    }
    return before + incl - my_bits;
}

// this thread's symbols in the fixed code into the image, from bit `at` on (BFINAL and BTYPE in front of thread 0's)
__device__ __forceinline__ void bd_fixed_write(uint32_t *s_out, uint32_t out_words, const uint8_t *s_sym, const uint32_t *s_ism, const uint32_t *match,
                                               uint64_t mask, uint32_t at, uint32_t n, uint32_t tid)
{
    const uint32_t base = 64u * tid;
    (void)out_words;                                                  // (read by the diagnostic build's checks only)
    if (base < n) {
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
}

// ---- the block: header, deflate data, CRC32 (zero here: bgzf_crc_kernel), ISIZE -- in aligned words (the slot is 64 KiB aligned;
// the bytes behind the block up to its last word's end are written too).  A word inside the deflate data is four bytes of the
// image (or of the input, five bytes behind the stored block's own header) at an odd offset; the others are put together byte by byte.
// Returns the block's size.
__device__ __forceinline__ uint32_t bd_write_slot(uint8_t *slot, const uint32_t *s_in, const uint32_t *s_out, uint32_t n, uint32_t csize, bool stored,
                                                  uint32_t tid)
{
    const uint32_t bs = csize + 26u;
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
    return bs;
}

// ---- C for the fixed code, whole: the block behind pass B (whichever parse filled the match row) into its slot, fixed or stored.
// s_out = s_in (the image takes the input's place), s_sym = the bytes of s_tab, s_ism = s_first.  Returns the block's size.
__device__ __forceinline__ uint32_t bd_fixed_block(uint8_t *slot, uint32_t *s_in, const uint32_t *s_tab, const uint32_t *s_ism, const uint32_t *s_path,
                                                   uint32_t *s_scan, const uint32_t *match, uint32_t n, uint32_t tid)
{
    const uint32_t lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t *const s_out = s_in;
    const uint8_t *const s_sym = reinterpret_cast<const uint8_t *>(s_tab);
    const uint64_t mask = bd_my_symbols(s_path, n, tid);
    const uint32_t my_bits = bd_fixed_bits(s_sym, s_ism, match, mask, n, tid);
    uint32_t all;
    const uint32_t before = bd_scan(my_bits, s_scan, lane, wave, all);
    const uint32_t total_bits = 3u + all + 7u;                           // block header, symbols, end of block
    const uint32_t coded = (total_bits + 7u) >> 3;
    const bool stored = coded > n + 5u;                                   // (workgroup-uniform)
    const uint32_t csize = stored ? n + 5u : coded;
    const uint32_t out_words = (csize + 3u) >> 2;                         // <= (65280 + 5 + 3) / 4 < kBdInWords
    if (!stored) {
        // (the input's last readers were pass B's: its place takes the image)
        for (uint32_t w = tid; w < out_words; w += kBdThreads) s_out[w] = 0u;
        __syncthreads();
        bd_fixed_write(s_out, out_words, s_sym, s_ism, match, mask, 3u + before, n, tid);     // this thread's first bit
        __syncthreads();
    }
    return bd_write_slot(slot, s_in, s_out, n, csize, stored, tid);
}

}  // namespace

}  // namespace bvc
