// bgzf_fields_device.h -- the field parse of the device deflate encoder (tuning key "bgzf_parse" = 1; docs/BGZF_FIELDS.md holds the rule,
// tests/bgzf_fields_model.py its plain Python copy): bd_field_matches fills the match row that bd_matches of bgzf_deflate_device.h fills
// for the general parse, in the same format, so that pass B and everything behind it run as they are.
//
// The text is fields ended by one of two bytes: a tab or a colon, or with tuning key "bgzf_cuts" = 1 a space or a newline (kBfDelimsTabColon,
// kBfDelimsSpaceNewline; the pair is a kernel argument).  Two bitmaps of one bit a position say where a field starts (CUTS; bit n, the block's
// end, is set too) and which fields are no byte-for-byte repeat of the field in front of them (HEADS).  A repeat's match is the run it
// stands in, at the distance of one field: nothing is searched.  A head of 4..32 bytes looks its key -- a hash of its length and bytes --
// up in pass A's tables, which only such heads enter: rounds of 256 positions, way (r mod 16) = the largest position of an earlier round
// r' = r (mod 16) with the key, and the first position of the round itself.  Four lanes a position: a keyed head is four bytes at least,
// so the lanes of the three positions behind it, which start nothing, join its own -- sixteen lanes, a candidate each (one of them two).
// A candidate that holds the whole field is extended sixteen bytes a step and cut back to the last cut it reaches; the head's lanes
// meet in an atomicMax of (length, nearness).  Every other position has no match.
// Every scan of a bitmap covers 259 bits at the most; every LDS index that comes from data is bounded before use.
#pragma once
#include "bgzf_deflate_device.h"

namespace bvc {

namespace {

constexpr uint32_t kBfMinKeyed = 4, kBfMaxKeyed = 32;    // the lengths of the heads that have a key
constexpr uint32_t kBfNone = 0xFFFFFFFFu;
constexpr uint32_t kBfDelimsTabColon = 0x09u | (0x3Au << 8), kBfDelimsSpaceNewline = 0x20u | (0x0Au << 8);   // the two bytes that end a field

__device__ __forceinline__ bool bf_bit(const uint32_t *bm, uint32_t p)
{
    return BVC_LDS_OK(0x931, p >> 5, kBdBitWords) && ((bm[p >> 5] >> (p & 31u)) & 1u) != 0u;
}

// the smallest set bit q with from <= q < from + span, or kBfNone.  from + span <= 32 kBdBitWords
__device__ __forceinline__ uint32_t bf_next(const uint32_t *bm, uint32_t from, uint32_t span)
{
    const uint32_t end = from + span;
    uint32_t w = from >> 5;
    if (span == 0u || !BVC_LDS_OK(0x932, (end - 1u) >> 5, kBdBitWords)) return kBfNone;
    uint32_t m = bm[w] & (~0u << (from & 31u));
    for (;;) {
        if (m != 0u) {
            const uint32_t q = (w << 5) + (uint32_t)__builtin_ctz(m);
            return q < end ? q : kBfNone;
        }
        ++w;
        if ((w << 5) >= end) return kBfNone;
        m = bm[w];                                                       // (w <= (end - 1) >> 5)
    }
}

// the largest set bit q with from - span < q <= from, or kBfNone.  span <= from + 1
__device__ __forceinline__ uint32_t bf_prev(const uint32_t *bm, uint32_t from, uint32_t span)
{
    uint32_t w = from >> 5;
    if (span == 0u || span > from + 1u || !BVC_LDS_OK(0x933, w, kBdBitWords)) return kBfNone;
    const uint32_t lo = from + 1u - span;
    uint32_t m = bm[w] & (~0u >> (31u - (from & 31u)));
    for (;;) {
        if (m != 0u) {
            const uint32_t q = (w << 5) + 31u - (uint32_t)__builtin_clz(m);
            return q >= lo ? q : kBfNone;
        }
        if ((w << 5) <= lo) return kBfNone;
        --w;
        m = bm[w];                                                       // (w >= lo >> 5)
    }
}

// the length of the field that starts at cut p < n: 1 .. 258, or 259 for every longer one
__device__ __forceinline__ uint32_t bf_field_len(const uint32_t *s_cut, uint32_t p, uint32_t n)
{
    const uint32_t q = bf_next(s_cut, p + 1u, n - p < kBdMaxMatch ? n - p : kBdMaxMatch);     // (bit n is set)
    return q != kBfNone ? q - p : kBdMaxMatch + 1u;
}

// x[a .. a + len) == x[b .. b + len)
__device__ __forceinline__ bool bf_same(const uint32_t *s_in, uint32_t a, uint32_t b, uint32_t len)
{
    for (uint32_t i = 0; i < len; i += 4u) {
        uint32_t x = ld32(s_in, a + i) ^ ld32(s_in, b + i);
        if (len - i < 4u) x &= (1u << (8u * (len - i))) - 1u;
        if (x != 0u) return false;
    }
    return true;
}

// the bytes x[a ..] and x[b ..] share, sixteen at the most.  (a, b + 19 < 4 kBdInWords)
__device__ __forceinline__ uint32_t bf_diff16(const uint32_t *s_in, uint32_t a, uint32_t b)
{
    const uint32_t ia = a >> 2, ib = b >> 2, sa = (a & 3u) * 8u, sb = (b & 3u) * 8u;
    uint32_t wa[5], wb[5];
#pragma unroll
    for (uint32_t k = 0; k < 5u; ++k) { wa[k] = s_in[ia + k]; wb[k] = s_in[ib + k]; }
    uint32_t at = 16u;
#pragma unroll
    for (uint32_t k = 4u; k-- > 0u;) {
        const uint32_t va = (uint32_t)((((uint64_t)wa[k + 1u] << 32) | wa[k]) >> sa), vb = (uint32_t)((((uint64_t)wb[k + 1u] << 32) | wb[k]) >> sb);
        const uint32_t x = va ^ vb;
        at = x != 0u ? 4u * k + ((uint32_t)__builtin_ctz(x) >> 3) : at;
    }
    return at;
}

// the key of a head: its length and its bytes, four at a time (the last word's bytes behind the field read as zero)
__device__ __forceinline__ uint32_t bf_key(const uint32_t *s_in, uint32_t p, uint32_t len)
{
    uint32_t h = len;
    for (uint32_t i = 0; i < len; i += 4u) {
        uint32_t w = ld32(s_in, p + i);
        if (len - i < 4u) w &= (1u << (8u * (len - i))) - 1u;
        h = (h ^ w) * 2654435761u;
        h ^= h >> 15;
    }
    return h >> (32 - kBdHashBits);
}

// ---- A for the field parse.  s_cut lies in s_path's place (pass B clears it behind this); s_head and s_best (a word a position of a
// round: the best match of the head there) are this parse's own.
__device__ __forceinline__ void bd_field_matches(const uint32_t *s_in, uint32_t *s_tab, uint32_t *s_first, uint32_t *s_cut, uint32_t *s_head,
                                                 uint32_t *s_best, uint32_t *match, uint32_t n, uint32_t tid, uint32_t delims)
{
    // cuts: position p starts a field iff p = 0 or byte p - 1 is one of the two delimiters (the bytes behind the block read as zero); bit n
    const uint32_t d0 = delims & 0xFFu, d1 = (delims >> 8) & 0xFFu;
    for (uint32_t g = tid; g < (uint32_t)kBdBitWords; g += kBdThreads) {
        uint32_t delim = 0u;                                              // bit j: byte 32 g + j ends a field
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            const uint32_t w = s_in[8u * g + j];                          // (8 g + j < kBdInWords)
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t b = (w >> (8u * k)) & 0xFFu;
                delim |= (b == d0 || b == d1 ? 1u : 0u) << (4u * j + k);
            }
        }
        const uint32_t before = g != 0u ? s_in[8u * g - 1u] >> 24 : d0;
        uint32_t cuts = (delim << 1) | (before == d0 || before == d1 ? 1u : 0u);
        if ((n >> 5) == g) cuts |= 1u << (n & 31u);
        s_cut[g] = cuts;
    }
    __syncthreads();
    // heads: the fields that are no repeat of the field in front of them.  (A field of more than 258 bytes is marked a head whatever
    // lies in front of it: neither class has a match at that length, and a run of such fields ends at a head either way)
    for (uint32_t g = tid; g < (uint32_t)kBdBitWords; g += kBdThreads) {
        uint32_t heads = 0u;
        for (uint32_t left = s_cut[g]; left != 0u; left &= left - 1u) {
            const uint32_t p = (g << 5) + (uint32_t)__builtin_ctz(left);
            if (p >= n) break;
            const uint32_t len = bf_field_len(s_cut, p, n);
            bool repeat = false;
            if (len <= kBdMaxMatch && p >= len && bf_prev(s_cut, p - 1u, len) == p - len) repeat = bf_same(s_in, p - len, p, len);
            heads |= repeat ? 0u : 1u << (p & 31u);
        }
        s_head[g] = heads;
    }
    __syncthreads();

    const uint32_t sub = tid & (kBdLanes - 1), slotpos = tid / kBdLanes;
    const uint32_t rounds = (n + kBdRound - 1) / kBdRound;
    uint32_t prev_h = 0u, prev_p = 0u;
    bool prev_ok = false;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t p = r * kBdRound + slotpos;
        const bool cut = p < n && bf_bit(s_cut, p), head = cut && bf_bit(s_head, p);
        const uint32_t len = cut ? bf_field_len(s_cut, p, n) : 0u;
        const bool ok = head && len >= kBfMinKeyed && len <= kBfMaxKeyed;    // a head with a key
        // A keyed head is four bytes at least: the three positions behind it start nothing, and their lanes look its candidates up with
        // its own -- c: the head this lane works for, of clen bytes; t: its number among that head's lanes, `team` of them in this round
        uint32_t c = kBfNone, clen = 0u, t = sub;
        if (ok) { c = p; clen = len; }
        else if (!cut && p < n && slotpos != 0u) {
            const uint32_t reach = slotpos < 3u ? slotpos : 3u;          // (the head lies in this round: its tables are this round's)
            const uint32_t q = bf_prev(s_cut, p, reach + 1u);
            if (q != kBfNone && q < p && bf_bit(s_head, q)) {
                const uint32_t ql = bf_field_len(s_cut, q, n);
                if (ql >= kBfMinKeyed && ql <= kBfMaxKeyed) { c = q; clen = ql; t = (p - q) * kBdLanes + sub; }
            }
        }
        const uint32_t h = c != kBfNone ? bf_key(s_in, c, clen) : 0u;    // (below kBdHash by the shift)
        if (sub == 0u) {
            // the round before into its way, this round's first positions: as pass A of the general parse
            if (prev_ok && BVC_LDS_OK(0x934, prev_h, kBdHash)) {
                const uint32_t way = (r - 1u) & (kBdWays - 1u);
                uint32_t *const cell = &s_tab[(way & 7u) * kBdHash + prev_h];
                const uint32_t cur = *cell;
                atomicMax(cell, way >> 3 ? (cur & 0xFFFFu) | ((prev_p + 1u) << 16) : (cur & 0xFFFF0000u) | (prev_p + 1u));
            }
            if (ok && BVC_LDS_OK(0x935, h, kBdHash)) atomicMax(&s_first[h], ((r + 1u) << 8) | (255u - slotpos));
            s_best[slotpos] = 0u;                                         // (its last reader was this lane, in the round before)
        }
        __syncthreads();
        uint32_t best = 0u, best_d = 0u;
        if (c != kBfNone) {
            const uint32_t cslot = c - r * kBdRound;
            const uint32_t team = (uint32_t)kBdLanes * ((uint32_t)kBdRound - cslot < 4u ? (uint32_t)kBdRound - cslot : 4u);
            const uint32_t mx = n - c < kBdMaxMatch ? n - c : kBdMaxMatch;
            // candidate i: way i of the table, i < 16; the round's own first head with the key, i = 16
            for (uint32_t i = t; i <= (uint32_t)kBdWays; i += team) {
                uint32_t q = kBfNone;
                if (i < (uint32_t)kBdWays) {
                    const uint32_t cell = BVC_LDS_OK(0x936, h, kBdHash) ? s_tab[(i & 7u) * kBdHash + h] : 0u;
                    const uint32_t q1 = i >> 3 ? cell >> 16 : cell & 0xFFFFu;    // position + 1; 0 = none
                    if (q1 != 0u) q = q1 - 1u;
                } else {
                    const uint32_t f = BVC_LDS_OK(0x938, h, kBdHash) ? s_first[h] : 0u;
                    if ((f >> 8) == r + 1u) q = r * kBdRound + 255u - (f & 255u);
                }
                if (q == kBfNone || q >= c || !BVC_LDS_OK(0x937, q, kBdIn)) continue;
                const uint32_t d = c - q;
                if (d > kBdMaxDist) continue;
                // it can only win, or tie, if it also matches where this lane's best so far ends
                if (best >= kBdMinMatch && ld32(s_in, q + best - 4u) != ld32(s_in, c + best - 4u)) continue;
                uint32_t l = 0u;
                while (l < mx) {                                          // sixteen bytes a step: five words of either side, read at once
                    const uint32_t x = bf_diff16(s_in, q + l, c + l);     // the first byte that differs, 16 = none
                    l += x;
                    if (x < 16u) break;
                }
                l = l < mx ? l : mx;
                if (l < clen) continue;                                   // another field with the key
                // back to the last cut at or before its end (c + clen is one, or the block's end)
                uint32_t end = c + l;
                if (!bf_bit(s_cut, end)) end = bf_prev(s_cut, end, l - clen + 1u);
                if (end == kBfNone) continue;
                l = end - c;
                if (l > best || (l == best && d < best_d)) { best = l; best_d = d; }
            }
            // the head's longest match, the nearest among equals: the largest key of its lanes
            if (best >= kBdMinMatch && BVC_LDS_OK(0x939, cslot, kBdRound)) atomicMax(&s_best[cslot], (best << 16) | (kBdMaxDist - best_d));
            best = 0u;
        } else if (cut && !head && sub == 0u) {
            // a repeat: the run up to the next head (or the block's end) at the distance of one field, in whole fields
            const uint32_t span = n - p < kBdMaxMatch ? n - p : kBdMaxMatch;
            const uint32_t e = bf_next(s_head, p + 1u, span);
            const uint32_t run = e != kBfNone ? e - p : span;
            if (len >= 1u && len <= kBdMaxMatch && len <= p) { best = run / len * len; best_d = len; }
        }
        __syncthreads();                                                  // the tables belong to the next round's writers from here
        if (sub == 0u && p < n) {
            const uint32_t key = ok ? s_best[slotpos] : best >= kBdMinMatch ? (best << 16) | (kBdMaxDist - best_d) : 0u;
            match[p] = key != 0u ? kBdMatchBit | (((key >> 16) - 3u) << 16) | (kBdMaxDist - (key & 0xFFFFu) - 1u) : 0u;
        }
        prev_h = ok ? h : 0u; prev_p = p; prev_ok = ok;
    }
    __threadfence();                                                      // the match row: written here, read below by other wavefronts
    __syncthreads();
}

}  // namespace

}  // namespace bvc
