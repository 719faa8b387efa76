// bgzf_codes_device.h -- the code-construction rule of the device deflate encoder's dynamic blocks (docs/BGZF_DYNAMIC.md; the plain
// Python copy is tests/bgzf_dynamic_model.py): code lengths from counts, the code-length sequence and its code, canonical codes, the
// sizes of a block in the dynamic and in the fixed code, and the bits of a dynamic block's header.
//
// ONE WAVEFRONT runs each function, all of its lanes calling it together (`nlanes` = 64).  The lanes share the sort; the dependent
// chains (the merge of the Huffman tree, depths, the repair, the sequence) are lane 0's: a few hundred LDS steps a block.  Every table
// lies in the caller's LDS (CodeTables): an array a thread indexes with data would become scratch memory.  Every index that comes from
// data is bounded before use.  Nothing here is HIP-only, so that a host program can walk the same code with nlanes = 1.
#pragma once
#include <stdint.h>

#include "bvc_device.h"

namespace bvc {

namespace {

constexpr uint32_t kDcLit = 286, kDcDist = 30, kDcMaxSyms = 288, kDcCl = 19, kDcRow = 320;
constexpr uint32_t kDcLitLimit = 15, kDcClLimit = 7;

struct CodeTables {
    uint32_t counts[kDcRow];                 // literal/length symbols 0..285 (end of block counted once), distance symbols at 286..315
    uint32_t codes[kDcRow];                  // the same symbols: canonical code, first bit lowest | length << 16
    uint32_t weight[kDcMaxSyms];             // the tree's internal nodes, in the order they are made
    uint16_t order[kDcMaxSyms];              // the used symbols by (count, symbol)
    uint16_t leaf_parent[kDcMaxSyms];        // of leaf order[k]: an internal node
    uint16_t node_parent[kDcMaxSyms];        // of an internal node, then its depth in its place
    uint32_t bl[16], next[16];               // symbols a length; the next code of a length
    uint32_t cl_counts[20], cl_codes[20];    // the code-length code's 19 symbols
    uint8_t len[kDcRow];                     // code lengths, indexed as counts
    uint8_t cl_len[20];
    uint8_t seq_sym[kDcRow], seq_extra[kDcRow];      // the code-length sequence: symbol 0..18, the value of its extra bits
    uint32_t n_seq, hlit, hdist, hclen;
    uint32_t header_bits;                    // HLIT .. the last symbol of the sequence (without BFINAL and BTYPE)
    uint32_t dyn_bits, fixed_bits;           // the whole block, end-of-block symbol included, in either code
    uint32_t pad;
};

#define BVC_DC __host__ __device__ __forceinline__
#ifdef __HIP_DEVICE_COMPILE__
#define BVC_DC_OK(id, value, limit) BVC_LDS_OK(id, value, limit)
#else
#define BVC_DC_OK(id, value, limit) ((uint32_t)(value) < (uint32_t)(limit))
#endif

// what one lane wrote to LDS is read by the others behind this
BVC_DC void dc_wave_sync()
{
#ifdef __HIP_DEVICE_COMPILE__
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#endif
}

BVC_DC uint32_t dc_rev(uint32_t x, uint32_t n) { return __builtin_bitreverse32(x) >> (32u - n); }

// the order in which the code-length code's lengths are written (RFC 1951, 3.2.7): 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
BVC_DC uint32_t dc_cl_order(uint32_t i)
{
    constexpr uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                           11ull << 50 | 4ull << 55;
    constexpr uint64_t b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? a >> (5u * i) : b >> (5u * (i - 12u))) & 31u);
}
BVC_DC uint32_t dc_cl_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
BVC_DC uint32_t dc_length_extra_bits(uint32_t sym) { return sym < 265u || sym >= 285u ? 0u : (sym - 261u) >> 2; }      // sym: 257..285
BVC_DC uint32_t dc_distance_extra_bits(uint32_t ds) { return ds < 4u ? 0u : (ds - 2u) >> 1; }
BVC_DC uint32_t dc_fixed_length(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }

// (a), (d): len[0 .. n) from counts[0 .. n), no length above limit.  n <= 288, 2^limit >= max(n, 2), the counts' sum below 2^24.
BVC_DC void dc_build_lengths(const uint32_t *counts, uint32_t n, uint32_t limit, uint8_t *len, CodeTables &t, uint32_t lane, uint32_t nlanes)
{
    uint32_t used = 0u;
    for (uint32_t q = 0; q < n; ++q) used += counts[q] != 0u ? 1u : 0u;       // (the same in every lane)
    // the used symbols by (count, symbol): a symbol's place is the number of those in front of it
    for (uint32_t s = lane; s < n; s += nlanes) {
        const uint32_t c = counts[s];
        len[s] = 0u;
        if (c != 0u) {
            uint32_t rank = 0u;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t cq = counts[q];
                rank += cq != 0u && (cq < c || (cq == c && q < s)) ? 1u : 0u;
            }
            if (BVC_DC_OK(0x911, rank, kDcMaxSyms)) t.order[rank] = (uint16_t)s;
        }
    }
    dc_wave_sync();
    if (lane == 0u) {
        if (used < 2u) {
            // padding: the used symbol, if there is one, and the smallest unused symbols up to two in all take one bit each
            uint32_t have = used;
            if (used == 1u) len[t.order[0] < n ? t.order[0] : 0u] = 1u;
            for (uint32_t s = 0; s < 2u && s < n; ++s)
                if (counts[s] == 0u && have < 2u) { len[s] = 1u; ++have; }
        } else {
            // the tree: the two smallest weights make a node; a leaf goes before a node of the same weight, nodes in the order they were made
            uint32_t li = 0u, ni = 0u;
            for (uint32_t m = 0; m + 1u < used; ++m) {
                uint32_t total = 0u;
                for (uint32_t k = 0; k < 2u; ++k) {
                    const uint32_t lw = li < used ? counts[t.order[li] < n ? t.order[li] : 0u] : 0u;
                    if (li < used && (ni >= m || lw <= t.weight[ni])) { total += lw; t.leaf_parent[li] = (uint16_t)m; ++li; }
                    else if (BVC_DC_OK(0x912, ni, kDcMaxSyms)) { total += t.weight[ni]; t.node_parent[ni] = (uint16_t)m; ++ni; }
                }
                t.weight[m] = total;
            }
            // depths from the root down (a node's parent was made behind it), leaves a level counted, those below the limit at the limit
            t.node_parent[used - 2u] = 0u;
            for (uint32_t i = used - 2u; i-- > 0u;) {
                const uint32_t p = t.node_parent[i];
                t.node_parent[i] = (uint16_t)((BVC_DC_OK(0x913, p, kDcMaxSyms) ? t.node_parent[p] : 0u) + 1u);
            }
            for (uint32_t b = 0; b < 16u; ++b) t.bl[b] = 0u;
            for (uint32_t k = 0; k < used; ++k) {
                const uint32_t p = t.leaf_parent[k];
                uint32_t d = (BVC_DC_OK(0x914, p, kDcMaxSyms) ? t.node_parent[p] : 0u) + 1u;
                d = d < limit ? d : limit;
                t.bl[d] += 1u;
            }
            // the Kraft sum is above 1 by `excess` units of 2^-limit.  zlib's move takes one unit away: the deepest leaf above the limit's
            // level goes one level down, and a leaf of the limit's level becomes its sibling
            uint32_t kraft = 0u;
            for (uint32_t b = 1; b <= limit; ++b) kraft += t.bl[b] << (limit - b);
            for (uint32_t excess = kraft > (1u << limit) ? kraft - (1u << limit) : 0u; excess > 0u; --excess) {
                uint32_t bits = limit - 1u;
                while (bits > 0u && t.bl[bits] == 0u) --bits;
                if (bits == 0u) break;                                        // (never: 2^limit >= n)
                t.bl[bits] -= 1u; t.bl[bits + 1u] += 2u; t.bl[limit] -= 1u;
            }
            // the longest lengths to the smallest (count, symbol)
            uint32_t at = 0u;
            for (uint32_t l = limit; l > 0u; --l)
                for (uint32_t k = t.bl[l]; k > 0u && at < used; --k, ++at) {
                    const uint32_t s = t.order[at];
                    if (BVC_DC_OK(0x915, s, n)) len[s] = (uint8_t)l;
                }
        }
    }
    dc_wave_sync();
}

// (e): canonical codes of len[0 .. n) (RFC 1951, 3.2.2), first bit lowest | length << 16; 0 for an unused symbol.  Lane 0's work.
BVC_DC void dc_make_codes(const uint8_t *len, uint32_t n, uint32_t *codes, CodeTables &t, uint32_t lane)
{
    if (lane == 0u) {
        for (uint32_t b = 0; b < 16u; ++b) t.bl[b] = 0u;
        for (uint32_t s = 0; s < n; ++s) t.bl[len[s] & 15u] += 1u;
        uint32_t code = 0u;
        t.bl[0] = 0u;
        for (uint32_t b = 1; b < 16u; ++b) { code = (code + t.bl[b - 1u]) << 1; t.next[b] = code; }
        for (uint32_t s = 0; s < n; ++s) {
            const uint32_t l = len[s] & 15u;
            uint32_t c = 0u;
            if (l != 0u) { c = dc_rev(t.next[l], l) | (l << 16); t.next[l] += 1u; }
            codes[s] = c;
        }
    }
    dc_wave_sync();
}

// All of a block's code from t.counts: lengths, codes, HLIT / HDIST / HCLEN, the sequence (b) and the block's size in both codes.
BVC_DC void dc_build_block(CodeTables &t, uint32_t lane, uint32_t nlanes)
{
    dc_build_lengths(t.counts, kDcLit, kDcLitLimit, t.len, t, lane, nlanes);
    dc_build_lengths(t.counts + kDcLit, kDcDist, kDcLitLimit, t.len + kDcLit, t, lane, nlanes);
    if (lane == 0u) {
        // (c): trimmed to the last used symbol
        uint32_t hlit = kDcLit, hdist = kDcDist;
        while (hlit > 257u && t.len[hlit - 1u] == 0u) --hlit;
        while (hdist > 1u && t.len[kDcLit + hdist - 1u] == 0u) --hdist;
        t.hlit = hlit; t.hdist = hdist;
        // (b): HLIT + HDIST lengths as ONE row (a run crosses from the first alphabet into the second), greedily from the front: a run of 11
        // or more zeros -> 18 (138 at the most), of 3..10 -> 17; 3 or more of the length just written -> 16 (6 at the most); else the length
        for (uint32_t s = 0; s < 20u; ++s) t.cl_counts[s] = 0u;
        const uint32_t rows = hlit + hdist;
        auto row = [&](uint32_t i) -> uint32_t { return t.len[i < hlit ? i : kDcLit + (i - hlit)]; };
        uint32_t i = 0u, k = 0u, prev = 0xFFu;
        while (i < rows && k < kDcRow) {
            const uint32_t v = row(i);
            uint32_t r = 1u;
            while (i + r < rows && row(i + r) == v) ++r;
            uint32_t sym = v & 15u, extra = 0u, step = 1u;
            if (v == 0u && r >= 11u) { step = r < 138u ? r : 138u; sym = 18u; extra = step - 11u; }
            else if (v == 0u && r >= 3u) { step = r; sym = 17u; extra = step - 3u; }
            else if (v != 0u && prev == v && r >= 3u) { step = r < 6u ? r : 6u; sym = 16u; extra = step - 3u; }
            t.seq_sym[k] = (uint8_t)sym; t.seq_extra[k] = (uint8_t)extra;
            t.cl_counts[sym] += 1u;
            ++k; i += step; prev = v;
        }
        t.n_seq = k;
    }
    dc_wave_sync();
    dc_build_lengths(t.cl_counts, kDcCl, kDcClLimit, t.cl_len, t, lane, nlanes);
    dc_make_codes(t.len, kDcLit, t.codes, t, lane);
    dc_make_codes(t.len + kDcLit, kDcDist, t.codes + kDcLit, t, lane);
    dc_make_codes(t.cl_len, kDcCl, t.cl_codes, t, lane);
    if (lane == 0u) {
        uint32_t hclen = kDcCl;
        while (hclen > 4u && t.cl_len[dc_cl_order(hclen - 1u)] == 0u) --hclen;
        t.hclen = hclen;
        uint32_t hb = 5u + 5u + 4u + 3u * hclen;
        for (uint32_t s = 0; s < kDcCl; ++s) hb += t.cl_counts[s] * ((uint32_t)t.cl_len[s] + dc_cl_extra_bits(s));
        t.header_bits = hb;
        uint32_t dyn = 3u + hb, fix = 3u;
        for (uint32_t s = 0; s < kDcLit; ++s) {
            const uint32_t c = t.counts[s], x = s > 256u ? dc_length_extra_bits(s) : 0u;
            dyn += c * ((uint32_t)t.len[s] + x);
            fix += c * (dc_fixed_length(s) + x);
        }
        for (uint32_t s = 0; s < kDcDist; ++s) {
            const uint32_t c = t.counts[kDcLit + s], x = dc_distance_extra_bits(s);
            dyn += c * ((uint32_t)t.len[kDcLit + s] + x);
            fix += c * (5u + x);
        }
        t.dyn_bits = dyn; t.fixed_bits = fix;
    }
    dc_wave_sync();
}

// Bits into an image of words, first bit lowest; whole words with one OR each (a word may be shared with another writer: OR does not
// depend on order).  put() takes up to 32 bits a call.
struct BitSink {
    uint32_t *out;
    uint32_t out_words, word, fill;
    uint64_t acc;
    BVC_DC void start(uint32_t *image, uint32_t words, uint32_t at) { out = image; out_words = words; word = at >> 5; fill = at & 31u; acc = 0u; }
    BVC_DC void or_word(uint32_t v)
    {
        if (v == 0u || !BVC_DC_OK(0x916, word, out_words)) return;
#ifdef __HIP_DEVICE_COMPILE__
        atomicOr(&out[word], v);
#else
        out[word] |= v;
#endif
    }
    BVC_DC void put(uint32_t bits, uint32_t n)
    {
        acc |= (uint64_t)bits << fill;
        fill += n;
        if (fill >= 32u) { or_word((uint32_t)acc); acc >>= 32; fill -= 32u; ++word; }
    }
    BVC_DC void code(uint32_t c) { put(c & 0xFFFFu, c >> 16); }                // a table entry: code | length << 16
    BVC_DC void finish() { or_word((uint32_t)acc); acc = 0u; }
};

// BFINAL, BTYPE = 10 and the header of t's code from bit 0 on: 3 + t.header_bits bits.  One lane's work; the sink goes on behind them.
BVC_DC void dc_put_header(BitSink &w, const CodeTables &t)
{
    w.put(1u | (2u << 1), 3u);
    w.put(t.hlit - 257u, 5u);
    w.put(t.hdist - 1u, 5u);
    w.put(t.hclen - 4u, 4u);
    for (uint32_t i = 0; i < t.hclen; ++i) w.put(t.cl_len[dc_cl_order(i)], 3u);
    for (uint32_t k = 0; k < t.n_seq && k < kDcRow; ++k) {
        const uint32_t sym = t.seq_sym[k] < kDcCl ? t.seq_sym[k] : 0u;
        w.code(t.cl_codes[sym]);
        w.put(t.seq_extra[k], dc_cl_extra_bits(sym));
    }
}

}  // namespace

}  // namespace bvc
