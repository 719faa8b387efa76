// bgzf_dynamic_device.h -- what the block kernel runs with a Huffman code of the block's own (bgzf_block_kernel.h, DYNAMIC, behind either
// parse): everything behind pass B -- counts, lengths, the choice among stored, fixed and
// dynamic, the bits, the slot.  The steps are described at the top of bgzf_dynamic_kernel.hip.  Inlined into its kernel; all of a
// workgroup's 1024 threads call it.
#pragma once
#include "bgzf_deflate_device.h"
#include "bgzf_codes_device.h"

namespace bvc {

namespace {

static_assert((kBdInWords + kBdTabWords + 2 * kBdBitWords + 32) * 4 + sizeof(CodeTables) <= 160 * 1024, "one workgroup's LDS");

// s_out = s_in (the image takes the input's place), s_sym = the bytes of s_tab, s_ism = s_first.  Returns the block's size.
__device__ __forceinline__ uint32_t bd_dynamic_block(uint8_t *slot, uint32_t *s_in, const uint32_t *s_tab, const uint32_t *s_ism, const uint32_t *s_path,
                                                     uint32_t *s_scan, CodeTables &s_codes, const uint32_t *match, uint32_t n, uint32_t tid)
{
    const uint32_t lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t *const s_out = s_in;
    const uint8_t *const s_sym = reinterpret_cast<const uint8_t *>(s_tab);

    // ---- counts
    const uint64_t mask = bd_my_symbols(s_path, n, tid);
    const uint32_t base = 64u * tid;
    const uint64_t ism = base < n ? (uint64_t)s_ism[2u * tid] | ((uint64_t)s_ism[2u * tid + 1u] << 32) : 0u;
    for (uint32_t w = tid; w < kDcRow; w += kBdThreads) s_codes.counts[w] = 0u;
    __syncthreads();
    for (uint64_t left = mask; left != 0u; left &= left - 1u) {
        const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
        if ((ism >> (p - base)) & 1u) {
            uint32_t le, lx, de, dx;
            const uint32_t sym = length_symbol((uint32_t)s_sym[p] + 3u, le, lx), ds = distance_symbol((match[p] & 0x7FFFu) + 1u, de, dx);
            if (BVC_LDS_OK(0x921, sym, kDcLit)) atomicAdd(&s_codes.counts[sym], 1u);
            if (BVC_LDS_OK(0x922, ds, kDcDist)) atomicAdd(&s_codes.counts[kDcLit + ds], 1u);
        } else {
            atomicAdd(&s_codes.counts[s_sym[p]], 1u);                    // (a byte: below 256)
        }
    }
    if (tid == 0u) atomicAdd(&s_codes.counts[256], 1u);                  // end of block
    __syncthreads();

    // ---- lengths, codes, sizes: one wavefront
    if (wave == 0u) dc_build_block(s_codes, lane, kWave);
    __syncthreads();

    // ---- choice (workgroup-uniform)
    const uint32_t coded = (s_codes.fixed_bits + 7u) >> 3, dyn = (s_codes.dyn_bits + 7u) >> 3;
    const bool fixed_stored = coded > n + 5u;                             // the fixed kernel's rule: F
    const uint32_t f_size = fixed_stored ? n + 5u : coded;
    const bool dynamic = dyn < f_size;
    const bool stored = !dynamic && fixed_stored;
    const uint32_t csize = dynamic ? dyn : f_size;
    const uint32_t out_words = (csize + 3u) >> 2;                         // <= (65280 + 5 + 3) / 4 < kBdInWords

    // ---- bits
    uint32_t my_bits = 0u;
    if (dynamic) {
        for (uint64_t left = mask; left != 0u; left &= left - 1u) {
            const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
            if ((ism >> (p - base)) & 1u) {
                uint32_t le, lx, de, dx;
                const uint32_t sym = length_symbol((uint32_t)s_sym[p] + 3u, le, lx), ds = distance_symbol((match[p] & 0x7FFFu) + 1u, de, dx);
                if (BVC_LDS_OK(0x923, sym, kDcLit) && BVC_LDS_OK(0x924, ds, kDcDist))
                    my_bits += (s_codes.codes[sym] >> 16) + le + (s_codes.codes[kDcLit + ds] >> 16) + de;
            } else {
                my_bits += s_codes.codes[s_sym[p]] >> 16;
            }
        }
    } else if (!stored) {
        my_bits = bd_fixed_bits(s_sym, s_ism, match, mask, n, tid);
    }
    uint32_t all;
    const uint32_t before = bd_scan(my_bits, s_scan, lane, wave, all);
    if (!stored) {
        // (the input's last readers were pass B's: its place takes the image)
        for (uint32_t w = tid; w < out_words; w += kBdThreads) s_out[w] = 0u;
        __syncthreads();
        if (dynamic) {
            const uint32_t first = 3u + s_codes.header_bits;              // where thread 0's symbols begin
            BitSink w;
            if (tid == 0u) { w.start(s_out, out_words, 0u); dc_put_header(w, s_codes); }
            else w.start(s_out, out_words, first + before);
            for (uint64_t left = mask; left != 0u; left &= left - 1u) {
                const uint32_t p = base + (uint32_t)__builtin_ctzll(left);
                if ((ism >> (p - base)) & 1u) {
                    uint32_t le, lx, de, dx;
                    const uint32_t sym = length_symbol((uint32_t)s_sym[p] + 3u, le, lx), ds = distance_symbol((match[p] & 0x7FFFu) + 1u, de, dx);
                    if (BVC_LDS_OK(0x925, sym, kDcLit) && BVC_LDS_OK(0x926, ds, kDcDist)) {
                        const uint32_t lc = s_codes.codes[sym], dcode = s_codes.codes[kDcLit + ds];
                        w.put((lc & 0xFFFFu) | (lx << (lc >> 16)), (lc >> 16) + le);          // up to 15 + 5 bits
                        w.put((dcode & 0xFFFFu) | (dx << (dcode >> 16)), (dcode >> 16) + de);  // up to 15 + 13 bits
                    }
                } else {
                    w.code(s_codes.codes[s_sym[p]]);
                }
            }
            w.finish();
            if (tid == 0u) {                                              // the end-of-block code behind the last thread's symbols
                BitSink e;
                e.start(s_out, out_words, first + all);
                e.code(s_codes.codes[256]);
                e.finish();
            }
        } else {
            bd_fixed_write(s_out, out_words, s_sym, s_ism, match, mask, 3u + before, n, tid);
        }
        __syncthreads();
    }
    return bd_write_slot(slot, s_in, s_out, n, csize, stored, tid);
}

}  // namespace

}  // namespace bvc
