// crc32_device.h -- CRC32 (RFC 1952) of a byte range by one wavefront, shared by the kernels that check a BGZF block's trailer
// (inflate_kernel.hip) and those that write one (bgzf_deflate_kernel.hip).
// Every lane takes a slice of the range (slices cut at absolute 16-byte boundaries: aligned 16-byte loads), runs the byte-wise table
// CRC over it, and the 64 slice CRCs are combined in order -- crc(A || B) = crc(A) * x^(8 |B|) mod P xor crc(B) in GF(2)[x] (zlib's
// crc32_combine; the powers x^(2^k) mod P are compile-time constants).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvc_device.h"

namespace bvc {
namespace {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t crc_multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1u)) == 0u) break; }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
struct CrcPowers { uint32_t v[32]; };
constexpr CrcPowers crc_powers()
{
    CrcPowers t{};
    uint32_t p = 1u << 30;                                       // x^1
    t.v[0] = p;
    for (int i = 1; i < 32; ++i) { p = crc_multmodp(p, p); t.v[i] = p; }
    return t;
}
__device__ const CrcPowers kCrcPowers = crc_powers();

// x^(8 n) mod P
__device__ uint32_t crc_shift_op(uint32_t n)
{
    uint32_t p = 1u << 31;
    int k = 3;
    while (n) { if (n & 1u) p = crc_multmodp(kCrcPowers.v[k & 31], p); n >>= 1; ++k; }
    return p;
}

// The 256-entry table of the byte-wise CRC into tab (LDS), by the wavefront's 64 lanes; visible to all of them on return.
__device__ __forceinline__ void crc_table_fill(uint32_t *tab, int lane)
{
    for (int i = lane; i < 256; i += kWave) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? kCrcPoly ^ (c >> 1) : c >> 1;
        tab[i] = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// CRC32 of out[o0 .. o0 + n), the same value in every lane.  `out` is 16-byte aligned; the range may start and end at any byte, and no
// byte outside it is read.
__device__ __forceinline__ uint32_t crc32_wave(const uint8_t *__restrict__ out, uint64_t o0, uint32_t n, const uint32_t *tab, int lane)
{
    // slice boundaries: o0 rounded down to 16, then every `per` bytes (a multiple of 16), clamped to the range
    const uint64_t base = o0 & ~(uint64_t)15;
    const uint32_t span = (uint32_t)(o0 - base) + n;
    const uint32_t per = ((span + kWave - 1) / kWave + 15u) & ~15u;
    const uint64_t lo64 = base + (uint64_t)per * (uint32_t)lane, hi64 = lo64 + per;
    const uint64_t lo = lo64 < o0 ? o0 : (lo64 > o0 + n ? o0 + n : lo64), hi = hi64 < o0 ? o0 : (hi64 > o0 + n ? o0 + n : hi64);
    uint32_t c = 0xFFFFFFFFu;
    uint64_t at = lo;
    while (at < hi && (at & 15u)) { c = tab[(c ^ out[at]) & 255u] ^ (c >> 8); ++at; }
    for (; at + 16 <= hi; at += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(out + at);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) c = tab[(c ^ (w[j] >> (8 * b))) & 255u] ^ (c >> 8);
    }
    for (; at < hi; ++at) c = tab[(c ^ out[at]) & 255u] ^ (c >> 8);
    const uint32_t mine = ~c;                                // the slice's CRC32 (0 for an empty slice)
    const uint32_t len = (uint32_t)(hi - lo);
    // in order: acc = acc * x^(8 len_k) xor crc_k; the slices behind the first are `per` bytes but the last (and the empty ones)
    const uint32_t op_full = crc_shift_op(per);
    uint32_t acc = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0);
    for (int k = 1; k < kWave; ++k) {
        const uint32_t lk = (uint32_t)__shfl((int)len, k, kWave), ck = (uint32_t)__shfl((int)mine, k, kWave);
        if (lk == 0u) continue;
        acc = crc_multmodp(lk == per ? op_full : crc_shift_op(lk), acc) ^ ck;
    }
    return acc;
}

}  // namespace
}  // namespace bvc
