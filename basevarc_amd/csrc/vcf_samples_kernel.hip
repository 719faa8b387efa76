// vcf_samples_kernel.hip -- the sample columns of a CALLED position's VCF line (WriteVcf, src/BaseType.cpp:187-212; the host program's
// vcf_line, host/pileup.cpp), formatted where the position's entries lie.  One field per sample, tab separated:
//     "./."                  a sample without an entry                                      4 bytes with its tab
//     "g:B:S:d.dddddd"       a sample with one: genotype, base letter, strand, 1 - 10^(-qual/10)   17 bytes with its tab
// Only the entries of the VALID PREFIX count: the host's loop stops at the first entry whose sample index does not ascend or lies
// outside 0 .. n_samples - 1.  Inside that prefix the sample indices ascend strictly, so entry k has exactly k covered samples in front
// of it and the field of sample i starts at byte 4 * i + 13 * (covered samples below i) of the site's slot.
//
// No floating point: the eight characters of d.dddddd depend on the quality byte alone and come from a 256-row table the host side of
// the library formats with the host program's own expression (bvc_vcf_bp_lut, bvc_vcf.hip).
//
// Three launches.  vcf_valid_kernel: a workgroup per site finds the length of the valid prefix (one min-reduction) and writes text_len.
// vcf_plan_kernel: one workgroup scans the slot sizes into text_off and lists the called sites.  vcf_samples_kernel: the workgroups stride
// over (called site, tile of kVcfSamplesTile consecutive samples); a site that is not called appears in no launch but the first two,
// where it costs one loop iteration, and none of its entries is read.  Per tile:
//   - every wavefront finds the first entry of the tile in the valid prefix with a 64-ary search (three rounds of loads for 2^18 entries);
//   - lane j takes entry first + j (the tile holds at most one entry per sample) and drops (genotype, base, strand, quality) as one word
//     into the LDS cell of its sample -- the index is DATA and is bounded before it is used;
//   - lane j then is sample tile_start + j: covered or not from its cell, its rank from a ballot and the wavefronts' counts, and it
//     writes its 4 or 17 bytes into an LDS image of the tile's output bytes;
//   - the workgroup stores the image with 16-byte stores to 16-byte aligned addresses.  A 16-byte piece belongs to the tile that holds
//     its FIRST byte: the piece across a tile's end takes up to 15 bytes of the next tile's fields, which is why a workgroup also formats
//     the kVsHalo = 4 samples behind its tile (four fields are at least 16 bytes), and the bytes in front of a tile's first whole piece
//     are the previous tile's.  The last piece of a slot runs into the slot's padding.  There are no narrower stores.
#include "bvc_device.h"
#include "bvc_internal.h"

namespace bvc {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kVsThreads = 512;                         // 8 wavefronts; lane j of the workgroup = entry j of the tile, then sample j
constexpr int kVsWaves = kVsThreads / kWave;
constexpr int kVsHalo = 4;                              // samples behind the tile whose first bytes fill the tile's last 16-byte piece
constexpr int kVsImage = kVsThreads * 17;               // bytes of the staging image: every sample of tile + halo covered (+ the 15 of rounding)
// dynamic LDS, in words: the image, a cell per sample, the quality table, the wavefronts' covered counts (all samples | the tile's own)
constexpr int kVsCell = kVsImage / 4, kVsLut = kVsCell + kVsThreads, kVsSum = kVsLut + 512, kVsWords = kVsSum + 2 * kVsWaves;
static_assert(kVcfSamplesTile == kVsThreads - kVsHalo, "the tile the tests straddle");
static_assert(kVsImage % 16 == 0 && kVsCell % 4 == 0 && kVsLut % 4 == 0 && kVsSum % 4 == 0, "16-byte aligned slices (ds_read_b128)");
static_assert(kVcfSamplesTile * 17 + 15 <= kVsImage, "a tile's bytes and the rounding of its end fit the image");

constexpr int kVpThreads = 256;                         // vcf_valid_kernel
constexpr int kVqThreads = 1024;                        // vcf_plan_kernel

__device__ __forceinline__ int64_t slot_bytes(int64_t n_samples, int64_t n_entries) { return (4 * n_samples + 13 * n_entries + 15) & ~(int64_t)15; }

}  // namespace

// n_valid[s] = the first k with samples[k] outside 0 .. n_samples - 1 or samples[k] <= samples[k - 1] (the entries in front of the first
// such k ascend strictly, so the test between neighbours is the host's test against `next`), text_len[s] = the bytes of the site's text.
__global__ __launch_bounds__(kVpThreads) void vcf_valid_kernel(
    int64_t n_sites, const int64_t *__restrict__ offsets, const int32_t *__restrict__ samples, const bvc_site_result *__restrict__ results,
    int64_t n_samples, uint32_t *__restrict__ n_valid, int64_t *__restrict__ text_len)
{
    BVC_POISON_LDS();
    __shared__ uint32_t s_min[kVpThreads / kWave];
    const int tid = threadIdx.x;
    for (int64_t site = blockIdx.x; site < n_sites; site += gridDim.x) {
        if (results[site].called == 0) {                                      // (workgroup-uniform)
            if (tid == 0) { n_valid[site] = 0u; text_len[site] = 0; }
            continue;
        }
        const int64_t o0 = offsets[site];
        const uint32_t n = (uint32_t)(offsets[site + 1] - o0);               // (a site holds fewer than 2^31 entries)
        const int32_t *__restrict__ p = samples + o0;
        uint32_t first = n;
        for (uint32_t k = (uint32_t)tid; k < n; k += kVpThreads) {
            const int32_t v = p[k];
            if (v < 0 || (int64_t)v >= n_samples || (k > 0u && v <= p[k - 1])) { first = k; break; }
        }
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)first, d);
            first = o < first ? o : first;
        }
        if ((tid & (kWave - 1)) == 0) s_min[tid >> 6] = first;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kVpThreads / kWave; ++w) first = s_min[w] < first ? s_min[w] : first;
            const int64_t len = 4 * n_samples + 13 * (int64_t)first - 1;
            n_valid[site] = first;
            text_len[site] = len > 0 ? len : 0;
        }
        __syncthreads();                                                      // s_min belongs to the next site from here
    }
}

// text_off[0 .. n_sites] = exclusive prefix sums of the called sites' slot sizes, called_list = the called sites in order,
// head[0] = how many, head[1] = the sum of the slots.  One workgroup; 1024 sites a round.
__global__ __launch_bounds__(kVqThreads) void vcf_plan_kernel(
    int64_t n_sites, const int64_t *__restrict__ offsets, const bvc_site_result *__restrict__ results, int64_t n_samples,
    int64_t *__restrict__ text_off, int32_t *__restrict__ called_list, int64_t *__restrict__ head)
{
    BVC_POISON_LDS();
    __shared__ int64_t s_sz[kVqThreads];
    __shared__ int32_t s_c[kVqThreads];
    const int tid = threadIdx.x;
    int64_t base = 0, n_called = 0;                                           // (the same in every thread)
    for (int64_t s0 = 0; s0 < n_sites; s0 += kVqThreads) {
        const int64_t s = s0 + tid;
        const bool called = s < n_sites && results[s].called != 0;
        const int64_t sz = called ? slot_bytes(n_samples, offsets[s + 1] - offsets[s]) : 0;
        s_sz[tid] = sz; s_c[tid] = called ? 1 : 0;
        __syncthreads();
        for (int d = 1; d < kVqThreads; d <<= 1) {
            const int64_t v = tid >= d ? s_sz[tid - d] : 0;
            const int32_t c = tid >= d ? s_c[tid - d] : 0;
            __syncthreads();
            s_sz[tid] += v; s_c[tid] += c;
            __syncthreads();
        }
        if (s < n_sites) text_off[s] = base + s_sz[tid] - sz;
        if (called) called_list[n_called + s_c[tid] - 1] = (int32_t)s;
        const int64_t tot = s_sz[kVqThreads - 1];
        const int32_t ctot = s_c[kVqThreads - 1];
        __syncthreads();                                                      // the arrays belong to the next round from here
        base += tot; n_called += ctot;
    }
    if (tid == 0) { text_off[n_sites] = base; head[0] = n_called; head[1] = base; }
}

// The text.  bp_lut: 256 rows of the eight characters d.dddddd.  Nothing is written when the slots do not fit text_cap (the host side
// compares head[1] with it too and reports).
__global__ __launch_bounds__(kVsThreads) void vcf_samples_kernel(
    const int64_t *__restrict__ offsets, const bvc_pileup_entry *__restrict__ entries, const int32_t *__restrict__ samples,
    const int8_t *__restrict__ ref_base, const bvc_site_result *__restrict__ results, int64_t n_samples,
    const int64_t *__restrict__ text_off, const uint32_t *__restrict__ n_valid, const int32_t *__restrict__ called_list,
    const int64_t *__restrict__ head, const uint32_t *__restrict__ bp_lut, char *__restrict__ text, int64_t text_cap)
{
    BVC_POISON_LDS();
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];          // kVsWords
    uint8_t *const image = reinterpret_cast<uint8_t *>(lds);
    uint32_t *const cell = lds + kVsCell, *const lut = lds + kVsLut, *const wsum = lds + kVsSum;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    lut[tid] = bp_lut[tid];                                                  // 512 words = 256 rows
    __syncthreads();
    if (head[1] > text_cap) return;
    const int64_t tiles = (n_samples + kVcfSamplesTile - 1) / kVcfSamplesTile;
    const uint32_t n_called = (uint32_t)head[0];                             // (a call holds fewer than 2^25 sites)
    // the grid is (tiles, called sites), each dimension strided (no division: the kernel has no floating point, the compiler's neither)
    for (uint32_t ci = blockIdx.y; ci < n_called; ci += gridDim.y)
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {                // (both workgroup-uniform)
        const int64_t site = called_list[ci];
        const int64_t i0 = t * kVcfSamplesTile;
        const int64_t i1 = i0 + kVcfSamplesTile < n_samples ? i0 + kVcfSamplesTile : n_samples;
        const int64_t o0 = offsets[site];
        const uint32_t nv = n_valid[site];
        const int32_t *__restrict__ p = samples + o0;
        // lo = the entries of the valid prefix with a sample below i0: 64 probes a round, every wavefront for itself.  Everything
        // below a has a sample below i0, everything from b on has not.
        uint32_t a = 0u, b = i0 > 0 ? nv : 0u;
        while (a < b) {                                                       // (wavefront-uniform)
            const uint32_t step = (b - a + 63u) >> 6;
            const uint32_t at = a + (uint32_t)lane * step;                   // (below 2^31 + 2^25)
            const bool less = at < b && (int64_t)p[at < b ? at : a] < i0;
            const uint32_t c = (uint32_t)__popcll(__ballot(less));           // probes 0 .. c - 1 are below (the samples ascend)
            const uint32_t b2 = a + c * step;
            if (c > 0u) a = a + (c - 1u) * step + 1u;
            b = b2 < b ? b2 : b;
        }
        const uint32_t lo = a;
        cell[tid] = 0u;
        __syncthreads();
        // entry lo + tid, where it belongs to a sample of tile + halo: its field's variable part as one word
        //   bit 31 covered | bits 12-14 genotype (0 "0/.", 1-3 "./1"-"./3", 4 "./.") | bits 8-11 base & 7, strand & 1 << 3 | bits 0-7 quality
        {
            const uint32_t k = lo + (uint32_t)tid;
            if (k < nv) {
                const int64_t rel = (int64_t)p[k] - i0;                       // >= 0: entry lo is the first with a sample from i0 on
                if ((uint64_t)rel < (uint64_t)kVsThreads) {                 // (the bound of the cell index: a sample of tile + halo)
                    const u32x2 e = *reinterpret_cast<const u32x2 *>(entries + o0 + k);
                    const uint32_t base = e.x & 7u, qual = (e.x >> 16) & 0xFFu, strand = e.y & 1u;
                    const int n_alt = results[site].n_alt < 3 ? results[site].n_alt : 3;
                    uint32_t gt = 4u;
                    for (int i = 0; i < n_alt; ++i)
                        if (((uint32_t)(int)results[site].alt_base[i] & 7u) == base) gt = (uint32_t)i + 1u;       // (the last one wins)
                    if ((int)base == (int)ref_base[site]) gt = 0u;
                    if (BVC_LDS_OK(0x801, rel, kVsThreads))
                        cell[(uint32_t)rel] = 0x80000000u | (gt << 12) | (strand << 11) | (base << 8) | qual;
                }
            }
        }
        __syncthreads();
        // sample i0 + tid
        const int64_t i = i0 + tid;
        const uint32_t c = cell[tid];
        const bool covered = i < n_samples && (c >> 31) != 0u;
        const uint64_t m_all = __ballot(covered), m_own = __ballot(covered && i < i1);
        if (lane == 0) { wsum[wave] = (uint32_t)__popcll(m_all); wsum[kVsWaves + wave] = (uint32_t)__popcll(m_own); }
        __syncthreads();
        uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m_all >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_all, 0u));
        uint32_t own = 0u;
        for (int v = 0; v < kVsWaves; ++v) {
            before += v < wave ? wsum[v] : 0u;
            own += wsum[kVsWaves + v];
        }
        // bytes of the slot: the tile's fields are [b0, b1); the image is [g0, g1), the 16-byte pieces that begin inside [b0, b1)
        const int64_t b0 = 4 * i0 + 13 * (int64_t)lo, b1 = 4 * i1 + 13 * (int64_t)(lo + own);
        const int64_t g0 = (b0 + 15) & ~(int64_t)15, g1 = (b1 + 15) & ~(int64_t)15;
        const uint32_t img = g1 - g0 < kVsImage ? (uint32_t)(g1 - g0) : (uint32_t)kVsImage;       // (at most 17 bytes a sample + 15: always the first)
        auto put = [&](int32_t x, uint32_t byte) {
            if ((uint32_t)x < img && BVC_LDS_OK(0x802, x, kVsImage)) image[x] = (uint8_t)byte;
        };
        // the slot's padding behind the site's last field, where it falls into this image: nobody else writes it
        const int64_t pad = 4 * n_samples + 13 * (int64_t)nv - g0;
        if (tid < 16 && pad < (int64_t)img) put((int32_t)pad + tid, 0u);
        if (i < n_samples) {
            const int32_t x = (int32_t)(4 * i + 13 * (int64_t)(lo + before) - g0);
            const uint32_t gt = (c >> 12) & 7u, base = (c >> 8) & 7u;
            // "g/g:" then "B:S:" then d.dddddd then the tab; a sample without an entry is "./." and the tab
            const uint32_t w0 = covered ? (gt == 0u ? (uint32_t)'0' : (uint32_t)'.') | ((uint32_t)'/' << 8) |
                                              ((gt == 0u || gt == 4u ? (uint32_t)'.' : (uint32_t)'0' + gt) << 16) | ((uint32_t)':' << 24)
                                        : (uint32_t)'.' | ((uint32_t)'/' << 8) | ((uint32_t)'.' << 16) | ((uint32_t)'\t' << 24);
#pragma unroll
            for (int j = 0; j < 4; ++j) put(x + j, (w0 >> (8 * j)) & 0xFFu);
            if (covered) {
                const uint32_t letter = (uint32_t)(0x4E4E54474341ULL >> (8 * (base < 5u ? base : 5u))) & 0xFFu;        // "ACGTNN"
                const uint32_t q = c & 0xFFu;
                const uint32_t wv[3] = {letter | ((uint32_t)':' << 8) | ((c >> 11) & 1u ? (uint32_t)'+' << 16 : (uint32_t)'-' << 16) | ((uint32_t)':' << 24),
                                        lut[2u * q], lut[2u * q + 1u]};
#pragma unroll
                for (int j = 0; j < 12; ++j) put(x + 4 + j, (wv[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                put(x + 16, (uint32_t)'\t');
            }
        }
        __syncthreads();
        char *const dst = text + text_off[site] + g0;                        // 16-byte aligned: text, text_off[site] and g0 are
        for (uint32_t piece = (uint32_t)tid; piece < (img >> 4); piece += kVsThreads)
            *reinterpret_cast<u32x4 *>(dst + 16u * piece) = *reinterpret_cast<const u32x4 *>(image + 16u * piece);
        __syncthreads();                                                      // image, cells and counts belong to the next item from here
    }
}

size_t vcf_samples_scratch_bytes(int64_t n_sites) { return 256 + 2 * round256((size_t)n_sites * 4); }

VcfSamplesScratch vcf_samples_scratch(void *buf, int64_t n_sites)
{
    Layout L{reinterpret_cast<uintptr_t>(buf)};
    VcfSamplesScratch s;
    s.head = L.take<int64_t>(2);
    s.called_list = L.take<int32_t>((size_t)n_sites);
    s.n_valid = L.take<uint32_t>((size_t)n_sites);
    return s;
}

hipError_t launch_vcf_samples_plan(hipStream_t stream, int64_t n_sites, const int64_t *offsets, const int32_t *samples,
                                   const bvc_site_result *results, int64_t n_samples, int64_t *text_off, int64_t *text_len,
                                   const VcfSamplesScratch &s)
{
    if (n_sites > 0)
        hipLaunchKernelGGL(vcf_valid_kernel, dim3((unsigned)(n_sites < 2048 ? n_sites : 2048)), dim3(kVpThreads), 0, stream, n_sites, offsets,
                           samples, results, n_samples, s.n_valid, text_len);
    // (with no site at all it still writes text_off[0] and the two sums)
    hipLaunchKernelGGL(vcf_plan_kernel, dim3(1), dim3(kVqThreads), 0, stream, n_sites, offsets, results, n_samples, text_off, s.called_list, s.head);
    return hipGetLastError();
}

hipError_t launch_vcf_samples(hipStream_t stream, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                              const int32_t *samples, const int8_t *ref_base, const bvc_site_result *results, int64_t n_samples,
                              const int64_t *text_off, const VcfSamplesScratch &s, const char *bp_lut, char *text, int64_t text_cap)
{
    if (n_sites <= 0 || n_samples <= 0) return hipSuccess;
    const int64_t tiles = (n_samples + kVcfSamplesTile - 1) / kVcfSamplesTile;
    // (about 2048 workgroups: more than the chip holds at a time; the tiles and sites beyond them follow in each workgroup's loops.  How
    // many sites are called the kernel reads for itself: n_sites bounds it)
    const unsigned gx = (unsigned)(tiles < 2048 ? tiles : 2048), rows = 2048u / gx;
    const unsigned gy = (unsigned)(n_sites < (int64_t)rows ? n_sites : (int64_t)rows);
    hipLaunchKernelGGL(vcf_samples_kernel, dim3(gx, gy), dim3(kVsThreads), kVsWords * sizeof(uint32_t), stream,
                       offsets, entries, samples, ref_base, results, n_samples, text_off, s.n_valid, s.called_list, s.head,
                       reinterpret_cast<const uint32_t *>(bp_lut), text, text_cap);
    return hipGetLastError();
}

static_assert(sizeof(bvc_pileup_entry) == 8, "record layout of include/bvc.h");

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_vcf_samples)
#endif

}  // namespace bvc
