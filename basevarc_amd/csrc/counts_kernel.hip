// counts_kernel.hip -- class counts that ACCUMULATE over chunks of a cohort's samples (bvc_counts_add_*, bvc_counts_merge): the fold of
// a chunk's histograms into the caller's counts, and the ragged stage 1 of site-chunks too short to be worth a histogram in LDS.
#include "bvc_device.h"
#include "bvc_internal.h"

namespace bvc {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kAddThreads = 256;

// dst[i] += src[i] (unsigned, wraps at 2^32).  Every word has ONE owner, so there is no atomic: 16-byte loads and stores over the
// whole words of four when both arrays start on a 16-byte boundary (vec), the rest -- or everything -- word by word.  12 bytes of
// traffic per word; the fold of a chunk's scratch histograms and bvc_counts_merge are this kernel.
__global__ __launch_bounds__(kAddThreads) void counts_add_kernel(int64_t n_words, int vec, uint32_t *__restrict__ dst,
                                                                 const uint32_t *__restrict__ src)
{
    BVC_POISON_LDS();
    const int64_t first = (int64_t)blockIdx.x * kAddThreads + threadIdx.x, stride = (int64_t)gridDim.x * kAddThreads;
    const int64_t n4 = vec ? n_words >> 2 : 0;
    u32x4 *__restrict__ d4 = reinterpret_cast<u32x4 *>(dst);
    const u32x4 *__restrict__ s4 = reinterpret_cast<const u32x4 *>(src);
    int64_t j = first;
    for (; j + stride < n4; j += 2 * stride) {                    // two owners' words in flight
        const u32x4 a0 = d4[j], b0 = s4[j], a1 = d4[j + stride], b1 = s4[j + stride];
        d4[j] = a0 + b0;
        d4[j + stride] = a1 + b1;
    }
    if (j < n4) d4[j] = d4[j] + s4[j];
    for (int64_t w = (n4 << 2) + first; w < n_words; w += stride) dst[w] += src[w];
}

// ---- short ragged site-chunks: no histogram, one atomic per observation --------------------------------------------------------
// A chunk of 500 samples at 6-10 % coverage brings a site a few dozen observations.  Zeroing and folding (k + 1) x 2 KB of LDS
// counters for them costs more than they do, and one wavefront (or workgroup) per site leaves most lanes idle.  Here the lanes run
// over the OBSERVATIONS of the call, across site boundaries: a wavefront takes 256 consecutive ones per trip, finds the sites of its
// first and last one in `offsets` (wave-uniform: a full binary search for its first trip, a galloping one from the previous trip's
// last site afterwards), every lane then searches only between those two, and each covered observation of a site with at most
// max_len observations in this call is ONE no-return atomic add on counts[site][group][class] (device scope: the adds of all
// workgroups meet in memory, whatever XCD they run on).  Longer sites are hist_csr_add_kernel's (pileup_kernel.hip); a trip that
// lies inside one of them loads nothing.  1-3 algorithmic bytes in and one 4-byte atomic out per observation.
//
// Loads as in hist_csr_labels_kernel: where the arrays agree on their alignment mod 4, a lane takes FOUR consecutive observations
// with one aligned 4-byte load per array (the first and last word of the call, which reach outside it, byte by byte); where they
// disagree, consecutive lanes take consecutive observations with byte loads, four per lane in flight.
constexpr int kScatterThreads = 256;
constexpr int kScatterWaves = kScatterThreads / kWave;
constexpr int64_t kScatterTrip = 4 * kWave;                       // observations of a wavefront per trip

// the largest s in [lo, hi] with offsets[s] <= i (offsets[lo] <= i is given)
__device__ __forceinline__ int64_t site_at(const int64_t *__restrict__ offsets, int64_t lo, int64_t hi, int64_t i)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the same from a site `from` at or just before it (offsets[from] <= i is given): doubling steps, then the search between the last two
__device__ __forceinline__ int64_t site_from(const int64_t *__restrict__ offsets, int64_t from, int64_t n_sites, int64_t i)
{
    int64_t step = 1;
    while (from + step < n_sites && offsets[from + step] <= i) step <<= 1;
    return site_at(offsets, from + (step >> 1), from + step - 1 < n_sites - 1 ? from + step - 1 : n_sites - 1, i);
}

template <bool PACKED, bool LABELS>
__global__ __launch_bounds__(kScatterThreads) void hist_csr_scatter_kernel(
    int64_t n_sites, const int64_t *__restrict__ offsets, const uint8_t *__restrict__ obs, const uint8_t *__restrict__ quals,
    const uint8_t *__restrict__ group_of_obs, int n_groups, int64_t max_len, uint32_t *__restrict__ counts)
{
    BVC_POISON_LDS();
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kScatterWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * kScatterWaves;
    const int64_t begin = offsets[0], end = offsets[n_sites];
    if (end <= begin) return;
    const int64_t n_hist = LABELS ? n_groups + 1 : 1;
    // j = i + mis indexes the arrays from their last 4-byte boundary: the word of j = 4w .. 4w + 3 is aligned
    const uint32_t mis = (uint32_t)(uintptr_t)obs & 3u;
    const bool words = (PACKED || ((uint32_t)(uintptr_t)quals & 3u) == mis) && (!LABELS || ((uint32_t)(uintptr_t)group_of_obs & 3u) == mis);
    const int64_t shift = words ? (int64_t)mis : 0;
    const int64_t t0 = (begin + shift) / kScatterTrip, t1 = (end + shift + kScatterTrip - 1) / kScatterTrip;   // trips of the call
    const int64_t per = (t1 - t0 + n_waves - 1) / n_waves;                                                     // a wavefront's, consecutive
    const int64_t my0 = t0 + wave * per, my1 = my0 + per < t1 ? my0 + per : t1;

    // one covered observation of site s
    auto add = [&](int64_t s, uint32_t b, uint32_t q, uint32_t lab) {
        if (PACKED) { q = b & 63u; b >>= 6; }
        if (PACKED ? q != 63u : (b < 4u && q < 128u)) {
            const int64_t g = LABELS ? (int64_t)(lab < (uint32_t)n_groups ? lab : (uint32_t)n_groups) : 0;
            (void)__hip_atomic_fetch_add(&counts[(s * n_hist + g) * BVC_NCLASS + ((b << 7) | q)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    int64_t prev = -1;                                             // the site of the previous trip's last observation
    for (int64_t t = my0; t < my1; ++t) {
        const int64_t i_first = t * kScatterTrip - shift > begin ? t * kScatterTrip - shift : begin;
        const int64_t i_last = (t + 1) * kScatterTrip - shift < end ? (t + 1) * kScatterTrip - shift - 1 : end - 1;
        // wave-uniform: the sites of the trip's first and last observation
        const int64_t lo = prev < 0 ? site_at(offsets, 0, n_sites - 1, i_first) : site_from(offsets, prev, n_sites, i_first);
        const int64_t hi = site_from(offsets, lo, n_sites, i_last);
        prev = hi;
        if (lo == hi && offsets[lo + 1] - offsets[lo] > max_len) continue;                           // inside one long site
        if (words) {
            const int64_t i0 = t * kScatterTrip - shift + 4 * lane;                                // the lane's word: observations i0 .. i0 + 3
            if (i0 < end && i0 + 4 > begin) {
                uint32_t wb, wq = 0u, wl = 0u;
                if (i0 >= begin && i0 + 4 <= end) {
                    wb = *reinterpret_cast<const uint32_t *>(obs + i0);
                    if (!PACKED) wq = *reinterpret_cast<const uint32_t *>(quals + i0);
                    if (LABELS) wl = *reinterpret_cast<const uint32_t *>(group_of_obs + i0);
                } else {                                           // the call's first or last word: only the bytes inside it
                    wb = 0u;
                    for (int k = 0; k < 4; ++k) {
                        const int64_t i = i0 + k;
                        if (i < begin || i >= end) continue;
                        wb |= (uint32_t)obs[i] << (8 * k);
                        if (!PACKED) wq |= (uint32_t)quals[i] << (8 * k);
                        if (LABELS) wl |= (uint32_t)group_of_obs[i] << (8 * k);
                    }
                }
                const int64_t i_own = i0 > begin ? i0 : begin;
                int64_t s = site_at(offsets, lo, hi, i_own);
                int64_t o0 = offsets[s], o1 = offsets[s + 1];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t i = i0 + k;
                    if (i < begin || i >= end) continue;
                    while (s < hi && o1 <= i) { ++s; o0 = o1; o1 = offsets[s + 1]; }
                    if (o1 - o0 <= max_len) add(s, (wb >> (8 * k)) & 0xFFu, (wq >> (8 * k)) & 0xFFu, (wl >> (8 * k)) & 0xFFu);
                }
            }
        } else {
            uint32_t b[4], q[4], lab[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = t * kScatterTrip + u * kWave + lane;
                const bool in = i >= begin && i < end;
                b[u] = in ? obs[i] : (PACKED ? 0xFFu : 4u);
                q[u] = in && !PACKED ? quals[i] : 0u;
                lab[u] = in && LABELS ? group_of_obs[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = t * kScatterTrip + u * kWave + lane;
                if (i < begin || i >= end) continue;
                const int64_t s = site_at(offsets, lo, hi, i);
                if (offsets[s + 1] - offsets[s] <= max_len) add(s, b[u], q[u], lab[u]);
            }
        }
    }
}

}  // namespace

hipError_t launch_counts_add(hipStream_t stream, int64_t n_words, uint32_t *dst, const uint32_t *src)
{
    if (n_words <= 0) return hipSuccess;
    const int vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
    const int64_t items = vec ? (n_words >> 2) / 2 + 4 : n_words;            // two words of four per thread and trip
    int64_t blocks = (items + kAddThreads - 1) / kAddThreads;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(counts_add_kernel, dim3((unsigned)blocks), dim3(kAddThreads), 0, stream, n_words, vec, dst, src);
    return hipGetLastError();
}

hipError_t launch_hist_csr_scatter(const LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const uint8_t *obs,
                                   const uint8_t *quals, const uint8_t *group_of_obs, int n_groups, int64_t max_len, uint32_t *counts)
{
    if (n_sites <= 0 || max_len <= 0) return hipSuccess;
    // the observations of the call are known on the device only: a grid that fills the chip, each wavefront a run of trips
    const unsigned grid = (unsigned)(st.n_cu * 8);
    const dim3 g(grid), b(kScatterThreads);
    if (group_of_obs) {
        if (quals) hipLaunchKernelGGL((hist_csr_scatter_kernel<false, true>), g, b, 0, stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, max_len, counts);
        else hipLaunchKernelGGL((hist_csr_scatter_kernel<true, true>), g, b, 0, stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, max_len, counts);
    } else {
        if (quals) hipLaunchKernelGGL((hist_csr_scatter_kernel<false, false>), g, b, 0, stream, n_sites, offsets, obs, quals, group_of_obs, 0, max_len, counts);
        else hipLaunchKernelGGL((hist_csr_scatter_kernel<true, false>), g, b, 0, stream, n_sites, offsets, obs, quals, group_of_obs, 0, max_len, counts);
    }
    return hipGetLastError();
}

}  // namespace bvc
