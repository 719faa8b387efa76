// site_stats_kernel.hip -- what WriteVcf (src/BaseType.cpp:141-234) takes from a CALLED position's entries besides the sample columns:
// the rank sums of the three 8-bit fields (mapq, qual, rpr) of the REF observations among the pooled ref + alt ones, the sizes of the
// two samples and the four strand counts (include/bvc.h, bvc_site_stats).
//
// rankR1 (src/Algorithm.cpp:27-53) ranks the pooled values in DESCENDING order and gives a run of equal values the mean of the ranks
// it spans.  The values are bytes, so the statistic is a function of two 256-bin histograms per field, r[v] (ref) and a[v] (alt):
// going down from value 255 with lo = the pooled observations of a larger value, the run of value v occupies ranks
// lo + 1 .. lo + r[v] + a[v], and
//     2 * r1 = sum_v r[v] * (2 * lo + r[v] + a[v] + 1)
// an integer: no sort, no floating point, and the host's double (stats.cpp, rank_r1) is exactly that integer divided by two.
//
// A workgroup takes one site at a time (the grid strides over all sites; a site that is not called costs it one loop iteration and a
// zeroed record).  It streams a called site's 8-byte entries with 16-byte loads (two entries a lane, kStatsLoads loads a
// lane in flight), counts them into LDS counters [ref|alt][mapq|qual|rpr][256] replicated [counter][copy], copy = lane mod C (the
// layout of hist_dense_kernel), folds the copies, and ranks with one thread per value.  A column whose observations all have one
// value -- the normal case for mapq -- would be C addresses for 64 lanes; so a wavefront first VOTES: the lanes whose counter is the
// first counting lane's are counted with a ballot and added by that one lane, only the others add for themselves.  The strand counts
// are ballots too, kept per wavefront in scalar registers.
#include "bvc_device.h"
#include "bvc_internal.h"

namespace bvc {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kStatsThreads = 512;                  // 8 wavefronts
constexpr int kStatsWaves = kStatsThreads / kWave;
constexpr int kStatsLoads = 4;                      // 16-byte loads per lane and trip
constexpr int kStatsCounters = 2 * 3 * 256;         // [ref|alt][mapq|qual|rpr][value]
// words of LDS behind the counter copies: the folded counters, per-wavefront strand counts [wave][4], the scan's per-wavefront
// sums [field][4 waves] and the per-wavefront partial sums of the products [field][4 waves] as (lo, hi) words
constexpr int kStatsTot = 0, kStatsStrand = kStatsCounters, kStatsScan = kStatsStrand + kStatsWaves * 4, kStatsProd = kStatsScan + 12,
              kStatsTailWords = kStatsProd + 24;

// One counter of every lane of the wavefront that has `on` set (wave-uniform control flow: every lane of the wavefront calls).
__device__ __forceinline__ void vote_add(uint32_t *cnt, bool on, uint32_t key, int log2c, uint32_t copy, int lane, uint32_t words)
{
    const uint64_t act = __ballot(on);
    if (act == 0) return;
    const int leader = __ffsll((unsigned long long)act) - 1;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
    const uint64_t same = __ballot(on && key == k0);
    const bool lead = lane == leader;
    if (lead || (on && key != k0)) {
        const uint32_t at = (key << log2c) | copy;
        if (BVC_LDS_OK(0x701, at, words)) atomicAdd(&cnt[at], lead ? (uint32_t)__popcll(same) : 1u);
    }
    (void)words;
}

// v of lane `src` mod 64 (ds_bpermute: no bound check of the lane, so none of its lane predicates either)
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }

}  // namespace

// stats[s] for every site; a site that is not called gets a zeroed record and none of its entries is read.
__global__ __launch_bounds__(kStatsThreads) void site_stats_kernel(
    int64_t n_sites, const int64_t *__restrict__ offsets, const bvc_pileup_entry *__restrict__ entries, const int8_t *__restrict__ ref_base,
    const bvc_site_result *__restrict__ results, bvc_site_stats *__restrict__ stats, int log2c)
{
    BVC_POISON_LDS();
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];          // [kStatsCounters][1 << log2c] + kStatsTailWords
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const uint32_t words = (uint32_t)kStatsCounters << log2c;
    const uint32_t copy = (uint32_t)lane & ((1u << log2c) - 1u);
    uint32_t *const cnt = lds;
    uint32_t *const tail = lds + words;
    for (uint32_t i = (uint32_t)tid * 4u; i < words; i += kStatsThreads * 4) *reinterpret_cast<u32x4 *>(&cnt[i]) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    for (int64_t site = blockIdx.x; site < n_sites; site += gridDim.x) {
        // (16-byte stores: the record array starts on a 16-byte boundary, include/bvc.h)
        u32x4 *const rec = reinterpret_cast<u32x4 *>(&stats[site]);
        if (results[site].called == 0) {                                      // (workgroup-uniform)
            if (tid < 4) rec[tid] = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
        // which bases are the reference / an alternative allele: a bit per base
        const int rb = ref_base[site];
        const uint32_t ref_mask = rb >= 0 && rb <= 3 ? 1u << rb : 0u;
        uint32_t alt_mask = 0;
        const int n_alt = results[site].n_alt < 3 ? results[site].n_alt : 3;
        for (int i = 0; i < n_alt; ++i) {
            const int ab = results[site].alt_base[i];
            if (ab >= 0 && ab <= 3) alt_mask |= 1u << ab;
        }
        alt_mask &= ~ref_mask;
        uint32_t n_rf = 0, n_rr = 0, n_af = 0, n_ar = 0;                      // this wavefront's strand counts (scalar)
        // w0 = base | mapq << 8 | qual << 16 | rpr << 24, w1 = strand | is_indel << 8
        auto count = [&](uint32_t w0, uint32_t w1, bool have) {
            const uint32_t base = w0 & 0xFFu;
            const bool counted = have && ((w1 >> 8) & 0xFFu) != 1u && base <= 3u;
            const uint32_t bit = 1u << (base & 3u);
            const bool is_ref = counted && (ref_mask & bit), is_alt = counted && (alt_mask & bit);
            const bool on = is_ref || is_alt, fwd = (w1 & 0xFFu) == 1u;
            n_rf += (uint32_t)__popcll(__ballot(is_ref && fwd)); n_rr += (uint32_t)__popcll(__ballot(is_ref && !fwd));
            n_af += (uint32_t)__popcll(__ballot(is_alt && fwd)); n_ar += (uint32_t)__popcll(__ballot(is_alt && !fwd));
            const uint32_t cls = is_ref ? 0u : 768u;
            vote_add(cnt, on, cls + ((w0 >> 8) & 0xFFu), log2c, copy, lane, words);
            vote_add(cnt, on, cls + 256u + ((w0 >> 16) & 0xFFu), log2c, copy, lane, words);
            vote_add(cnt, on, cls + 512u + (w0 >> 24), log2c, copy, lane, words);
        };
        // (a site holds fewer than 2^31 entries -- n_ref and n_alt are int32 -- so what indexes INSIDE a site is 32 bits wide)
        const int64_t o0 = offsets[site];
        const uint32_t n = (uint32_t)(offsets[site + 1] - o0);
        const bvc_pileup_entry *__restrict__ p = entries + o0;
        // entries are 8-byte aligned: the one in front of the first 16-byte boundary and the one behind the last pair go alone
        const uint32_t head = n > 0u && ((uintptr_t)p & 8u) ? 1u : 0u;
        const uint32_t n2 = (n - head) >> 1, last = head + 2u * n2;
        if (wave == 0 && (head || last < n)) {
            const bool have = lane == 0 ? head != 0u : (lane == 1 && last < n);
            u32x2 e = u32x2{0u, 0u};
            if (have) e = *reinterpret_cast<const u32x2 *>(p + (lane == 0 ? 0u : last));
            count(e.x, e.y, have);
        }
        const u32x4 *__restrict__ q = reinterpret_cast<const u32x4 *>(p + head);
        for (uint32_t j0 = (uint32_t)wave * kWave; j0 < n2; j0 += kStatsThreads * kStatsLoads) {                 // (wavefront-uniform)
            u32x4 v[kStatsLoads];
#pragma unroll
            for (int u = 0; u < kStatsLoads; ++u) {
                const uint32_t at = j0 + (uint32_t)u * kStatsThreads + (uint32_t)lane;
                v[u] = at < n2 ? q[at] : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < kStatsLoads; ++u) {
                const uint32_t first = j0 + (uint32_t)u * kStatsThreads;
                if (first >= n2) break;                                       // (wavefront-uniform)
                const bool have = first + (uint32_t)lane < n2;
                count(v[u].x, v[u].y, have);
                count(v[u].z, v[u].w, have);
            }
        }
        // the thread's index again, opaque to the compiler: what the steps below ask of it (is it below 256, is it lane 0 ...) is then
        // computed here, per site, and not kept in twenty scalar register pairs across the streaming loop
        int rt = tid;
        asm volatile("" : "+v"(rt));
        const int rl = rt & (kWave - 1), rw = rt >> 6;
        if (rl == 0) *reinterpret_cast<u32x4 *>(&tail[kStatsStrand + rw * 4]) = u32x4{n_rf, n_rr, n_af, n_ar};
        __syncthreads();
        // fold: the copies of a counter summed in an order rotated by the counter (the lanes of a wavefront start on different
        // banks) and left zero for the workgroup's next site
        for (int key = rt; key < kStatsCounters; key += kStatsThreads) {
            uint32_t sum = 0;
            for (int c = 0; c < (1 << log2c); ++c) {
                const uint32_t at = ((uint32_t)key << log2c) + (uint32_t)((c + key) & ((1 << log2c) - 1));
                sum += cnt[at]; cnt[at] = 0u;
            }
            tail[kStatsTot + key] = sum;
        }
        __syncthreads();
        // ranking: thread t < 256 is value 255 - t of all three fields (descending order); lo = exclusive prefix sum of r + a
        uint32_t r[3] = {0u, 0u, 0u}, a[3] = {0u, 0u, 0u};
        uint64_t incl[3] = {0u, 0u, 0u};
        if (rt < 256) {
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                r[f] = tail[kStatsTot + f * 256 + 255 - rt];
                a[f] = tail[kStatsTot + 768 + f * 256 + 255 - rt];
                uint32_t s = r[f] + a[f];                                     // (a site holds fewer than 2^31 entries)
                for (int d = 1; d < kWave; d <<= 1) {
                    // (the lanes below d add nothing: a mask from arithmetic, not a rl predicate held in scalar registers across the sites)
                    s += from_lane(s, rl - d) & (uint32_t)((d - 1 - rl) >> 31);
                }
                incl[f] = s;
                if (rl == kWave - 1) tail[kStatsScan + f * 4 + rw] = s;
            }
        }
        __syncthreads();
        if (rt < 256) {
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                uint64_t before = 0;
                for (int w = 0; w < rw; ++w) before += tail[kStatsScan + f * 4 + w];
                const uint64_t lo = before + incl[f] - (uint64_t)(r[f] + a[f]);
                uint64_t prod = (uint64_t)r[f] * (2u * lo + (uint64_t)r[f] + (uint64_t)a[f] + 1u);
                // (rl 0's sum takes in lanes 0..63 only; what wraps round reaches the other lanes' sums, which nobody reads)
                for (int d = kWave / 2; d > 0; d >>= 1)
                    prod += (uint64_t)from_lane((uint32_t)prod, rl + d) | ((uint64_t)from_lane((uint32_t)(prod >> 32), rl + d) << 32);
                if (rl == 0) {
                    tail[kStatsProd + (f * 4 + rw) * 2] = (uint32_t)prod;
                    tail[kStatsProd + (f * 4 + rw) * 2 + 1] = (uint32_t)(prod >> 32);
                }
            }
        }
        __syncthreads();
        if (rt == 0) {
            uint64_t rank2[3];
            for (int f = 0; f < 3; ++f) {
                rank2[f] = 0;
                for (int w = 0; w < 4; ++w)
                    rank2[f] += (uint64_t)tail[kStatsProd + (f * 4 + w) * 2] | ((uint64_t)tail[kStatsProd + (f * 4 + w) * 2 + 1] << 32);
            }
            uint32_t sc[4] = {0u, 0u, 0u, 0u};
            for (int w = 0; w < kStatsWaves; ++w)
                for (int k = 0; k < 4; ++k) sc[k] += tail[kStatsStrand + w * 4 + k];
            rec[0] = u32x4{(uint32_t)rank2[0], (uint32_t)(rank2[0] >> 32), (uint32_t)rank2[1], (uint32_t)(rank2[1] >> 32)};
            rec[1] = u32x4{(uint32_t)rank2[2], (uint32_t)(rank2[2] >> 32), sc[0] + sc[1], sc[2] + sc[3]};
            rec[2] = u32x4{sc[0], sc[1], sc[2], sc[3]};
            rec[3] = u32x4{1u, 0u, 0u, 0u};                                   // valid, pad
        }
        __syncthreads();                                                      // the tail words belong to the next site from here
    }
}

size_t site_stats_lds_bytes(int log2c) { return (((size_t)kStatsCounters << log2c) + kStatsTailWords) * sizeof(uint32_t); }

hipError_t launch_site_stats(LaunchState &st, hipStream_t stream, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                             const int8_t *ref_base, const bvc_site_result *results, bvc_site_stats *stats)
{
    if (n_sites <= 0) return hipSuccess;
    const int log2c = st.stats_log2c;
    const size_t lds = site_stats_lds_bytes(log2c);
    if (lds > 48 * 1024) {
        const hipError_t e = raise_lds(st, reinterpret_cast<const void *>(site_stats_kernel), site_stats_lds_bytes(kStatsMaxLog2c));
        if (e != hipSuccess) return e;
    }
    // (2048 workgroups: more than the chip holds at a time; the sites beyond them follow in each workgroup's loop)
    hipLaunchKernelGGL(site_stats_kernel, dim3((unsigned)(n_sites < 2048 ? n_sites : 2048)), dim3(kStatsThreads), lds, stream, n_sites,
                       offsets, entries, ref_base, results, stats, log2c);
    return hipGetLastError();
}

static_assert(sizeof(bvc_site_stats) == 64 && sizeof(bvc_pileup_entry) == 8, "record layouts of include/bvc.h");
static_assert(kSiteStatsTrip == kStatsThreads * kStatsLoads * 2, "the per-trip width the binding exposes");

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_site_stats)
#endif

}  // namespace bvc
