// store_kernel.hip -- temp batches kept on the device (include/bvc_store.h): the cumulative sizes of the kept batches, and a tile of
// positions gathered from all of them into the tile buffer that pileup_bin_kernel parses.
//
//   store_cum_kernel      cum[t] += rec_start[t] of a batch that has just been put: 64-bit atomic adds, batches put side by side commute.
//   store_plan_kernel     per batch the slice rec_start[t0] .. rec_start[t0 + T] of its records, clamped into the batch's allocation,
//                         its place in the tile buffer and its first work item.  Slice b goes to the first address behind slice b - 1 that
//                         is congruent to its source mod 16 (at most 15 pad bytes a batch), so both sides of the copy are 16-byte accesses;
//                         that recurrence and the items' prefix sum are one lane's walk over LDS, the loads around it all lanes'.
//   store_rows_kernel     the tile's table: row b = dst[b] + rec_start_b[t0 + t] - rec_start_b[t0], every word clamped into the slice.
//   store_gather_kernel   the copy, cut into items of BVC_STORE_CHUNK bytes (slices range from 4 * T bytes to many MB: not a workgroup a
//                         batch); a capped grid whose workgroups loop over the items.  An item: bytes to the first 16-byte boundary, 16-byte
//                         vectors with every load issued before the first store, bytes behind the last whole vector.
// A batch's addresses come out of a table in device memory: they are turned into global-address-space pointers, never generic ones.  No
// word read from a rec_start row reaches an address before it is clamped with the batch's size (the row of a bvc_store_put came from a
// caller).
#include "bvc_device.h"
#include "bvc_internal.h"
#include "../../include/bvc_store.h"

namespace bvc {

namespace {

constexpr int kStoreThreads = 256;
constexpr int kPlanBlock = 1024;         // batches per round of the plan kernel's walk
constexpr uint32_t kChunk = BVC_STORE_CHUNK;
static_assert(kChunk == 16u * kStoreThreads * 4u, "an item is four 16-byte vectors a thread");

typedef const __attribute__((address_space(1))) uint32_t *GlobalWords;
typedef const __attribute__((address_space(1))) uint8_t *GlobalBytes;
typedef uint32_t Vec16 __attribute__((ext_vector_type(4)));     // 16 bytes: one global_load_dwordx4 / global_store_dwordx4
typedef const __attribute__((address_space(1))) Vec16 *GlobalVecs;

__global__ __launch_bounds__(kStoreThreads) void store_cum_kernel(const uint32_t *__restrict__ rec_start, int32_t n_words,
                                                                  unsigned long long *__restrict__ cum)
{
    for (int64_t i = (int64_t)blockIdx.x * kStoreThreads + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * kStoreThreads)
        atomicAdd(&cum[i], (unsigned long long)rec_start[i]);
}

__global__ __launch_bounds__(kStoreThreads) void store_plan_kernel(const StoreBatch *__restrict__ batches, int32_t n_batches, int32_t t0, int32_t T,
                                                                   StorePlan P)
{
    BVC_POISON_LDS();
    __shared__ uint32_t s_len[kPlanBlock], s_mod[kPlanBlock], s_dst[kPlanBlock], s_item[kPlanBlock];
    __shared__ unsigned long long s_cursor;
    __shared__ uint32_t s_items;
    if (threadIdx.x == 0) { s_cursor = 0; s_items = 0; }
    for (int32_t base = 0; base < n_batches; base += kPlanBlock) {
        const int32_t n = n_batches - base < kPlanBlock ? n_batches - base : kPlanBlock;
        __syncthreads();
        for (int32_t i = threadIdx.x; i < n; i += kStoreThreads) {
            const StoreBatch B = batches[base + i];
            const GlobalWords rs = (GlobalWords)(uintptr_t)B.rec_start;
            uint64_t a = rs[t0], e = rs[t0 + T];
            a = a < B.bytes ? a : B.bytes;                           // clamped before anything is made of them
            e = e < a ? a : e < B.bytes ? e : B.bytes;
            P.lo[base + i] = (uint32_t)a;
            P.len[base + i] = (uint32_t)(e - a);
            s_len[i] = (uint32_t)(e - a);
            s_mod[i] = (uint32_t)((B.records + a) & 15u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long cursor = s_cursor;
            uint32_t items = s_items;
            for (int32_t i = 0; i < n; ++i) {
                cursor += (s_mod[i] - (uint32_t)cursor) & 15u;
                s_dst[i] = (uint32_t)(cursor < 0xFFFFFFFFull ? cursor : 0xFFFFFFFFull);   // (past 32 bits: the gather refuses the slice)
                s_item[i] = items;
                cursor += s_len[i];
                items += (s_len[i] + kChunk - 1u) / kChunk;
            }
            s_cursor = cursor; s_items = items;
        }
        __syncthreads();
        for (int32_t i = threadIdx.x; i < n; i += kStoreThreads) { P.dst[base + i] = s_dst[i]; P.first_item[base + i] = s_item[i]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) { P.first_item[n_batches] = s_items; *P.used = s_cursor; }
}

__global__ __launch_bounds__(kStoreThreads) void store_rows_kernel(const StoreBatch *__restrict__ batches, int32_t n_batches, int32_t t0, int32_t T,
                                                                   StorePlan P, uint32_t *__restrict__ rows)
{
    for (int32_t b = blockIdx.y; b < n_batches; b += gridDim.y) {
        const GlobalWords rs = (GlobalWords)(uintptr_t)batches[b].rec_start;
        const uint32_t lo = P.lo[b], hi = lo + P.len[b], dst = P.dst[b];
        for (int32_t t = blockIdx.x * kStoreThreads + threadIdx.x; t <= T; t += gridDim.x * kStoreThreads) {
            uint32_t r = rs[t0 + t];
            r = r < lo ? lo : r > hi ? hi : r;
            rows[(int64_t)b * (T + 1) + t] = dst + (r - lo);
        }
    }
}

__global__ __launch_bounds__(kStoreThreads) void store_gather_kernel(const StoreBatch *__restrict__ batches, int32_t n_batches, StorePlan P,
                                                                     uint8_t *__restrict__ tile, uint64_t tile_cap)
{
    const uint32_t n_items = P.first_item[n_batches];
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        int32_t b = 0, above = n_batches;                           // the last batch whose first item is not behind this one: the one that holds it
        while (above - b > 1) {
            const int32_t mid = b + (above - b) / 2;
            if (P.first_item[mid] <= item) b = mid; else above = mid;
        }
        const StoreBatch B = batches[b];
        const uint32_t lo = P.lo[b], len = P.len[b], dst = P.dst[b], at = (item - P.first_item[b]) * kChunk;
        if (at >= len || (uint64_t)lo + len > B.bytes || (uint64_t)dst + len > tile_cap) continue;     // (what the plan and the host's sizes rule out)
        const uint32_t n = len - at < kChunk ? len - at : kChunk;
        const uint64_t from = B.records + lo + at;
        const GlobalBytes src = (GlobalBytes)(uintptr_t)from;
        uint8_t *const to = tile + dst + at;                        // congruent to `from` mod 16: dst is, `at` is a multiple of 16
        uint32_t head = (uint32_t)(16u - (from & 15u)) & 15u;
        head = head < n ? head : n;
        if (threadIdx.x < head) to[threadIdx.x] = src[threadIdx.x];
        const uint32_t n_vec = (n - head) >> 4;
        const GlobalVecs sv = (GlobalVecs)(uintptr_t)(from + head);
        Vec16 *const dv = reinterpret_cast<Vec16 *>(to + head);
        Vec16 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = threadIdx.x + (uint32_t)j * kStoreThreads;
            if (i < n_vec) v[j] = sv[i];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = threadIdx.x + (uint32_t)j * kStoreThreads;
            if (i < n_vec) dv[i] = v[j];
        }
        const uint32_t done = head + (n_vec << 4);
        if (threadIdx.x < n - done) to[done + threadIdx.x] = src[done + threadIdx.x];
    }
}

}  // namespace

hipError_t launch_store_cum(hipStream_t stream, const uint32_t *rec_start, int32_t n_words, unsigned long long *cum)
{
    if (n_words <= 0) return hipSuccess;
    const int64_t blocks = ((int64_t)n_words + kStoreThreads - 1) / kStoreThreads;
    hipLaunchKernelGGL(store_cum_kernel, dim3((unsigned)(blocks < kStoreGrid ? blocks : kStoreGrid)), dim3(kStoreThreads), 0, stream, rec_start, n_words, cum);
    return hipGetLastError();
}

hipError_t launch_store_gather(hipStream_t stream, const StoreBatch *batches, int32_t n_batches, int32_t t0, int32_t T, const StorePlan &plan,
                               uint8_t *tile, int64_t tile_cap, uint32_t *rows)
{
    if (n_batches <= 0) return hipSuccess;
    hipLaunchKernelGGL(store_plan_kernel, dim3(1), dim3(kStoreThreads), 0, stream, batches, n_batches, t0, T, plan);
    const int64_t row_blocks = ((int64_t)T + 1 + kStoreThreads - 1) / kStoreThreads;
    hipLaunchKernelGGL(store_rows_kernel, dim3((unsigned)(row_blocks < 64 ? row_blocks : 64), (unsigned)(n_batches < kStoreGrid ? n_batches : kStoreGrid)),
                       dim3(kStoreThreads), 0, stream, batches, n_batches, t0, T, plan, rows);
    // the items: no more than a chunk's worth of the tile's bytes each, and the last, short one of every batch
    const int64_t items = tile_cap / kChunk + n_batches;
    hipLaunchKernelGGL(store_gather_kernel, dim3((unsigned)(items < kStoreGrid ? items : kStoreGrid)), dim3(kStoreThreads), 0, stream, batches, n_batches,
                       plan, tile, (uint64_t)tile_cap);
    return hipGetLastError();
}

}  // namespace bvc
