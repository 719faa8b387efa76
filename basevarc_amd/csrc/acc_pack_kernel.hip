// acc_pack_kernel.hip -- the kernels of the eleventh header (include/bvc_site_acc_pack.h): an accumulator's rows <-> their SPARSE form, the
// non-zero words of a position's LOGICAL row (class counts in the wide layout, tally words 0..9, depth words) as (cell, count) entries
// behind a row_start table.  The project's shape for such work: a SIZE pass and a PLACE pass over the same loads, a scan between them.
//
//   acc_pack_kernel<PLACE>         one wavefront a row, grid-strided over rows; the lanes take the row's 16-byte pieces in rounds of 64: the
//                                  count pieces (physical -> logical for narrow rows, as acc_expand_kernel maps them), the tally's three with
//                                  words 10 and 11 masked, the depth pieces.  PLACE = false: row_n[t] = the non-zero words (popcounts of
//                                  four ballots a round).  PLACE = true: a lane's rank in the row is mbcnt over the same ballots plus a running
//                                  base across rounds -- lane order across rounds is ascending cell order -- and it writes cell and count;
//                                  a rank is compared with the row's size in row_start before an address is made of it.
//   acc_pack_scan_kernel           one wavefront: row_n [n] -> row_start [n + 1] (64-bit, exclusive), four rows a lane and round
//   acc_add_packed_kernel<ADD>     one wavefront a row, lanes stride over the row's entries.  ADD = false: only raises the row's fault
//                                  (row_fault[t], 0: none) -- the row_start words, a cell >= W, cells that do not ascend strictly, on narrow
//                                  rows a count cell whose quality has no column.  ADD = true: a cell is translated to an address for the
//                                  accumulator's kind and its count added; every cell (and the row's place in the entries) is compared
//                                  with the bounds again before an address is made of it, whatever the dry pass found.
//   acc_first_fault_kernel         one wavefront: the first row whose fault is not 0, as first_status_kernel finds a status
// No LDS.  The adds are 32-bit integer atomics on global memory that return nothing; several launches (of several contexts) may add into
// the same arrays at once.  All index arithmetic is 64-bit: a chromosome's rows hold more than 2^32 words and may hold as many entries.
#include "bam_resolve_device.h"
#include "../../include/bvc_site_acc_pack.h"

namespace bvc {

constexpr int kPackThreads = 256;                   // 4 wavefronts, a row each
constexpr int kPackWaves = kPackThreads / kWave;
constexpr int kPackGrid = 704;                      // workgroups at most (2,816 rows a grid round): more rows go round the loop again

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Piece p (< s.count_pieces + 3 + s.depth_groups) of row `row`, and the logical cell of its first word.  ONE 16-byte load from the address
// the three kinds of piece select, and the tally's pad words masked behind it (a load in each branch is split into 8-byte halves).
__device__ __forceinline__ uint4 load_piece(const uint4 *__restrict__ counts, const uint4 *__restrict__ tally, const uint4 *__restrict__ depth,
                                            int64_t row, uint32_t p, const AccRowShape &s, uint32_t &cell0)
{
    // narrow rows: piece p is the qualities 4 * (p % q4) .. + 3 of base p / q4, q4 = n_quals / 4 (four bases: no division)
    const uint32_t base = s.q4 ? (uint32_t)(p >= s.q4) + (uint32_t)(p >= 2u * s.q4) + (uint32_t)(p >= 3u * s.q4) : 0u;
    const uint32_t j = p - s.count_pieces;          // (p >= count_pieces: tally piece j < 3, else depth piece j - 3)
    const uint4 *src = counts + (row * (int64_t)s.count_pieces + (int64_t)p);
    cell0 = s.q4 ? base * 128u + (p - base * s.q4) * 4u : p * 4u;
    uint32_t keep = 0xFFFFFFFFu;
    if (p >= s.count_pieces) {
        src = j < 3u ? tally + (row * 3 + (int64_t)j) : depth + (row * (int64_t)s.depth_groups + (int64_t)(j - 3u));
        cell0 = s.count_cells + (j < 3u ? j * 4u : 10u + (j - 3u) * 4u);
        if (j == 2u) keep = 0u;                     // the tally's pad words are no part of the row
    }
    uint4 v = *src;
    v.z &= keep; v.w &= keep;
    return v;
}

}  // namespace

template <bool PLACE>
__global__ __launch_bounds__(kPackThreads) void acc_pack_kernel(int64_t n_rows, AccRowShape s, const uint4 *__restrict__ counts,
                                                                const uint4 *__restrict__ tally, const uint4 *__restrict__ depth,
                                                                uint32_t *__restrict__ row_n, const int64_t *__restrict__ row_start,
                                                                uint16_t *__restrict__ cell, uint32_t *__restrict__ count)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)uniform(blockIdx.x * kPackWaves + (threadIdx.x >> 6));
    const uint32_t pieces = s.count_pieces + 3u + s.depth_groups;
    for (int64_t t = wave; t < n_rows; t += (int64_t)gridDim.x * kPackWaves) {
        int64_t at = 0;
        uint32_t limit = 0u;
        if (PLACE) {
            at = uniform64(row_start[t]);
            const int64_t size = uniform64(row_start[t + 1]) - at;
            limit = size < 0 ? 0u : size > 0x7FFFFFFF ? 0x7FFFFFFFu : (uint32_t)size;
        }
        uint32_t done = 0u;                         // the row's entries in front of this round
        for (uint32_t p0 = 0u; p0 < pieces; p0 += kWave) {
            const uint32_t p = p0 + lane;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            uint32_t cell0 = 0u;
            if (p < pieces) v = load_piece(counts, tally, depth, s.row0 + t, p, s, cell0);
            const uint64_t bx = __ballot(v.x != 0u), by = __ballot(v.y != 0u), bz = __ballot(v.z != 0u), bw = __ballot(v.w != 0u);
            if (PLACE) {
                uint32_t rank = done + lanes_below(bx) + lanes_below(by) + lanes_below(bz) + lanes_below(bw);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0u; k < 4u; ++k)
                    if (w[k] != 0u) {
                        if (rank < limit) {
                            cell[at + (int64_t)rank] = (uint16_t)(cell0 + k);
                            count[at + (int64_t)rank] = w[k];
                        }
                        ++rank;
                    }
            }
            done += (uint32_t)(__popcll(bx) + __popcll(by) + __popcll(bz) + __popcll(bw));
        }
        if (!PLACE && lane == 0u) row_n[t] = done;
    }
}

// row_start[t] = the sum of row_n[0 .. t), t = 0 .. n_rows: four rows a lane, 256 a round, the carry in 64 bits
__global__ __launch_bounds__(kWave) void acc_pack_scan_kernel(int64_t n_rows, const uint32_t *__restrict__ row_n, int64_t *__restrict__ row_start)
{
    const int lane = threadIdx.x;
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < n_rows; t0 += kWave * 4) {
        const int64_t t = t0 + (int64_t)lane * 4;
        uint32_t a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = t + k < n_rows ? row_n[t + k] : 0u;
        const uint32_t mine = a[0] + a[1] + a[2] + a[3];                  // (a row has fewer than 2^16 entries)
        uint32_t incl = mine;
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = from_lane(incl, lane - d);
            if (lane >= d) incl += o;
        }
        int64_t at = carry + (int64_t)(incl - mine);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (t + k < n_rows) row_start[t + k] = at;
            at += (int64_t)a[k];
        }
        carry += (int64_t)from_lane(incl, kWave - 1);
    }
    if (lane == 0) row_start[n_rows] = carry;
}

template <bool ADD>
__global__ __launch_bounds__(kPackThreads) void acc_add_packed_kernel(int64_t n_rows, AccRowShape s, uint32_t n_quals, uint32_t row_words,
                                                                      const int64_t *__restrict__ row_start, const uint16_t *__restrict__ cell,
                                                                      const uint32_t *__restrict__ count, int64_t n_entries,
                                                                      uint32_t *__restrict__ counts, uint32_t *__restrict__ tally,
                                                                      uint32_t *__restrict__ depth, uint32_t *__restrict__ row_fault)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)uniform(blockIdx.x * kPackWaves + (threadIdx.x >> 6));
    for (int64_t t = wave; t < n_rows; t += (int64_t)gridDim.x * kPackWaves) {
        const int64_t a = uniform64(row_start[t]), b = uniform64(row_start[t + 1]);
        // what the row's two words must be before an entry is read through them
        const bool bad = (t == 0 && a != 0) || a < 0 || b < a || b > n_entries || (t == n_rows - 1 && b != n_entries);
        if (bad) {
            if (!ADD && lane == 0u) row_fault[t] = kAccFaultRowStart;
            continue;
        }
        const int64_t row = s.row0 + t;
        uint32_t fault = 0u;
        for (int64_t i0 = a; i0 < b; i0 += kWave) {
            const int64_t i = i0 + (int64_t)lane;
            const bool in = i < b;
            const uint32_t c = in ? (uint32_t)cell[i] : 0u;
            if (!ADD) {
                uint32_t f = 0u;
                if (in) {
                    if (c >= row_words) f = kAccFaultCell;
                    else if (i > a && c <= (uint32_t)cell[i - 1]) f = kAccFaultOrder;
                    else if (c < s.count_cells && (c & 127u) >= n_quals) f = kAccFaultQual;
                }
                const uint64_t m = __ballot(f != 0u);
                if (m) { fault = uniform(from_lane(f, (int)__builtin_ctzll(m))); break; }       // the row's first entry at fault
                continue;
            }
            if (!in || c >= row_words) continue;
            const uint32_t v = count[i];
            if (v == 0u) continue;
            if (c < s.count_cells) {
                if (s.q4 == 0u) atomicAdd(counts + (row * (int64_t)s.count_cells + (int64_t)c), v);
                else if ((c & 127u) < n_quals) atomicAdd(counts + ((row * 4 + (int64_t)(c >> 7)) * (int64_t)n_quals + (int64_t)(c & 127u)), v);
            } else if (c < s.count_cells + 10u)
                atomicAdd(tally + (row * (int64_t)(sizeof(bvc_bam_site_tally) / 4) + (int64_t)(c - s.count_cells)), v);
            else
                atomicAdd(depth + (row * (int64_t)s.depth_groups * 4 + (int64_t)(c - s.count_cells - 10u)), v);
        }
        if (!ADD && lane == 0u) row_fault[t] = fault;
    }
}

// out[0] = the first row whose fault is not 0 (0x7FFFFFFFFFFFFFFF: none), out[1] = that fault
__global__ __launch_bounds__(kWave) void acc_first_fault_kernel(int64_t n_rows, const uint32_t *__restrict__ row_fault, int64_t *__restrict__ out)
{
    const int lane = threadIdx.x;
    int64_t first = 0x7FFFFFFFFFFFFFFFll;
    uint32_t code = 0u;
    for (int64_t t0 = 0; t0 < n_rows; t0 += kWave) {
        const int64_t t = t0 + lane;
        const uint32_t f = t < n_rows ? row_fault[t] : 0u;
        const uint64_t m = __ballot(f != 0u);
        if (m) {
            const int src = (int)__builtin_ctzll(m);
            first = t0 + src;
            code = from_lane(f, src);
            break;
        }
    }
    if (lane == 0) { out[0] = first; out[1] = (int64_t)code; }
}

namespace {

unsigned pack_grid(int64_t n_rows)
{
    const int64_t blocks = (n_rows + kPackWaves - 1) / kPackWaves;
    return (unsigned)(blocks < kPackGrid ? blocks : kPackGrid);
}

}  // namespace

hipError_t launch_acc_pack(hipStream_t stream, bool place, int64_t n_rows, const AccRowShape &s, const uint32_t *counts, const ::bvc_bam_site_tally *tally,
                           const uint32_t *depth, uint32_t *row_n, const int64_t *row_start, uint16_t *cell, uint32_t *count)
{
    if (n_rows < 0 || s.row0 < 0 || (s.depth_groups > 0u && !depth)) return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    const uint4 *c4 = reinterpret_cast<const uint4 *>(counts), *t4 = reinterpret_cast<const uint4 *>(tally), *d4 = reinterpret_cast<const uint4 *>(depth);
    if (place)
        hipLaunchKernelGGL(acc_pack_kernel<true>, dim3(pack_grid(n_rows)), dim3(kPackThreads), 0, stream, n_rows, s, c4, t4, d4, row_n, row_start, cell, count);
    else
        hipLaunchKernelGGL(acc_pack_kernel<false>, dim3(pack_grid(n_rows)), dim3(kPackThreads), 0, stream, n_rows, s, c4, t4, d4, row_n, row_start, cell, count);
    return hipGetLastError();
}

hipError_t launch_acc_pack_scan(hipStream_t stream, int64_t n_rows, const uint32_t *row_n, int64_t *row_start)
{
    if (n_rows < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(acc_pack_scan_kernel, dim3(1), dim3(kWave), 0, stream, n_rows, row_n, row_start);
    return hipGetLastError();
}

hipError_t launch_acc_add_packed(hipStream_t stream, bool add, int64_t n_rows, const AccRowShape &s, const int64_t *row_start, const uint16_t *cell,
                                 const uint32_t *count, int64_t n_entries, uint32_t *counts, ::bvc_bam_site_tally *tally, uint32_t *depth,
                                 uint32_t *row_fault)
{
    if (n_rows < 0 || s.row0 < 0 || n_entries < 0 || s.q4 >= 32u || (s.depth_groups > 0u && !depth)) return hipErrorInvalidValue;
    if (n_rows == 0) return hipSuccess;
    const uint32_t n_quals = s.q4 ? s.q4 * 4u : 128u, row_words = s.count_cells + 10u + 4u * s.depth_groups;
    uint32_t *const tw = reinterpret_cast<uint32_t *>(tally);
    if (add)
        hipLaunchKernelGGL(acc_add_packed_kernel<true>, dim3(pack_grid(n_rows)), dim3(kPackThreads), 0, stream, n_rows, s, n_quals, row_words, row_start,
                           cell, count, n_entries, counts, tw, depth, row_fault);
    else
        hipLaunchKernelGGL(acc_add_packed_kernel<false>, dim3(pack_grid(n_rows)), dim3(kPackThreads), 0, stream, n_rows, s, n_quals, row_words, row_start,
                           cell, count, n_entries, counts, tw, depth, row_fault);
    return hipGetLastError();
}

hipError_t launch_acc_first_fault(hipStream_t stream, int64_t n_rows, const uint32_t *row_fault, int64_t *out)
{
    hipLaunchKernelGGL(acc_first_fault_kernel, dim3(1), dim3(kWave), 0, stream, n_rows, row_fault, out);
    return hipGetLastError();
}

}  // namespace bvc
