// em_common.h -- what the two stage-2 engines (em_kernel.hip: one wavefront per site; em_items.hip: the item engine) must
// state identically to agree to rounding: the reference's constants, the convergence bracket, combs_ and the rules that turn
// a fitted model into a record.  Device side only; both translation units include it and hold no copy of their own.
#pragma once
#include "bvc_device.h"

namespace bvc {

constexpr double kLrtThreshold = 24.0;    // LRT_THRESHOLD, src/BaseType.h:9
constexpr int kEmIters = 100;             // src/BaseType.cpp:46
constexpr double kEmEpsilon = 0.001;      // src/BaseType.cpp:45
// var_qual is >= 0 or NaN; this marks records whose chi-square tail is still to be evaluated.  The libm-style
// log/exp/log10 of that step live in their own small kernel (var_qual_kernel, em_kernel.hip) so that their constants and
// registers stay out of the EM kernels (hoisted into VGPRs across the site loop they cost the wave kernel half its occupancy).
constexpr double kVarQualPending = -1.0;

// The stop rule delta = sum_c n_c |log m_c' - log m_c| < kEmEpsilon (delta_bylog, src/Algorithm.cpp:103-113) is bracketed
// instead of evaluated.  With u_c = m_c' / m_c - 1, delta = sum_c n_c |log1p(u_c)|, and with A = sum_c n_c |u_c| (one FMA per
// class in em_kernel.hip; sum_b |f'_b - f_b| D_b in em_items.hip, the same number):
//   A >= eps / (1 - 2^-8): not converged.  Either some |u| >= 2^-9, and that class alone (n_c >= 1) gives
//        delta > 1.9e-3; or every |u| < 2^-9, where |log1p(u)| >= |u| (1 - 2^-9), so delta >= eps.
//   A <  eps / (1 + 2^-8): every n_c |u_c| < eps, so every |u| < 2^-9, |log1p(u)| <= |u| (1 + 2^-9) and
//        delta < eps: converged.
//   in between (a few passes per fit at most): delta itself, log1p as a cubic (truncation 3e-12 relative),
//        with a reduction of its own.
// A is a sum of non-negative doubles (or NaN), so both comparisons are unsigned compares of its high
// word, done on the scalar unit; NaN and +inf compare high: "NaN never converges", as in the reference.
constexpr uint32_t hi_word(double x) { return (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32); }
constexpr uint32_t kSureBelowHi = hi_word(kEmEpsilon / (1.0 + 0.00390625));        // hi(A) <  this: converged
constexpr uint32_t kSureAboveHi = hi_word(kEmEpsilon / (1.0 - 0.00390625)) + 1u;   // hi(A) >= this: not converged

// k-subsets of positions 0..n-1 in lexicographic order (what combs_ yields, src/BaseType.cpp:237-255), as 4-bit position
// masks packed least-significant first; count returned through `cnt`.
__device__ __forceinline__ uint32_t subset_masks(int n, int k, int &cnt)
{
    switch (n * 8 + k) {
    case 1 * 8 + 1: cnt = 1; return 0x1u;
    case 2 * 8 + 2: cnt = 1; return 0x3u;
    case 2 * 8 + 1: cnt = 2; return 0x21u;
    case 3 * 8 + 3: cnt = 1; return 0x7u;
    case 3 * 8 + 2: cnt = 3; return 0x653u;
    case 3 * 8 + 1: cnt = 3; return 0x421u;
    case 4 * 8 + 4: cnt = 1; return 0xFu;
    case 4 * 8 + 3: cnt = 4; return 0xEDB7u;
    case 4 * 8 + 2: cnt = 6; return 0xCA6953u;
    case 4 * 8 + 1: cnt = 4; return 0x8421u;
    default: cnt = 0; return 0u;
    }
}

// v[j] of a per-base array held in registers (selects, no indexed access)
__device__ __forceinline__ double pick4(const double (&v)[4], int j)
{
    return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
}

__device__ __forceinline__ int32_t pick4(const int32_t (&v)[4], int j)
{
    return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
}

// var_qual of a site that has an ALT (src/BaseType.cpp:117-135): `n` bases in the accepted model, the first of them with
// `depth_first` observations.  The chi-square tail of the general case is left to var_qual_kernel.
__device__ __forceinline__ double call_var_qual(int n, int32_t depth_first, double depth_total, double chi)
{
    const double r = (double)depth_first / depth_total;
    if (n == 1 && depth_total > 10 && r > 0.5) return 5000.0;
    if (chi <= 0) return 0.0;
    return kVarQualPending;                                      // chisf(chi, 1): finished by var_qual_kernel
}

// Group record of a (site, group) that got no run of its own (src/BaseVarC.cpp:633-636, 640): the depth columns alone.
__device__ __forceinline__ bvc_group_result group_record_depths(int d0, int d1, int d2, int d3)
{
    bvc_group_result r;
    for (int j = 0; j < 3; ++j) r.af[j] = 0.0;
    r.depth[0] = d0; r.depth[1] = d1; r.depth[2] = d2; r.depth[3] = d3;
    r.ran = 0; r.present = 0;
    for (int j = 0; j < 6; ++j) r.pad[j] = 0;
    return r;
}

}  // namespace bvc
