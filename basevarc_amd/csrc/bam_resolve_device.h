// bam_resolve_device.h -- what the kernels over a batch's inflated BAM records share (bam_pileup_kernel.hip, bam_popmatrix_kernel.hip,
// bam_text_kernel.hip, bam_counts_kernel.hip):
// the byte loads (records lie at any byte address), the lane helpers, a sample's clamped byte range and resolve(), the per-position
// rule of find_snp_at_pos / fetch_allele_type (host/bam.cpp) for ONE position over the read table bam_index_kernel leaves.  Device
// code, every function inlined into its kernel, and the one grid formula of the sample-per-wavefront kernels.
#ifndef BVC_BAM_RESOLVE_DEVICE_H
#define BVC_BAM_RESOLVE_DEVICE_H

#include "bvc_device.h"
#include "bvc_internal.h"

namespace bvc {

namespace {

constexpr int kBamThreads = 256;                    // 4 wavefronts: 4 samples (index, pileup, popmatrix) or 4 positions (rows)
constexpr int kBamWaves = kBamThreads / kWave;
// (host side) the grid of the kernels that give a sample a wavefront and a position a lane: kBamWaves samples a workgroup in x, the
// positions' chunks of 64 in y -- 1024 at most, more go round the kernel's loop
inline dim3 bam_sample_grid(int32_t n_samples, int32_t n_positions)
{
    const int64_t chunks = ((int64_t)n_positions + kWave - 1) / kWave;
    return dim3((unsigned)((n_samples + kBamWaves - 1) / kBamWaves), (unsigned)(chunks < 1024 ? chunks : 1024));
}

__device__ __forceinline__ uint32_t ld16(const uint8_t *__restrict__ p, int64_t at) { return (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t *__restrict__ p, int64_t at)
{
    return (uint32_t)p[at] | ((uint32_t)p[at + 1] << 8) | ((uint32_t)p[at + 2] << 16) | ((uint32_t)p[at + 3] << 24);
}

// v of lane `src` mod 64
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); }
__device__ __forceinline__ uint64_t from_lane64(uint64_t v, int src)
{
    return (uint64_t)from_lane((uint32_t)v, src) | ((uint64_t)from_lane((uint32_t)(v >> 32), src) << 32);
}
// the value every lane holds alike, as a scalar
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t uniform64(int64_t v) { return (int64_t)((uint64_t)uniform((uint32_t)v) | ((uint64_t)uniform((uint32_t)((uint64_t)v >> 32)) << 32)); }

// Sample s's bytes [lo, hi) of bam, whatever the two arrays say: inside the buffer, not negative.
__device__ __forceinline__ void sample_range(const int64_t *__restrict__ sample_off, const int64_t *__restrict__ sample_end, int32_t s,
                                             int64_t bam_bytes, int64_t &lo, int64_t &hi)
{
    lo = sample_off[s];
    hi = sample_end[s];
    lo = lo < 0 ? 0 : lo > bam_bytes ? bam_bytes : lo;
    hi = hi < lo ? lo : hi > bam_bytes ? bam_bytes : hi;
}

__device__ __forceinline__ uint32_t cigar_op(uint32_t c) { return (c & 15u) < 9u ? (c & 15u) : 0u; }     // MIDNSHP=X = 0..8, read_record's rule

// the character of a 4-bit base code: "=ACMGRSVTWYHKDBN", eight characters a word
__device__ __forceinline__ uint8_t nt16_char(uint32_t nib)
{
    const uint64_t w = nib < 8u ? 0x565352474d43413dull : 0x4e42444b48595754ull;
    return (uint8_t)(w >> ((nib & 7u) * 8u));
}

// What one (sample, position) resolves to.  size 0: no entry.
struct Hit {
    uint32_t size = 0;          // bytes of the entry: 9, or 11 + text for an indel entry
    uint32_t fields = 0;        // base | mapq << 8 | qual << 16 | rpr << 24 (an indel entry's mapq comes from the carry)
    uint32_t flags = 0;         // bit 0 strand, bit 1 indel entry
    uint32_t nib = 0;           // a base entry: the read's 4-bit base code (its character: nt16_char)
    uint32_t text_len = 0;      // the sign included, bounded by the binary entry's 16-bit length field
    uint32_t text_full = 0;     // the sign included, whole (the text form has no such field: bam_text_kernel.hip)
    uint32_t text_at = 0;       // insertion: index of the first base in the read
    int64_t text_src = 0;       // insertion: where the read's packed bases begin in bam; deletion: index into refseq
    bool deletion = false;
    bool out_of_range = false;  // the rule's out-of-range cases (status 4)
};

// find_snp_at_pos for ONE position p of a sample with n > 0 kept reads.  TEXT_FIRST: fetch_allele_type's order -- a zero-length I / D next
// whose text would start past its source is out of range too (find_snp_at_pos looks at such an operation only when its length is not 0).
template <bool TEXT_FIRST = false>
__device__ __forceinline__ Hit resolve(const uint8_t *__restrict__ bam, const BamRead *__restrict__ reads, const int32_t *__restrict__ runmax,
                                       uint32_t n, int32_t p, int32_t rg_s, int64_t refseq_len)
{
    Hit h;
    uint32_t a = 0, b = n - 1u;                     // first(p): the answer lies in [a, b]; it sticks at the last read
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (runmax[m] >= p) b = m; else a = m + 1u;
    }
    uint32_t j = a;
    BamRead r = reads[j];
    if (!((int64_t)p >= (int64_t)r.pos + 1 && p <= r.end)) return h;
    for (;;) {
        const int64_t q = r.off + 4;
        const uint32_t l_rn = bam[q + 8], mapq = bam[q + 9], n_cig = ld16(bam, q + 12), flag = ld16(bam, q + 14);
        const uint32_t l_seq = ld32(bam, q + 16);
        const int64_t c0 = q + 32 + l_rn, seq0 = c0 + 4 * (int64_t)n_cig;
        // the rule's four coordinates (host/bam.cpp): ref_after (sx), qry_after (sy), aln_after (track), shift_after (shift)
        uint32_t sx = (uint32_t)r.pos, sy = 0, track = (uint32_t)r.pos, shift = 0;
        bool have_ref = false, have_aln = false, at_end = false;
        uint32_t k_ref = 0, op_k = 0, sy_k = 0, shift_k = 0;
        for (uint32_t k = 0; k < n_cig && !(have_ref && have_aln); ++k) {
            const uint32_t c = ld32(bam, c0 + 4 * (int64_t)k), op = cigar_op(c), l = c >> 4;
            const uint32_t shift_prev = shift;
            if (op == 0u || op == 1u || op == 4u || op == 8u) sy += l;
            if (op != 5u && op != 1u) sx += l;
            if (op != 1u && op != 4u && op != 5u) track += l;
            if (op == 1u || op == 4u) shift += l;
            else if (op == 2u || op == 6u || op == 3u) shift -= l;
            if (!have_ref && (int32_t)sx >= p) { have_ref = true; k_ref = k; op_k = op; sy_k = sy; at_end = (int32_t)sx == p; }
            if (!have_aln && (int32_t)track >= p) { have_aln = true; shift_k = shift_prev; }
        }
        if (!have_ref) return h;                    // the CIGAR ends short of the position
        if (!have_aln) shift_k = shift;
        const uint32_t strand = (flag & 0x10u) || (flag & 0x20u) ? 0u : 1u;
        if (at_end && k_ref + 1u < n_cig) {         // last reference base of its operation: an insertion or deletion next is the token
            const uint32_t c2 = ld32(bam, c0 + 4 * (int64_t)(k_ref + 1u)), op2 = cigar_op(c2), l2 = c2 >> 4;
            if (TEXT_FIRST && (op2 == 2u || op2 == 1u) && l2 == 0u) {
                // FetchAlleleType builds the token's text before it looks at the length: a start past the source throws even so
                const int64_t start = (int64_t)p - (int64_t)rg_s + 1;
                if (op2 == 2u ? (start < 0 || start > refseq_len) : ((int32_t)sy_k < 0 || sy_k > l_seq)) { h.out_of_range = true; return h; }
            }
            if ((op2 == 2u || op2 == 1u) && l2 != 0u) {
                int64_t avail;
                if (op2 == 2u) {
                    const int64_t start = (int64_t)p - (int64_t)rg_s + 1;
                    if (start < 0 || start > refseq_len) { h.out_of_range = true; return h; }
                    avail = refseq_len - start;
                    h.deletion = true; h.text_src = start;
                } else {
                    if ((int32_t)sy_k < 0 || sy_k > l_seq) { h.out_of_range = true; return h; }
                    avail = (int64_t)l_seq - (int64_t)sy_k;
                    h.text_src = seq0; h.text_at = sy_k;
                }
                const int64_t tl = (int64_t)l2 < avail ? (int64_t)l2 : avail;
                h.text_len = tl + 1 < 0xffff ? (uint32_t)(tl + 1) : 0xffffu;
                h.text_full = (uint32_t)(tl + 1);
                h.size = 11u + h.text_len;
                h.fields = 5u | (mapq << 16);
                h.flags = strand | 2u;
                return h;
            }
        }
        if (op_k != 2u && op_k != 3u) {             // a base of this read
            const uint32_t off = (uint32_t)(p - (r.pos + 1)) + shift_k;
            if (l_seq == 0u || (int32_t)l_seq < 0 || off > l_seq - 1u) { h.out_of_range = true; return h; }
            const uint32_t nib = (bam[seq0 + (off >> 1)] >> ((off & 1u) ? 0 : 4)) & 15u;
            const uint32_t base = nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u;
            const uint32_t qual = bam[seq0 + (((int64_t)l_seq + 1) >> 1) + off];
            h.size = 9u;
            h.fields = base | (mapq << 8) | (qual << 16) | (((off + 1u) & 0xFFu) << 24);
            h.flags = strand;
            h.nib = nib;
            return h;
        }
        if (j + 1u >= n) return h;                  // deleted or skipped in this read: the next read, if it covers the position
        r = reads[++j];
        if (!((int64_t)p >= (int64_t)r.pos + 1 && p <= r.end)) return h;
    }
}

}  // namespace

}  // namespace bvc
#endif
