// bvc_bam_counts.hip -- the inflated BAM records of a batch of samples added into per-position class counts and tallies
// (bam_counts_kernel.hip), and the accumulator bvc_site_acc that keeps such counts on the device.  Every form of the call -- bvc_bam_counts
// (include/bvc_bam_counts.h), bvc_bam_counts_depth (bvc_bam_group_depth.h), bvc_bam_counts_quals (bvc_site_acc_quals.h), and
// bvc_bam_counts_bgzf_acc on any accumulator -- is one path that a CountsLayout (counts_layout.h) steers: index -> dry pass -> scan -> first
// wait -> verdict (on narrow rows status 5 behind the others) -> add pass (-> second wait in the host forms); nothing is added unless the
// call returns BVC_OK.  The call's inputs (BamCall), their checks, their staging (BamStage) and the verdicts on the statuses and the blocks
// are bvc_bam.hip's.  Reading an accumulator: bvc_site_acc_get and bvc_site_acc_lrt (narrow rows pass through acc_expand_kernel), and
// bvc_site_acc_pack / bvc_site_acc_add_packed (bvc_site_acc_pack.h; acc_pack_kernel.hip), its rows as the entries of their non-zero words
// and back: size pass -> scan -> the wait for the total -> place pass, and dry pass -> first fault -> the wait for the verdict -> add pass.
#include "bvc_ctx.h"
#include "../../include/bvc_site_acc_pack.h"

// An accumulator is no part of a context: its device memory is its own, and its bookkeeping is fixed when it is made (the adds are atomic).
struct bvc_site_acc {
    int device = -1;
    int32_t n_positions = 0;
    int64_t budget = 0, used = 0;
    CountsLayout layout = CountsLayout::wide(0);
    uint32_t *d_counts = nullptr;                    // [n_positions][layout.count_words()]
    bvc_bam_site_tally *d_tally = nullptr;           // [n_positions]
    uint32_t *d_depth = nullptr;                     // [n_positions][layout.depth_groups][4]
};

// Rows a call expands at a time into the context's scratch (bvc_site_acc_get, bvc_site_acc_lrt on narrow rows): 64 MiB of [512] rows
constexpr int32_t kExpandRows = 32768;

namespace {

int check_acc(bvc_ctx *ctx, const bvc_site_acc *acc)
{
    if (!acc) return fail(ctx, BVC_ERR_ARG, "null accumulator");
    if (acc->device != ctx->device) return fail(ctx, BVC_ERR_ARG, "the accumulator lies on another device than the context");
    return BVC_OK;
}

int check_rows(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n)
{
    if (t0 < 0 || n < 0 || n > acc->n_positions - t0) return fail(ctx, BVC_ERR_ARG, "rows outside the accumulator");
    return BVC_OK;
}

// The labels' check of every form.  depth_form: the depths' forms with groups -- there is no such form without groups, and it words both
// refusals its own way
int check_labels(bvc_ctx *ctx, int32_t n_samples, const uint8_t *group_of_sample, int32_t n_groups, bool depth_form)
{
    if (n_groups < (depth_form ? 1 : 0) || n_groups > BVC_MAX_GROUPS)
        return fail(ctx, BVC_ERR_ARG, depth_form ? "n_groups must be 1..32" : "n_groups must be 0..32");
    if (n_groups > 0 && n_samples > 0 && !group_of_sample)
        return fail(ctx, BVC_ERR_ARG, depth_form ? "null group_of_sample with samples present" : "null group_of_sample with n_groups > 0");
    return BVC_OK;
}

// What every entry point checks of the sample and position arguments (h: the caller's pointers) before anything of the device is touched.
// n_groups: the groups the labels are compared with (CountsLayout::label_groups(), unchecked); a depth form names its labels behind the
// null pointers, the others in front of them.
int check_counts_call(bvc_ctx *ctx, const BamCall &h, const uint8_t *group_of_sample, int32_t n_groups, bool depth_form, const uint32_t *sample_status)
{
    int rc = check_sizes(ctx, h.n_samples, h.bam_bytes, h.n_positions, h.refseq_len, 0);
    if (rc != BVC_OK) return rc;
    if (!depth_form && (rc = check_labels(ctx, h.n_samples, group_of_sample, n_groups, false)) != BVC_OK) return rc;
    if ((h.n_samples > 0 && (!h.off || !h.end || !h.eof || !h.rid || !sample_status)) || (h.n_positions > 0 && !h.pos))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    return depth_form ? check_labels(ctx, h.n_samples, group_of_sample, n_groups, true) : BVC_OK;
}

// Index, dry pass, scan and the call's first wait, on inputs in device memory: the statuses (to sample_status on the host unless
// out_device) and the verdict -- the blocks' first (blocks: their statuses come down with the same wait; may be null), then the samples'.
// Narrow rows: their dry pass also raises status 5, whose first sample comes down with the same wait and is judged behind the existing
// verdict.
int bam_counts_verdict(bvc_ctx *ctx, PinIO &io, const BamCall &c, const CountsLayout &layout, bool out_device, uint32_t *d_status,
                       uint32_t *sample_status, const std::vector<uint32_t> *blocks, BamPileupScratch &S)
{
    const size_t ns = (size_t)c.n_samples;
    const bool narrow = layout.kind() == CountsKind::Narrow;
    int64_t *d_first5 = nullptr;
    int rc = carve(ctx, ctx->d_bam, 256, [&](Layout &L) {
        S = bam_popmatrix_scratch(L, c.bam_bytes, c.n_samples);
        if (narrow) d_first5 = L.take<int64_t>(1);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, launch_bam_index(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.eof, c.rid, c.beg0, c.end0, c.min_mapq, S, d_status));
    BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, false, c, layout, S, CountsArrays{nullptr, nullptr, nullptr, nullptr}, d_status));
    BVC_HIP_D(ctx, launch_bam_scan(ctx->stream, 0, c.n_samples, S, d_status));
    int64_t head[4] = {0, 0, 0, 0}, first5 = 0x7FFFFFFF;
    BVC_HIP_D(ctx, io.d2h(head, S.head, sizeof head));
    if (narrow) {
        BVC_HIP_D(ctx, launch_first_status(ctx->stream, c.n_samples, d_status, 5u, d_first5));
        BVC_HIP_D(ctx, io.d2h(&first5, d_first5, sizeof first5));
    }
    if (!out_device && ns) BVC_HIP_D(ctx, io.d2h(sample_status, d_status, ns * 4));
    BVC_HIP_D(ctx, wait_stream(ctx));               // the statuses decide whether anything is added
    io.deliver();
    // a block that did not inflate (or failed its CRC32) outranks what the kernels made of its bytes
    if (blocks && block_verdict(ctx, *blocks) != BVC_OK) return BVC_ERR_DATA;
    if ((rc = status_verdict(ctx, head)) != BVC_OK || first5 == 0x7FFFFFFF) return rc;
    char msg[160];
    std::snprintf(msg, sizeof msg, "sample %lld: a base quality of %d or more, and the counts keep n_quals = %d quality columns", (long long)first5,
                  (int)layout.n_quals, (int)layout.n_quals);
    return fail(ctx, BVC_ERR_DATA, msg);
}

// bvc_bam_counts, bvc_bam_counts_depth and bvc_bam_counts_quals behind their own checks (check_counts_call among them): h and a are the
// caller's pointers, device or host memory by flags.
int bam_counts_call(bvc_ctx *ctx, const BamCall &h, const CountsLayout &layout, CountsArrays a, uint32_t *sample_status, uint32_t flags)
{
    if ((h.bam_bytes > 0 && !h.bam) || (h.n_samples > 0 && h.n_positions > 0 && (!a.counts || !a.tally || (layout.depth_groups > 0u && !a.depth))))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)h.n_samples, np = (size_t)h.n_positions;
    BamPileupScratch S;
    PinIO io(ctx);
    int rc;
    if (flags & BVC_PTR_DEVICE) {
        if ((rc = io.reserve(0, 64 + 1024)) != BVC_OK) return rc;
        if ((rc = bam_counts_verdict(ctx, io, h, layout, true, sample_status, sample_status, nullptr, S)) != BVC_OK) return rc;
        BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, true, h, layout, S, a, sample_status));
        return BVC_OK;
    }
    if ((rc = check_host_arrays(ctx, h.n_samples, h.off, h.end, h.bam_bytes, h.n_positions, h.pos)) != BVC_OK) return rc;
    if ((rc = io.reserve(ns * 22 + np * 4 + 1024, 64 + ns * 4 + 1024)) != BVC_OK) return rc;
    // host pointers: the inputs and the accumulators live in the staging buffer for the length of the call
    const size_t cwords = ns ? np * layout.count_words() : 0, trows = ns ? np : 0, dwords = ns ? np * layout.depth_groups * 4 : 0;
    BamStage st(h, nullptr, 0, nullptr, 0, layout.label_groups() > 0u ? a.group_of_sample : nullptr);
    CountsArrays d{nullptr, nullptr, nullptr, nullptr};
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        st.take(L);
        d.counts = L.take<uint32_t>(cwords); d.tally = L.take<bvc_bam_site_tally>(trows); d.depth = L.take<uint32_t>(dwords);
    });
    if (rc != BVC_OK || (rc = st.upload(ctx, io)) != BVC_OK) return rc;
    d.group_of_sample = st.d_group;
    rc = bam_counts_verdict(ctx, io, st.c, layout, false, st.d_status, sample_status, nullptr, S);
    if (rc != BVC_OK || cwords == 0) return rc;
    // the accumulators go up only now: a call that fails has not touched them
    BVC_HIP_D(ctx, hipMemcpyAsync(d.counts, a.counts, cwords * 4, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d.tally, a.tally, trows * sizeof(bvc_bam_site_tally), hipMemcpyHostToDevice, ctx->stream));
    if (dwords) BVC_HIP_D(ctx, hipMemcpyAsync(d.depth, a.depth, dwords * 4, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, true, st.c, layout, S, d, st.d_status));
    BVC_HIP_D(ctx, hipMemcpyAsync(a.counts, d.counts, cwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(a.tally, d.tally, trows * sizeof(bvc_bam_site_tally), hipMemcpyDeviceToHost, ctx->stream));
    if (dwords) BVC_HIP_D(ctx, hipMemcpyAsync(a.depth, d.depth, dwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

// Every kind of accumulator is made here
int site_acc_create(bvc_site_acc **out, int device, int32_t n_positions, const CountsLayout &layout, int64_t byte_budget)
{
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return BVC_ERR_DEVICE; }
    bvc_site_acc *acc = new bvc_site_acc;
    acc->device = device; acc->n_positions = n_positions; acc->layout = layout;
    acc->budget = byte_budget > 0 ? byte_budget : 0;
    const size_t cbytes = (size_t)n_positions * layout.count_words() * 4, tbytes = (size_t)n_positions * sizeof(bvc_bam_site_tally);
    const size_t dbytes = (size_t)n_positions * layout.depth_groups * 16;
    acc->used = (int64_t)((size_t)n_positions * layout.bytes_per_position());
    if (acc->budget > 0 && acc->used > acc->budget) { delete acc; return BVC_ERR_ALLOC; }
    if (n_positions > 0 &&
        (hipMalloc(reinterpret_cast<void **>(&acc->d_counts), cbytes) != hipSuccess || hipMalloc(reinterpret_cast<void **>(&acc->d_tally), tbytes) != hipSuccess ||
         (dbytes && hipMalloc(reinterpret_cast<void **>(&acc->d_depth), dbytes) != hipSuccess) ||
         hipMemset(acc->d_counts, 0, cbytes) != hipSuccess || hipMemset(acc->d_tally, 0, tbytes) != hipSuccess ||
         (dbytes && hipMemset(acc->d_depth, 0, dbytes) != hipSuccess) || hipDeviceSynchronize() != hipSuccess)) {
        (void)hipGetLastError();
        bvc_site_acc_destroy(acc);
        return BVC_ERR_ALLOC;
    }
    *out = acc;
    return BVC_OK;
}

}  // namespace

extern "C" {

int bvc_bam_counts(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                   const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                   const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                   uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *sample_status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    const BamCall h = bam_call(n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    const int rc = check_counts_call(ctx, h, group_of_sample, n_groups, false, sample_status);
    if (rc != BVC_OK) return rc;
    return bam_counts_call(ctx, h, CountsLayout::wide(n_groups), CountsArrays{counts, tally, nullptr, group_of_sample}, sample_status, flags);
}

int bvc_bam_counts_depth(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    const BamCall h = bam_call(n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    const int rc = check_counts_call(ctx, h, group_of_sample, n_groups, true, sample_status);
    if (rc != BVC_OK) return rc;
    return bam_counts_call(ctx, h, CountsLayout::with_depth(n_groups), CountsArrays{counts, tally, group_depth, group_of_sample}, sample_status, flags);
}

int bvc_bam_counts_quals(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups, int32_t n_quals,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (!CountsLayout::quals_ok(n_quals)) return fail(ctx, BVC_ERR_ARG, "n_quals must be a multiple of 4 in 4..128");
    if (n_groups < 0 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 0..32");
    const BamCall h = bam_call(n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    const int rc = check_counts_call(ctx, h, group_of_sample, n_groups, n_groups > 0, sample_status);
    if (rc != BVC_OK) return rc;
    return bam_counts_call(ctx, h, CountsLayout::narrow(n_quals, n_groups), CountsArrays{counts, tally, group_depth, group_of_sample}, sample_status, flags);
}

int bvc_site_acc_create(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 0 || n_groups > BVC_MAX_GROUPS) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, CountsLayout::wide(n_groups), byte_budget);
}

int bvc_site_acc_create_depth(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 1 || n_groups > BVC_MAX_GROUPS) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, CountsLayout::with_depth(n_groups), byte_budget);
}

int bvc_site_acc_create_quals(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int32_t n_quals, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 0 || n_groups > BVC_MAX_GROUPS || !CountsLayout::quals_ok(n_quals)) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, CountsLayout::narrow(n_quals, n_groups), byte_budget);
}

int bvc_site_acc_quals(const bvc_site_acc *acc, int32_t *n_quals)
{
    if (!acc || !n_quals) return BVC_ERR_ARG;
    *n_quals = (int32_t)acc->layout.n_quals;
    return BVC_OK;
}

void bvc_site_acc_destroy(bvc_site_acc *acc)
{
    if (!acc) return;
    (void)hipSetDevice(acc->device);
    if (acc->d_counts) (void)hipFree(acc->d_counts);
    if (acc->d_tally) (void)hipFree(acc->d_tally);
    if (acc->d_depth) (void)hipFree(acc->d_depth);
    delete acc;
}

int bvc_site_acc_bytes(const bvc_site_acc *acc, int64_t *used, int64_t *budget)
{
    if (!acc) return BVC_ERR_ARG;
    if (used) *used = acc->used;
    if (budget) *budget = acc->budget;
    return BVC_OK;
}

int bvc_bam_counts_bgzf_acc(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                            int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                            int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                            int64_t refseq_len, const uint8_t *group_of_sample, bvc_site_acc *acc, uint32_t *sample_status)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if (n_positions != acc->n_positions) return fail(ctx, BVC_ERR_ARG, "n_positions is not the accumulator's");
    const CountsLayout &layout = acc->layout;
    const BamCall h = bam_call(n_samples, nullptr, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    if ((rc = check_counts_call(ctx, h, group_of_sample, (int32_t)layout.label_groups(), layout.depth_groups > 0u, sample_status)) != BVC_OK) return rc;
    if (comp_bytes < 0 || n_blocks < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (n_blocks > 0 && (!comp || !blocks)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if ((rc = check_blocks(ctx, blocks, n_blocks, comp_bytes, bam_bytes)) != BVC_OK) return rc;
    if ((rc = check_host_arrays(ctx, n_samples, sample_off, sample_end, bam_bytes, n_positions, positions)) != BVC_OK) return rc;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_samples, np = (size_t)n_positions, nb = (size_t)n_blocks;
    PinIO io(ctx);
    if ((rc = io.reserve(ns * 22 + np * 4 + nb * sizeof(bvc_bgzf_block) + 1024, 64 + ns * 4 + nb * 4 + 1024)) != BVC_OK) return rc;
    BamStage st(h, comp, comp_bytes, blocks, n_blocks, layout.label_groups() > 0u ? group_of_sample : nullptr);
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { st.take(L); });
    if (rc != BVC_OK || (rc = st.upload(ctx, io)) != BVC_OK) return rc;
    BamPileupScratch S;
    if ((rc = bam_counts_verdict(ctx, io, st.c, layout, false, st.d_status, sample_status, &st.block_status, S)) != BVC_OK) return rc;
    BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, true, st.c, layout, S, CountsArrays{acc->d_counts, acc->d_tally, acc->d_depth, st.d_group}, st.d_status));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_get(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, uint32_t *counts, bvc_bam_site_tally *tally)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    if (n > 0 && !tally) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rw = acc->layout.count_words();
    if (counts && acc->layout.expanded()) {
        // narrow rows: a bounded piece at a time is expanded into the context's scratch and comes down from there
        const int32_t piece = n < kExpandRows ? n : kExpandRows;
        uint32_t *d_wide;
        if ((rc = carve(ctx, ctx->d_acc, 256, [&](Layout &L) { d_wide = L.take<uint32_t>((size_t)piece * BVC_NCLASS); })) != BVC_OK) return rc;
        for (int32_t k = 0; k < n; k += piece) {
            const int32_t m = n - k < piece ? n - k : piece;
            BVC_HIP_D(ctx, launch_acc_expand(ctx->stream, m, (int32_t)acc->layout.n_quals, acc->d_counts + ((size_t)t0 + (size_t)k) * rw, d_wide));
            BVC_HIP_D(ctx, hipMemcpyAsync(counts + (size_t)k * BVC_NCLASS, d_wide, (size_t)m * BVC_NCLASS * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
    } else if (counts)
        BVC_HIP_D(ctx, hipMemcpyAsync(counts, acc->d_counts + (size_t)t0 * rw, (size_t)n * rw * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(tally, acc->d_tally + t0, (size_t)n * sizeof(bvc_bam_site_tally), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_row_words(const bvc_site_acc *acc, int32_t *row_words, int32_t *slots, int32_t *depth_groups)
{
    if (!acc) return BVC_ERR_ARG;
    if (row_words) *row_words = (int32_t)acc->layout.logical_words();
    if (slots) *slots = (int32_t)acc->layout.slots;
    if (depth_groups) *depth_groups = (int32_t)acc->layout.depth_groups;
    return BVC_OK;
}

int bvc_site_acc_pack(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, int64_t *row_start, uint16_t *cell, uint32_t *count,
                      int64_t entries_cap, int64_t *n_entries, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    if (!row_start || !n_entries) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (entries_cap < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & BVC_PTR_DEVICE) != 0;
    const size_t nr = (size_t)n;
    if (n == 0) {
        *n_entries = 0;
        if (!dev) { row_start[0] = 0; return BVC_OK; }
        BVC_HIP_D(ctx, hipMemsetAsync(row_start, 0, 8, ctx->stream));
        return BVC_OK;
    }
    // size pass -> scan -> the one wait, for the total (in the host form row_start comes down with it)
    uint32_t *d_row_n; int64_t *d_row_start = row_start;
    rc = carve(ctx, ctx->d_acc, 256, [&](Layout &L) {
        d_row_n = L.take<uint32_t>(nr);
        if (!dev) d_row_start = L.take<int64_t>(nr + 1);
    });
    if (rc != BVC_OK) return rc;
    const AccRowShape s = acc->layout.row_shape(t0);
    PinIO io(ctx);
    if ((rc = io.reserve(0, 64 + 1024)) != BVC_OK) return rc;
    BVC_HIP_D(ctx, launch_acc_pack(ctx->stream, false, n, s, acc->d_counts, acc->d_tally, acc->d_depth, d_row_n, nullptr, nullptr, nullptr));
    BVC_HIP_D(ctx, launch_acc_pack_scan(ctx->stream, n, d_row_n, d_row_start));
    int64_t total = 0;
    BVC_HIP_D(ctx, io.d2h(&total, d_row_start + nr, 8));
    if (!dev) BVC_HIP_D(ctx, hipMemcpyAsync(row_start, d_row_start, (nr + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    *n_entries = total;
    if (total > entries_cap) return BVC_ACC_MORE;
    if (total == 0) return BVC_OK;
    if (!cell || !count) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (dev) {
        BVC_HIP_D(ctx, launch_acc_pack(ctx->stream, true, n, s, acc->d_counts, acc->d_tally, acc->d_depth, nullptr, d_row_start, cell, count));
        return BVC_OK;
    }
    // host pointers: the entries are placed in the staging buffer and come down from there (d_row_start stays where it is, in d_acc)
    uint16_t *d_cell; uint32_t *d_count;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { d_cell = L.take<uint16_t>((size_t)total); d_count = L.take<uint32_t>((size_t)total); });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, launch_acc_pack(ctx->stream, true, n, s, acc->d_counts, acc->d_tally, acc->d_depth, nullptr, d_row_start, d_cell, d_count));
    BVC_HIP_D(ctx, hipMemcpyAsync(cell, d_cell, (size_t)total * 2, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(count, d_count, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_add_packed(bvc_ctx *ctx, bvc_site_acc *acc, int32_t t0, int32_t n, const int64_t *row_start, const uint16_t *cell,
                            const uint32_t *count, int64_t n_entries, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    if (n_entries < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (!row_start || (n_entries > 0 && (!cell || !count))) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return n_entries == 0 ? BVC_OK : fail(ctx, BVC_ERR_DATA, "row 0: row_start does not end at n_entries (no rows, yet entries)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & BVC_PTR_DEVICE) != 0;
    const size_t nr = (size_t)n, ne = (size_t)n_entries;
    uint32_t *d_fault; int64_t *d_first;
    if ((rc = carve(ctx, ctx->d_acc, 256, [&](Layout &L) { d_fault = L.take<uint32_t>(nr); d_first = L.take<int64_t>(2); })) != BVC_OK) return rc;
    const int64_t *d_row_start = row_start; const uint16_t *d_cell = cell; const uint32_t *d_count = count;
    if (!dev) {
        // host pointers: the piece lives in the staging buffer for the length of the call
        int64_t *u_rs; uint16_t *u_cell; uint32_t *u_count;
        rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { u_rs = L.take<int64_t>(nr + 1); u_cell = L.take<uint16_t>(ne); u_count = L.take<uint32_t>(ne); });
        if (rc != BVC_OK) return rc;
        BVC_HIP_D(ctx, hipMemcpyAsync(u_rs, row_start, (nr + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (ne) {
            BVC_HIP_D(ctx, hipMemcpyAsync(u_cell, cell, ne * 2, hipMemcpyHostToDevice, ctx->stream));
            BVC_HIP_D(ctx, hipMemcpyAsync(u_count, count, ne * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        d_row_start = u_rs; d_cell = u_cell; d_count = u_count;
    }
    const AccRowShape s = acc->layout.row_shape(t0);
    const int nq = (int)acc->layout.n_quals, row_words = (int)acc->layout.logical_words();
    PinIO io(ctx);
    if ((rc = io.reserve(0, 64 + 1024)) != BVC_OK) return rc;
    // dry pass -> first fault -> the one wait, for the verdict: nothing is added unless the whole piece is sound
    BVC_HIP_D(ctx, launch_acc_add_packed(ctx->stream, false, n, s, d_row_start, d_cell, d_count, n_entries, nullptr, nullptr, acc->d_depth, d_fault));
    BVC_HIP_D(ctx, launch_acc_first_fault(ctx->stream, n, d_fault, d_first));
    int64_t first[2] = {0, 0};
    BVC_HIP_D(ctx, io.d2h(first, d_first, sizeof first));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    if (first[1] != 0) {
        char msg[200];
        const long long t = (long long)first[0];
        switch ((uint32_t)first[1]) {
        case kAccFaultRowStart:
            std::snprintf(msg, sizeof msg, "row %lld: row_start must start at 0, never decrease and end at n_entries = %lld", t, (long long)n_entries);
            break;
        case kAccFaultCell:
            std::snprintf(msg, sizeof msg, "row %lld: a cell of %d or more, and the accumulator's row has %d words", t, row_words, row_words);
            break;
        case kAccFaultOrder: std::snprintf(msg, sizeof msg, "row %lld: the cells of a row must ascend strictly", t); break;
        default:
            std::snprintf(msg, sizeof msg, "row %lld: a count of a base quality of %d or more, and the counts keep n_quals = %d quality columns", t, nq, nq);
        }
        return fail(ctx, BVC_ERR_DATA, msg);
    }
    BVC_HIP_D(ctx, launch_acc_add_packed(ctx->stream, true, n, s, d_row_start, d_cell, d_count, n_entries, acc->d_counts, acc->d_tally, acc->d_depth,
                                         nullptr));
    if (!dev) BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_get_depth(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, uint32_t *group_depth)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if (acc->layout.depth_groups == 0u) return fail(ctx, BVC_ERR_ARG, "the accumulator keeps no group depths (bvc_site_acc_create_depth makes one that does)");
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    if (n > 0 && !group_depth) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rw = (size_t)acc->layout.depth_groups * 4;
    BVC_HIP_D(ctx, hipMemcpyAsync(group_depth, acc->d_depth + (size_t)t0 * rw, (size_t)n * rw * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_lrt(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, const int8_t *ref_base, double min_af,
                     bvc_site_result *results, bvc_group_result *grp_results)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    const int32_t ng = (int32_t)acc->layout.slots - 1;         // the groups that have a slot of their own
    if (n > 0 && (!ref_base || !results || (ng > 0 && !grp_results))) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    // the rows stay where they are: only ref_base goes up and the records come down, through the staging buffer
    int8_t *d_r; bvc_site_result *d_res; bvc_group_result *d_gres; uint32_t *d_wide;
    const int32_t piece = !acc->layout.expanded() ? 0 : n < kExpandRows ? n : kExpandRows;      // narrow rows: expanded a piece at a time
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_r = L.take<int8_t>((size_t)n);
        d_res = L.take<bvc_site_result>((size_t)n);
        d_gres = L.take<bvc_group_result>((size_t)n * (size_t)ng);
        d_wide = L.take<uint32_t>((size_t)piece * BVC_NCLASS);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    const size_t rw = acc->layout.count_words();
    const uint32_t *rows = acc->d_counts + (size_t)t0 * rw;
    if (piece > 0) {
        // (the stream orders a piece's stage 2 in front of the next piece's expansion into the same scratch)
        for (int32_t k = 0; k < n && rc == BVC_OK; k += piece) {
            const int32_t m = n - k < piece ? n - k : piece;
            BVC_HIP_D(ctx, launch_acc_expand(ctx->stream, m, (int32_t)acc->layout.n_quals, rows + (size_t)k * rw, d_wide));
            rc = bvc_lrt_hist(ctx, m, d_wide, d_r + k, min_af, nullptr, nullptr, d_res + k, BVC_PTR_DEVICE);
        }
    } else if (ng > 0) {
        rc = bvc_lrt_hist_groups(ctx, n, rows, d_r, min_af, ng, d_res, d_gres, BVC_PTR_DEVICE);
        if (rc == BVC_OK) rc = join_side(ctx);
    } else
        rc = bvc_lrt_hist(ctx, n, rows, d_r, min_af, nullptr, nullptr, d_res, BVC_PTR_DEVICE);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    if (ng > 0) BVC_HIP_D(ctx, hipMemcpyAsync(grp_results, d_gres, (size_t)n * (size_t)ng * sizeof(bvc_group_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

}  // extern "C"
