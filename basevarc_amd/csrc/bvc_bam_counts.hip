// bvc_bam_counts.hip -- bvc_bam_counts, bvc_bam_counts_bgzf_acc and the accumulator bvc_site_acc (include/bvc_bam_counts.h): the inflated BAM
// records of a batch of samples added into per-position class counts and tallies (bam_counts_kernel.hip).  The call's inputs (BamCall), their
// checks and the verdicts on the statuses and the blocks are bvc_bam.hip's.  Order of work: index -> dry pass -> scan -> first wait ->
// verdict -> add pass (-> second wait in the host forms): nothing is added unless the call returns BVC_OK.  The ninth header's calls
// (include/bvc_bam_group_depth.h: bvc_bam_counts_depth, the accumulator's second kind) live here too: they are the same calls with one slot
// of counts, the groups' depths beside it and bam_group_depth_kernel.hip as their add pass.  And the tenth header's
// (include/bvc_site_acc_quals.h: bvc_bam_counts_quals, the accumulator's third kind): the same calls again with narrow rows of counts
// [position][4][n_quals], bam_counts_quals_kernel.hip as both passes, one more verdict (status 5) behind the existing one, and
// acc_expand_kernel between narrow rows and the callers of bvc_site_acc_get / bvc_site_acc_lrt.  And the eleventh header's
// (include/bvc_site_acc_pack.h: bvc_site_acc_pack and bvc_site_acc_add_packed, beside bvc_site_acc_get): an accumulator's rows as the
// entries of their non-zero words and back, acc_pack_kernel.hip -- size pass -> scan -> the wait for the total -> place pass, and dry pass
// -> first fault -> the wait for the verdict -> add pass.
#include "bvc_ctx.h"
#include "../../include/bvc_site_acc_pack.h"

// An accumulator is no part of a context: its device memory is its own, and its bookkeeping is fixed when it is made (the adds are atomic).
struct bvc_site_acc {
    int device = -1;
    int32_t n_positions = 0, n_groups = 0;
    int64_t budget = 0, used = 0;
    int32_t depth_groups = 0;                        // the second kind (bvc_site_acc_create_depth): n_groups stays 0, one slot
    uint32_t *d_counts = nullptr;                    // [n_positions][slots][512]
    bvc_bam_site_tally *d_tally = nullptr;           // [n_positions]
    uint32_t *d_depth = nullptr;                     // [n_positions][depth_groups][4], the second and third kind
    int32_t n_quals = 0;                             // > 0: the third kind (bvc_site_acc_create_quals) -- n_groups stays 0, one slot of
                                                     // [4][n_quals] words, depth_groups 0..32
    size_t slots() const { return n_groups > 0 ? (size_t)n_groups + 1 : 1; }
    size_t row_words() const { return n_quals > 0 ? (size_t)n_quals * 4 : slots() * BVC_NCLASS; }
    bool expanded() const { return n_quals > 0 && n_quals < 128; }   // its rows are not the [512] layout: acc_expand_kernel makes it
    size_t logical_words() const { return slots() * BVC_NCLASS + 10 + (size_t)depth_groups * 4; }   // W of bvc_site_acc_pack.h
    // rows from t0 on as acc_pack_kernel.hip's kernels see them (128 columns are stored as the wide layout stores them)
    AccRowShape shape(int32_t t0) const
    {
        return AccRowShape{(int64_t)t0, (uint32_t)(row_words() / 4), expanded() ? (uint32_t)n_quals / 4u : 0u, (uint32_t)(slots() * BVC_NCLASS),
                           (uint32_t)depth_groups};
    }
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

int check_counts_groups(bvc_ctx *ctx, int32_t n_samples, const uint8_t *group_of_sample, int32_t n_groups)
{
    if (n_groups < 0 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 0..32");
    if (n_groups > 0 && n_samples > 0 && !group_of_sample) return fail(ctx, BVC_ERR_ARG, "null group_of_sample with n_groups > 0");
    return BVC_OK;
}

// Index, dry pass, scan and the call's first wait, on inputs in device memory: the statuses (to sample_status on the host unless
// out_device) and the verdict -- the blocks' first (blocks: their statuses come down with the same wait; may be null), then the samples'.
// n_quals > 0: the narrow forms -- their dry pass also raises status 5, whose first sample comes down with the same wait and is judged
// behind the existing verdict.
int bam_counts_verdict(bvc_ctx *ctx, PinIO &io, const BamCall &c, bool out_device, uint32_t *d_status, uint32_t *sample_status,
                       const std::vector<uint32_t> *blocks, BamPileupScratch &S, int32_t n_quals = 0)
{
    const size_t ns = (size_t)c.n_samples;
    int64_t *d_first5 = nullptr;
    int rc = carve(ctx, ctx->d_bam, 256, [&](Layout &L) {
        S = bam_popmatrix_scratch(L, c.bam_bytes, c.n_samples);
        if (n_quals > 0) d_first5 = L.take<int64_t>(1);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, launch_bam_index(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.eof, c.rid, c.beg0, c.end0, c.min_mapq, S, d_status));
    if (n_quals > 0)
        BVC_HIP_D(ctx, launch_bam_counts_quals(ctx->stream, false, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.rg_s,
                                               c.refseq_len, nullptr, 0, n_quals, S, nullptr, nullptr, nullptr, d_status));
    else
        BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, false, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.rg_s, c.refseq_len,
                                         nullptr, 0, S, nullptr, nullptr, d_status));
    BVC_HIP_D(ctx, launch_bam_scan(ctx->stream, 0, c.n_samples, S, d_status));
    int64_t head[4] = {0, 0, 0, 0}, first5 = 0x7FFFFFFF;
    BVC_HIP_D(ctx, io.d2h(head, S.head, sizeof head));
    if (n_quals > 0) {
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
                  (int)n_quals, (int)n_quals);
    return fail(ctx, BVC_ERR_DATA, msg);
}

// The add pass, enqueued on the context's stream.  d_depth: the depth form's array (one slot of counts, n_groups depth rows), else null.
// n_quals > 0: the narrow forms (d_counts [P][4][n_quals]; d_depth null with n_groups 0).
int bam_counts_add(bvc_ctx *ctx, const BamCall &c, const uint8_t *d_group, int32_t n_groups, const BamPileupScratch &S, uint32_t *d_counts,
                   bvc_bam_site_tally *d_tally, uint32_t *d_depth, uint32_t *d_status, int32_t n_quals = 0)
{
    if (n_quals > 0)
        BVC_HIP_D(ctx, launch_bam_counts_quals(ctx->stream, true, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.rg_s,
                                               c.refseq_len, d_group, n_groups, n_quals, S, d_counts, d_tally, d_depth, d_status));
    else if (d_depth)
        BVC_HIP_D(ctx, launch_bam_counts_depth(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.rg_s, c.refseq_len,
                                               d_group, n_groups, S, d_counts, d_tally, d_depth));
    else
        BVC_HIP_D(ctx, launch_bam_counts(ctx->stream, true, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.rg_s, c.refseq_len,
                                         d_group, n_groups, S, d_counts, d_tally, d_status));
    return BVC_OK;
}

// The depth forms' own check of the labels: there is no form without groups
int check_depth_groups(bvc_ctx *ctx, int32_t n_samples, const uint8_t *group_of_sample, int32_t n_groups)
{
    if (n_groups < 1 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
    if (n_samples > 0 && !group_of_sample) return fail(ctx, BVC_ERR_ARG, "null group_of_sample with samples present");
    return BVC_OK;
}

// What both entry points check of the sample and position arguments before anything of the device is touched; fills what they share.
int check_counts_call(bvc_ctx *ctx, BamCall &c, int32_t n_samples, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                      const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                      const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                      const uint32_t *sample_status)
{
    int rc = check_sizes(ctx, n_samples, bam_bytes, n_positions, refseq_len, 0);
    if (rc != BVC_OK) return rc;
    if ((rc = check_counts_groups(ctx, n_samples, group_of_sample, n_groups)) != BVC_OK) return rc;
    if ((n_samples > 0 && (!sample_off || !sample_end || !sample_eof || !rid || !sample_status)) || (n_positions > 0 && !positions))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    c.n_samples = n_samples; c.n_positions = n_positions; c.beg0 = beg0; c.end0 = end0; c.min_mapq = min_mapq; c.rg_s = rg_s;
    c.eof = sample_eof; c.off = sample_off; c.end = sample_end; c.rid = rid; c.pos = positions; c.bam_bytes = bam_bytes; c.refseq_len = refseq_len;
    return BVC_OK;
}

// bvc_bam_counts (depth = false: counts [P][slots][512], group_depth unused) and bvc_bam_counts_depth (depth = true: counts [P][512] and
// group_depth [P][n_groups][4]) are one call; so is bvc_bam_counts_quals (n_quals > 0: counts [P][4][n_quals]; depth says whether it has
// groups, n_groups 0 is allowed).
int bam_counts_call(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                    const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                    const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups, bool depth,
                    uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags, int32_t n_quals = 0)
{
    if (!ctx) return BVC_ERR_ARG;
    BamCall c;
    int rc = check_counts_call(ctx, c, n_samples, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s,
                               refseq_len, group_of_sample, depth ? 0 : n_groups, sample_status);
    if (rc != BVC_OK) return rc;
    if (depth && (rc = check_depth_groups(ctx, n_samples, group_of_sample, n_groups)) != BVC_OK) return rc;
    if ((bam_bytes > 0 && !bam) || (n_samples > 0 && n_positions > 0 && (!counts || !tally || (depth && !group_depth))))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    c.bam = bam;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_samples, np = (size_t)n_positions;
    const bool labels = n_groups > 0 && ns > 0;
    BamPileupScratch S;
    PinIO io(ctx);
    if (flags & BVC_PTR_DEVICE) {
        if ((rc = io.reserve(0, 64 + 1024)) != BVC_OK) return rc;
        rc = bam_counts_verdict(ctx, io, c, true, sample_status, sample_status, nullptr, S, n_quals);
        return rc != BVC_OK ? rc : bam_counts_add(ctx, c, group_of_sample, n_groups, S, counts, tally, depth ? group_depth : nullptr, sample_status, n_quals);
    }
    if ((rc = check_host_arrays(ctx, n_samples, sample_off, sample_end, bam_bytes, n_positions, positions)) != BVC_OK) return rc;
    if ((rc = io.reserve(ns * 22 + np * 4 + 1024, 64 + ns * 4 + 1024)) != BVC_OK) return rc;
    // host pointers: the inputs and the accumulators live in the staging buffer for the length of the call
    const size_t row = n_quals > 0 ? (size_t)n_quals * 4 : (n_groups > 0 && !depth ? (size_t)n_groups + 1 : 1) * BVC_NCLASS;
    const size_t cwords = ns ? np * row : 0, trows = ns ? np : 0;
    const size_t dwords = depth && ns ? np * (size_t)n_groups * 4 : 0;
    uint8_t *u_bam, *u_eof, *u_grp; int64_t *u_off, *u_end; int32_t *u_rid, *u_pos; uint32_t *d_status, *d_counts, *d_depth; bvc_bam_site_tally *d_tally;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        u_bam = L.take<uint8_t>((size_t)bam_bytes);
        u_off = L.take<int64_t>(ns); u_end = L.take<int64_t>(ns); u_eof = L.take<uint8_t>(ns); u_rid = L.take<int32_t>(ns); u_grp = L.take<uint8_t>(ns);
        u_pos = L.take<int32_t>(np); d_status = L.take<uint32_t>(ns);
        d_counts = L.take<uint32_t>(cwords); d_tally = L.take<bvc_bam_site_tally>(trows); d_depth = L.take<uint32_t>(dwords);
    });
    if (rc != BVC_OK) return rc;
    if (bam_bytes) BVC_HIP_D(ctx, hipMemcpyAsync(u_bam, bam, (size_t)bam_bytes, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, io.h2d(u_off, sample_off, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_end, sample_end, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_eof, sample_eof, ns));
    BVC_HIP_D(ctx, io.h2d(u_rid, rid, ns * 4));
    if (labels) BVC_HIP_D(ctx, io.h2d(u_grp, group_of_sample, ns));
    BVC_HIP_D(ctx, io.h2d(u_pos, positions, np * 4));
    c.bam = u_bam; c.off = u_off; c.end = u_end; c.eof = u_eof; c.rid = u_rid; c.pos = u_pos;
    rc = bam_counts_verdict(ctx, io, c, false, d_status, sample_status, nullptr, S, n_quals);
    if (rc != BVC_OK || cwords == 0) return rc;
    // the accumulators go up only now: a call that fails has not touched them
    BVC_HIP_D(ctx, hipMemcpyAsync(d_counts, counts, cwords * 4, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_tally, tally, trows * sizeof(bvc_bam_site_tally), hipMemcpyHostToDevice, ctx->stream));
    if (dwords) BVC_HIP_D(ctx, hipMemcpyAsync(d_depth, group_depth, dwords * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = bam_counts_add(ctx, c, u_grp, n_groups, S, d_counts, d_tally, depth ? d_depth : nullptr, d_status, n_quals)) != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(counts, d_counts, cwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(tally, d_tally, trows * sizeof(bvc_bam_site_tally), hipMemcpyDeviceToHost, ctx->stream));
    if (dwords) BVC_HIP_D(ctx, hipMemcpyAsync(group_depth, d_depth, dwords * 4, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

// Every kind of accumulator is made here: depth_groups > 0 is the second kind (n_groups is then 0), n_quals > 0 the third (n_groups 0,
// depth_groups 0..32)
int site_acc_create(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int32_t depth_groups, int64_t byte_budget, int32_t n_quals = 0)
{
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return BVC_ERR_DEVICE; }
    bvc_site_acc *acc = new bvc_site_acc;
    acc->device = device; acc->n_positions = n_positions; acc->n_groups = n_groups; acc->depth_groups = depth_groups; acc->n_quals = n_quals;
    acc->budget = byte_budget > 0 ? byte_budget : 0;
    const size_t cbytes = (size_t)n_positions * acc->row_words() * 4, tbytes = (size_t)n_positions * sizeof(bvc_bam_site_tally);
    const size_t dbytes = (size_t)n_positions * (size_t)depth_groups * 16;
    acc->used = (int64_t)(cbytes + tbytes + dbytes);
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
    return bam_counts_call(ctx, n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s,
                           refseq_len, group_of_sample, n_groups, false, counts, tally, nullptr, sample_status, flags);
}

int bvc_bam_counts_depth(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags)
{
    return bam_counts_call(ctx, n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s,
                           refseq_len, group_of_sample, n_groups, true, counts, tally, group_depth, sample_status, flags);
}

int bvc_bam_counts_quals(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                         const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                         const int32_t *positions, int32_t rg_s, int64_t refseq_len, const uint8_t *group_of_sample, int32_t n_groups, int32_t n_quals,
                         uint32_t *counts, bvc_bam_site_tally *tally, uint32_t *group_depth, uint32_t *sample_status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (!quals_ok(n_quals)) return fail(ctx, BVC_ERR_ARG, "n_quals must be a multiple of 4 in 4..128");
    if (n_groups < 0 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 0..32");
    return bam_counts_call(ctx, n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s,
                           refseq_len, n_groups > 0 ? group_of_sample : nullptr, n_groups, n_groups > 0, counts, tally, group_depth, sample_status, flags,
                           n_quals);
}

int bvc_site_acc_create(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 0 || n_groups > BVC_MAX_GROUPS) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, n_groups, 0, byte_budget);
}

int bvc_site_acc_create_depth(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 1 || n_groups > BVC_MAX_GROUPS) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, 0, n_groups, byte_budget);
}

int bvc_site_acc_create_quals(bvc_site_acc **out, int device, int32_t n_positions, int32_t n_groups, int32_t n_quals, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_groups < 0 || n_groups > BVC_MAX_GROUPS || !quals_ok(n_quals)) return BVC_ERR_ARG;
    return site_acc_create(out, device, n_positions, 0, n_groups, byte_budget, n_quals);
}

int bvc_site_acc_quals(const bvc_site_acc *acc, int32_t *n_quals)
{
    if (!acc || !n_quals) return BVC_ERR_ARG;
    *n_quals = acc->n_quals > 0 ? acc->n_quals : 128;
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
    BamCall c;
    rc = check_counts_call(ctx, c, n_samples, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s,
                           refseq_len, group_of_sample, acc->n_groups, sample_status);
    if (rc != BVC_OK) return rc;
    const int32_t dg = acc->depth_groups;                               // (> 0: the second kind, whose n_groups is 0)
    if (dg > 0 && (rc = check_depth_groups(ctx, n_samples, group_of_sample, dg)) != BVC_OK) return rc;
    if (comp_bytes < 0 || n_blocks < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (n_blocks > 0 && (!comp || !blocks)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if ((rc = check_blocks(ctx, blocks, n_blocks, comp_bytes, bam_bytes)) != BVC_OK) return rc;
    if ((rc = check_host_arrays(ctx, n_samples, sample_off, sample_end, bam_bytes, n_positions, positions)) != BVC_OK) return rc;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_samples, np = (size_t)n_positions, nb = (size_t)n_blocks;
    const bool labels = (acc->n_groups > 0 || dg > 0) && ns > 0;
    PinIO io(ctx);
    if ((rc = io.reserve(ns * 22 + np * 4 + nb * sizeof(bvc_bgzf_block) + 1024, 64 + ns * 4 + nb * 4 + 1024)) != BVC_OK) return rc;
    uint8_t *u_comp, *u_bam, *u_eof, *u_grp; bvc_bgzf_block *u_blk; uint32_t *u_bst, *d_status; int64_t *u_off, *u_end; int32_t *u_rid, *u_pos;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        u_comp = L.take<uint8_t>((size_t)comp_bytes, 16); u_blk = L.take<bvc_bgzf_block>(nb); u_bst = L.take<uint32_t>(nb);
        u_bam = L.take<uint8_t>((size_t)bam_bytes);
        u_off = L.take<int64_t>(ns); u_end = L.take<int64_t>(ns); u_eof = L.take<uint8_t>(ns); u_rid = L.take<int32_t>(ns); u_grp = L.take<uint8_t>(ns);
        u_pos = L.take<int32_t>(np); d_status = L.take<uint32_t>(ns);
    });
    if (rc != BVC_OK) return rc;
    std::vector<uint32_t> block_status(nb);
    if (nb) {
        BVC_HIP_D(ctx, hipMemcpyAsync(u_comp, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, io.h2d(u_blk, blocks, nb * sizeof(bvc_bgzf_block)));
        BVC_HIP_D(ctx, launch_inflate(ctx->stream, u_comp, u_blk, n_blocks, u_bam, u_bst));
        BVC_HIP_D(ctx, io.d2h(block_status.data(), u_bst, nb * 4));
    }
    BVC_HIP_D(ctx, io.h2d(u_off, sample_off, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_end, sample_end, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_eof, sample_eof, ns));
    BVC_HIP_D(ctx, io.h2d(u_rid, rid, ns * 4));
    if (labels) BVC_HIP_D(ctx, io.h2d(u_grp, group_of_sample, ns));
    BVC_HIP_D(ctx, io.h2d(u_pos, positions, np * 4));
    c.bam = u_bam; c.off = u_off; c.end = u_end; c.eof = u_eof; c.rid = u_rid; c.pos = u_pos;
    BamPileupScratch S;
    rc = bam_counts_verdict(ctx, io, c, false, d_status, sample_status, &block_status, S, acc->n_quals);
    if (rc != BVC_OK) return rc;
    if ((rc = bam_counts_add(ctx, c, u_grp, dg > 0 ? dg : acc->n_groups, S, acc->d_counts, acc->d_tally, dg > 0 ? acc->d_depth : nullptr, d_status,
                             acc->n_quals)) != BVC_OK)
        return rc;
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
    const size_t rw = acc->row_words();
    if (counts && acc->expanded()) {
        // narrow rows: a bounded piece at a time is expanded into the context's scratch and comes down from there
        const int32_t piece = n < kExpandRows ? n : kExpandRows;
        uint32_t *d_wide;
        if ((rc = carve(ctx, ctx->d_acc, 256, [&](Layout &L) { d_wide = L.take<uint32_t>((size_t)piece * BVC_NCLASS); })) != BVC_OK) return rc;
        for (int32_t k = 0; k < n; k += piece) {
            const int32_t m = n - k < piece ? n - k : piece;
            BVC_HIP_D(ctx, launch_acc_expand(ctx->stream, m, acc->n_quals, acc->d_counts + ((size_t)t0 + (size_t)k) * rw, d_wide));
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
    if (row_words) *row_words = (int32_t)acc->logical_words();
    if (slots) *slots = (int32_t)acc->slots();
    if (depth_groups) *depth_groups = acc->depth_groups;
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
    const AccRowShape s = acc->shape(t0);
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
    const AccRowShape s = acc->shape(t0);
    const int32_t nq = acc->expanded() ? acc->n_quals : 128;
    PinIO io(ctx);
    if ((rc = io.reserve(0, 64 + 1024)) != BVC_OK) return rc;
    // dry pass -> first fault -> the one wait, for the verdict: nothing is added unless the whole piece is sound
    BVC_HIP_D(ctx, launch_acc_add_packed(ctx->stream, false, n, s, nq, d_row_start, d_cell, d_count, n_entries, nullptr, nullptr, acc->d_depth, d_fault));
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
            std::snprintf(msg, sizeof msg, "row %lld: a cell of %d or more, and the accumulator's row has %d words", t, (int)acc->logical_words(),
                          (int)acc->logical_words());
            break;
        case kAccFaultOrder: std::snprintf(msg, sizeof msg, "row %lld: the cells of a row must ascend strictly", t); break;
        default:
            std::snprintf(msg, sizeof msg, "row %lld: a count of a base quality of %d or more, and the counts keep n_quals = %d quality columns", t, (int)nq,
                          (int)nq);
        }
        return fail(ctx, BVC_ERR_DATA, msg);
    }
    BVC_HIP_D(ctx, launch_acc_add_packed(ctx->stream, true, n, s, nq, d_row_start, d_cell, d_count, n_entries, acc->d_counts, acc->d_tally, acc->d_depth,
                                         nullptr));
    if (!dev) BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_site_acc_get_depth(bvc_ctx *ctx, const bvc_site_acc *acc, int32_t t0, int32_t n, uint32_t *group_depth)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_acc(ctx, acc);
    if (rc != BVC_OK) return rc;
    if (acc->depth_groups <= 0) return fail(ctx, BVC_ERR_ARG, "the accumulator keeps no group depths (bvc_site_acc_create_depth makes one that does)");
    if ((rc = check_rows(ctx, acc, t0, n)) != BVC_OK) return rc;
    if (n > 0 && !group_depth) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rw = (size_t)acc->depth_groups * 4;
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
    const int32_t ng = acc->n_groups;
    if (n > 0 && (!ref_base || !results || (ng > 0 && !grp_results))) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    // the rows stay where they are: only ref_base goes up and the records come down, through the staging buffer
    int8_t *d_r; bvc_site_result *d_res; bvc_group_result *d_gres; uint32_t *d_wide;
    const int32_t piece = !acc->expanded() ? 0 : n < kExpandRows ? n : kExpandRows;      // narrow rows: expanded a piece at a time
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_r = L.take<int8_t>((size_t)n);
        d_res = L.take<bvc_site_result>((size_t)n);
        d_gres = L.take<bvc_group_result>((size_t)n * (size_t)ng);
        d_wide = L.take<uint32_t>((size_t)piece * BVC_NCLASS);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t *rows = acc->d_counts + (size_t)t0 * acc->row_words();
    if (piece > 0) {
        // (the stream orders a piece's stage 2 in front of the next piece's expansion into the same scratch)
        for (int32_t k = 0; k < n && rc == BVC_OK; k += piece) {
            const int32_t m = n - k < piece ? n - k : piece;
            BVC_HIP_D(ctx, launch_acc_expand(ctx->stream, m, acc->n_quals, rows + (size_t)k * acc->row_words(), d_wide));
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
