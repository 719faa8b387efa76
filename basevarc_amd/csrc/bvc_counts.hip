// bvc_counts.hip -- class counts accumulated over chunks of a cohort's samples: stage 1 that ADDS into the caller's counts (dense tiles of a
// chunk's columns, ragged columns of a chunk's samples, plain and with groups) and the merge of two partial counts.  Stage 2 of the result is
// bvc_lrt_hist / bvc_lrt_hist_groups (bvc_lrt.hip).  Everything here runs on the context's stream, in overlap mode too.
#include "bvc_ctx.h"

namespace {

// A dense chunk: `stage1(scratch)` runs an existing histogram launcher, unchanged, into the context's scratch (`words` counters; zeroed first
// where the launcher adds with atomics), counts_add_kernel then adds the scratch to the caller's counts.
template <class Stage1>
int add_through_scratch(bvc_ctx *ctx, size_t words, bool zero, uint32_t *counts, Stage1 stage1)
{
    const int rc = ensure(ctx, ctx->d_acc, words * sizeof(uint32_t));
    if (rc != BVC_OK) return rc;
    uint32_t *scratch = reinterpret_cast<uint32_t *>(ctx->d_acc.p);
    if (zero) BVC_HIP(ctx, hipMemsetAsync(scratch, 0, words * sizeof(uint32_t), ctx->stream));
    BVC_HIP(ctx, stage1(scratch));
    BVC_HIP(ctx, launch_counts_add(ctx->stream, (int64_t)words, counts, scratch));
    return BVC_OK;
}

// quals == nullptr: packed rows in `bases`
int add_dense_device(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases, const int8_t *quals,
                     uint32_t *counts)
{
    if (n_samples == 0) return BVC_OK;
    const int split = choose_hist_split(ctx->ls, n_sites, n_samples);
    return add_through_scratch(ctx, (size_t)n_sites * BVC_NCLASS, split > 1, counts, [&](uint32_t *scratch) {
        if (!quals) return launch_hist_packed(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, reinterpret_cast<const uint8_t *>(bases), scratch, split);
        return launch_hist_dense(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, bases, quals, nullptr, 0, scratch, split);
    });
}

int add_dense_groups_device(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases, const int8_t *quals,
                            const uint8_t *group_of_sample, int32_t n_groups, uint32_t *grp_counts)
{
    if (n_samples == 0) return BVC_OK;
    const int rc = ensure_joined(ctx, ctx->d_grp_labels, group_labels_bytes(n_samples, n_sites));
    if (rc != BVC_OK) return rc;
    return add_through_scratch(ctx, (size_t)n_sites * (size_t)(n_groups + 1) * BVC_NCLASS, false, grp_counts, [&](uint32_t *scratch) {
        return launch_hist_dense(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, bases, quals, group_of_sample, n_groups, scratch, 1,
                                 ctx->d_grp_scratch, reinterpret_cast<uint8_t *>(ctx->d_grp_labels.p));
    });
}

// Ragged columns: every site's observations go straight into the caller's counts, by one of two kernels -- the sites of at most
// csr_scatter_max observations in this call by one atomic per observation, the others through a histogram in LDS that its workgroup adds.
// quals == nullptr: packed observations; group_of_obs == nullptr: [site][512], else [site][n_groups + 1][512].
int add_csr_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals, const uint8_t *group_of_obs,
                   int32_t n_groups, uint32_t *counts)
{
    // the key's largest value means "every site": the scatter kernel then takes sites of any length and there is no second launch
    const bool all = ctx->ls.csr_scatter_max >= (1 << 30);
    const int64_t cut = all ? INT64_MAX : ctx->ls.csr_scatter_max;
    BVC_HIP(ctx, launch_hist_csr_scatter(ctx->ls, ctx->stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, cut, counts));
    if (!all) BVC_HIP(ctx, launch_hist_csr_add(ctx->ls, ctx->stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, cut, counts));
    return BVC_OK;
}

// One array of a host-pointer call: the caller's, its bytes, its staged copy.
struct Staged { const void *host; size_t bytes; void *dev; };

// The convenience form of every call here: the input arrays and the caller's counts go up through staging set 0 (in one piece), `device(counts)`
// adds on the device, the counts come back.  Synchronous.
template <class Device>
int add_on_host_pointers(bvc_ctx *ctx, Staged *in, int n_in, uint32_t *counts, size_t words, Device device)
{
    uint32_t *d_c = nullptr;
    int rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        for (int a = 0; a < n_in; ++a) in[a].dev = L.take<char>(in[a].bytes, 16);
        d_c = L.take<uint32_t>(words);
    });
    if (rc != BVC_OK) return rc;
    for (int a = 0; a < n_in; ++a)
        if (in[a].bytes) BVC_HIP_D(ctx, hipMemcpyAsync(in[a].dev, in[a].host, in[a].bytes, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_c, counts, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = device(d_c);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(counts, d_c, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

// bytes of a dense tile that are addressed: the last row may be shorter than row_stride in the caller's allocation
size_t tile_bytes(int64_t n_sites, int64_t n_samples, int64_t row_stride)
{
    return n_samples ? (size_t)(n_sites - 1) * (size_t)row_stride + (size_t)n_samples : 0;
}

// bvc_counts_add_dense (quals given), bvc_counts_add_dense_packed (quals == nullptr) and, with group_of_sample, bvc_counts_add_dense_groups
int counts_add_dense_impl(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases, const int8_t *quals,
                          bool packed, const uint8_t *group_of_sample, int32_t n_groups, bool groups, uint32_t *counts, uint32_t flags)
{
    // rows of zero samples carry no data: their pointers may be null
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? (const void *)bases : (const void *)counts,
                         n_samples && !packed ? (const void *)quals : (const void *)counts, counts, counts);
    if (rc != BVC_OK) return rc;
    if (groups) {
        if ((rc = check_n_groups(ctx, n_groups)) != BVC_OK) return rc;
        if (n_samples > 0 && !group_of_sample) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    }
    if (n_sites == 0 || n_samples == 0) return BVC_OK;
    auto run_device = [&](const int8_t *b, const int8_t *q, const uint8_t *g, uint32_t *c) {
        return groups ? add_dense_groups_device(ctx, n_sites, n_samples, row_stride, b, q, g, n_groups, c)
                      : add_dense_device(ctx, n_sites, n_samples, row_stride, b, packed ? nullptr : q, c);
    };
    if (flags & BVC_PTR_DEVICE) return run_device(bases, quals, group_of_sample, counts);
    const size_t bytes = tile_bytes(n_sites, n_samples, row_stride);
    Staged in[3] = {{bases, bytes, nullptr}, {quals, packed ? 0 : bytes, nullptr}, {group_of_sample, groups ? (size_t)n_samples : 0, nullptr}};
    return add_on_host_pointers(ctx, in, 3, counts, (size_t)n_sites * (size_t)(groups ? n_groups + 1 : 1) * BVC_NCLASS, [&](uint32_t *c) {
        return run_device(static_cast<const int8_t *>(in[0].dev), static_cast<const int8_t *>(in[1].dev), static_cast<const uint8_t *>(in[2].dev), c);
    });
}

// bvc_counts_add_csr (quals given), bvc_counts_add_csr_packed (packed) and, with labels, bvc_counts_add_csr_group_labels
int counts_add_csr_impl(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals, bool packed,
                        const uint8_t *group_of_obs, int32_t n_groups, bool groups, uint32_t *counts, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, offsets, counts, counts, counts);
    if (rc != BVC_OK) return rc;
    if (groups && (rc = check_n_groups(ctx, n_groups)) != BVC_OK) return rc;
    if (n_sites == 0) return BVC_OK;
    if (packed) quals = nullptr;
    const bool have_all = obs && (packed || quals) && (!groups || group_of_obs);
    if (flags & BVC_PTR_DEVICE) {
        if (!have_all) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        return add_csr_device(ctx, n_sites, offsets, obs, quals, groups ? group_of_obs : nullptr, n_groups, counts);
    }
    if ((rc = check_offsets_host(ctx, n_sites, offsets)) != BVC_OK) return rc;
    const size_t total = (size_t)offsets[n_sites];
    if (total > 0 && !have_all) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (total == 0) return BVC_OK;
    Staged in[4] = {{offsets, (size_t)(n_sites + 1) * sizeof(int64_t), nullptr}, {obs, total, nullptr}, {quals, packed ? 0 : total, nullptr},
                    {group_of_obs, groups ? total : 0, nullptr}};
    return add_on_host_pointers(ctx, in, 4, counts, (size_t)n_sites * (size_t)(groups ? n_groups + 1 : 1) * BVC_NCLASS, [&](uint32_t *c) {
        return add_csr_device(ctx, n_sites, static_cast<const int64_t *>(in[0].dev), static_cast<const uint8_t *>(in[1].dev),
                              packed ? nullptr : static_cast<const uint8_t *>(in[2].dev),
                              groups ? static_cast<const uint8_t *>(in[3].dev) : nullptr, n_groups, c);
    });
}

}  // namespace

extern "C" {

int bvc_counts_add_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases, const int8_t *quals,
                         uint32_t *counts, uint32_t flags)
{
    return counts_add_dense_impl(ctx, n_sites, n_samples, row_stride, bases, quals, false, nullptr, 0, false, counts, flags);
}

int bvc_counts_add_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const uint8_t *packed, uint32_t *counts,
                                uint32_t flags)
{
    return counts_add_dense_impl(ctx, n_sites, n_samples, row_stride, reinterpret_cast<const int8_t *>(packed), nullptr, true, nullptr, 0, false,
                                 counts, flags);
}

int bvc_counts_add_dense_groups(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases, const int8_t *quals,
                                const uint8_t *group_of_sample, int32_t n_groups, uint32_t *grp_counts, uint32_t flags)
{
    return counts_add_dense_impl(ctx, n_sites, n_samples, row_stride, bases, quals, false, group_of_sample, n_groups, true, grp_counts, flags);
}

int bvc_counts_add_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals, uint32_t *counts,
                       uint32_t flags)
{
    return counts_add_csr_impl(ctx, n_sites, offsets, reinterpret_cast<const uint8_t *>(bases), reinterpret_cast<const uint8_t *>(quals), false,
                               nullptr, 0, false, counts, flags);
}

int bvc_counts_add_csr_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed, uint32_t *counts, uint32_t flags)
{
    return counts_add_csr_impl(ctx, n_sites, offsets, packed, nullptr, true, nullptr, 0, false, counts, flags);
}

int bvc_counts_add_csr_group_labels(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                                    const uint8_t *group_of_obs, int32_t n_groups, uint32_t *grp_counts, uint32_t flags)
{
    return counts_add_csr_impl(ctx, n_sites, offsets, reinterpret_cast<const uint8_t *>(bases), reinterpret_cast<const uint8_t *>(quals), false,
                               group_of_obs, n_groups, true, grp_counts, flags);
}

int bvc_counts_merge(bvc_ctx *ctx, int64_t n_words, uint32_t *dst, const uint32_t *src, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_words < 0) return fail(ctx, BVC_ERR_ARG, "n_words < 0");
    if (n_words > 0 && (!dst || !src)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    if (n_words == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE) {
        BVC_HIP(ctx, launch_counts_add(ctx->stream, n_words, dst, src));
        return BVC_OK;
    }
    Staged in[1] = {{src, (size_t)n_words * sizeof(uint32_t), nullptr}};
    return add_on_host_pointers(ctx, in, 1, dst, (size_t)n_words, [&](uint32_t *d) -> int {
        BVC_HIP(ctx, launch_counts_add(ctx->stream, n_words, d, static_cast<const uint32_t *>(in[0].dev)));
        return BVC_OK;
    });
}

}  // extern "C"
