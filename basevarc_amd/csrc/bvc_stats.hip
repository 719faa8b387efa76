// bvc_stats.hip -- bvc_site_stats_csr: the called sites' rank sums and strand counts from their entries (site_stats_kernel.hip).  The same
// kernel serves bvc_pileup_finish_called_stats on a tile's own device buffers (bvc_pileup.hip).
#include "bvc_ctx.h"

extern "C" {

int bvc_site_stats_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                       const int8_t *ref_base, const bvc_site_result *results, bvc_site_stats *stats, uint32_t flags)
{
    const int rc0 = check_common(ctx, n_sites, offsets, ref_base, results, stats);
    if (rc0 != BVC_OK) return rc0;
    if (n_sites == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE) {
        // (the offsets are on the device: whether there are entries at all is not known here, so the array must be there)
        if (!entries) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        BVC_HIP(ctx, launch_site_stats(ctx->ls, ctx->stream, n_sites, offsets, entries, ref_base, results, stats));
        return BVC_OK;
    }
    int rc = check_offsets_host(ctx, n_sites, offsets);
    if (rc != BVC_OK) return rc;
    const size_t total = (size_t)offsets[n_sites], ns = (size_t)n_sites;
    if (total > 0 && !entries) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    int64_t *d_off; bvc_pileup_entry *d_ent; int8_t *d_ref; bvc_site_result *d_res; bvc_site_stats *d_st;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_off = L.take<int64_t>(ns + 1);
        d_ent = L.take<bvc_pileup_entry>(total, 16);
        d_ref = L.take<int8_t>(ns, 16);
        d_res = L.take<bvc_site_result>(ns);
        d_st = L.take<bvc_site_stats>(ns);
    });
    if (rc != BVC_OK) return rc;
    PinIO io(ctx);
    rc = io.reserve((ns + 1) * 8 + ns * (1 + sizeof(bvc_site_result)) + 1024, ns * sizeof(bvc_site_stats) + 1024);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.h2d(d_off, offsets, (ns + 1) * 8));
    // the entries are the bulk: straight from the caller's memory (a DMA where it is page-locked), not through the bounce buffer
    if (total) BVC_HIP_D(ctx, hipMemcpyAsync(d_ent, entries, total * sizeof(bvc_pileup_entry), hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, io.h2d(d_ref, ref_base, ns));
    BVC_HIP_D(ctx, io.h2d(d_res, results, ns * sizeof(bvc_site_result)));
    BVC_HIP_D(ctx, launch_site_stats(ctx->ls, ctx->stream, n_sites, d_off, d_ent, d_ref, d_res, d_st));
    BVC_HIP_D(ctx, io.d2h(stats, d_st, ns * sizeof(bvc_site_stats)));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    return BVC_OK;
}

}  // extern "C"
