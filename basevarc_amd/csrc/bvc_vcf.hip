// bvc_vcf.hip -- bvc_vcf_samples_csr: the sample columns of the called sites' VCF lines from their entries (vcf_samples_kernel.hip), and
// bvc_vcf_bp_lut, the 256 preformatted BP values the kernel copies.  The same kernels serve bvc_pileup_sample_text on a tile's own device
// buffers (bvc_pileup.hip).
#include <cmath>
#include <cstdio>

#include "bvc_ctx.h"

int vcf_lut_device(bvc_ctx *ctx)
{
    if (ctx->d_vcf_lut.p) return BVC_OK;
    const int rc = ensure(ctx, ctx->d_vcf_lut, 2048);
    if (rc != BVC_OK) return rc;
    char lut[2048];
    bvc_vcf_bp_lut(lut);
    const hipError_t e = hipMemcpy(ctx->d_vcf_lut.p, lut, sizeof lut, hipMemcpyHostToDevice);      // (once per context)
    if (e != hipSuccess) {
        (void)hipFree(ctx->d_vcf_lut.p);
        ctx->d_vcf_lut.p = nullptr; ctx->d_vcf_lut.cap = 0;
        return fail(ctx, BVC_ERR_DEVICE, "upload of the BP table", e);
    }
    return BVC_OK;
}

extern "C" {

// The BP sub-field of a covered sample, "d.dddddd" = 1 - 10^(-qual / 10) as %.6f, for every 8-bit quality: the expression and the
// formatting of the host program's bp_field (host/pileup.cpp; src/BaseType.h:10, src/BaseType.cpp:207), eight characters for all 256.
void bvc_vcf_bp_lut(char out[2048])
{
    static const double kMln10To10 = -0.23025850929940458;
    char b[32];
    for (int q = 0; q < 256; ++q) {
        std::snprintf(b, sizeof b, "%.6f", 1 - std::exp(kMln10To10 * q));
        std::memcpy(out + 8 * q, b, 8);
    }
}

int bvc_vcf_samples_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries, const int32_t *samples,
                        const int8_t *ref_base, const bvc_site_result *results, int64_t n_samples, char *text, int64_t text_cap,
                        int64_t *text_off, int64_t *text_len, uint32_t flags)
{
    const int rc0 = check_common(ctx, n_sites, offsets, ref_base, results, text_off);
    if (rc0 != BVC_OK) return rc0;
    if (n_samples < 0 || text_cap < 0) return fail(ctx, BVC_ERR_ARG, "n_samples < 0 or text_cap < 0");
    if (!text_off || (n_sites > 0 && !text_len)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (text_cap > 0 && !text) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    const size_t ns = (size_t)n_sites;
    if (flags & BVC_PTR_DEVICE) {
        if (n_sites == 0) { BVC_HIP(ctx, hipMemsetAsync(text_off, 0, 8, ctx->stream)); return BVC_OK; }
        // (the offsets are on the device: whether there are entries at all is not known here, so the arrays must be there)
        if (!entries || !samples) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        if (reinterpret_cast<uintptr_t>(text) & 15u) return fail(ctx, BVC_ERR_ARG, "device text must start on a 16-byte boundary");
        int rc = vcf_lut_device(ctx);
        if (rc == BVC_OK) rc = ensure(ctx, ctx->d_vcf, vcf_samples_scratch_bytes(n_sites));
        if (rc != BVC_OK) return rc;
        const VcfSamplesScratch scr = vcf_samples_scratch(ctx->d_vcf.p, n_sites);
        BVC_HIP(ctx, launch_vcf_samples_plan(ctx->stream, n_sites, offsets, samples, results, n_samples, text_off, text_len, scr));
        // the one wait of the device form: the sum of the slots is known on the device only, and a caller whose buffer is too small must hear of it
        PinIO io(ctx);
        rc = io.reserve(0, 64);
        if (rc != BVC_OK) return rc;
        int64_t need = 0;
        BVC_HIP_D(ctx, io.d2h(&need, scr.head + 1, 8));
        BVC_HIP_D(ctx, wait_stream(ctx));
        io.deliver();
        if (need > text_cap) return fail_cap(ctx, "text_cap", text_cap, "the called sites' slots", need);
        BVC_HIP(ctx, launch_vcf_samples(ctx->stream, n_sites, offsets, entries, samples, ref_base, results, n_samples, text_off, scr,
                                        ctx->d_vcf_lut.p, text, text_cap));
        return BVC_OK;
    }
    if (n_sites == 0) { text_off[0] = 0; return BVC_OK; }
    int rc = check_offsets_host(ctx, n_sites, offsets);
    if (rc != BVC_OK) return rc;
    const size_t total = (size_t)offsets[n_sites];
    if (total > 0 && (!entries || !samples)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    int64_t need = 0;
    for (int64_t s = 0; s < n_sites; ++s)
        if (results[s].called) need += bvc_vcf_samples_slot(n_samples, offsets[s + 1] - offsets[s]);
    if (need > text_cap) return fail_cap(ctx, "text_cap", text_cap, "the called sites' slots", need);
    rc = vcf_lut_device(ctx);
    if (rc != BVC_OK) return rc;
    int64_t *d_off, *d_toff, *d_tlen; bvc_pileup_entry *d_ent; int32_t *d_smp; int8_t *d_ref; bvc_site_result *d_res; char *d_text, *d_scr;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_off = L.take<int64_t>(ns + 1);
        d_ent = L.take<bvc_pileup_entry>(total, 16);
        d_smp = L.take<int32_t>(total, 16);
        d_ref = L.take<int8_t>(ns, 16);
        d_res = L.take<bvc_site_result>(ns);
        d_toff = L.take<int64_t>(ns + 1);
        d_tlen = L.take<int64_t>(ns);
        d_text = L.take<char>((size_t)need, 16);
        d_scr = L.take<char>(vcf_samples_scratch_bytes(n_sites));
    });
    if (rc != BVC_OK) return rc;
    const VcfSamplesScratch scr = vcf_samples_scratch(d_scr, n_sites);
    PinIO io(ctx);
    rc = io.reserve((ns + 1) * 8 + ns * (1 + sizeof(bvc_site_result)) + 1024, (2 * ns + 1) * 8 + 1024);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.h2d(d_off, offsets, (ns + 1) * 8));
    // the entries and their samples are the bulk going up, the text the bulk coming down: from and to the caller's memory as it is (a DMA
    // where it is page-locked), not through the bounce buffers
    if (total) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_ent, entries, total * sizeof(bvc_pileup_entry), hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_smp, samples, total * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    BVC_HIP_D(ctx, io.h2d(d_ref, ref_base, ns));
    BVC_HIP_D(ctx, io.h2d(d_res, results, ns * sizeof(bvc_site_result)));
    BVC_HIP_D(ctx, launch_vcf_samples_plan(ctx->stream, n_sites, d_off, d_smp, d_res, n_samples, d_toff, d_tlen, scr));
    BVC_HIP_D(ctx, launch_vcf_samples(ctx->stream, n_sites, d_off, d_ent, d_smp, d_ref, d_res, n_samples, d_toff, scr, ctx->d_vcf_lut.p, d_text, need));
    if (need) BVC_HIP_D(ctx, hipMemcpyAsync(text, d_text, (size_t)need, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, io.d2h(text_off, d_toff, (ns + 1) * 8));
    BVC_HIP_D(ctx, io.d2h(text_len, d_tlen, ns * 8));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    return BVC_OK;
}

}  // extern "C"
