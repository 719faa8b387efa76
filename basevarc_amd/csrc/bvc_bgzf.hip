// bvc_bgzf.hip -- bvc_bgzf_deflate: byte ranges deflated into finished BGZF blocks on the device (bgzf_deflate_kernel.hip; tuning keys
// "bgzf_codes", "bgzf_parse" and "bgzf_cuts" choose the block kernel's instantiation, bgzf_block_kernel.h), and bvc_bgzf_code_lengths: the
// dynamic code's code-length builder on its own.
// bvc_pileup_sample_bgzf (bvc_pileup.hip) hands a tile's sample columns to the same kernels where they are made.
#include "bvc_ctx.h"
#include "../../include/bvc_bgzf_codes.h"

int bgzf_deflate_device(bvc_ctx *ctx, PinIO &io, int64_t n_pieces, const uint8_t *d_data, const int64_t *d_off, const int64_t *d_len,
                        const int64_t *upper, uint8_t *d_comp, int64_t comp_cap, int64_t *d_comp_off, bool wait_for_upload)
{
    std::vector<int64_t> first((size_t)n_pieces + 1);
    int64_t n_blocks = 0;
    for (int64_t i = 0; i < n_pieces; ++i) { first[(size_t)i] = n_blocks; n_blocks += bvc_bgzf_blocks(upper[i]); }
    first[(size_t)n_pieces] = n_blocks;
    const int rc = ensure(ctx, ctx->d_bgzf, bgzf_deflate_scratch_bytes(n_pieces, n_blocks));
    if (rc != BVC_OK) return rc;
    const BgzfDeflateScratch scr = bgzf_deflate_scratch(ctx->d_bgzf.p, n_pieces, n_blocks);
    BVC_HIP_D(ctx, io.h2d(scr.first_block, first.data(), first.size() * 8));
    // a call that returns with its launches in flight must not leave a transfer out of the page-locked buffer in flight too: the next
    // call on the context fills that buffer at once.  (The stream holds nothing but this copy here: its caller has just waited.)
    if (wait_for_upload) BVC_HIP_D(ctx, wait_stream(ctx));
    BVC_HIP_D(ctx, launch_bgzf_deflate(ctx->stream, n_pieces, d_data, d_off, d_len, n_blocks, scr, d_comp, comp_cap, d_comp_off, bgzf_mode(ctx->ls)));
    return BVC_OK;
}

int bgzf_blocks_down(bvc_ctx *ctx, PinIO &io, int64_t n_pieces, const uint8_t *d_comp, const int64_t *d_comp_off, uint8_t *comp,
                     int64_t *comp_off, int64_t comp_cap)
{
    BVC_HIP_D(ctx, io.d2h(comp_off, d_comp_off, ((size_t)n_pieces + 1) * 8));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    // the second wait: only the packed bytes come down, and how many they are was not known before
    const int64_t packed = comp_off[n_pieces];
    if (comp_cap >= 0 && packed > comp_cap) return BVC_BAM_MORE;
    if (packed > 0) {
        BVC_HIP_D(ctx, hipMemcpyAsync(comp, d_comp, (size_t)packed, hipMemcpyDeviceToHost, ctx->stream));
        BVC_HIP_D(ctx, wait_stream(ctx));
    }
    return BVC_OK;
}

// The sum of the pieces' lengths and of their bounds; false where an offset or a length is negative.
static bool sum_pieces(int64_t n_pieces, const int64_t *off, const int64_t *len, int64_t *total, int64_t *need)
{
    *total = 0; *need = 0;
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (off[i] < 0 || len[i] < 0) return false;
        *total += len[i];
        *need += bvc_bgzf_bound(len[i]);
    }
    return true;
}

extern "C" {

int bvc_bgzf_deflate(bvc_ctx *ctx, int64_t n_pieces, const uint8_t *data, const int64_t *piece_off, const int64_t *piece_len,
                     uint8_t *comp, int64_t comp_cap, int64_t *comp_off, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_pieces < 0 || comp_cap < 0) return fail(ctx, BVC_ERR_ARG, "n_pieces < 0 or comp_cap < 0");
    if (!comp_off || (n_pieces > 0 && (!piece_off || !piece_len))) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_pieces > (int64_t)0x7FFFFFFF / 64) return fail(ctx, BVC_ERR_ARG, "too many pieces in one call");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)n_pieces;
    PinIO io(ctx);
    const bool device = (flags & BVC_PTR_DEVICE) != 0;
    if (n_pieces == 0) {                                          // (no piece: nothing below could refuse the call)
        if (device) BVC_HIP(ctx, hipMemsetAsync(comp_off, 0, 8, ctx->stream)); else comp_off[0] = 0;
        return BVC_OK;
    }
    int rc;
    std::vector<int64_t> down;                                    // the device form: the pieces' offsets, then their lengths, on the host
    const int64_t *h_off = piece_off, *h_len = piece_len;
    if (device) {
        // the wait of the device form: the launches and the scratch are sized from the pieces' lengths
        rc = io.reserve((np + 1) * 8 + 64, 2 * np * 8 + 128);
        if (rc != BVC_OK) return rc;
        down.resize(2 * np);
        h_off = down.data(); h_len = down.data() + np;
        BVC_HIP_D(ctx, io.d2h(down.data(), piece_off, np * 8));
        BVC_HIP_D(ctx, io.d2h(down.data() + np, piece_len, np * 8));
        BVC_HIP_D(ctx, wait_stream(ctx));
        io.deliver();
    }
    int64_t total = 0, need = 0;
    if (!sum_pieces(n_pieces, h_off, h_len, &total, &need)) return fail(ctx, BVC_ERR_ARG, "a negative piece_off or piece_len");
    if ((total > 0 && !data) || (need > 0 && !comp)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (need > comp_cap) return fail_cap(ctx, "comp_cap", comp_cap, "the bounds of the pieces", need);
    if (device) return bgzf_deflate_device(ctx, io, n_pieces, data, piece_off, piece_len, h_len, comp, comp_cap, comp_off, true);
    uint8_t *d_data, *d_comp; int64_t *d_off, *d_len, *d_coff;
    rc = carve(ctx, ctx->d_bgzf_io, 256, [&](Layout &L) {
        d_data = L.take<uint8_t>((size_t)total, 16);
        d_off = L.take<int64_t>(np);
        d_len = L.take<int64_t>(np);
        d_comp = L.take<uint8_t>((size_t)need);
        d_coff = L.take<int64_t>(np + 1);
    });
    if (rc != BVC_OK) return rc;
    rc = io.reserve((size_t)total + (3 * np + 1) * 8 + 512, (np + 1) * 8 + 64);
    if (rc != BVC_OK) return rc;
    // the pieces one after the other (wherever they lie in the caller's memory) through the page-locked buffer: one transfer
    std::vector<int64_t> off(np);
    {
        char *const stage = ctx->h_up + io.up_used;
        int64_t at = 0;
        for (size_t i = 0; i < np; ++i) {
            off[i] = at;
            if (piece_len[i]) std::memcpy(stage + at, data + piece_off[i], (size_t)piece_len[i]);
            at += piece_len[i];
        }
        io.up_used += PinIO::al((size_t)total);
        if (total) BVC_HIP_D(ctx, hipMemcpyAsync(d_data, stage, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    }
    BVC_HIP_D(ctx, io.h2d(d_off, off.data(), np * 8));
    BVC_HIP_D(ctx, io.h2d(d_len, piece_len, np * 8));
    rc = bgzf_deflate_device(ctx, io, n_pieces, d_data, d_off, d_len, piece_len, d_comp, need, d_coff, false);
    if (rc != BVC_OK) return rc;
    return bgzf_blocks_down(ctx, io, n_pieces, d_comp, d_coff, comp, comp_off);
}

int bvc_bgzf_code_lengths(bvc_ctx *ctx, int64_t n_sets, const uint32_t *counts, int32_t n_symbols, int32_t limit, uint8_t *lengths)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_sets < 0 || n_sets > ((int64_t)1 << 22)) return fail(ctx, BVC_ERR_ARG, "n_sets < 0 or above 2^22");
    if (n_symbols < 1 || n_symbols > 288) return fail(ctx, BVC_ERR_ARG, "n_symbols outside 1..288");
    if (limit < 1 || limit > 15 || (1 << limit) < (n_symbols > 2 ? n_symbols : 2)) return fail(ctx, BVC_ERR_ARG, "limit outside 1..15 or 2^limit below n_symbols");
    if (n_sets == 0) return BVC_OK;
    if (!counts || !lengths) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    const size_t total = (size_t)n_sets * (size_t)n_symbols;
    for (int64_t i = 0; i < n_sets; ++i) {
        uint64_t sum = 0;
        for (int32_t s = 0; s < n_symbols; ++s) sum += counts[(size_t)i * (size_t)n_symbols + (size_t)s];
        if (sum >= ((uint64_t)1 << 24)) return fail(ctx, BVC_ERR_ARG, "the counts of a set sum to 2^24 or more");
    }
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *d_counts; uint8_t *d_len;
    int rc = carve(ctx, ctx->d_bgzf_io, 256, [&](Layout &L) {
        d_counts = L.take<uint32_t>(total);
        d_len = L.take<uint8_t>(total);
    });
    if (rc != BVC_OK) return rc;
    PinIO io(ctx);
    rc = io.reserve(total * 4 + 256, total + 256);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.h2d(d_counts, counts, total * 4));
    BVC_HIP_D(ctx, launch_bgzf_code_lengths(ctx->stream, n_sets, d_counts, n_symbols, limit, d_len));
    BVC_HIP_D(ctx, io.d2h(lengths, d_len, total));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    return BVC_OK;
}

}  // extern "C"
