// bvc_bam_deflate.hip -- bvc_bam_pileup_bgzf_deflate, bvc_bam_pileup_text_bgzf_deflate and bvc_bam_pileup_deflate_fetch
// (include/bvc_bam_deflate.h): phase 1's temp batch deflated where it is made.  No kernel of its own: bam_pileup_bgzf_call (bvc_bam.hip)
// with a sink that keeps the records or lines in the context's scratch, then bgzf_deflate_device and bgzf_blocks_down (bvc_bgzf.hip) on
// the pieces of that scratch.  Three waits: the pileup's first (sizes, statuses and the rec_start row, from which the host cuts the
// pieces), out_off, the packed bytes.
#include "bvc_ctx.h"
#include "../../include/bvc_bam_deflate.h"

namespace {

// The batch stays in ctx->d_bamz: the rec_start row, then (from a 256-byte boundary) the records, with room behind them for the encoder's
// whole-word loads.  The pileup returns with its second pass enqueued: the encoder's kernels follow it on the same stream.
struct DeflateSink final : BatchSink {
    std::vector<uint32_t> row;
    uint8_t *d_records = nullptr;
    explicit DeflateSink(size_t np) : row(np + 1, 0u)
    {
        h_rec_start = row.data();
        wait = false;
    }
    int reserve(bvc_ctx *ctx, int64_t records_bytes, uint8_t **records, uint32_t **d_rec_start) override
    {
        const size_t head = round256(row.size() * 4);
        const int rc = ensure(ctx, ctx->d_bamz, head + (size_t)records_bytes + 256);
        if (rc != BVC_OK) return rc;
        *d_rec_start = reinterpret_cast<uint32_t *>(ctx->d_bamz.p);
        *records = d_records = reinterpret_cast<uint8_t *>(ctx->d_bamz.p) + head;
        return BVC_OK;
    }
};

int bam_pileup_deflate_call(bool text, bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                            int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof,
                            const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions,
                            int32_t rg_s, const char *refseq, int64_t refseq_len, int32_t n_pieces, const int32_t *piece_pos, uint8_t *out,
                            int64_t out_cap, int64_t *out_needed, int64_t *out_off, int64_t *piece_bytes, uint32_t *sample_status)
{
    if (!ctx) return BVC_ERR_ARG;
    ctx->bamz_kept = -1;                            // whatever an earlier call left is gone from here
    if (out_needed) *out_needed = 0;
    if (n_pieces < 0 || out_cap < 0 || n_positions < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (!out_needed || !piece_pos || !out_off || (n_pieces > 0 && !piece_bytes) || (out_cap > 0 && !out))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (piece_pos[0] != 0 || piece_pos[n_pieces] != n_positions) return fail(ctx, BVC_ERR_ARG, "piece_pos must run from 0 to n_positions");
    for (int32_t i = 0; i < n_pieces; ++i)
        if (piece_pos[i + 1] < piece_pos[i]) return fail(ctx, BVC_ERR_ARG, "piece_pos must not descend");
    const size_t npc = (size_t)n_pieces;
    DeflateSink sink((size_t)n_positions);
    int64_t need = 0;
    int rc = bam_pileup_bgzf_call(text, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0,
                                  min_mapq, n_positions, positions, rg_s, refseq, refseq_len, nullptr, 0, &need, nullptr, sample_status, &sink);
    if (rc != BVC_OK) {
        if (rc == BVC_ERR_ARG && need > (int64_t)0xFFFFFF00u) *out_needed = need;   // (the one failure that reports a size: the uncompressed one)
        return rc;
    }
    // the pieces, from the row the first wait brought down
    std::vector<int64_t> off(npc), len(npc);
    int64_t bound = 0;
    for (size_t i = 0; i < npc; ++i) {
        off[i] = (int64_t)sink.row[(size_t)piece_pos[i]];
        len[i] = (int64_t)sink.row[(size_t)piece_pos[i + 1]] - off[i];
        bound += bvc_bgzf_bound(len[i]);
    }
    if (n_pieces == 0) {                            // (no position: nothing was written, nothing is enqueued)
        out_off[0] = 0;
        return BVC_OK;
    }
    // the packed blocks lie at the FRONT of the buffer: that is where a fetch finds them
    uint8_t *d_comp; int64_t *d_off, *d_len, *d_coff;
    rc = carve(ctx, ctx->d_bamz_out, 256, [&](Layout &L) {
        d_comp = L.take<uint8_t>((size_t)bound);
        d_off = L.take<int64_t>(npc);
        d_len = L.take<int64_t>(npc);
        d_coff = L.take<int64_t>(npc + 1);
    });
    if (rc != BVC_OK) return rc;
    // (the transfers the pileup made through the page-locked buffers are complete: its wait is behind them, its second pass uses none)
    PinIO io(ctx);
    rc = io.reserve((3 * npc + 1) * 8 + 512, (npc + 1) * 8 + 64);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.h2d(d_off, off.data(), npc * 8));
    BVC_HIP_D(ctx, io.h2d(d_len, len.data(), npc * 8));
    rc = bgzf_deflate_device(ctx, io, n_pieces, sink.d_records, d_off, d_len, len.data(), d_comp, bound, d_coff, false);
    if (rc != BVC_OK) return rc;
    std::vector<int64_t> coff(npc + 1);
    rc = bgzf_blocks_down(ctx, io, n_pieces, d_comp, d_coff, out, coff.data(), out_cap);
    if (rc != BVC_OK && rc != BVC_BAM_MORE) return rc;
    *out_needed = coff[npc];
    std::memcpy(out_off, coff.data(), (npc + 1) * 8);
    std::memcpy(piece_bytes, len.data(), npc * 8);
    if (rc == BVC_BAM_MORE) {
        ctx->bamz_kept = coff[npc];
        (void)fail_cap(ctx, "out_cap", out_cap, "the batch's blocks", coff[npc]);
    }
    return rc;
}

}  // namespace

extern "C" {

int bvc_bam_pileup_bgzf_deflate(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                                int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                                const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                                int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                                int32_t n_pieces, const int32_t *piece_pos, uint8_t *out, int64_t out_cap, int64_t *out_needed,
                                int64_t *out_off, int64_t *piece_bytes, uint32_t *sample_status)
{
    return bam_pileup_deflate_call(false, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0,
                                   end0, min_mapq, n_positions, positions, rg_s, refseq, refseq_len, n_pieces, piece_pos, out, out_cap, out_needed,
                                   out_off, piece_bytes, sample_status);
}

int bvc_bam_pileup_text_bgzf_deflate(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                                     int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                                     const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                                     int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                                     int32_t n_pieces, const int32_t *piece_pos, uint8_t *out, int64_t out_cap, int64_t *out_needed,
                                     int64_t *out_off, int64_t *piece_bytes, uint32_t *sample_status)
{
    return bam_pileup_deflate_call(true, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0,
                                   end0, min_mapq, n_positions, positions, rg_s, refseq, refseq_len, n_pieces, piece_pos, out, out_cap, out_needed,
                                   out_off, piece_bytes, sample_status);
}

int bvc_bam_pileup_deflate_fetch(bvc_ctx *ctx, uint8_t *out, int64_t out_cap)
{
    if (!ctx) return BVC_ERR_ARG;
    if (ctx->bamz_kept < 0) return fail(ctx, BVC_ERR_ARG, "no blocks are kept: the last bvc_bam_pileup*_bgzf_deflate did not end in BVC_BAM_MORE for out_cap");
    if (out_cap < ctx->bamz_kept) return fail_cap(ctx, "out_cap", out_cap, "the kept blocks", ctx->bamz_kept);
    if (ctx->bamz_kept > 0 && !out) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (ctx->bamz_kept == 0) return BVC_OK;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    BVC_HIP_D(ctx, hipMemcpyAsync(out, ctx->d_bamz_out.p, (size_t)ctx->bamz_kept, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

}  // extern "C"
