// bvc_bam.hip -- bvc_bam_pileup and bvc_bam_pileup_bgzf (include/bvc_bam.h): the inflated BAM records of a batch of samples -> the batch's
// position records in the binary temp-batch form (bam_pileup_kernel.hip).  Two passes over the positions in tiles: sizes, one wait for
// the total and the statuses, then the records.
// bvc_bam_pileup_text and bvc_bam_pileup_text_bgzf (include/bvc_bam_text.h): the same call with the batch's lines in the text temp-batch
// form as its output (bam_text_kernel.hip); each shares its whole body with its binary twin (bam_pileup_call, bam_pileup_bgzf_call).
// bvc_bam_popmatrix and bvc_bam_popmatrix_bgzf (include/bvc_popmatrix.h): the same records -> one row of '0' / '1' / '.' per sample
// (bam_popmatrix_kernel.hip).  One pass and one wait.  The two families share the call's inputs (BamCall), their checks and the verdicts
// on the statuses and the blocks; the matrix's two entry points share one tail (bam_popmatrix_from_host, run_bam_popmatrix).
#include "bvc_ctx.h"
#include "../../include/bvc_bam.h"
#include "../../include/bvc_bam_text.h"
#include "../../include/bvc_popmatrix.h"

// (the checks, the staging of a host-pointer call's inputs (BamStage) and the two verdicts are declared in bvc_ctx.h: bvc_bam_counts.hip
// shares them)
int check_sizes(bvc_ctx *ctx, int32_t n_samples, int64_t bam_bytes, int32_t n_positions, int64_t refseq_len, int64_t records_cap)
{
    if (n_samples < 0 || bam_bytes < 0 || n_positions < 0 || refseq_len < 0 || records_cap < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    return BVC_OK;
}

// strict: the positions ascend strictly (the records: one per position); else they may repeat (the matrix: a multi-allelic site is two lines)
int check_host_arrays(bvc_ctx *ctx, int32_t n_samples, const int64_t *sample_off, const int64_t *sample_end, int64_t bam_bytes, int32_t n_positions,
                      const int32_t *positions, bool strict)
{
    for (int32_t s = 0; s < n_samples; ++s)
        if (!(sample_off[s] >= (s ? sample_end[s - 1] : 0) && sample_end[s] >= sample_off[s] && sample_end[s] <= bam_bytes))
            return fail(ctx, BVC_ERR_ARG, "the samples' ranges must lie inside bam, one behind the other");
    for (int32_t t = 1; t < n_positions; ++t)
        if (strict ? positions[t] <= positions[t - 1] : positions[t] < positions[t - 1])
            return fail(ctx, BVC_ERR_ARG, strict ? "positions must be strictly ascending" : "positions must not descend");
    return BVC_OK;
}

int check_blocks(bvc_ctx *ctx, const bvc_bgzf_block *blocks, int64_t n_blocks, int64_t comp_bytes, int64_t bam_bytes)
{
    for (int64_t i = 0; i < n_blocks; ++i) {
        const bvc_bgzf_block &b = blocks[i];
        if (b.comp_off < 0 || b.comp_len < 0 || b.comp_off + b.comp_len > comp_bytes || b.isize < 0 || b.isize > 65536 || b.out_off < 0 ||
            b.out_off + b.isize > bam_bytes)
            return fail(ctx, BVC_ERR_ARG, "block outside its buffer");
    }
    return BVC_OK;
}

// What the statuses' scan found (head[1..3]: the first sample of status 2, 3, 4): BVC_ERR_DATA, BVC_BAM_MORE or BVC_OK, the first named.
int status_verdict(bvc_ctx *ctx, const int64_t head[4])
{
    const int64_t none = 0x7FFFFFFF, bad = head[2] < head[3] ? head[2] : head[3];
    char msg[160];
    if (bad != none) {
        std::snprintf(msg, sizeof msg, "sample %lld: %s", (long long)bad,
                      head[2] == bad ? "truncated or corrupt BAM record" : "index offset is out of range of the sequence");
        return fail(ctx, BVC_ERR_DATA, msg);
    }
    if (head[1] != none) {
        std::snprintf(msg, sizeof msg, "sample %lld: the bytes ran out before a stop record", (long long)head[1]);
        return fail(ctx, BVC_BAM_MORE, msg);
    }
    return BVC_OK;
}

// The first block that did not inflate (or failed its CRC32), as BVC_ERR_DATA; BVC_OK: none.
int block_verdict(bvc_ctx *ctx, const std::vector<uint32_t> &block_status)
{
    for (size_t i = 0; i < block_status.size(); ++i)
        if (block_status[i] != 0) {
            char msg[160];
            std::snprintf(msg, sizeof msg, "BGZF block %lld: %s", (long long)i, block_status[i] == 10 ? "CRC32 mismatch" : "not valid deflate of its ISIZE bytes");
            return fail(ctx, BVC_ERR_DATA, msg);
        }
    return BVC_OK;
}

void BamStage::take(Layout &L)
{
    const size_t ns = (size_t)h.n_samples, np = (size_t)h.n_positions, nb = (size_t)n_blocks;
    u_comp = L.take<uint8_t>((size_t)comp_bytes, 16); u_blk = L.take<bvc_bgzf_block>(nb); u_bst = L.take<uint32_t>(nb);
    u_bam = L.take<uint8_t>((size_t)h.bam_bytes);
    u_off = L.take<int64_t>(ns); u_end = L.take<int64_t>(ns); u_eof = L.take<uint8_t>(ns); u_rid = L.take<int32_t>(ns);
    u_pos = L.take<int32_t>(np); d_status = L.take<uint32_t>(ns);
    d_group = group ? L.take<uint8_t>(ns) : nullptr;
    c.bam = u_bam; c.off = u_off; c.end = u_end; c.eof = u_eof; c.rid = u_rid; c.pos = u_pos;
}

int BamStage::upload(bvc_ctx *ctx, PinIO &io)
{
    const size_t ns = (size_t)h.n_samples, np = (size_t)h.n_positions, nb = (size_t)n_blocks;
    if (nb) {
        BVC_HIP_D(ctx, hipMemcpyAsync(u_comp, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, io.h2d(u_blk, blocks, nb * sizeof(bvc_bgzf_block)));
        // (the bytes between the blocks' outputs, if the caller left any, are no sample's: nothing reads them)
        BVC_HIP_D(ctx, launch_inflate(ctx->stream, u_comp, u_blk, n_blocks, u_bam, u_bst));
        BVC_HIP_D(ctx, io.d2h(block_status.data(), u_bst, nb * 4));
    } else if (h.bam && h.bam_bytes)                // the records are the bulk: straight from the caller's memory (a DMA where it is page-locked)
        BVC_HIP_D(ctx, hipMemcpyAsync(u_bam, h.bam, (size_t)h.bam_bytes, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, io.h2d(u_off, h.off, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_end, h.end, ns * 8));
    BVC_HIP_D(ctx, io.h2d(u_eof, h.eof, ns));
    BVC_HIP_D(ctx, io.h2d(u_rid, h.rid, ns * 4));
    if (group) BVC_HIP_D(ctx, io.h2d(d_group, group, ns));
    BVC_HIP_D(ctx, io.h2d(u_pos, h.pos, np * 4));
    return BVC_OK;
}

namespace {

// The kernels of one call on inputs in device memory.  out_device: records, rec_start and sample_status are device memory and the call
// returns with the second pass enqueued; else they are host memory (d_status: the statuses' place on the device) and the call waits.
// text: the output is the batch's lines (records: the text, rec_start: line_start) instead of its binary records.
// sink (host statuses, out_device false): the records and rec_start go to the device memory it names once the size is known, and the call
// returns with both complete there (sink->wait false: enqueued); records, records_cap and rec_start are unused.  With sink->h_rec_start the
// row comes to the host with the first wait too: the scan has made it, the second pass only reads it.
int run_bam_pileup(bvc_ctx *ctx, PinIO &io, const BamCall &c, bool text, bool out_device, uint32_t *d_status, uint8_t *records, int64_t records_cap,
                   int64_t *records_needed, uint32_t *rec_start, uint32_t *sample_status, BatchSink *sink = nullptr)
{
    const size_t ns = (size_t)c.n_samples, np = (size_t)c.n_positions;
    BamPileupScratch S;
    int rc = carve(ctx, ctx->d_bam, 256, [&](Layout &L) { S = bam_pileup_scratch(L, c.bam_bytes, c.n_samples, c.n_positions); });
    if (rc != BVC_OK) return rc;
    auto tiles = [&](bool place, uint8_t *out) -> hipError_t {
        for (int32_t t0 = 0; t0 < c.n_positions; t0 += S.tile) {
            const int32_t tn = c.n_positions - t0 < S.tile ? c.n_positions - t0 : S.tile;
            const hipError_t e = (text ? launch_bam_text_tile : launch_bam_tile)(ctx->stream, place, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.pos,
                                                                                 t0, tn, c.rg_s, c.ref, c.refseq_len, S, d_status, out);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    BVC_HIP_D(ctx, launch_bam_index(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.eof, c.rid, c.beg0, c.end0, c.min_mapq, S, d_status));
    BVC_HIP_D(ctx, tiles(false, nullptr));
    BVC_HIP_D(ctx, launch_bam_scan(ctx->stream, c.n_positions, c.n_samples, S, d_status));
    int64_t head[4] = {0, 0, 0, 0};
    BVC_HIP_D(ctx, io.d2h(head, S.head, sizeof head));
    if (!out_device && ns) BVC_HIP_D(ctx, io.d2h(sample_status, d_status, ns * 4));
    if (sink && sink->h_rec_start) BVC_HIP_D(ctx, io.d2h(sink->h_rec_start, S.rec_start, (np + 1) * 4));
    BVC_HIP_D(ctx, wait_stream(ctx));               // the one wait of a device-pointer call: the size and the statuses decide what it returns
    io.deliver();
    rc = status_verdict(ctx, head);
    if (rc != BVC_OK) return rc;
    const int64_t need = head[0];
    *records_needed = need;
    if (need > (int64_t)0xFFFFFF00u)
        return fail(ctx, BVC_ERR_ARG, text ? "the text exceeds 0xFFFFFF00 bytes (split the positions)" : "the records exceed 0xFFFFFF00 bytes (split the positions)");
    if (!sink && need > records_cap) {
        (void)fail_cap(ctx, text ? "text" : "records", records_cap, text ? "the batch's lines" : "the batch's records", need);
        return BVC_BAM_MORE;
    }
    uint8_t *d_records = records;
    uint32_t *d_rec_start = rec_start;
    if (sink) {
        rc = sink->reserve(ctx, need, &d_records, &d_rec_start);
        if (rc != BVC_OK) return rc;
    } else if (!out_device) {
        rc = ensure(ctx, ctx->d_bam_out, (size_t)need + 256);
        if (rc != BVC_OK) return rc;
        d_records = reinterpret_cast<uint8_t *>(ctx->d_bam_out.p);
    }
    if (!text) BVC_HIP_D(ctx, hipMemsetAsync(S.carry, 0, ns ? ns : 1, ctx->stream));   // (a text indel token shows no fields: no carry)
    BVC_HIP_D(ctx, tiles(true, d_records));
    if (out_device || sink) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_rec_start, S.rec_start, (np + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (sink && sink->wait) BVC_HIP_D(ctx, wait_stream(ctx));
        return BVC_OK;
    }
    BVC_HIP_D(ctx, io.d2h(rec_start, S.rec_start, (np + 1) * 4));
    if (need) BVC_HIP_D(ctx, hipMemcpyAsync(records, d_records, (size_t)need, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    return BVC_OK;
}


// ---- the population matrix ----------------------------------------------------------------------------------------------------------
// The kernels of one call on inputs in device memory, and its ONE wait.  out_device: matrix and sample_status are device memory; else they
// are host memory (d_status: the statuses' place on the device) and the rows come down through a compact matrix of the context's.
int run_bam_popmatrix(bvc_ctx *ctx, PinIO &io, const BamCall &c, bool out_device, uint32_t *d_status, uint8_t *matrix, int64_t row_stride,
                      uint32_t *sample_status)
{
    const size_t ns = (size_t)c.n_samples, np = (size_t)c.n_positions;
    BamPileupScratch S;
    int rc = carve(ctx, ctx->d_bam, 256, [&](Layout &L) { S = bam_popmatrix_scratch(L, c.bam_bytes, c.n_samples); });
    if (rc != BVC_OK) return rc;
    uint8_t *d_matrix = matrix;
    int64_t d_stride = row_stride;
    if (!out_device) {
        rc = ensure(ctx, ctx->d_bam_out, ns * np + 256);
        if (rc != BVC_OK) return rc;
        d_matrix = reinterpret_cast<uint8_t *>(ctx->d_bam_out.p);
        d_stride = (int64_t)np;
    }
    BVC_HIP_D(ctx, launch_bam_index(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.eof, c.rid, c.beg0, c.end0, c.min_mapq, S, d_status));
    BVC_HIP_D(ctx, launch_bam_popmatrix(ctx->stream, c.n_samples, c.bam, c.bam_bytes, c.off, c.end, c.n_positions, c.pos, c.pref, c.palt, c.rg_s,
                                        c.refseq_len, S, d_matrix, d_stride, d_status));
    BVC_HIP_D(ctx, launch_bam_scan(ctx->stream, 0, c.n_samples, S, d_status));
    int64_t head[4] = {0, 0, 0, 0};
    BVC_HIP_D(ctx, io.d2h(head, S.head, sizeof head));
    if (!out_device) {
        if (ns) BVC_HIP_D(ctx, io.d2h(sample_status, d_status, ns * 4));
        // bytes n_positions .. row_stride of a row stay the caller's
        if (ns && np) BVC_HIP_D(ctx, hipMemcpy2DAsync(matrix, (size_t)row_stride, d_matrix, np, np, ns, hipMemcpyDeviceToHost, ctx->stream));
    }
    BVC_HIP_D(ctx, wait_stream(ctx));               // the one wait: the statuses decide what the call returns
    io.deliver();
    return status_verdict(ctx, head);
}

// Both host-pointer forms: the records from the caller's inflated bytes (bam) or from its BGZF blocks (comp / blocks, CRC checked).
int bam_popmatrix_from_host(bvc_ctx *ctx, const BamCall &h, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                            uint8_t *matrix, int64_t row_stride, uint32_t *sample_status)
{
    int rc = check_host_arrays(ctx, h.n_samples, h.off, h.end, h.bam_bytes, h.n_positions, h.pos, false);
    if (rc != BVC_OK) return rc;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)h.n_samples, np = (size_t)h.n_positions, nb = (size_t)n_blocks;
    PinIO io(ctx);
    rc = io.reserve(ns * 21 + np * 6 + nb * sizeof(bvc_bgzf_block) + 1024, 64 + ns * 4 + nb * 4 + 1024);
    if (rc != BVC_OK) return rc;
    BamStage st(h, comp, comp_bytes, blocks, n_blocks);
    uint8_t *u_ref, *u_alt;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { st.take(L); u_ref = L.take<uint8_t>(np); u_alt = L.take<uint8_t>(np); });
    if (rc != BVC_OK || (rc = st.upload(ctx, io)) != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.h2d(u_ref, h.pref, np));
    BVC_HIP_D(ctx, io.h2d(u_alt, h.palt, np));
    st.c.pref = u_ref; st.c.palt = u_alt;
    rc = run_bam_popmatrix(ctx, io, st.c, false, st.d_status, matrix, row_stride, sample_status);
    // the wait delivered the blocks' statuses too: a block that did not inflate outranks what the kernels made of its bytes
    return block_verdict(ctx, st.block_status) != BVC_OK ? BVC_ERR_DATA : rc;
}

// The checks both entry points make before anything of the device is touched; fills what of the call they share.
int check_popmatrix(bvc_ctx *ctx, BamCall &c, int32_t n_samples, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                    const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                    const int32_t *positions, const uint8_t *ref, const uint8_t *alt, int32_t rg_s, int64_t refseq_len, const uint8_t *matrix,
                    int64_t row_stride, const uint32_t *sample_status)
{
    const int rc = check_sizes(ctx, n_samples, bam_bytes, n_positions, refseq_len, 0);
    if (rc != BVC_OK) return rc;
    if (row_stride < n_positions) return fail(ctx, BVC_ERR_ARG, "need row_stride >= n_positions");
    if ((n_samples > 0 && (!sample_off || !sample_end || !sample_eof || !rid || !sample_status)) || (n_positions > 0 && (!positions || !ref || !alt)) ||
        (n_samples > 0 && n_positions > 0 && !matrix))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    c = bam_call(n_samples, nullptr, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    c.pref = ref; c.palt = alt;
    return BVC_OK;
}

// bvc_bam_pileup (text = false) and bvc_bam_pileup_text (text = true): one body, the output's form apart.
int bam_pileup_call(bool text, bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                   const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                   int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                   uint8_t *records, int64_t records_cap, int64_t *records_needed, uint32_t *rec_start, uint32_t *sample_status,
                   uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (records_needed) *records_needed = 0;
    int rc = check_sizes(ctx, n_samples, bam_bytes, n_positions, refseq_len, records_cap);
    if (rc != BVC_OK) return rc;
    if (!records_needed || !rec_start || (n_samples > 0 && (!sample_off || !sample_end || !sample_eof || !rid || !sample_status)) ||
        (bam_bytes > 0 && !bam) || (n_positions > 0 && !positions) || (refseq_len > 0 && !refseq) || (records_cap > 0 && !records))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const bool device = (flags & BVC_PTR_DEVICE) != 0;
    const size_t ns = (size_t)n_samples, np = (size_t)n_positions;
    if (!device) {
        rc = check_host_arrays(ctx, n_samples, sample_off, sample_end, bam_bytes, n_positions, positions);
        if (rc != BVC_OK) return rc;
    }
    PinIO io(ctx);
    rc = io.reserve(device ? 0 : ns * 21 + np * 4 + 1024, 64 + ns * 4 + (np + 1) * 4 + 1024);
    if (rc != BVC_OK) return rc;
    BamCall c = bam_call(n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len);
    c.ref = reinterpret_cast<const uint8_t *>(refseq);
    if (device) return run_bam_pileup(ctx, io, c, text, true, sample_status, records, records_cap, records_needed, rec_start, sample_status);
    // host pointers: the inputs live in the staging buffer for the length of the call
    BamStage st(c, nullptr, 0, nullptr, 0);
    uint8_t *u_ref;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { st.take(L); u_ref = L.take<uint8_t>((size_t)refseq_len); });
    if (rc != BVC_OK || (rc = st.upload(ctx, io)) != BVC_OK) return rc;
    // (the reference is bulk too: straight from the caller's memory)
    if (refseq_len) BVC_HIP_D(ctx, hipMemcpyAsync(u_ref, refseq, (size_t)refseq_len, hipMemcpyHostToDevice, ctx->stream));
    st.c.ref = u_ref;
    return run_bam_pileup(ctx, io, st.c, text, false, st.d_status, records, records_cap, records_needed, rec_start, sample_status);
}

}  // namespace

// bvc_bam_pileup_bgzf (text = false) and bvc_bam_pileup_text_bgzf (text = true); with a sink bvc_bam_pileup_bgzf_store (bvc_store.hip)
int bam_pileup_bgzf_call(bool text, bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                         int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                         int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                         const char *refseq, int64_t refseq_len, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                         uint32_t *rec_start, uint32_t *sample_status, BatchSink *sink)
{
    if (!ctx) return BVC_ERR_ARG;
    if (records_needed) *records_needed = 0;
    int rc = check_sizes(ctx, n_samples, bam_bytes, n_positions, refseq_len, records_cap);
    if (rc != BVC_OK) return rc;
    if (comp_bytes < 0 || n_blocks < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (!records_needed || (!rec_start && !sink) || (n_samples > 0 && (!sample_off || !sample_end || !sample_eof || !rid || !sample_status)) ||
        (n_blocks > 0 && (!comp || !blocks)) || (n_positions > 0 && !positions) || (refseq_len > 0 && !refseq) || (records_cap > 0 && !records))
        return fail(ctx, BVC_ERR_ARG, "null data pointer");
    rc = check_blocks(ctx, blocks, n_blocks, comp_bytes, bam_bytes);
    if (rc != BVC_OK) return rc;
    rc = check_host_arrays(ctx, n_samples, sample_off, sample_end, bam_bytes, n_positions, positions);
    if (rc != BVC_OK) return rc;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ns = (size_t)n_samples, np = (size_t)n_positions, nb = (size_t)n_blocks;
    PinIO io(ctx);
    rc = io.reserve(ns * 21 + np * 4 + nb * sizeof(bvc_bgzf_block) + 1024, 64 + ns * 4 + (np + 1) * 4 + nb * 4 + 1024);
    if (rc != BVC_OK) return rc;
    BamStage st(bam_call(n_samples, nullptr, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, rg_s, refseq_len),
                comp, comp_bytes, blocks, n_blocks);
    uint8_t *u_ref;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) { st.take(L); u_ref = L.take<uint8_t>((size_t)refseq_len); });
    if (rc != BVC_OK || (rc = st.upload(ctx, io)) != BVC_OK) return rc;
    if (refseq_len) BVC_HIP_D(ctx, hipMemcpyAsync(u_ref, refseq, (size_t)refseq_len, hipMemcpyHostToDevice, ctx->stream));
    st.c.ref = u_ref;
    // the pileup's first wait delivers the blocks' statuses too: a block that did not inflate (or failed its CRC32) outranks what the
    // kernels made of its bytes
    rc = run_bam_pileup(ctx, io, st.c, text, false, st.d_status, records, records_cap, records_needed, rec_start, sample_status, sink);
    if (block_verdict(ctx, st.block_status) != BVC_OK) {
        *records_needed = 0;
        return BVC_ERR_DATA;
    }
    return rc;
}

extern "C" {

int bvc_bam_pileup(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                   const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                   int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                   uint8_t *records, int64_t records_cap, int64_t *records_needed, uint32_t *rec_start, uint32_t *sample_status,
                   uint32_t flags)
{
    return bam_pileup_call(false, ctx, n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions,
                           rg_s, refseq, refseq_len, records, records_cap, records_needed, rec_start, sample_status, flags);
}

int bvc_bam_pileup_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                        int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                        int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                        const char *refseq, int64_t refseq_len, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                        uint32_t *rec_start, uint32_t *sample_status)
{
    return bam_pileup_bgzf_call(false, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0,
                                min_mapq, n_positions, positions, rg_s, refseq, refseq_len, records, records_cap, records_needed, rec_start,
                                sample_status);
}

int bvc_bam_pileup_text(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off,
                        const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                        int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                        uint8_t *text, int64_t text_cap, int64_t *text_needed, uint32_t *line_start, uint32_t *sample_status, uint32_t flags)
{
    return bam_pileup_call(true, ctx, n_samples, bam, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions,
                           rg_s, refseq, refseq_len, text, text_cap, text_needed, line_start, sample_status, flags);
}

int bvc_bam_pileup_text_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                             int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                             int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                             const char *refseq, int64_t refseq_len, uint8_t *text, int64_t text_cap, int64_t *text_needed,
                             uint32_t *line_start, uint32_t *sample_status)
{
    return bam_pileup_bgzf_call(true, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0,
                                min_mapq, n_positions, positions, rg_s, refseq, refseq_len, text, text_cap, text_needed, line_start, sample_status);
}

int bvc_bam_popmatrix(bvc_ctx *ctx, int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                      const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                      const int32_t *positions, const uint8_t *ref, const uint8_t *alt, int32_t rg_s, int64_t refseq_len, uint8_t *matrix,
                      int64_t row_stride, uint32_t *sample_status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    BamCall c;
    const int rc = check_popmatrix(ctx, c, n_samples, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions,
                                   ref, alt, rg_s, refseq_len, matrix, row_stride, sample_status);
    if (rc != BVC_OK) return rc;
    if (bam_bytes > 0 && !bam) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    c.bam = bam;
    if (!(flags & BVC_PTR_DEVICE)) return bam_popmatrix_from_host(ctx, c, nullptr, 0, nullptr, 0, matrix, row_stride, sample_status);
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    PinIO io(ctx);
    const int rs = io.reserve(0, 64 + 1024);
    if (rs != BVC_OK) return rs;
    return run_bam_popmatrix(ctx, io, c, true, sample_status, matrix, row_stride, sample_status);
}

int bvc_bam_popmatrix_bgzf(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                           int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                           int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, const uint8_t *ref,
                           const uint8_t *alt, int32_t rg_s, int64_t refseq_len, uint8_t *matrix, int64_t row_stride, uint32_t *sample_status)
{
    if (!ctx) return BVC_ERR_ARG;
    BamCall c;
    int rc = check_popmatrix(ctx, c, n_samples, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, n_positions, positions, ref,
                             alt, rg_s, refseq_len, matrix, row_stride, sample_status);
    if (rc != BVC_OK) return rc;
    if (comp_bytes < 0 || n_blocks < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (n_blocks > 0 && (!comp || !blocks)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    rc = check_blocks(ctx, blocks, n_blocks, comp_bytes, bam_bytes);
    if (rc != BVC_OK) return rc;
    return bam_popmatrix_from_host(ctx, c, comp, comp_bytes, blocks, n_blocks, matrix, row_stride, sample_status);
}

}  // extern "C"
