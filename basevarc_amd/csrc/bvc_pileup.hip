// bvc_pileup.hip -- the producer: BGZF blocks inflated on the device, and temp-batch tiles (text, binary records, or BGZF blocks of
// text) -> columns -> records between a begin call and a finish call (pileup_kernel.hip, inflate_kernel.hip).
#include "bvc_ctx.h"

extern "C" {

// ---- BGZF blocks on the device (inflate_kernel.hip) ------------------------------------------------------------------------
int bvc_inflate_blocks(bvc_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                       uint8_t *out, int64_t out_bytes, uint32_t *status, uint32_t flags)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_blocks < 0 || comp_bytes < 0 || out_bytes < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (n_blocks == 0) return BVC_OK;
    if (!comp || !blocks || !status || (!out && out_bytes > 0)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    if (flags & BVC_PTR_DEVICE) {
        BVC_HIP(ctx, launch_inflate(ctx->stream, comp, blocks, n_blocks, out, status));
        return BVC_OK;
    }
    for (int64_t i = 0; i < n_blocks; ++i) {
        const bvc_bgzf_block &b = blocks[i];
        if (b.comp_off < 0 || b.comp_len < 0 || b.comp_off + b.comp_len > comp_bytes || b.isize < 0 || b.isize > 65536 || b.out_off < 0 ||
            b.out_off + b.isize > out_bytes)
            return fail(ctx, BVC_ERR_ARG, "block outside its buffer");
    }
    uint8_t *d_c, *d_o; bvc_bgzf_block *d_b; uint32_t *d_s;
    int rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_c = L.take<uint8_t>((size_t)comp_bytes, 16);
        d_b = L.take<bvc_bgzf_block>((size_t)n_blocks);
        d_s = L.take<uint32_t>((size_t)n_blocks);
        d_o = L.take<uint8_t>((size_t)out_bytes);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_c, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_b, blocks, (size_t)n_blocks * sizeof(bvc_bgzf_block), hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, launch_inflate(ctx->stream, d_c, d_b, n_blocks, d_o, d_s));
    BVC_HIP_D(ctx, hipMemcpyAsync(status, d_s, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_bytes) BVC_HIP_D(ctx, hipMemcpyAsync(out, d_o, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

// ---- temp-batch pileup text -> columns -> records (pileup_kernel.hip) -------------------------------------------------------
}  // extern "C": the three helpers below are shared with bvc_store.hip (bvc_ctx.h)

// The slices of a tile's meta buffer that both begin calls lay out alike: the line table, the first sample and the size of every
// batch (each slice batch_pad bytes longer), the per-line words, 256 bytes of status (the totals at +64), the two offset arrays
// and the tallies.  Returns the bytes from the status to the end of the tallies: what a begin call clears.
size_t carve_tile(Layout &L, PileupTile &P, int32_t n_batches, int32_t n_pos, size_t batch_pad, uint32_t *&line_start,
                  int32_t *&sample0, int32_t *&n_in_batch)
{
    const size_t T = (size_t)n_pos, nb = (size_t)n_batches;
    P.n_batches = n_batches; P.n_pos = n_pos; P.line_stride = n_pos + 1;
    P.n_lines_cap = (int64_t)n_batches * n_pos;
    P.line_start = line_start = L.take<uint32_t>(nb * (T + 1));
    P.sample0 = sample0 = L.take<int32_t>(nb, batch_pad);
    P.n_in_batch = n_in_batch = L.take<int32_t>(nb, batch_pad);
    P.line_words = L.take<uint32_t>((size_t)P.n_lines_cap * 4);
    const size_t from = L.at;
    char *st = L.take<char>(256);
    P.status = reinterpret_cast<uint32_t *>(st);
    P.totals = reinterpret_cast<int64_t *>(st + 64);
    P.entry_off = L.take<int64_t>(T + 1);
    P.obs_off = L.take<int64_t>(T + 1);
    P.tally = L.take<int32_t>(T * 32);
    return L.at - from;
}

// What a begin call checks of a batch's row of the host's table before a kernel indexes the tile with it.  Text: every line inside the text,
// the lines of a batch in order.
static int check_lines(bvc_ctx *ctx, const uint32_t *ls, int32_t n_positions, int64_t text_bytes)
{
    for (int32_t t = 0; t < n_positions; ++t)
        if (ls[t + 1] <= ls[t]) return fail(ctx, BVC_ERR_ARG, "line_start: every line holds at least its newline, lines of a batch ascend");
    if (n_positions > 0 && (int64_t)ls[n_positions] > text_bytes) return fail(ctx, BVC_ERR_ARG, "line_start points outside the text");
    return BVC_OK;
}

// Binary records: every record inside the buffer, as long as its length word says (the kernel bounds every load with the table).
int check_records(bvc_ctx *ctx, const uint8_t *records, const uint32_t *rs, int32_t n_positions, int64_t records_bytes)
{
    for (int32_t t = 0; t < n_positions; ++t) {
        const int64_t r0 = rs[t], r1 = rs[t + 1];
        if (r1 < r0 + 4 || r1 > records_bytes) return fail(ctx, BVC_ERR_ARG, "rec_start: records of a batch ascend, each holds its length word, all lie inside records_bytes");
        const uint8_t *q = records + r0;
        const int64_t len = (int64_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
        if (r1 - r0 != 4 + len) return fail(ctx, BVC_ERR_ARG, "rec_start disagrees with a record's length word");
    }
    return BVC_OK;
}

// The end of a begin call whose count pass is enqueued: the one wait, the verdict on the status, the tile marked begun.
int pileup_begin_verdict(bvc_ctx *ctx, bool bin, int64_t *n_entries, int64_t *n_indels, int64_t *indel_text_bytes)
{
    PileupState::Tile &tile = ctx->pile.tile;
    const PileupTile &P = tile.P;
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t tot[2] = {0, 0};
    BVC_HIP_D(ctx, hipMemcpyAsync(st, P.status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(tot, P.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    if (st[0] != 0) {
        if (!bin) return BVC_PILEUP_IRREGULAR;                           // the caller parses such a tile on the host
        const std::string what = std::to_string(st[0]) + " malformed record(s) in the tile (an entry or an indel text runs past its record's end, or a "
                                 "sample index is not below the batch's size)";
        return fail(ctx, BVC_ERR_DATA, what.c_str());
    }
    tile.entries = tot[0]; tile.obs = tot[1]; tile.indels = st[1];
    // pileup_finish_impl gathers indel_bytes of indel text on the device: a text tile's caller has the text itself and its tile gathers none
    tile.indel_bytes = bin ? st[4] : 0;
    tile.begun = true;
    *n_entries = tot[0]; *n_indels = st[1];
    if (indel_text_bytes) *indel_text_bytes = tile.indel_bytes;
    return BVC_OK;
}

extern "C" {

// bvc_pileup_begin (bin = false: `data` is the text, row_start its line table) and bvc_pileup_begin_bin (true: the binary records of the same
// content (host/pileup.h) go where the text goes, rec_start where line_start goes, and the tile is marked so that the count and write passes
// launch pileup_bin_kernel); bvc_pileup_finish[_called] serve both alike.  The forms differ in the check of the table, in P.bin and in what
// a tile that does not parse means.
static int pileup_begin_impl(bvc_ctx *ctx, bool bin, const uint8_t *data, int64_t data_bytes, const uint32_t *row_start,
                             const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                             int64_t *n_entries, int64_t *n_indels)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState::Tile &tile = ctx->pile.tile;
    tile = PileupState::Tile{};
    if (n_batches < 0 || n_positions < 0 || data_bytes < 0 || !n_entries || !n_indels) return fail(ctx, BVC_ERR_ARG, "bad argument");
    if (data_bytes > (int64_t)0xFFFFFF00)
        return fail(ctx, BVC_ERR_ARG, bin ? "more than 4 GiB of records in one tile (use fewer positions)"
                                          : "more than 4 GiB of text in one tile (use fewer positions)");
    const int64_t n_rows = (int64_t)n_batches * n_positions;
    if (n_rows > 0 && (!data || !row_start || !sample0 || !n_in_batch)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_positions > (int32_t)(0x7FFFFFFF / 64)) return fail(ctx, BVC_ERR_ARG, "too many positions in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    *n_entries = 0; *n_indels = 0;
    for (int32_t b = 0; b < n_batches; ++b) {
        const uint32_t *rows = row_start + (int64_t)b * (n_positions + 1);
        if (n_in_batch[b] < 0) return fail(ctx, BVC_ERR_ARG, "negative batch size");
        const int rcb = bin ? check_records(ctx, data, rows, n_positions, data_bytes) : check_lines(ctx, rows, n_positions, data_bytes);
        if (rcb != BVC_OK) return rcb;
    }
    const size_t T = (size_t)n_positions, nb = (size_t)n_batches;
    PileupTile &P = tile.P;
    uint32_t *d_rows; int32_t *d_s0, *d_nib;
    size_t clear = 0;
    int rc = ensure(ctx, ctx->pile.text, (size_t)data_bytes + 64);
    if (rc == BVC_OK)
        rc = carve(ctx, ctx->pile.meta, 0, [&](Layout &L) { clear = carve_tile(L, P, n_batches, n_positions, 0, d_rows, d_s0, d_nib); });
    if (rc != BVC_OK) return rc;
    P.text = reinterpret_cast<const uint8_t *>(ctx->pile.text.p);
    P.bin = bin;
    BVC_HIP_D(ctx, hipMemsetAsync(P.status, 0, clear, ctx->stream));     // status, totals, offsets of an empty tile, tallies
    if (n_rows > 0) {
        BVC_HIP_D(ctx, hipMemcpyAsync(ctx->pile.text.p, data, (size_t)data_bytes, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_rows, row_start, nb * (T + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_s0, sample0, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_nib, n_in_batch, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, launch_pileup_count(ctx->stream, P));
    }
    return pileup_begin_verdict(ctx, bin, n_entries, n_indels, nullptr);
}

int bvc_pileup_begin(bvc_ctx *ctx, const char *text, int64_t text_bytes, const uint32_t *line_start,
                     const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                     int64_t *n_entries, int64_t *n_indels)
{
    return pileup_begin_impl(ctx, false, reinterpret_cast<const uint8_t *>(text), text_bytes, line_start, sample0, n_in_batch, n_batches,
                             n_positions, n_entries, n_indels);
}

int bvc_pileup_begin_bin(bvc_ctx *ctx, const uint8_t *records, int64_t records_bytes, const uint32_t *rec_start,
                         const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                         int64_t *n_entries, int64_t *n_indels)
{
    return pileup_begin_impl(ctx, true, records, records_bytes, rec_start, sample0, n_in_batch, n_batches, n_positions, n_entries, n_indels);
}

int bvc_pileup_begin_bgzf(bvc_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                          const int32_t *blocks_of_batch, const int32_t *skip_bytes, const int32_t *sample0, const int32_t *n_in_batch,
                          int32_t n_batches, int32_t max_positions, int32_t reset, int32_t *n_positions, int32_t *lines_of_batch,
                          int64_t *n_entries, int64_t *n_indels, int64_t *indel_text_bytes)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState &pile = ctx->pile;
    pile.tile = PileupState::Tile{};
    if (n_batches < 0 || max_positions < 0 || comp_bytes < 0 || !n_positions || !n_entries || !n_indels || !indel_text_bytes)
        return fail(ctx, BVC_ERR_ARG, "bad argument");
    if (n_batches > 0 && (!blocks_of_batch || !sample0 || !n_in_batch || !lines_of_batch)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (max_positions > (int32_t)(0x7FFFFFFF / 64)) return fail(ctx, BVC_ERR_ARG, "too many positions in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    *n_positions = 0; *n_entries = 0; *n_indels = 0; *indel_text_bytes = 0;
    const size_t nb = (size_t)n_batches;
    if (reset || pile.left_len.size() != nb) { pile.left_len.assign(nb, 0u); pile.left_src.assign(nb, 0u); }
    int64_t n_blocks = 0;
    for (size_t b = 0; b < nb; ++b) { if (blocks_of_batch[b] < 0 || n_in_batch[b] < 0) return fail(ctx, BVC_ERR_ARG, "negative count"); n_blocks += blocks_of_batch[b]; }
    if (n_blocks > 0 && (!comp || !blocks)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    // layout of the new text buffer: per batch [left over | its new blocks' output], every region from a 16-byte boundary
    std::vector<bvc_bgzf_block> blk((size_t)n_blocks);
    std::vector<bvc_pileup_region> reg(nb);
    std::vector<uint32_t> seg_base(nb + 1);
    std::vector<uint32_t> region_end(nb);
    uint64_t at = 0;
    int64_t bi = 0;
    uint32_t segs = 0;
    for (size_t b = 0; b < nb; ++b) {
        at = (at + 15) & ~(uint64_t)15;
        const uint32_t left = pile.left_len[b];
        uint64_t fresh = 0;
        for (int32_t k = 0; k < blocks_of_batch[b]; ++k, ++bi) {
            const bvc_bgzf_block &in = blocks[bi];
            if (in.comp_off < 0 || in.comp_len < 0 || in.comp_off + in.comp_len > comp_bytes || in.isize < 0 || in.isize > 65536)
                return fail(ctx, BVC_ERR_ARG, "block outside its buffer");
            blk[(size_t)bi] = in;
            blk[(size_t)bi].out_off = (int64_t)(at + left + fresh);
            fresh += (uint64_t)in.isize;
        }
        uint32_t skip = 0;
        if (skip_bytes && left == 0 && skip_bytes[b] > 0) skip = (uint32_t)skip_bytes[b];
        if (skip > fresh) return fail(ctx, BVC_ERR_ARG, "skip_bytes beyond the batch's first blocks");
        if (at + left + fresh > (uint64_t)0xFFFFFF00u) return fail(ctx, BVC_ERR_ARG, "more than 4 GiB of text in one tile (send fewer blocks)");
        reg[b].start = (uint32_t)at + skip; reg[b].len = left + (uint32_t)fresh - skip; reg[b].left_src = pile.left_src[b]; reg[b].left_len = left;
        region_end[b] = reg[b].start + reg[b].len;
        seg_base[b] = segs;
        segs += (reg[b].len + 1023u) / 1024u;
        at += left + fresh;
    }
    seg_base[nb] = segs;
    const uint64_t text_bytes = at;
    const int nw = 1 - pile.pz_cur;
    PileupTile &P = pile.tile.P;
    int32_t *d_s0, *d_nib, *d_lines; uint32_t *d_ls, *d_bst, *d_sb, *d_sn, *d_ends; bvc_bgzf_block *d_blk; bvc_pileup_region *d_reg;
    size_t clear = 0;
    int rc = ensure(ctx, pile.pz_text[nw], (size_t)text_bytes + 64);
    if (rc == BVC_OK) rc = ensure(ctx, pile.pz_comp, (size_t)comp_bytes + 64);
    if (rc == BVC_OK)
        rc = carve(ctx, pile.meta, 0, [&](Layout &L) {
            clear = carve_tile(L, P, n_batches, max_positions, 4, d_ls, d_s0, d_nib);
            d_blk = L.take<bvc_bgzf_block>((size_t)n_blocks);
            d_bst = L.take<uint32_t>((size_t)n_blocks);
            d_reg = L.take<bvc_pileup_region>(nb);
            d_sb = L.take<uint32_t>(nb + 1);
            d_sn = L.take<uint32_t>(segs, 4);
            d_lines = L.take<int32_t>(nb, 4);
            d_ends = L.take<uint32_t>(nb, 4);
        });
    if (rc != BVC_OK) return rc;
    uint8_t *text_out = reinterpret_cast<uint8_t *>(pile.pz_text[nw].p);
    P.text = text_out;
    int32_t *d_T = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(P.status) + 128);
    P.n_pos_dev = d_T;
    PinIO io(ctx);
    rc = io.reserve((n_blocks > 0 && in_pinned(comp, (size_t)comp_bytes) ? 0 : (size_t)comp_bytes) + (size_t)n_blocks * sizeof(bvc_bgzf_block) +
                        nb * (sizeof(bvc_pileup_region) + 12) + 1024,
                    (size_t)n_blocks * 4 + nb * 8 + 1024);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemsetAsync(P.status, 0, clear, ctx->stream));
    std::vector<uint32_t> bst((size_t)n_blocks);
    std::vector<uint32_t> ends(nb);
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t tot[2] = {0, 0};
    int32_t Tgot = 0;
    if (nb > 0) {
        if (n_blocks > 0) {
            BVC_HIP_D(ctx, io.h2d(pile.pz_comp.p, comp, (size_t)comp_bytes));
            BVC_HIP_D(ctx, io.h2d(d_blk, blk.data(), (size_t)n_blocks * sizeof(bvc_bgzf_block)));
        }
        BVC_HIP_D(ctx, io.h2d(d_reg, reg.data(), nb * sizeof(bvc_pileup_region)));
        BVC_HIP_D(ctx, io.h2d(d_sb, seg_base.data(), (nb + 1) * 4));
        BVC_HIP_D(ctx, io.h2d(d_s0, sample0, nb * 4));
        BVC_HIP_D(ctx, io.h2d(d_nib, n_in_batch, nb * 4));
        BVC_HIP_D(ctx, launch_region_carry(ctx->stream, reinterpret_cast<const uint8_t *>(pile.pz_text[pile.pz_cur].p), text_out, d_reg,
                                           n_batches));
        if (n_blocks > 0)
            BVC_HIP_D(ctx, launch_inflate(ctx->stream, reinterpret_cast<const uint8_t *>(pile.pz_comp.p), d_blk, n_blocks, text_out, d_bst));
        BVC_HIP_D(ctx, launch_region_index(ctx->stream, P, d_reg, d_sb, (int64_t)segs, d_sn, d_lines, max_positions));
        BVC_HIP_D(ctx, launch_region_ends(ctx->stream, P, d_ends));
        BVC_HIP_D(ctx, launch_pileup_count(ctx->stream, P));
        if (n_blocks > 0) BVC_HIP_D(ctx, io.d2h(bst.data(), d_bst, (size_t)n_blocks * 4));
        BVC_HIP_D(ctx, io.d2h(lines_of_batch, d_lines, nb * 4));
        BVC_HIP_D(ctx, io.d2h(ends.data(), d_ends, nb * 4));
        BVC_HIP_D(ctx, io.d2h(&Tgot, d_T, 4));
    }
    BVC_HIP_D(ctx, io.d2h(st, P.status, sizeof st));
    BVC_HIP_D(ctx, io.d2h(tot, P.totals, sizeof tot));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    for (int64_t i = 0; i < n_blocks; ++i)
        if (bst[(size_t)i] != 0) {
            pile.left_len.assign(nb, 0u);                        // the stream of this window is broken: nothing to carry on with
            return fail(ctx, BVC_ERR_DATA, bst[(size_t)i] == 10 ? "a BGZF block of a temp batch fails its CRC32"
                                                                : "a BGZF block of a temp batch is not valid deflate of its ISIZE bytes");
        }
    // what this tile leaves of every batch: from the end of its last line to the end of its region
    for (size_t b = 0; b < nb; ++b) { pile.left_src[b] = ends[b]; pile.left_len[b] = region_end[b] - ends[b]; }
    pile.pz_cur = nw;
    P.n_pos = Tgot; P.n_pos_dev = nullptr;
    pile.tile.text_bytes = (int64_t)text_bytes;
    pile.tile.on_device_text = true;
    *n_positions = Tgot;
    if (Tgot == 0) return BVC_OK;
    if (st[0] != 0) return BVC_PILEUP_IRREGULAR;
    pile.tile.entries = tot[0]; pile.tile.obs = tot[1]; pile.tile.indels = st[1]; pile.tile.indel_bytes = st[4];
    pile.tile.begun = true;
    *n_entries = tot[0]; *n_indels = st[1]; *indel_text_bytes = st[4];
    return BVC_OK;
}

int bvc_pileup_text(bvc_ctx *ctx, char *text, int64_t text_cap, int64_t *text_bytes_needed, uint32_t *line_start)
{
    if (!ctx || !text_bytes_needed) return BVC_ERR_ARG;
    const PileupState::Tile &tile = ctx->pile.tile;
    if (!tile.on_device_text) return fail(ctx, BVC_ERR_ARG, "bvc_pileup_text without a tile from bvc_pileup_begin_bgzf");
    *text_bytes_needed = tile.text_bytes;
    if (!text) return BVC_OK;
    if (text_cap < tile.text_bytes || !line_start) return fail(ctx, BVC_ERR_ARG, "text buffer too small / null line table");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const PileupTile &P = tile.P;
    if (tile.text_bytes) BVC_HIP(ctx, hipMemcpyAsync(text, P.text, (size_t)tile.text_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (P.n_batches > 0)
        BVC_HIP(ctx, hipMemcpy2DAsync(line_start, (size_t)(P.n_pos + 1) * 4, P.line_start, (size_t)P.line_stride * 4, (size_t)(P.n_pos + 1) * 4,
                                      (size_t)P.n_batches, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP(ctx, wait_stream(ctx));
    return BVC_OK;
}

// What a finish call delivers besides entry_off and tally, and which of the forms it is.  All (bvc_pileup_finish): the entries of every
// position.  Called (bvc_pileup_finish_called[_stats]): the entries of the called positions only, compacted on the device into called_off
// / entries / samples (called_cap = room in the two).  CalledText (bvc_pileup_finish_called_text): no entries or samples come down at all
// -- the tile's columns and records stay on the device for bvc_pileup_sample_text / _bgzf.  stats (Called: optional, CalledText:
// required): the called positions' rank sums and strand counts too, computed where the entries lie and delivered with the records.
enum class Finish { All, Called, CalledText };
struct FinishOut {
    int64_t *called_off = nullptr;
    int64_t called_cap = 0;
    bvc_pileup_entry *entries = nullptr;
    int32_t *samples = nullptr;
    bvc_pileup_indel *indels = nullptr;
    char *indel_text = nullptr;
    bvc_site_result *results = nullptr;
    bvc_group_result *grp_results = nullptr;
    bvc_site_stats *stats = nullptr;
};

static int pileup_finish_impl(bvc_ctx *ctx, Finish mode, const int8_t *ref_base, double min_af, const uint8_t carry_in[5],
                              uint8_t carry_out[5], const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                              int64_t *entry_off, int32_t *tally, const FinishOut &out)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState &pile = ctx->pile;
    PileupState::Tile &tile = pile.tile;
    const bool called_only = mode == Finish::Called, for_text = mode == Finish::CalledText;
    const bvc_site_stats *const stats = out.stats;
    if (!tile.begun) return fail(ctx, BVC_ERR_ARG, "bvc_pileup_finish without a bvc_pileup_begin that returned BVC_OK");
    if (tile.on_device_text && tile.indels > 0 && !out.indel_text) return fail(ctx, BVC_ERR_ARG, "indel_text is needed: the tile's text is on the device only");
    tile.begun = false;
    PileupTile &P = tile.P;
    const int64_t T = P.n_pos, n_e = tile.entries, n_o = tile.obs, n_i = tile.indels, n_it = tile.indel_bytes;
    if (!carry_in || !carry_out || !entry_off) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (T > 0 && (!ref_base || !tally || !out.results)) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if ((n_e > 0 && !called_only && !for_text && (!out.entries || !out.samples)) || (n_i > 0 && !out.indels)) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (called_only && (out.called_cap < 0 || (out.called_cap > 0 && (!out.entries || !out.samples)))) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (n_groups < 0 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 0..32");
    if (n_groups > 0 && (!out.grp_results || n_samples < 0 || (n_samples > 0 && !group_of_sample))) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    int8_t *d_ref; bvc_site_result *d_res; uint8_t *d_g, *d_itext; bvc_group_result *d_gres; int64_t *d_called_off; bvc_site_stats *d_stats;
    int rc = carve(ctx, pile.out, 256, [&](Layout &L) {
        P.entries = L.take<bvc_pileup_entry>((size_t)n_e, 16);
        P.samples = L.take<int32_t>((size_t)n_e, 16);
        P.obs_base = L.take<int8_t>((size_t)n_o, 16);
        P.obs_qual = L.take<int8_t>((size_t)n_o, 16);
        P.obs_label = L.take<uint8_t>((size_t)(n_groups ? n_o : 0), 16);
        P.indels = L.take<bvc_pileup_indel>((size_t)n_i, 16);
        d_ref = L.take<int8_t>((size_t)T, 16);
        d_res = L.take<bvc_site_result>((size_t)T);
        d_g = L.take<uint8_t>((size_t)(n_groups ? n_samples : 0), 16);
        d_gres = L.take<bvc_group_result>((size_t)T * (size_t)n_groups);
        d_itext = L.take<uint8_t>((size_t)(out.indel_text ? n_it : 0), 16);
        d_called_off = L.take<int64_t>(called_only ? (size_t)(T + 1) : 0);
        d_stats = L.take<bvc_site_stats>(stats ? (size_t)T : 0);
    });
    if (rc != BVC_OK) return rc;
    P.indel_cap = (uint32_t)n_i;
    P.group_of_sample = d_g; P.n_samples = n_groups ? n_samples : 0; P.n_groups = n_groups;
    const uint32_t cin = (uint32_t)(carry_in[0] & 7u) | ((uint32_t)(carry_in[4] & 1u) << 3) | 0x80u | ((uint32_t)carry_in[1] << 8) |
                         ((uint32_t)carry_in[2] << 16) | ((uint32_t)carry_in[3] << 24);
    uint32_t cout = cin;
    PinIO io(ctx);
    rc = io.reserve((size_t)T + (size_t)(n_groups > 0 ? n_samples : 0) + 1024,
                    (size_t)T * (sizeof(bvc_site_result) + 32 * 4 + 8 + (size_t)n_groups * sizeof(bvc_group_result)) +
                        (size_t)(called_only || for_text ? 0 : n_e) * (sizeof(bvc_pileup_entry) + 4) + (called_only ? (size_t)(T + 1) * 8 : 0) +
                        (size_t)n_i * sizeof(bvc_pileup_indel) + (size_t)n_it + (stats ? (size_t)T * sizeof(bvc_site_stats) : 0) + 4096);
    if (rc != BVC_OK) return rc;
    if (T > 0) {
        BVC_HIP_D(ctx, io.h2d(d_ref, ref_base, (size_t)T));
        // the label vector goes up in front of the write pass: that pass turns it into one label byte per observation (obs_label)
        if (n_groups > 0 && n_samples > 0) BVC_HIP_D(ctx, io.h2d(d_g, group_of_sample, (size_t)n_samples));
        if ((int64_t)P.n_pos * P.n_batches > 0) BVC_HIP_D(ctx, launch_pileup_write(ctx->stream, P, cin));
        if (n_groups > 0)
            rc = run_csr_labels_device(ctx, T, P.obs_off, reinterpret_cast<const uint8_t *>(P.obs_base),
                                       reinterpret_cast<const uint8_t *>(P.obs_qual), P.obs_label, d_ref, min_af, n_groups, d_res, d_gres);
        else
            rc = run_csr_device(ctx, T, P.obs_off, P.obs_base, P.obs_qual, d_ref, min_af, nullptr, nullptr, d_res);
        if (rc == BVC_OK) rc = join_side(ctx);
        if (rc != BVC_OK) return drain_on_error(ctx, rc);
        if (stats) BVC_HIP_D(ctx, launch_site_stats(ctx->ls, ctx->stream, T, P.entry_off, P.entries, d_ref, d_res, d_stats));
        BVC_HIP_D(ctx, io.d2h(out.results, d_res, (size_t)T * sizeof(bvc_site_result)));
        if (stats) BVC_HIP_D(ctx, io.d2h(out.stats, d_stats, (size_t)T * sizeof(bvc_site_stats)));
        if (n_groups > 0)
            BVC_HIP_D(ctx, io.d2h(out.grp_results, d_gres, (size_t)T * (size_t)n_groups * sizeof(bvc_group_result)));
        BVC_HIP_D(ctx, io.d2h(tally, P.tally, (size_t)T * 32 * 4));
        if (n_e && !called_only && !for_text) {
            BVC_HIP_D(ctx, io.d2h(out.entries, P.entries, (size_t)n_e * sizeof(bvc_pileup_entry)));
            BVC_HIP_D(ctx, io.d2h(out.samples, P.samples, (size_t)n_e * 4));
        }
        if (called_only) {
            BVC_HIP_D(ctx, launch_called_scan(ctx->stream, P, d_res, d_called_off));
            BVC_HIP_D(ctx, io.d2h(out.called_off, d_called_off, (size_t)(T + 1) * 8));
        }
        if (n_i && out.indel_text) {
            BVC_HIP_D(ctx, launch_indel_text(ctx->stream, P, d_itext, (uint32_t)n_it, P.status + 5));
            if (n_it) BVC_HIP_D(ctx, io.d2h(out.indel_text, d_itext, (size_t)n_it));
        }
        if (n_i) BVC_HIP_D(ctx, io.d2h(out.indels, P.indels, (size_t)n_i * sizeof(bvc_pileup_indel)));
        if ((int64_t)P.n_pos * P.n_batches > 0) BVC_HIP_D(ctx, io.d2h(&cout, P.status + 3, 4));
    }
    BVC_HIP_D(ctx, io.d2h(entry_off, P.entry_off, (size_t)(T + 1) * 8));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    if (called_only && T == 0) out.called_off[0] = 0;
    if (called_only && T > 0 && out.called_off[T] > 0) {
        // the second trip: the called positions' entries, gathered on the device (typically a few per cent of the tile's)
        const int64_t n_c = out.called_off[T];
        if (n_c > out.called_cap) return fail(ctx, BVC_ERR_ARG, "called_cap is smaller than the entries of the called positions (n_entries of the begin call always suffices)");
        bvc_pileup_entry *d_ce; int32_t *d_cs;
        rc = carve(ctx, pile.called, 0, [&](Layout &L) {
            d_ce = L.take<bvc_pileup_entry>((size_t)n_c);
            d_cs = L.take<int32_t>((size_t)n_c);
        });
        if (rc != BVC_OK) return rc;
        io.down_used = 0;
        rc = io.reserve(0, (size_t)n_c * (sizeof(bvc_pileup_entry) + 4) + 4096);
        if (rc != BVC_OK) return rc;
        BVC_HIP_D(ctx, launch_called_gather(ctx->stream, P, d_called_off, d_ce, d_cs));
        BVC_HIP_D(ctx, io.d2h(out.entries, d_ce, (size_t)n_c * sizeof(bvc_pileup_entry)));
        BVC_HIP_D(ctx, io.d2h(out.samples, d_cs, (size_t)n_c * 4));
        BVC_HIP_D(ctx, wait_stream(ctx));
        io.deliver();
    }
    carry_out[0] = (uint8_t)(cout & 7u); carry_out[1] = (uint8_t)(cout >> 8); carry_out[2] = (uint8_t)(cout >> 16);
    carry_out[3] = (uint8_t)(cout >> 24); carry_out[4] = (uint8_t)((cout >> 3) & 1u);
    if (for_text) {
        tile.d_ref = d_ref; tile.d_res = d_res;
        tile.h_entry_off.assign(entry_off, entry_off + T + 1);
        tile.h_called.resize((size_t)T);
        for (int64_t t = 0; t < T; ++t) tile.h_called[(size_t)t] = out.results[t].called;
        tile.text_ready = true;
    }
    return BVC_OK;
}

int bvc_pileup_finish(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                      const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                      int64_t *entry_off, int32_t *tally, bvc_pileup_entry *entries, int32_t *samples,
                      bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results, bvc_group_result *grp_results)
{
    FinishOut out;
    out.entries = entries; out.samples = samples; out.indels = indels; out.indel_text = indel_text;
    out.results = results; out.grp_results = grp_results;
    return pileup_finish_impl(ctx, Finish::All, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, out);
}

int bvc_pileup_finish_called(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                             const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                             int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                             int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                             bvc_group_result *grp_results)
{
    if (ctx && !called_off) return fail(ctx, BVC_ERR_ARG, "null pointer");
    FinishOut out;
    out.called_off = called_off; out.called_cap = called_cap; out.entries = entries; out.samples = samples;
    out.indels = indels; out.indel_text = indel_text; out.results = results; out.grp_results = grp_results;
    return pileup_finish_impl(ctx, Finish::Called, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, out);
}

int bvc_pileup_finish_called_stats(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                                   const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                                   int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                                   int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                                   bvc_group_result *grp_results, bvc_site_stats *stats)
{
    if (ctx && !called_off) return fail(ctx, BVC_ERR_ARG, "null pointer");
    FinishOut out;
    out.called_off = called_off; out.called_cap = called_cap; out.entries = entries; out.samples = samples;
    out.indels = indels; out.indel_text = indel_text; out.results = results; out.grp_results = grp_results; out.stats = stats;
    return pileup_finish_impl(ctx, Finish::Called, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, out);
}

int bvc_pileup_finish_called_text(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                                  const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                                  int64_t *entry_off, int32_t *tally, bvc_pileup_indel *indels, char *indel_text,
                                  bvc_site_result *results, bvc_group_result *grp_results, bvc_site_stats *stats)
{
    if (ctx && !stats) return fail(ctx, BVC_ERR_ARG, "null pointer");
    FinishOut out;
    out.indels = indels; out.indel_text = indel_text; out.results = results; out.grp_results = grp_results; out.stats = stats;
    return pileup_finish_impl(ctx, Finish::CalledText, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, out);
}

// The called positions' sample columns of the tile that bvc_pileup_finish_called_text left, formatted into the context's device memory
// on the stream: d_toff [T + 1], d_tlen [T], d_text [need] (need = the sum of their slots).
static int pileup_sample_text_device(bvc_ctx *ctx, int64_t n_samples, int64_t need, int64_t **d_toff, int64_t **d_tlen, char **d_text)
{
    PileupState &pile = ctx->pile;
    const PileupState::Tile &tile = pile.tile;
    const PileupTile &P = tile.P;
    const int64_t T = P.n_pos;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    int rc = vcf_lut_device(ctx);
    if (rc != BVC_OK) return rc;
    char *d_scr;
    rc = carve(ctx, pile.vtext, 256, [&](Layout &L) {
        *d_toff = L.take<int64_t>((size_t)T + 1);
        *d_tlen = L.take<int64_t>((size_t)T);
        *d_text = L.take<char>((size_t)need, 16);
        d_scr = L.take<char>(vcf_samples_scratch_bytes(T));
    });
    if (rc != BVC_OK) return rc;
    const VcfSamplesScratch scr = vcf_samples_scratch(d_scr, T);
    BVC_HIP_D(ctx, launch_vcf_samples_plan(ctx->stream, T, P.entry_off, P.samples, tile.d_res, n_samples, *d_toff, *d_tlen, scr));
    BVC_HIP_D(ctx, launch_vcf_samples(ctx->stream, T, P.entry_off, P.entries, P.samples, tile.d_ref, tile.d_res, n_samples, *d_toff, scr,
                                      ctx->d_vcf_lut.p, *d_text, need));
    return BVC_OK;
}

// bvc_pileup_sample_text (deflate = false: out / cap / off are text / text_cap / text_off) and bvc_pileup_sample_bgzf (deflate = true:
// comp / comp_cap / comp_off).  Both format the text on the device; the first brings it down with its offsets and lengths (one wait),
// the second deflates it there and brings down the offsets and lengths, then the packed blocks (two waits).
static int pileup_sample_impl(bvc_ctx *ctx, bool deflate, int64_t n_samples, void *out, int64_t cap, int64_t *off, int64_t *text_len)
{
    if (!ctx) return BVC_ERR_ARG;
    const PileupState::Tile &tile = ctx->pile.tile;
    if (!tile.text_ready)
        return fail(ctx, BVC_ERR_ARG, deflate ? "bvc_pileup_sample_bgzf without the tile of a bvc_pileup_finish_called_text"
                                              : "bvc_pileup_sample_text without the tile of a bvc_pileup_finish_called_text");
    if (n_samples < 0) return fail(ctx, BVC_ERR_ARG, "n_samples < 0 or text_cap < 0");
    if (cap < 0) return fail(ctx, BVC_ERR_ARG, deflate ? "n_samples < 0 or comp_cap < 0" : "n_samples < 0 or text_cap < 0");
    const int64_t T = tile.P.n_pos;
    if (!off || (T > 0 && !text_len) || (cap > 0 && !out)) return fail(ctx, BVC_ERR_ARG, "null pointer");
    // the needs from what the finish call delivered -- the sum of the called positions' slots, and of the bounds of their blocks (a
    // position's text is at most its slot): a buffer that is too small costs no launch and leaves the tile as it is
    std::vector<int64_t> slot((size_t)T);
    int64_t need_text = 0, need_comp = 0;
    for (int64_t t = 0; t < T; ++t) {
        slot[(size_t)t] = tile.h_called[(size_t)t] ? bvc_vcf_samples_slot(n_samples, tile.h_entry_off[(size_t)t + 1] - tile.h_entry_off[(size_t)t]) : 0;
        need_text += slot[(size_t)t];
        need_comp += bvc_bgzf_bound(slot[(size_t)t]);
    }
    if (deflate && need_comp > cap) return fail_cap(ctx, "comp_cap", cap, "the bounds of the pieces", need_comp);
    if (!deflate && need_text > cap) return fail_cap(ctx, "text_cap", cap, "the called positions' slots", need_text);
    if (T == 0) { off[0] = 0; return BVC_OK; }
    int64_t *d_toff, *d_tlen; char *d_text;
    int rc = pileup_sample_text_device(ctx, n_samples, need_text, &d_toff, &d_tlen, &d_text);
    if (rc != BVC_OK) return rc;
    uint8_t *d_comp = nullptr; int64_t *d_coff = nullptr;
    if (deflate) {
        rc = carve(ctx, ctx->d_bgzf_io, 256, [&](Layout &L) {
            d_comp = L.take<uint8_t>((size_t)need_comp);
            d_coff = L.take<int64_t>((size_t)T + 1);
        });
        if (rc != BVC_OK) return rc;
    }
    PinIO io(ctx);
    rc = io.reserve(deflate ? ((size_t)T + 1) * 8 + 64 : 0, (2 * (size_t)T + 1) * 8 + 1024);
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, io.d2h(text_len, d_tlen, (size_t)T * 8));
    if (deflate) {
        // position t's piece: its text_len bytes at text_off[t] of the text
        rc = bgzf_deflate_device(ctx, io, T, reinterpret_cast<const uint8_t *>(d_text), d_toff, d_tlen, slot.data(), d_comp, need_comp, d_coff, false);
        return rc == BVC_OK ? bgzf_blocks_down(ctx, io, T, d_comp, d_coff, static_cast<uint8_t *>(out), off) : rc;
    }
    // (straight into the caller's memory: a DMA where that is bvc_host_alloc memory)
    if (need_text) BVC_HIP_D(ctx, hipMemcpyAsync(out, d_text, (size_t)need_text, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, io.d2h(off, d_toff, ((size_t)T + 1) * 8));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    return BVC_OK;
}

int bvc_pileup_sample_text(bvc_ctx *ctx, int64_t n_samples, char *text, int64_t text_cap, int64_t *text_off, int64_t *text_len)
{
    return pileup_sample_impl(ctx, false, n_samples, text, text_cap, text_off, text_len);
}

int bvc_pileup_sample_bgzf(bvc_ctx *ctx, int64_t n_samples, uint8_t *comp, int64_t comp_cap, int64_t *comp_off, int64_t *text_len)
{
    return pileup_sample_impl(ctx, true, n_samples, comp, comp_cap, comp_off, text_len);
}

}  // extern "C"
