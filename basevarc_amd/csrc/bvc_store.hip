// bvc_store.hip -- temp batches kept on the device (include/bvc_store.h): the store's bookkeeping, the two ways a batch gets into it
// (bvc_store_put from host memory, bvc_bam_pileup_bgzf_store straight from phase 1's kernels), and bvc_pileup_begin_store, which gathers
// a tile of positions from all kept batches (store_kernel.hip) and begins it as bvc_pileup_begin_bin begins one (bvc_pileup.hip).
#include <mutex>

#include "bvc_ctx.h"
#include "../../include/bvc_store.h"

// A store is no part of a context: its bookkeeping is under its mutex, its device memory is its own.
struct bvc_store {
    int device = -1;
    int32_t n_positions = 0, n_batches = 0;
    int64_t budget = 0;
    mutable std::mutex mu;
    enum State : uint8_t { Empty, Busy, Kept };      // Busy: a put has reserved the batch and is filling it
    struct Batch {
        char *p = nullptr;                           // one allocation: the rec_start row, then (from a 16-byte boundary) the records
        int64_t bytes = 0, alloc = 0;                // the records' bytes; the allocation's
        int32_t n_in_batch = 0;
        State state = Empty;
    };
    std::vector<Batch> batches;
    int64_t used = 0;                                // the allocations of the batches that are Busy or Kept
    unsigned long long *d_cum = nullptr;             // [n_positions + 1]: the sum over the kept batches of rec_start
    bool sealed = false;
    std::vector<int64_t> cum;                        // d_cum on the host, from bvc_store_seal
    char *d_table = nullptr;                         // from bvc_store_seal: StoreBatch [n_batches], sample0 [n_batches], n_in_batch [n_batches]
    size_t row_bytes() const { return (((size_t)n_positions + 1) * 4 + 15) & ~(size_t)15; }
    uint32_t *row_of(const Batch &b) const { return reinterpret_cast<uint32_t *>(b.p); }
    uint8_t *records_of(const Batch &b) const { return reinterpret_cast<uint8_t *>(b.p) + row_bytes(); }
    const StoreBatch *d_batches() const { return reinterpret_cast<const StoreBatch *>(d_table); }
    const int32_t *d_sample0() const { return reinterpret_cast<const int32_t *>(d_table + round256((size_t)n_batches * sizeof(StoreBatch))); }
    const int32_t *d_n_in_batch() const { return d_sample0() + round256((size_t)n_batches * 4) / 4; }
};

namespace {

int check_store(bvc_ctx *ctx, const bvc_store *st)
{
    if (!st) return fail(ctx, BVC_ERR_ARG, "null store");
    if (st->device != ctx->device) return fail(ctx, BVC_ERR_ARG, "the store lies on another device than the context");
    return BVC_OK;
}

// Reserves batch `batch` for a put of records_bytes bytes of records: the refusals, the budget, the allocation.  BVC_OK: the batch is Busy
// and counted; commit() or release() must follow.
int reserve_batch(bvc_ctx *ctx, bvc_store *st, int32_t batch, int32_t n_in_batch, int64_t records_bytes)
{
    if (batch < 0 || batch >= st->n_batches) return fail(ctx, BVC_ERR_ARG, "batch index outside the store");
    if (n_in_batch < 0 || records_bytes < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (records_bytes > (int64_t)0xFFFFFF00u) return fail(ctx, BVC_ERR_ARG, "the records exceed 0xFFFFFF00 bytes (split the positions)");
    bvc_store::Batch &B = st->batches[(size_t)batch];
    const int64_t alloc = (int64_t)st->row_bytes() + (records_bytes > 0 ? records_bytes : 16);
    {
        std::lock_guard<std::mutex> g(st->mu);
        if (st->sealed) return fail(ctx, BVC_ERR_ARG, "the store is sealed: no batch can be put any more");
        if (B.state != bvc_store::Empty) return fail(ctx, BVC_ERR_ARG, "the batch has been put already");
        if (st->budget > 0 && st->used + alloc > st->budget) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "the store's budget is %lld bytes: %lld are in use and the batch takes %lld", (long long)st->budget,
                          (long long)st->used, (long long)alloc);
            return fail(ctx, BVC_ERR_ALLOC, msg);
        }
        B.state = bvc_store::Busy;
        st->used += alloc;
    }
    B.bytes = records_bytes; B.alloc = alloc; B.n_in_batch = n_in_batch;
    if (hipMalloc(reinterpret_cast<void **>(&B.p), (size_t)alloc) != hipSuccess) {
        (void)hipGetLastError();
        B.p = nullptr;
        std::lock_guard<std::mutex> g(st->mu);
        B.state = bvc_store::Empty;
        st->used -= alloc;
        return fail(ctx, BVC_ERR_ALLOC, "the device has no room for the batch");
    }
    return BVC_OK;
}

// Gives a reserved batch back: nothing of it was added to the cumulative sizes.
void release_batch(bvc_ctx *ctx, bvc_store *st, int32_t batch)
{
    bvc_store::Batch &B = st->batches[(size_t)batch];
    (void)wait_stream(ctx);                          // (whatever was enqueued on its memory)
    if (B.p) (void)hipFree(B.p);
    B.p = nullptr;
    std::lock_guard<std::mutex> g(st->mu);
    st->used -= B.alloc;
    B.bytes = 0; B.alloc = 0;
    B.state = bvc_store::Empty;
}

// The batch's row and records are on the device (enqueued on the context's stream or complete): its row is added to the cumulative sizes
// and the batch is Kept when the call returns.
int commit_batch(bvc_ctx *ctx, bvc_store *st, int32_t batch)
{
    bvc_store::Batch &B = st->batches[(size_t)batch];
    hipError_t e = launch_store_cum(ctx->stream, st->row_of(B), st->n_positions + 1, st->d_cum);
    if (e == hipSuccess) e = wait_stream(ctx);
    if (e != hipSuccess) {
        release_batch(ctx, st, batch);
        return drain_on_error(ctx, fail(ctx, BVC_ERR_DEVICE, "the batch's cumulative sizes", e));
    }
    std::lock_guard<std::mutex> g(st->mu);
    B.state = bvc_store::Kept;
    return BVC_OK;
}

struct StoreSink final : BatchSink {
    bvc_store *st;
    int32_t batch, n_in_batch;
    bool reserved = false;
    StoreSink(bvc_store *s, int32_t b, int32_t n) : st(s), batch(b), n_in_batch(n) {}
    int reserve(bvc_ctx *ctx, int64_t records_bytes, uint8_t **d_records, uint32_t **d_rec_start) override
    {
        const int rc = reserve_batch(ctx, st, batch, n_in_batch, records_bytes);
        if (rc != BVC_OK) return rc;
        reserved = true;
        const bvc_store::Batch &B = st->batches[(size_t)batch];
        *d_records = st->records_of(B); *d_rec_start = st->row_of(B);
        return BVC_OK;
    }
};

}  // namespace

extern "C" {

int bvc_store_create(bvc_store **out, int device, int32_t n_positions, int32_t n_batches, int64_t byte_budget)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    if (n_positions < 0 || n_batches < 0 || n_positions > (int32_t)(0x7FFFFFFF / 64)) return BVC_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return BVC_ERR_DEVICE; }
    bvc_store *st = new bvc_store;
    st->device = device; st->n_positions = n_positions; st->n_batches = n_batches; st->budget = byte_budget > 0 ? byte_budget : 0;
    st->batches.resize((size_t)n_batches);
    const size_t cum_bytes = ((size_t)n_positions + 1) * 8;
    if (hipMalloc(reinterpret_cast<void **>(&st->d_cum), cum_bytes) != hipSuccess || hipMemset(st->d_cum, 0, cum_bytes) != hipSuccess) {
        (void)hipGetLastError();
        bvc_store_destroy(st);
        return BVC_ERR_ALLOC;
    }
    *out = st;
    return BVC_OK;
}

void bvc_store_destroy(bvc_store *st)
{
    if (!st) return;
    (void)hipSetDevice(st->device);
    for (auto &B : st->batches) if (B.p) (void)hipFree(B.p);
    if (st->d_cum) (void)hipFree(st->d_cum);
    if (st->d_table) (void)hipFree(st->d_table);
    delete st;
}

int bvc_store_put(bvc_ctx *ctx, bvc_store *st, int32_t batch, int32_t n_in_batch, const uint8_t *records, int64_t records_bytes,
                  const uint32_t *rec_start)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_store(ctx, st);
    if (rc != BVC_OK) return rc;
    if (records_bytes < 0) return fail(ctx, BVC_ERR_ARG, "negative size");
    if (!rec_start || (records_bytes > 0 && !records)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    rc = check_records(ctx, records, rec_start, st->n_positions, records_bytes);
    if (rc != BVC_OK) return rc;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    rc = reserve_batch(ctx, st, batch, n_in_batch, records_bytes);
    if (rc != BVC_OK) return rc;
    const bvc_store::Batch &B = st->batches[(size_t)batch];
    hipError_t e = hipMemcpyAsync(st->row_of(B), rec_start, ((size_t)st->n_positions + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && records_bytes) e = hipMemcpyAsync(st->records_of(B), records, (size_t)records_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        release_batch(ctx, st, batch);
        return drain_on_error(ctx, fail(ctx, BVC_ERR_DEVICE, "the batch's upload", e));
    }
    return commit_batch(ctx, st, batch);
}

int bvc_bam_pileup_bgzf_store(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                              int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                              const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                              int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                              bvc_store *st, int32_t batch, int64_t *records_bytes, uint32_t *sample_status)
{
    if (!ctx) return BVC_ERR_ARG;
    if (records_bytes) *records_bytes = 0;
    int rc = check_store(ctx, st);
    if (rc != BVC_OK) return rc;
    if (n_positions != st->n_positions) return fail(ctx, BVC_ERR_ARG, "n_positions is not the store's");
    if (batch < 0 || batch >= st->n_batches) return fail(ctx, BVC_ERR_ARG, "batch index outside the store");
    {
        // (refused before the kernels run; reserve_batch decides again, under the same mutex, once the size is known)
        std::lock_guard<std::mutex> g(st->mu);
        if (st->sealed) return fail(ctx, BVC_ERR_ARG, "the store is sealed: no batch can be put any more");
        if (st->batches[(size_t)batch].state != bvc_store::Empty) return fail(ctx, BVC_ERR_ARG, "the batch has been put already");
    }
    StoreSink sink(st, batch, n_samples);
    rc = bam_pileup_bgzf_call(false, ctx, n_samples, comp, comp_bytes, blocks, n_blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0,
                              min_mapq, n_positions, positions, rg_s, refseq, refseq_len, nullptr, 0, records_bytes, nullptr, sample_status, &sink);
    if (rc != BVC_OK) {
        if (sink.reserved) {
            const std::string why = ctx->err;        // (release_batch waits, which may not fail quietly)
            release_batch(ctx, st, batch);
            ctx->err = why;
        }
        return rc;
    }
    return commit_batch(ctx, st, batch);
}

int bvc_store_get(bvc_ctx *ctx, const bvc_store *st, int32_t batch, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                  uint32_t *rec_start)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_store(ctx, st);
    if (rc != BVC_OK) return rc;
    if (!records_needed) return fail(ctx, BVC_ERR_ARG, "null pointer");
    *records_needed = 0;
    if (batch < 0 || batch >= st->n_batches) return fail(ctx, BVC_ERR_ARG, "batch index outside the store");
    const bvc_store::Batch &B = st->batches[(size_t)batch];
    {
        std::lock_guard<std::mutex> g(st->mu);
        if (B.state != bvc_store::Kept) return fail(ctx, BVC_ERR_ARG, "the batch has not been put");
    }
    *records_needed = B.bytes;
    if (!records && !rec_start) return BVC_OK;
    if (records_cap < B.bytes || (B.bytes > 0 && !records) || !rec_start) return fail(ctx, BVC_ERR_ARG, "records buffer too small / null rec_start");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    BVC_HIP_D(ctx, hipMemcpyAsync(rec_start, st->row_of(B), ((size_t)st->n_positions + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (B.bytes) BVC_HIP_D(ctx, hipMemcpyAsync(records, st->records_of(B), (size_t)B.bytes, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    return BVC_OK;
}

int bvc_store_seal(bvc_ctx *ctx, bvc_store *st)
{
    if (!ctx) return BVC_ERR_ARG;
    int rc = check_store(ctx, st);
    if (rc != BVC_OK) return rc;
    std::lock_guard<std::mutex> g(st->mu);
    if (st->sealed) return BVC_OK;
    const size_t nb = (size_t)st->n_batches, np = (size_t)st->n_positions;
    for (size_t b = 0; b < nb; ++b)
        if (st->batches[b].state != bvc_store::Kept) {
            const std::string what = "batch " + std::to_string(b) + " has not been put: every batch must be, before the store is sealed";
            return fail(ctx, BVC_ERR_ARG, what.c_str());
        }
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    // the batches' table as the gather kernels read it, with the batches' first samples and sizes behind it
    const size_t off_s0 = round256(nb * sizeof(StoreBatch)), off_nib = off_s0 + round256(nb * 4), bytes = off_nib + round256(nb * 4) + 256;
    std::vector<char> table(bytes, 0);
    int64_t s0 = 0;
    for (size_t b = 0; b < nb; ++b) {
        const bvc_store::Batch &B = st->batches[b];
        StoreBatch row = {(uint64_t)reinterpret_cast<uintptr_t>(st->row_of(B)), (uint64_t)reinterpret_cast<uintptr_t>(st->records_of(B)), (uint64_t)B.bytes};
        std::memcpy(&table[b * sizeof(StoreBatch)], &row, sizeof row);
        if (s0 > (int64_t)0x7FFFFFFF - B.n_in_batch) return fail(ctx, BVC_ERR_ARG, "more than 2^31 samples in the store");
        const int32_t first = (int32_t)s0;
        std::memcpy(&table[off_s0 + b * 4], &first, 4);
        std::memcpy(&table[off_nib + b * 4], &B.n_in_batch, 4);
        s0 += B.n_in_batch;
    }
    char *d_table = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_table), bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, BVC_ERR_ALLOC, "the device has no room for the store's table"); }
    std::vector<int64_t> cum(np + 1);
    hipError_t e = hipMemcpyAsync(d_table, table.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cum.data(), st->d_cum, (np + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = wait_stream(ctx);
    if (e != hipSuccess) {
        (void)hipFree(d_table);
        return drain_on_error(ctx, fail(ctx, BVC_ERR_DEVICE, "the store's table", e));
    }
    st->d_table = d_table;
    st->cum.swap(cum);
    st->sealed = true;
    return BVC_OK;
}

int bvc_store_tile(const bvc_store *st, int32_t t0, int32_t max_positions, int64_t max_bytes, int32_t *n_positions, int64_t *bytes)
{
    if (!st || !n_positions || !bytes) return BVC_ERR_ARG;
    *n_positions = 0; *bytes = 0;
    {
        std::lock_guard<std::mutex> g(st->mu);
        if (!st->sealed) return BVC_ERR_ARG;
    }
    if (t0 < 0 || t0 >= st->n_positions || max_positions < 1) return BVC_ERR_ARG;
    *n_positions = bvc_store_tile_fit(st->cum.data(), st->n_positions, st->n_batches, t0, max_positions, max_bytes, bytes);
    return BVC_OK;
}

int bvc_store_bytes(const bvc_store *st, int64_t *used, int64_t *budget)
{
    if (!st) return BVC_ERR_ARG;
    std::lock_guard<std::mutex> g(st->mu);
    if (used) *used = st->used;
    if (budget) *budget = st->budget;
    return BVC_OK;
}

int bvc_pileup_begin_store(bvc_ctx *ctx, const bvc_store *st, int32_t t0, int32_t n_positions, int64_t *n_entries, int64_t *n_indels,
                           int64_t *indel_text_bytes)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState::Tile &tile = ctx->pile.tile;
    tile = PileupState::Tile{};
    int rc = check_store(ctx, st);
    if (rc != BVC_OK) return rc;
    if (!n_entries || !n_indels || !indel_text_bytes) return fail(ctx, BVC_ERR_ARG, "bad argument");
    *n_entries = 0; *n_indels = 0; *indel_text_bytes = 0;
    {
        std::lock_guard<std::mutex> g(st->mu);
        if (!st->sealed) return fail(ctx, BVC_ERR_ARG, "the store is not sealed (bvc_store_seal)");
    }
    if (t0 < 0 || n_positions < 0 || n_positions > st->n_positions - t0) return fail(ctx, BVC_ERR_ARG, "positions outside the store");
    // the tile buffer: the slices and at most 15 bytes in front of each -- decided from the cumulative sizes, before anything is launched
    const int32_t n_batches = st->n_batches;
    const int64_t tile_cap = st->cum[(size_t)(t0 + n_positions)] - st->cum[(size_t)t0] + (int64_t)16 * n_batches;
    if (tile_cap > (int64_t)0xFFFFFF00u) return fail(ctx, BVC_ERR_ARG, "more than 0xFFFFFF00 bytes of records in one tile (use fewer positions)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nb = (size_t)n_batches;
    const int64_t n_rows = (int64_t)n_batches * n_positions;
    PileupTile &P = tile.P;
    uint32_t *d_rows; int32_t *d_s0, *d_nib;
    StorePlan plan;
    size_t clear = 0;
    rc = ensure(ctx, ctx->pile.text, (size_t)tile_cap + 64);
    if (rc == BVC_OK)
        rc = carve(ctx, ctx->pile.meta, 0, [&](Layout &L) {
            clear = carve_tile(L, P, n_batches, n_positions, 0, d_rows, d_s0, d_nib);
            plan.lo = L.take<uint32_t>(nb); plan.len = L.take<uint32_t>(nb); plan.dst = L.take<uint32_t>(nb);
            plan.first_item = L.take<uint32_t>(nb + 1); plan.used = L.take<unsigned long long>(1);
        });
    if (rc != BVC_OK) return rc;
    P.text = reinterpret_cast<const uint8_t *>(ctx->pile.text.p);
    P.bin = true;
    BVC_HIP_D(ctx, hipMemsetAsync(P.status, 0, clear, ctx->stream));     // status, totals, offsets of an empty tile, tallies
    unsigned long long used = 0;
    if (n_rows > 0) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_s0, st->d_sample0(), nb * 4, hipMemcpyDeviceToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_nib, st->d_n_in_batch(), nb * 4, hipMemcpyDeviceToDevice, ctx->stream));
        BVC_HIP_D(ctx, launch_store_gather(ctx->stream, st->d_batches(), n_batches, t0, n_positions, plan, reinterpret_cast<uint8_t *>(ctx->pile.text.p),
                                           tile_cap, d_rows));
        BVC_HIP_D(ctx, launch_pileup_count(ctx->stream, P));
        BVC_HIP_D(ctx, hipMemcpyAsync(&used, plan.used, sizeof used, hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = pileup_begin_verdict(ctx, true, n_entries, n_indels, indel_text_bytes);
    // the tile's records are on the device only: a finish call gathers its indel tokens' text there, and bvc_pileup_text delivers the tile
    tile.text_bytes = (int64_t)used;
    tile.on_device_text = true;
    return rc;
}

}  // extern "C"
