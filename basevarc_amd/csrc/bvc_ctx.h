// bvc_ctx.h -- the context of libbvc and what every family of entry points needs of it (not installed).  The C ABI of include/bvc.h
// is defined in bvc_context.hip (a context's life, streams, tuning, profile), bvc_lrt.hip (the two stages on tiles and ragged columns)
// and bvc_pileup.hip (BGZF blocks and temp-batch tiles).  One context = one gfx950 device + one HIP stream + device scratch.  No CPU
// fallback exists: every compute entry point launches the HIP kernels or fails with an error code.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvc_internal.h"

using namespace bvc;

// the helpers below are shared by the library's translation units, not exported by it
#pragma GCC visibility push(hidden)

// Device scratch of a context: grown by ensure(), freed with the context.
struct DevBuf {
    char *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// bvc_pileup_begin / bvc_pileup_begin_bgzf / bvc_pileup_finish: their device buffers and the tile between the calls.
struct PileupState {
    DevBuf text, meta, out, called;    // the tile's text, its line tables and counts, its parsed columns and records, the called entries
    // tiles inflated on the device (bvc_pileup_begin_bgzf): two text buffers (what a tile leaves of a batch is carried from one to the
    // other), the compressed bytes, what the calls left of every batch
    DevBuf pz_text[2], pz_comp;
    int pz_cur = 0;                    // the buffer that holds the leftovers
    std::vector<uint32_t> left_src, left_len;
    struct Tile {                      // what a begin call leaves for the finish call; every begin starts from Tile{}
        PileupTile P;
        bool begun = false;
        int64_t entries = 0, obs = 0, indels = 0;
        int64_t text_bytes = 0, indel_bytes = 0;
        bool on_device_text = false;
        // after bvc_pileup_finish_called_text: the tile's columns stay where they are for bvc_pileup_sample_text -- the reference bases
        // and records on the device, and on the host what sizes the text (every position's entries, which positions are called)
        bool text_ready = false;
        const int8_t *d_ref = nullptr;
        const bvc_site_result *d_res = nullptr;
        std::vector<int64_t> h_entry_off;
        std::vector<uint8_t> h_called;
    } tile;
    DevBuf vtext;                      // bvc_pileup_sample_text: the text, its offsets and lengths
};

struct bvc_ctx {
    int device = -1;
    hipStream_t stream = nullptr;      // the stream the entry points work on: own_stream until bvc_set_stream names another
    hipStream_t own_stream = nullptr;  // created with the context.  A BLOCKING stream: ordered against the device's default stream as the
                                       // default stream itself is (callers that prepare buffers there need no extra synchronisation), but the
                                       // streams of different contexts run side by side -- sixteen threads of the host program, each with
                                       // its context, were one queue when every context worked on the default stream
    hipEvent_t ev_wait = nullptr;      // blocking-sync event: the long waits of the pileup calls SLEEP on it (wait_stream) where
                                       // hipStreamSynchronize polls -- a host program with a thread per context on a CPU quota cannot afford that
    QualLut *d_lut = nullptr;
    // [sites][512] scratch between the two stages.  Overlap mode cycles through kRing buffers: with three, the
    // histogram pass of call i+1 waits only for the EM of call i-2 (long finished), never for the one running
    // beside it, so both streams run back to back.
    static constexpr int kRing = 4;
    DevBuf d_cnt[kRing];
    // overlap mode: stage 2 of call i runs on `side` while stage 1 of call i+1 streams on `stream`
    bool overlap = false;
    hipStream_t side = nullptr;        // stage 2 of even calls
    hipStream_t side_b = nullptr, side_c = nullptr;   // further stage-2 streams (two_em_streams below)
    unsigned side_flip = 0;
    int flip = 0;
    hipEvent_t ev_hist_done[kRing] = {};
    hipEvent_t ev_em_done[kRing] = {};
    bool em_pending[kRing] = {};
    DevBuf d_grp[kRing];               // [sites][groups + 1][512] in group mode
    // item-engine scratch of stage 2 (em_items.hip), one per ring buffer (the stage 2 of consecutive calls may run
    // side by side); the last one serves bvc_lrt_hist on the context's own stream
    DevBuf d_em[kRing + 1];
    DevBuf d_emg[kRing];               // the same for the (site, group) pseudo-sites of group calls
    uint32_t *d_sink = nullptr;        // 256 bytes: sink of the streaming-read measurement kernel; bvc_pack_dense's counter at byte 64
    DevBuf d_acc;                      // bvc_counts_add_dense*: a chunk's histograms, before they are added to the caller's counts
    DevBuf d_grp_labels;               // group mode: the call's group vector clamped to 0..n_groups (hist_kernel.hip)
    int64_t *d_grp_scratch = nullptr;  // group mode: "samples ordered by group" flag + column bounds (hist_kernel.hip)
    // staging for BVC_PTR_HOST calls: two sets, so that the upload of chunk i+1 (copy stream) runs under the kernels
    // of chunk i
    DevBuf d_stage[2];
    hipStream_t copy = nullptr;
    hipEvent_t ev_upload[2] = {nullptr, nullptr};
    hipEvent_t ev_set_free[2] = {nullptr, nullptr};   // ragged host calls: the kernels that read staging set k have finished
    PileupState pile;
    DevBuf d_vcf, d_vcf_lut;           // vcf_samples_kernel.hip: the plan's scratch (device-pointer calls); the 256 x 8 bytes of bvc_vcf_bp_lut
    DevBuf d_bgzf, d_bgzf_io;          // bgzf_deflate_kernel.hip: block tables, match rows, staged blocks; a call's staged pieces (host pointers), its packed blocks and comp_off
    DevBuf d_bam, d_bam_out;           // bam_pileup_kernel.hip: the read table, one tile's size matrix, the per-position sizes; a host-pointer call's records
    DevBuf d_bamz, d_bamz_out;         // bvc_bam_deflate.hip: a batch's records or lines and their rec_start row; the pieces' tables, the packed blocks, out_off
    int64_t bamz_kept = -1;            // >= 0: the packed bytes at the front of d_bamz_out that bvc_bam_pileup_deflate_fetch delivers
    // pinned host memory the pileup calls bounce their transfers through: a copy from or to pageable memory makes the calling thread
    // wait inside the runtime -- spinning -- for the whole transfer; from pinned memory it is a DMA the thread sleeps behind (wait_stream)
    char *h_up = nullptr, *h_down = nullptr;
    size_t up_cap = 0, down_cap = 0;
    LaunchState ls;                    // launch policy + one-time kernel setup of this context
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;   // free events
    struct Triple { hipEvent_t a, b, c, d; int64_t sites; };   // hist = a..b, EM = c..d
    std::vector<Triple> ev_pending;
    bvc_profile prof{};
    std::string err;
};

// The ring buffers of one call: [n_sites][512] counts, the [n_sites][n_groups + 1][512] group histograms (group calls)
// and the item-engine scratch of both (null when stage 2 does not use the engine).
struct RingSlot {
    uint32_t *counts = nullptr, *grp = nullptr;
    void *em = nullptr, *emg = nullptr;
};

inline int fail(bvc_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}

// BVC_ERR_ARG for an output buffer that is too small: "<name> is <cap> bytes, <what> need <need>".
inline int fail_cap(bvc_ctx *ctx, const char *name, int64_t cap, const char *what, int64_t need)
{
    char msg[160];
    std::snprintf(msg, sizeof msg, "%s is %lld bytes, %s need %lld", name, (long long)cap, what, (long long)need);
    return fail(ctx, BVC_ERR_ARG, msg);
}

// Waits for the context's stream without spinning: the thread sleeps until the event behind everything enqueued so far fires.
inline hipError_t wait_stream(bvc_ctx *ctx)
{
    hipError_t e = hipEventRecord(ctx->ev_wait, ctx->stream);
    return e == hipSuccess ? hipEventSynchronize(ctx->ev_wait) : e;
}

#define BVC_HIP(ctx, call)                                                         \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) return fail((ctx), BVC_ERR_DEVICE, #call, e__);     \
    } while (0)

// Every stream a context enqueues work on.
inline std::array<hipStream_t, 5> streams_of(const bvc_ctx *ctx) { return {ctx->stream, ctx->copy, ctx->side, ctx->side_b, ctx->side_c}; }

// Waits for every stream of the context (all of them, whatever one returns; the first error is the result): nothing of stage 2 is
// pending afterwards.
hipError_t sync_streams(bvc_ctx *ctx);

// A failed call must not leave an upload or a kernel running on the context's buffers: the next call may free or refill
// them, and stage 2 of what was already launched may still run on the side streams.  Returns `code`.
int drain_on_error(bvc_ctx *ctx, int code);

#define BVC_HIP_D(ctx, call)                                                                         \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return drain_on_error((ctx), fail((ctx), BVC_ERR_DEVICE, #call, e__)); \
    } while (0)

// Grows `buf` to `need` bytes (and a quarter more) after waiting for the context's stream and the copy stream; the new buffer is cleared.
int ensure(bvc_ctx *ctx, DevBuf &buf, size_t need);

// Grows `buf` to the slices of `list` (a function of a Layout &, bvc_internal.h) + `slack` bytes and carves it: the one list of take() calls runs
// once to size the buffer and once to hand out the pointers, so the two cannot disagree.
template <class List>
int carve(bvc_ctx *ctx, DevBuf &buf, size_t slack, List list)
{
    Layout size;
    list(size);
    const int rc = ensure(ctx, buf, size.at + slack);
    if (rc != BVC_OK) return rc;
    Layout slices{reinterpret_cast<uintptr_t>(buf.p)};
    list(slices);
    return BVC_OK;
}

// The pool of timing events (profiling, bvc_stream_read_ms).
hipEvent_t take_event(bvc_ctx *ctx);
void give_back(bvc_ctx *ctx, hipEvent_t e);
void give_back(bvc_ctx *ctx, bvc_ctx::Triple &t);
// Four timing events for one call, or none at all (never a partial set).
bool take_timing_events(bvc_ctx *ctx, bvc_ctx::Triple &t);
// Drains finished timing records into the running totals so that ev_pending stays bounded when the caller never
// asks for the profile.
void reap_timing(bvc_ctx *ctx, bool all);

// Make the context's stream wait for every stage-2 launch still running on the side stream.
inline int join_side(bvc_ctx *ctx)
{
    for (int b = 0; b < bvc_ctx::kRing; ++b)
        if (ctx->em_pending[b]) {
            BVC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_em_done[b], 0));
            ctx->em_pending[b] = false;
        }
    return BVC_OK;
}

// Grows a buffer that a stage 2 on a side stream may still be reading: the context's stream waits for the side streams first (ensure
// waits for the context's stream).
inline int ensure_joined(bvc_ctx *ctx, DevBuf &buf, size_t need)
{
    if (need > buf.cap) {
        const int rc = join_side(ctx);
        if (rc != BVC_OK) return rc;
    }
    return ensure(ctx, buf, need);
}

// Does [p, p + n) lie inside an allocation of bvc_host_alloc?  A transfer from / to it needs no bounce buffer.
bool in_pinned(const void *p, size_t n);

// Transfers of one call through the context's pinned buffers: h2d copies the caller's bytes into pinned memory and enqueues the DMA,
// d2h enqueues a DMA into pinned memory and deliver() -- after the stream has been waited for -- copies the bytes to the caller.
struct PinIO {
    bvc_ctx *ctx;
    size_t up_used = 0, down_used = 0;
    struct Out { void *dst; const char *src; size_t n; };
    std::vector<Out> outs;
    explicit PinIO(bvc_ctx *c) : ctx(c) {}
    static size_t al(size_t n) { return (n + 63) & ~(size_t)63; }
    int reserve(size_t up_bytes, size_t down_bytes)
    {
        auto grow = [&](char **buf, size_t *cap, size_t need) -> int {
            if (need <= *cap) return BVC_OK;
            if (*buf) {
                if (wait_stream(ctx) != hipSuccess) return fail(ctx, BVC_ERR_DEVICE, "wait before growing a pinned buffer");
                (void)hipHostFree(*buf);
                *buf = nullptr; *cap = 0;
            }
            const size_t want = need + need / 4 + 4096;
            if (hipHostMalloc(reinterpret_cast<void **>(buf), want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, BVC_ERR_ALLOC, "pinned host allocation failed");
            }
            *cap = want;
            return BVC_OK;
        };
        int rc = grow(&ctx->h_up, &ctx->up_cap, up_bytes);
        return rc == BVC_OK ? grow(&ctx->h_down, &ctx->down_cap, down_bytes) : rc;
    }
    hipError_t h2d(void *dev, const void *host, size_t n)
    {
        if (n == 0) return hipSuccess;
        if (in_pinned(host, n)) return hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, ctx->stream);
        if (up_used + n > ctx->up_cap) return hipErrorOutOfMemory;
        char *p = ctx->h_up + up_used;
        std::memcpy(p, host, n);
        up_used += al(n);
        return hipMemcpyAsync(dev, p, n, hipMemcpyHostToDevice, ctx->stream);
    }
    hipError_t d2h(void *host, const void *dev, size_t n)
    {
        if (n == 0) return hipSuccess;
        if (down_used + n > ctx->down_cap) return hipErrorOutOfMemory;
        char *p = ctx->h_down + down_used;
        down_used += al(n);
        outs.push_back(Out{host, p, n});
        return hipMemcpyAsync(p, dev, n, hipMemcpyDeviceToHost, ctx->stream);
    }
    void deliver() { for (auto const &o : outs) std::memcpy(o.dst, o.src, o.n); outs.clear(); }
};

inline int check_common(bvc_ctx *ctx, int64_t n_sites, const void *a, const void *b, const void *c, const void *d)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_sites < 0) return fail(ctx, BVC_ERR_ARG, "n_sites < 0");
    if (n_sites > 0 && (!a || !b || !c || !d)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_sites > (int64_t)0x7FFFFFFF / 64) return fail(ctx, BVC_ERR_ARG, "too many sites in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    return BVC_OK;
}

// check_common for rows of n_samples samples, row_stride bytes apart
inline int check_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const void *a, const void *b, const void *c,
                       const void *d)
{
    const int rc = check_common(ctx, n_sites, a, b, c, d);
    if (rc != BVC_OK) return rc;
    return n_samples >= 0 && row_stride >= n_samples ? BVC_OK : fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
}

// Host-pointer ragged calls: the chunking and the uploads index the observations with offsets[0..n_sites].
inline int check_offsets_host(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets)
{
    bool ok = offsets[0] == 0;
    for (int64_t s = 0; s < n_sites && ok; ++s) ok = offsets[s + 1] >= offsets[s];
    return ok ? BVC_OK : fail(ctx, BVC_ERR_ARG, "offsets must start at 0 and be non-decreasing");
}

inline int check_n_groups(bvc_ctx *ctx, int32_t n_groups)
{
    return n_groups >= 1 && n_groups <= BVC_MAX_GROUPS ? BVC_OK : fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
}

// The two stages on ragged columns in device memory (bvc_lrt.hip); bvc_pileup_finish runs them on the columns of its tile.
int run_csr_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                   const int8_t *ref_base, double min_af, const int8_t *comb, const uint8_t *n_comb,
                   bvc_site_result *results);
// group records from one label byte per observation; obs = the bases, or with quals == nullptr the packed bytes
int run_csr_labels_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals,
                          const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                          bvc_site_result *results, bvc_group_result *grp_results);

// bvc_bgzf.hip: pieces in device memory -> BGZF blocks in d_comp (device), comp_off [n_pieces + 1] in d_comp_off (device), all on the
// stream.  upper[i] >= piece i's length, on the host (the lengths themselves where it knows them): it sizes the launches and the scratch
// (ctx->d_bgzf).  io: the call's transfers, with (n_pieces + 1) * 8 + 64 bytes reserved going up.  wait_for_upload: for a caller that
// returns without a wait of its own behind this -- the block table has left the page-locked buffer before the kernels are launched.
int bgzf_deflate_device(bvc_ctx *ctx, PinIO &io, int64_t n_pieces, const uint8_t *d_data, const int64_t *d_off, const int64_t *d_len,
                        const int64_t *upper, uint8_t *d_comp, int64_t comp_cap, int64_t *d_comp_off, bool wait_for_upload);
// The tail of a call that delivers blocks to the host: comp_off [n_pieces + 1] comes down through io and is waited for and delivered (with
// whatever else io has coming down), then only the comp_off[n_pieces] packed bytes come straight into the caller's memory (a DMA where
// that is bvc_host_alloc memory), with a second wait.  io: (n_pieces + 1) * 8 + 64 bytes reserved coming down.
// comp_cap >= 0: a caller that could not size comp before -- where comp_off[n_pieces] exceeds it nothing more comes down and the call returns
// BVC_BAM_MORE (comp_off is written; the blocks stay where they are).
int bgzf_blocks_down(bvc_ctx *ctx, PinIO &io, int64_t n_pieces, const uint8_t *d_comp, const int64_t *d_comp_off, uint8_t *comp,
                     int64_t *comp_off, int64_t comp_cap = -1);

// bvc_pileup.hip, shared with bvc_store.hip (a tile gathered from kept batches is laid out, checked and begun as bvc_pileup_begin_bin's):
// the slices of a tile's meta buffer (returns the bytes from the status to the end of the tallies: what a begin call clears) ...
size_t carve_tile(Layout &L, PileupTile &P, int32_t n_batches, int32_t n_pos, size_t batch_pad, uint32_t *&line_start, int32_t *&sample0,
                  int32_t *&n_in_batch);
// ... what a begin call checks of a batch's row of binary records before a kernel indexes with it ...
int check_records(bvc_ctx *ctx, const uint8_t *records, const uint32_t *rs, int32_t n_positions, int64_t records_bytes);
// ... and the end of a begin call whose count pass is enqueued: the one wait for the status and the totals, the verdict on them, the
// tile marked begun.  *indel_text_bytes (may be null): the bytes of the tile's indel tokens
int pileup_begin_verdict(bvc_ctx *ctx, bool bin, int64_t *n_entries, int64_t *n_indels, int64_t *indel_text_bytes);

// bvc_bam.hip, shared with bvc_store.hip: where bvc_bam_pileup_bgzf's records go when they stay on the device.  reserve() is called between
// the call's two passes, once the size is known, and names the device memory the second pass writes (anything but BVC_OK ends the call with
// that code); the call returns BVC_OK with both complete on the device.
struct BatchSink {
    uint32_t *h_rec_start = nullptr;   // not null: rec_start [n_positions + 1] comes down to it with the call's first wait, before reserve()
    bool wait = true;                  // false: the call returns with its second pass enqueued on the context's stream, as a device-pointer call
    virtual int reserve(bvc_ctx *ctx, int64_t records_bytes, uint8_t **d_records, uint32_t **d_rec_start) = 0;
protected:
    ~BatchSink() = default;
};
// bvc_bam_pileup_bgzf (text = false) and bvc_bam_pileup_text_bgzf (text = true); sink: records, records_cap and rec_start are unused
int bam_pileup_bgzf_call(bool text, bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
                         int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end, const uint8_t *sample_eof, const int32_t *rid,
                         int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions, const int32_t *positions, int32_t rg_s,
                         const char *refseq, int64_t refseq_len, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                         uint32_t *rec_start, uint32_t *sample_status, BatchSink *sink = nullptr);

// bvc_bam.hip, shared with bvc_bam_counts.hip: a call's inputs (BamCall, bvc_internal.h) from the arguments every entry point has ...
inline BamCall bam_call(int32_t n_samples, const uint8_t *bam, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                        const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq, int32_t n_positions,
                        const int32_t *positions, int32_t rg_s, int64_t refseq_len)
{
    BamCall c;
    c.n_samples = n_samples; c.n_positions = n_positions; c.beg0 = beg0; c.end0 = end0; c.min_mapq = min_mapq; c.rg_s = rg_s;
    c.bam = bam; c.eof = sample_eof; c.off = sample_off; c.end = sample_end; c.rid = rid; c.pos = positions; c.bam_bytes = bam_bytes; c.refseq_len = refseq_len;
    return c;
}
// ... the way of a host-pointer call's inputs into the staging buffer: take() among the caller's own takes of one carve, then upload(),
// which enqueues on the context's stream the bulk (the BGZF bytes, else the inflated records) straight from the caller's memory, the
// arrays through io, and with blocks the inflate and the blocks' statuses on their way down (the call's first wait delivers them) ...
struct BamStage {
    BamCall c;                              // the call with bam and the sample and position arrays where the kernels read them
    uint32_t *d_status = nullptr;           // [n_samples]
    uint8_t *d_group = nullptr;             // [n_samples]: the labels (null without group_of_sample)
    std::vector<uint32_t> block_status;     // [n_blocks]
    // host: the caller's pointers; comp / blocks: its BGZF blocks (host.bam is then unused); group_of_sample may be null
    BamStage(const BamCall &host, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks, int64_t n_blocks,
             const uint8_t *group_of_sample = nullptr)
        : c(host), block_status((size_t)n_blocks), h(host), comp(comp), group(group_of_sample), blocks(blocks), comp_bytes(comp_bytes), n_blocks(n_blocks) {}
    void take(Layout &L);
    int upload(bvc_ctx *ctx, PinIO &io);
private:
    const BamCall h;
    const uint8_t *comp, *group;
    const bvc_bgzf_block *blocks;
    int64_t comp_bytes, n_blocks;
    uint8_t *u_comp = nullptr, *u_bam = nullptr, *u_eof = nullptr; bvc_bgzf_block *u_blk = nullptr; uint32_t *u_bst = nullptr;
    int64_t *u_off = nullptr, *u_end = nullptr; int32_t *u_rid = nullptr, *u_pos = nullptr;
};
// ... the checks made before anything of the device is touched (strict: the positions ascend strictly; else they may repeat) ...
int check_sizes(bvc_ctx *ctx, int32_t n_samples, int64_t bam_bytes, int32_t n_positions, int64_t refseq_len, int64_t records_cap);
int check_host_arrays(bvc_ctx *ctx, int32_t n_samples, const int64_t *sample_off, const int64_t *sample_end, int64_t bam_bytes, int32_t n_positions,
                      const int32_t *positions, bool strict = true);
int check_blocks(bvc_ctx *ctx, const bvc_bgzf_block *blocks, int64_t n_blocks, int64_t comp_bytes, int64_t bam_bytes);
// ... and the verdicts on what the statuses' scan found (head[1..3]: the first sample of status 2, 3, 4) and on the blocks' statuses
int status_verdict(bvc_ctx *ctx, const int64_t head[4]);
int block_verdict(bvc_ctx *ctx, const std::vector<uint32_t> &block_status);

// bvc_vcf.hip: the device copy of bvc_vcf_bp_lut in ctx->d_vcf_lut, made at the context's first use of it
int vcf_lut_device(bvc_ctx *ctx);

#pragma GCC visibility pop
