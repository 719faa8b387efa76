// bvc_api.hip -- host side of libbvc: the C ABI declared in include/bvc.h.
// One context = one gfx950 device + one HIP stream + device scratch.  No CPU fallback exists: every
// compute entry point launches the HIP kernels or fails with an error code.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <mutex>
#include <vector>

#include "bvc_internal.h"

using namespace bvc;

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
    } tile;
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
    DevBuf d_grp_labels;               // group mode: the call's group vector clamped to 0..n_groups (hist_kernel.hip)
    int64_t *d_grp_scratch = nullptr;  // group mode: "samples ordered by group" flag + column bounds (hist_kernel.hip)
    // staging for BVC_PTR_HOST calls: two sets, so that the upload of chunk i+1 (copy stream) runs under the kernels
    // of chunk i
    DevBuf d_stage[2];
    hipStream_t copy = nullptr;
    hipEvent_t ev_upload[2] = {nullptr, nullptr};
    hipEvent_t ev_set_free[2] = {nullptr, nullptr};   // ragged host calls: the kernels that read staging set k have finished
    PileupState pile;
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

namespace {

int fail(bvc_ctx *ctx, int code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) { ctx->err += ": "; ctx->err += hipGetErrorString(e); }
    }
    return code;
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
std::array<hipStream_t, 5> streams_of(const bvc_ctx *ctx) { return {ctx->stream, ctx->copy, ctx->side, ctx->side_b, ctx->side_c}; }

// A failed call must not leave an upload or a kernel running on the context's buffers: the next call may free or refill
// them, and stage 2 of what was already launched may still run on the side streams.  Returns `code`.
int drain_on_error(bvc_ctx *ctx, int code)
{
    for (hipStream_t s : streams_of(ctx)) (void)hipStreamSynchronize(s);
    for (bool &p : ctx->em_pending) p = false;
    (void)hipGetLastError();
    return code;
}

#define BVC_HIP_D(ctx, call)                                                                         \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return drain_on_error((ctx), fail((ctx), BVC_ERR_DEVICE, #call, e__)); \
    } while (0)

int ensure(bvc_ctx *ctx, DevBuf &buf, size_t need)
{
    if (need <= buf.cap) return BVC_OK;
    if (buf.p) {
        // nothing may still be reading or writing the old buffer: the context's stream, and the copy stream (a staging
        // set may have an upload in flight after a failed host-pointer call)
        BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->copy) BVC_HIP(ctx, hipStreamSynchronize(ctx->copy));
        BVC_HIP(ctx, hipFree(buf.p));
        buf.p = nullptr; buf.cap = 0;
    }
    size_t want = need + need / 4;
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc(&p, need) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, BVC_ERR_ALLOC, "device scratch allocation failed"); }
        want = need;
    }
    buf.p = static_cast<char *>(p);
    buf.cap = want;
    // Fresh device memory holds whatever its last owner left.  No kernel of the library is meant to read scratch it has not
    // written, and so that a slip there can never read another call's (or another process's) leftovers the new buffer is
    // cleared before anything can touch it -- to 0xFF bytes in the -DBVC_POISON build, which makes such a slip loud.
    // (Allocation happens once per buffer and size: the synchronize is not on the steady-state path.)
#ifdef BVC_POISON
    constexpr int kFill = 0xFF;
#else
    constexpr int kFill = 0;
#endif
    BVC_HIP(ctx, hipMemsetAsync(buf.p, kFill, want, ctx->stream));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

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

hipEvent_t take_event(bvc_ctx *ctx)
{
    if (!ctx->ev_pool.empty()) { hipEvent_t e = ctx->ev_pool.back(); ctx->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void give_back(bvc_ctx *ctx, hipEvent_t e) { if (e) ctx->ev_pool.push_back(e); }

void give_back(bvc_ctx *ctx, bvc_ctx::Triple &t)
{
    give_back(ctx, t.a); give_back(ctx, t.b); give_back(ctx, t.c); give_back(ctx, t.d);
    t.a = t.b = t.c = t.d = nullptr;
}

// Four timing events for one call, or none at all (never a partial set).
bool take_timing_events(bvc_ctx *ctx, bvc_ctx::Triple &t)
{
    t.a = take_event(ctx); t.b = take_event(ctx); t.c = take_event(ctx); t.d = take_event(ctx);
    if (t.a && t.b && t.c && t.d) return true;
    give_back(ctx, t);
    return false;
}

// Drains finished timing records into the running totals so that ev_pending stays bounded when the caller never
// asks for the profile.
void reap_timing(bvc_ctx *ctx, bool all);

// Make the context's stream wait for every stage-2 launch still running on the side stream.
int join_side(bvc_ctx *ctx)
{
    for (int b = 0; b < bvc_ctx::kRing; ++b)
        if (ctx->em_pending[b]) {
            BVC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_em_done[b], 0));
            ctx->em_pending[b] = false;
        }
    return BVC_OK;
}

// Stage 2 of consecutive calls on alternating side streams?  An EM launch ends in a long tail of few busy waves (sites
// differ 4x in EM work and a launch has 1.6-2 sites per wave); on two streams the next launch's workgroups move in as
// the previous one's drain: +20-28 % where the EM is the bound (1e4 x 1e4: 1.46e7 -> 1.76e7 sites/s; ragged sites at
// 10 % coverage: 7.9e6 -> 1.02e7).  Underneath a long histogram pass the EM is not the bound and a second launch only
// adds to the crowd (-0.4 % on the headline), so long rows keep one stream.  (profiles/r02_sweep_em_streams.txt)
// Group mode's stage 2 IS the bound underneath its long histogram pass (k = 5, labels in any order): there two
// streams at half the wave budget each (2 x 4 per CU instead of 1 x 8) give +3.8 % (any order) / +1 % (ordered
// columns) -- the same chip share, the tails covered.  (profiles/r02_sweep_group_em_streams.txt)
int em_stream_count(const bvc_ctx *ctx, int by_default) { return ctx->ls.em_streams > 0 ? ctx->ls.em_streams : by_default; }

hipStream_t em_stream(bvc_ctx *ctx, int by_default)
{
    const int n = em_stream_count(ctx, by_default);
    const int k = (int)(ctx->side_flip++ % (unsigned)n);
    return k == 0 ? ctx->side : (k == 1 ? ctx->side_b : ctx->side_c);
}

// Device scratch of the item engine for a stage 2 of n_sites sites on ring buffer `slot` (null when the call will not
// use the engine: launch_lrt's rule).  Growing it waits for whatever may still be using the old one.
int em_scratch_for(bvc_ctx *ctx, int slot, int64_t n_sites, double min_af, void **out, int n_groups = 0)
{
    *out = nullptr;
    if (!uses_item_engine(ctx->ls, min_af)) return BVC_OK;
    const size_t need = n_groups > 0 ? em_group_scratch_bytes(n_sites, n_groups) : em_items_scratch_bytes(n_sites);
    DevBuf &buf = n_groups > 0 ? ctx->d_emg[slot] : ctx->d_em[slot];
    if (need > buf.cap) {
        int rcj = join_side(ctx);
        if (rcj != BVC_OK) return rcj;
    }
    int rc = ensure(ctx, buf, need);
    if (rc != BVC_OK) return rc;
    *out = buf.p;
    return BVC_OK;
}

// The ring buffers of one call: [n_sites][512] counts, the [n_sites][n_groups + 1][512] group histograms (group calls)
// and the item-engine scratch of both (null when stage 2 does not use the engine).
struct RingSlot {
    uint32_t *counts = nullptr, *grp = nullptr;
    void *em = nullptr, *emg = nullptr;
};

// The two stages of one call on device pointers.  `stage1(hist)` launches the histogram pass (dense, ragged, ...) on the
// context's stream into a buffer of the ring -- the counts, or with n_groups > 0 the group histograms; `stage2(s2, slot)`
// launches the EM/LRT on the same stream, or in overlap mode on a side stream (of em_stream(ctx, em_streams)) behind an event.
template <class Stage1, class Stage2>
int run_stages(bvc_ctx *ctx, int64_t n_sites, int n_groups, bool zero_counts, double min_af, int em_streams, Stage1 stage1,
               Stage2 stage2)
{
    const size_t cbytes = (size_t)n_sites * BVC_NCLASS * sizeof(uint32_t), gbytes = cbytes * (size_t)(n_groups + 1);
    const int buf = ctx->overlap ? ctx->flip : 0;
    if (ctx->overlap) ctx->flip = (ctx->flip + 1) % bvc_ctx::kRing;
    DevBuf &cnt = ctx->d_cnt[buf], &grp = ctx->d_grp[buf];
    if (cbytes > cnt.cap || (n_groups > 0 && gbytes > grp.cap)) {   // growing a buffer: nothing may still be reading it
        int rcj = join_side(ctx);
        if (rcj != BVC_OK) return rcj;
    }
    int rc = ensure(ctx, cnt, cbytes);
    if (rc == BVC_OK && n_groups > 0) rc = ensure(ctx, grp, gbytes);
    RingSlot slot;
    if (rc == BVC_OK) rc = em_scratch_for(ctx, buf, n_sites, min_af, &slot.em);
    if (rc == BVC_OK && n_groups > 0) rc = em_scratch_for(ctx, buf, n_sites, min_af, &slot.emg, n_groups);
    if (rc != BVC_OK) return rc;
    slot.counts = reinterpret_cast<uint32_t *>(cnt.p);
    if (n_groups > 0) slot.grp = reinterpret_cast<uint32_t *>(grp.p);
    bvc_ctx::Triple t{nullptr, nullptr, nullptr, nullptr, n_sites};
    const bool timed = ctx->profiling && take_timing_events(ctx, t);
    auto enqueue = [&]() -> int {
        // stage 1 on the context's stream; the histogram buffer is free once the EM that read it has finished
        if (ctx->overlap && ctx->em_pending[buf]) {
            BVC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_em_done[buf], 0));
            ctx->em_pending[buf] = false;
        }
        if (zero_counts) BVC_HIP(ctx, hipMemsetAsync(slot.counts, 0, cbytes, ctx->stream));
        if (timed) BVC_HIP(ctx, hipEventRecord(t.a, ctx->stream));
        BVC_HIP(ctx, stage1(n_groups > 0 ? slot.grp : slot.counts));
        if (timed) BVC_HIP(ctx, hipEventRecord(t.b, ctx->stream));
        // stage 2: same stream, or a side stream behind an event
        hipStream_t s2 = ctx->stream;
        if (ctx->overlap) {
            s2 = em_stream(ctx, em_streams);
            BVC_HIP(ctx, hipEventRecord(ctx->ev_hist_done[buf], ctx->stream));
            BVC_HIP(ctx, hipStreamWaitEvent(s2, ctx->ev_hist_done[buf], 0));
        }
        if (timed) BVC_HIP(ctx, hipEventRecord(t.c, s2));
        const int rc2 = stage2(s2, slot);
        if (rc2 != BVC_OK) return rc2;
        if (timed) {
            BVC_HIP(ctx, hipEventRecord(t.d, s2));
            ctx->ev_pending.push_back(t);
            t = bvc_ctx::Triple{nullptr, nullptr, nullptr, nullptr, 0};
            if (ctx->ev_pending.size() > 256) reap_timing(ctx, false);
        }
        if (ctx->overlap) {
            BVC_HIP(ctx, hipEventRecord(ctx->ev_em_done[buf], s2));
            ctx->em_pending[buf] = true;
        }
        return BVC_OK;
    };
    rc = enqueue();
    give_back(ctx, t);                          // an early exit returns the timing events to the pool
    return rc;
}

// The two stages of a plain call: stage 2 is the EM/LRT of the counts.
template <class Stage1>
int run_two_stages(bvc_ctx *ctx, int64_t n_sites, bool zero_counts, bool long_rows, Stage1 stage1,
                   const int8_t *ref_base, double min_af, const int8_t *comb, const uint8_t *n_comb,
                   bvc_site_result *results, int em_streams_long_rows = 1)
{
    return run_stages(ctx, n_sites, 0, zero_counts, min_af, long_rows ? em_streams_long_rows : 2, stage1,
                      [&](hipStream_t s2, const RingSlot &slot) -> int {
                          // underneath a long streaming pass the EM kernel keeps to a few wave slots; with short rows it is the
                          // longer kernel and takes the chip
                          const bool shared = ctx->overlap && long_rows;
                          BVC_HIP(ctx, launch_lrt(ctx->ls, s2, n_sites, slot.counts, BVC_NCLASS, ref_base, min_af, ctx->d_lut, comb,
                                                  n_comb, results, shared, 0, slot.em));
                          return BVC_OK;
                      });
}

int run_dense_device(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                     const int8_t *bases, const int8_t *quals, const int8_t *ref_base, double min_af,
                     bvc_site_result *results)
{
    const int split = choose_hist_split(ctx->ls, n_sites, n_samples);
    return run_two_stages(ctx, n_sites, split > 1, n_samples >= 200000,
                          [&](uint32_t *counts) {
                              return launch_hist_dense(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, bases, quals,
                                                       nullptr, 0, counts, split);
                          },
                          ref_base, min_af, nullptr, nullptr, results);
}

int run_packed_device(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const uint8_t *packed,
                      const int8_t *ref_base, double min_af, bvc_site_result *results)
{
    const int split = choose_hist_split(ctx->ls, n_sites, n_samples);
    return run_two_stages(ctx, n_sites, split > 1, n_samples >= 200000,
                          [&](uint32_t *counts) {
                              return launch_hist_packed(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, packed, counts, split);
                          },
                          // at one byte per sample stage 1 is as short as stage 2 and the call is bound by the VALU the
                          // two share: stage 2 on two streams (4.0e6 -> 4.55e6 sites/s, profiles/r02_packed_sweep.txt)
                          ref_base, min_af, nullptr, nullptr, results, 2);
}

int run_csr_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                   const int8_t *ref_base, double min_af, const int8_t *comb, const uint8_t *n_comb,
                   bvc_site_result *results)
{
    return run_two_stages(ctx, n_sites, false, false,
                          [&](uint32_t *counts) { return launch_hist_csr(ctx->ls, ctx->stream, n_sites, offsets, bases, quals, counts); },
                          ref_base, min_af, comb, n_comb, results);
}

void reap_timing(bvc_ctx *ctx, bool all)
{
    size_t kept = 0;
    for (size_t i = 0; i < ctx->ev_pending.size(); ++i) {
        bvc_ctx::Triple &t = ctx->ev_pending[i];
        if (!all && hipEventQuery(t.d) != hipSuccess) { (void)hipGetLastError(); ctx->ev_pending[kept++] = t; continue; }
        float ms1 = 0.f, ms2 = 0.f;
        if (hipEventElapsedTime(&ms1, t.a, t.b) == hipSuccess && hipEventElapsedTime(&ms2, t.c, t.d) == hipSuccess) {
            ctx->prof.hist_ms += ms1; ctx->prof.em_ms += ms2;
            ctx->prof.hist_launches += 1; ctx->prof.em_launches += 1; ctx->prof.sites += t.sites;
        } else {
            (void)hipGetLastError();
        }
        give_back(ctx, t.a); give_back(ctx, t.b); give_back(ctx, t.c); give_back(ctx, t.d);
    }
    ctx->ev_pending.resize(kept);
}

// Host-pointer calls go through device staging in chunks of sites; `upload(set, s0, ns)` enqueues the H2D copies of
// a chunk on the copy stream into staging set `set`, `compute(set, s0, ns)` enqueues its kernels and the D2H copies
// of its records on the context's stream.  The upload of chunk i+1 is issued before the (blocking) download of chunk
// i, so it runs under chunk i's kernels.
template <class Upload, class Compute>
int run_chunks(bvc_ctx *ctx, int64_t n_sites, int64_t chunk, Upload upload, Compute compute)
{
    int set = 0;
    int rc = upload(set, (int64_t)0, n_sites < chunk ? n_sites : chunk);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipEventRecord(ctx->ev_upload[set], ctx->copy));
    for (int64_t s0 = 0; s0 < n_sites; s0 += chunk, set ^= 1) {
        const int64_t ns = n_sites - s0 < chunk ? n_sites - s0 : chunk;
        BVC_HIP_D(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upload[set], 0));
        rc = compute(set, s0, ns, /*download=*/false);
        if (rc != BVC_OK) return drain_on_error(ctx, rc);
        const int64_t s1 = s0 + chunk;
        if (s1 < n_sites) {
            // the other set's previous chunk (i-1) has been downloaded synchronously below: it is free
            rc = upload(set ^ 1, s1, n_sites - s1 < chunk ? n_sites - s1 : chunk);
            if (rc != BVC_OK) return drain_on_error(ctx, rc);
            BVC_HIP_D(ctx, hipEventRecord(ctx->ev_upload[set ^ 1], ctx->copy));
        }
        rc = compute(set, s0, ns, /*download=*/true);
        if (rc != BVC_OK) return drain_on_error(ctx, rc);
        BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    }
    return BVC_OK;
}

// One staging set of a host-pointer dense call (run_dense_host).
struct DenseSet {
    int8_t *rows[2] = {nullptr, nullptr};
    int8_t *ref = nullptr;
    uint8_t *labels = nullptr;
    bvc_site_result *res = nullptr;
    bvc_group_result *gres = nullptr;
};

// Host-pointer dense tiles (bvc_lrt_dense, bvc_lrt_dense_packed, the group calls): site chunks of at most host_chunk_bytes per
// array through two staging sets.  `n_rows` row arrays (2: bases and quals, 1: packed rows); with n_groups > 0 the group vector
// `labels` goes up and the group records come down too.  `device(ns, set)` runs the two stages on a chunk staged in `set`.
template <class Device>
int run_dense_host(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, int n_rows, const int8_t *const rows[2],
                   const int8_t *ref_base, const uint8_t *labels, int n_groups, bvc_site_result *results, bvc_group_result *grp_results,
                   Device device)
{
    const int64_t row_bytes = row_stride > 0 ? row_stride : 1;
    int64_t chunk = ctx->ls.host_chunk_bytes / row_bytes;
    if (chunk < 1) chunk = 1;
    if (chunk > n_sites) chunk = n_sites;
    DenseSet sets[2];
    const int n_sets = n_sites > chunk ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        DenseSet &d = sets[k];
        int rc = carve(ctx, ctx->d_stage[k], 256, [&](Layout &L) {
            for (int a = 0; a < n_rows; ++a) d.rows[a] = L.take<int8_t>((size_t)chunk * (size_t)row_stride);
            d.ref = L.take<int8_t>((size_t)chunk);
            if (n_groups > 0) d.labels = L.take<uint8_t>((size_t)n_samples);
            d.res = L.take<bvc_site_result>((size_t)chunk);
            if (n_groups > 0) d.gres = L.take<bvc_group_result>((size_t)chunk * n_groups);
        });
        if (rc != BVC_OK) return rc;
        if (n_rows == 1) d.rows[1] = d.rows[0];
    }
    return run_chunks(ctx, n_sites, chunk,
        [&](int set, int64_t s0, int64_t ns) -> int {
            const DenseSet &d = sets[set];
            // the last row may be shorter than row_stride in the caller's allocation: copy exactly what is addressed
            const size_t bytes = n_samples ? (size_t)(ns - 1) * (size_t)row_stride + (size_t)n_samples : 0;
            // the group vector travels with the first chunk of each staging set
            if (n_groups > 0 && s0 < 2 * chunk && n_samples)
                BVC_HIP(ctx, hipMemcpyAsync(d.labels, labels, (size_t)n_samples, hipMemcpyHostToDevice, ctx->copy));
            for (int a = 0; a < n_rows && bytes; ++a)
                BVC_HIP(ctx, hipMemcpyAsync(d.rows[a], rows[a] + s0 * row_stride, bytes, hipMemcpyHostToDevice, ctx->copy));
            BVC_HIP(ctx, hipMemcpyAsync(d.ref, ref_base + s0, (size_t)ns, hipMemcpyHostToDevice, ctx->copy));
            return BVC_OK;
        },
        [&](int set, int64_t s0, int64_t ns, bool download) -> int {
            const DenseSet &d = sets[set];
            if (!download) {
                int rc = device(ns, d);
                return rc == BVC_OK ? join_side(ctx) : rc;
            }
            BVC_HIP(ctx, hipMemcpyAsync(results + s0, d.res, (size_t)ns * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
            if (n_groups > 0)
                BVC_HIP(ctx, hipMemcpyAsync(grp_results + s0 * n_groups, d.gres, (size_t)ns * n_groups * sizeof(bvc_group_result),
                                            hipMemcpyDeviceToHost, ctx->stream));
            return BVC_OK;
        });
}

// Group calls: stage 1 (`stage1(grp_counts)`: one pass, n_groups + 1 histograms per site, [site][n_groups + 1][512]) on the
// context's stream; stage 2 (sum, overall LRT, per-group LRT: src/BaseVarC.cpp:612-613, 617-661) on the same stream or, in
// overlap mode, on a side stream.  Dense tiles and ragged columns differ only in their stage 1.
template <class Stage1>
int run_group_stages(bvc_ctx *ctx, int64_t ns, int n_groups, bool long_rows, Stage1 stage1, const int8_t *r, double min_af,
                     bvc_site_result *res, bvc_group_result *gres)
{
    return run_stages(ctx, ns, n_groups, false, min_af, 2, stage1, [&](hipStream_t s2, const RingSlot &slot) -> int {
        BVC_HIP(ctx, launch_sum_groups(s2, ns, n_groups + 1, slot.grp, slot.counts));
        const bool shared = ctx->overlap && long_rows;
        const int per_launch = kGroupSharedWavesPerCu / em_stream_count(ctx, 2) > 2 ? kGroupSharedWavesPerCu / em_stream_count(ctx, 2) : 2;
        BVC_HIP(ctx, launch_lrt(ctx->ls, s2, ns, slot.counts, BVC_NCLASS, r, min_af, ctx->d_lut, nullptr, nullptr, res, shared, per_launch,
                                slot.em));
        BVC_HIP(ctx, launch_lrt_groups(ctx->ls, s2, ns, n_groups, slot.grp, r, min_af, ctx->d_lut, res, gres, shared, per_launch, slot.emg));
        return BVC_OK;
    });
}

// bvc_host_alloc's allocations: a transfer from / to a buffer inside one of them needs no bounce buffer
std::mutex g_pinned_mu;
std::vector<std::pair<const char *, size_t>> g_pinned;
bool in_pinned(const void *p, size_t n)
{
    std::lock_guard<std::mutex> g(g_pinned_mu);
    const char *c = static_cast<const char *>(p);
    for (auto const &r : g_pinned)
        if (c >= r.first && c + n <= r.first + r.second) return true;
    return false;
}

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

int check_common(bvc_ctx *ctx, int64_t n_sites, const void *a, const void *b, const void *c, const void *d)
{
    if (!ctx) return BVC_ERR_ARG;
    if (n_sites < 0) return fail(ctx, BVC_ERR_ARG, "n_sites < 0");
    if (n_sites > 0 && (!a || !b || !c || !d)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_sites > (int64_t)0x7FFFFFFF / 64) return fail(ctx, BVC_ERR_ARG, "too many sites in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    return BVC_OK;
}

}  // namespace

extern "C" {

const char *bvc_version(void) { return "libbvc 0.3.0 (gfx950)"; }

int bvc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

static int env_int(const char *name, int lo, int hi, int dflt)
{
    const char *e = getenv(name);
    if (!e) return dflt;
    const int v = atoi(e);
    return (v >= lo && v <= hi) ? v : dflt;
}

int bvc_create(bvc_ctx **out, int device)
{
    if (!out) return BVC_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return BVC_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) return BVC_ERR_NO_DEVICE;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return BVC_ERR_DEVICE;
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0) return BVC_ERR_NO_DEVICE;   // code objects are gfx950 only
    bvc_ctx *ctx = new (std::nothrow) bvc_ctx();
    if (!ctx) return BVC_ERR_ALLOC;
    ctx->device = device;
#ifdef BVC_DIAG_KNOBS
    // experiment (host program on a CPU quota): let host threads SLEEP in hipStreamSynchronize instead of polling.  Process-wide,
    // which is why it is not a tuning of a context.
    if (env_int("BVC_BLOCKING_SYNC", 0, 1, 0)) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
#endif
    ctx->ls.n_cu = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    // starting values of the tuning knobs (bvc_set_tuning changes them per context; results never depend on them)
    ctx->ls.em_waves_per_cu = env_int("BVC_EM_WAVES_PER_CU", 1, 32, 0);
    ctx->ls.em_wpb = env_int("BVC_EM_WPB", 1, 4, 4) == 1 ? 1 : 4;
    ctx->ls.hist_split = env_int("BVC_HIST_SPLIT", 1, 64, 0);
    ctx->ls.group_pipe = env_int("BVC_GROUP_PIPE", 0, 1, 1);
    ctx->ls.group_log2c = env_int("BVC_GROUP_LOG2C", 0, 5, -1);
    ctx->ls.group_big_lds = env_int("BVC_GROUP_BIG_LDS", 0, 1, 1);
    ctx->ls.group_h16 = env_int("BVC_GROUP_H16", 0, 1, 0);
    ctx->ls.em_streams = env_int("BVC_EM_STREAMS", 0, 3, 0);
    ctx->ls.em_engine = env_int("BVC_EM_ENGINE", 0, 1, 0);
#ifdef BVC_DIAG_KNOBS
    // timing experiments only (tools/em_stage2.py phase breakdown): cuts region_kernel short, so the records are WRONG.  Not
    // compiled into the product: a stray environment variable must never be able to do that.
    ctx->ls.dbg_levels = env_int("BVC_DBG_LEVELS", 0, 12, 0);
#endif
    ctx->ls.em_tiny_regions = env_int("BVC_EM_TINY_REGIONS", 0, 1, 0);
    ctx->ls.em_prune = env_int("BVC_EM_PRUNE", 0, 1, 1);
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return BVC_ERR_DEVICE; }
    // likelihood table from the host's exp(), as the CPU path computes it (src/BaseType.cpp:13,15)
    QualLut lut;
    for (int q = 0; q < 128; ++q) {
        const double eps = std::exp(-0.23025850929940458 * q);   // MLN10TO10, src/BaseType.h:10
        lut.a[q] = 1.0 - eps;
        lut.e[q] = eps / 3.0;
        lut.log_e[q] = std::log(lut.e[q]);
        lut.log_a[q] = std::log(lut.a[q]);                       // (-inf / NaN below quality 2: such sites never reach the item engine)
    }
    lut.e_empty = 0.25;
    if (hipMalloc(reinterpret_cast<void **>(&ctx->d_lut), sizeof(QualLut)) != hipSuccess ||
        hipMemcpy(ctx->d_lut, &lut, sizeof(QualLut), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (ctx->d_lut) (void)hipFree(ctx->d_lut);
        delete ctx;
        return BVC_ERR_ALLOC;
    }
    // Stage 2 runs on side streams underneath the histogram pass of the next call (overlap mode).  They get the LOWEST dispatch
    // priority: when wave slots free up, the histogram kernel of the next call -- which the next stage 2 is waiting for -- goes
    // first, instead of queueing behind two stage-2 launches that fill the chip (BVC_SIDE_PRIORITY=0: plain streams, A/B runs).
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = 0; }
    const int side_prio = env_int("BVC_SIDE_PRIORITY", 0, 1, 1) ? prio_least : 0;
    bool ok = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamDefault) == hipSuccess &&
              hipEventCreateWithFlags(&ctx->ev_wait, hipEventBlockingSync | hipEventDisableTiming) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, side_prio) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->side_b, hipStreamNonBlocking, side_prio) == hipSuccess &&
              hipStreamCreateWithPriority(&ctx->side_c, hipStreamNonBlocking, side_prio) == hipSuccess &&
              hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&ctx->d_grp_scratch), kGroupScratchWords * sizeof(int64_t)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&ctx->d_sink), 256) == hipSuccess;
    for (int b = 0; b < bvc_ctx::kRing && ok; ++b)
        ok = hipEventCreateWithFlags(&ctx->ev_hist_done[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ctx->ev_em_done[b], hipEventDisableTiming) == hipSuccess;
    for (int b = 0; b < 2 && ok; ++b) ok = hipEventCreateWithFlags(&ctx->ev_upload[b], hipEventDisableTiming) == hipSuccess;
    for (int b = 0; b < 2 && ok; ++b) ok = hipEventCreateWithFlags(&ctx->ev_set_free[b], hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); bvc_destroy(ctx); return BVC_ERR_DEVICE; }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return BVC_OK;
}

void *bvc_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0) bytes = 1;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> g(g_pinned_mu);
    g_pinned.push_back({static_cast<const char *>(p), bytes});
    return p;
}

void bvc_host_free(void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        for (size_t i = 0; i < g_pinned.size(); ++i)
            if (g_pinned[i].first == p) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
    }
    (void)hipHostFree(p);
}

void bvc_destroy(bvc_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
    if (ctx->side_b) { (void)hipStreamSynchronize(ctx->side_b); (void)hipStreamDestroy(ctx->side_b); }
    if (ctx->side_c) { (void)hipStreamSynchronize(ctx->side_c); (void)hipStreamDestroy(ctx->side_c); }
    if (ctx->copy) { (void)hipStreamSynchronize(ctx->copy); (void)hipStreamDestroy(ctx->copy); }
    if (ctx->own_stream) { (void)hipStreamSynchronize(ctx->own_stream); (void)hipStreamDestroy(ctx->own_stream); }
    if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
    for (int b = 0; b < bvc_ctx::kRing; ++b) {
        if (ctx->ev_hist_done[b]) (void)hipEventDestroy(ctx->ev_hist_done[b]);
        if (ctx->ev_em_done[b]) (void)hipEventDestroy(ctx->ev_em_done[b]);
    }
    for (int b = 0; b < 2; ++b) {
        if (ctx->ev_upload[b]) (void)hipEventDestroy(ctx->ev_upload[b]);
        if (ctx->ev_set_free[b]) (void)hipEventDestroy(ctx->ev_set_free[b]);
    }
    for (auto &t : ctx->ev_pending) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); (void)hipEventDestroy(t.c); (void)hipEventDestroy(t.d); }
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->d_lut) (void)hipFree(ctx->d_lut);
    if (ctx->d_grp_scratch) (void)hipFree(ctx->d_grp_scratch);
    if (ctx->d_sink) (void)hipFree(ctx->d_sink);
    if (ctx->h_up) (void)hipHostFree(ctx->h_up);
    if (ctx->h_down) (void)hipHostFree(ctx->h_down);
    delete ctx;                        // frees the device scratch (DevBuf)
}

const char *bvc_last_error(const bvc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bvc_set_stream(bvc_ctx *ctx, void *hip_stream)
{
    if (!ctx) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side_b));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side_c));
    for (bool &p : ctx->em_pending) p = false;
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return BVC_OK;
}

int bvc_synchronize(bvc_ctx *ctx)
{
    if (!ctx) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    for (hipStream_t s : streams_of(ctx)) BVC_HIP(ctx, hipStreamSynchronize(s));
    for (bool &p : ctx->em_pending) p = false;
    return BVC_OK;
}

int bvc_set_overlap(bvc_ctx *ctx, int on)
{
    if (!ctx) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    int rc = join_side(ctx);
    if (rc != BVC_OK) return rc;
    ctx->overlap = on != 0;
    return BVC_OK;
}

int bvc_join(bvc_ctx *ctx)
{
    if (!ctx) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    return join_side(ctx);
}

int bvc_set_profiling(bvc_ctx *ctx, int on)
{
    if (!ctx) return BVC_ERR_ARG;
    ctx->profiling = on != 0;
    return BVC_OK;
}

int bvc_get_profile(bvc_ctx *ctx, bvc_profile *out, int reset)
{
    if (!ctx || !out) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side_b));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->side_c));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    reap_timing(ctx, true);
    *out = ctx->prof;
    if (reset) ctx->prof = bvc_profile{};
    return BVC_OK;
}

int bvc_lrt_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                  const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                  double min_af, bvc_site_result *results, uint32_t flags)
{
    // rows of zero samples carry no data: their pointers may be null
    int rc = check_common(ctx, n_sites, n_samples ? bases : ref_base, n_samples ? quals : ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    if (n_sites == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE)
        return run_dense_device(ctx, n_sites, n_samples, row_stride, bases, quals, ref_base, min_af, results);

    const int8_t *rows[2] = {bases, quals};
    return run_dense_host(ctx, n_sites, n_samples, row_stride, 2, rows, ref_base, nullptr, 0, results, nullptr,
                          [&](int64_t ns, const DenseSet &d) {
                              return run_dense_device(ctx, ns, n_samples, row_stride, d.rows[0], d.rows[1], d.ref, min_af, d.res);
                          });
}

int bvc_lrt_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const uint8_t *packed,
                         const int8_t *ref_base, double min_af, bvc_site_result *results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, n_samples ? (const void *)packed : (const void *)ref_base, ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    if (n_sites == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE) return run_packed_device(ctx, n_sites, n_samples, row_stride, packed, ref_base, min_af, results);

    const int8_t *rows[2] = {reinterpret_cast<const int8_t *>(packed), nullptr};
    return run_dense_host(ctx, n_sites, n_samples, row_stride, 1, rows, ref_base, nullptr, 0, results, nullptr,
                          [&](int64_t ns, const DenseSet &d) {
                              return run_packed_device(ctx, ns, n_samples, row_stride, reinterpret_cast<const uint8_t *>(d.rows[0]), d.ref,
                                                       min_af, d.res);
                          });
}

int bvc_pack_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const int8_t *bases,
                   const int8_t *quals, int64_t packed_stride, uint8_t *packed, int64_t *n_unrepresentable, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, n_samples ? (const void *)bases : (const void *)n_unrepresentable,
                          n_samples ? (const void *)quals : (const void *)n_unrepresentable,
                          n_samples ? (const void *)packed : (const void *)n_unrepresentable, n_unrepresentable);
    if (rc != BVC_OK) return rc;
    if (!n_unrepresentable) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_samples < 0 || row_stride < n_samples || packed_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row strides");
    if (!(flags & BVC_PTR_DEVICE)) return fail(ctx, BVC_ERR_ARG, "bvc_pack_dense takes device pointers (a host producer writes base << 6 | qual itself)");
    *n_unrepresentable = 0;
    if (n_sites == 0 || n_samples == 0) return BVC_OK;
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(ctx->d_sink) + 8;   // bytes 64..71 of the context's 256-byte sink
    BVC_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), ctx->stream));
    BVC_HIP(ctx, launch_pack_dense(ctx->stream, n_sites, n_samples, row_stride, bases, quals, packed_stride, packed, d_bad));
    unsigned long long bad = 0;
    BVC_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_unrepresentable = (int64_t)bad;
    return BVC_OK;
}

int bvc_hist_dense_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, const uint8_t *packed,
                          uint32_t *counts, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, n_samples ? (const void *)packed : (const void *)counts, counts, counts, counts);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    if (!(flags & BVC_PTR_DEVICE)) return fail(ctx, BVC_ERR_ARG, "bvc_hist_dense_packed takes device pointers");
    if (n_sites == 0) return BVC_OK;
    const int split = choose_hist_split(ctx->ls, n_sites, n_samples);
    if (split > 1) BVC_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n_sites * BVC_NCLASS * sizeof(uint32_t), ctx->stream));
    BVC_HIP(ctx, launch_hist_packed(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, packed, counts, split));
    return BVC_OK;
}

int bvc_hist_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                   const int8_t *bases, const int8_t *quals, uint32_t *counts, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, n_samples ? (const void *)bases : (const void *)counts,
                          n_samples ? (const void *)quals : (const void *)counts, counts, counts);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    if (n_sites == 0) return BVC_OK;
    const int split = choose_hist_split(ctx->ls, n_sites, n_samples);
    const size_t cbytes = (size_t)n_sites * BVC_NCLASS * sizeof(uint32_t);
    if (flags & BVC_PTR_DEVICE) {
        if (split > 1) BVC_HIP(ctx, hipMemsetAsync(counts, 0, cbytes, ctx->stream));
        BVC_HIP(ctx, launch_hist_dense(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, bases, quals, nullptr, 0, counts, split));
        return BVC_OK;
    }
    const size_t bytes = n_samples ? (size_t)(n_sites - 1) * (size_t)row_stride + (size_t)n_samples : 0;
    int8_t *d_b, *d_q;
    uint32_t *d_c;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_b = L.take<int8_t>(bytes);
        d_q = L.take<int8_t>(bytes);
        d_c = L.take<uint32_t>((size_t)n_sites * BVC_NCLASS);
    });
    if (rc != BVC_OK) return rc;
    if (bytes) BVC_HIP(ctx, hipMemcpyAsync(d_b, bases, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (bytes) BVC_HIP(ctx, hipMemcpyAsync(d_q, quals, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (split > 1) BVC_HIP(ctx, hipMemsetAsync(d_c, 0, cbytes, ctx->stream));
    BVC_HIP(ctx, launch_hist_dense(ctx->ls, ctx->stream, n_sites, n_samples, row_stride, d_b, d_q, nullptr, 0, d_c, split));
    BVC_HIP(ctx, hipMemcpyAsync(counts, d_c, cbytes, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

static int check_comb_host(bvc_ctx *ctx, int64_t n_sites, const int8_t *base_comb, const uint8_t *n_comb)
{
    for (int64_t s = 0; s < n_sites; ++s) {
        if (n_comb[s] > 4) return fail(ctx, BVC_ERR_ARG, "n_comb > 4");
        for (int c = 0; c < n_comb[s]; ++c)
            if (base_comb[s * 4 + c] < 0 || base_comb[s * 4 + c] > 3) return fail(ctx, BVC_ERR_ARG, "base_comb entry outside 0..3");
    }
    return BVC_OK;
}

int bvc_lrt_hist(bvc_ctx *ctx, int64_t n_sites, const uint32_t *counts, const int8_t *ref_base,
                 double min_af, const int8_t *base_comb, const uint8_t *n_comb,
                 bvc_site_result *results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, counts, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if ((base_comb == nullptr) != (n_comb == nullptr)) return fail(ctx, BVC_ERR_ARG, "base_comb and n_comb go together");
    if (n_sites == 0) return BVC_OK;
    void *em_scratch = nullptr;
    rc = em_scratch_for(ctx, bvc_ctx::kRing, n_sites, min_af, &em_scratch);
    if (rc != BVC_OK) return rc;
    if (flags & BVC_PTR_DEVICE) {
        BVC_HIP(ctx, launch_lrt(ctx->ls, ctx->stream, n_sites, counts, BVC_NCLASS, ref_base, min_af, ctx->d_lut, base_comb,
                                n_comb, results, false, 0, em_scratch));
        return BVC_OK;
    }
    if (base_comb && (rc = check_comb_host(ctx, n_sites, base_comb, n_comb)) != BVC_OK) return rc;
    const size_t cbytes = (size_t)n_sites * BVC_NCLASS * sizeof(uint32_t);
    uint32_t *d_c; int8_t *d_r, *d_cb; uint8_t *d_nc; bvc_site_result *d_res;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_c = L.take<uint32_t>((size_t)n_sites * BVC_NCLASS);
        d_r = L.take<int8_t>((size_t)n_sites);
        d_nc = L.take<uint8_t>((size_t)n_sites);
        d_cb = L.take<int8_t>((size_t)n_sites * 4);
        d_res = L.take<bvc_site_result>((size_t)n_sites);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP(ctx, hipMemcpyAsync(d_c, counts, cbytes, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    if (base_comb) {
        BVC_HIP(ctx, hipMemcpyAsync(d_nc, n_comb, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP(ctx, hipMemcpyAsync(d_cb, base_comb, (size_t)n_sites * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    BVC_HIP(ctx, launch_lrt(ctx->ls, ctx->stream, n_sites, d_c, BVC_NCLASS, d_r, min_af, ctx->d_lut,
                            base_comb ? d_cb : nullptr, base_comb ? d_nc : nullptr, d_res, false, 0, em_scratch));
    BVC_HIP(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost,
                                ctx->stream));
    BVC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

// Ragged host-pointer calls (bvc_lrt_csr, bvc_lrt_csr_comb, bvc_lrt_csr_packed).  quals == nullptr: packed observations.
// The per-site arrays (offsets, ref_base, candidate lists) go up once and the records come down once; the observations go
// through two staging sets in chunks of sites, the upload of chunk i + 1 (copy stream) under the kernels of chunk i, the
// sets handed back and forth by events -- the host blocks only in its uploads (pageable memory) and at the end.  A chunk's
// observations keep their element offsets: they are staged `lead` = offsets[s0] mod 256 bytes into the set and the kernels
// get the staging address minus offsets[s0] as their array base (never dereferenced outside the chunk), so every site
// sees the alignment it has in a one-piece call.  (Per-chunk uploads of the small arrays, a per-chunk download and a
// per-chunk synchronize cost 0.12 ms a chunk -- more than the kernels they were to hide; without them a chunk costs 0.06.)
static int run_csr_host(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                        const int8_t *ref_base, double min_af, const int8_t *base_comb, const uint8_t *n_comb,
                        bvc_site_result *results)
{
    const int64_t total = offsets[n_sites];
    // bytes per chunk and array: host_chunk_kib (512 MiB by default).  Smaller chunks do not pay: a pageable upload of 400 MB
    // takes 7.07 ms (56.6 GB/s), the whole call 7.54 ms in one piece and 7.50 / 7.53 / 7.70 ms in 3 / 6 / 12 chunks -- what
    // the hidden kernels give, the extra uploads take (profiles/r03_host_pointer_ragged_chunks.txt).
    const int64_t target = ctx->ls.host_chunk_bytes;
    const int64_t mean = total / n_sites > 0 ? total / n_sites : 1;
    int64_t chunk = target / mean;
    if (chunk < 1) chunk = 1;
    if (chunk > n_sites) chunk = n_sites;
    int64_t widest = 0;
    for (int64_t s0 = 0; s0 < n_sites; s0 += chunk) {
        const int64_t s1 = s0 + chunk < n_sites ? s0 + chunk : n_sites;
        if (offsets[s1] - offsets[s0] > widest) widest = offsets[s1] - offsets[s0];
    }
    // set 0 carries the per-site arrays in front of its observations
    int64_t *d_o; int8_t *d_r, *d_cb; uint8_t *d_nc; bvc_site_result *d_res;
    int8_t *d_b[2] = {nullptr, nullptr}, *d_q[2] = {nullptr, nullptr};
    const int n_sets = n_sites > chunk ? 2 : 1;
    int rc = BVC_OK;
    for (int k = 0; k < n_sets && rc == BVC_OK; ++k)
        rc = carve(ctx, ctx->d_stage[k], 256, [&](Layout &L) {
            if (k == 0) {
                d_o = L.take<int64_t>((size_t)n_sites + 1);
                d_r = L.take<int8_t>((size_t)n_sites);
                d_nc = L.take<uint8_t>((size_t)n_sites);
                d_cb = L.take<int8_t>((size_t)n_sites * 4);
                d_res = L.take<bvc_site_result>((size_t)n_sites);
            }
            d_b[k] = L.take<int8_t>((size_t)widest, 256);                  // + the lead
            if (quals) d_q[k] = L.take<int8_t>((size_t)widest, 256);
        });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_o, offsets, (size_t)(n_sites + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    if (base_comb) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_nc, n_comb, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_cb, base_comb, (size_t)n_sites * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    auto upload = [&](int set, int64_t s0, int64_t ns, bool reuse) -> int {
        const int64_t o0 = offsets[s0];
        const size_t bytes = (size_t)(offsets[s0 + ns] - o0), lead = (size_t)(o0 & 255);
        if (reuse) BVC_HIP_D(ctx, hipStreamWaitEvent(ctx->copy, ctx->ev_set_free[set], 0));   // the kernels of chunk i - 2 are done with it
        if (bytes) BVC_HIP_D(ctx, hipMemcpyAsync(d_b[set] + lead, bases + o0, bytes, hipMemcpyHostToDevice, ctx->copy));
        if (bytes && quals) BVC_HIP_D(ctx, hipMemcpyAsync(d_q[set] + lead, quals + o0, bytes, hipMemcpyHostToDevice, ctx->copy));
        BVC_HIP_D(ctx, hipEventRecord(ctx->ev_upload[set], ctx->copy));
        return BVC_OK;
    };
    int set = 0;
    rc = upload(0, 0, n_sites < chunk ? n_sites : chunk, false);
    if (rc != BVC_OK) return rc;
    int64_t i = 0;
    for (int64_t s0 = 0; s0 < n_sites; s0 += chunk, set ^= 1, ++i) {
        const int64_t ns = n_sites - s0 < chunk ? n_sites - s0 : chunk;
        const int64_t o0 = offsets[s0];
        const uintptr_t shift = (uintptr_t)(o0 - (o0 & 255));                // array base = staging + lead - o0
        const int8_t *pb = reinterpret_cast<const int8_t *>(reinterpret_cast<uintptr_t>(d_b[set]) - shift);
        const int8_t *pq = quals ? reinterpret_cast<const int8_t *>(reinterpret_cast<uintptr_t>(d_q[set]) - shift) : nullptr;
        BVC_HIP_D(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upload[set], 0));
        rc = run_csr_device(ctx, ns, d_o + s0, pb, pq, d_r + s0, min_af, base_comb ? d_cb + s0 * 4 : nullptr,
                            base_comb ? d_nc + s0 : nullptr, d_res + s0);
        if (rc != BVC_OK) return drain_on_error(ctx, rc);
        // the histogram kernels are the only readers of the set and they run on the context's stream
        BVC_HIP_D(ctx, hipEventRecord(ctx->ev_set_free[set], ctx->stream));
        const int64_t s1 = s0 + chunk;
        if (s1 < n_sites) {
            rc = upload(set ^ 1, s1, n_sites - s1 < chunk ? n_sites - s1 : chunk, i >= 1);
            if (rc != BVC_OK) return rc;
        }
    }
    rc = join_side(ctx);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

// Host-pointer ragged calls: the chunking and the uploads index the observations with offsets[0..n_sites].
static int check_offsets_host(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets)
{
    bool ok = offsets[0] == 0;
    for (int64_t s = 0; s < n_sites && ok; ++s) ok = offsets[s + 1] >= offsets[s];
    return ok ? BVC_OK : fail(ctx, BVC_ERR_ARG, "offsets must start at 0 and be non-decreasing");
}

int bvc_lrt_csr_comb(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets,
                     const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                     double min_af, const int8_t *base_comb, const uint8_t *n_comb,
                     bvc_site_result *results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, offsets, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if ((base_comb == nullptr) != (n_comb == nullptr)) return fail(ctx, BVC_ERR_ARG, "base_comb and n_comb go together");
    if (n_sites == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE) {
        if (!bases || !quals) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        return run_csr_device(ctx, n_sites, offsets, bases, quals, ref_base, min_af, base_comb, n_comb, results);
    }
    if ((rc = check_offsets_host(ctx, n_sites, offsets)) != BVC_OK) return rc;
    const int64_t total = offsets[n_sites];
    if (total > 0 && (!bases || !quals)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (base_comb && (rc = check_comb_host(ctx, n_sites, base_comb, n_comb)) != BVC_OK) return rc;
    return run_csr_host(ctx, n_sites, offsets, bases, quals, ref_base, min_af, base_comb, n_comb, results);
}

int bvc_lrt_csr_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed,
                       const int8_t *ref_base, double min_af, bvc_site_result *results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, offsets, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if (n_sites == 0) return BVC_OK;
    const int8_t *obs = reinterpret_cast<const int8_t *>(packed);
    if (flags & BVC_PTR_DEVICE) {
        if (!packed) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        return run_csr_device(ctx, n_sites, offsets, obs, nullptr, ref_base, min_af, nullptr, nullptr, results);
    }
    if ((rc = check_offsets_host(ctx, n_sites, offsets)) != BVC_OK) return rc;
    const int64_t total = offsets[n_sites];
    if (total > 0 && !packed) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    // half the bytes of bvc_lrt_csr over the host link
    return run_csr_host(ctx, n_sites, offsets, obs, nullptr, ref_base, min_af, nullptr, nullptr, results);
}

int bvc_lrt_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets,
                const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                double min_af, bvc_site_result *results, uint32_t flags)
{
    return bvc_lrt_csr_comb(ctx, n_sites, offsets, bases, quals, ref_base, min_af, nullptr, nullptr, results, flags);
}


// ---- ragged group calls ----------------------------------------------------------------------------------------------------
static int run_csr_groups_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                                 const int32_t *sample_of_obs, const int8_t *ref_base, double min_af, const uint8_t *group_of_sample,
                                 int64_t n_samples, int32_t n_groups, bvc_site_result *results, bvc_group_result *grp_results)
{
    return run_group_stages(ctx, n_sites, n_groups, false,
                            [&](uint32_t *gp) {
                                return launch_hist_csr_groups(ctx->ls, ctx->stream, n_sites, offsets, bases, quals, sample_of_obs,
                                                              group_of_sample, n_samples, n_groups, gp);
                            },
                            ref_base, min_af, results, grp_results);
}

int bvc_lrt_csr_groups(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                       const int32_t *sample_of_obs, const int8_t *ref_base, double min_af,
                       const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                       bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, offsets, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if (n_groups < 1 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
    if (n_samples < 0 || (n_samples > 0 && !group_of_sample) || !grp_results) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    if (n_sites == 0) return BVC_OK;
    if (flags & BVC_PTR_DEVICE) {
        if (!bases || !quals || !sample_of_obs) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        return run_csr_groups_device(ctx, n_sites, offsets, bases, quals, sample_of_obs, ref_base, min_af, group_of_sample, n_samples,
                                     n_groups, results, grp_results);
    }
    if ((rc = check_offsets_host(ctx, n_sites, offsets)) != BVC_OK) return rc;
    const int64_t total = offsets[n_sites];
    if (total > 0 && (!bases || !quals || !sample_of_obs)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    // one piece through staging set 0
    int64_t *d_o; int8_t *d_r, *d_b, *d_q; uint8_t *d_g; int32_t *d_s; bvc_site_result *d_res; bvc_group_result *d_gres;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_o = L.take<int64_t>((size_t)n_sites + 1);
        d_r = L.take<int8_t>((size_t)n_sites);
        d_g = L.take<uint8_t>((size_t)n_samples, 1);
        d_b = L.take<int8_t>((size_t)total, 16);
        d_q = L.take<int8_t>((size_t)total, 16);
        d_s = L.take<int32_t>((size_t)total, 16);
        d_res = L.take<bvc_site_result>((size_t)n_sites);
        d_gres = L.take<bvc_group_result>((size_t)n_sites * n_groups);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_o, offsets, (size_t)(n_sites + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    if (n_samples) BVC_HIP_D(ctx, hipMemcpyAsync(d_g, group_of_sample, (size_t)n_samples, hipMemcpyHostToDevice, ctx->stream));
    if (total) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_b, bases, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_q, quals, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_s, sample_of_obs, (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run_csr_groups_device(ctx, n_sites, d_o, d_b, d_q, d_s, d_r, min_af, d_g, n_samples, n_groups, d_res, d_gres);
    if (rc == BVC_OK) rc = join_side(ctx);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(grp_results, d_gres, (size_t)n_sites * n_groups * sizeof(bvc_group_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

// ---- ragged group calls with one label byte per observation ------------------------------------------------------------------
// obs = the bases, or with quals == nullptr the packed bytes (as run_csr_device takes them)
static int run_csr_labels_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals,
                                 const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                                 bvc_site_result *results, bvc_group_result *grp_results)
{
    return run_group_stages(ctx, n_sites, n_groups, false,
                            [&](uint32_t *gp) {
                                return launch_hist_csr_labels(ctx->ls, ctx->stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, gp);
                            },
                            ref_base, min_af, results, grp_results);
}

// bvc_lrt_csr_group_labels (n_arrays = 2: obs = bases, quals) and bvc_lrt_csr_group_labels_packed (1: obs = packed, quals not used)
static int lrt_csr_labels_impl(bvc_ctx *ctx, int n_arrays, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals,
                               const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                               bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, offsets, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if (n_groups < 1 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
    if (!grp_results) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    if (n_sites == 0) return BVC_OK;
    if (n_arrays == 1) quals = nullptr;
    const bool have_all = obs && (n_arrays == 1 || quals) && group_of_obs;
    if (flags & BVC_PTR_DEVICE) {
        if (!have_all) return fail(ctx, BVC_ERR_ARG, "null data pointer");
        return run_csr_labels_device(ctx, n_sites, offsets, obs, quals, group_of_obs, ref_base, min_af, n_groups, results, grp_results);
    }
    if ((rc = check_offsets_host(ctx, n_sites, offsets)) != BVC_OK) return rc;
    const int64_t total = offsets[n_sites];
    if (total > 0 && !have_all) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    // one piece through staging set 0
    int64_t *d_o; int8_t *d_r; uint8_t *d_b, *d_q = nullptr, *d_l; bvc_site_result *d_res; bvc_group_result *d_gres;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_o = L.take<int64_t>((size_t)n_sites + 1);
        d_r = L.take<int8_t>((size_t)n_sites);
        d_b = L.take<uint8_t>((size_t)total, 16);
        if (n_arrays == 2) d_q = L.take<uint8_t>((size_t)total, 16);
        d_l = L.take<uint8_t>((size_t)total, 16);
        d_res = L.take<bvc_site_result>((size_t)n_sites);
        d_gres = L.take<bvc_group_result>((size_t)n_sites * n_groups);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_o, offsets, (size_t)(n_sites + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    if (total) {
        BVC_HIP_D(ctx, hipMemcpyAsync(d_b, obs, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
        if (n_arrays == 2) BVC_HIP_D(ctx, hipMemcpyAsync(d_q, quals, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_l, group_of_obs, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = run_csr_labels_device(ctx, n_sites, d_o, d_b, d_q, d_l, d_r, min_af, n_groups, d_res, d_gres);
    if (rc == BVC_OK) rc = join_side(ctx);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(grp_results, d_gres, (size_t)n_sites * n_groups * sizeof(bvc_group_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

int bvc_lrt_csr_group_labels(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                             const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                             bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    return lrt_csr_labels_impl(ctx, 2, n_sites, offsets, reinterpret_cast<const uint8_t *>(bases), reinterpret_cast<const uint8_t *>(quals),
                               group_of_obs, ref_base, min_af, n_groups, results, grp_results, flags);
}

int bvc_lrt_csr_group_labels_packed(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *packed, const uint8_t *group_of_obs,
                                    const int8_t *ref_base, double min_af, int32_t n_groups,
                                    bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    return lrt_csr_labels_impl(ctx, 1, n_sites, offsets, packed, nullptr, group_of_obs, ref_base, min_af, n_groups, results, grp_results,
                               flags);
}

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
// The slices of a tile's meta buffer that both begin calls lay out alike: the line table, the first sample and the size of every
// batch (each slice batch_pad bytes longer), the per-line words, 256 bytes of status (the totals at +64), the two offset arrays
// and the tallies.  Returns the bytes from the status to the end of the tallies: what a begin call clears.
static size_t carve_tile(Layout &L, PileupTile &P, int32_t n_batches, int32_t n_pos, size_t batch_pad, uint32_t *&line_start,
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

int bvc_pileup_begin(bvc_ctx *ctx, const char *text, int64_t text_bytes, const uint32_t *line_start,
                     const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                     int64_t *n_entries, int64_t *n_indels)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState::Tile &tile = ctx->pile.tile;
    tile = PileupState::Tile{};
    if (n_batches < 0 || n_positions < 0 || text_bytes < 0 || !n_entries || !n_indels) return fail(ctx, BVC_ERR_ARG, "bad argument");
    if (text_bytes > (int64_t)0xFFFFFF00) return fail(ctx, BVC_ERR_ARG, "more than 4 GiB of text in one tile (use fewer positions)");
    const int64_t n_lines = (int64_t)n_batches * n_positions;
    if (n_lines > 0 && (!text || !line_start || !sample0 || !n_in_batch)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_positions > (int32_t)(0x7FFFFFFF / 64)) return fail(ctx, BVC_ERR_ARG, "too many positions in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    *n_entries = 0; *n_indels = 0;
    // the line table is what the kernels index the text with: every line inside the text, the lines of a batch in order
    for (int32_t b = 0; b < n_batches; ++b) {
        const uint32_t *ls = line_start + (int64_t)b * (n_positions + 1);
        if (n_in_batch[b] < 0) return fail(ctx, BVC_ERR_ARG, "negative batch size");
        for (int32_t t = 0; t < n_positions; ++t)
            if (ls[t + 1] <= ls[t]) return fail(ctx, BVC_ERR_ARG, "line_start: every line holds at least its newline, lines of a batch ascend");
        if (n_positions > 0 && (int64_t)ls[n_positions] > text_bytes) return fail(ctx, BVC_ERR_ARG, "line_start points outside the text");
    }
    const size_t T = (size_t)n_positions, nb = (size_t)n_batches;
    PileupTile &P = tile.P;
    uint32_t *d_ls; int32_t *d_s0, *d_nib;
    size_t clear = 0;
    int rc = ensure(ctx, ctx->pile.text, (size_t)text_bytes + 64);
    if (rc == BVC_OK)
        rc = carve(ctx, ctx->pile.meta, 0, [&](Layout &L) { clear = carve_tile(L, P, n_batches, n_positions, 0, d_ls, d_s0, d_nib); });
    if (rc != BVC_OK) return rc;
    P.text = reinterpret_cast<const uint8_t *>(ctx->pile.text.p);
    BVC_HIP_D(ctx, hipMemsetAsync(P.status, 0, clear, ctx->stream));     // status, totals, offsets of an empty tile, tallies
    if (n_lines > 0) {
        BVC_HIP_D(ctx, hipMemcpyAsync(ctx->pile.text.p, text, (size_t)text_bytes, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_ls, line_start, nb * (T + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_s0, sample0, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_nib, n_in_batch, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, launch_pileup_count(ctx->stream, P));
    }
    uint32_t st[4] = {0, 0, 0, 0};
    int64_t tot[2] = {0, 0};
    BVC_HIP_D(ctx, hipMemcpyAsync(st, P.status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(tot, P.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    if (st[0] != 0) return BVC_PILEUP_IRREGULAR;
    tile.entries = tot[0]; tile.obs = tot[1]; tile.indels = st[1];
    tile.begun = true;
    *n_entries = tot[0]; *n_indels = st[1];
    return BVC_OK;
}

// The binary records of the same content (host/pileup.h): the records go where the text goes, rec_start where line_start goes, and the
// tile is marked so that the count and write passes launch pileup_bin_kernel; bvc_pileup_finish[_called] serve it as they serve text.
int bvc_pileup_begin_bin(bvc_ctx *ctx, const uint8_t *records, int64_t records_bytes, const uint32_t *rec_start,
                         const int32_t *sample0, const int32_t *n_in_batch, int32_t n_batches, int32_t n_positions,
                         int64_t *n_entries, int64_t *n_indels)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState::Tile &tile = ctx->pile.tile;
    tile = PileupState::Tile{};
    if (n_batches < 0 || n_positions < 0 || records_bytes < 0 || !n_entries || !n_indels) return fail(ctx, BVC_ERR_ARG, "bad argument");
    if (records_bytes > (int64_t)0xFFFFFF00) return fail(ctx, BVC_ERR_ARG, "more than 4 GiB of records in one tile (use fewer positions)");
    const int64_t n_recs = (int64_t)n_batches * n_positions;
    if (n_recs > 0 && (!records || !rec_start || !sample0 || !n_in_batch)) return fail(ctx, BVC_ERR_ARG, "null data pointer");
    if (n_positions > (int32_t)(0x7FFFFFFF / 64)) return fail(ctx, BVC_ERR_ARG, "too many positions in one call (split the tile)");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    *n_entries = 0; *n_indels = 0;
    // the record table is what the kernel bounds every load with: every record inside the buffer, as long as its length word says
    for (int32_t b = 0; b < n_batches; ++b) {
        const uint32_t *rs = rec_start + (int64_t)b * (n_positions + 1);
        if (n_in_batch[b] < 0) return fail(ctx, BVC_ERR_ARG, "negative batch size");
        for (int32_t t = 0; t < n_positions; ++t) {
            const int64_t r0 = rs[t], r1 = rs[t + 1];
            if (r1 < r0 + 4 || r1 > records_bytes) return fail(ctx, BVC_ERR_ARG, "rec_start: records of a batch ascend, each holds its length word, all lie inside records_bytes");
            const uint8_t *q = records + r0;
            const int64_t len = (int64_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
            if (r1 - r0 != 4 + len) return fail(ctx, BVC_ERR_ARG, "rec_start disagrees with a record's length word");
        }
    }
    const size_t T = (size_t)n_positions, nb = (size_t)n_batches;
    PileupTile &P = tile.P;
    uint32_t *d_rs; int32_t *d_s0, *d_nib;
    size_t clear = 0;
    int rc = ensure(ctx, ctx->pile.text, (size_t)records_bytes + 64);
    if (rc == BVC_OK)
        rc = carve(ctx, ctx->pile.meta, 0, [&](Layout &L) { clear = carve_tile(L, P, n_batches, n_positions, 0, d_rs, d_s0, d_nib); });
    if (rc != BVC_OK) return rc;
    P.text = reinterpret_cast<const uint8_t *>(ctx->pile.text.p);
    P.bin = true;
    BVC_HIP_D(ctx, hipMemsetAsync(P.status, 0, clear, ctx->stream));     // status, totals, offsets of an empty tile, tallies
    if (n_recs > 0) {
        BVC_HIP_D(ctx, hipMemcpyAsync(ctx->pile.text.p, records, (size_t)records_bytes, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_rs, rec_start, nb * (T + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_s0, sample0, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, hipMemcpyAsync(d_nib, n_in_batch, nb * 4, hipMemcpyHostToDevice, ctx->stream));
        BVC_HIP_D(ctx, launch_pileup_count(ctx->stream, P));
    }
    uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t tot[2] = {0, 0};
    BVC_HIP_D(ctx, hipMemcpyAsync(st, P.status, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(tot, P.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, wait_stream(ctx));
    if (st[0] != 0) {
        const std::string what = std::to_string(st[0]) + " malformed record(s) in the tile (an entry or an indel text runs past its record's end, or a "
                                 "sample index is not below the batch's size)";
        return fail(ctx, BVC_ERR_DATA, what.c_str());
    }
    tile.entries = tot[0]; tile.obs = tot[1]; tile.indels = st[1]; tile.indel_bytes = st[4];
    tile.begun = true;
    *n_entries = tot[0]; *n_indels = st[1];
    return BVC_OK;
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

// bvc_pileup_finish (called_off = null: the entries of every position) and bvc_pileup_finish_called (the entries of the called
// positions only, compacted on the device; called_cap = room in entries / samples)
static int pileup_finish_impl(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                              const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                              int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                              int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                              bvc_group_result *grp_results)
{
    if (!ctx) return BVC_ERR_ARG;
    PileupState &pile = ctx->pile;
    PileupState::Tile &tile = pile.tile;
    if (!tile.begun) return fail(ctx, BVC_ERR_ARG, "bvc_pileup_finish without a bvc_pileup_begin that returned BVC_OK");
    if (tile.on_device_text && tile.indels > 0 && !indel_text) return fail(ctx, BVC_ERR_ARG, "indel_text is needed: the tile's text is on the device only");
    tile.begun = false;
    PileupTile &P = tile.P;
    const int64_t T = P.n_pos, n_e = tile.entries, n_o = tile.obs, n_i = tile.indels, n_it = tile.indel_bytes;
    if (!carry_in || !carry_out || !entry_off) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (T > 0 && (!ref_base || !tally || !results)) return fail(ctx, BVC_ERR_ARG, "null pointer");
    const bool called_only = called_off != nullptr;
    if ((n_e > 0 && !called_only && (!entries || !samples)) || (n_i > 0 && !indels)) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (called_only && (called_cap < 0 || (called_cap > 0 && (!entries || !samples)))) return fail(ctx, BVC_ERR_ARG, "null pointer");
    if (n_groups < 0 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 0..32");
    if (n_groups > 0 && (!grp_results || n_samples < 0 || (n_samples > 0 && !group_of_sample))) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    int8_t *d_ref; bvc_site_result *d_res; uint8_t *d_g, *d_itext; bvc_group_result *d_gres; int64_t *d_called_off;
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
        d_itext = L.take<uint8_t>((size_t)(indel_text ? n_it : 0), 16);
        d_called_off = L.take<int64_t>(called_only ? (size_t)(T + 1) : 0);
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
                        (size_t)(called_only ? 0 : n_e) * (sizeof(bvc_pileup_entry) + 4) + (called_only ? (size_t)(T + 1) * 8 : 0) +
                        (size_t)n_i * sizeof(bvc_pileup_indel) + (size_t)n_it + 4096);
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
        BVC_HIP_D(ctx, io.d2h(results, d_res, (size_t)T * sizeof(bvc_site_result)));
        if (n_groups > 0)
            BVC_HIP_D(ctx, io.d2h(grp_results, d_gres, (size_t)T * (size_t)n_groups * sizeof(bvc_group_result)));
        BVC_HIP_D(ctx, io.d2h(tally, P.tally, (size_t)T * 32 * 4));
        if (n_e && !called_only) {
            BVC_HIP_D(ctx, io.d2h(entries, P.entries, (size_t)n_e * sizeof(bvc_pileup_entry)));
            BVC_HIP_D(ctx, io.d2h(samples, P.samples, (size_t)n_e * 4));
        }
        if (called_only) {
            BVC_HIP_D(ctx, launch_called_scan(ctx->stream, P, d_res, d_called_off));
            BVC_HIP_D(ctx, io.d2h(called_off, d_called_off, (size_t)(T + 1) * 8));
        }
        if (n_i && indel_text) {
            BVC_HIP_D(ctx, launch_indel_text(ctx->stream, P, d_itext, (uint32_t)n_it, P.status + 5));
            if (n_it) BVC_HIP_D(ctx, io.d2h(indel_text, d_itext, (size_t)n_it));
        }
        if (n_i) BVC_HIP_D(ctx, io.d2h(indels, P.indels, (size_t)n_i * sizeof(bvc_pileup_indel)));
        if ((int64_t)P.n_pos * P.n_batches > 0) BVC_HIP_D(ctx, io.d2h(&cout, P.status + 3, 4));
    }
    BVC_HIP_D(ctx, io.d2h(entry_off, P.entry_off, (size_t)(T + 1) * 8));
    BVC_HIP_D(ctx, wait_stream(ctx));
    io.deliver();
    if (called_only && T == 0) called_off[0] = 0;
    if (called_only && T > 0 && called_off[T] > 0) {
        // the second trip: the called positions' entries, gathered on the device (typically a few per cent of the tile's)
        const int64_t n_c = called_off[T];
        if (n_c > called_cap) return fail(ctx, BVC_ERR_ARG, "called_cap is smaller than the entries of the called positions (n_entries of the begin call always suffices)");
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
        BVC_HIP_D(ctx, io.d2h(entries, d_ce, (size_t)n_c * sizeof(bvc_pileup_entry)));
        BVC_HIP_D(ctx, io.d2h(samples, d_cs, (size_t)n_c * 4));
        BVC_HIP_D(ctx, wait_stream(ctx));
        io.deliver();
    }
    carry_out[0] = (uint8_t)(cout & 7u); carry_out[1] = (uint8_t)(cout >> 8); carry_out[2] = (uint8_t)(cout >> 16);
    carry_out[3] = (uint8_t)(cout >> 24); carry_out[4] = (uint8_t)((cout >> 3) & 1u);
    return BVC_OK;
}

int bvc_pileup_finish(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                      const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                      int64_t *entry_off, int32_t *tally, bvc_pileup_entry *entries, int32_t *samples,
                      bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results, bvc_group_result *grp_results)
{
    return pileup_finish_impl(ctx, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, nullptr, 0,
                              entries, samples, indels, indel_text, results, grp_results);
}

int bvc_pileup_finish_called(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                             const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                             int64_t *entry_off, int32_t *tally, int64_t *called_off, int64_t called_cap, bvc_pileup_entry *entries,
                             int32_t *samples, bvc_pileup_indel *indels, char *indel_text, bvc_site_result *results,
                             bvc_group_result *grp_results)
{
    if (ctx && !called_off) return fail(ctx, BVC_ERR_ARG, "null pointer");
    return pileup_finish_impl(ctx, ref_base, min_af, carry_in, carry_out, group_of_sample, n_samples, n_groups, entry_off, tally, called_off,
                              called_cap, entries, samples, indels, indel_text, results, grp_results);
}

// bvc_lrt_dense_groups and bvc_lrt_dense_groups_packed: `packed` = the tile is one byte per sample in `bases`
// (base << 6 | qual, include/bvc.h) and `quals` is not used.
static int lrt_groups_impl(bvc_ctx *ctx, bool packed, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                           const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                           double min_af, const uint8_t *group_of_sample, int32_t n_groups,
                           bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    if (packed) quals = bases;
    // rows of zero samples carry no data: their pointers may be null
    int rc = check_common(ctx, n_sites, n_samples ? bases : ref_base, n_samples ? quals : ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    if (n_groups < 1 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
    if (!group_of_sample || !grp_results) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    if (n_sites == 0) return BVC_OK;
    auto run_device = [&](int64_t ns, const int8_t *b, const int8_t *q, const int8_t *r, const uint8_t *g,
                          bvc_site_result *res, bvc_group_result *gres) -> int {
        const size_t lbytes = group_labels_bytes(n_samples, ns);       // the call's labels clamped to 0..n_groups + a flag per site
        if (lbytes > ctx->d_grp_labels.cap) { int rj = join_side(ctx); if (rj != BVC_OK) return rj; }
        int rc2 = ensure(ctx, ctx->d_grp_labels, lbytes);
        if (rc2 != BVC_OK) return rc2;
        uint8_t *labels = reinterpret_cast<uint8_t *>(ctx->d_grp_labels.p);
        return run_group_stages(ctx, ns, n_groups, n_samples >= 200000,
                                [&](uint32_t *gp) {
                                    if (packed)
                                        return launch_hist_packed_groups(ctx->ls, ctx->stream, ns, n_samples, row_stride,
                                                                         reinterpret_cast<const uint8_t *>(b), g, n_groups, gp,
                                                                         ctx->d_grp_scratch, labels);
                                    return launch_hist_dense(ctx->ls, ctx->stream, ns, n_samples, row_stride, b, q, g, n_groups, gp, 1,
                                                             ctx->d_grp_scratch, labels);
                                },
                                r, min_af, res, gres);
    };

    if (flags & BVC_PTR_DEVICE)
        return run_device(n_sites, bases, quals, ref_base, group_of_sample, results, grp_results);

    const int8_t *rows[2] = {bases, quals};
    return run_dense_host(ctx, n_sites, n_samples, row_stride, packed ? 1 : 2, rows, ref_base, group_of_sample, n_groups, results,
                          grp_results, [&](int64_t ns, const DenseSet &d) {
                              return run_device(ns, d.rows[0], d.rows[1], d.ref, d.labels, d.res, d.gres);
                          });
}

int bvc_lrt_dense_groups(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                         const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                         double min_af, const uint8_t *group_of_sample, int32_t n_groups,
                         bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    return lrt_groups_impl(ctx, false, n_sites, n_samples, row_stride, bases, quals, ref_base, min_af, group_of_sample, n_groups,
                           results, grp_results, flags);
}

int bvc_lrt_dense_groups_packed(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                                const uint8_t *packed, const int8_t *ref_base, double min_af,
                                const uint8_t *group_of_sample, int32_t n_groups,
                                bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    return lrt_groups_impl(ctx, true, n_sites, n_samples, row_stride, reinterpret_cast<const int8_t *>(packed), nullptr, ref_base,
                           min_af, group_of_sample, n_groups, results, grp_results, flags);
}

#ifdef BVC_CHECK_LDS
// Diagnostic builds only (bvc_device.h): the violations the checked kernels recorded, 8 words per translation unit
// (histogram kernels, wave engine, item engine): [0] count, [1..5] the first one's check id, value, limit, blockIdx.x,
// threadIdx.x.  Synchronises the device.  reset != 0 clears the records.
int bvc_debug_report(bvc_ctx *ctx, uint32_t *out24, int reset)
{
    if (!out24) return BVC_ERR_ARG;
    if (ctx) BVC_HIP(ctx, hipSetDevice(ctx->device));            // null: the calling thread's current device
    BVC_HIP(ctx, hipDeviceSynchronize());
    BVC_HIP(ctx, debug_read_hist(out24, reset != 0));
    BVC_HIP(ctx, debug_read_wave_engine(out24 + 8, reset != 0));
    BVC_HIP(ctx, debug_read_items(out24 + 16, reset != 0));
    uint32_t pl[8];                                              // pileup_kernel.hip: folded into the histogram unit's count
    BVC_HIP(ctx, debug_read_pileup(pl, reset != 0));
    if (pl[0]) { if (out24[0] == 0) for (int i = 1; i < 8; ++i) out24[i] = pl[i]; out24[0] += pl[0]; }
    BVC_HIP(ctx, debug_read_inflate(pl, reset != 0));
    if (pl[0]) { if (out24[0] == 0) for (int i = 1; i < 8; ++i) out24[i] = pl[i]; out24[0] += pl[0]; }
    return BVC_OK;
}
#endif

int bvc_set_tuning(bvc_ctx *ctx, const char *key, int value)
{
    if (!ctx) return BVC_ERR_ARG;
    if (!key) return fail(ctx, BVC_ERR_ARG, "null tuning key");
    BVC_HIP(ctx, hipSetDevice(ctx->device));                     // "em_streams" joins the side streams of THIS device
    if (std::strcmp(key, "em_waves_per_cu") == 0 && value >= 0 && value <= 32) { ctx->ls.em_waves_per_cu = value; return BVC_OK; }
    if (std::strcmp(key, "em_wpb") == 0 && (value == 1 || value == 4)) { ctx->ls.em_wpb = value; return BVC_OK; }
    if (std::strcmp(key, "hist_split") == 0 && value >= 0 && value <= 64) { ctx->ls.hist_split = value; return BVC_OK; }
    if (std::strcmp(key, "group_pipe") == 0 && (value == 0 || value == 1)) { ctx->ls.group_pipe = value; return BVC_OK; }
    if (std::strcmp(key, "group_copies_log2") == 0 && value >= -1 && value <= 5) { ctx->ls.group_log2c = value; return BVC_OK; }
    if (std::strcmp(key, "group_big_lds") == 0 && (value == 0 || value == 1)) { ctx->ls.group_big_lds = value; return BVC_OK; }
    if (std::strcmp(key, "group_h16") == 0 && (value == 0 || value == 1)) { ctx->ls.group_h16 = value; return BVC_OK; }
    if (std::strcmp(key, "em_engine") == 0 && value >= 0 && value <= 1) { ctx->ls.em_engine = value; return BVC_OK; }
    if (std::strcmp(key, "em_tiny_regions") == 0 && value >= 0 && value <= 1) { ctx->ls.em_tiny_regions = value; return BVC_OK; }
    if (std::strcmp(key, "em_prune") == 0 && value >= 0 && value <= 1) { ctx->ls.em_prune = value; return BVC_OK; }
    if (std::strcmp(key, "em_streams") == 0 && value >= 0 && value <= 3) {
        int rcj = join_side(ctx);
        if (rcj != BVC_OK) return rcj;
        ctx->ls.em_streams = value;
        return BVC_OK;
    }
    if (std::strcmp(key, "host_chunk_kib") == 0 && value >= 1 && value <= (1 << 21)) { ctx->ls.host_chunk_bytes = (int64_t)value << 10; return BVC_OK; }
    return fail(ctx, BVC_ERR_ARG, "unknown tuning key or value out of range");
}

int bvc_stream_read_ms(bvc_ctx *ctx, const void *device_ptr, int64_t bytes, int repeats, double *ms_per_pass)
{
    if (!ctx || !device_ptr || !ms_per_pass || bytes < 16 || repeats < 1) return ctx ? fail(ctx, BVC_ERR_ARG, "bad argument") : BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t a = take_event(ctx), b = take_event(ctx);
    if (!a || !b) { give_back(ctx, a); give_back(ctx, b); return fail(ctx, BVC_ERR_DEVICE, "hipEventCreate failed"); }
    auto bail = [&](int code) { give_back(ctx, a); give_back(ctx, b); return code; };
    hipError_t e = launch_stream_read(ctx->stream, device_ptr, bytes, ctx->d_sink);        // warm-up
    if (e == hipSuccess) e = hipEventRecord(a, ctx->stream);
    for (int i = 0; i < repeats && e == hipSuccess; ++i) e = launch_stream_read(ctx->stream, device_ptr, bytes, ctx->d_sink);
    if (e == hipSuccess) e = hipEventRecord(b, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    if (e != hipSuccess) return bail(fail(ctx, BVC_ERR_DEVICE, "stream read measurement", e));
    give_back(ctx, a); give_back(ctx, b);
    *ms_per_pass = (double)ms / repeats;
    return BVC_OK;
}

int bvc_synth_dense(bvc_ctx *ctx, uint64_t seed, int64_t site0, int64_t n_sites, int64_t n_samples,
                    int64_t row_stride, uint32_t cov_thr16, int8_t *bases, int8_t *quals, int8_t *ref_base)
{
    int rc = check_common(ctx, n_sites, bases, quals, ref_base, ref_base);
    if (rc != BVC_OK) return rc;
    if (n_samples < 0 || row_stride < n_samples) return fail(ctx, BVC_ERR_ARG, "need 0 <= n_samples <= row_stride");
    BVC_HIP(ctx, launch_synth_dense(ctx->stream, seed, site0, n_sites, n_samples, row_stride, cov_thr16, bases, quals,
                                    ref_base));
    return BVC_OK;
}

}  // extern "C"
