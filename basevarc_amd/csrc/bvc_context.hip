// bvc_context.hip -- a context's life: creation from the environment, streams, overlap mode, tuning, profile, pinned host memory,
// and the helpers of bvc_ctx.h that own a context's scratch, streams and timing events.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "bvc_ctx.h"

hipError_t sync_streams(bvc_ctx *ctx)
{
    hipError_t first = hipSuccess;
    for (hipStream_t s : streams_of(ctx)) {
        const hipError_t e = hipStreamSynchronize(s);
        if (first == hipSuccess) first = e;
    }
    for (bool &p : ctx->em_pending) p = false;
    return first;
}

int drain_on_error(bvc_ctx *ctx, int code)
{
    (void)sync_streams(ctx);
    (void)hipGetLastError();
    return code;
}

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

bool take_timing_events(bvc_ctx *ctx, bvc_ctx::Triple &t)
{
    t.a = take_event(ctx); t.b = take_event(ctx); t.c = take_event(ctx); t.d = take_event(ctx);
    if (t.a && t.b && t.c && t.d) return true;
    give_back(ctx, t);
    return false;
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
        give_back(ctx, t);
    }
    ctx->ev_pending.resize(kept);
}

// bvc_host_alloc's allocations
namespace {
std::mutex g_pinned_mu;
std::vector<std::pair<const char *, size_t>> g_pinned;
}  // namespace

bool in_pinned(const void *p, size_t n)
{
    std::lock_guard<std::mutex> g(g_pinned_mu);
    const char *c = static_cast<const char *>(p);
    for (auto const &r : g_pinned)
        if (c >= r.first && c + n <= r.first + r.second) return true;
    return false;
}

// The tuning knobs of a context, once: the key of bvc_set_tuning, the environment variable a new context starts from (or none), the
// accepted values lo, lo + step, .. hi, the default, the member of LaunchState.  (include/bvc.h describes them.)
namespace {
struct Knob {
    const char *key, *env;
    int lo, hi, step, dflt;
    int LaunchState::*member;
    bool takes(int v) const { return v >= lo && v <= hi && (v - lo) % step == 0; }
};
const Knob kKnobs[] = {
    {"em_waves_per_cu", "BVC_EM_WAVES_PER_CU", 0, 32, 1, 0, &LaunchState::em_waves_per_cu},
    {"em_wpb", "BVC_EM_WPB", 1, 4, 3, 4, &LaunchState::em_wpb},                       // 1 or 4
    {"hist_split", "BVC_HIST_SPLIT", 0, 64, 1, 0, &LaunchState::hist_split},
    {"group_pipe", "BVC_GROUP_PIPE", 0, 1, 1, 1, &LaunchState::group_pipe},
    {"group_copies_log2", "BVC_GROUP_LOG2C", -1, 5, 1, -1, &LaunchState::group_log2c},
    {"group_big_lds", "BVC_GROUP_BIG_LDS", 0, 1, 1, 1, &LaunchState::group_big_lds},
    {"group_h16", "BVC_GROUP_H16", 0, 1, 1, 0, &LaunchState::group_h16},
    {"em_streams", "BVC_EM_STREAMS", 0, 3, 1, 0, &LaunchState::em_streams},
    {"em_engine", "BVC_EM_ENGINE", 0, 1, 1, 0, &LaunchState::em_engine},
    {"em_tiny_regions", "BVC_EM_TINY_REGIONS", 0, 1, 1, 0, &LaunchState::em_tiny_regions},
    {"em_prune", "BVC_EM_PRUNE", 0, 1, 1, 1, &LaunchState::em_prune},
    {"bgzf_codes", "BVC_BGZF_CODES", 0, 1, 1, 0, &LaunchState::bgzf_codes},
    {"bgzf_parse", "BVC_BGZF_PARSE", 0, 1, 1, 0, &LaunchState::bgzf_parse},
    {"bgzf_cuts", "BVC_BGZF_CUTS", 0, 1, 1, 0, &LaunchState::bgzf_cuts},
    {"csr_scatter_max", "BVC_CSR_SCATTER_MAX", 0, 1 << 30, 1, 64, &LaunchState::csr_scatter_max},
    {"stats_copies_log2", "BVC_STATS_LOG2C", 0, kStatsMaxLog2c, 1, 2, &LaunchState::stats_log2c},
    {"host_chunk_kib", nullptr, 1, 1 << 21, 1, 1 << 19, &LaunchState::host_chunk_kib},
};
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
    // starting values of the tuning knobs (bvc_set_tuning changes them per context; results never depend on them): a variable that is
    // not set, or holds a value its knob does not take, leaves the default
    for (const Knob &k : kKnobs) {
        const char *e = k.env ? getenv(k.env) : nullptr;
        ctx->ls.*k.member = e && k.takes(atoi(e)) ? atoi(e) : k.dflt;
    }
#ifdef BVC_DIAG_KNOBS
    // timing experiments only (tools/em_stage2.py phase breakdown): cuts region_kernel short, so the records are WRONG.  Not
    // compiled into the product: a stray environment variable must never be able to do that.
    ctx->ls.dbg_levels = env_int("BVC_DBG_LEVELS", 0, 12, 0);
#endif
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
    (void)sync_streams(ctx);
    for (hipStream_t s : {ctx->side, ctx->side_b, ctx->side_c, ctx->copy, ctx->own_stream})
        if (s) (void)hipStreamDestroy(s);
    if (ctx->ev_wait) (void)hipEventDestroy(ctx->ev_wait);
    for (int b = 0; b < bvc_ctx::kRing; ++b) {
        if (ctx->ev_hist_done[b]) (void)hipEventDestroy(ctx->ev_hist_done[b]);
        if (ctx->ev_em_done[b]) (void)hipEventDestroy(ctx->ev_em_done[b]);
    }
    for (int b = 0; b < 2; ++b) {
        if (ctx->ev_upload[b]) (void)hipEventDestroy(ctx->ev_upload[b]);
        if (ctx->ev_set_free[b]) (void)hipEventDestroy(ctx->ev_set_free[b]);
    }
    for (auto &t : ctx->ev_pending) give_back(ctx, t);
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
    BVC_HIP(ctx, sync_streams(ctx));
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return BVC_OK;
}

int bvc_synchronize(bvc_ctx *ctx)
{
    if (!ctx) return BVC_ERR_ARG;
    BVC_HIP(ctx, hipSetDevice(ctx->device));
    BVC_HIP(ctx, sync_streams(ctx));
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
    BVC_HIP(ctx, sync_streams(ctx));
    reap_timing(ctx, true);
    *out = ctx->prof;
    if (reset) ctx->prof = bvc_profile{};
    return BVC_OK;
}

int bvc_set_tuning(bvc_ctx *ctx, const char *key, int value)
{
    if (!ctx) return BVC_ERR_ARG;
    if (!key) return fail(ctx, BVC_ERR_ARG, "null tuning key");
    BVC_HIP(ctx, hipSetDevice(ctx->device));                     // "em_streams" joins the side streams of THIS device
    for (const Knob &k : kKnobs) {
        if (std::strcmp(key, k.key) != 0 || !k.takes(value)) continue;
        if (k.member == &LaunchState::em_streams) {              // no stage 2 in flight while the streams it alternates between change
            const int rc = join_side(ctx);
            if (rc != BVC_OK) return rc;
        }
        ctx->ls.*k.member = value;
        return BVC_OK;
    }
    return fail(ctx, BVC_ERR_ARG, "unknown tuning key or value out of range");
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
    // the other translation units: folded into the histogram unit's count, the first violation kept
    hipError_t (*const folded[])(uint32_t *, bool) = {debug_read_pileup, debug_read_inflate, debug_read_site_stats, debug_read_vcf_samples,
                                                      debug_read_bgzf_deflate, debug_read_bgzf_dynamic, debug_read_bgzf_fields};
    for (auto *read : folded) {
        uint32_t pl[8];
        BVC_HIP(ctx, read(pl, reset != 0));
        if (pl[0]) { if (out24[0] == 0) for (int i = 1; i < 8; ++i) out24[i] = pl[i]; out24[0] += pl[0]; }
    }
    return BVC_OK;
}
#endif

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
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, bases, quals, ref_base, ref_base);
    if (rc != BVC_OK) return rc;
    BVC_HIP(ctx, launch_synth_dense(ctx->stream, seed, site0, n_sites, n_samples, row_stride, cov_thr16, bases, quals,
                                    ref_base));
    return BVC_OK;
}

}  // extern "C"
