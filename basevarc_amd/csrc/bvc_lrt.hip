// bvc_lrt.hip -- the two stages (histogram pass, EM/LRT) on every form of input: dense tiles and ragged columns, plain and with sample
// groups, from device pointers or from host pointers through the context's staging sets.
#include "bvc_ctx.h"

namespace {

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
    const int rc = ensure_joined(ctx, buf, need);
    if (rc != BVC_OK) return rc;
    *out = buf.p;
    return BVC_OK;
}

// The two stages of one call on device pointers.  `stage1(hist)` launches the histogram pass (dense, ragged, ...) on the
// context's stream into a buffer of the ring -- the counts, or with n_groups > 0 the group histograms; `stage2(s2, slot)`
// launches the EM/LRT on the same stream, or in overlap mode on a side stream (of em_stream(ctx, em_streams)) behind an event.
// grp_in: the group histograms are the caller's (bvc_lrt_hist_groups): stage 1 has nothing to fill and stage 2 only reads them.
template <class Stage1, class Stage2>
int run_stages(bvc_ctx *ctx, int64_t n_sites, int n_groups, bool zero_counts, double min_af, int em_streams, Stage1 stage1,
               Stage2 stage2, const uint32_t *grp_in = nullptr)
{
    const size_t cbytes = (size_t)n_sites * BVC_NCLASS * sizeof(uint32_t), gbytes = cbytes * (size_t)(n_groups + 1);
    const int buf = ctx->overlap ? ctx->flip : 0;
    if (ctx->overlap) ctx->flip = (ctx->flip + 1) % bvc_ctx::kRing;
    DevBuf &cnt = ctx->d_cnt[buf], &grp = ctx->d_grp[buf];
    int rc = ensure_joined(ctx, cnt, cbytes);
    if (rc == BVC_OK && n_groups > 0 && !grp_in) rc = ensure_joined(ctx, grp, gbytes);
    RingSlot slot;
    if (rc == BVC_OK) rc = em_scratch_for(ctx, buf, n_sites, min_af, &slot.em);
    if (rc == BVC_OK && n_groups > 0) rc = em_scratch_for(ctx, buf, n_sites, min_af, &slot.emg, n_groups);
    if (rc != BVC_OK) return rc;
    slot.counts = reinterpret_cast<uint32_t *>(cnt.p);
    if (n_groups > 0) slot.grp = grp_in ? const_cast<uint32_t *>(grp_in) : reinterpret_cast<uint32_t *>(grp.p);
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

// Host-pointer dense tiles (bvc_lrt_dense, bvc_lrt_dense_packed, the group calls): site chunks of at most host_chunk_kib per
// array through two staging sets.  `n_rows` row arrays (2: bases and quals, 1: packed rows); with n_groups > 0 the group vector
// `labels` goes up and the group records come down too.  `device(ns, set)` runs the two stages on a chunk staged in `set`.
template <class Device>
int run_dense_host(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride, int n_rows, const int8_t *const rows[2],
                   const int8_t *ref_base, const uint8_t *labels, int n_groups, bvc_site_result *results, bvc_group_result *grp_results,
                   Device device)
{
    const int64_t row_bytes = row_stride > 0 ? row_stride : 1;
    int64_t chunk = ((int64_t)ctx->ls.host_chunk_kib << 10) / row_bytes;
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
                     bvc_site_result *res, bvc_group_result *gres, const uint32_t *grp_in = nullptr)
{
    return run_stages(ctx, ns, n_groups, false, min_af, 2, stage1, [&](hipStream_t s2, const RingSlot &slot) -> int {
        BVC_HIP(ctx, launch_sum_groups(s2, ns, n_groups + 1, slot.grp, slot.counts));
        const bool shared = ctx->overlap && long_rows;
        const int per_launch = kGroupSharedWavesPerCu / em_stream_count(ctx, 2) > 2 ? kGroupSharedWavesPerCu / em_stream_count(ctx, 2) : 2;
        BVC_HIP(ctx, launch_lrt(ctx->ls, s2, ns, slot.counts, BVC_NCLASS, r, min_af, ctx->d_lut, nullptr, nullptr, res, shared, per_launch,
                                slot.em));
        BVC_HIP(ctx, launch_lrt_groups(ctx->ls, s2, ns, n_groups, slot.grp, r, min_af, ctx->d_lut, res, gres, shared, per_launch, slot.emg));
        return BVC_OK;
    }, grp_in);
}

// The group calls on ragged columns with a sample index per observation.
int run_csr_groups_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
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


// One per-observation array of a host-pointer ragged group call: the caller's array, its element size, its staged copy.
struct ObsArray { const void *host; size_t elem; void *dev; };

// A ragged group call on host pointers, in one piece through staging set 0: the offsets, ref_base, the label vector of the samples (n_samples = 0:
// the call has none) and the per-observation `arrays` go up, `device(offsets, ref_base, group_of_sample, results, grp_results)` runs the two stages
// on the staged copies and the two record arrays come down.  Every staged array starts on a 256-byte boundary.
template <class Device>
int run_csr_groups_host(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *ref_base, const uint8_t *group_of_sample,
                        int64_t n_samples, ObsArray *arrays, int n_arrays, int32_t n_groups, bvc_site_result *results,
                        bvc_group_result *grp_results, Device device)
{
    const size_t total = (size_t)offsets[n_sites];
    int64_t *d_o; int8_t *d_r; uint8_t *d_g; bvc_site_result *d_res; bvc_group_result *d_gres;
    int rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_o = L.take<int64_t>((size_t)n_sites + 1);
        d_r = L.take<int8_t>((size_t)n_sites);
        d_g = L.take<uint8_t>((size_t)n_samples, 1);
        for (int a = 0; a < n_arrays; ++a) arrays[a].dev = L.take<char>(total * arrays[a].elem, 16);
        d_res = L.take<bvc_site_result>((size_t)n_sites);
        d_gres = L.take<bvc_group_result>((size_t)n_sites * n_groups);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_o, offsets, (size_t)(n_sites + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    if (n_samples) BVC_HIP_D(ctx, hipMemcpyAsync(d_g, group_of_sample, (size_t)n_samples, hipMemcpyHostToDevice, ctx->stream));
    for (int a = 0; a < n_arrays && total; ++a)
        BVC_HIP_D(ctx, hipMemcpyAsync(arrays[a].dev, arrays[a].host, total * arrays[a].elem, hipMemcpyHostToDevice, ctx->stream));
    rc = device(d_o, d_r, d_g, d_res, d_gres);
    if (rc == BVC_OK) rc = join_side(ctx);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(grp_results, d_gres, (size_t)n_sites * n_groups * sizeof(bvc_group_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
    return BVC_OK;
}

}  // namespace

int run_csr_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const int8_t *bases, const int8_t *quals,
                   const int8_t *ref_base, double min_af, const int8_t *comb, const uint8_t *n_comb,
                   bvc_site_result *results)
{
    return run_two_stages(ctx, n_sites, false, false,
                          [&](uint32_t *counts) { return launch_hist_csr(ctx->ls, ctx->stream, n_sites, offsets, bases, quals, counts); },
                          ref_base, min_af, comb, n_comb, results);
}

int run_csr_labels_device(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const uint8_t *obs, const uint8_t *quals,
                          const uint8_t *group_of_obs, const int8_t *ref_base, double min_af, int32_t n_groups,
                          bvc_site_result *results, bvc_group_result *grp_results)
{
    return run_group_stages(ctx, n_sites, n_groups, false,
                            [&](uint32_t *gp) {
                                return launch_hist_csr_labels(ctx->ls, ctx->stream, n_sites, offsets, obs, quals, group_of_obs, n_groups, gp);
                            },
                            ref_base, min_af, results, grp_results);
}

extern "C" {

int bvc_lrt_dense(bvc_ctx *ctx, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                  const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                  double min_af, bvc_site_result *results, uint32_t flags)
{
    // rows of zero samples carry no data: their pointers may be null
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? bases : ref_base, n_samples ? quals : ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
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
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? (const void *)packed : (const void *)ref_base, ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
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
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? (const void *)packed : (const void *)counts, counts, counts, counts);
    if (rc != BVC_OK) return rc;
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
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? (const void *)bases : (const void *)counts,
                         n_samples ? (const void *)quals : (const void *)counts, counts, counts);
    if (rc != BVC_OK) return rc;
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

// Stage 2 of the group calls on the caller's group histograms [n_sites][n_groups + 1][512] (slot n_groups: the samples in no group), as
// bvc_counts_add_dense_groups / bvc_counts_add_csr_group_labels accumulate them: run_group_stages with no stage 1.  The overall counts are
// summed into the context's ring; grp_counts is only read.
int bvc_lrt_hist_groups(bvc_ctx *ctx, int64_t n_sites, const uint32_t *grp_counts, const int8_t *ref_base, double min_af, int32_t n_groups,
                        bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    int rc = check_common(ctx, n_sites, grp_counts, ref_base, results, results);
    if (rc != BVC_OK) return rc;
    if ((rc = check_n_groups(ctx, n_groups)) != BVC_OK) return rc;
    if (!grp_results) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    if (n_sites == 0) return BVC_OK;
    auto run_device = [&](const uint32_t *g, const int8_t *r, bvc_site_result *res, bvc_group_result *gres) {
        return run_group_stages(ctx, n_sites, n_groups, false, [](uint32_t *) { return hipSuccess; }, r, min_af, res, gres, g);
    };
    if (flags & BVC_PTR_DEVICE) return run_device(grp_counts, ref_base, results, grp_results);
    const size_t gwords = (size_t)n_sites * (size_t)(n_groups + 1) * BVC_NCLASS;
    uint32_t *d_g; int8_t *d_r; bvc_site_result *d_res; bvc_group_result *d_gres;
    rc = carve(ctx, ctx->d_stage[0], 256, [&](Layout &L) {
        d_g = L.take<uint32_t>(gwords);
        d_r = L.take<int8_t>((size_t)n_sites);
        d_res = L.take<bvc_site_result>((size_t)n_sites);
        d_gres = L.take<bvc_group_result>((size_t)n_sites * n_groups);
    });
    if (rc != BVC_OK) return rc;
    BVC_HIP_D(ctx, hipMemcpyAsync(d_g, grp_counts, gwords * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(d_r, ref_base, (size_t)n_sites, hipMemcpyHostToDevice, ctx->stream));
    rc = run_device(d_g, d_r, d_res, d_gres);
    if (rc == BVC_OK) rc = join_side(ctx);
    if (rc != BVC_OK) return drain_on_error(ctx, rc);
    BVC_HIP_D(ctx, hipMemcpyAsync(results, d_res, (size_t)n_sites * sizeof(bvc_site_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipMemcpyAsync(grp_results, d_gres, (size_t)n_sites * n_groups * sizeof(bvc_group_result), hipMemcpyDeviceToHost, ctx->stream));
    BVC_HIP_D(ctx, hipStreamSynchronize(ctx->stream));
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
    const int64_t target = (int64_t)ctx->ls.host_chunk_kib << 10;
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

// ---- ragged group calls (run_csr_groups_device and run_csr_groups_host above) ----------------------------------------------
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
    ObsArray arr[3] = {{bases, 1, nullptr}, {quals, 1, nullptr}, {sample_of_obs, 4, nullptr}};
    return run_csr_groups_host(ctx, n_sites, offsets, ref_base, group_of_sample, n_samples, arr, 3, n_groups, results, grp_results,
                               [&](const int64_t *o, const int8_t *r, const uint8_t *g, bvc_site_result *res, bvc_group_result *gres) {
                                   return run_csr_groups_device(ctx, n_sites, o, static_cast<const int8_t *>(arr[0].dev),
                                                                static_cast<const int8_t *>(arr[1].dev), static_cast<const int32_t *>(arr[2].dev),
                                                                r, min_af, g, n_samples, n_groups, res, gres);
                               });
}

// ---- ragged group calls with one label byte per observation ------------------------------------------------------------------
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
    ObsArray arr[3] = {{obs, 1, nullptr}, {group_of_obs, 1, nullptr}, {quals, 1, nullptr}};      // the quals: only with n_arrays == 2
    return run_csr_groups_host(ctx, n_sites, offsets, ref_base, nullptr, 0, arr, n_arrays + 1, n_groups, results, grp_results,
                               [&](const int64_t *o, const int8_t *r, const uint8_t *, bvc_site_result *res, bvc_group_result *gres) {
                                   return run_csr_labels_device(ctx, n_sites, o, static_cast<const uint8_t *>(arr[0].dev),
                                                                quals ? static_cast<const uint8_t *>(arr[2].dev) : nullptr,
                                                                static_cast<const uint8_t *>(arr[1].dev), r, min_af, n_groups, res, gres);
                               });
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

// bvc_lrt_dense_groups and bvc_lrt_dense_groups_packed: `packed` = the tile is one byte per sample in `bases`
// (base << 6 | qual, include/bvc.h) and `quals` is not used.
static int lrt_groups_impl(bvc_ctx *ctx, bool packed, int64_t n_sites, int64_t n_samples, int64_t row_stride,
                           const int8_t *bases, const int8_t *quals, const int8_t *ref_base,
                           double min_af, const uint8_t *group_of_sample, int32_t n_groups,
                           bvc_site_result *results, bvc_group_result *grp_results, uint32_t flags)
{
    if (packed) quals = bases;
    // rows of zero samples carry no data: their pointers may be null
    int rc = check_dense(ctx, n_sites, n_samples, row_stride, n_samples ? bases : ref_base, n_samples ? quals : ref_base, ref_base, results);
    if (rc != BVC_OK) return rc;
    if (n_groups < 1 || n_groups > BVC_MAX_GROUPS) return fail(ctx, BVC_ERR_ARG, "n_groups must be 1..32");
    if (!group_of_sample || !grp_results) return fail(ctx, BVC_ERR_ARG, "null group pointer");
    if (n_sites == 0) return BVC_OK;
    auto run_device = [&](int64_t ns, const int8_t *b, const int8_t *q, const int8_t *r, const uint8_t *g,
                          bvc_site_result *res, bvc_group_result *gres) -> int {
        const size_t lbytes = group_labels_bytes(n_samples, ns);       // the call's labels clamped to 0..n_groups + a flag per site
        int rc2 = ensure_joined(ctx, ctx->d_grp_labels, lbytes);
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

}  // extern "C"
