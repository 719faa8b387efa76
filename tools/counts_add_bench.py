#!/usr/bin/env python3
"""Stage 1 into accumulating counts (bvc_counts_add_*), the pass alone, device pointers, HIP-event time on the context's stream.

Every figure is the median of three windows of about 200 ms of back-to-back calls; versions that are compared alternate their windows.

  1. cut-over sweep   bvc_counts_add_csr (k = 0) and bvc_counts_add_csr_group_labels (k = 5) on 4000 and 40,000 sites of EXACTLY d
                      observations each, d = 8 .. 4096, with "csr_scatter_max" = 0 (every site through hist_csr_add_kernel: a histogram
                      in LDS per site) and = 1 << 30 (every site through hist_csr_scatter_kernel: one atomic per observation).  The
                      crossing of a configuration is the first d at which the scatter kernel is the slower one by more than the windows' spread; the default of the key
                      is the smallest crossing of the four configurations, halved to the power of two below it (the last d at which
                      scatter won everywhere).
  2. dense chunks     a whole tile by bvc_hist_dense against the same tile added as chunks of 500 / 10,000 / 200,000 columns.
  3. ragged chunks    4000 sites at 10 % coverage: all samples in one bvc_counts_add_csr call against chunks of 500 samples
                      (~50 observations per site and chunk), scatter on (the default) and off.

  python tools/counts_add_bench.py [--out profiles/counts_add/README.txt] [--skip-dense] [--skip-ragged]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTHS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
REPEATS = 3
WINDOW_MS = 200.0               # a timed window holds this much work: shorter ones measure the clock and the scheduler


def window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed(ctx, torch, fn, calls=None):
    """ms per call of one version: (median, spread) of REPEATS windows -- see compared()."""
    return compared(ctx, torch, [(lambda: None, fn)], calls)[0]


def compared(ctx, torch, versions, calls=None):
    """versions: [(prepare, call)].  Per version (median, max - min) of the ms per call of REPEATS windows of back-to-back calls between
    two events; the windows of the versions ALTERNATE, so that what else runs on the machine meets them alike.  A window is `calls`
    calls, by default as many as fill WINDOW_MS (from a warm-up window of 10)."""
    n_calls = []
    for prepare, call in versions:
        prepare()
        window(torch, call, 3)
        est = window(torch, call, 10)
        n_calls.append(calls or max(10, min(20000, int(WINDOW_MS / max(est, 1e-4)))))
    ms = [[] for _ in versions]
    for _ in range(REPEATS):
        for v, (prepare, call) in enumerate(versions):
            prepare()
            ms[v].append(window(torch, call, n_calls[v]))
    return [(sorted(m)[len(m) // 2], max(m) - min(m)) for m in ms]


def uniform_sites(torch, n_sites, depth, k):
    """n_sites sites of `depth` observations: the reference base with 3 % others, qualities 5..41, labels 0..k-1 with a tenth in no group."""
    total = n_sites * depth
    offs = torch.arange(n_sites + 1, dtype=torch.int64, device="cuda") * depth
    ref = torch.randint(0, 4, (n_sites,), dtype=torch.int8, device="cuda")
    b = ref.repeat_interleave(depth)
    other = torch.rand(total, device="cuda") < 0.03
    b = torch.where(other, torch.randint(0, 4, (total,), dtype=torch.int8, device="cuda"), b)
    q = torch.randint(5, 42, (total,), dtype=torch.int8, device="cuda")
    lab = None
    if k:
        lab = torch.randint(0, k, (total,), dtype=torch.uint8, device="cuda")
        lab[torch.rand(total, device="cuda") < 0.1] = 255
    return offs, b, q, lab


def sweep(ctx, torch, lines):
    lines.append("## 1. cut-over sweep: ms per call (median of the windows, +- their spread), every site of the call has exactly d observations")
    lines.append("# hist = \"csr_scatter_max\" 0: one launch of hist_csr_add_kernel; scatter = 1 << 30: one launch of hist_csr_scatter_kernel")
    lines.append(f"{'sites':>6s} {'k':>2s} {'d':>5s} {'hist ms':>9s} {'+-':>7s} {'scatter ms':>10s} {'+-':>7s} {'hist ns/obs':>11s} {'scatter ns/obs':>14s}  faster")
    crossings = {}
    for n_sites in (4000, 40000):
        for k in (0, 5):
            counts = torch.zeros((n_sites, k + 1, 512), dtype=torch.int32, device="cuda")
            first_loss = None
            for d in DEPTHS:
                offs, b, q, lab = uniform_sites(torch, n_sites, d, k)
                if k:
                    call = lambda: ctx.counts_add_csr_group_labels_device(offs, b, q, lab, k, counts)
                else:
                    call = lambda: ctx.counts_add_csr_device(offs, b, q, counts)
                (hist, hist_sp), (scat, scat_sp) = compared(ctx, torch, [(lambda: ctx.set_tuning("csr_scatter_max", 0), call),
                                                                         (lambda: ctx.set_tuning("csr_scatter_max", 1 << 30), call)])
                n_obs = n_sites * d
                noise = max(hist_sp, scat_sp)
                faster = "within the spread" if abs(hist - scat) <= noise else ("scatter" if scat < hist else "hist")
                if faster == "hist" and first_loss is None:
                    first_loss = d
                lines.append(f"{n_sites:6d} {k:2d} {d:5d} {hist:9.4f} {hist_sp:7.4f} {scat:10.4f} {scat_sp:7.4f} {hist * 1e6 / n_obs:11.3f} "
                             f"{scat * 1e6 / n_obs:14.3f}  {faster}")
                del offs, b, q, lab
            crossings[(n_sites, k)] = first_loss
            del counts
            torch.cuda.empty_cache()
    lines.append("# crossing (first d at which scatter is the slower kernel by more than the spread; None: it never was): "
                 + ", ".join(f"{s} sites k={k}: {c}" for (s, k), c in crossings.items()))
    known = [c for c in crossings.values() if c is not None]
    chosen = min(known) // 2 if known else DEPTHS[-1]
    lines.append(f"# csr_scatter_max by the rule (smallest crossing, the power of two below it): {chosen}")
    return chosen


def dense_chunks(ctx, torch, lines, n_sites, n):
    lines.append(f"## 2. dense tile of {n_sites} sites x {n} samples (two bytes per sample), whole and as column chunks: ms per tile")
    b = torch.empty((n_sites, n), dtype=torch.int8, device="cuda")
    q = torch.empty((n_sites, n), dtype=torch.int8, device="cuda")
    r = torch.empty(n_sites, dtype=torch.int8, device="cuda")
    ctx.synth_dense_device(1, 0, b, q, r)
    ctx.synchronize()
    counts = torch.zeros((n_sites, 512), dtype=torch.int32, device="cuda")
    whole, _ = timed(ctx, torch, lambda: ctx.hist_dense_device(b, q, counts))
    lines.append(f"{'bvc_hist_dense, whole tile':44s} {whole:10.3f} ms   {2.0 * n_sites * n / whole / 1e6:8.0f} GB/s")
    once, _ = timed(ctx, torch, lambda: ctx.counts_add_dense_device(b, q, counts))
    lines.append(f"{'bvc_counts_add_dense, whole tile':44s} {once:10.3f} ms   {2.0 * n_sites * n / once / 1e6:8.0f} GB/s")
    for width in (200000, 10000, 500):
        def tile():
            for lo in range(0, n, width):
                ctx.counts_add_dense_device(b[:, lo:lo + width], q[:, lo:lo + width], counts)
        ms, _ = timed(ctx, torch, tile)
        lines.append(f"{'bvc_counts_add_dense, chunks of ' + str(width) + ' columns':44s} {ms:10.3f} ms   {2.0 * n_sites * n / ms / 1e6:8.0f} GB/s"
                     f"   {(n + width - 1) // width} calls, {ms / ((n + width - 1) // width) * 1e3:8.1f} us per call")


def ragged_chunks(ctx, torch, lines, n_sites, n, default_cut):
    lines.append(f"## 3. {n_sites} ragged sites, N = {n} at 10 % coverage, all samples in one call and in chunks of 500 samples: ms per tile")
    width = 500
    whole_b, whole_q, whole_n, chunks = [], [], torch.zeros(n_sites, dtype=torch.int64, device="cuda"), []
    bb = torch.empty((n_sites, width), dtype=torch.int8, device="cuda")
    qq = torch.empty((n_sites, width), dtype=torch.int8, device="cuda")
    r = torch.empty(n_sites, dtype=torch.int8, device="cuda")
    for c in range(n // width):
        ctx.synth_dense_device(7 + c, 0, bb, qq, r, cov_thr16=int(round(0.1 * 65536)))
        ctx.synchronize()
        m = bb >= 0
        per = m.sum(dim=1).to(torch.int64)
        offs = torch.zeros(n_sites + 1, dtype=torch.int64, device="cuda")
        offs[1:] = torch.cumsum(per, 0)
        chunks.append((offs, bb[m].clone(), qq[m].clone()))
        whole_n += per
    # the whole columns: every site's observations of all chunks (their order within a site does not matter to a count)
    woffs = torch.zeros(n_sites + 1, dtype=torch.int64, device="cuda")
    woffs[1:] = torch.cumsum(whole_n, 0)
    wb = torch.empty(int(woffs[-1].item()), dtype=torch.int8, device="cuda")
    wq = torch.empty_like(wb)
    at = woffs[:-1].clone()
    for offs, cb, cq in chunks:
        per = offs[1:] - offs[:-1]
        dst = torch.repeat_interleave(at - offs[:-1], per) + torch.arange(cb.numel(), device="cuda")
        wb[dst] = cb
        wq[dst] = cq
        at += per
    n_obs = wb.numel()
    counts = torch.zeros((n_sites, 512), dtype=torch.int32, device="cuda")
    ctx.set_tuning("csr_scatter_max", default_cut)
    ms, _ = timed(ctx, torch, lambda: ctx.counts_add_csr_device(woffs, wb, wq, counts))
    lines.append(f"{'bvc_counts_add_csr, all samples, one call':52s} {ms:10.3f} ms   {n_obs} observations, {n_obs / n_sites:.0f} per site")
    def tile():
        for offs, cb, cq in chunks:
            ctx.counts_add_csr_device(offs, cb, cq, counts)
    cuts = [(f"scatter on (csr_scatter_max {default_cut})", default_cut), ("scatter off (csr_scatter_max 0)", 0),
            ("scatter only (csr_scatter_max 1 << 30)", 1 << 30)]
    times = compared(ctx, torch, [(lambda cut=cut: ctx.set_tuning("csr_scatter_max", cut), tile) for _, cut in cuts])
    check = {}
    for (name, cut), (ms, spread) in zip(cuts, times):
        lines.append(f"{'chunks of 500 samples, ' + name:62s} {ms:10.3f} +- {spread:6.3f} ms   {len(chunks)} calls, {ms / len(chunks) * 1e3:8.1f} us per call, "
                     f"{n_obs / len(chunks) / n_sites:.0f} observations per site and call")
        ctx.set_tuning("csr_scatter_max", cut)
        counts.zero_()
        tile()
        ctx.synchronize()
        check[cut] = counts.clone()
        counts.zero_()
    ctx.counts_add_csr_device(woffs, wb, wq, counts)
    ctx.synchronize()
    assert all(torch.equal(c, counts) for c in check.values()), "the chunked counts differ from the one-piece counts"
    ctx.set_tuning("csr_scatter_max", default_cut)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counts_add", "README.txt"))
    ap.add_argument("--dense-sites", type=int, default=2000)
    ap.add_argument("--dense-samples", type=int, default=1_000_000)
    ap.add_argument("--ragged-sites", type=int, default=4000)
    ap.add_argument("--ragged-samples", type=int, default=200_000)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--skip-ragged", action="store_true")
    a = ap.parse_args()
    import torch
    from basevarc_amd import Context
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream())                      # the events of `timed` are recorded on the stream the calls run on
    lines = ["# tools/counts_add_bench.py: stage 1 into accumulating counts, the pass alone (device pointers, HIP events; median of "
             f"{REPEATS} windows of about {WINDOW_MS:.0f} ms each after a warm-up)"]
    chosen = sweep(ctx, torch, lines)
    if not a.skip_dense:
        dense_chunks(ctx, torch, lines, a.dense_sites, a.dense_samples)
        torch.cuda.empty_cache()
    if not a.skip_ragged:
        ragged_chunks(ctx, torch, lines, a.ragged_sites, a.ragged_samples, chosen)
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
