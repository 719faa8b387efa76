#!/usr/bin/env python3
"""The histogram pass of the ragged group call in its three input forms, on the same observations (device pointers):

  bvc_lrt_csr_groups               base, quality, 4-byte sample index + a gathered label byte   6 algorithmic bytes per observation
  bvc_lrt_csr_group_labels         base, quality, label byte                                    3
  bvc_lrt_csr_group_labels_packed  base << 6 | quality, label byte                              2

Shape: bench.py's csr_groups5_coverage10pct leg -- 4000 ragged sites of N = 1e6 samples at 10 % coverage (about 1e5 observations
each), k = 5 groups interleaved, every 10th sample in no group.  Per form a warm-up and three repeats; the time of the histogram
pass is the library's own (bvc_set_profiling / bvc_get_profile: HIP events around stage 1, the chip to itself), the call's time is
the wall clock.  The three record sets must be the same bytes.  A fourth row runs the label form on arrays 1, 2 and 3 bytes behind
their allocations: no common alignment, so hist_csr_labels_kernel takes its byte loads -- what its 4-byte loads are worth.

  python tools/csr_labels_bench.py [--sites 4000] [--samples 1000000] [--out profiles/csr_labels/README.txt]

The rule the producer follows: bvc_pileup_finish writes label bytes and calls the label form if that form's histogram
pass is not slower than the sample-index form's by more than the spread of that form's three repeats.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
K = 5
REPEATS, CALLS = 3, 4


def observations(ctx, torch, n_sites, n, seed):
    """bench.py's ragged tile: (offsets, bases, quals, ref, sample_of_obs) on the device."""
    slice_sites = 500
    tmp_b = torch.empty((slice_sites, n), dtype=torch.int8, device="cuda")
    tmp_q = torch.empty((slice_sites, n), dtype=torch.int8, device="cuda")
    r = torch.empty(n_sites, dtype=torch.int8, device="cuda")
    pb, pq, ps, counts = [], [], [], []
    for c0 in range(0, n_sites, slice_sites):
        ns = min(slice_sites, n_sites - c0)
        bb, qq = tmp_b[:ns], tmp_q[:ns]
        ctx.synth_dense_device(seed, 10_000_000 + c0, bb, qq, r[c0:c0 + ns], cov_thr16=int(round(0.1 * 65536)))
        ctx.synchronize()
        m = bb >= 0
        counts.append(m.sum(dim=1))
        pb.append(bb[m]); pq.append(qq[m])
        ps.append(torch.nonzero(m)[:, 1].to(torch.int32))
    offs = torch.zeros(n_sites + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(torch.cat(counts).to(torch.int64), 0)
    return offs, torch.cat(pb), torch.cat(pq), r, torch.cat(ps)


def behind(torch, t, shift):
    """The bytes of t, `shift` bytes behind the start of an allocation of their own."""
    a = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = a[shift:shift + t.numel()]
    v.copy_(t)
    return v


def measure(ctx, torch, call):
    """(ms per call, histogram ms per call) of each repeat, and the records of the last call."""
    out = call()
    ctx.synchronize(); torch.cuda.synchronize()
    wall, hist = [], []
    for _ in range(REPEATS):
        ctx.set_profiling(True)
        ctx.profile(reset=True)
        t0 = time.perf_counter()
        for _ in range(CALLS):
            out = call()
        ctx.synchronize(); torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / CALLS * 1e3)
        p = ctx.profile(reset=True)
        ctx.set_profiling(False)
        assert p["hist_launches"] >= 1, p
        hist.append(p["hist_ms"] / p["hist_launches"])
    return wall, hist, (out[0].cpu().numpy().tobytes(), out[1].cpu().numpy().tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_labels", "README.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from basevarc_amd import Context
    n = a.samples
    min_af = min(0.001, 100.0 / n)
    ctx = Context(0)
    offs, b, q, r, smp = observations(ctx, torch, a.sites, n, a.seed)
    n_obs = int(offs[-1].item())
    assert int(q.max().item()) <= 62, "the packed form holds qualities up to 62"
    lab = (np.arange(n) % K).astype(np.uint8)
    lab[9::10] = 255
    g = torch.from_numpy(lab).cuda()
    g_obs = g[smp.long()]
    packed = (b.to(torch.uint8) << 6) | q.to(torch.uint8)
    vb, vq, vl = behind(torch, b, 1), behind(torch, q, 2), behind(torch, g_obs, 3)
    torch.cuda.synchronize()
    forms = [
        ("bvc_lrt_csr_groups", 6, lambda: ctx.lrt_csr_groups_device(offs, b, q, smp, r, min_af, g, K)),
        ("bvc_lrt_csr_group_labels", 3, lambda: ctx.lrt_csr_group_labels_device(offs, b, q, g_obs, r, min_af, K)),
        ("bvc_lrt_csr_group_labels_packed", 2, lambda: ctx.lrt_csr_group_labels_packed_device(offs, packed, g_obs, r, min_af, K)),
        ("bvc_lrt_csr_group_labels, byte loads", 3, lambda: ctx.lrt_csr_group_labels_device(offs, vb, vq, vl, r, min_af, K)),
    ]
    rows, records = [], []
    for name, nbytes, call in forms:
        wall, hist, rec = measure(ctx, torch, call)
        records.append(rec)
        rows.append((name, nbytes, wall, hist))
    assert all(rec == records[0] for rec in records), "the forms' records differ"
    ctx.close()
    base_hist = rows[0][3]
    spread = max(base_hist) - min(base_hist)
    lines = [f"# tools/csr_labels_bench.py: {a.sites} ragged sites, N = {n} at 10 % coverage = {n_obs} observations ({n_obs / a.sites:.0f} per site), "
             f"k = {K}, every 10th sample in no group; device pointers",
             f"# per form a warm-up, then {REPEATS} repeats of {CALLS} calls; hist = stage 1 alone (HIP events of bvc_set_profiling), "
             f"GB/s = algorithmic bytes / hist, frac = of {HBM_PEAK_GBS:.0f} GB/s; the records of all forms are the same bytes",
             f"{'form':40s} {'B/obs':>5s} {'ms/call (3 repeats)':>26s} {'hist ms (3 repeats)':>26s} {'hist ms':>8s} {'GB/s':>7s} {'frac':>6s}"]
    for name, nbytes, wall, hist in rows:
        med = sorted(hist)[len(hist) // 2]
        gbs = nbytes * n_obs / (med * 1e-3) / 1e9
        lines.append(f"{name:40s} {nbytes:5d} {' '.join(f'{x:8.3f}' for x in wall):>26s} {' '.join(f'{x:8.4f}' for x in hist):>26s} "
                     f"{med:8.4f} {gbs:7.0f} {gbs / HBM_PEAK_GBS:6.3f}")
    med = lambda h: sorted(h)[len(h) // 2]
    ok = med(rows[1][3]) <= med(base_hist) + spread
    lines.append(f"# spread of the sample-index form's repeats: {spread:.4f} ms; label form {med(rows[1][3]):.4f} ms against "
                 f"{med(base_hist):.4f} ms: {'not slower: the producer writes label bytes' if ok else 'SLOWER: the producer stays on sample indices'}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
