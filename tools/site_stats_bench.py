#!/usr/bin/env python3
"""site_stats_kernel alone (bvc_site_stats_csr, device pointers): every site called, `--entries` entries a site, next to a plain
streaming read of the same bytes (bvc_stream_read_ms).

Two inputs of the same shape answer what the number of LDS copies of the counters (tuning key "stats_copies_log2") is chosen by:

  mapq equal     every mapping quality 60 (qual and rpr random): the column a wavefront's vote collapses to one add
  mapq uniform   every field a uniformly random byte: no vote helps, every lane adds for itself

  python tools/site_stats_bench.py [--sites 4000] [--entries 100000] [--out profiles/site_stats/kernel.txt]

Per input and copy count a warm-up and three timed calls (HIP events on the context's stream); the median is reported with the fraction
of the streaming read's time.  The records of all copy counts must be the same bytes.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3


def entries_of(torch, n, equal_mapq, seed):
    """n bvc_pileup_entry records on the device: nine in ten the reference base A, the others G (the alternative) or C (neither)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    e = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    chunk = 1 << 26
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        u = torch.randint(0, 100, (m,), generator=g, device="cuda", dtype=torch.int32)
        e[c0:c0 + m, 0] = torch.where(u < 90, 0, torch.where(u < 98, 2, 1)).to(torch.uint8)
        for col in (1, 2, 3):
            e[c0:c0 + m, col] = torch.randint(0, 256, (m,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
        e[c0:c0 + m, 4] = torch.randint(0, 2, (m,), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    if equal_mapq:
        e[:, 1] = 60
    return e.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=4000)
    ap.add_argument("--entries", type=int, default=100_000)
    ap.add_argument("--copies", default="0,1,2,3,4", help="log2 of the LDS copies to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_stats", "kernel.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from basevarc_amd import Context
    from basevarc_amd.lib import SITE_DTYPE
    ctx = Context(0, stream=torch.cuda.current_stream())
    ns, n = a.sites, a.entries
    offs = (torch.arange(ns + 1, dtype=torch.int64, device="cuda") * n).contiguous()
    res = np.zeros(ns, dtype=SITE_DTYPE)
    res["called"] = 1; res["n_alt"] = 1; res["alt_base"] = (2, -1, -1)
    res_t = torch.from_numpy(np.frombuffer(res.tobytes(), dtype=np.uint8).copy()).cuda()
    ref_t = torch.zeros(ns, dtype=torch.int8, device="cuda")
    nbytes = ns * n * 8
    lines = [f"# tools/site_stats_bench.py: {ns} called sites x {n} entries = {nbytes / 1e9:.2f} GB of entries; device pointers",
             f"# per row a warm-up, then {REPEATS} calls timed with HIP events; ms = their median; stream = bvc_stream_read_ms over the same bytes",
             f"{'input':14s} {'copies':>6s} {'ms (3 repeats)':>26s} {'ms':>8s} {'GB/s':>7s} {'stream ms':>9s} {'of stream':>9s}"]
    for name, equal in (("mapq equal", True), ("mapq uniform", False)):
        e_t = entries_of(torch, ns * n, equal, 1)
        torch.cuda.synchronize()
        stream_ms = nbytes / (ctx.stream_read_gbs(e_t, repeats=3) * 1e9) * 1e3
        first = None
        for log2c in [int(x) for x in a.copies.split(",")]:
            ctx.set_tuning("stats_copies_log2", log2c)
            out = ctx.site_stats_csr_device(offs, e_t, ref_t, res_t)
            torch.cuda.synchronize()
            ms = []
            for _ in range(REPEATS):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                out = ctx.site_stats_csr_device(offs, e_t, ref_t, res_t, stats_t=out)
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1))
            rec = out.cpu().numpy().tobytes()
            first = first or rec
            assert rec == first, "the records depend on the number of copies"
            med = sorted(ms)[len(ms) // 2]
            lines.append(f"{name:14s} {1 << log2c:6d} {' '.join(f'{x:8.3f}' for x in ms):>26s} {med:8.3f} {nbytes / (med * 1e-3) / 1e9:7.0f} "
                         f"{stream_ms:9.3f} {med / stream_ms:9.2f}")
        del e_t
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
