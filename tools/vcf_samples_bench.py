#!/usr/bin/env python3
"""vcf_samples_kernel alone (bvc_vcf_samples_csr, device pointers): the rate at which the called sites' sample columns are written.

  python tools/vcf_samples_bench.py [--sites 4000] [--samples 100000] [--out profiles/vcf_samples/kernel.txt]

Three shapes: `--sites` sites of `--samples` samples at 10 % coverage of which 2 % and 100 % are called, and one called site of a million
samples.  Per shape a warm-up and three timed calls (HIP events on the context's stream; the call's own wait for the sum of the slots is
inside the interval); the median is reported with the algorithmic bytes -- 4 N + 13 n written and 12 n read per called site -- as GB/s
and as a fraction of the 8 TB/s HBM peak.  The first called site's text is checked for its length and its field count.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3
PEAK = 8e12


def shape_inputs(torch, np, ns, n, called_every, seed):
    """ns sites of n samples, one entry in every ten samples (sample 10 k + a random digit), every called_every-th site called."""
    from basevarc_amd.lib import SITE_DTYPE
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = n // 10
    samples = torch.empty((ns, k), dtype=torch.int32, device="cuda")
    step = torch.arange(k, dtype=torch.int32, device="cuda") * 10
    rows = max(1, (1 << 26) // max(1, k))
    for s0 in range(0, ns, rows):
        m = min(rows, ns - s0)
        samples[s0:s0 + m] = step + torch.randint(0, 10, (m, k), generator=g, device="cuda", dtype=torch.int32)
    entries = torch.randint(0, 256, (ns * k, 8), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    entries[:, 0] = entries[:, 0] & 3
    offs = (torch.arange(ns + 1, dtype=torch.int64, device="cuda") * k).contiguous()
    res = np.zeros(ns, dtype=SITE_DTYPE)
    res["called"][::called_every] = 1
    res["n_alt"] = 1; res["alt_base"] = (2, -1, -1)
    res_t = torch.from_numpy(np.frombuffer(res.tobytes(), dtype=np.uint8).copy()).cuda()
    ref_t = torch.zeros(ns, dtype=torch.int8, device="cuda")
    return offs, entries.reshape(-1), samples.reshape(-1), ref_t, res_t, int(res["called"].sum()), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_samples", "kernel.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from basevarc_amd import Context
    from basevarc_amd.lib import vcf_samples_slot
    ctx = Context(0, stream=torch.cuda.current_stream())
    lines = ["# tools/vcf_samples_bench.py: bvc_vcf_samples_csr with device pointers, 10 % coverage; per row a warm-up, then "
             f"{REPEATS} calls timed with HIP events (plan launches, the wait for the sum of the slots and the formatting launch)",
             "# bytes = (4 N + 13 n) written + 12 n read per called site; of peak = against 8 TB/s",
             f"{'sites':>6s} {'called':>6s} {'samples':>8s} {'ms (3 repeats)':>26s} {'ms':>8s} {'MB':>8s} {'GB/s':>7s} {'of peak':>8s}"]
    for ns, n, every in ((a.sites, a.samples, 50), (a.sites, a.samples, 1), (1, 1_000_000, 1)):
        offs, e_t, s_t, ref_t, res_t, called, k = shape_inputs(torch, np, ns, n, every, 1)
        need = called * vcf_samples_slot(n, k)
        text_t = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
        off_t = len_t = None
        ms = []
        for rep in range(REPEATS + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            text_t, off_t, len_t = ctx.vcf_samples_csr_device(offs, e_t, s_t, ref_t, res_t, n, text_t, off_t, len_t)
            t1.record()
            torch.cuda.synchronize()
            if rep:
                ms.append(t0.elapsed_time(t1))
        assert int(off_t[-1]) == need and int(len_t[0]) == 4 * n + 13 * k - 1
        first = bytes(text_t[:int(len_t[0])].cpu().numpy())
        assert first.count(b"\t") == n - 1 and first.count(b":") == 3 * k, "the first site's text is not n fields with k covered"
        med = sorted(ms)[len(ms) // 2]
        nbytes = called * (4 * n + 13 * k + 12 * k)
        lines.append(f"{ns:6d} {called:6d} {n:8d} {' '.join(f'{x:8.3f}' for x in ms):>26s} {med:8.3f} {nbytes / 1e6:8.1f} "
                     f"{nbytes / (med * 1e-3) / 1e9:7.0f} {nbytes / (med * 1e-3) / PEAK:8.3f}")
        del e_t, s_t, text_t
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
