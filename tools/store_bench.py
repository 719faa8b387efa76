#!/usr/bin/env python3
"""`BaseVarC basetype --tmp-format mem` (the batches stay on the device, include/bvc_store.h) next to the two fastest forms that go through
temp files (needs a gfx950 device): the whole process on a list that names each of the 100 test BAMs several times, at 1, 4 and 8
threads; and bvc_pileup_begin_store alone on a tile of 32 MB from 200 batches, next to bvc_pileup_begin_bin of the same tile from host
memory and a device-to-device copy of the same bytes.

  python tools/store_bench.py [--copies 50] [--repeats 3] [--out profiles/store_feed/README.txt]
  python tools/store_bench.py --gather-only          # the tile alone: under `rocprofv3 --kernel-trace --stats -- python ...` the
                                                     # row of store_gather_kernel is the gather kernel's own time
  python tools/store_bench.py --windows 4 [--overlap] [--out profiles/store_windows/README.txt]
                                                     # mem in one window (the yardstick), in K position windows (BVC_HOST_STORE_WINDOWS)
                                                     # and, with --overlap, in K windows with the next one loaded beside this one's threads
                                                     # (BVC_HOST_STORE_OVERLAP); beside each the largest store's bytes and the windows'
                                                     # load and compute seconds, from the profile lines of one more run

Every process time is the best of --repeats wall-clock runs of the whole program, start-up and the contexts' creation included; the page
cache serves all forms alike (the larger list repeats the same files)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = (("text (default)", ["--tmp-format", "text"], {}),
         ("raw, BVC_HOST_DEVICE_PILEUP=1", ["--tmp-format", "raw"], {"BVC_HOST_DEVICE_PILEUP": "1"}),
         ("mem", ["--tmp-format", "mem"], {}))


class Lines(list):
    """The report's lines, shown as they come."""

    def append(self, line):
        list.append(self, line)
        print(line, flush=True)


def run_seconds(exe, lst, fa, region, out, threads, batch, extra, env, repeats):
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        r = subprocess.run([exe, "basetype", "-q", "20", "-t", str(threads), "-b", str(batch), "-i", lst, "-s", region, "-r", fa, "-o", out] + extra,
                           capture_output=True, text=True, env=dict(os.environ, **env))
        dt = time.perf_counter() - t
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        best = dt if best is None else min(best, dt)
    return best


def windows_report(lines, exe, lst, fa, region, d, copies, windows, overlap, repeats):
    """mem in one window, in `windows` windows and (overlap) in windows loaded beside the threads: the whole process, best of `repeats`;
    then one run of each with BVC_HOST_PROFILE=1 for the stores' bytes and the windows' seconds (not timed: the profile costs)."""
    import re
    forms = [("mem, 1 window", {"BVC_HOST_STORE_WINDOWS": "1"}), (f"mem, {windows} windows", {"BVC_HOST_STORE_WINDOWS": str(windows)})]
    if overlap:
        forms.append((f"mem, {windows} windows, overlap", {"BVC_HOST_STORE_WINDOWS": str(windows), "BVC_HOST_STORE_OVERLAP": "1"}))
    lines.append(f"{100 * copies} samples (each test BAM {copies} times), batches of 100")
    lines.append(f"  {'threads':>7s} " + " ".join(f"{name:>30s}" for name, _ in forms))
    detail = []
    for threads in (1, 4, 8):
        ts = []
        for i, (name, env) in enumerate(forms):
            out = os.path.join(d, f"w{i}")
            ts.append(run_seconds(exe, lst, fa, region, out, threads, 100, ["--tmp-format", "mem"], env, repeats))
            r = subprocess.run([exe, "basetype", "-q", "20", "-t", str(threads), "-b", "100", "-i", lst, "-s", region, "-r", fa, "-o", out,
                                "--tmp-format", "mem"], capture_output=True, text=True, env=dict(os.environ, BVC_HOST_PROFILE="1", **env))
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            per = re.findall(r"window (\d+) of \d+: .*?, (\d+) bytes, load ([0-9.e+-]+) s, compute ([0-9.e+-]+) s", r.stderr)
            whole = re.search(r"batches kept there \(bvc_bam_pileup_bgzf_store\), (\d+) bytes", r.stderr)
            largest = max(int(b) for _, b, _, _ in per) if per else int(whole.group(1))
            detail.append(f"  {threads} threads, {name}: largest store {largest} bytes" +
                          ("; per window load / compute s: " + ", ".join(f"{float(a):.3f} / {float(c):.3f}" for _, _, a, c in per) if per else ""))
        lines.append(f"  {threads:7d} " + " ".join(f"{t:30.2f}" for t in ts))
    lines.extend(detail)


def gather_alone(lines, repeats, n_batches=200, tile_mb=32):
    import numpy as np
    import torch
    from basevarc_amd import Context, Store
    P, k = 512, max(1, (tile_mb << 20) // (n_batches * 512 * 9))
    rng = np.random.default_rng(1)
    rec = np.zeros((P, 4 + 9 * k), dtype=np.uint8)
    rec[:, :4] = np.frombuffer(np.uint32(9 * k).tobytes(), dtype=np.uint8)
    ent = rec[:, 4:].reshape(P, k, 9)
    ent[:, :, :4] = np.arange(k, dtype=np.uint32).view(np.uint8).reshape(k, 4)     # sample in batch, ascending
    ent[:, :, 4] = rng.integers(0, 4, size=(P, k))                                 # base
    ent[:, :, 5:8] = rng.integers(0, 42, size=(P, k, 3))                           # mapq, qual, rpr
    ent[:, :, 8] = rng.integers(0, 2, size=(P, k))                                 # strand
    body = rec.tobytes()
    step = 4 + 9 * k
    ctx = Context(0)
    st = Store(0, P, n_batches)
    batches = []
    for b in range(n_batches):
        filler = b % 16
        rs = (filler + step * np.arange(P + 1)).astype(np.uint32)
        batches.append((b"\xEE" * filler + body, rs))
        st.put(ctx, b, k, *batches[-1])
    st.seal(ctx)
    T, nbytes = st.tile(0, P, 1 << 40)
    assert T == P

    def best_of(fn):
        best = None
        for _ in range(repeats + 2):
            ctx.synchronize()
            t = time.perf_counter()
            fn()
            ctx.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best
    t_store = best_of(lambda: ctx.pileup_begin_store(st, 0, P))
    data = b"".join(r[int(rs[0]):int(rs[P])] for r, rs in batches)
    rows = np.stack([len(body) * b + (rs.astype(np.int64) - int(rs[0])) for b, (_, rs) in enumerate(batches)]).astype(np.uint32)
    s0 = (k * np.arange(n_batches)).astype(np.int32)
    nib = np.full(n_batches, k, dtype=np.int32)
    buf = np.frombuffer(data, dtype=np.uint8)
    ne, ni = C.c_int64(0), C.c_int64(0)
    t_bin = best_of(lambda: ctx._check(ctx._L.bvc_pileup_begin_bin(ctx._h, buf.ctypes.data, len(buf), rows.ctypes.data, s0.ctypes.data, nib.ctypes.data,
                                                                   n_batches, P, C.byref(ne), C.byref(ni))))
    src = torch.from_numpy(buf.copy()).cuda()
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_copy = None
    for _ in range(repeats + 2):
        torch.cuda.synchronize()
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        dt = ev[0].elapsed_time(ev[1]) * 1e-3
        t_copy = dt if t_copy is None else min(t_copy, dt)
    lines.append(f"one tile of {P} positions from {n_batches} batches kept on the device, {len(data)} bytes of records ({nbytes} with the pads' bound):")
    lines.append(f"  bvc_pileup_begin_store (plan + table + gather + count pass, one wait): {t_store * 1e3:.2f} ms a call, {len(data) / t_store / 1e9:.1f} GB/s of records")
    lines.append(f"  bvc_pileup_begin_bin of the same tile from host memory (upload + count pass, one wait): {t_bin * 1e3:.2f} ms a call")
    lines.append(f"  device-to-device copy of the same bytes (torch copy_, stream events): {t_copy * 1e3:.3f} ms, {len(data) / t_copy / 1e9:.0f} GB/s")
    st.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gather-only", action="store_true")
    ap.add_argument("--windows", type=int, default=0, help="K: mem in one window next to mem in K position windows, nothing else")
    ap.add_argument("--overlap", action="store_true", help="with --windows: and K windows with BVC_HOST_STORE_OVERLAP=1")
    a = ap.parse_args()
    from basevarc_amd import build as b
    from tests import hostref
    exe, _ = b.build_host()
    lines = Lines()
    lines.append("# `BaseVarC basetype`, whole process: tools/store_bench.py, best of %d runs, seconds" % a.repeats)
    if a.windows > 1:
        with tempfile.TemporaryDirectory() as d:
            fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
            lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
            big = os.path.join(d, "big.list")
            with open(big, "w") as f:
                f.write(open(lst).read() * a.copies)
            windows_report(lines, exe, big, fa, hostref.REGION, d, a.copies, a.windows, a.overlap, a.repeats)
    elif not a.gather_only:
        with tempfile.TemporaryDirectory() as d:
            fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
            lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
            big = os.path.join(d, "big.list")
            with open(big, "w") as f:
                f.write(open(lst).read() * a.copies)
            lines.append(f"{100 * a.copies} samples (each test BAM {a.copies} times), batches of 100")
            lines.append(f"  {'threads':>7s} " + " ".join(f"{name:>30s}" for name, _, _ in FORMS))
            for threads in (1, 4, 8):
                ts = [run_seconds(exe, big, fa, hostref.REGION, os.path.join(d, f"o{i}"), threads, 100, extra, env, a.repeats)
                      for i, (_, extra, env) in enumerate(FORMS)]
                lines.append(f"  {threads:7d} " + " ".join(f"{t:30.2f}" for t in ts))
    if a.windows <= 1:
        gather_alone(lines, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
