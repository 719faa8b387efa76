#!/usr/bin/env python3
"""`BaseVarC popmatrix` with BVC_HOST_DEVICE_POPMATRIX at 0 and at 1 (needs a gfx950 device): the whole process on the 100 test BAMs and
on a list that names each of them several times, with a position file of every tenth position of the test region; and bvc_bam_popmatrix
alone on the inflated records of the 100 test BAMs in device memory, for that position list and for the one tools/bam_pileup_bench.py
gives bvc_bam_pileup.

  python tools/popmatrix_bench.py [--copies 50] [--repeats 3] [--out profiles/popmatrix/README.txt]

The larger list repeats the same files: the page cache serves both runs alike.  Every process time is the best of --repeats wall-clock
runs, start-up and the context's creation included.  Knob 0 is the reference's serial algorithm on one thread."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bam_pileup_bench import Lines  # noqa: E402


def sites():
    """[(pos, ref, alt)]: every tenth position of hostref.REGION whose reference base is one of ACGT."""
    from tests import hostref
    from tests import popmatrix_model as pm
    from tests.golden import make_testdata_pileup as tp
    _, start, _, refseq = hostref.region_fixture()
    _, s, e = tp.REGION
    return pm.refalt([p for p in range(s, e, 10) if refseq[p - start] in "ACGT"], start, refseq)


def process_seconds(exe, lst, fa, posfile, out, knob, repeats):
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        r = subprocess.run([exe, "popmatrix", "-q", "20", "-i", lst, "-p", posfile, "-r", fa, "-o", out], capture_output=True, text=True,
                           env=dict(os.environ, BVC_HOST_DEVICE_POPMATRIX=str(knob)))
        dt = time.perf_counter() - t
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        best = dt if best is None else min(best, dt)
    return best


def kernel_alone(lines, repeats):
    import numpy as np
    import torch
    from basevarc_amd import Context
    from tests import popmatrix_model as pm
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    contig, beg0, end0, mapq, pv_all, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    bam = b"".join(d for d, _, _ in data)
    off, end, at, n_records = [], [], 0, 0
    for d, first, _ in data:
        off.append(at + first)
        at += len(d)
        end.append(at)
        q = first
        while q < len(d):
            q += 4 + int.from_bytes(d[q:q + 4], "little")
            n_records += 1
    dev = lambda a: torch.from_numpy(a).cuda()
    ctx = Context(0)
    d_bam = dev(np.frombuffer(bam, dtype=np.uint8).copy())
    head = (d_bam, dev(np.array(off, dtype=np.int64)), dev(np.array(end, dtype=np.int64)), torch.ones(len(data), dtype=torch.uint8, device="cuda"),
            dev(np.array([refs.index(contig) for _, _, refs in data], dtype=np.int32)), beg0, end0, mapq)
    lines.append(f"bvc_bam_popmatrix alone, device pointers, 100 samples, {len(bam)} inflated bytes, {n_records} alignment records "
                 "(index + one resolve pass + the statuses' scan, one wait):")
    for name, positions in (("every 10th position of the region", [p for p, _, _ in sites()]), ("bvc_bam_pileup's position list", pv_all)):
        pv = pm.refalt(positions, rg_s, refseq)
        args = head + (dev(np.array([p for p, _, _ in pv], dtype=np.int32)), dev(np.array([ord(r) for _, r, _ in pv], dtype=np.uint8)),
                       dev(np.array([ord(x) for _, _, x in pv], dtype=np.uint8)), rg_s, len(refseq))
        rc, mat, st = ctx.bam_popmatrix(*args)                           # sizes the scratch
        assert rc == 0
        best = None
        for _ in range(repeats + 2):
            ctx.synchronize()
            t = time.perf_counter()
            ctx.bam_popmatrix(*args, matrix=mat, sample_status=st)
            ctx.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        lines.append(f"  {name}, {len(pv)} positions: {best * 1e3:.2f} ms a call, {n_records / best / 1e6:.2f} M alignment records/s, "
                     f"{len(bam) / best / 1e9:.3f} GB/s of BAM bytes, {len(pv) * len(data) / best / 1e6:.1f} M (position, sample) cells/s")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from basevarc_amd import build as b
    from tests import hostref
    exe, _ = b.build_host()
    lines = Lines()
    lines.append("# popmatrix with BVC_HOST_DEVICE_POPMATRIX = 0 | 1: tools/popmatrix_bench.py, best of %d runs, seconds of the whole process" % a.repeats)
    with tempfile.TemporaryDirectory() as d:
        fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
        lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
        big = os.path.join(d, "big.list")
        with open(big, "w") as f:
            f.write(open(lst).read() * a.copies)
        pv = sites()
        pos = os.path.join(d, "sites.pos")
        with open(pos, "w") as f:
            f.write("".join(f"chr17\t{p}\t{r}\t{x}\n" for p, r, x in pv))
        lines.append(f"position file: {len(pv)} lines (every 10th position of {hostref.REGION}); -q 20; batches of 100 with the knob on")
        lines.append(f"  {'samples':>40s} {'knob 0':>9s} {'knob 1':>9s} {'1 / 0':>7s}")
        for name, path in (("100 (the test BAMs)", lst), (f"{100 * a.copies} (each test BAM {a.copies} times)", big)):
            t0 = process_seconds(exe, path, fa, pos, os.path.join(d, "o0.gz"), 0, a.repeats)
            t1 = process_seconds(exe, path, fa, pos, os.path.join(d, "o1.gz"), 1, a.repeats)
            lines.append(f"  {name:>40s} {t0:9.2f} {t1:9.2f} {t1 / t0:7.2f}")
    kernel_alone(lines, a.repeats)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
