#!/usr/bin/env python3
"""Phase 1 of `BaseVarC basetype` with BVC_HOST_DEVICE_PILEUP at 0 and at 1 (needs a gfx950 device): the load phase (--load) of the host
program on the 100 test BAMs and on a larger list that names each of them several times, at 1, 4 and 8 threads; and bvc_bam_pileup alone
on the inflated records of the 100 test BAMs in device memory, next to a plain streaming read of the same bytes.

  python tools/bam_pileup_bench.py [--copies 20] [--repeats 3] [--out profiles/bam_pileup/README.txt]
  python tools/bam_pileup_bench.py --form text [--copies 50] [--out profiles/bam_pileup_text/README.txt]

  python tools/bam_pileup_bench.py --deflate 1 --form bin|text [--codes 1] [--tokens 1] [--copies 50] [--out profiles/bam_pileup_deflate/README.txt]

--form text: the same with --tmp-format text and BVC_HOST_DEVICE_PILEUP_TEXT, and bvc_bam_pileup_text next to bvc_bam_pileup on the same
input, with the bytes of text a second.

--deflate 1 (--form bin or text): the table of BVC_HOST_DEVICE_PILEUP_DEFLATE -- per thread count the CPU path (every knob 0), the pileup
knob alone, and the pileup knob with the deflate knob (--codes 1: and with _CODES; --tokens 1, text: and with _TOKENS), the rows in turn within
one session: seconds of the whole --load process, its CPU seconds (user + system of the child), the bytes of the batch files it leaves, and
(--phase2 1) the positions a second of the slowest position loop of a run with every knob off that reads those files (--rerun).

The larger list repeats the same files (and so the same sample names, which the load phase does not look at): the page cache serves both
runs alike.  Every time is the best of --repeats wall-clock runs of the whole process, start-up and the context's creation included."""
import argparse
import glob
import os
import re
import resource
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Lines(list):
    """The report's lines, shown as they come."""

    def append(self, line):
        list.append(self, line)
        print(line, flush=True)


KNOB = dict(raw="BVC_HOST_DEVICE_PILEUP", bin="BVC_HOST_DEVICE_PILEUP", text="BVC_HOST_DEVICE_PILEUP_TEXT")
DEFLATE_KNOBS = ("BVC_HOST_DEVICE_PILEUP", "BVC_HOST_DEVICE_PILEUP_TEXT", "BVC_HOST_DEVICE_PILEUP_DEFLATE", "BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES",
                 "BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS")


def load_seconds(exe, lst, fa, region, out, threads, batch, knob, fmt, repeats):
    best = None
    for _ in range(repeats):
        t = time.perf_counter()
        r = subprocess.run([exe, "basetype", "--load", "--tmp-format", fmt, "-q", "20", "-t", str(threads), "-b", str(batch), "-i", lst, "-s", region,
                            "-r", fa, "-o", out], capture_output=True, text=True, env=dict(os.environ, **{KNOB[fmt]: str(knob)}))
        dt = time.perf_counter() - t
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        best = dt if best is None else min(best, dt)
    return best


def deflate_variants(fmt, codes, tokens):
    """[(row name, the knobs at 1)]: the CPU path, the parent's device path, and the deflate knob alone and with what was asked for."""
    pile, z = KNOB[fmt], "BVC_HOST_DEVICE_PILEUP_DEFLATE"
    rows = [("cpu path", ()), ("pileup", (pile,)), ("pileup + deflate", (pile, z))]
    if codes:
        rows.append(("+ codes", (pile, z, z + "_CODES")))
    if tokens and fmt == "text":
        rows.append(("+ tokens", (pile, z, z + "_TOKENS")))
        if codes:
            rows.append(("+ codes + tokens", (pile, z, z + "_CODES", z + "_TOKENS")))
    return rows


def deflate_table(lines, exe, lst, fa, region, d, fmt, batch, codes, tokens, repeats, phase2, n_positions, thread_counts=(1, 4, 8)):
    """One line a (threads, row): best wall seconds of --load, the CPU seconds of that run, the batch files' bytes, phase 2's loop rate."""
    lines.append(f"  {'threads':>7s} {'row':<18s} {'load s':>8s} {'cpu s':>8s} {'batch bytes':>13s} {'/ level 6':>9s} {'phase-2 pos/s':>14s}")
    for threads in thread_counts:
        level6 = None
        for name, on in deflate_variants(fmt, codes, tokens):
            env = dict(os.environ, **{k: "1" if k in on else "0" for k in DEFLATE_KNOBS})
            out = os.path.join(d, "z_" + re.sub(r"\W+", "_", name))
            cmd = [exe, "basetype", "--tmp-format", fmt, "-q", "20", "-t", str(threads), "-b", str(batch), "-i", lst, "-s", region, "-r", fa, "-o", out]
            best = None
            for _ in range(repeats):
                before = resource.getrusage(resource.RUSAGE_CHILDREN)
                t = time.perf_counter()
                r = subprocess.run(cmd + ["--load", "--keep_tmp"], capture_output=True, text=True, env=env)
                dt = time.perf_counter() - t
                after = resource.getrusage(resource.RUSAGE_CHILDREN)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                cpu = after.ru_utime + after.ru_stime - before.ru_utime - before.ru_stime
                best = (dt, cpu) if best is None or dt < best[0] else best
            size = sum(os.path.getsize(f) for f in glob.glob(out + ".tmp.thread.*/batch.*"))
            level6 = size if level6 is None else level6                  # (the first row: zlib level 6 on the CPU)
            rate = "-"
            if phase2:
                off = dict(os.environ, BVC_HOST_PROFILE="1", **{k: "0" for k in DEFLATE_KNOBS})
                r = subprocess.run(cmd + ["--rerun"], capture_output=True, text=True, env=off)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                loops = [float(m.group(1)) for m in (re.search(r"position loop ([0-9.e+-]+) s", l) for l in r.stderr.splitlines()) if m]
                rate = f"{n_positions / max(loops):.0f}" if loops else "-"
            for f in glob.glob(out + "*"):
                shutil.rmtree(f) if os.path.isdir(f) else os.remove(f)
            lines.append(f"  {threads:7d} {name:<18s} {best[0]:8.2f} {best[1]:8.2f} {size:13d} {size / level6:9.3f} {rate:>14s}")


def kernel_pair(lines, repeats, text=False):
    import numpy as np
    import torch
    from basevarc_amd import Context
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    bam = b"".join(d for d, _, _ in data)
    off, end, at = [], [], 0
    n_records = 0
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
    args = (d_bam, dev(np.array(off, dtype=np.int64)), dev(np.array(end, dtype=np.int64)), torch.ones(len(data), dtype=torch.uint8, device="cuda"),
            dev(np.array([refs.index(contig) for _, _, refs in data], dtype=np.int32)), beg0, end0, mapq, dev(np.array(pv, dtype=np.int32)), rg_s,
            dev(np.frombuffer(refseq.encode(), dtype=np.uint8).copy()))
    rc, rec, rs, st, need = ctx.bam_pileup(*args)                        # sizes the scratch and the records
    assert rc == 0
    best = None
    for _ in range(repeats + 2):
        ctx.synchronize()
        t = time.perf_counter()
        ctx.bam_pileup(*args, records=rec, rec_start=rs, sample_status=st)
        ctx.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    gbs = ctx.stream_read_gbs(d_bam, repeats=5)
    lines.append(f"bvc_bam_pileup alone, device pointers, 100 samples x {len(pv)} positions, {len(bam)} inflated bytes, {n_records} alignment records, "
                 f"{need} bytes of position records:")
    lines.append(f"  {best * 1e3:.2f} ms a call (index + two passes of sizes + placement, one wait): {n_records / best / 1e6:.2f} M alignment records/s, "
                 f"{len(bam) / best / 1e9:.3f} GB/s of BAM bytes, {len(pv) * len(data) / best / 1e6:.1f} M (position, sample) cells/s")
    lines.append(f"  bvc_stream_read_ms on the same bytes: {gbs:.0f} GB/s")
    if text:
        rc, txt, ls, st, need = ctx.bam_pileup_text(*args)               # sizes the lines
        assert rc == 0
        tbest = None
        for _ in range(repeats + 2):
            ctx.synchronize()
            t = time.perf_counter()
            ctx.bam_pileup_text(*args, text=txt, line_start=ls, sample_status=st)
            ctx.synchronize()
            dt = time.perf_counter() - t
            tbest = dt if tbest is None else min(tbest, dt)
        lines.append(f"bvc_bam_pileup_text alone on the same input, {need} bytes of text:")
        lines.append(f"  {tbest * 1e3:.2f} ms a call (index + two passes of sizes + filler rows + tokens, one wait): {need / tbest / 1e9:.3f} GB/s of text, "
                     f"{len(pv) * len(data) / tbest / 1e6:.1f} M (position, sample) cells/s, {tbest / best:.2f} x the binary call")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--form", choices=("raw", "bin", "text"), default="raw")
    ap.add_argument("--deflate", type=int, choices=(0, 1), default=0)
    ap.add_argument("--codes", type=int, choices=(0, 1), default=0)
    ap.add_argument("--tokens", type=int, choices=(0, 1), default=0)
    ap.add_argument("--phase2", type=int, choices=(0, 1), default=1)
    ap.add_argument("--threads", default="1,4,8", help="--deflate 1: the thread counts of the table")
    a = ap.parse_args()
    if a.deflate and a.form == "raw":
        ap.error("--deflate 1 takes --form bin or text (raw ignores the knob)")
    from basevarc_amd import build as b
    from tests import hostref
    exe, _ = b.build_host()
    lines = Lines()
    if a.deflate:
        from tests.test_bam_pileup_abi import bam_data_call
        n_positions = len(bam_data_call()[4])
        lines.append("# phase 1 with BVC_HOST_DEVICE_PILEUP_DEFLATE: tools/bam_pileup_bench.py --deflate 1, best of %d runs of the whole --load process" % a.repeats)
        with tempfile.TemporaryDirectory() as d:
            fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
            lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
            big = os.path.join(d, "big.list")
            with open(big, "w") as f:
                f.write(open(lst).read() * a.copies)
            lines.append(f"{100 * a.copies} samples (each test BAM {a.copies} times), batches of 100, --tmp-format {a.form}")
            deflate_table(lines, exe, big, fa, hostref.REGION, d, a.form, 100, a.codes, a.tokens, a.repeats, a.phase2, n_positions,
                          tuple(int(t) for t in a.threads.split(",")))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    lines.append("# phase 1 (bt_r) with %s = 0 | 1: tools/bam_pileup_bench.py, best of %d runs, seconds of the whole --load process" % (KNOB[a.form], a.repeats))
    with tempfile.TemporaryDirectory() as d:
        fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
        lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
        big = os.path.join(d, "big.list")
        with open(big, "w") as f:
            f.write(open(lst).read() * a.copies)
        for name, path, batch in (("100 test BAMs, batches of 10", lst, 10), (f"{100 * a.copies} samples (each test BAM {a.copies} times), batches of 100", big, 100)):
            lines.append(f"{name}, --tmp-format {a.form}")
            lines.append(f"  {'threads':>7s} {'knob 0':>9s} {'knob 1':>9s} {'1 / 0':>7s}")
            for threads in (1, 4, 8):
                t0 = load_seconds(exe, path, fa, hostref.REGION, os.path.join(d, "o0"), threads, batch, 0, a.form, a.repeats)
                t1 = load_seconds(exe, path, fa, hostref.REGION, os.path.join(d, "o1"), threads, batch, 1, a.form, a.repeats)
                lines.append(f"  {threads:7d} {t0:9.2f} {t1:9.2f} {t1 / t0:7.2f}")
    kernel_pair(lines, a.repeats, a.form == "text")
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
