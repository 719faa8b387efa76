#!/usr/bin/env python3
"""bvc_bam_counts alone (needs a gfx950 device) on the inflated records of the 100 test BAMs in device memory, for bvc_bam_pileup's
position list of the test region, next to bvc_bam_pileup and bvc_bam_popmatrix on the same records in the same run; with n_groups 0 and 5.

  python tools/bam_counts_bench.py [--repeats 5] [--depth G ...] [--out FILE]  # (a) the call alone; --depth G: and bvc_bam_counts_depth
                                                     # (include/bvc_bam_group_depth.h: one slot of counts and the depths of G groups) behind it
  python tools/bam_counts_bench.py --quals Q ...     # and bvc_bam_counts_quals (include/bvc_site_acc_quals.h: narrow rows of Q quality columns) with
                                                     # 0 and 5 groups behind those, 8 fetches of 8,192 rows of an accumulator of Q columns
                                                     # (acc_expand_kernel) and the time to make a wide and a narrow accumulator of the region
  python tools/bam_counts_bench.py --process [--copies 50] [--repeats 3] [--out FILE]
                                                     # (b) the whole `BaseVarC basetype` process with --tmp-format counts next to mem and bin
                                                     # (bin with BVC_HOST_DEVICE_PILEUP=1: its phase 1 on the device like the other two), at
                                                     # 100 samples and at 100 x copies, 1 / 4 / 8 threads, best of --repeats wall-clock runs;
                                                     # and from one more run of each with BVC_HOST_PROFILE=1 the accumulator's, the second
                                                     # pile-up's store's and mem's store's bytes

  python tools/bam_counts_bench.py --pack [--repeats 5] [--out FILE]
                                                     # (e) packed rows (include/bvc_site_acc_pack.h) on the accumulator of the test positions,
                                                     # wide and at 40 columns with 5 groups: the entries and packed bytes beside the dense
                                                     # bytes, bvc_site_acc_pack and bvc_site_acc_add_packed from device pointers, 8,192 rows
                                                     # expanded (acc_expand_kernel) and a streaming read of as many bytes as each accumulator
                                                     # holds; with --kernel-trace DIR: the size, place, scan, dry and add kernels of that run

Every time it prints is the best wall-clock time of a device-pointer call with the context synchronised before and after (as
tools/popmatrix_bench.py and tools/bam_pileup_bench.py take theirs).  At 100 samples that is launch and wait latency, not kernel time: a
counts call is index + dry pass + scan + one wait + add pass.  The kernels' own times come from the same run under the profiler's kernel
trace (HIP's timestamps of every dispatch):

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bam_counts_bench.py

and --kernel-trace DIR, given the same --repeats, --depth and --quals, reads that run's kernel trace back: the add passes' dispatches in the order
the forms ran, each form's fastest, median and slowest dispatch.

The adds are counted by the model (tests/bam_counts_model.py): one per tallied entry and one more per counted observation; the depth form
adds one more per counted observation of a sample that is in a group."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bam_pileup_bench import Lines  # noqa: E402


def best_of(ctx, repeats, call):
    best = None
    for _ in range(repeats + 2):
        ctx.synchronize()
        t = time.perf_counter()
        call()
        ctx.synchronize()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best


def trace_report(a):
    """The add passes of one profiled run, form by form: every form made 1 + (repeats + 2) calls, in the order main() makes them."""
    import csv
    import glob
    import statistics
    files = glob.glob(os.path.join(a.kernel_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one kernel trace expected under {a.kernel_trace}, found {len(files)}")
    rows = list(csv.DictReader(open(files[0])))
    calls = a.repeats + 3
    lines = Lines()
    lines.append(f"# the add passes' kernel times of one profiled run (rocprofv3 --kernel-trace), {calls} dispatches a form: min / median / max, microseconds")
    narrow = [f"bvc_bam_counts_quals, n_quals {q}, n_groups {g}" for q in a.quals for g in (0, 5)]
    # the instantiations of bam_counts_kernel<ADD, CountsKind> (0 Slots, 1 Depth, 2 Narrow) as the trace names them
    for kernel, forms in (("bam_counts_kernel<true, (bvc::CountsKind)0>", ["bvc_bam_counts, n_groups 0", "bvc_bam_counts, n_groups 5"]),
                          ("bam_counts_kernel<true, (bvc::CountsKind)1>", [f"bvc_bam_counts_depth, n_groups {g}" for g in a.depth]),
                          ("bam_counts_kernel<true, (bvc::CountsKind)2>", narrow),
                          # the dry passes, every form's pooled: the wide one serves bvc_bam_counts and bvc_bam_counts_depth
                          ("bam_counts_kernel<false, (bvc::CountsKind)0>", ["the dry pass of the wide forms"] * (2 + len(a.depth))),
                          ("bam_counts_kernel<false, (bvc::CountsKind)2>", ["the dry pass of the narrow forms"] * len(narrow))):
        mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if kernel in r["Kernel_Name"])
        if len(mine) != calls * len(forms):
            raise SystemExit(f"{kernel}: {len(mine)} dispatches in the trace, {calls * len(forms)} expected")
        if len(set(forms)) == 1 and len(forms) > 1:                # (pooled: one line for all of them)
            us = [(e - b) / 1e3 for b, e in mine]
            lines.append(f"  {kernel:46s} {forms[0]:44s} {min(us):8.1f} {statistics.median(us):8.1f} {max(us):8.1f}  ({len(us)} dispatches)")
            continue
        for i, form in enumerate(forms):
            us = [(e - b) / 1e3 for b, e in mine[i * calls:(i + 1) * calls]]
            lines.append(f"  {kernel:46s} {form:44s} {min(us):8.1f} {statistics.median(us):8.1f} {max(us):8.1f}")
    mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "acc_expand_kernel" in r["Kernel_Name"]]
    if mine:
        q = a.quals[0]
        gbs = 8192 * (16 * q + 2048) / (statistics.median(mine) * 1e-6) / 1e9
        lines.append(f"  {'acc_expand_kernel':46s} {f'8,192 rows of {q} columns, {len(mine)} dispatches':44s} {min(mine):8.1f} {statistics.median(mine):8.1f} {max(mine):8.1f}"
                     f"  ({8192 * (16 * q + 2048)} bytes read and written: {gbs:.0f} GB/s at the median)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


PACK_FORMS = (("wide", None, 0), ("40 columns, 5 groups", 40, 5))


def pack_trace_report(a):
    """The packed-rows kernels of one profiled --pack run: per kernel the dispatches in order, the wide accumulator's first."""
    import csv
    import glob
    import statistics
    files = glob.glob(os.path.join(a.kernel_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"one kernel trace expected under {a.kernel_trace}, found {len(files)}")
    rows = list(csv.DictReader(open(files[0])))
    P = 66615
    dense = {"wide": P * 2096, "40 columns, 5 groups": P * (640 + 48 + 80)}
    lines = Lines()
    lines.append("# the packed-rows kernels of one profiled run (rocprofv3 --kernel-trace): min / median / max, microseconds; GB/s = the accumulator's dense "
                 "bytes over the median")
    for kernel in ("acc_pack_kernel<false>", "acc_pack_scan_kernel", "acc_pack_kernel<true>", "acc_add_packed_kernel<false>", "acc_first_fault_kernel",
                   "acc_add_packed_kernel<true>"):
        mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if kernel in r["Kernel_Name"])
        if not mine or len(mine) % len(PACK_FORMS):
            raise SystemExit(f"{kernel}: {len(mine)} dispatches in the trace")
        k = len(mine) // len(PACK_FORMS)
        for i, (form, _, _) in enumerate(PACK_FORMS):
            us = [(e - b) / 1e3 for b, e in mine[i * k:(i + 1) * k]]
            med = statistics.median(us)
            rate = f"  {dense[form] / (med * 1e-6) / 1e9:7.0f} GB/s" if kernel.startswith("acc_pack_kernel") else ""
            lines.append(f"  {kernel:30s} {form:22s} {min(us):8.1f} {med:8.1f} {max(us):8.1f}  ({len(us)} dispatches){rate}")
    mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "acc_expand_kernel" in r["Kernel_Name"]]
    if mine:
        med = statistics.median(mine)
        nbytes = 8192 * (16 * 40 + 2048)
        lines.append(f"  {'acc_expand_kernel':30s} {'8,192 rows, 40 columns':22s} {min(mine):8.1f} {med:8.1f} {max(mine):8.1f}  ({len(mine)} dispatches)"
                     f"  {nbytes / (med * 1e-6) / 1e9:7.0f} GB/s ({nbytes} bytes read and written)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def pack(a):
    import ctypes as C
    import numpy as np
    import torch
    from basevarc_amd import Context, SiteAcc
    from tests import acc_pack_model as am
    from tests import bam_group_depth_model as gm
    from tests import bam_pileup_model as bm
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    rid = [refs.index(contig) for _, _, refs in data]
    n, P = len(data), len(pv)
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    assert exp["rc"] == 0
    labels = (np.arange(n) % 7).astype(np.uint8)
    want_c, want_t, want_d = gm.fold_maps(exp["maps"], pv, labels, 5)
    ctx = Context(0)
    L = ctx._L
    lines = Lines()
    lines.append(f"# packed rows: tools/bam_counts_bench.py --pack, best of {a.repeats + 2} device-pointer calls, wall clock around a synchronised context")
    lines.append(f"{n} samples, {P} positions, -q {mapq}; {int(want_c.sum())} counted observations")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    for form, n_quals, G in PACK_FORMS:
        rows = am.logical_rows(want_c.reshape(P, 512), want_t, want_d if G else None)
        rs, cell, count = am.entries(rows)
        E = len(cell)
        with (SiteAcc.create_quals(0, P, n_quals, G) if n_quals else SiteAcc(0, P)) as acc, \
                (SiteAcc.create_quals(0, P, n_quals, G) if n_quals else SiteAcc(0, P)) as sink:
            acc.add_packed(ctx, rs, cell, count)
            got = acc.pack(ctx)
            assert all(np.array_equal(x, y) for x, y in zip(got, (rs, cell, count)))
            used = acc.bytes()[0]
            packed = 8 * (P + 1) + 6 * E
            lines.append(f"{form}: {E} entries in {int((np.diff(rs) > 0).sum())} rows that hold any; packed {packed} bytes ({8 * (P + 1)} of row_start, {6 * E} of "
                         f"entries), dense {used} bytes on the device, {P * (2048 + 48 + 16 * G)} through bvc_site_acc_get: {used / packed:.1f} x and "
                         f"{P * (2048 + 48 + 16 * G) / packed:.1f} x")
            d_rs = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
            d_cell = torch.zeros(E, dtype=torch.int16, device="cuda")
            d_count = torch.zeros(E, dtype=torch.int32, device="cuda")
            need = C.c_int64(0)
            call = lambda: L.bvc_site_acc_pack(ctx._h, acc._h, 0, P, ptr(d_rs), ptr(d_cell), ptr(d_count), E, C.byref(need), 1)
            assert call() == 0 and need.value == E
            t = best_of(ctx, a.repeats, call)
            assert np.array_equal(d_cell.cpu().numpy().view(np.uint16), cell) and np.array_equal(d_count.cpu().numpy().view(np.uint32), count)
            lines.append(f"  bvc_site_acc_pack, device pointers (size pass, scan, one wait, place pass): {t * 1e3:8.3f} ms a call")
            add = lambda: L.bvc_site_acc_add_packed(ctx._h, sink._h, 0, P, ptr(d_rs), ptr(d_cell), ptr(d_count), E, 1)
            assert add() == 0
            t = best_of(ctx, a.repeats, add)
            lines.append(f"  bvc_site_acc_add_packed, device pointers (dry pass, first fault, one wait, add pass): {t * 1e3:8.3f} ms a call, {E} atomic adds")
            if n_quals:
                t = best_of(ctx, a.repeats, lambda: acc.get(ctx, 1000, 8192))
                lines.append(f"  bvc_site_acc_get, 8,192 rows of {n_quals} columns expanded and brought to the host: {t * 1e3:8.3f} ms a call")
            buf = torch.zeros(used // 4, dtype=torch.int32, device="cuda")
            gbs = ctx.stream_read_gbs(buf, a.repeats)
            lines.append(f"  a streaming read of {used} bytes: {used / gbs / 1e3:8.1f} us ({gbs:.0f} GB/s)")
            del buf
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def process(a):
    import re
    import subprocess
    import tempfile
    from basevarc_amd import build as b
    from tests import hostref
    from tools.store_bench import run_seconds
    exe, _ = b.build_host()
    forms = (("bin, BVC_HOST_DEVICE_PILEUP=1", ["--tmp-format", "bin"], {"BVC_HOST_DEVICE_PILEUP": "1"}), ("mem", ["--tmp-format", "mem"], {}),
             ("counts", ["--tmp-format", "counts"], {}))
    lines = Lines()
    lines.append(f"# `BaseVarC basetype`, whole process: tools/bam_counts_bench.py --process, best of {a.repeats} runs, seconds")
    with tempfile.TemporaryDirectory() as d:
        fa = hostref.write_fasta(os.path.join(d, "chr17.fa"))
        lst = hostref.write_bam_list(os.path.join(d, "bam.list"))
        big = os.path.join(d, "big.list")
        with open(big, "w") as f:
            f.write(open(lst).read() * a.copies)
        for name, path in (("100 samples (the test BAMs)", lst), (f"{100 * a.copies} samples (each test BAM {a.copies} times)", big)):
            lines.append(f"{name}, batches of 100, {hostref.REGION}, -q 20")
            lines.append(f"  {'threads':>7s} " + " ".join(f"{n:>30s}" for n, _, _ in forms))
            for threads in (1, 4, 8):
                ts = [run_seconds(exe, path, fa, hostref.REGION, os.path.join(d, f"o{i}"), threads, 100, extra, env, a.repeats)
                      for i, (_, extra, env) in enumerate(forms)]
                lines.append(f"  {threads:7d} " + " ".join(f"{t:30.2f}" for t in ts))
            for fmt, pattern in (("counts", r"counts pass: .*"), ("mem", r"batches kept there \(bvc_bam_pileup_bgzf_store\), \d+ bytes")):
                r = subprocess.run([exe, "basetype", "-q", "20", "-t", "4", "-b", "100", "-i", path, "-s", hostref.REGION, "-r", fa, "-o", os.path.join(d, "p"),
                                    "--tmp-format", fmt], capture_output=True, text=True, env=dict(os.environ, BVC_HOST_PROFILE="1"))
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                lines.append(f"  {fmt}, 4 threads: " + re.search(pattern, r.stderr).group(0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--copies", type=int, default=50)
    ap.add_argument("--process", action="store_true")
    ap.add_argument("--pack", action="store_true", help="packed rows: bvc_site_acc_pack / bvc_site_acc_add_packed on the test positions' accumulator")
    ap.add_argument("--out", default=None)
    ap.add_argument("--depth", type=int, action="append", default=[], help="also bvc_bam_counts_depth with this many groups (may be given more than once)")
    ap.add_argument("--quals", type=int, action="append", default=[], help="also bvc_bam_counts_quals with this many quality columns, 0 and 5 groups (may be given more than once)")
    ap.add_argument("--kernel-trace", default=None, help="the directory of a rocprofv3 --kernel-trace run of this tool with the same --repeats, --depth and --quals")
    a = ap.parse_args()
    if a.pack:
        a.repeats = 5 if a.repeats is None else a.repeats
        return pack_trace_report(a) if a.kernel_trace else pack(a)
    if a.kernel_trace:
        a.repeats = 5 if a.repeats is None else a.repeats
        return trace_report(a)
    if a.process:
        a.repeats = 3 if a.repeats is None else a.repeats
        return process(a)
    a.repeats = 5 if a.repeats is None else a.repeats
    import numpy as np
    import torch
    from basevarc_amd import Context
    from tests import bam_counts_model as cm
    from tests import bam_pileup_model as bm
    from tests import popmatrix_model as pm
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    bam = b"".join(d for d, _, _ in data)
    off, end, at = [], [], 0
    for d, first, _ in data:
        off.append(at + first)
        at += len(d)
        end.append(at)
    rid = [refs.index(contig) for _, _, refs in data]
    n, P = len(data), len(pv)
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    assert exp["rc"] == 0
    dev = lambda x: torch.from_numpy(x).cuda()
    ctx = Context(0)
    head = (dev(np.frombuffer(bam, dtype=np.uint8).copy()), dev(np.array(off, dtype=np.int64)), dev(np.array(end, dtype=np.int64)),
            torch.ones(n, dtype=torch.uint8, device="cuda"), dev(np.array(rid, dtype=np.int32)), beg0, end0, mapq)
    d_pos = dev(np.array(pv, dtype=np.int32))
    lines = Lines()
    lines.append(f"# bvc_bam_counts alone: tools/bam_counts_bench.py, best of {a.repeats + 2} device-pointer calls, wall clock around a synchronised context")
    lines.append(f"{n} samples, {len(bam)} inflated bytes, {P} positions, -q {mapq}")
    # the two calls it stands between
    d_ref = dev(np.frombuffer(refseq.encode(), dtype=np.uint8).copy())
    rc, rec, rs, st, need = ctx.bam_pileup(*head, d_pos, rg_s, d_ref)
    assert rc == 0
    t_pileup = best_of(ctx, a.repeats, lambda: ctx.bam_pileup(*head, d_pos, rg_s, d_ref, records=rec, rec_start=rs, sample_status=st))
    lines.append(f"  bvc_bam_pileup     {t_pileup * 1e3:8.2f} ms a call ({need} bytes of records)")
    ra = pm.refalt(pv, rg_s, refseq)
    m_args = head + (d_pos, dev(np.array([ord(r) for _, r, _ in ra], dtype=np.uint8)), dev(np.array([ord(x) for _, _, x in ra], dtype=np.uint8)), rg_s, len(refseq))
    rc, mat, st2 = ctx.bam_popmatrix(*m_args)
    assert rc == 0
    t_matrix = best_of(ctx, a.repeats, lambda: ctx.bam_popmatrix(*m_args, matrix=mat, sample_status=st2))
    lines.append(f"  bvc_bam_popmatrix  {t_matrix * 1e3:8.2f} ms a call")
    for n_groups in (0, 5):
        labels = (np.arange(n) % 7).astype(np.uint8) if n_groups else None
        want_c, want_t = cm.fold(exp["maps"], pv, labels, n_groups)
        adds = int(want_c.sum()) + int(want_t["strand_base"].sum()) + int(want_t["n_other"].sum()) + int(want_t["n_indel"].sum())
        d_counts = torch.zeros(P * cm.slots_of(n_groups) * 512, dtype=torch.int32, device="cuda")
        d_tally = torch.zeros(P * 12, dtype=torch.int32, device="cuda")
        kw = dict(group_of_sample=dev(labels) if n_groups else None, n_groups=n_groups, sample_status=st2)
        assert ctx.bam_counts(*head, d_pos, rg_s, len(refseq), d_counts, d_tally, **kw)[0] == 0
        ctx.synchronize()
        assert (d_counts.cpu().numpy().view(np.uint32) == want_c.reshape(-1)).all() and d_tally.cpu().numpy().tobytes() == want_t.tobytes()
        t = best_of(ctx, a.repeats, lambda: ctx.bam_counts(*head, d_pos, rg_s, len(refseq), d_counts, d_tally, **kw))
        lines.append(f"  bvc_bam_counts, n_groups {n_groups}: {t * 1e3:8.2f} ms a call, {adds} atomic adds into {d_counts.numel() * 4 + d_tally.numel() * 4} bytes "
                     f"of accumulators ({adds / t / 1e6:.1f} M adds/s over the whole call)")
    for n_groups in a.depth:
        from tests import bam_group_depth_model as gm
        labels = (np.arange(n) % 7).astype(np.uint8)                  # (the labels of the grouped form above: with 5 groups two of seven are in none)
        want_c, want_t, want_d = gm.fold_maps(exp["maps"], pv, labels, n_groups)
        adds = int(want_c.sum()) + int(want_d.sum()) + int(want_t["strand_base"].sum()) + int(want_t["n_other"].sum()) + int(want_t["n_indel"].sum())
        d_counts = torch.zeros(P * 512, dtype=torch.int32, device="cuda")
        d_tally = torch.zeros(P * 12, dtype=torch.int32, device="cuda")
        d_depth = torch.zeros(P * n_groups * 4, dtype=torch.int32, device="cuda")
        kw = dict(group_of_sample=dev(labels), n_groups=n_groups, sample_status=st2)
        assert ctx.bam_counts_depth(*head, d_pos, rg_s, len(refseq), d_counts, d_tally, d_depth, **kw)[0] == 0
        ctx.synchronize()
        assert (d_counts.cpu().numpy().view(np.uint32) == want_c.reshape(-1)).all() and d_tally.cpu().numpy().tobytes() == want_t.tobytes()
        assert (d_depth.cpu().numpy().view(np.uint32) == want_d.reshape(-1)).all()
        t = best_of(ctx, a.repeats, lambda: ctx.bam_counts_depth(*head, d_pos, rg_s, len(refseq), d_counts, d_tally, d_depth, **kw))
        hot = int(want_d.max())
        lines.append(f"  bvc_bam_counts_depth, n_groups {n_groups}: {t * 1e3:8.2f} ms a call, {adds} atomic adds into "
                     f"{(d_counts.numel() + d_tally.numel() + d_depth.numel()) * 4} bytes of accumulators ({adds / t / 1e6:.1f} M adds/s over the whole call); "
                     f"the most adds of one call into one depth word: {hot}")
    for n_quals in a.quals:
        from basevarc_amd import SiteAcc
        from tests import bam_counts_quals_model as qm
        want = qm.expected(None, None, None, None, pv, None, None, n_quals, exp=exp)
        if want["rc"] != 0:
            raise SystemExit(f"--quals {n_quals}: the records hold a counted quality of {n_quals} or more")
        for n_groups in (0, 5):
            labels = (np.arange(n) % 7).astype(np.uint8)
            want = qm.expected(None, None, None, None, pv, None, None, n_quals, labels, n_groups, exp=exp)
            adds = int(want["counts"].sum()) + (int(want["depth"].sum()) if n_groups else 0) + int(want["tally"]["strand_base"].sum()) + \
                int(want["tally"]["n_other"].sum()) + int(want["tally"]["n_indel"].sum())
            d_counts = torch.zeros(P * 4 * n_quals, dtype=torch.int32, device="cuda")
            d_tally = torch.zeros(P * 12, dtype=torch.int32, device="cuda")
            d_depth = torch.zeros(P * n_groups * 4, dtype=torch.int32, device="cuda") if n_groups else None
            kw = dict(group_depth=d_depth, group_of_sample=dev(labels) if n_groups else None, n_groups=n_groups, sample_status=st2)
            assert ctx.bam_counts_quals(*head, d_pos, rg_s, len(refseq), n_quals, d_counts, d_tally, **kw)[0] == 0
            ctx.synchronize()
            assert (d_counts.cpu().numpy().view(np.uint32) == want["counts"].reshape(-1)).all() and d_tally.cpu().numpy().tobytes() == want["tally"].tobytes()
            assert not n_groups or (d_depth.cpu().numpy().view(np.uint32) == want["depth"].reshape(-1)).all()
            t = best_of(ctx, a.repeats, lambda: ctx.bam_counts_quals(*head, d_pos, rg_s, len(refseq), n_quals, d_counts, d_tally, **kw))
            nbytes = (d_counts.numel() + d_tally.numel() + (d_depth.numel() if n_groups else 0)) * 4
            lines.append(f"  bvc_bam_counts_quals, n_quals {n_quals}, n_groups {n_groups}: {t * 1e3:8.2f} ms a call, {adds} atomic adds into {nbytes} bytes "
                         f"of accumulators ({adds / t / 1e6:.1f} M adds/s over the whole call)")
        # the accumulators: the time to make (and zero) one of each kind for the region, and fetches of 8,192 expanded rows
        made = {}
        for kind, make in (("wide (bvc_site_acc_create)", lambda: SiteAcc(0, P)), (f"{n_quals} columns (bvc_site_acc_create_quals)", lambda: SiteAcc.create_quals(0, P, n_quals))):
            best = None
            for _ in range(a.repeats + 2):
                t = time.perf_counter()
                acc = make()
                dt = time.perf_counter() - t
                used = acc.bytes()[0]
                acc.close()
                best = dt if best is None else min(best, dt)
            made[kind] = (best, used)
            lines.append(f"  an accumulator of {P} positions, {kind}: {best * 1e3:8.2f} ms to make and zero, {used} bytes")
        with SiteAcc.create_quals(0, P, n_quals) as acc:
            t = best_of(ctx, 6, lambda: acc.get(ctx, 1000, 8192))
            lines.append(f"  bvc_site_acc_get, 8,192 rows of {n_quals} columns expanded and brought to the host: {t * 1e3:8.2f} ms a call")
    ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
