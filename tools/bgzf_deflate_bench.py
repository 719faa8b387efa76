#!/usr/bin/env python3
"""The device deflate encoder alone (bvc_bgzf_deflate, device pointers; bgzf_deflate_kernel.hip): the rate at which sample-column text becomes BGZF blocks.

  python tools/bgzf_deflate_bench.py [--samples 100000] [--codes 0|1] [--parse 0|1] [--out profiles/vcf_deflate/kernel.txt]

--codes: the context's tuning key "bgzf_codes" (1: the block kernel's dynamic instantiations, bgzf_block_kernel<*, true>: each block the smallest of stored, fixed and dynamic).
--parse 1: the tuning key "bgzf_parse" at 1 (the field parse, bgzf_block_kernel<true, *>) AGAINST 0 in the same run: every row is timed at
both values in turn -- key 0, key 1, key 0, ... -- and key 1's row ends with its time and its size against key 0's.

The texts are the three of tests/bgzf_deflate_cases.py (one called site's sample columns at coverage 0.10, 0.01 and 1.0), each as one
piece (one called position: 7 - 27 blocks, as many workgroups busy), as seven pieces (a tile's called positions) and as 64 pieces (more
blocks than the chip has CUs).  Per row a warm-up and three timed calls (HIP events on the context's stream; the call's own wait for the
pieces' lengths is inside the interval); the median is reported as input GB/s, with the size of the output against the input and
against zlib at levels 1 and 6 on the same bytes cut at the same marks.  The first row's blocks are inflated and compared.  Beside it:
the host program's BgzfWriter (zlib level 6, foreground: one core) on the same text, MB/s.
"""
import argparse
import ctypes as C
import gzip
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3


def writer_rate(text):
    """BgzfWriter at level 6 on one core: MB/s of input, the median of three."""
    from basevarc_amd import build as b
    _, hostlib = b.build_host()
    H = C.CDLL(hostlib)
    H.bvchost_bgzf_write.restype = C.c_int
    H.bvchost_bgzf_write.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int, C.c_int]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.gz").encode()
        secs = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            assert H.bvchost_bgzf_write(path, text, len(text), 1 << 20, 6, 0) == 1
            secs.append(time.perf_counter() - t0)
    return len(text) / sorted(secs)[len(secs) // 2] / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_deflate", "kernel.txt"))
    ap.add_argument("--codes", type=int, default=0, choices=(0, 1))
    ap.add_argument("--parse", type=int, default=0, choices=(0, 1))
    a = ap.parse_args()
    import numpy as np
    import torch
    from basevarc_amd import Context
    from basevarc_amd.lib import bgzf_blocks, bgzf_bound
    from tests import bgzf_deflate_cases as dc
    ctx = Context(0, stream=torch.cuda.current_stream())
    if a.codes:
        ctx.set_tuning("bgzf_codes", a.codes)
    parses = (0, 1) if a.parse else (0,)
    lines = [f"# tools/bgzf_deflate_bench.py --codes {a.codes} --parse {a.parse}: bvc_bgzf_deflate with device pointers; per row a warm-up, then "
             f"{REPEATS} calls timed with HIP events (the wait for the pieces' lengths and the five launches)",
             "# out/in = packed bytes / input bytes; /z1, /z6 = packed bytes against zlib level 1 and 6 on the same 65280-byte cuts (+ 26 a block)",
             f"{'coverage':>8s} {'pieces':>6s} {'blocks':>6s} {'input MB':>9s} {'ms (3 repeats)':>26s} {'ms':>8s} {'GB/s':>7s} {'out/in':>7s} {'/z1':>6s} "
             f"{'/z6':>6s} {'BgzfWriter level 6, one core MB/s':>34s}" + (f" {'parse':>5s} {'ms / parse 0':>12s} {'size / parse 0':>14s}" if a.parse else "")]
    for coverage, seed, _ in dc.SIZE_TEXTS:
        text = dc.sample_text(a.samples, coverage, seed)
        z1, z6 = dc.zlib_size(text, 1), dc.zlib_size(text, 6)
        cpu = writer_rate(text)
        for copies in (1, 7, 64):
            data_t = torch.from_numpy(np.frombuffer(text * copies, dtype=np.uint8).copy()).cuda()
            off_t = (torch.arange(copies, dtype=torch.int64, device="cuda") * len(text)).contiguous()
            len_t = torch.full((copies,), len(text), dtype=torch.int64, device="cuda")
            comp_t = torch.empty(copies * bgzf_bound(len(text)), dtype=torch.uint8, device="cuda")
            coff_t = None
            ms, packed_of = {p: [] for p in parses}, {}
            for rep in range(REPEATS + 1):
                for parse in parses:                                     # (in turn: whatever drifts, drifts for both)
                    if a.parse:
                        ctx.set_tuning("bgzf_parse", parse)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    comp_t, coff_t = ctx.bgzf_deflate_device(data_t, off_t, len_t, comp_t, coff_t)
                    t1.record()
                    torch.cuda.synchronize()
                    if rep:
                        ms[parse].append(t0.elapsed_time(t1))
                        continue
                    off = coff_t.cpu().numpy()
                    packed_of[parse] = int(off[-1])
                    assert packed_of[parse] == copies * int(off[1])
                    if copies == 1:
                        assert gzip.decompress(bytes(comp_t[:packed_of[parse]].cpu().numpy())) == text, "the blocks do not inflate to the text"
            nbytes = copies * len(text)
            med = {p: sorted(ms[p])[len(ms[p]) // 2] for p in parses}
            for parse in parses:
                packed = packed_of[parse]
                lines.append(f"{coverage:8.2f} {copies:6d} {copies * bgzf_blocks(len(text)):6d} {nbytes / 1e6:9.2f} {' '.join(f'{x:8.3f}' for x in ms[parse]):>26s} "
                             f"{med[parse]:8.3f} {nbytes / (med[parse] * 1e-3) / 1e9:7.2f} {packed / nbytes:7.4f} {packed / copies / z1:6.3f} {packed / copies / z6:6.3f} "
                             f"{cpu:34.1f}" + (f" {parse:5d} {med[parse] / med[0]:12.3f} {packed / packed_of[0]:14.3f}" if a.parse else ""))
            del data_t, comp_t
    ctx.close()
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
