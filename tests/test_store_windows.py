"""Position windows of `--tmp-format mem` (BVC_HOST_STORE_WINDOWS), the parts that need no device: the window arithmetic the host program
uses (bvchost_store_windows, bvchost_store_window_ranges) against a plain restatement of thread_window; the knob's refusals, which end the
program before it touches a device; and, with the model of bvc_bam_pileup (tests/bam_pileup_model.py) on the 100 test BAMs, the two facts
the windows rest on: a window's records -- piled up from the records behind the index's offset for the window's start, filtered by the
REGION's start -- are the whole-region call's records for its positions but for the mapq an indel entry inherits, and a sample is empty
in the region exactly when it is empty in every window.  (tests/test_cohort_cases.py has the reads that tell the region's start from the
window's as the filter; the 100 test BAMs hold none.)"""
import ctypes as C
import glob
import os
import struct
import subprocess

import pytest

from tests import bam_pileup_model as bm
from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call


@pytest.fixture(scope="module")
def host():
    from basevarc_amd import build as b
    exe, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_store_windows.restype = C.c_int32
    H.bvchost_store_windows.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    H.bvchost_store_window_ranges.restype = None
    H.bvchost_store_window_ranges.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    H.bvchost_parse_store_windows.restype = C.c_int32
    H.bvchost_parse_store_windows.argtypes = [C.c_char_p, C.c_int32]
    return exe, H


def thread_window(psize, thread, ithread):
    """host/pileup.cpp's thread_window (src/BaseVarC.cpp:399-403 with the clamp), restated"""
    window = psize % thread + psize // thread
    lo = min(psize, ithread * window)
    hi = psize if ithread == thread - 1 else min(psize, (ithread + 1) * window)
    return lo, hi


def store_windows(psize, T, K):
    """host/pileup.cpp's store_windows, restated: window w is the ranges of threads wT .. wT+T-1 of a run with T*K threads"""
    ranges = [thread_window(psize, T * K, j) for j in range(T * K)]
    return [ranges[w * T][0] for w in range(K)], [ranges[w * T + T - 1][1] for w in range(K)]


def store_window_ranges(pv, a, b, beg0, end0):
    """host/pileup.cpp's store_window_ranges, restated: the windows' gather ranges [wbeg, wend), 0-based, tiling [beg0, end0)"""
    wbeg, wend, at = [], [], beg0
    for w in range(len(a)):
        last = w + 1 == len(a) or a[w + 1] == b[w + 1]
        wbeg.append(at)
        at = at if a[w] == b[w] and w > 0 else end0 if last else min(end0, max(at, pv[b[w] - 1]))
        wend.append(at)
    return wbeg, wend


def windows_of(H, psize, T, K):
    a, b = (C.c_int64 * K)(), (C.c_int64 * K)()
    assert H.bvchost_store_windows(psize, T, K, a, b) == 0
    return list(a), list(b)


def fetch_ranges_of(H, pv, a, b, beg0, end0):
    K = len(a)
    wbeg, wend = (C.c_int32 * K)(), (C.c_int32 * K)()
    H.bvchost_store_window_ranges((C.c_int32 * len(pv))(*pv), K, (C.c_int64 * K)(*a), (C.c_int64 * K)(*b), beg0, end0, wbeg, wend)
    return list(wbeg), list(wend)


@pytest.mark.parametrize("psize", [0, 1, 5, 64, 1000, 66615])
def test_the_windows_are_the_ranges_of_a_run_with_t_times_k_threads(host, psize):
    _, H = host
    for T in (1, 2, 4, 8):
        for K in (1, 2, 3, 7, 100):
            a, b = windows_of(H, psize, T, K)
            n = T * K
            ranges = [thread_window(psize, n, j) for j in range(n)]
            for w in range(K):
                mine = ranges[w * T:(w + 1) * T]
                # the ranges of threads wT .. wT+T-1 follow each other, and the window is all of them
                assert all(mine[i][1] == mine[i + 1][0] for i in range(T - 1)), (psize, T, K, w)
                assert (a[w], b[w]) == (mine[0][0], mine[-1][1]), (psize, T, K, w)
                assert 0 <= a[w] <= b[w] <= psize
            # contiguous, ascending, disjoint, covering [0, psize)
            assert a[0] == 0 and b[-1] == psize and all(b[w] == a[w + 1] for w in range(K - 1)), (psize, T, K)
            # empty windows come last only
            empty = [a[w] == b[w] for w in range(K)]
            assert empty == sorted(empty), (psize, T, K)
            if K == 1:
                assert (a[0], b[0]) == (0, psize)


def test_the_arithmetic_refuses_what_the_program_refuses(host):
    _, H = host
    one = (C.c_int64 * 1)()
    assert H.bvchost_store_windows(10, 1, 0, one, one) == -1 and H.bvchost_store_windows(10, 0, 1, one, one) == -1
    assert H.bvchost_store_windows(10, 2, 32769, one, one) == -1 and H.bvchost_store_windows(-1, 1, 1, one, one) == -1
    for text, thread, want in ((None, 1, 1), (b"1", 4, 1), (b"auto", 4, 0), (b"65536", 1, 65536), (b"16384", 4, 16384), (b"16385", 4, -1), (b"0", 1, -1),
                               (b"-2", 1, -1), (b"x", 1, -1), (b"70000", 1, -1), (b"", 1, -1), (b"3x", 1, -1), (b" 3", 1, -1), (b"+3", 1, -1),
                               (b"99999999999", 1, -1), (b"AUTO", 1, -1)):
        assert H.bvchost_parse_store_windows(text, thread) == want, text


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from tests import hostref
    d = tmp_path_factory.mktemp("store_windows")
    return hostref.write_fasta(str(d / "chr17.fa")), hostref.write_bam_list(str(d / "bam.list"))


@pytest.mark.parametrize("value", ["0", "-2", "x", "70000"])
def test_the_knobs_refusals_end_the_program_before_anything_is_written(host, inputs, tmp_path, value):
    from tests import hostref
    exe, _ = host
    fa, lst = inputs
    out = str(tmp_path / "mem")
    r = subprocess.run([exe, "basetype", "-q", "20", "-t", "1", "-b", "25", "-i", lst, "-s", hostref.REGION, "-r", fa, "-o", out, "--tmp-format", "mem"],
                       capture_output=True, text=True, env=dict(os.environ, BVC_HOST_STORE_WINDOWS=value))
    assert r.returncode == 1, (r.returncode, r.stderr[-1000:])
    assert r.stderr.count("\n") == 1 and "BVC_HOST_STORE_WINDOWS" in r.stderr, r.stderr[-1000:]
    assert glob.glob(out + "*") == []


# ---- the model on the 100 test BAMs ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def region():
    """The whole-region call, once: (its arguments, the samples' bytes, [status], {pos: {batch size: the position's masked records}})."""
    call = bam_data_call()
    contig, beg0, end0, mapq, pv, rg_s, refseq = call
    samples = [(d[off:], refs.index(contig)) for d, off, refs in bam_data_bytes()]
    status, maps = per_sample(samples, beg0, end0, mapq, pv, rg_s, refseq)
    whole = entries_by_position(maps)
    return call, samples, status, {p: {batch: records_of(e, batch) for batch in BATCHES} for p, e in whole.items()}


@pytest.fixture(scope="module")
def gathered():
    """What bam_region_blocks starts a window's gathering from, per test BAM: (inflated bytes, the region's reference, its linear index
    from the .bam.bai, {virtual offset: offset in the inflated bytes} of the records)."""
    from tests import bam_files as bf
    from tests import hostref
    out = []
    for (d, _, refs), line in zip(bam_data_bytes(), (l for l in open(os.path.join(hostref.DATA, "bam.list")) if l.strip())):
        path = os.path.join(hostref.DATA, line.strip().replace("data/", "", 1))
        rid = refs.index(bam_data_call()[0])
        out.append((d, rid, bf.read_bai_linear(path + ".bai")[rid], {r[4]: r[6] for r in bf.walk_bam(path)[1]}))
    return out


def window_samples(gathered, wbeg):
    """The samples' bytes from the record the index names for the 16 kbp window of wbeg (clamped to its last window, as bai_linear_offset)"""
    return [(d[at[lin[min(wbeg >> 14, len(lin) - 1)]]:], rid) for d, rid, lin, at in gathered]


def per_sample(samples, beg0, end0, mapq, positions, rg_s, refseq):
    """bam_pileup_model.expected's first half, sample by sample (the batches below share it)"""
    status, maps = [], []
    for data, rid in samples:
        st, rv = bm.scan_sample(data, True, rid, beg0, end0, mapq)
        m = bm.sample_entries(rv, positions, rg_s, refseq) if st == 0 else {}
        assert st in (0, 1) and m is not None
        status.append(st)
        maps.append(m)
    return status, maps


BATCHES = (25, 7)


def entries_by_position(maps):
    """{pos: [(sample, entry)]} in sample order: the columns that bam_pileup_model.expected's second half walks"""
    out = {}
    for s, m in enumerate(maps):
        for p, e in m.items():
            out.setdefault(p, []).append((s, e))
    return out


def records_of(entries, batch):
    """bam_pileup_model.expected's second half for one position and batches of `batch` samples: {batch: the position's record in it}
    (a batch that is not named holds the empty record), with bytes 4..7 (base, mapq, qual, rpr) of every indel entry zeroed: what
    parse_pileup_bin never reads of one.  (Without the mask nothing differs on this data either: none of its indel entries is its
    sample's first entry of a window below, so each inherits the same mapq in both calls.)"""
    payload = {}
    for s, e in entries or ():
        raw = bm.entry_bytes(e, s % batch)
        if e["is_indel"]:
            raw = raw[:4] + b"\0\0\0\0" + raw[8:]
        payload[s // batch] = payload.get(s // batch, b"") + raw
    return {ib: struct.pack("<I", len(v)) + v for ib, v in payload.items()}


@pytest.mark.parametrize("T, K", [(1, 2), (2, 3), (4, 7)])
def test_a_windows_records_are_the_regions_but_for_the_mapq_an_indel_entry_inherits(host, region, gathered, T, K):
    _, H = host
    (contig, beg0, end0, mapq, pv, rg_s, refseq), samples, status, whole = region
    a, b = windows_of(H, len(pv), T, K)
    wbeg, wend = fetch_ranges_of(H, pv, a, b, beg0, end0)
    assert (a, b) == store_windows(len(pv), T, K) and (wbeg, wend) == store_window_ranges(pv, a, b, beg0, end0)
    # the fetch ranges tile the region's; the cut lies between the last position of a window and the first of the next (0-based
    # coordinates: position p is coordinate p - 1)
    assert wbeg[0] == beg0 and wend[-1] == end0 and all(wend[w] == wbeg[w + 1] for w in range(K - 1))
    for w in range(K - 1):
        assert pv[b[w] - 1] - 1 < wend[w] <= pv[a[w + 1]] - 1, w
    empty_everywhere = [True] * len(samples)
    compared = 0
    for w in range(K):
        # (gathered from the window's start, filtered by the region's: host/main.cpp, MemBatches::keep_from)
        st_w, maps_w = per_sample(window_samples(gathered, wbeg[w]), beg0, wend[w], mapq, pv[a[w]:b[w]], rg_s, refseq)
        for s, st in enumerate(st_w):
            empty_everywhere[s] = empty_everywhere[s] and st == 1
        mine = entries_by_position(maps_w)
        assert set(mine) <= set(pv[a[w]:b[w]])
        for p in pv[a[w]:b[w]]:
            if p not in whole and p not in mine:
                continue                                                # (the empty record in every batch, either way)
            for batch in BATCHES:
                assert records_of(mine.get(p), batch) == whole.get(p, {}).get(batch, {}), (w, batch, p)
            compared += 1
    assert compared == len(whole) > 60000
    # a sample is empty in the region exactly when it is empty in every window
    assert empty_everywhere == [st == 1 for st in status]


def test_the_window_arithmetic_and_the_knobs_parsing_under_the_address_sanitizer(tmp_path):
    """host/pileup.cpp's store_windows and store_window_ranges and host/knobs.h's parsing in a stand-alone program
    (tests/cpp/store_windows_main.cpp) built with -fsanitize=address,undefined: every array a heap block of exactly its size."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_dir = os.path.join(root, "basevarc_amd", "host")
    exe = str(tmp_path / "store_windows")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-pthread", "-I", host_dir, "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "store_windows_main.cpp")] +
                          [os.path.join(host_dir, f) for f in ("pileup.cpp", "stats.cpp", "bgzf.cpp", "inflate.cpp")] + ["-lz", "-o", exe])
    r = subprocess.run([exe, "1", "7", "auto", "0", "-2", "x", "70000", "", "12x", "999999999999"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert "144 cases, 0 wrong" in text
    for line in ("1 -> 1", "7 -> 7", "auto -> 0", "0 -> -1", "-2 -> -1", "x -> -1", "70000 -> 70000", " -> -1", "12x -> -1", "999999999999 -> -1", "(unset) -> 1"):
        assert line + "\n" in text, (line, text[:400])
