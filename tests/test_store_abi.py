"""Temp batches kept on the device (include/bvc_store.h) as far as a machine without a GPU can see them: the entry points are declared,
exported, in the binding's sixth table and refuse a null context or store; the chunk size and the grid cap the GPU tests straddle are the
library's; the kernels are built from their own source without private memory, scratch, flat addressing or spills; the host program has
its fourth --tmp-format, its knob and the refusals that need no device; and bvc_store_tile's arithmetic (bvc_store_tile_fit, the inline
function the library calls) is held against a plain Python search (tests/store_model.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import store_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_store_create", "bvc_store_destroy", "bvc_store_put", "bvc_bam_pileup_bgzf_store", "bvc_store_get", "bvc_store_seal", "bvc_store_tile",
         "bvc_store_bytes", "bvc_pileup_begin_store"]


def sixth_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_store.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc_store.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(bvc_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        assert name not in decls, name
        decls[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",")])
    return decls


def test_the_library_the_header_and_the_binding_know_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_bam_pileup_abi as tb
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    decls = sixth_header_declarations()
    assert list(decls) == bl.STORE_EXPORTS == NAMES
    # the closed lists stay as they were
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(tb.third_header_declarations()) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    others = set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES) | set(bl.BAM_PROTOTYPES) | set(bl.POPMATRIX_PROTOTYPES) | set(bl.BAM_TEXT_PROTOTYPES)
    assert not set(decls) & others
    returns = dict(ta.RETURNS, void=None)
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.STORE_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is returns[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # the _store call takes bvc_bam_pileup_bgzf's arguments up to refseq_len, name for name
    twin = tb.third_header_declarations()["bvc_bam_pileup_bgzf"][1]
    mine = decls["bvc_bam_pileup_bgzf_store"][1]
    k = next(i for i, p in enumerate(twin) if p.endswith("refseq_len")) + 1
    assert mine[:k] == twin[:k] and [p.split()[-1].lstrip("*") for p in mine[k:]] == ["st", "batch", "records_bytes", "sample_status"]
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc_bam.h"' in open(os.path.join(ROOT, "include", "bvc_store.h")).read() and "bvc_store.h" in header
    for m in ("create", "put", "get", "seal", "tile", "bytes"):
        assert callable(getattr(bl.Store, m, None)), m
    assert callable(getattr(bl.Context, "bam_pileup_bgzf_store", None)) and callable(getattr(bl.Context, "pileup_begin_store", None))
    # no context, no store: refused before anything of the device is touched
    n64, n32 = C.c_int64(7), C.c_int32(7)
    assert L.bvc_store_create(None, 0, 1, 1, 0) == -1
    assert L.bvc_store_put(None, None, 0, 0, None, 0, None) == -1 and L.bvc_store_seal(None, None) == -1
    assert L.bvc_store_get(None, None, 0, None, 0, C.byref(n64), None) == -1
    assert L.bvc_bam_pileup_bgzf_store(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(n64), None) == -1
    assert L.bvc_store_tile(None, 0, 1, 0, C.byref(n32), C.byref(n64)) == -1 and L.bvc_store_bytes(None, C.byref(n64), C.byref(n64)) == -1
    assert L.bvc_pileup_begin_store(None, None, 0, 0, C.byref(n64), C.byref(n64), C.byref(n64)) == -1
    L.bvc_store_destroy(None)


def test_the_sizes_the_gpu_tests_straddle_are_the_librarys():
    from basevarc_amd import lib as bl
    header = open(os.path.join(ROOT, "include", "bvc_store.h")).read()
    internal = open(os.path.join(ROOT, "basevarc_amd", "csrc", "bvc_internal.h")).read()
    assert int(re.search(r"#define BVC_STORE_CHUNK (\d+)", header).group(1)) == bl.STORE_CHUNK
    assert int(re.search(r"constexpr int kStoreGrid = (\d+);", internal).group(1)) == bl.STORE_GRID


def test_the_kernels_are_built_from_their_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "store_kernel.hip" in b.SOURCES and "bvc_store.hip" in b.SOURCES and "store_kernel.hip" in isa_report.DEVICE_SOURCES
    for flags in ((), ("-DBVC_POISON", "-DBVC_CHECK_LDS")):
        rows = {re.match(r"(?:bvc::)?([\w<>]+)", k["pretty"]).group(1): k for k in isa_report.kernels_of(isa_report.assembly("store_kernel.hip", flags))}
        assert set(rows) == {"store_cum_kernel", "store_plan_kernel", "store_rows_kernel", "store_gather_kernel"}, sorted(rows)
        for name, k in rows.items():
            assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["mfma"] == 0, (name, k)
        # both sides of the bulk copy are 16-byte vector accesses; the cumulative sizes are added with 64-bit vector atomics
        m = rows["store_gather_kernel"]["mnemonics"]
        assert m.get("global_load_dwordx4", 0) >= 4 and m.get("global_store_dwordx4", 0) >= 4, m
        assert rows["store_cum_kernel"]["mnemonics"].get("global_atomic_add_x2", 0) == 1


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    from basevarc_amd import build as b
    exe, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_store_tile_fit.restype = C.c_int32
    H.bvchost_store_tile_fit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
    return exe, H


def test_the_host_program_has_its_option_its_knob_and_keeps_the_phase_one_dispatch(host):
    exe, _ = host
    knobs = open(os.path.join(ROOT, "basevarc_amd", "host", "knobs.h")).read()
    assert re.search(r'store_gb = std::max\(0\.0, real\("BVC_HOST_STORE_GB", 0\)\);', knobs)
    main = open(os.path.join(ROOT, "basevarc_amd", "host", "main.cpp")).read()
    # the existing dispatch as it was, the mem branch in front of it
    a, b_, c = main.index("if (in_memory) {"), main.index('knobs.device_pileup && opt::tmp_format != "text"'), main.index(
        'knobs.device_pileup_text && opt::tmp_format == "text"')
    assert a < b_ < c
    feeds = open(os.path.join(ROOT, "basevarc_amd", "host", "feeds.h")).read()
    assert "feed_store_tiles" in feeds and "feed_store_tiles" in main and "TileForm::Stored" in feeds
    r = subprocess.run([exe, "basetype", "--help"], capture_output=True, text=True)
    assert "mem:" in r.stderr and "BVC_HOST_STORE_GB" in r.stderr, r.stderr
    # a fifth value is still refused with the usage
    r = subprocess.run([exe, "basetype", "--tmp-format", "disk", "-i", "x", "-o", "y"], capture_output=True, text=True)
    assert r.returncode == 1 and "--tmp-format" in r.stderr


@pytest.mark.parametrize("extra, line", [(["--load"], "--tmp-format mem with --load"), (["--keep_tmp"], "--tmp-format mem with --keep_tmp"),
                                         (["--gpus", "2"], "--tmp-format mem with --gpus above 1")])
def test_the_refusals_that_need_no_device(host, tmp_path, extra, line):
    """Each is one line on stderr and exit code 1, before a file is opened or a directory made.  (The fourth, a batch over
    BVC_HOST_STORE_GB, needs the device: tests/test_gpu_host_mem.py.)"""
    exe, _ = host
    out = str(tmp_path / "o")
    r = subprocess.run([exe, "basetype", "--tmp-format", "mem", "-i", str(tmp_path / "none.list"), "-r", "none.fa", "-s", "chr1:1-2", "-o", out] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and line in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


# ---- bvc_store_tile's arithmetic ------------------------------------------------------------------------------------------------------
def fit(H, cum, n_batches, t0, max_positions, max_bytes):
    c = np.ascontiguousarray(cum, dtype=np.int64)
    nbytes = C.c_int64(-1)
    T = H.bvchost_store_tile_fit(C.c_void_p(c.ctypes.data), len(c) - 1, n_batches, t0, max_positions, max_bytes, C.byref(nbytes))
    return T, nbytes.value


def test_the_tile_arithmetic_against_the_plain_search(host):
    _, H = host
    rng = np.random.default_rng(20261020)
    n_batches, P = 7, 40
    # every record holds its length word: a position takes at least 4 bytes a batch
    sizes = 4 * n_batches + rng.integers(0, 5000, size=P)
    sizes[10:14] = 4 * n_batches                                  # a run of all-empty positions
    cum = np.concatenate([[123], 123 + np.cumsum(sizes)]).astype(np.int64)      # (rec_start[0] need not be 0: only differences count)
    pad = 16 * n_batches
    checked = 0
    for t0 in (0, 1, 9, 10, P - 2, P - 1):
        for T in range(1, P - t0 + 1):
            exact = int(cum[t0 + T] - cum[t0]) + pad
            for max_bytes, want in ((exact, T), (exact - 1, max(1, T - 1)), (exact + 1, None), (0, 1), (pad + 4 * n_batches, None)):
                for max_positions in (1, T, P):
                    model = sm.tile(cum, n_batches, t0, max_positions, max_bytes)
                    assert fit(H, cum, n_batches, t0, max_positions, max_bytes) == model, (t0, T, max_bytes, max_positions)
                    if want is not None and max_positions >= T:
                        # a budget that admits exactly T positions gives T; one byte less gives T - 1 (positions take at least 4 bytes a
                        # batch, so no two prefixes tie) or the one position a tile always has
                        assert model[0] == want, (t0, T, max_bytes, model)
                    checked += 1
    assert checked == 15 * sum(P - t0 for t0 in (0, 1, 9, 10, P - 2, P - 1))
    # the pad term: the same sizes admit fewer positions with more batches (16 bytes each), and the bytes reported carry it
    room = int(cum[8] - cum[0]) + 112                            # exactly eight positions of 7 batches
    T7, b7 = fit(H, cum, 7, 0, P, room)
    T70, b70 = fit(H, cum, 70, 0, P, room)
    assert T7 == 8 and T70 < T7 and b7 == int(cum[T7] - cum[0]) + 112 and b70 == int(cum[T70] - cum[0]) + 1120
    # t0 at both ends, one position asked for, nothing fits: one position
    assert fit(H, cum, 7, P - 1, P, 1 << 40) == (1, int(cum[P] - cum[P - 1]) + 112)
    assert fit(H, cum, 7, 0, P, 1 << 40) == (P, int(cum[P] - cum[0]) + 112)
    assert fit(H, cum, 7, 0, 1, 1 << 40)[0] == 1 and fit(H, cum, 7, 5, P, -1)[0] == 1


def test_the_models_tile_layout_keeps_every_slice_congruent_to_its_source():
    rng = np.random.default_rng(7)
    batches = [sm.random_batch(rng, 3, 6, filler=int(f)) for f in range(16)]
    places, rows, used = sm.gathered(batches, 1, 4)
    at = 0
    for (dst, data), (rec, rs), row in zip(places, batches, rows):
        assert dst % 16 == int(rs[1]) % 16 and 0 <= dst - at <= 15 and list(row) == [dst + int(r) - int(rs[1]) for r in rs[1:6]]
        at = dst + len(data)
    assert used == at <= sum(len(d) for _, d in places) + 16 * len(batches)
