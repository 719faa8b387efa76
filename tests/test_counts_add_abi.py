"""Counts accumulated over sample chunks, as far as a machine without a GPU can see them: libbvc.so exports the eight entry points,
include/bvc.h declares them, the Python binding binds each with the header's argument count, the new kernels are built (tests/test_isa.py
then holds them to the rules of every kernel), and the by-sample helpers of basevarc_amd.sharding split and sum exactly."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bvc_counts_add_dense", "bvc_counts_add_dense_packed", "bvc_counts_add_csr", "bvc_counts_add_csr_packed",
           "bvc_counts_add_dense_groups", "bvc_counts_add_csr_group_labels", "bvc_lrt_hist_groups", "bvc_counts_merge")


def test_the_library_exports_the_eight_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    # (the symbol table only: loading through basevarc_amd.lib would bring the HIP runtime in, which this test does not need)
    L = C.CDLL(bl.library_path(), mode=os.RTLD_LAZY)
    for s in SYMBOLS:
        assert hasattr(L, s), s


def header_parameters(name):
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
    assert m, f"{name} is not declared in include/bvc.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_the_header_declares_them_and_the_binding_matches():
    from basevarc_amd import lib as bl
    for s in SYMBOLS:
        params = header_parameters(s)
        assert params[0] == "bvc_ctx *ctx" and params[-1] == "uint32_t flags", s
        assert s in bl.EXPORTS, s
        assert s in bl.PROTOTYPES, f"basevarc_amd.lib does not bind {s}"
        restype, argtypes = bl.PROTOTYPES[s]
        assert restype is C.c_int, (s, restype)
        assert len(argtypes) == len(params), (s, argtypes, params)
        # pointers are bound as pointers, sizes as 64-bit integers
        for a, prm in zip(argtypes, params):
            assert (a is C.c_void_p) == ("*" in prm), (s, a, prm)
            if prm.startswith("int64_t"):
                assert a is C.c_int64, (s, a, prm)
    for m in ("counts_add_dense", "counts_add_dense_device", "counts_add_dense_packed", "counts_add_dense_packed_device", "counts_add_csr",
              "counts_add_csr_device", "counts_add_csr_packed", "counts_add_csr_packed_device", "counts_add_dense_groups",
              "counts_add_dense_groups_device", "counts_add_csr_group_labels", "counts_add_csr_group_labels_device", "lrt_hist_groups",
              "lrt_hist_groups_device", "counts_merge", "counts_merge_device"):
        assert callable(getattr(bl.Context, m, None)), m


def test_the_header_says_which_slot_holds_the_samples_in_no_group():
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert re.search(r"LAST slot, n_groups, holds those in no group", header)
    assert '"csr_scatter_max"' in header


def test_the_new_kernels_are_built():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    rows = {}
    for src in ("counts_kernel.hip", "pileup_kernel.hip"):
        for k in isa_report.kernels_of(isa_report.assembly(src)):
            rows[k["pretty"]] = k
    want = ["counts_add_kernel"] + [f"{n}<{a}, {b}>" for n in ("hist_csr_scatter_kernel", "hist_csr_add_kernel")
                                    for a in ("false", "true") for b in ("false", "true")]
    for name in want:
        assert name in rows, (name, sorted(rows))
        k = rows[name]
        assert k["flat"] == 0 and k["scratch"] == 0 and k["private"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 0, k
    # the fold has one owner per word and the scatter kernel no histogram: atomics only where they are meant to be
    assert not any(m.startswith("global_atomic") or m.startswith("ds_") for m in rows["counts_add_kernel"]["mnemonics"])
    for a in ("false", "true"):
        for b in ("false", "true"):
            mn = rows[f"hist_csr_scatter_kernel<{a}, {b}>"]["mnemonics"]
            assert mn.get("global_atomic_add", 0) >= 1 and not any(m.startswith("ds_") for m in mn), mn
    assert rows["counts_add_kernel"]["mnemonics"].get("global_load_dwordx4", 0) >= 2
    assert rows["counts_add_kernel"]["mnemonics"].get("global_store_dwordx4", 0) >= 1


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_sample_ranges_cover_the_cohort_exactly_once(world):
    from basevarc_amd.sharding import sample_ranges
    for n in (0, 1, 2, 5, 7, 500, 1000003):
        r = sample_ranges(n, world)
        assert len(r) == world and r[0][0] == 0 and r[-1][1] == n
        assert all(lo <= hi for lo, hi in r) and all(r[i][1] == r[i + 1][0] for i in range(world - 1))
        sizes = [hi - lo for lo, hi in r]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        sample_ranges(5, 0)


def _allreduce_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from basevarc_amd.sharding import allreduce_counts
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(100 + rank)
        part = rng.integers(0, 1 << 32, (3, 512), dtype=np.uint64).astype(np.uint32)
        part[0, 0] = 0xFFFFFFFF if rank == 0 else 1                  # wraps to 0
        part[0, 1] = 0x80000000                                      # twice: wraps to 0
        total = allreduce_counts(part)
        as_tensor = allreduce_counts(torch.from_numpy(part.view(np.int32).copy()))
        q.put((rank, part, total, as_tensor.numpy().view(np.uint32)))
    finally:
        dist.destroy_process_group()


def test_allreduce_counts_sums_exactly_over_two_gloo_ranks():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctxmp = mp.get_context("spawn")
    q = ctxmp.Queue()
    procs = [ctxmp.Process(target=_allreduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = got[0][1] + got[1][1]                                     # uint32: wraps like the library
    assert want[0, 0] == 0 and want[0, 1] == 0
    for _, part, total, as_tensor in got:
        assert total.dtype == np.uint32 and total.shape == part.shape
        assert np.array_equal(total, want) and np.array_equal(as_tensor, want)
