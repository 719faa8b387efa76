"""The called sites' rank-sum and strand statistics on the device, as far as a machine without a GPU can see them: libbvc.so exports
bvc_site_stats_csr and bvc_pileup_finish_called_stats, libbvchost.so exports bvchost_ranksum_from_rank2, include/bvc.h declares the two,
the Python binding requires them, site_stats_kernel is built from site_stats_kernel.hip (tests/test_isa.py then holds it to the rules of
every kernel), and the host's phred value computed from the integer the device delivers (rank2 = 2 x rankR1) is the double RankSumTest
computes from the vectors."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bvc_site_stats_csr", "bvc_pileup_finish_called_stats")


def test_the_libraries_export_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    # (the symbol table only: loading through basevarc_amd.lib would bring the HIP runtime in, which this test does not need)
    L = C.CDLL(bl.library_path(), mode=os.RTLD_LAZY)
    for s in SYMBOLS:
        assert hasattr(L, s), s
    _, hostlib = b.build_host()
    assert hasattr(C.CDLL(hostlib), "bvchost_ranksum_from_rank2")


def test_the_header_declares_them_and_the_binding_requires_them():
    from basevarc_amd import lib as bl
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert re.search(r"\bint bvc_site_stats_csr\(bvc_ctx \*ctx, int64_t n_sites, const int64_t \*offsets, const bvc_pileup_entry \*entries,",
                     header)
    assert re.search(r"\bint bvc_pileup_finish_called_stats\(bvc_ctx \*ctx, const int8_t \*ref_base, double min_af,", header)
    assert re.search(r"typedef struct bvc_site_stats \{\s*/\* 64 bytes \*/", header)
    for s in SYMBOLS:
        assert s in bl.EXPORTS, s
    for m in ("site_stats_csr", "site_stats_csr_device"):
        assert callable(getattr(bl.Context, m, None)), m
    assert bl.STATS_DTYPE.itemsize == 64
    assert [(n, bl.STATS_DTYPE.fields[n][1]) for n in ("rank2", "n_ref", "n_alt", "ref_fwd", "ref_rev", "alt_fwd", "alt_rev", "valid")] == \
        [("rank2", 0), ("n_ref", 24), ("n_alt", 28), ("ref_fwd", 32), ("ref_rev", 36), ("alt_fwd", 40), ("alt_rev", 44), ("valid", 48)]
    # the per-trip width the GPU tests straddle is the kernel's: threads x 16-byte loads per lane x two entries per load
    internal = open(os.path.join(ROOT, "basevarc_amd", "csrc", "bvc_internal.h")).read()
    kernel = open(os.path.join(ROOT, "basevarc_amd", "csrc", "site_stats_kernel.hip")).read()
    trip = int(re.search(r"constexpr int kSiteStatsTrip = (\d+);", internal).group(1))
    threads = int(re.search(r"constexpr int kStatsThreads = (\d+);", kernel).group(1))
    loads = int(re.search(r"constexpr int kStatsLoads = (\d+);", kernel).group(1))
    assert bl.SITE_STATS_TRIP == trip == threads * loads * 2


def test_the_kernel_is_built_from_its_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "site_stats_kernel.hip" in b.SOURCES and "bvc_stats.hip" in b.SOURCES
    assert "site_stats_kernel.hip" in isa_report.DEVICE_SOURCES
    rows = [k for k in isa_report.kernels_of(isa_report.assembly("site_stats_kernel.hip")) if k["pretty"].endswith("site_stats_kernel")]
    assert len(rows) == 1, rows
    k = rows[0]
    # one workgroup's LDS is the launch's (dynamic): no static LDS, no private memory, no spill of either kind
    assert k["lds"] == 0 and k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0, k
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k


# ---- bvchost_ranksum_from_rank2 against bvchost_ranksum on the expanded vectors ----------------------------------------------------
def rank2_model(ref, alt):
    """2 x rankR1 of `ref` among ref + alt (bytes), as the integer function of the two histograms (include/bvc.h)."""
    r = np.bincount(np.asarray(ref, dtype=np.int64), minlength=256)[::-1]
    a = np.bincount(np.asarray(alt, dtype=np.int64), minlength=256)[::-1]
    m = r + a
    lo = np.cumsum(m) - m                                          # pooled observations of a larger value
    return sum(int(r[i]) * (2 * int(lo[i]) + int(r[i]) + int(a[i]) + 1) for i in range(256))


@pytest.fixture(scope="module")
def host():
    from basevarc_amd import build as b
    _, hostlib = b.build_host()
    H = C.CDLL(hostlib)
    H.bvchost_ranksum.restype = C.c_double
    H.bvchost_ranksum.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    H.bvchost_ranksum_from_rank2.restype = C.c_double
    H.bvchost_ranksum_from_rank2.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    return H


def _cases():
    rng = np.random.default_rng(20261018)
    cases = []
    for distinct in (1, 2, 256):
        values = {1: [60], 2: [0, 255], 256: list(range(256))}[distinct]
        for n1 in (0, 1, 2, 300):
            for n2 in (0, 1, 2, 300):
                cases.append((f"{distinct} values, n1={n1}, n2={n2}", rng.choice(values, n1), rng.choice(values, n2)))
    cases.append(("n1 = 0", np.zeros(0, np.int64), rng.integers(0, 256, 57)))
    cases.append(("n2 = 0", rng.integers(0, 256, 57), np.zeros(0, np.int64)))
    return cases


def _both(host, ref, alt):
    x = np.ascontiguousarray(ref, dtype=np.float64)
    y = np.ascontiguousarray(alt, dtype=np.float64)
    xp = x.ctypes.data if len(x) else None
    yp = y.ctypes.data if len(y) else None
    want = host.bvchost_ranksum(xp, len(x), yp, len(y))
    got = host.bvchost_ranksum_from_rank2(rank2_model(ref, alt), len(x), len(y))
    return got, want


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_phred_from_rank2_is_the_double_of_ranksum_on_the_vectors(host, case):
    from oracle.emit_oracle import rank_sum_test
    _, ref, alt = case
    got, want = _both(host, ref, alt)
    assert _same_double(got, want), (case[0], got, want)
    orc = rank_sum_test([float(v) for v in ref], [float(v) for v in alt])
    assert _same_double(got, orc) or abs(got - orc) <= 1e-12, (case[0], got, orc)


def test_one_run_of_70000_equal_values(host):
    """Longer than the run at which the reference's own int32 rank sum wraps (about 65,536): the host program's statistic does not
    (host/stats.cpp), and the integer from the histograms is that statistic."""
    from oracle.emit_oracle import rank_sum_test
    ref, alt = np.full(40000, 60), np.full(30000, 60)
    got, want = _both(host, ref, alt)
    assert _same_double(got, want), (got, want)
    orc = rank_sum_test([60.0] * 40000, [60.0] * 30000)
    assert _same_double(got, orc) or abs(got - orc) <= 1e-12, (got, orc)
