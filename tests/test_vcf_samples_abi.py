"""The VCF sample columns formatted on the device, as far as a machine without a GPU can see them: both libraries export the new entry
points, include/bvc.h declares them and the binding's table names them, the slot formula and the kernel's tile are the ones the binding and
the GPU tests use, the kernel is built from its own source under the rules of every kernel, the 256 BP strings the kernel copies are the
host program's, the plain Python model of the text (tests/vcf_samples_cases.py) equals the host program's columns on the whole catalogue,
and the VCF line built around existing columns equals the one built from the entries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tests import vcf_samples_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bvc_vcf_bp_lut", "bvc_vcf_samples_csr", "bvc_pileup_finish_called_text", "bvc_pileup_sample_text")
HOST_SYMBOLS = ("bvchost_vcf_samples", "bvchost_vcf_line_from_text", "bvchost_site_from_arrays")


@pytest.fixture(scope="module")
def host():
    return vc.host_library()


def test_the_libraries_export_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    # (the symbol table only: loading through basevarc_amd.lib would bring the HIP runtime in, which this test does not need)
    L = C.CDLL(bl.library_path(), mode=os.RTLD_LAZY)
    for s in SYMBOLS:
        assert hasattr(L, s), s
    _, hostlib = b.build_host()
    H = C.CDLL(hostlib)
    for s in HOST_SYMBOLS:
        assert hasattr(H, s), s


def test_the_header_declares_them_and_the_binding_requires_them():
    from basevarc_amd import lib as bl
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert re.search(r"static inline int64_t bvc_vcf_samples_slot\(int64_t n_samples, int64_t n_entries\)", header)
    assert re.search(r"\bvoid bvc_vcf_bp_lut\(char out\[2048\]\);", header)
    assert re.search(r"\bint bvc_vcf_samples_csr\(bvc_ctx \*ctx, int64_t n_sites, const int64_t \*offsets, const bvc_pileup_entry \*entries,",
                     header)
    assert re.search(r"\bint bvc_pileup_finish_called_text\(bvc_ctx \*ctx, const int8_t \*ref_base, double min_af,", header)
    assert re.search(r"\bint bvc_pileup_sample_text\(bvc_ctx \*ctx, int64_t n_samples, char \*text, int64_t text_cap, int64_t \*text_off, "
                     r"int64_t \*text_len\);", header)
    # declared in this order, and rows of the binding's one table (tests/test_binding_abi.py compares every row with its declaration)
    from tests import test_binding_abi as ta
    assert [name for name in ta.header_declarations() if name in SYMBOLS] == list(SYMBOLS)
    assert [name for name in bl.EXPORTS if name in SYMBOLS] == list(SYMBOLS)
    for m in ("vcf_samples_csr", "vcf_samples_csr_device", "pileup_sample_text"):
        assert callable(getattr(bl.Context, m, None)), m


def test_the_slot_formula_and_the_tile_are_the_ones_the_tests_use(tmp_path):
    from basevarc_amd import lib as bl
    # the header's inline function, compiled: against the binding's formula on every residue of both arguments and on large sizes
    src = tmp_path / "slot.c"
    src.write_text('#include "bvc.h"\nlong long slot(long long n, long long e) { return bvc_vcf_samples_slot(n, e); }\n')
    so = tmp_path / "slot.so"
    import subprocess
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", str(so), str(src)])
    S = C.CDLL(str(so))
    S.slot.restype = C.c_longlong
    S.slot.argtypes = [C.c_longlong, C.c_longlong]
    for n in list(range(0, 40)) + [10 ** 5, 10 ** 6 + 3, 2 ** 31 - 1]:
        for e in list(range(0, 40)) + [10 ** 4, n]:
            want = bl.vcf_samples_slot(n, e)
            assert S.slot(n, e) == want and want % 16 == 0 and 0 <= want - (4 * n + 13 * e) < 16, (n, e)
    internal = open(os.path.join(ROOT, "basevarc_amd", "csrc", "bvc_internal.h")).read()
    kernel = open(os.path.join(ROOT, "basevarc_amd", "csrc", "vcf_samples_kernel.hip")).read()
    tile = int(re.search(r"constexpr int kVcfSamplesTile = (\d+);", internal).group(1))
    threads = int(re.search(r"constexpr int kVsThreads = (\d+);", kernel).group(1))
    halo = int(re.search(r"constexpr int kVsHalo = (\d+);", kernel).group(1))
    assert bl.VCF_SAMPLES_TILE == vc.T == tile == threads - halo
    assert {tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1} <= set(vc.SIZES)


def test_the_kernel_is_built_from_its_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "vcf_samples_kernel.hip" in b.SOURCES and "bvc_vcf.hip" in b.SOURCES
    assert "vcf_samples_kernel.hip" in isa_report.DEVICE_SOURCES
    rows = {k["pretty"].split("::")[-1]: k for k in isa_report.kernels_of(isa_report.assembly("vcf_samples_kernel.hip"))}
    assert set(rows) == {"vcf_valid_kernel", "vcf_plan_kernel", "vcf_samples_kernel"}, sorted(rows)
    for name, k in rows.items():
        assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)
    k = rows["vcf_samples_kernel"]
    assert k["lds"] == 0                                           # one workgroup's LDS is the launch's (dynamic)
    # the text leaves in 16-byte stores and in nothing narrower; no floating point in the kernel that formats
    stores = {m: n for m, n in k["mnemonics"].items() if m.startswith("global_store") or m.startswith("buffer_store")}
    assert set(stores) == {"global_store_dwordx4"}, stores
    assert not [m for m in k["mnemonics"] if re.match(r"v_(add|mul|fma|exp|log|cvt|rcp|div)\w*_f(16|32|64)", m)], k["mnemonics"]


def test_the_bp_table_is_the_host_programs(host):
    from basevarc_amd import lib as bl
    lut = bl.vcf_bp_lut()
    assert len(lut) == 2048
    res = vc.make_result(1, 0, (-1, -1, -1))
    for q in range(256):
        got = vc.host_columns(host, 1, np.zeros(1, np.int32), vc.make_entries(1, qual=q), 0, res)
        assert got == b"0/.:A:-:" + lut[8 * q:8 * q + 8], q
        assert lut[8 * q:8 * q + 8] == vc.BP[q], q
    assert lut[:8] == b"0.000000" and lut[-8:] == b"1.000000"


@pytest.mark.parametrize("n", vc.SIZES)
def test_the_model_equals_the_host_programs_columns(host, n):
    sites = vc.sites_of(n)
    called = 0
    for (name, samples, entries, ref, res), want in zip(sites, vc.model_of(n, sites)):
        if not int(res["called"]) or not vc.host_defined(res):
            continue
        assert vc.host_columns(host, n, samples, entries, ref, res) == want, (n, name)
        called += 1
    assert called > 100


def test_the_catalogue_holds_what_it_is_meant_to():
    for n in vc.SIZES:
        sites = vc.sites_of(n)
        names = [s[0] for s in sites]
        for must in ("coverage none", "coverage all", "coverage first", "coverage last", "coverage tile_ends", "coverage runs_across_edges",
                     "coverage alternating", "n = 0 on a called site", "first entry negative", "first entry = n", "first entry 2^31 - 1",
                     "everything repeated", "n_alt 5 is read as 3"):
            assert must in names, (n, must)
        assert any(not int(s[4]["called"]) for s in sites)
        quals = set()
        for s in sites:
            if s[0].startswith("qualities"):
                quals |= set(int(q) for q in s[2]["qual"])
        assert quals == set(range(256)), n
        seen = {(int(b) & 7, s[3]) for s in sites if s[0].startswith("ref ") for b in s[2]["base"]}
        assert seen == {(b, r) for b in range(8) for r in range(-1, 6)}, n
        assert {int(x) for s in sites for x in s[2]["strand"]} >= {0, 1, 2, 3} or n < 4
        nv = [vc.valid_prefix(n, s[1]) for s in sites if int(s[4]["called"])]
        lens = [len(s[1]) for s in sites if int(s[4]["called"])]
        assert any(v < m for v, m in zip(nv, lens)) and any(v == 0 and m > 0 for v, m in zip(nv, lens)), n
    big = vc.sites_of(vc.T + 1)
    assert len({tuple(int(x) for x in s[4]["alt_base"][:int(s[4]["n_alt"])]) for s in big if s[0].startswith("ref ")}) >= 1 + 4 + 16 + 64


# ---- the line around existing columns ----------------------------------------------------------------------------------------
def rank2_model(ref, alt):
    r = np.bincount(np.asarray(ref, dtype=np.int64), minlength=256)[::-1]
    a = np.bincount(np.asarray(alt, dtype=np.int64), minlength=256)[::-1]
    m = r + a
    lo = np.cumsum(m) - m
    return sum(int(r[i]) * (2 * int(lo[i]) + int(r[i]) + int(a[i]) + 1) for i in range(256))


def stats_model(e, ref, res):
    """bvc_site_stats of one called site from its entries (include/bvc.h), as the device computes it."""
    from basevarc_amd.lib import STATS_DTYPE
    st = np.zeros((), dtype=STATS_DTYPE)
    base = e["base"].astype(np.int64)
    counted = (e["is_indel"] != 1) & (base <= 3)
    is_ref = counted & (base == int(ref))
    alts = [int(res["alt_base"][i]) for i in range(int(res["n_alt"]))]
    is_alt = counted & ~is_ref & np.isin(base, alts)
    fwd = e["strand"] == 1
    st["rank2"] = [rank2_model(e[f][is_ref], e[f][is_alt]) for f in ("mapq", "qual", "rpr")]
    st["n_ref"] = is_ref.sum(); st["n_alt"] = is_alt.sum()
    st["ref_fwd"] = (is_ref & fwd).sum(); st["ref_rev"] = (is_ref & ~fwd).sum()
    st["alt_fwd"] = (is_alt & fwd).sum(); st["alt_rev"] = (is_alt & ~fwd).sum()
    st["valid"] = 1
    return st


@pytest.mark.parametrize("extra", [(None, None), (b"EAS_AF;AFR_AF;zz_AF", b"0.250000,0;0;0.5")], ids=["plain", "groups"])
def test_the_line_from_existing_columns_equals_the_line_from_the_entries(host, extra):
    rng = np.random.default_rng(5)
    checked = 0
    for n in (1, 5, vc.T + 1, 2 * vc.T + 1):
        for k in (0, 1, min(n, 40), n):
            for trial in range(3):
                samples = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
                e = vc.make_entries(k, rng)
                e["base"] = rng.choice([0, 1, 2, 3, 4, 5], k, p=[0.5, 0.2, 0.1, 0.1, 0.05, 0.05])
                e["strand"] = rng.integers(0, 2, k)
                ref = int(rng.integers(0, 4))
                n_alt = int(rng.integers(1, 4))
                alt = [(ref + 1 + i) % 4 for i in range(n_alt)]
                res = vc.make_result(1, n_alt, tuple(alt) + (-1,) * (3 - n_alt))
                res["var_qual"] = float(rng.choice([3.5, 1234.5678])); res["depth_total"] = float(max(1, k))
                res["depth"] = [int(((e["base"] == b) & (e["is_indel"] != 1)).sum()) for b in range(4)]
                res["af"] = rng.random(3)
                st = stats_model(e, ref, res)
                site = vc.HostSite(host, e, samples, pos=12345 + trial)
                cap = 4 * n + 17 * k + 4096
                a, b = C.create_string_buffer(cap), C.create_string_buffer(cap)
                na = host.bvchost_vcf_line(site.h, res.ctypes.data, b"chr7", ref, n, extra[0], extra[1], a, cap)
                cols = vc.host_columns(host, n, samples, e, ref, res)
                assert cols == vc.model_columns(n, samples, e, ref, n_alt, alt + [-1] * 3)
                nb = host.bvchost_vcf_line_from_text(res.ctypes.data, b"chr7", 12345 + trial, ref, st.ctypes.data, extra[0], extra[1],
                                                     cols, len(cols), b, cap)
                assert na == nb and a.raw[:na] == b.raw[:nb], (n, k, trial)
                assert a.raw[:na - 1].endswith(b"\tGT:AB:SO:BP\t" + cols + b"\n")
                if extra[0]:
                    assert b"AFR_AF=0;" in a.raw[:na] and b"EAS_AF=0.250000,0;" in a.raw[:na]
                checked += 1
    assert checked == 48
