"""The ragged group call with one label byte per observation, as far as a machine without a GPU can see it: libbvc.so exports
bvc_lrt_csr_group_labels and bvc_lrt_csr_group_labels_packed, include/bvc.h declares them, the Python binding requires them, and
hist_csr_labels_kernel is built in both instantiations (tests/test_isa.py then holds it to the rules of every kernel)."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bvc_lrt_csr_group_labels", "bvc_lrt_csr_group_labels_packed")


def test_the_library_exports_both_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    # (the symbol table only: loading through basevarc_amd.lib would bring the HIP runtime in, which this test does not need)
    L = C.CDLL(bl.library_path(), mode=os.RTLD_LAZY)
    for s in SYMBOLS:
        assert hasattr(L, s), s


def test_the_header_declares_them_and_the_binding_requires_them():
    from basevarc_amd import lib as bl
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(bvc_ctx \*ctx, int64_t n_sites, const int64_t \*offsets,", header), s
        assert s in bl.EXPORTS, s
    for m in ("lrt_csr_group_labels", "lrt_csr_group_labels_device", "lrt_csr_group_labels_packed", "lrt_csr_group_labels_packed_device"):
        assert callable(getattr(bl.Context, m, None)), m


def test_the_label_kernel_is_built_unpacked_and_packed():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    rows = [k for k in isa_report.report() if k["pretty"].startswith("hist_csr_labels_kernel")]
    assert all(k["source"] == "pileup_kernel.hip" for k in rows)
    assert sorted(k["pretty"] for k in rows) == ["hist_csr_labels_kernel<false>", "hist_csr_labels_kernel<true>"]
    # one workgroup's LDS is the launch's (dynamic): the kernels own no static LDS and no private memory
    assert all(k["lds"] == 0 and k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 for k in rows), rows
