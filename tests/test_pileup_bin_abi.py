"""bvc_pileup_begin_bin without a device: the entry point is declared in include/bvc.h and exported by libbvc.so, and the compiler
emitted its kernel -- both template forms, the count pass and the write pass -- without FLAT or scratch addressing, a private segment
or a VGPR spill (the product build and the diagnostic one)."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_the_entry_point_is_declared_and_exported():
    from basevarc_amd import build as b
    from basevarc_amd import lib
    header = open(os.path.join(ROOT, "include", "bvc.h"), encoding="utf-8").read()
    m = re.search(r"\bint\s+bvc_pileup_begin_bin\s*\(([^;]*)\)\s*;", header)
    assert m, "include/bvc.h does not declare bvc_pileup_begin_bin"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 10 and args[0].startswith("bvc_ctx") and "rec_start" in args[3] and args[1].startswith("const uint8_t")
    assert "bvc_pileup_begin_bin" in lib.EXPORTS
    L = C.CDLL(b.build())                                        # dlopen only: no device is touched
    for name in lib.EXPORTS:
        assert hasattr(L, name), name
    # a null context is refused before anything else is looked at (BVC_ERR_ARG)
    lib.bind(L)
    assert L.bvc_pileup_begin_bin(None, None, 0, None, None, None, 0, 0, None, None) == -1


def test_the_record_kernel_is_compiled_in_both_forms_without_flat_scratch_or_spills():
    from tools import isa_report
    for flags in ((), ("-DBVC_POISON", "-DBVC_CHECK_LDS")):
        rows = [k for k in isa_report.kernels_of(isa_report.assembly("pileup_kernel.hip", flags)) if "pileup_bin_kernel" in k["pretty"]]
        forms = sorted(re.search(r"<(\w+)>", k["pretty"]).group(1) for k in rows)
        assert forms == ["false", "true"], (flags, [k["pretty"] for k in rows])
        for k in rows:
            assert k["instructions"] > 100, k
            assert k["flat"] == k["scratch"] == k["private"] == k["vgpr_spill"] == 0, (flags, k)
    assert any("pileup_bin_kernel" in k["pretty"] for k in isa_report.report() if k["source"] == "pileup_kernel.hip")
