"""bvc_bam_popmatrix as far as a machine without a GPU can see it: both entry points are declared (include/bvc_popmatrix.h, which bvc.h
names), exported, in the binding's fourth table type by type and refuse a null context; bvc.h's own list is untouched; the host
program reads its knob; the new kernel is built from its own source without private memory, scratch, flat addressing or spills and the
moved device code left bam_pileup_kernel.hip's kernels as they were; and fetch_allele_type with the position-file reader runs its
hand-built cases under the address sanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess
import sys

from tests import bam_pileup_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fourth_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_popmatrix.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc_popmatrix.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(bvc_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        assert name not in decls, name
        decls[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",")])
    return decls


def test_the_library_the_header_and_the_binding_know_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    decls = fourth_header_declarations()
    assert list(decls) == bl.POPMATRIX_EXPORTS == ["bvc_bam_popmatrix", "bvc_bam_popmatrix_bgzf"]
    others = set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES) | set(bl.BAM_PROTOTYPES)
    assert not set(decls) & set(ta.header_declarations()) and not set(bl.POPMATRIX_PROTOTYPES) & others
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.POPMATRIX_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is ta.RETURNS[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    params = decls["bvc_bam_popmatrix"][1]
    assert params[:4] == ["bvc_ctx *ctx", "int32_t n_samples", "const uint8_t *bam", "int64_t bam_bytes"] and params[-1] == "uint32_t flags"
    assert params[-4:-1] == ["uint8_t *matrix", "int64_t row_stride", "uint32_t *sample_status"]
    assert "const char *refseq" not in " ".join(params)                       # the reference's text never reaches the call
    # bvc.h's list is closed and untouched: the same names as the first table, the new header only named in a comment
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert list(ta.header_declarations()) == bl.EXPORTS and "bvc_popmatrix.h" in header
    assert '#include "bvc.h"' in open(os.path.join(ROOT, "include", "bvc_popmatrix.h")).read()
    assert callable(getattr(bl.Context, "bam_popmatrix", None))
    # the host program reads its knob in knobs.h: default 0
    knobs = open(os.path.join(ROOT, "basevarc_amd", "host", "knobs.h")).read()
    assert re.search(r'device_popmatrix = num\("BVC_HOST_DEVICE_POPMATRIX", 0\) != 0;', knobs)
    main = open(os.path.join(ROOT, "basevarc_amd", "host", "main.cpp")).read()
    assert "knobs.device_popmatrix" in main and "is not part of the MI355X build" not in main
    # no context: refused before anything of the device is touched
    assert L.bvc_bam_popmatrix(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, None, None, 0, 0, None, 0, None, 0) == bm.ERR_ARG
    assert L.bvc_bam_popmatrix_bgzf(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, None, None, 0, 0, None, 0, None) == bm.ERR_ARG


def test_the_kernel_is_built_from_its_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "bam_popmatrix_kernel.hip" in b.SOURCES and "bam_resolve_device.h" in b.DEPS and "popmatrix.cpp" in b.HOST_SOURCES
    assert "bam_popmatrix_kernel.hip" in isa_report.DEVICE_SOURCES
    name = lambda k: re.match(r"(?:bvc::)?([\w<>]+)", k["pretty"]).group(1)
    rows = {name(k): k for k in isa_report.kernels_of(isa_report.assembly("bam_popmatrix_kernel.hip"))}
    assert set(rows) == {"bam_popmatrix_kernel"}, sorted(rows)
    k = rows["bam_popmatrix_kernel"]
    assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, k
    # resolve() lives in the header both sources include, and nowhere else
    csrc = os.path.join(ROOT, "basevarc_amd", "csrc")
    for src in ("bam_pileup_kernel.hip", "bam_popmatrix_kernel.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "bam_resolve_device.h"' in text and "Hit resolve(" not in text, src
    assert "Hit resolve(" in open(os.path.join(csrc, "bam_resolve_device.h")).read()


def test_fetch_allele_type_and_the_position_file_under_the_address_sanitizer(tmp_path):
    """tests/cpp/popmatrix_main.cpp with host/bam.cpp and host/popmatrix.cpp, built with -fsanitize=address,undefined and run directly."""
    host = os.path.join(ROOT, "basevarc_amd", "host")
    exe = str(tmp_path / "popmatrix_cases")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-pthread", "-I", host, os.path.join(ROOT, "tests", "cpp", "popmatrix_main.cpp")] +
                          [os.path.join(host, f) for f in ("popmatrix.cpp", "bam.cpp", "bgzf.cpp", "inflate.cpp")] + ["-lz", "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert "21 cases, 0 wrong" in text, text[-2000:]
