"""Phase 1 straight into class counts (include/bvc_bam_counts.h) as far as a machine without a GPU can see it: the entry points are declared,
exported, in the binding's eighth table and refuse a null context or accumulator; the tally's layout is the binding's and the model's; the
new kernel is built from its own source without private memory, scratch, flat addressing or spills, in the product and the diagnostic
build; and the model (tests/bam_counts_model.py) folds a hand-made batch as the header says."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from tests import bam_counts_model as cm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_bam_counts", "bvc_site_acc_create", "bvc_site_acc_destroy", "bvc_site_acc_bytes", "bvc_bam_counts_bgzf_acc", "bvc_site_acc_get",
         "bvc_site_acc_lrt"]


def eighth_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_bam_counts.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc_bam_counts.h")).read()
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
    decls = eighth_header_declarations()
    assert list(decls) == bl.BAM_COUNTS_EXPORTS == NAMES
    # the closed lists stay as they were
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(tb.third_header_declarations()) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    others = (set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES) | set(bl.BAM_PROTOTYPES) | set(bl.POPMATRIX_PROTOTYPES) | set(bl.BAM_TEXT_PROTOTYPES) |
              set(bl.STORE_PROTOTYPES) | set(bl.BAM_DEFLATE_PROTOTYPES))
    assert not set(decls) & others
    returns = dict(ta.RETURNS, void=None)
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.BAM_COUNTS_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is returns[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # bvc_bam_counts takes bvc_bam_pileup's arguments up to rg_s, the _bgzf_acc call bvc_bam_pileup_bgzf's, name for name; neither takes the
    # reference's text
    third = tb.third_header_declarations()
    for mine, twin, tail in (("bvc_bam_counts", "bvc_bam_pileup", ["refseq_len", "group_of_sample", "n_groups", "counts", "tally", "sample_status", "flags"]),
                             ("bvc_bam_counts_bgzf_acc", "bvc_bam_pileup_bgzf", ["refseq_len", "group_of_sample", "acc", "sample_status"])):
        t, m = third[twin][1], decls[mine][1]
        k = next(i for i, p in enumerate(t) if p.endswith("rg_s")) + 1
        assert m[:k] == t[:k] and [p.split()[-1].lstrip("*") for p in m[k:]] == tail, mine
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc_bam.h"' in open(os.path.join(ROOT, "include", "bvc_bam_counts.h")).read() and "bvc_bam_counts.h" in header
    for m in ("create", "get", "lrt", "bytes", "close"):
        assert callable(getattr(bl.SiteAcc, m, None)), m
    assert callable(getattr(bl.Context, "bam_counts", None)) and callable(getattr(bl.Context, "bam_counts_bgzf_acc", None))
    import basevarc_amd
    assert basevarc_amd.SiteAcc is bl.SiteAcc
    # no context, no accumulator: refused before anything of the device is touched
    n64 = C.c_int64(7)
    assert L.bvc_bam_counts(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, 0, None, None, None, 0) == bm.ERR_ARG
    assert L.bvc_bam_counts_bgzf_acc(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, None, None) == bm.ERR_ARG
    assert L.bvc_site_acc_create(None, 0, 1, 0, 0) == bm.ERR_ARG
    assert L.bvc_site_acc_bytes(None, C.byref(n64), C.byref(n64)) == bm.ERR_ARG and n64.value == 7
    assert L.bvc_site_acc_get(None, None, 0, 0, None, None) == bm.ERR_ARG and L.bvc_site_acc_lrt(None, None, 0, 0, None, 0.001, None, None) == bm.ERR_ARG
    L.bvc_site_acc_destroy(None)
    # an accumulator's shape is refused before the device is looked for
    h = C.c_void_p(5)
    for n_positions, n_groups in ((-1, 0), (1, -1), (1, 33)):
        assert L.bvc_site_acc_create(C.byref(h), 0, n_positions, n_groups, 0) == bm.ERR_ARG and not h.value


def test_the_tally_is_forty_eight_bytes_in_the_header_the_binding_and_the_model():
    from basevarc_amd import lib as bl
    txt = open(os.path.join(ROOT, "include", "bvc_bam_counts.h")).read()
    body = re.search(r"typedef struct bvc_bam_site_tally \{(.*?)\} bvc_bam_site_tally;", txt, flags=re.S).group(1)
    fields = re.findall(r"uint32_t (\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", " ", body, flags=re.S))
    assert fields == [("strand_base", "8"), ("n_other", ""), ("n_indel", ""), ("pad", "2")]
    for dt in (bl.TALLY_DTYPE, cm.TALLY):
        assert dt.itemsize == 48 and dt.names == ("strand_base", "n_other", "n_indel", "pad")
        assert [dt.fields[n][1] for n in dt.names] == [0, 32, 36, 40]
    assert bl.NCLASS == cm.NCLASS == 512


COUNTS_SOURCE = "bam_counts_kernel.hip"
# the five instantiations of the one kernel (CountsKind 0 Slots, 1 Depth, 2 Narrow: no dry pass of Depth's own) and the two beside them
COUNTS_KERNELS = {f"bam_counts_kernel<{add}, (bvc::CountsKind){kind}>" for add, kind in (("false", 0), ("false", 2), ("true", 0), ("true", 1), ("true", 2))} | \
    {"first_status_kernel", "acc_expand_kernel"}


@functools.lru_cache(maxsize=None)
def check_the_counts_kernels():
    """The one check of the three headers' kernel source, in the product and the diagnostic build (made once a session): exactly the seven
    kernels, none with private memory, scratch, flat addressing, spills or MFMA; one resolve without text and no LDS in the source."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert COUNTS_SOURCE in b.SOURCES and COUNTS_SOURCE in isa_report.DEVICE_SOURCES and set(isa_report.DEVICE_SOURCES) <= set(b.SOURCES)
    text = open(os.path.join(ROOT, "basevarc_amd", "csrc", COUNTS_SOURCE)).read()
    assert text.count("resolve<false>(") == 1 and "__shared__" not in text
    for flags in ((), ("-DBVC_POISON", "-DBVC_CHECK_LDS")):
        rows = {re.match(r"(?:bvc::)?(\w+(?:<[^>]*>)?)", k["pretty"]).group(1): k for k in isa_report.kernels_of(isa_report.assembly(COUNTS_SOURCE, flags))}
        assert set(rows) == COUNTS_KERNELS, sorted(rows)
        for name, k in rows.items():
            assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["mfma"] == 0, (name, k)


def test_the_kernel_is_built_from_its_own_source_without_private_memory_or_flat_addressing():
    from basevarc_amd import build as b
    assert "bvc_bam_counts.hip" in b.SOURCES
    assert any(d.endswith("bvc_bam_counts.h") for d in b.DEPS)
    check_the_counts_kernels()


def test_the_model_folds_a_hand_made_batch_as_the_header_says():
    """Three samples over four positions: base entries of both strands, a quality byte above 127 (tallied, not counted), an N (class 4) and an
    insertion; with two groups and a label outside them."""
    R = bm.make_read
    reads = [R(1009, "4M", seq="ACGT", qual=[30, 127, 128, 255], flag=0),                     # strand 1
             R(1009, "2M2I2M", seq="CNGGTT", qual=[10, 11, 12, 13, 14, 15], flag=0x10),       # strand 0; an N at 1011; "+GG" at 1011
             R(1010, "3M", seq="GGG", qual=[5, 5, 5], flag=0)]
    samples = [(bm.pack_record(r), True, 0) for r in reads]
    positions = [1010, 1011, 1012, 1013]
    exp = cm.expected(samples, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), group_of_sample=[1, 0, 7], n_groups=2)
    assert exp["rc"] == 0 and exp["status"] == [0, 0, 0]
    c, t = exp["counts"], exp["tally"]
    A, Cc, G, T = 0, 1, 2, 3
    want = np.zeros((4, 3, 512), dtype=np.uint32)
    want[0, 1, A * 128 + 30] = 1; want[0, 0, Cc * 128 + 10] = 1                               # 1010: A q30 (+, group 1), C q10 (-, group 0)
    want[1, 1, Cc * 128 + 127] = 1; want[1, 2, G * 128 + 5] = 1                               # 1011: C q127; sample 1's indel; G q5 (in no group)
    want[2, 2, G * 128 + 5] = 1; want[2, 0, T * 128 + 14] = 1                                 # 1012: G q128 is tallied only; T q14 (-)
    want[3, 0, T * 128 + 15] = 1; want[3, 2, G * 128 + 5] = 1                                 # 1013: T q255 is tallied only
    assert (c == want).all(), np.argwhere(c != want)
    sb = t["strand_base"]
    assert sb[0].tolist() == [0, 1, 0, 0, 1, 0, 0, 0] and sb[1].tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert sb[2].tolist() == [0, 0, 0, 1, 0, 0, 2, 0] and sb[3].tolist() == [0, 0, 0, 1, 0, 0, 1, 1]
    assert t["n_indel"].tolist() == [0, 1, 0, 0] and t["n_other"].tolist() == [0, 0, 0, 0] and not t["pad"].any()
    # without groups everything lands in the one slot; an N where the position is not the insertion's anchor is class 4
    exp0 = cm.expected(samples[1:2], 0, 1 << 30, 20, [1010, 1011, 1013], bc.RG_S, len(bc.REFSEQ))
    assert exp0["counts"].shape == (3, 1, 512) and int(exp0["counts"].sum()) == 2 and exp0["tally"]["n_indel"].tolist() == [0, 1, 0]
    n_at = cm.expected([(bm.pack_record(R(1009, "3M", seq="CNG", qual=[9, 9, 9])), True, 0)], 0, 1 << 30, 20, [1011], bc.RG_S, len(bc.REFSEQ))
    assert n_at["tally"]["n_other"].tolist() == [1] and not n_at["counts"].any() and not n_at["tally"]["strand_base"].any()
    # a failing batch adds nothing
    bad = cm.expected([(bm.pack_record(reads[0])[:-3], True, 0)], 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ))
    assert bad["rc"] == bm.ERR_DATA and bad["status"] == [3] and bad["counts"] is None and bad["tally"] is None


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    from basevarc_amd import build as b
    return b.build_host()[0]


def test_the_host_program_has_its_option_and_its_rule(exe):
    import subprocess
    main = open(os.path.join(ROOT, "basevarc_amd", "host", "main.cpp")).read()
    assert "bvc_bam_counts_bgzf_acc" in main and "bvc_site_acc_lrt" in main and "counts_revisit(" in main
    assert "inline void counts_revisit(" in open(os.path.join(ROOT, "basevarc_amd", "host", "pileup.h")).read()
    r = subprocess.run([exe, "basetype", "--help"], capture_output=True, text=True)
    assert "counts:" in r.stderr and "mem:" in r.stderr, r.stderr
    # a sixth value is still refused with the usage
    r = subprocess.run([exe, "basetype", "--tmp-format", "disk", "-i", "x", "-o", "y"], capture_output=True, text=True)
    assert r.returncode == 1 and "--tmp-format" in r.stderr


@pytest.mark.parametrize("extra, line", [(["--load"], "--tmp-format counts with --load"), (["--keep_tmp"], "--tmp-format counts with --keep_tmp"),
                                         (["--gpus", "2"], "--tmp-format counts with --gpus above 1"),
                                         (["--group", "none.txt"], "--tmp-format counts with --group")])
def test_the_refusals_that_need_no_device(exe, tmp_path, extra, line):
    """Each is one line on stderr and exit code 1, before a file is opened or a directory made; the one for --group names --tmp-format mem.
    (A budget the class counts do not fit needs the region's positions: tests/test_gpu_host_counts.py.)"""
    import subprocess
    out = str(tmp_path / "o")
    r = subprocess.run([exe, "basetype", "--tmp-format", "counts", "-i", str(tmp_path / "none.list"), "-r", "none.fa", "-s", "chr1:1-2", "-o", out] + extra,
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and line in r.stderr, r.stderr
    if "--group" in extra:
        assert "--tmp-format mem" in r.stderr
    assert os.listdir(str(tmp_path)) == []
