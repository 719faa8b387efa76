"""Class counts in narrow quality rows (include/bvc_site_acc_quals.h) as far as a machine without a GPU can see them: the entry points are
declared, exported, in the binding's tenth table and refuse a null context and a bad shape; the nine older lists are what they were; the
new source is in the build's and the ISA report's lists; the byte formula and the chromosome arithmetic it is for; the model
(tests/bam_counts_quals_model.py) by hand on two tiny cases and on the 100 test BAMs, whose highest counted quality is 39; and the host
program's knob BVC_HOST_COUNTS_QUALS: its parse rule and its refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_counts_model as cm
from tests import bam_counts_quals_model as qm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_bam_counts_quals", "bvc_site_acc_create_quals", "bvc_site_acc_quals"]


def test_the_library_the_header_and_the_binding_know_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_bam_counts_abi as t8
    from tests import test_bam_group_depth_abi as t9
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    decls = t9.declarations_of("bvc_site_acc_quals.h")
    assert list(decls) == bl.SITE_ACC_QUALS_EXPORTS == list(bl.SITE_ACC_QUALS_PROTOTYPES) == NAMES
    # the nine older lists are what they were, and none of them holds a new name
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(t8.eighth_header_declarations()) == bl.BAM_COUNTS_EXPORTS == t8.NAMES
    assert list(t9.declarations_of("bvc_bam_group_depth.h")) == bl.BAM_GROUP_DEPTH_EXPORTS == t9.NAMES
    older = (bl.PROTOTYPES, bl.BGZF_CODES_PROTOTYPES, bl.BAM_PROTOTYPES, bl.POPMATRIX_PROTOTYPES, bl.BAM_TEXT_PROTOTYPES, bl.STORE_PROTOTYPES,
             bl.BAM_DEFLATE_PROTOTYPES, bl.BAM_COUNTS_PROTOTYPES, bl.BAM_GROUP_DEPTH_PROTOTYPES)
    assert [len(t) for t in older[1:]] == [1, 2, 2, 2, 9, 3, 7, 3], [len(t) for t in older]
    for table in older:
        assert not set(table) & set(decls)
    returns = dict(ta.RETURNS, void=None)
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.SITE_ACC_QUALS_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is returns[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # bvc_bam_counts_quals takes bvc_bam_counts_depth's arguments, name for name, with n_quals behind n_groups
    mine, twin = decls["bvc_bam_counts_quals"][1], t9.declarations_of("bvc_bam_group_depth.h")["bvc_bam_counts_depth"][1]
    k = next(i for i, p in enumerate(twin) if p.endswith("n_groups")) + 1
    assert mine[:k] == twin[:k] and k == 17 and mine[k] == "int32_t n_quals" and mine[k + 1:] == twin[k:]
    assert decls["bvc_site_acc_create_quals"][1] == ["bvc_site_acc **out", "int device", "int32_t n_positions", "int32_t n_groups", "int32_t n_quals",
                                                     "int64_t byte_budget"]
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc_bam_group_depth.h"' in open(os.path.join(ROOT, "include", "bvc_site_acc_quals.h")).read() and "bvc_site_acc_quals.h" in header
    assert callable(getattr(bl.SiteAcc, "create_quals", None)) and callable(getattr(bl.Context, "bam_counts_quals", None))
    # no context, no accumulator: refused before anything of the device is touched
    assert L.bvc_bam_counts_quals(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, 0, 40, None, None, None, None, 0) == bm.ERR_ARG
    assert L.bvc_site_acc_create_quals(None, 0, 1, 0, 40, 0) == bm.ERR_ARG
    q = C.c_int32(-7)
    assert L.bvc_site_acc_quals(None, C.byref(q)) == bm.ERR_ARG and q.value == -7
    # an accumulator's shape is refused before the device is looked for
    for n_positions, n_groups, n_quals in ((-1, 0, 40), (1, -1, 40), (1, 33, 40), (1, 0, 0), (1, 0, 2), (1, 0, 42), (1, 0, 132), (1, 0, -4), (1, 5, 127)):
        h = C.c_void_p(5)
        assert L.bvc_site_acc_create_quals(C.byref(h), 0, n_positions, n_groups, n_quals, 0) == bm.ERR_ARG and not h.value, (n_positions, n_groups, n_quals)


def test_the_new_source_is_built_and_in_the_isa_reports_list():
    from basevarc_amd import build as b
    from tests import test_bam_counts_abi as t8
    assert any(d.endswith("bvc_site_acc_quals.h") for d in b.DEPS)
    t8.check_the_counts_kernels()                     # (bam_counts_kernel.hip: both passes are bam_counts_kernel<ADD, Narrow>)
    text = open(os.path.join(ROOT, "basevarc_amd", "csrc", t8.COUNTS_SOURCE)).read()
    for kernel in ("bam_counts_kernel", "first_status_kernel", "acc_expand_kernel"):
        assert kernel in text, kernel


def test_the_byte_formula_and_what_it_buys():
    assert qm.acc_bytes(1, 128) == 2048 + 48 and qm.acc_bytes(1, 128, 5) == 2048 + 48 + 80           # the first and the second kind's bytes
    assert qm.acc_bytes(1, 48) == 816 and qm.acc_bytes(1, 4, 32) == 64 + 48 + 512
    assert qm.acc_bytes(66615, 128) == 139625040 and qm.acc_bytes(66615, 40) == 45831120             # the budget test's two runs
    assert qm.acc_bytes(66615, 40, 5) == 66615 * (640 + 48 + 80)
    # 288 GB hold about 137 million wide positions; chromosome 1 (248,956,422 bp) takes 203 GB at 48 columns
    assert 288e9 // 2096 == 137404580 and 203e9 < qm.acc_bytes(248956422, 48) < 204e9 and qm.acc_bytes(248956422, 128) > 288e9
    assert [q for q in range(-4, 140) if qm.quals_ok(q)] == list(range(4, 129, 4))


def test_the_layouts_sizes_are_the_models_and_the_headers(tmp_path):
    """csrc/counts_layout.h in a stand-alone program (tests/cpp/counts_layout_main.cpp) built with -fsanitize=address,undefined: every kind's
    sizes against tests/bam_counts_quals_model.py, tests/acc_pack_model.py and the closed forms of the three headers."""
    from tests import acc_pack_model as pm
    exe = str(tmp_path / "counts_layout")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "basevarc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "counts_layout_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    lines = text.splitlines()
    want = [("wide", g, 128) for g in (0, 1, 5, 32)] + [("with_depth", g, 128) for g in (1, 5, 32)] + \
        [("narrow", g, q) for q in (4, 40, 124, 128) for g in (0, 5, 32)]
    assert len(lines) == len(want) + 1 == 20
    for line, (kind, g, q) in zip(lines, want):
        head, _, tail = line.partition(" -> ")
        assert head.split() == [kind, str(g), str(q)], line
        count_words, logical_words, bytes_per_position, expanded, label_groups = (int(x) for x in tail.split())
        slots, depth_groups = (g + 1 if g else 1, 0) if kind == "wide" else (1, g)
        assert count_words == slots * 4 * q and logical_words == pm.row_words(slots, depth_groups) == slots * 512 + 10 + 4 * depth_groups, line
        assert bytes_per_position == 4 * count_words + 48 + 16 * depth_groups and expanded == (q < 128) and label_groups == g, line
        if kind == "wide":
            assert count_words == slots * 512 and bytes_per_position == slots * 2048 + 48, line
        else:
            assert count_words == 4 * q and bytes_per_position == qm.acc_bytes(1, q, g), line
    assert lines[-1].split() == ["quals_ok"] + [str(q) for q in range(4, 129, 4)]
    assert [q for q in range(-4, 140) if qm.quals_ok(q)] == list(range(4, 129, 4))


def test_the_model_by_hand_on_two_tiny_cases():
    R = bm.make_read
    A, Cc, G, T = 0, 1, 2, 3
    # 1. one sample, qualities 7, 3, 128 and 255 over ACGT at 1010..1013, eight columns
    one = [(bm.pack_record(R(1009, "4M", seq="ACGT", qual=[7, 3, 128, 255])), True, 0)]
    positions = [1010, 1011, 1012, 1013]
    exp = qm.expected(one, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 8)
    assert exp["rc"] == 0 and exp["status"] == [0] and exp["depth"] is None
    want = np.zeros((4, 4, 8), dtype=np.uint32)
    want[0, A, 7] = 1; want[1, Cc, 3] = 1                      # 128 and 255 are tallied, never counted and never a refusal
    assert exp["counts"].dtype == np.uint32 and exp["counts"].shape == (4, 4, 8) and (exp["counts"] == want).all()
    assert exp["tally"]["strand_base"][:, 4:].sum(axis=1).tolist() == [1, 1, 1, 1]
    wide = cm.expected(one, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ))
    assert (qm.expand(exp["counts"]) == wide["counts"].reshape(4, 512)).all() and exp["tally"].tobytes() == wide["tally"].tobytes()
    # one column fewer than the highest quality needs (4: the 7 has no column): status 5, ERR_DATA, nothing to add
    short = qm.expected(one, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 4)
    assert short["rc"] == bm.ERR_DATA and short["status"] == [5] and short["counts"] is None and short["tally"] is None
    # 2. three samples with two groups: the second's quality 8 is refused at eight columns whatever the others hold (and its 127 at 124
    # columns); at 128 the depths are the ninth header's, and the existing verdict (a cut record: status 3) goes first and keeps its status beside the 5
    reads = [R(1009, "3M", seq="ACG", qual=[0, 1, 2]), R(1009, "3M", seq="TTT", qual=[7, 8, 127], flag=0x10), R(1010, "2M", seq="GN", qual=[5, 5])]
    three = [(bm.pack_record(r), True, 0) for r in reads]
    positions = [1010, 1011, 1012]
    refused = qm.expected(three, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 8, [1, 0, 7], 2)
    assert refused["rc"] == bm.ERR_DATA and refused["status"] == [0, 5, 0] and refused["depth"] is None
    assert qm.expected(three, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 124, [1, 0, 7], 2)["status"] == [0, 5, 0]      # (the 127)
    ok = qm.expected(three, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 128, [1, 0, 7], 2)
    assert ok["rc"] == 0 and ok["status"] == [0, 0, 0] and ok["counts"].shape == (3, 4, 128) and int(ok["counts"].sum()) == 7
    depth = np.zeros((3, 2, 4), dtype=np.uint32)
    depth[0, 1, A] = 1; depth[1, 1, Cc] = 1; depth[2, 1, G] = 1; depth[:, 0, T] = 1          # (the third sample is in no group)
    assert (ok["depth"] == depth).all() and ok["tally"]["n_other"].tolist() == [0, 0, 1]
    assert (ok["counts"].reshape(3, 512) == cm.expected(three, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ))["counts"].reshape(3, 512)).all()
    cut = [three[0], three[1], (three[2][0][:-3], True, 0)]
    both = qm.expected(cut, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), 8, [1, 0, 7], 2)
    assert both["rc"] == bm.ERR_DATA and both["status"] == [0, 5, 3] and both["counts"] is None
    # expand() puts the columns where the wide layout has them and zeros elsewhere
    rows = np.arange(2 * 4 * 8, dtype=np.uint32).reshape(2, 4, 8) + 1
    wide = qm.expand(rows).reshape(2, 4, 128)
    assert (wide[:, :, :8] == rows).all() and not wide[:, :, 8:].any() and (qm.narrow(wide.reshape(2, 512), 8) == rows).all()


def test_status_four_outranks_status_five_in_one_sample():
    """The header's precedence: the out-of-range rule at one position and a quality without a column at another leave status 4."""
    c = next(x for x in bc.catalogue() if x["name"] == "a query offset past the sequence")
    assert bc.expected(c)["status"] == [4] and c["positions"] == [1012, 1016]
    assert min(bm.make_read(1010, "10M", seq="ACGTA", qual=[30] * 5)["qual"]) >= 8                     # 1012 holds a base of quality 30
    exp = qm.expected(None, None, None, None, c["positions"], None, None, 8, exp=bc.expected(c))
    assert exp["rc"] == bm.ERR_DATA and exp["status"] == [4]


def test_on_the_test_bams_forty_columns_hold_every_count_and_thirty_six_do_not():
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    pv = pv[::13]
    rid = [refs.index(contig) for _, _, refs in data]
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    quals = qm.counted_qualities(exp["maps"])
    assert exp["rc"] == 0 and len(quals) > 30000 and min(quals) >= 1 and max(quals) == 39
    forty = qm.expected(None, None, None, None, pv, None, None, 40, exp=exp)
    assert forty["rc"] == 0 and 5 not in forty["status"] and int(forty["counts"].sum()) == len(quals)
    wide = cm.fold(exp["maps"], pv)[0]
    assert (qm.expand(forty["counts"]) == wide.reshape(len(pv), 512)).all()
    thirty_six = qm.expected(None, None, None, None, pv, None, None, 36, exp=exp)
    assert thirty_six["rc"] == bm.ERR_DATA and thirty_six["status"].count(5) > 50 and thirty_six["counts"] is None


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from basevarc_amd import build as b
    return b.build_host()


def test_the_knobs_parse_rule(built):
    H = C.CDLL(built[1])
    H.bvchost_parse_counts_quals.restype = C.c_int32
    H.bvchost_parse_counts_quals.argtypes = [C.c_char_p]
    assert H.bvchost_parse_counts_quals(None) == 128
    for q in range(0, 200):
        assert H.bvchost_parse_counts_quals(str(q).encode()) == (q if qm.quals_ok(q) else -1), q
    for text in (b"", b" 40", b"40 ", b"+40", b"-40", b"4e1", b"0x28", b"40.0", b"forty", b"auto", b"040x", b"1280", b"4294967336"):
        assert H.bvchost_parse_counts_quals(text) == -1, text
    assert H.bvchost_parse_counts_quals(b"040") == 40                         # (plain digits)


def counts_run(exe, tmp_path, fmt, knob, sub):
    """(the finished run, what it left in its output directory): a run on inputs that do not exist."""
    env = dict(os.environ)
    env.pop("BVC_HOST_COUNTS_QUALS", None)
    if knob is not None:
        env["BVC_HOST_COUNTS_QUALS"] = knob
    out = tmp_path / sub
    out.mkdir()
    r = subprocess.run([exe, "basetype", "--tmp-format", fmt, "-i", str(out / "none.list"), "-r", "none.fa", "-s", "chr1:1-2", "-o", str(out / "o")],
                       capture_output=True, text=True, env=env)
    return r, os.listdir(str(out))


def test_a_bad_knob_value_is_refused_before_anything_is_opened_and_only_with_counts(built, tmp_path):
    for i, knob in enumerate(("0", "2", "42", "132", "-4", "forty", "")):
        r, left = counts_run(built[0], tmp_path, "counts", knob, f"bad{i}")
        assert r.returncode == 1 and r.stderr.count("\n") == 1 and "BVC_HOST_COUNTS_QUALS must be a multiple of 4 in 4..128" in r.stderr and left == [], (knob, r.stderr)
    # a good value, or none, passes this check: the run then ends on its next one (the input list is empty), naming no knob
    for i, knob in enumerate(("40", "128", "4", None)):
        r, left = counts_run(built[0], tmp_path, "counts", knob, f"good{i}")
        assert r.returncode == 1 and "BVC_HOST_COUNTS_QUALS" not in r.stderr and left == [], (knob, r.stderr)
    # every other format ignores the knob, whatever it holds
    for fmt in ("bin", "mem"):
        r, left = counts_run(built[0], tmp_path, fmt, "forty", "other_" + fmt)
        assert r.returncode == 1 and "BVC_HOST_COUNTS_QUALS" not in r.stderr, (fmt, r.stderr)
    usage = subprocess.run([built[0], "basetype", "--help"], capture_output=True, text=True)
    assert "BVC_HOST_COUNTS_QUALS=Q" in usage.stdout + usage.stderr
