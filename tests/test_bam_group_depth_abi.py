"""The groups' depths beside one slot of class counts (include/bvc_bam_group_depth.h) as far as a machine without a GPU can see them: the
entry points are declared, exported, in the binding's ninth table and refuse a null context and a bad shape; the eight older lists are what
they were; the new kernel is built from its own source, one kernel without private memory, scratch, flat addressing, spills or MFMA in the
product and the diagnostic build; the model (tests/bam_group_depth_model.py) folds the hand-made batch as the header says; and the host
program's knob, its refusals and its label rule (host/pileup.h, counts_group_map)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_counts_model as cm
from tests import bam_group_depth_model as gm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_bam_counts_depth", "bvc_site_acc_create_depth", "bvc_site_acc_get_depth"]


def declarations_of(header):
    """{name: (return type, [parameter text])} of a header under include/, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(bvc_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        assert name not in decls, name
        decls[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",")])
    return decls


def test_the_library_the_header_and_the_binding_know_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_bam_counts_abi as t8
    from tests import test_bam_pileup_abi as tb
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    decls = declarations_of("bvc_bam_group_depth.h")
    assert list(decls) == bl.BAM_GROUP_DEPTH_EXPORTS == list(bl.BAM_GROUP_DEPTH_PROTOTYPES) == NAMES
    # the eight older lists are what they were, and none of them holds a new name
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(tb.third_header_declarations()) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    assert list(t8.eighth_header_declarations()) == bl.BAM_COUNTS_EXPORTS == t8.NAMES
    older = (bl.PROTOTYPES, bl.BGZF_CODES_PROTOTYPES, bl.BAM_PROTOTYPES, bl.POPMATRIX_PROTOTYPES, bl.BAM_TEXT_PROTOTYPES, bl.STORE_PROTOTYPES,
             bl.BAM_DEFLATE_PROTOTYPES, bl.BAM_COUNTS_PROTOTYPES)
    assert [len(t) for t in older[1:]] == [1, 2, 2, 2, 9, 3, 7], [len(t) for t in older]
    for table in older:
        assert not set(table) & set(decls)
    returns = dict(ta.RETURNS, void=None)
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.BAM_GROUP_DEPTH_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is returns[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # bvc_bam_counts_depth takes bvc_bam_counts's arguments up to refseq_len, name for name; then its own
    mine, twin = decls["bvc_bam_counts_depth"][1], t8.eighth_header_declarations()["bvc_bam_counts"][1]
    k = next(i for i, p in enumerate(twin) if p.endswith("refseq_len")) + 1
    assert mine[:k] == twin[:k] and k == 15
    assert [p.split()[-1].lstrip("*") for p in mine[k:]] == ["group_of_sample", "n_groups", "counts", "tally", "group_depth", "sample_status", "flags"]
    assert mine[k:k + 4] == twin[k:k + 4] and mine[-2:] == twin[-2:]
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc_bam_counts.h"' in open(os.path.join(ROOT, "include", "bvc_bam_group_depth.h")).read() and "bvc_bam_group_depth.h" in header
    for m in ("create_depth", "get_depth"):
        assert callable(getattr(bl.SiteAcc, m, None)), m
    assert callable(getattr(bl.Context, "bam_counts_depth", None))
    # no context: refused before anything of the device is touched
    assert L.bvc_bam_counts_depth(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, 0, None, 1, None, None, None, None, 0) == bm.ERR_ARG
    assert L.bvc_site_acc_get_depth(None, None, 0, 0, None) == bm.ERR_ARG
    assert L.bvc_site_acc_create_depth(None, 0, 1, 1, 0) == bm.ERR_ARG
    # an accumulator's shape is refused before the device is looked for
    h = C.c_void_p(5)
    for n_positions, n_groups in ((-1, 1), (1, 0), (1, 33), (1, -1)):
        assert L.bvc_site_acc_create_depth(C.byref(h), 0, n_positions, n_groups, 0) == bm.ERR_ARG and not h.value
        h = C.c_void_p(5)


def test_the_kernel_is_one_built_from_its_own_source_without_private_memory_or_flat_addressing():
    from basevarc_amd import build as b
    from tests import test_bam_counts_abi as t8
    assert any(d.endswith("bvc_bam_group_depth.h") for d in b.DEPS)
    t8.check_the_counts_kernels()                     # (bam_counts_kernel.hip: the add pass is bam_counts_kernel<true, Depth>)


def test_the_model_folds_the_hand_made_batch_as_the_header_says():
    """The three samples of tests/test_bam_counts_abi.py's hand-made batch: a quality byte above 127, an N, an insertion and a label outside
    the two groups add no depth; everything that adds a class count adds it to the one slot."""
    R = bm.make_read
    reads = [R(1009, "4M", seq="ACGT", qual=[30, 127, 128, 255], flag=0),
             R(1009, "2M2I2M", seq="CNGGTT", qual=[10, 11, 12, 13, 14, 15], flag=0x10),       # an N at 1011; "+GG" at 1011
             R(1010, "3M", seq="GGG", qual=[5, 5, 5], flag=0)]
    samples = [(bm.pack_record(r), True, 0) for r in reads]
    positions = [1010, 1011, 1012, 1013]
    exp = gm.expected(samples, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), [1, 0, 7], 2)
    assert exp["rc"] == 0 and exp["status"] == [0, 0, 0]
    A, Cc, G, T = 0, 1, 2, 3
    depth = np.zeros((4, 2, 4), dtype=np.uint32)
    depth[0, 1, A] = 1; depth[0, 0, Cc] = 1           # 1010: A q30 of group 1, C q10 of group 0
    depth[1, 1, Cc] = 1                               # 1011: C q127 of group 1; group 0's sample holds the insertion; G q5 is in no group
    depth[2, 0, T] = 1                                # 1012: group 1's G has quality 128; T q14 of group 0; G q5 in no group
    depth[3, 0, T] = 1                                # 1013: group 1's T has quality 255; T q15 of group 0; G q5 in no group
    assert exp["depth"].dtype == np.uint32 and (exp["depth"] == depth).all(), np.argwhere(exp["depth"] != depth)
    counts = np.zeros((4, 512), dtype=np.uint32)
    for t, cls in ((0, A * 128 + 30), (0, Cc * 128 + 10), (1, Cc * 128 + 127), (1, G * 128 + 5), (2, G * 128 + 5), (2, T * 128 + 14), (3, T * 128 + 15),
                   (3, G * 128 + 5)):
        counts[t, cls] += 1
    assert (exp["counts"] == counts).all()
    # the one slot and the tally are what the plain call adds without groups
    plain = cm.expected(samples, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ))
    assert (plain["counts"].reshape(4, 512) == exp["counts"]).all() and plain["tally"].tobytes() == exp["tally"].tobytes()
    assert exp["tally"]["n_indel"].tolist() == [0, 1, 0, 0] and int(exp["tally"]["strand_base"].sum()) == 10 and int(exp["depth"].sum()) == 5
    # the same from the entries themselves
    maps = bm.expected(samples, 0, 1 << 30, 20, positions, bc.RG_S, "N" * len(bc.REFSEQ))["maps"]
    direct = gm.fold_maps(maps, positions, [1, 0, 7], 2)
    assert (direct[0] == exp["counts"]).all() and direct[1].tobytes() == exp["tally"].tobytes() and (direct[2] == exp["depth"]).all()
    # with the third sample in group 1 its G counts; an N where the position is not the insertion's anchor adds nothing anywhere
    three = gm.expected(samples, 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), [1, 0, 1], 2)
    assert three["depth"][:, 1, G].tolist() == [0, 1, 1, 1] and int(three["depth"].sum()) == 8
    n_at = gm.expected([(bm.pack_record(R(1009, "3M", seq="CNG", qual=[9, 9, 9])), True, 0)], 0, 1 << 30, 20, [1011], bc.RG_S, len(bc.REFSEQ), [0], 1)
    assert n_at["tally"]["n_other"].tolist() == [1] and not n_at["depth"].any() and not n_at["counts"].any()
    # a failing batch adds nothing
    bad = gm.expected([(bm.pack_record(reads[0])[:-3], True, 0)], 0, 1 << 30, 20, positions, bc.RG_S, len(bc.REFSEQ), [0], 1)
    assert bad["rc"] == bm.ERR_DATA and bad["status"] == [3] and bad["counts"] is None and bad["tally"] is None and bad["depth"] is None


# ---- the host program -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from basevarc_amd import build as b
    return b.build_host()


def counts_run(exe, tmp_path, extra, knob, sub="out"):
    """(the finished run, what it left in its output directory): --tmp-format counts on inputs that do not exist."""
    env = dict(os.environ)
    env.pop("BVC_HOST_COUNTS_GROUPS", None)
    if knob is not None:
        env["BVC_HOST_COUNTS_GROUPS"] = knob
    out = tmp_path / sub
    out.mkdir()
    r = subprocess.run([exe, "basetype", "--tmp-format", "counts", "-i", str(out / "none.list"), "-r", "none.fa", "-s", "chr1:1-2", "-o", str(out / "o")] + extra,
                       capture_output=True, text=True, env=env)
    return r, os.listdir(str(out))


@pytest.mark.parametrize("extra, line", [(["--load"], "--tmp-format counts with --load"), (["--keep_tmp"], "--tmp-format counts with --keep_tmp"),
                                         (["--gpus", "2"], "--tmp-format counts with --gpus above 1")])
def test_with_the_knob_and_no_group_file_the_other_refusals_are_unchanged(built, tmp_path, extra, line):
    r, left = counts_run(built[0], tmp_path, extra, "1")
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and line in r.stderr and left == [], r.stderr


@pytest.mark.parametrize("knob", [None, "0"])
def test_without_the_knob_the_group_file_is_refused_with_the_line_that_names_mem(built, tmp_path, knob):
    r, left = counts_run(built[0], tmp_path, ["--group", str(tmp_path / "none.txt")], knob)
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and "--tmp-format counts with --group" in r.stderr and "--tmp-format mem" in r.stderr, r.stderr
    assert r.stderr.rstrip().endswith("BVC_HOST_COUNTS_GROUPS=1)") and left == []


def test_with_the_knob_a_file_of_thirty_three_group_names_ends_the_run_before_anything_is_made(built, tmp_path):
    groups = tmp_path / "groups.txt"
    groups.write_text("".join(f"S{i}\tG{i:02d}\n" for i in range(33)))
    r, left = counts_run(built[0], tmp_path, ["--group", str(groups)], "1")
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and "--tmp-format mem" in r.stderr and "33 group names" in r.stderr and left == [], r.stderr
    # thirty-two names pass this check: the run then ends on its next one (the reference file is missing), naming neither
    groups.write_text("".join(f"S{i}\tG{i % 32:02d}\n" for i in range(40)))
    r, left = counts_run(built[0], tmp_path, ["--group", str(groups)], "1", sub="second")
    assert r.returncode == 1 and "--tmp-format mem" not in r.stderr and "group names" not in r.stderr and left == [], r.stderr


@pytest.fixture(scope="module")
def H(built):
    h = C.CDLL(built[1])
    h.bvchost_counts_group_map.restype = C.c_int32
    h.bvchost_counts_group_map.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    return h


def host_group_map(H, lines, samples):
    text = "".join(f"{i}\t{g}\n" for i, g in lines).encode()
    label = np.full(len(samples) + 8, 0xEE, dtype=np.uint8)
    cols = np.full(64 + 8, -7, dtype=np.int32)
    n_cols = C.c_int32(-1)
    n_names = H.bvchost_counts_group_map(text, "".join(s + "\n" for s in samples).encode(), C.c_void_p(label.ctypes.data), C.c_void_p(cols.ctypes.data), 64,
                                         C.byref(n_cols))
    assert (label[len(samples):] == 0xEE).all() and (cols[n_cols.value:] == -7).all()
    return n_names, label[:len(samples)].tolist(), cols[:n_cols.value].tolist()


def test_the_label_rule_is_the_models():
    """The model's own rule on a case small enough to check by hand: the file's first and last sorted names have no sample."""
    lines = [("x1", "AAA"), ("s2", "POP2"), ("s0", "POP1"), ("s3", "POP2"), ("x2", "ZZZ"), ("s0", "POP2")]
    names, label, cols = gm.group_map(lines, ["s0", "s1", "s2", "s3"])
    assert names == ["AAA", "POP1", "POP2", "ZZZ"] and label == [1, 255, 2, 2] and cols == [1, 2]


def test_the_host_programs_label_rule_is_the_models(H):
    lines = [("x1", "AAA"), ("s2", "POP2"), ("s0", "POP1"), ("s3", "POP2"), ("x2", "ZZZ"), ("s0", "POP2")]
    assert host_group_map(H, lines, ["s0", "s1", "s2", "s3"]) == (4, [1, 255, 2, 2], [1, 2])
    assert host_group_map(H, [], ["a", "b"]) == (0, [255, 255], [])
    assert host_group_map(H, lines, []) == (4, [], [])
    rng = np.random.default_rng(20271020)
    for trial in range(200):
        n_names = int(rng.integers(1, 33))
        pool = [f"g{int(x):03d}" for x in rng.choice(500, size=n_names, replace=False)]
        ids = [f"id{int(x)}" for x in rng.integers(0, 60, size=int(rng.integers(1, 80)))]          # (some listed twice, some never)
        lines = [(i, pool[int(rng.integers(0, n_names))]) for i in ids]
        samples = [f"id{int(x)}" for x in rng.permutation(70)[:int(rng.integers(0, 50))]]
        names, label, cols = gm.group_map(lines, samples)
        got = host_group_map(H, lines, samples)
        assert got == (len(names), label, cols), trial
        # what the program's read_groups makes of all the names: the groups that have a sample, sorted -- a subsequence of the file's names
        first = {}
        for i, g in lines:
            first.setdefault(i, g)
        have = sorted({first[s] for s in samples if s in first})
        assert [names[c] for c in cols] == have
        assert all((l == 255) == (s not in first) and (l == 255 or names[l] == first[s]) for s, l in zip(samples, label))
