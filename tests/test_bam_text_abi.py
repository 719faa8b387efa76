"""bvc_bam_pileup_text as far as a machine without a GPU can see it: both entry points are declared (include/bvc_bam_text.h, which bvc.h
names), exported, in the binding's fifth table and refuse a null context; the host program has its knob, off by default; the new kernels
are built from their own source without private memory, scratch, flat addressing or spills; and the Python model that judges the device
(tests/bam_text_model.py) is itself held to the CPU path: its lines for the 100 test BAMs are the host program's `--load --tmp-format text`
temp batches, and its tokens for the random cases are bvchost_pileup_tokens'."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import bam_text_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fifth_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_bam_text.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc_bam_text.h")).read()
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
    decls = fifth_header_declarations()
    assert list(decls) == bl.BAM_TEXT_EXPORTS == ["bvc_bam_pileup_text", "bvc_bam_pileup_text_bgzf"]
    # the closed lists stay as they were: bvc.h's is the first table, bvc_bam.h's the third
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(tb.third_header_declarations()) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    others = set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES) | set(bl.BAM_PROTOTYPES) | set(bl.POPMATRIX_PROTOTYPES)
    assert not set(decls) & (set(ta.header_declarations()) | set(tb.third_header_declarations())) and not set(bl.BAM_TEXT_PROTOTYPES) & others
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.BAM_TEXT_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is ta.RETURNS[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # the twins take their binary calls' arguments, type for type; only the outputs' names differ
    twin = tb.third_header_declarations()
    rename = lambda p: p.replace("records_needed", "text_needed").replace("records_cap", "text_cap").replace("records", "text").replace("rec_start", "line_start")
    assert [rename(p) for p in twin["bvc_bam_pileup"][1]] == decls["bvc_bam_pileup_text"][1]
    assert [rename(p) for p in twin["bvc_bam_pileup_bgzf"][1]] == decls["bvc_bam_pileup_text_bgzf"][1]
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc.h"' in open(os.path.join(ROOT, "include", "bvc_bam_text.h")).read() and "bvc_bam_text.h" in header
    assert callable(getattr(bl.Context, "bam_pileup_text", None)) and callable(getattr(bl.Context, "bam_pileup_text_bgzf", None))
    # no context: refused before anything of the device is touched
    need = C.c_int64(7)
    assert L.bvc_bam_pileup_text(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(need), None, None, 0) == bm.ERR_ARG
    assert L.bvc_bam_pileup_text_bgzf(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(need), None,
                                      None) == bm.ERR_ARG


def test_the_host_program_has_its_knob_off_by_default():
    knobs = open(os.path.join(ROOT, "basevarc_amd", "host", "knobs.h")).read()
    assert re.search(r'device_pileup_text = num\("BVC_HOST_DEVICE_PILEUP_TEXT", 0\) != 0;', knobs)
    main = open(os.path.join(ROOT, "basevarc_amd", "host", "main.cpp")).read()
    assert 'knobs.device_pileup_text && opt::tmp_format == "text"' in main
    # the binary knob's line and condition stay as they are
    assert re.search(r'device_pileup = num\("BVC_HOST_DEVICE_PILEUP", 0\) != 0;', knobs) and 'knobs.device_pileup && opt::tmp_format != "text"' in main


def test_the_kernels_are_built_from_their_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "bam_text_kernel.hip" in b.SOURCES and "bam_text_kernel.hip" in isa_report.DEVICE_SOURCES
    rows = {re.match(r"(?:bvc::)?([\w<>]+)", k["pretty"]).group(1): k for k in isa_report.kernels_of(isa_report.assembly("bam_text_kernel.hip"))}
    assert set(rows) == {"bam_text_token_kernel<false>", "bam_text_token_kernel<true>", "bam_text_rows_kernel<false>", "bam_text_rows_kernel<true>"}, sorted(rows)
    for name, k in rows.items():
        assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)


# ---- the model against the CPU path ---------------------------------------------------------------------------------------------------
def test_the_cases_meet_their_census():
    """Every case the text form adds is reached, shown by the model alone."""
    cases = tm.cases()
    assert len({c["name"] for c in cases}) == len(cases) and not {c["name"] for c in cases} & {c["name"] for c in bc.catalogue()}
    tot = {}
    for c in cases:
        assert tm.expected(c)["rc"] == bm.OK, c["name"]
        for k, v in tm.census(c).items():
            tot[k] = tot.get(k, 0) + v
    for f in ("mapq", "qual", "rpr"):
        assert all(tot.get((f, v), 0) > 0 for v in tm.WIDTHS), (f, sorted(k for k in tot if isinstance(k, tuple) and k[0] == f))
    assert all(tot.get(("base", v), 0) > 0 for v in range(5)) and all(tot.get(("strand", v), 0) > 0 for v in (0, 1))
    assert tot["one_byte_text"] > 0 and tot["long_text"] > 0 and tot["empty_line"] > 0 and tot["status1_among_covered"] > 0, tot
    assert tot["filler"] > tot["base"] > tot["indel"] > 0
    assert all(tot.get(("n_samples", n), 0) > 0 for n in (0, 1, 63, 64, 65, 129)), tot
    assert all(tot.get(("n_positions", n), 0) > 0 for n in (0, 1, 63, 64, 65, 1023, 1024, 1025)), tot
    by_name = {c["name"]: c for c in cases}
    # rpr wraps through 256: offset 255 shows 0, offset 256 shows 1
    c = by_name["every field at 0, 9, 10, 99, 100 and 255, rpr through 256"]
    m = tm.expected(c)["maps"][0]
    assert [m[1011 + k]["rpr"] for k in (254, 255, 256)] == [255, 0, 1]
    # the 1-byte text is the whole token "- "
    c = by_name["an indel text of 1 byte"]
    assert tm.token(tm.expected(c)["maps"][0][1029]) == "- " and b" - " in tm.expected(c)["text"]
    # the inserted bases, from an odd and from an even query index
    c = by_name["an insertion on an odd and on an even nibble"]
    for m, x, n in zip(tm.expected(c)["maps"], (tm.ODD_INSERTION, tm.EVEN_INSERTION), (2, 3)):
        ins = [e["indel"] for e in m.values() if e["is_indel"]]
        assert ins == ["+" + x["seq"][x["at"]:x["at"] + n]] and x["at"] % 2 == (1 if x is tm.ODD_INSERTION else 0), ins
    # the long deletion's token is whole in the lines, and cut in the binary records
    c = by_name["a deletion of 70,000 bases"]
    e = tm.expected(c)["maps"][0][1015]
    assert len(e["indel"]) == 1 + tm.LONG_DELETION and (e["indel"] + " ").encode() in tm.expected(c)["text"]
    assert len(bm.entry_bytes(e, 0)) == 11 + 0xffff


@pytest.fixture(scope="module")
def host():
    from basevarc_amd import build as b
    exe, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_pileup_tokens.restype = C.c_size_t
    H.bvchost_pileup_tokens.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.c_size_t]
    return exe, H


def test_every_token_of_the_random_cases_and_of_the_text_cases_is_the_host_programs(host):
    """Per sample of every seeded random case and of every case the text form adds: the kept reads through bvchost_pileup_tokens
    (find_snp_at_pos + format_pileup_token of the host program) against the model's column of the lines."""
    _, H = host
    checked = 0
    buf = C.create_string_buffer(4 << 20)
    for c in [bc.random_case(s) for s in bc.RANDOM_SEEDS] + tm.cases():
        e = tm.expected(c)
        pv = c["positions"]
        arr = (C.c_int32 * max(1, len(pv)))(*pv)
        for (data, eof, rid), st, m in zip(c["samples"], e["status"], e["maps"]):
            if st != 0:
                continue
            _, rv = bm.scan_sample(data, eof, rid, c["beg0"], c["end0"], c["min_mapq"])
            H.bvchost_pileup_tokens(bc.reads_text(rv).encode(), arr, len(pv), c["rg_s"], c["refseq"].encode(), buf, len(buf))
            assert buf.value.decode() == "".join(tm.token(m.get(p)) for p in pv), (c["name"], buf.value[:200])
            checked += len(pv)
    assert checked > 15000, checked


@pytest.mark.parametrize("batch", [7, 100])
def test_the_models_lines_for_the_test_bams_are_the_host_programs(host, tmp_path, batch):
    """`BaseVarC basetype --load --keep_tmp --tmp-format text` on the 100 test BAMs (the CPU path): every batch file inflates to its names
    line and the model's lines of that batch's samples.  Batch size 7 leaves a short last batch."""
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    exe, _ = host
    fa = hostref.write_fasta(str(tmp_path / "chr17.fa"))
    lst = hostref.write_bam_list(str(tmp_path / "bam.list"))
    out = str(tmp_path / "test.out")
    subprocess.run([exe, "basetype", "--load", "--keep_tmp", "--tmp-format", "text", "-q", "20", "-t", "1", "-b", str(batch), "-i", lst, "-s", hostref.REGION,
                    "-r", fa, "-o", out], check=True, capture_output=True)
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    n_batches = 1 + (len(data) - 1) // batch
    assert len(data) == 100 and (len(data) % batch != 0) == (batch == 7)
    for ib in range(n_batches):
        part = data[ib * batch:(ib + 1) * batch]
        exp = bm.expected([(d[off:], True, refs.index(contig)) for d, off, refs in part], beg0, end0, mapq, pv, rg_s, refseq)
        assert exp["rc"] == 0
        text, line_start = tm.lines(exp["maps"], pv)
        raw = gzip.open(f"{out}.tmp.thread.0/batch.{ib}").read()
        names, _, body = raw.partition(b"\n")
        assert names.count(b"\t") == len(part) and body == text and line_start[-1] == len(body), ib
