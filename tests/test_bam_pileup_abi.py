"""bvc_bam_pileup as far as a machine without a GPU can see it: the entry point is declared (include/bvc_bam.h, which bvc.h names),
exported, in the binding's third table and refuses a null context; the new kernels are built from their own source without private
memory, scratch, flat addressing or spills; and the Python model that judges the device (tests/bam_pileup_model.py) is itself held to the
CPU path: its records for the 100 test BAMs are the host program's `--load --tmp-format raw` temp batches, and its tokens for the random
cases are bvchost_pileup_tokens'."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def third_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_bam.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = open(os.path.join(ROOT, "include", "bvc_bam.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    decls = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\*?)\s*\b(bvc_\w+)\s*\(([^;{}()]*)\)\s*;", txt):
        assert name not in decls, name
        decls[name] = (" ".join(ret.split()), [p.strip() for p in " ".join(params.split()).split(",")])
    return decls


def test_the_library_the_header_and_the_binding_know_the_entry_point():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    # bvc.h's list of entry points is closed (tests/test_binding_abi.py): the new one is declared in a header of its own that includes
    # bvc.h and that bvc.h names, and bound from a table of its own, name by name and type by type as the first
    decls = third_header_declarations()
    assert list(decls) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    assert not set(decls) & set(ta.header_declarations()) and not set(bl.BAM_PROTOTYPES) & (set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES))
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.BAM_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is ta.RETURNS[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    params = decls["bvc_bam_pileup"][1]
    assert params[:4] == ["bvc_ctx *ctx", "int32_t n_samples", "const uint8_t *bam", "int64_t bam_bytes"] and params[-1] == "uint32_t flags"
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert '#include "bvc.h"' in open(os.path.join(ROOT, "include", "bvc_bam.h")).read() and "bvc_bam.h" in header
    assert re.search(r"#define BVC_BAM_MORE\s+2\b", header) and bl.BAM_MORE == bm.BAM_MORE == 2
    assert callable(getattr(bl.Context, "bam_pileup", None))
    # the host program reads its knob: default 0, acting on the binary forms only (host/main.cpp)
    knobs = open(os.path.join(ROOT, "basevarc_amd", "host", "knobs.h")).read()
    assert re.search(r'device_pileup = num\("BVC_HOST_DEVICE_PILEUP", 0\) != 0;', knobs)
    assert 'knobs.device_pileup && opt::tmp_format != "text"' in open(os.path.join(ROOT, "basevarc_amd", "host", "main.cpp")).read()
    # no context: refused before anything of the device is touched
    need = C.c_int64(7)
    assert L.bvc_bam_pileup(None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(need), None, None, 0) == bm.ERR_ARG
    assert L.bvc_bam_pileup_bgzf(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, 0, C.byref(need), None, None) == bm.ERR_ARG


def test_the_kernels_are_built_from_their_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "bam_pileup_kernel.hip" in b.SOURCES and "bvc_bam.hip" in b.SOURCES
    assert "bam_pileup_kernel.hip" in isa_report.DEVICE_SOURCES
    rows = {re.match(r"(?:bvc::)?([\w<>]+)", k["pretty"]).group(1): k for k in isa_report.kernels_of(isa_report.assembly("bam_pileup_kernel.hip"))}
    assert set(rows) == {"bam_index_kernel", "bam_pileup_kernel<false>", "bam_pileup_kernel<true>", "bam_rows_kernel<false>",
                         "bam_rows_kernel<true>", "bam_scan_kernel"}, sorted(rows)
    for name, k in rows.items():
        assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)


# ---- the model against the CPU path ---------------------------------------------------------------------------------------------------
def test_the_catalogue_and_the_seeds_meet_their_census():
    """Chosen so that the model alone shows it: the random cases hold indel entries, entries taken from a read behind the first covering
    one, and every status; the catalogue holds every status and return code too."""
    tot, fall = {}, 0
    for seed in bc.RANDOM_SEEDS:
        c = bc.random_case(seed)
        e = bc.expected(c)
        for k, v in bm.census(e).items():
            tot[k] = tot.get(k, 0) + v
        tot[f"rc{e['rc']}"] = tot.get(f"rc{e['rc']}", 0) + 1
        for (data, eof, rid), m in zip(c["samples"], e["maps"]):
            _, rv = bm.scan_sample(data, eof, rid, c["beg0"], c["end0"], c["min_mapq"])
            fall += sum(1 for p, x in m.items() if not x["is_indel"] and x["mapq"] != next(r for r in rv if bm.tp.end_pos(r) >= p)["mapq"])
    assert len(bc.RANDOM_SEEDS) == 40 and all(1 <= len(bc.random_case(s)["samples"]) <= 12 for s in bc.RANDOM_SEEDS)
    assert tot["indel"] > 100 and tot["base"] > 5000 and fall > 0, (tot, fall)
    assert all(tot.get(f"status{s}", 0) > 0 for s in range(5)) and all(tot.get(f"rc{r}", 0) > 0 for r in (0, 2, -5)), tot
    cat = {}
    for c in bc.catalogue():
        for k, v in bm.census(bc.expected(c)).items():
            cat[k] = cat.get(k, 0) + v
    assert all(cat.get(f"status{s}", 0) > 0 for s in range(5)) and cat["indel"] > 100, cat
    assert len({c["name"] for c in bc.catalogue()}) == len(bc.catalogue())


@pytest.fixture(scope="module")
def host():
    from basevarc_amd import build as b
    exe, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_pileup_tokens.restype = C.c_size_t
    H.bvchost_pileup_tokens.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.c_size_t]
    return exe, H


def _token(e):
    if e is None:
        return ". "
    return e["indel"] + " " if e["is_indel"] else f"{e['base']},{e['mapq']},{e['qual']},{e['rpr']},{e['strand']} "


def test_every_random_cases_tokens_are_the_host_programs(host):
    """Per sample of every random case: the kept reads through bvchost_pileup_tokens (find_snp_at_pos of host/bam.cpp) against the
    model's entries; where the model says status 4 the host's rule throws."""
    _, H = host
    checked = thrown = 0
    buf = C.create_string_buffer(1 << 20)
    for seed in bc.RANDOM_SEEDS:
        c = bc.random_case(seed)
        e = bc.expected(c)
        pv = c["positions"]
        arr = (C.c_int32 * len(pv))(*pv)
        for (data, eof, rid), st, m in zip(c["samples"], e["status"], e["maps"]):
            if st not in (0, 4):
                continue
            _, rv = bm.scan_sample(data, eof, rid, c["beg0"], c["end0"], c["min_mapq"])
            H.bvchost_pileup_tokens(bc.reads_text(rv).encode(), arr, len(pv), c["rg_s"], c["refseq"].encode(), buf, len(buf))
            got = buf.value.decode()
            if st == 4:
                assert got.startswith("!"), (seed, got[:80])
                thrown += 1
            else:
                assert got == "".join(_token(m.get(p)) for p in pv), (seed, got[:200])
                checked += len(pv)
    assert checked > 10000 and thrown > 0, (checked, thrown)


def bam_data_bytes():
    """[(inflated bytes, offset of the first alignment record, the reference names)] of the 100 test BAMs, in the list's order."""
    from tests import hostref
    out = []
    for line in open(os.path.join(hostref.DATA, "bam.list")):
        if not line.strip():
            continue
        d = gzip.open(os.path.join(hostref.DATA, line.strip().replace("data/", "", 1))).read()
        off = 8 + int.from_bytes(d[4:8], "little")
        n_ref = int.from_bytes(d[off:off + 4], "little")
        off += 4
        refs = []
        for _ in range(n_ref):
            ln = int.from_bytes(d[off:off + 4], "little")
            refs.append(d[off + 4:off + 4 + ln - 1].decode())
            off += 8 + ln
        out.append((d, off, refs))
    return out


def bam_data_call(mapq=20):
    """The arguments bt_r's fetch and find_snp_at_pos get for the test data: (beg0, end0, min_mapq, positions, rg_s, refseq)."""
    from tests import hostref
    contig, start, _, refseq = hostref.region_fixture()
    _, s, e = bm.tp.REGION
    rg_s, rg_e = s, e - 1
    pv = [rg_s + i for i in range(len(refseq) - 1000) if refseq[i] in "ACGT"]
    return contig, max(0, rg_s - 1 - 1000), rg_e + 1000, mapq, pv, rg_s, refseq


@pytest.mark.parametrize("batch", [7, 100])
def test_the_models_records_for_the_test_bams_are_the_host_programs(host, tmp_path, batch):
    """`BaseVarC basetype --load --tmp-format raw` on the 100 test BAMs: the inflated bytes behind every batch file's header are the
    model's records of that batch's samples."""
    from tests import hostref
    exe, _ = host
    fa = hostref.write_fasta(str(tmp_path / "chr17.fa"))
    lst = hostref.write_bam_list(str(tmp_path / "bam.list"))
    out = str(tmp_path / "test.out")
    subprocess.run([exe, "basetype", "--load", "--tmp-format", "raw", "-q", "20", "-t", "1", "-b", str(batch), "-i", lst, "-s", hostref.REGION,
                    "-r", fa, "-o", out], check=True, capture_output=True)
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    data = bam_data_bytes()
    for ib in range(1 + (len(data) - 1) // batch):
        part = data[ib * batch:(ib + 1) * batch]
        exp = bm.expected([(d[off:], True, refs.index(contig)) for d, off, refs in part], beg0, end0, mapq, pv, rg_s, refseq)
        assert exp["rc"] == 0
        raw = gzip.open(f"{out}.tmp.thread.0/batch.{ib}").read()
        assert raw[:8] == b"BVCBAT1\n" and int.from_bytes(raw[8:12], "little") == len(part)
        head = 16 + int.from_bytes(raw[12:16], "little")
        assert raw[head:] == exp["records"], ib


def test_the_block_gathering_and_the_window_cuts_under_the_address_sanitizer(tmp_path):
    """host/bam_blocks.cpp in a stand-alone program (tests/cpp/bam_blocks_main.cpp) built with -fsanitize=address,undefined, on the 100
    test BAMs and on two damaged copies: one cut inside a BGZF block, one with a payload byte flipped."""
    from tests import hostref
    host = os.path.join(ROOT, "basevarc_amd", "host")
    exe = str(tmp_path / "bam_blocks")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-pthread", "-I", host, os.path.join(ROOT, "tests", "cpp", "bam_blocks_main.cpp")] +
                          [os.path.join(host, f) for f in ("bam_blocks.cpp", "bam.cpp", "bgzf.cpp", "inflate.cpp")] + ["-lz", "-o", exe])
    files = [os.path.join(hostref.DATA, l.strip().replace("data/", "", 1)) for l in open(os.path.join(hostref.DATA, "bam.list")) if l.strip()]
    raw = open(files[0], "rb").read()
    cut, flipped = str(tmp_path / "cut.bam.bad"), str(tmp_path / "flipped.bam.bad")
    open(cut, "wb").write(raw[:len(raw) * 2 // 3])
    open(flipped, "wb").write(raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 0x5A]) + raw[len(raw) // 2 + 1:])
    contig, beg0, end0, _, _, _, _ = bam_data_call()
    r = subprocess.run([exe, contig, str(beg0), str(end0)] + files + [cut, flipped], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert "102 files, 0 wrong" in text
