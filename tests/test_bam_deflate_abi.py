"""Phase 1's temp batches deflated on the device (include/bvc_bam_deflate.h) and tuning key "bgzf_cuts" as far as a machine without a GPU
can see them: the three entry points are declared, exported, in the binding's seventh table and refuse a null context; the key is declared in
the header and in the library's table of knobs; the host program reads its three knobs with their dependencies.  The plain Python model of the
field parse with DELIMITERS a space and a newline (tests/bgzf_fields_model.py: the model of "bgzf_cuts" = 1) on the text temp batches
tests/bam_text_model.py makes for its catalogue and for the 100 test BAMs (batches of 7 and 100, every 29th position): its symbols reproduce
every piece, zlib and the host program's inflater read what tests/bgzf_dynamic_model.encode writes from them, and its size next to zlib
level 1 and level 6 at the same 65280-byte cuts is what profiles/bam_pileup_deflate/README.txt records."""
import ctypes as C
import os
import re
import zlib

import pytest

from tests import bam_deflate_cases as zc
from tests import bam_pileup_model as bm
from tests import bam_text_model as tm
from tests import bgzf_deflate_cases as dc
from tests import bgzf_dynamic_model as dm
from tests import bgzf_fields_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_bam_pileup_bgzf_deflate", "bvc_bam_pileup_text_bgzf_deflate", "bvc_bam_pileup_deflate_fetch"]
CUTS_1 = (0x20, 0x0A)
# The committed model's output (cuts 1) against zlib on the same bytes cut at the same marks (dc.zlib_size), taken once on the CPU:
# {text: (fixed code or stored / level 1, the smallest of stored, fixed and dynamic / level 1, the same two / level 6)}
SIZE_AGAINST_ZLIB = {"batches of 100": (2.1861, 1.0553, 3.0094, 1.4527), "batches of 7": (2.9879, 1.3668, 4.3388, 1.9848),
                     "the catalogue": (4.2999, 1.6325, 5.6931, 2.1615)}
MARGIN = 1.05


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def seventh_header_declarations():
    """{name: (return type, [parameter text])} of include/bvc_bam_deflate.h, read as tests/test_binding_abi.py reads bvc.h."""
    txt = re.sub(r"/\*.*?\*/", " ", read("include", "bvc_bam_deflate.h"), flags=re.S)
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
    decls = seventh_header_declarations()
    assert list(decls) == bl.BAM_DEFLATE_EXPORTS == NAMES and len(bl.BAM_DEFLATE_PROTOTYPES) == len(decls) == 3
    # the closed lists stay as they were
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(tb.third_header_declarations()) == bl.BAM_EXPORTS == ["bvc_bam_pileup", "bvc_bam_pileup_bgzf"]
    others = (set(bl.PROTOTYPES) | set(bl.BGZF_CODES_PROTOTYPES) | set(bl.BAM_PROTOTYPES) | set(bl.POPMATRIX_PROTOTYPES) | set(bl.BAM_TEXT_PROTOTYPES) |
              set(bl.STORE_PROTOTYPES))
    assert not set(decls) & others
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.BAM_DEFLATE_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is ta.RETURNS[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    # both calls take bvc_bam_pileup_bgzf's arguments up to refseq_len, name for name, then the pieces and the outputs
    twin = tb.third_header_declarations()["bvc_bam_pileup_bgzf"][1]
    k = next(i for i, p in enumerate(twin) if p.endswith("refseq_len")) + 1
    tail = ["n_pieces", "piece_pos", "out", "out_cap", "out_needed", "out_off", "piece_bytes", "sample_status"]
    for name in NAMES[:2]:
        mine = decls[name][1]
        assert mine[:k] == twin[:k] and [p.split()[-1].lstrip("*") for p in mine[k:]] == tail, name
    assert decls[NAMES[0]][1] == decls[NAMES[1]][1]
    seventh = read("include", "bvc_bam_deflate.h")
    assert '#include "bvc_bam.h"' in seventh and '#include "bvc_bam_text.h"' in seventh and "bvc_bam_deflate.h" in read("include", "bvc.h")
    assert callable(getattr(bl.Context, "bam_pileup_bgzf_deflate", None)) and callable(getattr(bl.Context, "bam_pileup_deflate_fetch", None))
    assert "bvc_bam_deflate.hip" in b.SOURCES and any(d.endswith("bvc_bam_deflate.h") for d in b.DEPS)
    # no context: refused before anything of the device is touched
    n64 = C.c_int64(7)
    for name in NAMES[:2]:
        assert getattr(L, name)(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, 0, None, None, 0, C.byref(n64), None,
                                None, None) == -1
    assert L.bvc_bam_pileup_deflate_fetch(None, None, 0) == -1


def test_the_key_is_declared_beside_bgzf_parse():
    header = read("include", "bvc.h")
    assert '"bgzf_cuts"' in header and "BVC_BGZF_CUTS" in header and "a space or a newline" in header
    assert header.index('"bgzf_parse"       0 (default) / 1') < header.index('"bgzf_cuts"        0 (default) / 1') < header.index("int bvc_set_tuning(")
    context = read("basevarc_amd", "csrc", "bvc_context.hip")
    assert re.search(r'\{"bgzf_cuts", "BVC_BGZF_CUTS", 0, 1, 1, 0, &LaunchState::bgzf_cuts\}', context)
    # the rows the existing tests pin stay as they are, and the pair of bytes is carried into both kernels as an argument
    assert re.search(r'\{"bgzf_parse", "BVC_BGZF_PARSE", 0, 1, 1, 0, &LaunchState::bgzf_parse\}', context)
    dc.assert_the_mode_is_built_in_one_place()                               # all three keys, bgzf_cuts as the pair of bytes
    # the one block kernel takes the pair as its last argument, whatever it is instantiated with, and hands it to the field parse
    kernel = read("basevarc_amd", "csrc", "bgzf_block_kernel.h")
    assert kernel.count("uint32_t *__restrict__ match_rows, uint32_t delims)") == 1 and kernel.count("match, n, tid, delims);") == 1
    assert read("basevarc_amd", "csrc", "bgzf_dynamic_kernel.hip").count("bsize, match_rows, mode.delims);") == 1
    assert read("basevarc_amd", "csrc", "bgzf_deflate_kernel.hip").count("s.match_rows, mode.delims);") == 1
    device = read("basevarc_amd", "csrc", "bgzf_fields_device.h")
    assert "kBfDelimsTabColon = 0x09u | (0x3Au << 8)" in device and "kBfDelimsSpaceNewline = 0x20u | (0x0Au << 8)" in device
    assert "bgzf_cuts" in read("docs", "BGZF_FIELDS.md")
    assert fm.DELIMITERS == (0x09, 0x3A)


def test_the_host_program_reads_its_three_knobs_with_their_dependencies():
    knobs = read("basevarc_amd", "host", "knobs.h")
    assert re.search(r'device_pileup_deflate = num\("BVC_HOST_DEVICE_PILEUP_DEFLATE", 0\) != 0 && \(device_pileup \|\| device_pileup_text\);', knobs)
    assert re.search(r'device_pileup_deflate_codes = num\("BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES", 0\) != 0 && device_pileup_deflate;', knobs)
    assert re.search(r'device_pileup_deflate_tokens = num\("BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS", 0\) != 0 && device_pileup_deflate && device_pileup_text;',
                     knobs)
    main = read("basevarc_amd", "host", "main.cpp")
    assert 'knobs.device_pileup_deflate && opt::tmp_format != "raw"' in main                       # ignored with raw; the mem branch never asks
    assert "bvc_bam_pileup_text_bgzf_deflate : bvc_bam_pileup_bgzf_deflate" in main and "bvc_bam_pileup_deflate_fetch(" in main
    assert re.search(r'knobs\.device_pileup_deflate_codes && bvc_set_tuning\(dev\.ctx, "bgzf_codes", 1\)', main)
    assert re.search(r'bvc_set_tuning\(dev\.ctx, "bgzf_parse", 1\) != BVC_OK \|\| bvc_set_tuning\(dev\.ctx, "bgzf_cuts", 1\)', main)
    assert "fp.write_blocks(blocks.data() + out_off[" in main
    # the existing dispatch as it was
    a, b_, c = main.index("if (in_memory) {"), main.index('knobs.device_pileup && opt::tmp_format != "text"'), main.index(
        'knobs.device_pileup_text && opt::tmp_format == "text"')
    assert a < b_ < c
    tool = read("tools", "bam_pileup_bench.py")
    assert "--deflate" in tool and "--codes" in tool and "--tokens" in tool


def test_the_piece_layouts():
    for P in (0, 1, 2, 3, 7, 100):
        for name, pos in zc.layouts(P):
            assert pos[0] == 0 and pos[-1] == P and all(a <= b for a, b in zip(pos[:-1], pos[1:])), (P, name)
            assert ("empty" in name) <= any(a == b for a, b in zip(pos[:-1], pos[1:])), (P, name)
        for name, pos in zc.bad_layouts(max(P, 2)):
            assert pos[0] != 0 or pos[-1] != max(P, 2) or any(a > b for a, b in zip(pos[:-1], pos[1:])), name
    for text in (False, True):
        P, pos, sizes = zc.exact_pieces(text)
        unit = 1 if text else 4
        assert [(b - a) * unit for a, b in zip(pos[:-1], pos[1:])] == sizes and pos[-1] == P
        assert [dc.B - s for s in sizes[1:4]] == ([1, 0, -1] if text else [4, 0, -4]) and sizes[4] == 2 * dc.B


# ---- the model of "bgzf_cuts" = 1 on the text temp batches
@pytest.fixture(scope="module")
def texts():
    """{name: [pieces]}: the lines of every case of the text form's catalogue that has any, and of the 100 test BAMs (every 29th position) in
    one batch of 100 and in batches of 7."""
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    out = {"the catalogue": [e["text"] for e in (tm.expected(c) for c in tm.cases()) if e["text"]]}
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    pv = pv[::29]
    data = bam_data_bytes()
    for batch in (100, 7):
        pieces = []
        for at in range(0, len(data), batch):
            exp = bm.expected([(d[off:], True, refs.index(contig)) for d, off, refs in data[at:at + batch]], beg0, end0, mapq, pv, rg_s, refseq)
            assert exp["rc"] == 0
            pieces.append(tm.lines(exp["maps"], pv)[0])
        out[f"batches of {batch}"] = pieces
    assert len(out["batches of 7"]) == 15 and len(out["batches of 100"][0]) > 400000
    return out


@pytest.fixture(scope="module")
def parsed(texts):
    """{name: [(block, parse, symbols)]} under DELIMITERS = a space and a newline; the module's own value is put back."""
    mp = pytest.MonkeyPatch()
    mp.setattr(fm, "DELIMITERS", CUTS_1)
    try:
        out = {}
        for name, pieces in texts.items():
            rows = []
            for piece in pieces:
                for data in fm.blocks_of(piece):
                    ps = fm.parse(data)
                    rows.append((data, ps, fm.symbols(data, ps)))
            out[name] = rows
    finally:
        mp.undo()
    assert fm.DELIMITERS == (0x09, 0x3A)
    return out


def test_the_cuts_1_models_symbols_reproduce_every_piece_and_keep_the_rule(parsed, monkeypatch):
    monkeypatch.setattr(fm, "DELIMITERS", CUTS_1)
    runs = keyed = 0
    for name, rows in parsed.items():
        for data, ps, symbols in rows:
            assert dm.plain_bytes(symbols) == data, name
            n = len(data)
            assert ps["fields"] == fm.fields_of(data) and sum(length for _, length in ps["fields"]) == n
            cuts, length_of = {p for p, _ in ps["fields"]} | {n}, dict(ps["fields"])
            # a cut behind every space and newline, and nowhere else: ". " is a field of two bytes
            assert cuts == {0, n} | {p + 1 for p in range(n) if data[p] in CUTS_1}, name
            for p, (length, dist) in ps["match"].items():
                assert p in cuts and p + length in cuts and 4 <= length <= 258 and 1 <= dist <= min(p, 32768), (name, p, length, dist)
                assert data[p:p + length] == (data[p - dist:p] * (length // dist + 1))[:length], (name, p)
                if p not in ps["heads"]:
                    assert dist == length_of[p] and length % dist == 0, (name, p)
                    runs += data[p:p + 2] == b". " and dist == 2
                else:
                    keyed += data[p:p + length_of[p]].count(b",") == 4
    assert runs > 1000 and keyed > 1000, (runs, keyed)        # runs of ". " at the distance of one field; "b,m,q,r,s " tokens found by their key


def test_zlib_and_the_host_programs_inflater_read_both_encodings(parsed):
    from basevarc_amd import build as b
    _, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_fast_inflate.restype = C.c_long
    H.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    forms, checked = set(), 0
    for name, rows in parsed.items():
        for data, _, symbols in rows:
            m = dm.encode(symbols)
            forms.add(m["chosen"])
            for f in ("fixed", "dynamic"):
                d = zlib.decompressobj(-15)
                assert d.decompress(m[f]) == data and d.eof and d.unused_data == b"", (name, f)
                buf = C.create_string_buffer(len(data) + 1)
                assert H.bvchost_fast_inflate(m[f], len(m[f]), buf, len(data)) == len(data) and buf.raw[:len(data)] == data, (name, f)
            checked += 1
    assert checked > 40 and "dynamic" in forms


def test_size_on_the_text_temp_batches_against_zlib_level_1_and_6(texts, parsed):
    measured = {}
    for name, rows in parsed.items():
        fixed = dynamic = 0
        for data, _, symbols in rows:
            m = dm.encode(symbols)
            fixed += min(len(m["fixed"]), len(data) + 5) + 26
            dynamic += len(m["data"]) + 26
        total = sum(len(p) for p in texts[name])
        z1, z6 = sum(dc.zlib_size(p, 1) for p in texts[name]), sum(dc.zlib_size(p, 6) for p in texts[name])
        got = (fixed / z1, dynamic / z1, fixed / z6, dynamic / z6)
        print(f"{name}: text {total}, {len(rows)} blocks, fixed {fixed}, dynamic {dynamic}, zlib level 1 {z1}, level 6 {z6}: "
              f"fixed / level 1 {got[0]:.4f}, dynamic / level 1 {got[1]:.4f}, / level 6 {got[2]:.4f}, {got[3]:.4f}")
        measured[name] = got
    for name, got in measured.items():
        for g, want in zip(got, SIZE_AGAINST_ZLIB[name]):
            assert want / MARGIN <= g <= want * MARGIN, (name, got, SIZE_AGAINST_ZLIB[name])
