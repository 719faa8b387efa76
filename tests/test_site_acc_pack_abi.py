"""Packed accumulator rows (include/bvc_site_acc_pack.h) and the host program's counts files (docs/COUNTS_FILES.md) as far as a machine
without a GPU can see them: the entry points are declared, exported, in the binding's eleventh table and refuse null arguments; the ten
older lists are what they were; the new source is in the build's and the ISA report's lists; W against the formula; the model
(tests/acc_pack_model.py) by hand on three rows; the model's file written and read back; the host library's writer and reader against the
model's bytes, both ways; each refusal of the reader, truncation at every section boundary included; the knobs' parse rules; and
host/counts_file.cpp in a stand-alone program under the sanitizers (tests/cpp/counts_file_main.cpp)."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import acc_pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bvc_site_acc_row_words", "bvc_site_acc_pack", "bvc_site_acc_add_packed"]


def test_the_library_the_header_and_the_binding_know_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    from tests import test_bam_counts_abi as t8
    from tests import test_bam_counts_quals_abi as t10
    from tests import test_bam_group_depth_abi as t9
    from tests import test_binding_abi as ta
    b.build(force=b.needs_build())
    L = bl.bind(C.CDLL(bl.library_path(), mode=os.RTLD_LAZY))                 # (the symbol table only, no HIP runtime call)
    decls = t9.declarations_of("bvc_site_acc_pack.h")
    assert list(decls) == bl.SITE_ACC_PACK_EXPORTS == list(bl.SITE_ACC_PACK_PROTOTYPES) == NAMES
    # the ten older lists are what they were, and none of them holds a new name
    assert list(ta.header_declarations()) == bl.EXPORTS
    assert list(t8.eighth_header_declarations()) == bl.BAM_COUNTS_EXPORTS == t8.NAMES
    assert list(t9.declarations_of("bvc_bam_group_depth.h")) == bl.BAM_GROUP_DEPTH_EXPORTS == t9.NAMES
    assert list(t9.declarations_of("bvc_site_acc_quals.h")) == bl.SITE_ACC_QUALS_EXPORTS == t10.NAMES
    older = (bl.PROTOTYPES, bl.BGZF_CODES_PROTOTYPES, bl.BAM_PROTOTYPES, bl.POPMATRIX_PROTOTYPES, bl.BAM_TEXT_PROTOTYPES, bl.STORE_PROTOTYPES,
             bl.BAM_DEFLATE_PROTOTYPES, bl.BAM_COUNTS_PROTOTYPES, bl.BAM_GROUP_DEPTH_PROTOTYPES, bl.SITE_ACC_QUALS_PROTOTYPES)
    assert [len(t) for t in older[1:]] == [1, 2, 2, 2, 9, 3, 7, 3, 3], [len(t) for t in older]
    for table in older:
        assert not set(table) & set(decls)
    returns = dict(ta.RETURNS, void=None)
    for name, (ret, params) in decls.items():
        restype, argtypes = bl.SITE_ACC_PACK_PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is restype is returns[ret] and list(fn.argtypes) == argtypes and len(argtypes) == len(params), name
        for a, prm in zip(argtypes, params):
            if "*" in prm:
                assert ta.is_pointer(a), (name, prm, a)
            else:
                assert not ta.is_pointer(a) and a is ta.scalar_of(prm), (name, prm, a)
    assert decls["bvc_site_acc_pack"][1] == ["bvc_ctx *ctx", "const bvc_site_acc *acc", "int32_t t0", "int32_t n", "int64_t *row_start", "uint16_t *cell",
                                             "uint32_t *count", "int64_t entries_cap", "int64_t *n_entries", "uint32_t flags"]
    assert decls["bvc_site_acc_add_packed"][1] == ["bvc_ctx *ctx", "bvc_site_acc *acc", "int32_t t0", "int32_t n", "const int64_t *row_start",
                                                   "const uint16_t *cell", "const uint32_t *count", "int64_t n_entries", "uint32_t flags"]
    header = open(os.path.join(ROOT, "include", "bvc_site_acc_pack.h")).read()
    assert '#include "bvc_site_acc_quals.h"' in header
    assert re.search(r"#define\s+BVC_ACC_MORE\s+2\b", header) and bl.ACC_MORE == pm.ACC_MORE == 2
    for method in ("row_words", "pack", "add_packed"):
        assert callable(getattr(bl.SiteAcc, method, None)), method
    # no context, no accumulator: refused before anything of the device is touched, and nothing is written
    need, w = C.c_int64(-7), C.c_int32(-7)
    rs = np.full(4, 5, dtype=np.int64)
    assert L.bvc_site_acc_row_words(None, C.byref(w), None, None) == pm.ERR_ARG and w.value == -7
    assert L.bvc_site_acc_pack(None, None, 0, 3, C.c_void_p(rs.ctypes.data), None, None, 0, C.byref(need), 0) == pm.ERR_ARG
    assert L.bvc_site_acc_add_packed(None, None, 0, 3, C.c_void_p(rs.ctypes.data), None, None, 0, 0) == pm.ERR_ARG
    assert need.value == -7 and (rs == 5).all()


def test_the_new_source_is_built_and_in_the_isa_reports_list():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    src = "acc_pack_kernel.hip"
    assert src in b.SOURCES and src in isa_report.DEVICE_SOURCES and set(isa_report.DEVICE_SOURCES) <= set(b.SOURCES)
    assert any(d.endswith("bvc_site_acc_pack.h") for d in b.DEPS) and "counts_file.cpp" in b.HOST_SOURCES
    text = open(os.path.join(ROOT, "basevarc_amd", "csrc", src)).read()
    assert "__shared__" not in text and "mbcnt" in text and "__ballot" in text
    for kernel in ("acc_pack_kernel", "acc_pack_scan_kernel", "acc_add_packed_kernel", "acc_first_fault_kernel"):
        assert kernel in text, kernel


def test_the_row_words_of_all_three_kinds():
    assert pm.row_words() == 522 and pm.row_words(1, 5) == 542 and pm.row_words(33) == 33 * 512 + 10
    assert max(pm.row_words(s, g) for s in range(1, 34) for g in range(33)) == 33 * 512 + 10 + 128 == 17034 < 1 << 16
    for slots, groups, q in ((1, 0, None), (6, 0, None), (1, 5, None), (1, 32, None), (1, 0, 40), (1, 5, 40), (1, 32, 4)):
        n = 3
        counts = np.zeros((n, 4, q), dtype=np.uint32) if q else np.zeros((n, slots, 512), dtype=np.uint32)
        depth = np.zeros((n, groups, 4), dtype=np.uint32) if groups else None
        assert pm.logical_rows(counts, np.zeros((n, 12), dtype=np.uint32), depth).shape == (n, slots * 512 + 10 + 4 * groups)


def three_rows():
    """An empty row, a row with its first and last cell set, a narrow row whose set column is n_quals - 1: 40 columns, two groups."""
    counts, tally, depth = np.zeros((3, 4, 40), dtype=np.uint32), np.zeros((3, 12), dtype=np.uint32), np.zeros((3, 2, 4), dtype=np.uint32)
    counts[1, 0, 0] = 3
    depth[1, 1, 3] = 0xFFFFFFFF
    counts[2, 2, 39] = 0x10000
    tally[2, 9] = 1
    tally[2, 10:] = 77                             # (the pad words are no part of the row)
    return counts, tally, depth


def test_the_model_by_hand_on_three_rows():
    counts, tally, depth = three_rows()
    W = pm.row_words(1, 2)
    rows = pm.logical_rows(counts, tally, depth)
    assert rows.shape == (3, W) and W == 530
    rs, cell, count = pm.entries(rows)
    assert rs.tolist() == [0, 0, 2, 4] and rs.dtype == np.int64 and cell.dtype == np.uint16 and count.dtype == np.uint32
    assert cell.tolist() == [0, W - 1, 2 * 128 + 39, 512 + 9] and count.tolist() == [3, 0xFFFFFFFF, 0x10000, 1]
    assert pm.verdict(rs, cell, count, 3, W, 40) is None and pm.verdict(rs, cell, count, 3, W, 36) == (2, pm.FAULT_QUAL)
    # and back: into a narrow and into a wide accumulator of the same counts
    back = pm.add_entries(np.zeros_like(rows), rs, cell, count)
    c40, t, d = pm.dense(back, 1, 2, 40)
    assert (c40 == counts).all() and (t[:, :10] == tally[:, :10]).all() and not t[:, 10:].any() and (d == depth).all()
    wide = pm.dense(back, 1, 2)[0].reshape(3, 4, 128)
    assert (wide[:, :, :40] == counts).all() and not wide[:, :, 40:].any()
    with pytest.raises(ValueError):
        pm.dense(back, 1, 2, 36)
    # adds are modulo 2^32, and a count of 0 adds nothing
    twice = pm.add_entries(back.copy(), [0, 0, 2, 2], [W - 1, 5], [1, 0], 0)
    assert twice[1, W - 1] == 0 and twice[1, 5] == 0 and (np.delete(twice, W - 1, axis=1) == np.delete(back, W - 1, axis=1)).all()
    # the verdict's order: row_start first, then the row's first entry at fault
    assert pm.verdict([1, 0, 2, 4], cell, count, 3, W) == (0, pm.FAULT_ROW_START)
    assert pm.verdict([0, 0, 2, 5], cell, count, 3, W) == (2, pm.FAULT_ROW_START)
    assert pm.verdict([0, 3, 2, 4], cell, count, 3, W) == (0, pm.FAULT_ORDER) and pm.verdict([0, 2, 1, 4], cell, count, 3, W)[1] == pm.FAULT_ROW_START
    assert pm.verdict(rs, [0, W, 1, 2], count, 3, W) == (1, pm.FAULT_CELL) and pm.verdict(rs, [0, 0, 1, 2], count, 3, W) == (1, pm.FAULT_ORDER)
    assert pm.concat([pm.entries(rows[:1]), pm.entries(rows[1:2]), pm.entries(rows[2:])])[0].tolist() == rs.tolist()


def file_case():
    counts, tally, depth = three_rows()
    rows = pm.logical_rows(counts, tally, depth)
    positions = [5246595, 5246597, 5246600]
    meta = dict(chrom="chr11", rg_s=5246595, rg_e=5246600, n_positions=3, pos_hash=pm.positions_hash(positions), mapq=10, slots=1, depth_groups=2,
                n_quals=40, groups=["EAS", "EUR"], bams=[("data/a.bam", "S1"), ("data/b c.bam", "S2")])
    pieces = [(0, *pm.entries(rows[:2])), (2, *pm.entries(rows[2:]))]
    return meta, pieces, rows


def sections(data, meta, pieces):
    """The byte offsets at which a section of the file ends."""
    at = [8, 48]
    at.append(at[-1] + 4 + len(meta["chrom"]))
    at.append(at[-1] + 4)
    for g in meta["groups"]:
        at.append(at[-1] + 4 + len(g))
    at.append(at[-1] + 4)
    for path, sample in meta["bams"]:
        at += [at[-1] + 4 + len(path), at[-1] + 8 + len(path) + len(sample)]
    for t0, rs, cell, count in pieces:
        at += [at[-1] + 4, at[-1] + 20, at[-1] + 20 + len(rs) * 8, at[-1] + 20 + len(rs) * 8 + len(cell) * 2, at[-1] + 20 + len(rs) * 8 + len(cell) * 6]
    at += [at[-1] + 4, at[-1] + 8]
    assert at[-1] + 8 == len(data), (at, len(data))
    return at


def test_the_models_file_written_and_read_back():
    meta, pieces, rows = file_case()
    data = pm.file_bytes(meta, pieces)
    assert data[:8] == b"BVCCNTS\0" and struct.unpack_from("<I", data, 8)[0] == 1 and data[-16:-12] == b"END!"
    got_meta, got_pieces = pm.parse_file(data)
    assert got_meta == meta and len(got_pieces) == 2
    back = np.zeros_like(rows)
    for (t0, rs, cell, count), want in zip(got_pieces, pieces):
        assert t0 == want[0] and all(np.array_equal(a, b) for a, b in zip((rs, cell, count), want[1:]))
        pm.add_entries(back, rs, cell, count, t0)
    assert (back == rows).all()
    assert pm.fnv1a64(b"") == 0xCBF29CE484222325 and pm.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    for cut in sections(data, meta, pieces) + [len(data) - 1]:
        with pytest.raises(pm.FileError):
            pm.parse_file(data[:cut])
    with pytest.raises(pm.FileError):
        pm.parse_file(data + b"\0")


# ---- the host library ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    h = C.CDLL(b.build_host()[1])
    h.bvchost_counts_fnv1a64.restype = C.c_uint64
    h.bvchost_counts_fnv1a64.argtypes = [C.c_void_p, C.c_int64]
    h.bvchost_counts_file_write.restype = C.c_int32
    h.bvchost_counts_file_write.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_char_p, C.c_size_t]
    h.bvchost_counts_file_read.restype = C.c_int32
    h.bvchost_counts_file_read.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    h.bvchost_parse_counts_load.restype = C.c_int32
    h.bvchost_parse_counts_load.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    h.bvchost_parse_counts_save.restype = C.c_int32
    h.bvchost_parse_counts_save.argtypes = [C.c_char_p]
    return h


def meta_text(meta):
    return (meta["chrom"] + "\n" + "".join(f"G\t{g}\n" for g in meta["groups"]) + "".join(f"B\t{p}\t{s}\n" for p, s in meta["bams"])).encode()


def host_write(H, path, meta, pieces):
    ints = np.array([meta[k] for k in ("rg_s", "rg_e", "n_positions", "mapq", "slots", "depth_groups", "n_quals")], dtype=np.int32)
    t0 = np.array([p[0] for p in pieces], dtype=np.int32)
    n = np.array([len(p[1]) - 1 for p in pieces], dtype=np.int32)
    rs = np.concatenate([np.asarray(p[1], dtype=np.int64) for p in pieces] or [np.zeros(0, dtype=np.int64)])
    cell = np.concatenate([np.asarray(p[2], dtype=np.uint16) for p in pieces] + [np.zeros(1, dtype=np.uint16)])
    count = np.concatenate([np.asarray(p[3], dtype=np.uint32) for p in pieces] + [np.zeros(1, dtype=np.uint32)])
    err = C.create_string_buffer(512)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc = H.bvchost_counts_file_write(str(path).encode(), ptr(ints), meta["pos_hash"], meta_text(meta), len(pieces), ptr(t0), ptr(n), ptr(rs), ptr(cell), ptr(count),
                                     err, 512)
    return rc, err.value.decode()


def host_read(H, path):
    """(0, meta, pieces) or (1, the reader's line)."""
    ints, h, totals = np.zeros(7, dtype=np.int32), C.c_uint64(0), np.zeros(3, dtype=np.int64)
    text, err = C.create_string_buffer(1 << 16), C.create_string_buffer(512)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    caps = (0, 0, 0)
    for _ in range(2):
        t0, n = np.zeros(caps[0] + 1, dtype=np.int32), np.zeros(caps[0] + 1, dtype=np.int32)
        rs, cell, count = np.zeros(caps[1] + 1, dtype=np.int64), np.zeros(caps[2] + 1, dtype=np.uint16), np.zeros(caps[2] + 1, dtype=np.uint32)
        rc = H.bvchost_counts_file_read(str(path).encode(), ptr(ints), C.byref(h), text, 1 << 16, caps[0], ptr(t0), ptr(n), caps[1], ptr(rs), caps[2], ptr(cell),
                                        ptr(count), ptr(totals), err, 512)
        if rc == 1:
            return 1, err.value.decode()
        if rc == 0:
            break
        caps = tuple(int(x) for x in totals)
    assert rc == 0
    lines = text.value.decode().split("\n")
    meta = dict(zip(("rg_s", "rg_e", "n_positions", "mapq", "slots", "depth_groups", "n_quals"), (int(x) for x in ints)), pos_hash=h.value, chrom=lines[0],
                groups=[l[2:] for l in lines[1:] if l.startswith("G\t")], bams=[tuple(l[2:].split("\t")) for l in lines[1:] if l.startswith("B\t")])
    pieces, wa, ea = [], 0, 0
    for i in range(caps[0]):
        r = rs[wa:wa + n[i] + 1]
        pieces.append((int(t0[i]), r.copy(), cell[ea:ea + r[-1]].copy(), count[ea:ea + r[-1]].copy()))
        wa += n[i] + 1
        ea += int(r[-1])
    return 0, meta, pieces


def test_the_host_librarys_writer_and_reader_against_the_models_bytes(H, tmp_path):
    meta, pieces, rows = file_case()
    data = pm.file_bytes(meta, pieces)
    # the library writes the model's bytes ...
    rc, err = host_write(H, tmp_path / "host.counts", meta, pieces)
    assert rc == 0, err
    assert (tmp_path / "host.counts").read_bytes() == data
    # ... and reads the model's file
    (tmp_path / "model.counts").write_bytes(data)
    rc, got_meta, got_pieces = host_read(H, tmp_path / "model.counts")
    assert rc == 0 and got_meta == meta and len(got_pieces) == len(pieces)
    for got, want in zip(got_pieces, pieces):
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    # a file without a piece, a group or a BAM
    bare = dict(meta, groups=[], bams=[], depth_groups=0)
    rc, err = host_write(H, tmp_path / "bare.counts", bare, [])
    assert rc == 0 and (tmp_path / "bare.counts").read_bytes() == pm.file_bytes(bare, [])
    assert host_read(H, tmp_path / "bare.counts")[1:] == (bare, [])
    positions = np.array([5246595, 5246597, 5246600], dtype=np.int32)
    assert H.bvchost_counts_fnv1a64(C.c_void_p(positions.ctypes.data), 12) == meta["pos_hash"] == pm.fnv1a64(positions.tobytes())
    rc, err = host_write(H, tmp_path / "no_such_directory" / "x.counts", meta, pieces)
    assert rc == 1 and err.startswith(str(tmp_path / "no_such_directory" / "x.counts") + ": ") and "\n" not in err


def test_each_refusal_of_the_file_reader(H, tmp_path):
    meta, pieces, rows = file_case()
    data = pm.file_bytes(meta, pieces)
    path = tmp_path / "bad.counts"

    def refused(blob, *words):
        path.write_bytes(blob)
        rc, line = host_read(H, path)[:2]
        assert rc == 1 and line.startswith(str(path) + ": ") and "\n" not in line and all(w in line for w in words), (line, words)
        with pytest.raises(pm.FileError):
            pm.parse_file(blob)
    # truncation at every section boundary, one byte short of the end, and no bytes at all
    for cut in [0] + sections(data, meta, pieces) + [len(data) - 1]:
        refused(data[:cut], "truncated")
    refused(data + b"\0", "damaged", "end mark")
    refused(b"BVCCNTZ\0" + data[8:], "magic")
    refused(data[:8] + struct.pack("<I", 2) + data[12:], "version 2")
    refused(data[:12] + struct.pack("<I", 34) + data[16:], "damaged")
    s = sections(data, meta, pieces)
    first_piece = s[-13]                            # (two pieces of five sections each and the end mark's two)
    assert data[first_piece:first_piece + 4] == b"PIEC"
    refused(data[:first_piece] + b"PIEX" + data[first_piece + 4:], "damaged", "tag")
    refused(data[:first_piece + 4] + struct.pack("<i", 2) + data[first_piece + 8:], "damaged", "piece header")            # rows 2..3 of 3
    refused(data[:first_piece + 20] + struct.pack("<q", 1) + data[first_piece + 28:], "damaged", "row_start")             # row_start[0] = 1
    cell0 = first_piece + 20 + 3 * 8
    refused(data[:cell0] + struct.pack("<H", 530) + data[cell0 + 2:], "damaged", "cell")                                    # a cell of W
    refused(data[:-8] + struct.pack("<q", 5) + b"", "damaged", "end mark")                                                  # the total
    rc, line = host_read(H, tmp_path / "none.counts")[:2]
    assert rc == 1 and "can not open" in line


def test_the_knobs_parse_rules(H):
    out = C.create_string_buffer(256)
    assert H.bvchost_parse_counts_load(None, out, 256) == 0 and out.value == b""
    for text, want in ((b"a", ["a"]), (b"a:b", ["a", "b"]), (b"/x/y.counts:rel/z:w w", ["/x/y.counts", "rel/z", "w w"]), (b"a:a", ["a", "a"])):
        assert H.bvchost_parse_counts_load(text, out, 256) == len(want) and out.value.decode().split("\n")[:-1] == want, text
    for text in (b"", b":", b"a:", b":a", b"a::b", b"::"):
        assert H.bvchost_parse_counts_load(text, out, 256) == -1, text
    assert H.bvchost_parse_counts_save(None) == 0 and H.bvchost_parse_counts_save(b"") == -1
    assert H.bvchost_parse_counts_save(b"a") == 1 and H.bvchost_parse_counts_save(b"a:b") == 1


def counts_run(exe, tmp_path, fmt, env_add, sub):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BVC_HOST_COUNTS_")}
    env.update(env_add)
    out = tmp_path / sub
    out.mkdir()
    r = subprocess.run([exe, "basetype", "--tmp-format", fmt, "-i", str(out / "none.list"), "-r", "none.fa", "-s", "chr1:1-2", "-o", str(out / "o")],
                       capture_output=True, text=True, env=env)
    return r, os.listdir(str(out))


def test_a_bad_knob_value_is_refused_before_anything_is_opened_and_only_with_counts(tmp_path):
    from basevarc_amd import build as b
    exe = b.build_host()[0]
    for i, (knob, value, words) in enumerate((("BVC_HOST_COUNTS_LOAD", "", "FILE[:FILE...]"), ("BVC_HOST_COUNTS_LOAD", "a::b", "FILE[:FILE...]"),
                                              ("BVC_HOST_COUNTS_SAVE", "", "must name a file"))):
        r, left = counts_run(exe, tmp_path, "counts", {knob: value}, f"bad{i}")
        assert r.returncode == 1 and r.stderr.count("\n") == 1 and knob in r.stderr and words in r.stderr and left == [], (knob, value, r.stderr)
        # every other format ignores the knobs
        r, left = counts_run(exe, tmp_path, "bin", {knob: value}, f"other{i}")
        assert r.returncode == 1 and knob not in r.stderr, r.stderr
    # good values pass this check: the run ends on its next one (the input list is empty), naming no knob
    r, left = counts_run(exe, tmp_path, "counts", {"BVC_HOST_COUNTS_LOAD": "a:b", "BVC_HOST_COUNTS_SAVE": "c"}, "good")
    assert r.returncode == 1 and "BVC_HOST_COUNTS" not in r.stderr and left == [], r.stderr
    usage = subprocess.run([exe, "basetype", "--help"], capture_output=True, text=True)
    assert "BVC_HOST_COUNTS_SAVE=FILE" in usage.stdout + usage.stderr and "BVC_HOST_COUNTS_LOAD=FILE[:FILE...]" in usage.stdout + usage.stderr


def test_the_counts_file_under_the_address_sanitizer(tmp_path):
    """host/counts_file.cpp in a stand-alone program (tests/cpp/counts_file_main.cpp) built with -fsanitize=address,undefined: a round trip,
    the file cut at every length, changed bytes."""
    host_dir = os.path.join(ROOT, "basevarc_amd", "host")
    exe = str(tmp_path / "counts_file")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-I", host_dir, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "counts_file_main.cpp"), os.path.join(host_dir, "counts_file.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert re.search(r"\b3\d\d checks, 0 wrong", text), text[-400:]
