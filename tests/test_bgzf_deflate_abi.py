"""The device deflate encoder as far as a machine without a GPU can see it: the library exports the two entry points, include/bvc.h
declares them and the binding's table names them, the header's inline functions agree with the binding's, the kernels are
built from their own source under the rules of every kernel, and the host program's writer takes finished blocks between its own
(BgzfWriter::write_blocks through bvchost_bgzf_splice) in order, foreground and with deflating threads."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import bgzf_blocks as bb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bvc_bgzf_deflate", "bvc_pileup_sample_bgzf")


def test_the_libraries_export_the_entry_points():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    L = C.CDLL(bl.library_path(), mode=os.RTLD_LAZY)                 # (the symbol table only, no HIP runtime call)
    for s in SYMBOLS:
        assert hasattr(L, s), s
    _, hostlib = b.build_host()
    assert hasattr(C.CDLL(hostlib), "bvchost_bgzf_splice")


def test_the_header_declares_them_and_the_binding_requires_them():
    from basevarc_amd import lib as bl
    from tests import test_binding_abi as ta
    header = open(os.path.join(ROOT, "include", "bvc.h")).read()
    assert re.search(r"#define BVC_BGZF_BLOCK_INPUT 65280\b", header)
    assert re.search(r"static inline int64_t bvc_bgzf_blocks\(int64_t len\)", header)
    assert re.search(r"static inline int64_t bvc_bgzf_bound\(int64_t len\)", header)
    # declared in this order, and rows of the binding's one table (tests/test_binding_abi.py compares every row with its declaration)
    assert [name for name in ta.header_declarations() if name in SYMBOLS] == list(SYMBOLS)
    assert [name for name in bl.EXPORTS if name in SYMBOLS] == list(SYMBOLS)
    for m in ("bgzf_deflate", "bgzf_deflate_device", "pileup_sample_bgzf"):
        assert callable(getattr(bl.Context, m, None)), m


def test_the_inline_functions_and_the_constants_are_the_ones_the_tests_use(tmp_path):
    from basevarc_amd import lib as bl
    from tests import bgzf_deflate_cases as dc
    src = tmp_path / "bound.c"
    src.write_text('#include "bvc.h"\nlong long blocks(long long n) { return bvc_bgzf_blocks(n); }\n'
                   'long long bound(long long n) { return bvc_bgzf_bound(n); }\nlong long block_input(void) { return BVC_BGZF_BLOCK_INPUT; }\n')
    so = tmp_path / "bound.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", str(so), str(src)])
    S = C.CDLL(str(so))
    for f in (S.blocks, S.bound, S.block_input):
        f.restype = C.c_longlong
    S.blocks.argtypes = S.bound.argtypes = [C.c_longlong]
    B = 65280
    assert S.block_input() == B == bl.BGZF_BLOCK_INPUT == bb.BLOCK_INPUT == dc.B
    for n, blocks in ((0, 0), (1, 1), (B - 1, 1), (B, 1), (B + 1, 2), (2 * B, 2), (2 ** 40, (2 ** 40 + B - 1) // B), (-5, 0)):
        assert S.blocks(n) == bl.bgzf_blocks(n) == blocks, n
        assert S.bound(n) == bl.bgzf_bound(n) == (n + 31 * blocks if n > 0 else 0), n
    internal = open(os.path.join(ROOT, "basevarc_amd", "csrc", "bvc_internal.h")).read()
    assert int(re.search(r"constexpr int kBgzfDeflateGrid = (\d+);", internal).group(1)) == bl.BGZF_DEFLATE_GRID == dc.GRID


def test_the_kernels_are_built_from_their_own_source_without_private_memory_or_flat_addressing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "bgzf_deflate_kernel.hip" in b.SOURCES and "bvc_bgzf.hip" in b.SOURCES
    assert "bgzf_deflate_kernel.hip" in isa_report.DEVICE_SOURCES
    rows = {k["pretty"].split("::")[-1]: k for k in isa_report.kernels_of(isa_report.assembly("bgzf_deflate_kernel.hip"))}
    assert set(rows) == {"bgzf_plan_kernel", "bgzf_block_kernel<false, false>", "bgzf_crc_kernel", "bgzf_scan_kernel", "bgzf_pack_kernel"}, sorted(rows)
    for name, k in rows.items():
        assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["mfma"] == 0, (name, k)
        assert k["vgprs"] <= 128, (name, k["vgprs"])                          # sixteen wavefronts a CU: 128 registers a lane at the most
    assert rows["bgzf_block_kernel<false, false>"]["lds"] == 147600           # the block and its tables: one workgroup a CU
    # without the flag of the other three instantiations' sources (tests/test_bgzf_dynamic_abi.py, tests/test_bgzf_fields_abi.py)
    assert "bgzf_deflate_kernel.hip" not in b.PER_SOURCE_FLAGS
    # the CRC's slice-and-combine code is shared with the inflate kernels, not copied
    assert "crc_multmodp" not in open(os.path.join(ROOT, "basevarc_amd", "csrc", "bgzf_deflate_kernel.hip")).read().replace("crc32_device.h", "")
    assert "crc_multmodp" not in open(os.path.join(ROOT, "basevarc_amd", "csrc", "inflate_kernel.hip")).read()


# ---- BgzfWriter::write_blocks ------------------------------------------------------------------------------------------------
def ready_blocks(data, level, cut):
    """`data` as finished BGZF blocks of `cut` input bytes, made with zlib."""
    out = bytearray()
    for at in range(0, len(data), cut):
        part = data[at:at + cut]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = c.compress(part) + c.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", len(payload) + 25)
        out += payload + struct.pack("<II", zlib.crc32(part) & 0xFFFFFFFF, len(part))
    return bytes(out)


@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    _, lib = b.build_host()
    L = C.CDLL(lib)
    L.bvchost_bgzf_splice.restype = C.c_int
    L.bvchost_bgzf_splice.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.c_int, C.c_int]
    return L


def splice(H, path, parts, background):
    """parts: [(kind, plain bytes)]; kind 1 goes in as finished blocks.  Returns the file."""
    raw = [ready_blocks(d, 1 + i % 6, (65280, 700, 30000)[i % 3]) if kind else d for i, (kind, d) in enumerate(parts)]
    n = len(parts)
    bufs = [C.create_string_buffer(r, max(1, len(r))) for r in raw]
    ptrs = (C.c_char_p * n)(*[C.cast(b, C.c_char_p) for b in bufs])
    lens = (C.c_int64 * n)(*[len(r) for r in raw])
    kinds = (C.c_int32 * n)(*[k for k, _ in parts])
    assert H.bvchost_bgzf_splice(str(path).encode(), ptrs, lens, kinds, n, 6, background) == 1
    return open(path, "rb").read()


@pytest.mark.parametrize("background", [0, 1, 3])
def test_ready_blocks_between_text_keep_their_place(H, tmp_path, background):
    rng = np.random.default_rng(7)

    def text(n):
        return bytes(rng.choice(np.frombuffer(b"./.\t0:ACGT+-19", dtype=np.uint8), n))
    # text, blocks (several per part), text, blocks, blocks, empty text, text; a long text in front of ready blocks keeps the workers busy
    parts = [(0, text(1000)), (1, text(150000)), (0, text(200000)), (1, text(5000)), (1, text(70000)), (0, b""), (0, text(77))]
    raw = splice(H, tmp_path / "s.gz", parts, background)
    blocks = bb.walk_file(raw)
    assert gzip.decompress(raw) == b"".join(d for _, d in parts)
    # the text in front of a ready part ends its block there: no block holds bytes of both
    ends, at = set(), 0
    for data, _, _ in blocks:
        at += len(data)
        ends.add(at)
    at = 0
    for _, d in parts:
        at += len(d)
        assert at in ends, at
    # only ready parts, and none at all
    raw = splice(H, tmp_path / "r.gz", [(1, text(3)), (1, text(65281))], background)
    assert len(bb.walk_file(raw)) == 1 + 94 and len(gzip.decompress(raw)) == 65284
    raw = splice(H, tmp_path / "e.gz", [(1, b""), (0, b"")], background)
    assert raw == bb.EOF_MARKER
