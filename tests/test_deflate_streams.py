"""CPU tests of the hand-built deflate streams (tests/deflate_streams.py) and of host/inflate.cpp on them.

zlib's compressor emits a narrow slice of RFC 1951; the catalogue holds what it never emits: 15-bit codes of every kind, one-code
and empty distance sets, every header run count, matches on every edge of the device kernel's copy paths, objects across the
reader window's end, and the refusals.  Here: (1) the catalogue is right -- zlib, the reference, inflates every stream meant to be
valid to exactly its data and refuses every other, and so does the model (tests/deflate_model.py); (2) the census: the valid
streams reach every path class of the device kernel at least four times, which is what keeps tests/test_gpu_inflate_streams.py
from passing without having met an edge; (3) host/inflate.cpp over the whole catalogue and every truncation, in-process with guard
bytes and in a stand-alone program built with -fsanitize=address,undefined.
"""
import collections
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import pytest

from tests import deflate_model as M
from tests import deflate_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLERS = (b"\x00", b"\xFF")
ERR_NAMES = {S.ERR_TYPE: "type", S.ERR_STORED: "stored", S.ERR_HEADER: "header", S.ERR_CODES: "codes", S.ERR_DISTANCE: "distance"}


def zlib_inflates(comp, isize):
    """The data if zlib takes `comp` for one complete raw deflate stream of isize bytes, else None."""
    z = zlib.decompressobj(-15)
    try:
        data = z.decompress(comp)
    except zlib.error:
        return None
    return data if z.eof and z.unused_data == b"" and len(data) == isize else None


@pytest.fixture(scope="module")
def modelled():
    return {s.name: M.inflate(s.comp, s.isize) for s in S.catalogue()}


def test_census_constants_are_the_kernels():
    """The five constants the census is computed from, against the text of csrc/inflate_kernel.hip."""
    text = open(os.path.join(ROOT, "basevarc_amd", "csrc", "inflate_kernel.hip"), encoding="utf-8").read()
    assert re.search(r"#define BVC_INFLATE_WINDOW %d\b" % M.RING, text)
    assert re.search(r"kLitBits = %d, kDistBits = %d\b" % (M.LIT_BITS, M.DIST_BITS), text)
    # fast_symbols: the batch's last lane (the batch used up; a pair's last piece) and the longest fast copy
    assert len(re.findall(r"s_cmp_gt_u32 %%\[off\], %d\\n" % M.FAST_COPY, text)) == 1
    assert len(re.findall(r"s_cmp_gt_u32 %%\[p\], %d\\n" % M.FAST_COPY, text)) == 1
    assert len(re.findall(r"s_cmp_gt_u32 %%\[len\], %d\\n" % M.FAST_COPY, text)) == 1
    assert not re.findall(r"s_cmp_gt_u32 %\[(?:off|p|len)\], (?!" + str(M.FAST_COPY) + r"\\n)", text)
    assert "if (p3 > %du)" % M.FAST_COPY in text and "if (p2 <= %du)" % M.FAST_COPY in text
    assert re.search(r"\[lim\] \"s\"\(kWinBytes - 64u\)", text) and "dist + len + 64u <= kWinBytes" in text
    assert 's_cmp_ge_u32 %%[bp], %d\\n' % M.READER_WINDOW in text and "while (bp >= %du)" % M.READER_WINDOW in text


def test_catalogue_is_what_zlib_and_the_model_say(modelled):
    """zlib is the reference: a stream meant to be valid inflates to exactly its data (eof, nothing unused), one meant to be refused
    does not; the model agrees with both.  Where zlib and the intent disagree the catalogue is wrong."""
    assert len(S.valid()) > 400 and len(S.refused()) > 60
    for s in S.catalogue():
        got = zlib_inflates(s.comp, s.isize)
        m = modelled[s.name]
        if s.reason is None:
            assert got == s.data and len(s.data) == s.isize <= 65536, s.name
            assert m.error is None and m.data == s.data, (s.name, m.error)
        else:
            assert got is None, s.name + ": zlib inflates a stream meant to be refused (" + s.reason + ")"
            assert m.error is not None, s.name
            if s.err is not None:                                  # the device's code asked for is the model's reason too
                assert m.error.startswith(ERR_NAMES[s.err]), (s.name, s.err, m.error)
    names = {s.name for s in S.catalogue()}
    assert set(S.TRUNCATED) <= names
    for name, prefix, isize in S.truncations():
        assert zlib_inflates(prefix, isize) is None, name
        assert M.inflate(prefix, isize).error is not None, name


def test_census_every_path_class_is_reached(modelled):
    """Every path class of the device kernel at least four times over the valid streams; the classes of the reader window at every
    alignment of the payload.  A condition, not a measurement: a catalogue that loses an edge fails here."""
    census = collections.Counter()
    for s in S.valid():
        census.update(modelled[s.name].census)
    low = {c: census[c] for c in M.CENSUS_CLASSES if census[c] < 4}
    for c in M.CENSUS_PER_LEAD:
        per_lead = [census[c % lead] for lead in range(4)]
        if min(per_lead) < 1 or sum(per_lead) < 4:
            low[c] = per_lead
    assert not low, low
    print("\n".join("%8d  %s" % (census[c], c) for c in sorted(census)))


@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    _, lib = b.build_host()
    L = C.CDLL(lib)
    L.bvchost_fast_inflate.restype = C.c_long
    L.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return L


def host_inflate(H, comp, cap, behind=b""):
    """bvchost_fast_inflate on `comp` (followed in memory by `behind`, which is not part of it) with `cap` bytes of room and the guard
    bytes of tests/test_host.py behind them."""
    src = C.create_string_buffer(comp + behind, len(comp) + len(behind) + 1)
    out = C.create_string_buffer(max(cap, 1) + 64)
    guard = b"\xA5" * 64
    out[cap:cap + 64] = guard
    r = H.bvchost_fast_inflate(src, len(comp), out, cap)
    assert out.raw[cap:cap + 64] == guard, "wrote past its output buffer"
    return r, out.raw[:max(r, 0)]


def test_host_decoder_on_the_catalogue(H):
    """host/inflate.cpp: a valid stream inflates to exactly its data, a stream to be refused returns anything but ISIZE, a truncated one
    too whatever lies behind it in memory, and nothing is written beyond the room given."""
    wrong = []
    for s in S.catalogue():
        r, out = host_inflate(H, s.comp, s.isize)
        if s.reason is None:
            if r != s.isize or out != s.data:
                wrong.append((s.name, r))
            if s.isize > 0 and host_inflate(H, s.comp, s.isize - 1)[0] == s.isize:
                wrong.append((s.name, "too little room"))
        elif r == s.isize:
            wrong.append((s.name, r, s.reason))
    for name, prefix, isize in S.truncations():
        for filler in FILLERS:
            if host_inflate(H, prefix, isize, filler * 16)[0] == isize:
                wrong.append((name, filler))
    assert not wrong, wrong[:20]


def test_host_decoder_under_the_address_sanitizer(tmp_path):
    """The same in a stand-alone program (tests/cpp/inflate_streams_main.cpp + host/inflate.cpp) built with
    -fsanitize=address,undefined: every stream in a heap block of exactly its size, the output in one of exactly ISIZE bytes."""
    records = [(s.comp, s.isize, s.data if s.reason is None else None) for s in S.catalogue()]
    records += [(prefix, isize, None) for _, prefix, isize in S.truncations()]
    records += [(s.comp, s.isize - 1, None) for s in S.valid() if s.isize > 0]
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for comp, cap, data in records:
            f.write(struct.pack("<III", len(comp), cap, 1 if data is not None else 0) + comp + (data or b""))
    exe = str(tmp_path / "inflate_streams")
    host = os.path.join(ROOT, "basevarc_amd", "host")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-fno-omit-frame-pointer", "-I", host, os.path.join(ROOT, "tests", "cpp", "inflate_streams_main.cpp"),
                           os.path.join(host, "inflate.cpp"), "-o", exe])
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert "%d streams, 0 wrong" % len(records) in text
