"""The device deflate encoder (bvc_bgzf_deflate; GPU).  Every piece of the catalogue of tests/bgzf_deflate_cases.py goes through the
block walker of tests/bgzf_blocks.py -- every header field, each block inflated on its own with zlib, CRC32, ISIZE, no empty block --
and is compared with the input, from host and from device pointers (device pieces start at odd addresses).  The blocks also go
through the project's own decoders.  The size of the output on three sample-column texts is held against zlib level 1 on the same
bytes cut at the same marks: not above it at coverage 0.10 and 0.01, not above 1.10 times it at coverage 1.0.  The ratios one run on
an MI355X gave are in profiles/vcf_deflate/README.txt."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import bgzf_blocks as bb
from tests import bgzf_deflate_cases as dc

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
GUARD = 0xA7


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def deflate_host(ctx, pieces, **kw):
    data = np.frombuffer(b"".join(pieces) + b"\0", dtype=np.uint8)
    ln = np.array([len(p) for p in pieces], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64) if len(pieces) else np.zeros(0, np.int64)
    return ctx.bgzf_deflate(data, off, ln, **kw)


def deflate_device(ctx, pieces):
    """The pieces at odd addresses of one device buffer, in another order than they are numbered, with bytes between them."""
    import torch
    from basevarc_amd.lib import bgzf_bound
    buf, off = bytearray(b"\xEE"), []
    order = list(range(len(pieces)))[::-1]
    where = {}
    for i in order:
        if len(buf) % 2 == 0:
            buf += b"\xEE"
        where[i] = len(buf)
        buf += pieces[i] + b"\xEE\xEE\xEE"
    off = np.array([where[i] for i in range(len(pieces))], dtype=np.int64)
    ln = np.array([len(p) for p in pieces], dtype=np.int64)
    need = sum(bgzf_bound(len(p)) for p in pieces)
    base = torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    assert base.data_ptr() % 2 == 0
    comp = torch.full((need + 3,), GUARD, dtype=torch.uint8, device="cuda")
    comp_t, off_t = ctx.bgzf_deflate_device(base, torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda(), comp[1:], comp_cap=need)
    ctx.synchronize()
    o = off_t.cpu().numpy()
    c = comp.cpu().numpy()
    assert c[0] == GUARD and (c[1 + int(o[-1]):] == GUARD).all(), "a byte outside the blocks changed"
    return c[1:], o


def check(pieces, names, comp, off):
    assert int(off[0]) == 0 and len(off) == len(pieces) + 1
    walked = []
    for i, p in enumerate(pieces):
        try:
            walked.append(bb.walk_piece(comp[int(off[i]):int(off[i + 1])].tobytes(), p))
        except AssertionError as e:
            raise AssertionError((names[i], len(p), e.args))
    return walked


@pytest.fixture(scope="module")
def catalogue(ctx):
    """(names, pieces, host call's (comp, off), its walked blocks): made once."""
    cases = dc.catalogue()
    names, pieces = [c[0] for c in cases], [c[1] for c in cases]
    comp, off = deflate_host(ctx, pieces)
    return names, pieces, (comp, off), check(pieces, names, comp, off)


def test_the_catalogue_from_host_pointers(catalogue):
    names, pieces, (comp, off), walked = catalogue
    by = dict(zip(names, walked))
    assert by["length 0"] == [] and len(by["length 1"]) == 1
    # what must be stored and what must be coded: random bytes cost 8 or 9 bits each; letters of four cost at most 8 bits each as
    # literals (n + 2 bytes of deflate data, less than the n + 5 of the stored form) and a match of 4 or more at most 25 bits, less than its literals
    assert bb.is_stored(by["65280 random bytes"][0][1]) and by["65280 random bytes"][0][2] == dc.B + 31
    four = by["65280 random letters of four"][0]
    assert not bb.is_stored(four[1]) and four[2] <= dc.B + 2 + 26
    assert not bb.is_stored(by["all 256 byte values"][0][1]) and not bb.is_stored(by["all 256 byte values in three orders"][0][1])
    for name, blocks in by.items():
        # runs and periodic text are found: every position has an earlier one in phase, so a block is matches of up to 258 bytes --
        # 2 bytes each at these distances -- behind a first period of literals; a symbol per 40 bytes is four times that
        if name.startswith("run of") or name.startswith("period"):
            n = sum(len(b[0]) for b in blocks)
            assert sum(b[2] for b in blocks) < 26 * len(blocks) + 40 + n // 40, name
        # the copies of tests/bgzf_deflate_cases.py are written as matches at the case's distance, of the case's length: the symbols the
        # encoder wrote, read back from the fixed code (tests/bgzf_blocks.py); 32769 is beyond what deflate can say, 3 below what is used
        if name.startswith("distance ") or name.startswith("match length "):
            assert len(blocks) == 1 and not bb.is_stored(blocks[0][1]), name
            pairs = [x for x in bb.fixed_symbols(blocks[0][1]) if isinstance(x, tuple)]
            assert all(4 <= ln <= 258 and 1 <= d <= 32768 for ln, d, _, _ in pairs), name
            k = int(name.split()[-1])
            if name.startswith("distance "):
                assert (k in [d for _, d, _, _ in pairs]) == (k <= 32768), (name, pairs)
            elif k >= 4:
                assert (min(k, 258), k + 1) in [(ln, d) for ln, d, _, _ in pairs], (name, pairs)
    # ... so every length symbol from 258 (length 4) on and every distance symbol has been written and read back
    seen = [x for blocks in walked for _, payload, _ in blocks if not bb.is_stored(payload) for x in bb.fixed_symbols(payload) if isinstance(x, tuple)]
    assert {x[2] for x in seen} == set(range(258, 286)) and {x[3] for x in seen} == set(range(30))


def test_the_catalogue_from_device_pointers_at_odd_addresses(ctx, catalogue):
    names, pieces, (comp, off), _ = catalogue
    dcomp, doff = deflate_device(ctx, pieces)
    check(pieces, names, dcomp, doff)
    # the output is a function of the bytes: wherever they lie and whichever form of the call
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()


def test_more_blocks_than_workgroups_and_one_byte_pieces(ctx):
    pieces = dc.stream_pieces()
    assert sum((len(p) + dc.B - 1) // dc.B for p in pieces) > 2 * dc.GRID and sum(1 for p in pieces if len(p) == 1) > 200
    names = [f"piece {i}" for i in range(len(pieces))]
    comp, off = deflate_host(ctx, pieces)
    check(pieces, names, comp, off)
    assert int(off[301]) == int(off[300]) == int(off[302])        # empty pieces: empty ranges, no block
    # two calls on the same input give the same bytes; so does the device form
    comp2, off2 = deflate_host(ctx, pieces)
    assert (off2 == off).all() and (comp2[:int(off[-1])] == comp[:int(off[-1])]).all()
    dcomp, doff = deflate_device(ctx, pieces)
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()


def test_a_guard_byte_behind_the_blocks_survives(ctx):
    from basevarc_amd.lib import bgzf_bound
    pieces = [dc.periodic(b"./.\t", 70000), b"x", dc.periodic(b"0/.:A:+:0.999369\t", 3000)]
    need = sum(bgzf_bound(len(p)) for p in pieces)
    comp = np.full(need + 64, GUARD, dtype=np.uint8)
    comp, off = deflate_host(ctx, pieces, comp=comp, comp_cap=need)
    check(pieces, ["a", "b", "c"], comp, off)
    assert (comp[int(off[-1]):] == GUARD).all()


def test_refusals_leave_the_context_usable(ctx):
    from basevarc_amd.lib import BvcError, bgzf_bound
    import torch
    L, h = ctx._L, ctx._h
    data = np.frombuffer(dc.periodic(b"./.\t", 1000), dtype=np.uint8)
    off, ln = np.array([0, 500], dtype=np.int64), np.array([500, 500], dtype=np.int64)
    comp, coff = np.zeros(4096, dtype=np.uint8), np.zeros(3, dtype=np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def call(n, d, o, l, c, cap, co, flags=0):
        return L.bvc_bgzf_deflate(h, n, d, o, l, c, cap, co, flags)
    assert call(-1, p(data), p(off), p(ln), p(comp), 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), p(off), p(ln), p(comp), -1, p(coff)) == BVC_ERR_ARG
    assert call(2, None, p(off), p(ln), p(comp), 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), None, p(ln), p(comp), 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), p(off), None, p(comp), 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), p(off), p(ln), None, 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), p(off), p(ln), p(comp), 4096, None) == BVC_ERR_ARG
    neg = np.array([500, -1], dtype=np.int64)
    assert call(2, p(data), p(off), p(neg), p(comp), 4096, p(coff)) == BVC_ERR_ARG
    assert call(2, p(data), p(neg), p(ln), p(comp), 4096, p(coff)) == BVC_ERR_ARG
    need = 2 * bgzf_bound(500)
    comp[:] = GUARD
    assert call(2, p(data), p(off), p(ln), p(comp), need - 1, p(coff)) == BVC_ERR_ARG
    assert str(need) in L.bvc_last_error(h).decode() and (comp == GUARD).all()
    # the device form: the same refusals once the lengths are known
    d_t, o_t, l_t = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda()
    c_t = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    with pytest.raises(BvcError) as e:
        ctx.bgzf_deflate_device(d_t, o_t, l_t, c_t, comp_cap=need - 1)
    assert e.value.status == BVC_ERR_ARG and str(need) in str(e.value)
    with pytest.raises(BvcError):
        ctx.bgzf_deflate_device(d_t, o_t, torch.from_numpy(neg).cuda(), c_t)
    ctx.synchronize()
    assert bool((c_t == GUARD).all())
    # nothing to do is no error, and the context works afterwards
    assert call(0, None, None, None, None, 0, p(coff)) == 0 and int(coff[0]) == 0
    assert call(2, None, p(off), p(np.zeros(2, np.int64)), None, 0, p(coff)) == 0 and list(coff) == [0, 0, 0]
    assert call(2, p(data), p(off), p(ln), p(comp), need, p(coff)) == 0
    check([data[:500].tobytes(), data[500:].tobytes()], ["a", "b"], comp, coff)


def test_the_projects_own_decoders_read_the_blocks(ctx, catalogue):
    """Context.inflate_blocks (inflate_kernel.hip, CRC compared) and bvchost_fast_inflate (host/inflate.cpp) on the catalogue's blocks."""
    from basevarc_amd import build as b
    names, pieces, (comp, off), walked = catalogue
    _, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_fast_inflate.restype = C.c_long
    H.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    payloads, table, want = bytearray(), [], []
    for name, blocks in zip(names, walked):
        for data, payload, _ in blocks:
            out = C.create_string_buffer(len(data) + 1)
            assert H.bvchost_fast_inflate(bytes(payload), len(payload), out, len(data)) == len(data) and out.raw[:len(data)] == data, name
            table.append((len(payloads), len(payload), len(data), bb.zlib.crc32(data) & 0xFFFFFFFF))
            payloads += payload + b"\xA5" * 5
            want.append(data)
    got, status = ctx.inflate_blocks(bytes(payloads), table)
    assert [int(s) for s in status] == [0] * len(table)
    assert got == want


def test_size_against_zlib_level_1_on_sample_column_texts(ctx):
    figures = []
    for coverage, seed, bound in dc.SIZE_TEXTS:
        text = dc.sample_text(100000, coverage, seed)
        comp, off = deflate_host(ctx, [text])
        bb.walk_piece(comp[:int(off[1])].tobytes(), text)
        z1, z6 = dc.zlib_size(text, 1), dc.zlib_size(text, 6)
        figures.append((coverage, len(text), int(off[1]), z1, z6, bound))
        print(f"coverage {coverage}: text {len(text)}, device {int(off[1])}, zlib level 1 {z1}, level 6 {z6}: "
              f"device / level 1 {int(off[1]) / z1:.3f}, / level 6 {int(off[1]) / z6:.3f}")
    for coverage, n, dev, z1, z6, bound in figures:
        assert dev <= bound * z1, (coverage, dev, z1, dev / z1)
