"""The device deflate encoder with tuning key "bgzf_codes" at 1 (bgzf_dynamic_kernel.hip; GPU): each block the smallest of stored, fixed
and a Huffman code of its own.  The catalogue of tests/bgzf_deflate_cases.py and the pieces of tests/bgzf_dynamic_cases.py go through the
block walker, from host and from device pointers; every block is held against the same block at key 0 (never larger, the same parse)
and, byte for byte, against the plain Python model of the rule (tests/bgzf_dynamic_model.py, docs/BGZF_DYNAMIC.md), and is read by the
project's own decoders.  bvc_bgzf_code_lengths runs the builder on counts no small text gives.  The bytes at key 0 are held against
digests taken on the commit before the key existed (tests/golden/bgzf_fixed_catalogue.json)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import bgzf_blocks as bb
from tests import bgzf_deflate_cases as dc
from tests import bgzf_dynamic_cases as yc
from tests import bgzf_dynamic_model as dm
from tests.test_gpu_bgzf_deflate import GUARD, check, deflate_device, deflate_host

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
FORMS = {0: "stored", 1: "fixed", 2: "dynamic"}
RANDOM = ("65280 random bytes", "65280 random letters of four")          # os.urandom: other bytes on every run


def form(payload):
    return FORMS[(payload[0] >> 1) & 3]


def symbols_of(payload):
    """The symbols of a coded block as 4-tuples / ints (None for a stored one) and, for a dynamic one, the header's symbols."""
    if form(payload) == "stored":
        return None, []
    if form(payload) == "fixed":
        return bb.fixed_symbols(payload), []
    blocks, end = dm.read_blocks(payload)
    assert len(blocks) == 1 and blocks[0]["final"] == 1 and (end + 7) // 8 == len(payload)
    return blocks[0]["symbols"], blocks[0]["header"]


@pytest.fixture(scope="module")
def ctx1():
    from basevarc_amd import Context
    c = Context(0)
    c.set_tuning("bgzf_codes", 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx0():
    from basevarc_amd import Context
    c = Context(0)
    c.set_tuning("bgzf_codes", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def catalogue(ctx0, ctx1):
    """names, pieces, the forms the new pieces must take, and per key the host call's (comp, off) and its walked blocks: made once."""
    cases = [(n, p, None) for n, p in dc.catalogue()] + yc.catalogue()
    names, pieces, forms = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    assert len(set(names)) == len(names)
    out = {}
    for key, ctx in ((0, ctx0), (1, ctx1)):
        comp, off = deflate_host(ctx, pieces)
        out[key] = ((comp, off), check(pieces, names, comp, off))                 # (check 1: every piece walks and equals its input)
    return names, pieces, forms, out


def test_the_key_takes_0_and_1_only(ctx1):
    from basevarc_amd.lib import BvcError
    with pytest.raises(BvcError) as e:
        ctx1.set_tuning("bgzf_codes", 2)
    assert e.value.status == BVC_ERR_ARG
    ctx1.set_tuning("bgzf_codes", 0)
    ctx1.set_tuning("bgzf_codes", 1)


def test_the_catalogue_block_by_block_against_key_0_and_the_model(catalogue):
    names, pieces, forms, out = catalogue
    seen, census = set(), set()
    for name, want_form, blocks0, blocks1 in zip(names, forms, out[0][1], out[1][1]):
        assert len(blocks0) == len(blocks1), name
        if want_form is not None:
            assert form(blocks1[0][1]) == want_form, (name, form(blocks1[0][1]), len(blocks0[0][1]), len(blocks1[0][1]))
        for (data, p0, size0), (_, p1, size1) in zip(blocks0, blocks1):
            seen.add(form(p1))
            assert form(p0) != "dynamic"
            # check 3: never larger; equal size = the same block; a dynamic block is strictly smaller
            assert size1 <= size0, (name, size0, size1)
            if size1 == size0:
                assert p1 == p0, name
            assert (form(p1) == "dynamic") == (size1 < size0), (name, form(p1), size0, size1)
            # check 4: the parse is the one key 0 computes
            sym0, _ = symbols_of(p0)
            sym1, header = symbols_of(p1)
            census |= set(header)
            if sym0 is not None and sym1 is not None:
                assert sym1 == sym0, name
            # check 5: the whole deflate data is the model's encoding of those symbols, the choice among the three forms included
            symbols = sym0 if sym0 is not None else sym1
            if symbols is None:
                assert p1 == bytes([1, len(data) & 255, len(data) >> 8, ~len(data) & 255, (~len(data) >> 8) & 255]) + data, name
                continue
            assert dm.plain_bytes(symbols) == data, name
            m = dm.encode(symbols)
            assert m["chosen"] == form(p1), (name, m["chosen"], form(p1), {f: len(m[f]) for f in FORMS.values()}, len(p1))
            assert m["data"] == p1, (name, form(p1), next(i for i in range(len(p1)) if m["data"][i:i + 1] != p1[i:i + 1]))
            assert m["fixed" if len(m["fixed"]) <= len(data) + 5 else "stored"] == p0, name
    by0, by1 = dict(zip(names, out[0][1])), dict(zip(names, out[1][1]))
    # stored at key 0 (8 or 9 bits a byte in the fixed code), dynamic at key 1 (7.64 bits a byte)
    assert form(by0["65280 random bytes over 200 values"][0][1]) == "stored"
    assert form(by1["65280 random bytes"][0][1]) == "stored" and form(by1["length 1"][0][1]) == "fixed"
    # no distance used (both codes of the padded distance alphabet are written), one used distance, HLIT at its ends
    for name, n_dist, hlit in (("literals 0..143 only", 0, 257), ("literals 0..255 only", 0, 257), ("one match among literals", 1, None),
                               ("every length and distance symbol in one block", 30, 286)):
        blk = dm.read_blocks(by1[name][0][1])[0][0]
        used = {x[3] for x in blk["symbols"] if isinstance(x, tuple)}
        assert len(used) == n_dist and (hlit is None or blk["hlit"] == hlit), (name, sorted(used), blk["hlit"])
        if n_dist < 2:
            assert sum(1 for ln in blk["dl"] if ln) == 2 and dm.kraft(blk["dl"]) == 1 << 15, (name, blk["dl"])
    blk = dm.read_blocks(by1["every length and distance symbol in one block"][0][1])[0][0]
    pairs = [x for x in blk["symbols"] if isinstance(x, tuple)]
    assert {x[2] for x in pairs} == set(range(258, 286)) and {x[3] for x in pairs} == set(range(30))      # (257 = length 3: never used)
    assert seen == {"stored", "fixed", "dynamic"}
    assert census == set(range(19)), sorted(set(range(19)) - census)


def test_device_pointers_and_a_second_call_give_the_same_bytes(ctx1, catalogue):
    names, pieces, _, out = catalogue
    comp, off = out[1][0]
    dcomp, doff = deflate_device(ctx1, pieces)
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()
    comp2, off2 = deflate_host(ctx1, pieces)
    assert (off2 == off).all() and (comp2[:int(off[-1])] == comp[:int(off[-1])]).all()


def test_the_projects_own_decoders_read_the_blocks(ctx1, catalogue):
    from basevarc_amd import build as b
    names, pieces, _, out = catalogue
    _, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_fast_inflate.restype = C.c_long
    H.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    payloads, table, want = bytearray(), [], []
    for name, blocks in zip(names, out[1][1]):
        for data, payload, _ in blocks:
            buf = C.create_string_buffer(len(data) + 1)
            assert H.bvchost_fast_inflate(bytes(payload), len(payload), buf, len(data)) == len(data) and buf.raw[:len(data)] == data, name
            table.append((len(payloads), len(payload), len(data), bb.zlib.crc32(data) & 0xFFFFFFFF))
            payloads += payload + b"\xA5" * 5
            want.append(data)
    got, status = ctx1.inflate_blocks(bytes(payloads), table)
    assert [int(s) for s in status] == [0] * len(table)
    assert got == want


def test_key_0_writes_the_bytes_it_wrote_before_the_key_existed(catalogue):
    names, pieces, _, out = catalogue
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_fixed_catalogue.json")))
    comp, off = out[0][0]
    assert set(golden) == set(names) - set(RANDOM)
    for i, name in enumerate(names):
        if name not in RANDOM:
            assert hashlib.sha256(comp[int(off[i]):int(off[i + 1])].tobytes()).hexdigest() == golden[name], name


def test_more_blocks_than_workgroups_and_a_guard_byte(ctx1):
    from basevarc_amd.lib import bgzf_bound
    pieces = dc.stream_pieces()
    names = [f"piece {i}" for i in range(len(pieces))]
    need = sum(bgzf_bound(len(p)) for p in pieces)
    comp = np.full(need + 64, GUARD, dtype=np.uint8)
    comp, off = deflate_host(ctx1, pieces, comp=comp, comp_cap=need)
    blocks = check(pieces, names, comp, off)
    assert int(off[301]) == int(off[300]) == int(off[302]) and (comp[int(off[-1]):] == GUARD).all()
    assert any(form(b[1]) == "dynamic" for bl in blocks for b in bl) and any(form(b[1]) == "fixed" for bl in blocks for b in bl)
    dcomp, doff = deflate_device(ctx1, pieces)                            # (a guard byte on either side of its buffer)
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()


def zlib_count_sets():
    """The literal/length, distance and code-length counts of zlib's own dynamic blocks (tests/test_bgzf_dynamic_abi.py reads the same)."""
    out = []
    for coverage, seed, _ in dc.SIZE_TEXTS:
        text = dc.sample_text(10000, coverage, seed)[:dc.B]
        c = bb.zlib.compressobj(6, bb.zlib.DEFLATED, -15)
        blocks, _ = dm.read_blocks(c.compress(text) + c.flush())
        m = dm.encode([s for b in blocks for s in b["symbols"]])
        ll, dl = dm.symbol_counts([s for b in blocks for s in b["symbols"]])
        cc = [0] * 19
        for s, _ in m["sequence"]:
            cc[s] += 1
        out += [(f"zlib litlen {coverage}", ll, 15), (f"zlib distance {coverage}", dl, 15), (f"zlib code lengths {coverage}", cc, 7)]
    return out


def test_code_lengths_on_the_count_families(ctx1):
    families = yc.count_families() + zlib_count_sets()
    for name, counts, limit in families:
        got = ctx1.bgzf_code_lengths(np.array(counts, dtype=np.uint32), limit)
        assert list(got) == dm.code_lengths(counts, limit), name
    # 64 sets in one call: more than one wavefront's worth of sets, every one another row of counts
    rng = np.random.default_rng(11)
    rows = np.where(rng.random((64, 286)) < 0.3, 0, (2.0 ** (rng.random((64, 286)) * 15)).astype(np.uint32)).astype(np.uint32)
    rows[5] = 0
    rows[6] = 0
    rows[6, 200] = 3
    rows[7, :20] = yc.fibonacci(20)
    got = ctx1.bgzf_code_lengths(rows, 15)
    for i in range(64):
        assert list(got[i]) == dm.code_lengths([int(x) for x in rows[i]], 15), i
    assert got[7].max() == 15


def test_code_lengths_refusals_leave_the_context_usable(ctx1):
    L, h = ctx1._L, ctx1._h
    counts, lengths = np.ones((2, 30), dtype=np.uint32), np.full((2, 30), GUARD, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.bvc_bgzf_code_lengths(h, 2, None, 30, 15, p(lengths)) == BVC_ERR_ARG
    assert L.bvc_bgzf_code_lengths(h, 2, p(counts), 30, 15, None) == BVC_ERR_ARG
    assert L.bvc_bgzf_code_lengths(h, -1, p(counts), 30, 15, p(lengths)) == BVC_ERR_ARG
    for n_symbols, limit in ((0, 15), (289, 15), (30, 0), (30, 16), (30, 4), (3, 1)):
        assert L.bvc_bgzf_code_lengths(h, 1, p(counts), n_symbols, limit, p(lengths)) == BVC_ERR_ARG, (n_symbols, limit)
    big = counts.copy()
    big[1, 3] = (1 << 24) - 29                                            # the row's sum is 2^24
    assert L.bvc_bgzf_code_lengths(h, 2, p(big), 30, 15, p(lengths)) == BVC_ERR_ARG
    assert (lengths == GUARD).all()
    assert L.bvc_bgzf_code_lengths(h, 0, None, 30, 15, None) == 0
    big[1, 3] -= 1
    assert L.bvc_bgzf_code_lengths(h, 2, p(big), 30, 15, p(lengths)) == 0
    assert list(lengths[0]) == dm.code_lengths([1] * 30, 15) and list(lengths[1]) == dm.code_lengths([int(x) for x in big[1]], 15)
    assert L.bvc_bgzf_code_lengths(h, 1, p(counts), 2, 1, p(lengths)) == 0 and list(lengths[0, :2]) == [1, 1]


def test_size_on_sample_column_texts(ctx0, ctx1):
    for coverage, seed, bound in dc.SIZE_TEXTS:
        text = dc.sample_text(100000, coverage, seed)
        sizes = []
        for ctx in (ctx0, ctx1):
            comp, off = deflate_host(ctx, [text])
            bb.walk_piece(comp[:int(off[1])].tobytes(), text)
            sizes.append(int(off[1]))
        z1, z6 = dc.zlib_size(text, 1), dc.zlib_size(text, 6)
        print(f"coverage {coverage}: text {len(text)}, device fixed {sizes[0]}, dynamic {sizes[1]}, zlib level 1 {z1}, level 6 {z6}: "
              f"dynamic / fixed {sizes[1] / sizes[0]:.3f}, / level 1 {sizes[1] / z1:.3f}, / level 6 {sizes[1] / z6:.3f}")
        assert sizes[1] < sizes[0], (coverage, sizes)
        assert sizes[1] <= bound * z1, (coverage, sizes[1], z1)
