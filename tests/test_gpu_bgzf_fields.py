"""The device deflate encoder with tuning key "bgzf_parse" at 1 (bgzf_block_kernel<true, *>, bgzf_fields_device.h; GPU), at both values of "bgzf_codes".  The
pieces of tests/bgzf_fields_cases.py and the catalogue of tests/bgzf_deflate_cases.py go through the block walker, from host and from
device pointers (device pieces at odd addresses); every block is held, byte for byte, against the encoding
(tests/bgzf_dynamic_model.encode) of the symbols the plain Python model of the rule gives (tests/bgzf_fields_model.py,
docs/BGZF_FIELDS.md), and is read by zlib and the project's own decoders.  With the key at 0 a context writes the bytes of a context
whose key was never set.  The size of the output on the three sample-column texts is held against key 0's in the same test:
not larger at coverage 0.10 and 1.0 with either code, at most 1.05 times at coverage 0.01 with dynamic codes and 1.15 times with the
fixed code (the ratios of the two parses' models, 0.97 and 0.95 | 0.93 and 0.83 | 1.09 and 0.96, and a margin for the candidate set).
What one run on an MI355X gave is in profiles/vcf_deflate_fields/README.txt."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bgzf_blocks as bb
from tests import bgzf_deflate_cases as dc
from tests import bgzf_dynamic_model as dm
from tests import bgzf_fields_cases as fc
from tests import bgzf_fields_model as fm
from tests.test_gpu_bgzf_deflate import GUARD, check, deflate_device, deflate_host
from tests.test_gpu_host_deflate import inputs  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
CODES = (0, 1)
# device key 1 / device key 0 at the same codes key: {coverage: {codes: bound}}
SIZE_BOUNDS = {0.10: {0: 1.0, 1: 1.0}, 0.01: {0: 1.15, 1: 1.05}, 1.0: {0: 1.0, 1: 1.0}}


def context(codes, parse):
    """parse None: the key is never set."""
    from basevarc_amd import Context
    c = Context(0)
    c.set_tuning("bgzf_codes", codes)
    if parse is not None:
        c.set_tuning("bgzf_parse", parse)
    return c


@pytest.fixture(scope="module")
def ctxs():
    out = {codes: context(codes, 1) for codes in CODES}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def catalogue(ctxs):
    """names, pieces, per piece and block the model's two encodings (codes 0, codes 1), and per codes key the host call's (comp, off) and
    its walked blocks: made once."""
    cases = fc.catalogue() + dc.catalogue()
    names, pieces = [c[0] for c in cases], [c[1] for c in cases]
    assert len(set(names)) == len(names)
    want = []
    for piece in pieces:
        rows = []
        for data in fm.blocks_of(piece):
            symbols = fm.symbols(data)
            assert dm.plain_bytes(symbols) == data
            m = dm.encode(symbols)
            rows.append((m["fixed"] if len(m["fixed"]) <= len(data) + 5 else m["stored"], m["data"]))
        want.append(rows)
    out = {}
    for codes in CODES:
        comp, off = deflate_host(ctxs[codes], pieces)
        out[codes] = ((comp, off), check(pieces, names, comp, off))       # (every piece walks, inflates with zlib and equals its input)
    return names, pieces, want, out


def test_the_key_takes_0_and_1_only(ctxs):
    from basevarc_amd.lib import BvcError
    for value in (-1, 2):
        with pytest.raises(BvcError) as e:
            ctxs[0].set_tuning("bgzf_parse", value)
        assert e.value.status == BVC_ERR_ARG
    ctxs[0].set_tuning("bgzf_parse", 0)
    ctxs[0].set_tuning("bgzf_parse", 1)


@pytest.mark.parametrize("codes", CODES)
def test_every_block_is_the_models_encoding_byte_for_byte(catalogue, codes):
    names, pieces, want, out = catalogue
    matches = 0
    for name, rows, blocks in zip(names, want, out[codes][1]):
        assert len(blocks) == len(rows), name
        for row, (data, payload, _) in zip(rows, blocks):
            assert payload == row[codes], (name, len(data), len(payload), len(row[codes]),
                                           next((i for i in range(len(payload)) if payload[i:i + 1] != row[codes][i:i + 1]), None))
            matches += (payload[0] & 6) != 0
    assert matches > 100                                                  # (coded blocks: the parse was at work)


@pytest.mark.parametrize("codes", CODES)
def test_device_pointers_and_a_second_call_give_the_same_bytes(ctxs, catalogue, codes):
    names, pieces, _, out = catalogue
    comp, off = out[codes][0]
    dcomp, doff = deflate_device(ctxs[codes], pieces)                    # (pieces at odd addresses, a guard byte on either side of comp)
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()
    comp2, off2 = deflate_host(ctxs[codes], pieces)
    assert (off2 == off).all() and (comp2[:int(off[-1])] == comp[:int(off[-1])]).all()


@pytest.mark.parametrize("codes", CODES)
def test_the_projects_own_decoders_read_the_blocks(ctxs, catalogue, codes):
    from basevarc_amd import build as b
    names, pieces, _, out = catalogue
    _, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_fast_inflate.restype = C.c_long
    H.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    payloads, table, want = bytearray(), [], []
    for name, blocks in zip(names, out[codes][1]):
        for data, payload, _ in blocks:
            buf = C.create_string_buffer(len(data) + 1)
            assert H.bvchost_fast_inflate(bytes(payload), len(payload), buf, len(data)) == len(data) and buf.raw[:len(data)] == data, name
            table.append((len(payloads), len(payload), len(data), bb.zlib.crc32(data) & 0xFFFFFFFF))
            payloads += payload + b"\xA5" * 5
            want.append(data)
    got, status = ctxs[codes].inflate_blocks(bytes(payloads), table)
    assert [int(s) for s in status] == [0] * len(table)
    assert got == want


@pytest.mark.parametrize("codes", CODES)
def test_more_blocks_than_workgroups_and_a_guard_byte(ctxs, codes):
    from basevarc_amd.lib import bgzf_bound
    pieces = dc.stream_pieces()
    names = [f"piece {i}" for i in range(len(pieces))]
    need = sum(bgzf_bound(len(p)) for p in pieces)
    comp = np.full(need + 64, GUARD, dtype=np.uint8)
    comp, off = deflate_host(ctxs[codes], pieces, comp=comp, comp_cap=need)
    blocks = check(pieces, names, comp, off)
    assert int(off[301]) == int(off[300]) == int(off[302]) and (comp[int(off[-1]):] == GUARD).all()
    for piece, walked in zip(pieces, blocks):
        for data, (_, payload, _) in zip(fm.blocks_of(piece), walked):
            m = dm.encode(fm.symbols(data))
            assert payload == (m["data"] if codes else m["fixed"] if len(m["fixed"]) <= len(data) + 5 else m["stored"])
    dcomp, doff = deflate_device(ctxs[codes], pieces)
    assert (doff == off).all() and (dcomp[:int(off[-1])] == comp[:int(off[-1])]).all()


@pytest.mark.parametrize("codes", CODES)
def test_key_0_writes_the_bytes_of_a_context_whose_key_was_never_set(catalogue, codes):
    names, pieces, _, out = catalogue
    never, zero = context(codes, None), context(codes, 1)
    try:
        zero.set_tuning("bgzf_parse", 0)                                  # (it was 1: back to 0)
        comp_n, off_n = deflate_host(never, pieces)
        comp_z, off_z = deflate_host(zero, pieces)
        assert (off_z == off_n).all() and comp_z[:int(off_n[-1])].tobytes() == comp_n[:int(off_n[-1])].tobytes()
        # ... and key 1 is another parse: the bytes differ
        comp_1, off_1 = out[codes][0]
        assert int(off_1[-1]) != int(off_n[-1]) or comp_1[:int(off_n[-1])].tobytes() != comp_n[:int(off_n[-1])].tobytes()
    finally:
        never.close()
        zero.close()


def test_size_on_sample_column_texts_against_key_0(ctxs):
    ctx0 = {codes: context(codes, 0) for codes in CODES}
    try:
        failures = []
        for coverage, seed, _ in dc.SIZE_TEXTS:
            text = dc.sample_text(100000, coverage, seed)
            z1 = dc.zlib_size(text, 1)
            for codes in CODES:
                sizes = []
                for ctx in (ctx0[codes], ctxs[codes]):
                    comp, off = deflate_host(ctx, [text])
                    bb.walk_piece(comp[:int(off[1])].tobytes(), text)
                    sizes.append(int(off[1]))
                print(f"coverage {coverage}, codes {codes}: text {len(text)}, key 0 {sizes[0]}, key 1 {sizes[1]}, zlib level 1 {z1}: "
                      f"key 1 / key 0 {sizes[1] / sizes[0]:.4f}, key 1 / level 1 {sizes[1] / z1:.4f}")
                if sizes[1] > SIZE_BOUNDS[coverage][codes] * sizes[0]:
                    failures.append((coverage, codes, sizes, SIZE_BOUNDS[coverage][codes]))
        assert not failures, failures
    finally:
        for c in ctx0.values():
            c.close()


def test_pileup_sample_bgzf_at_key_1_inflates_to_the_text():
    from basevarc_amd import Context
    from tests.test_gpu_pileup_bin import encode, fuzz_tiles, sample0_of
    from tests.test_gpu_pileup_sample_bgzf import GUARD as G, check_blocks, comp_need, text_of
    n_in_batch, tiles = fuzz_tiles("wide")
    n = int(n_in_batch.sum())
    s0 = sample0_of(n_in_batch)
    batch_tokens, ref = tiles[0]
    _, records, rs, _ = encode(batch_tokens)
    T = len(ref)
    with Context(0) as ctx:
        out = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, sample_text=True)
        need = comp_need(n, out)
        got = {}
        for codes, parse in ((0, 0), (0, 1), (1, 1), (1, 1)):             # (the keys act from the next call on; the last one repeats)
            ctx.set_tuning("bgzf_codes", codes)
            ctx.set_tuning("bgzf_parse", parse)
            want, want_ln = text_of(ctx, T, n, out)                       # the twin first
            comp = np.full(need + 32, G, dtype=np.uint8)
            comp, off, ln = ctx.pileup_sample_bgzf(T, n, comp, comp_cap=need)
            assert check_blocks(T, out, want, comp, off, ln, want_ln, f"codes {codes}, parse {parse}") > 0
            assert (comp[int(off[T]):] == G).all()
            if (codes, parse) in got:
                prev = got[(codes, parse)]
                assert (off == prev[1]).all() and comp[:int(off[T])].tobytes() == prev[0][:int(off[T])].tobytes()
            got[(codes, parse)] = (comp, off)
    print({k: int(v[1][T]) for k, v in got.items()})
    assert got[(0, 1)][0][:int(got[(0, 1)][1][T])].tobytes() != got[(0, 0)][0][:int(got[(0, 0)][1][T])].tobytes()


def test_the_host_program_with_the_knob_0_and_1(tmp_path, inputs):  # noqa: F811
    from tests.test_gpu_host import _run
    from tests.test_gpu_host_deflate import _outputs, _tiles
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    out = str(tmp_path / "out")
    raw, text = {}, {}
    runs = (("off", {}), ("general", dict(BVC_HOST_DEVICE_DEFLATE="1", BVC_HOST_DEVICE_DEFLATE_FIELDS="0")),
            ("fields", dict(BVC_HOST_DEVICE_DEFLATE="1", BVC_HOST_DEVICE_DEFLATE_FIELDS="1")),
            ("fields, dynamic", dict(BVC_HOST_DEVICE_DEFLATE="1", BVC_HOST_DEVICE_DEFLATE_FIELDS="1", BVC_HOST_DEVICE_DEFLATE_CODES="1")),
            ("fields alone", dict(BVC_HOST_DEVICE_DEFLATE_FIELDS="1")))
    for i, (name, env) in enumerate(runs):
        r = _run(exe, out, lst, fa, ["--keep_tmp"] + (["--rerun"] if i else []), dict(os.environ, BVC_HOST_PROFILE="1", **env), thread=1)
        assert r.returncode == 0, r.stderr[-2000:]
        dev, _, deflated = _tiles(r.stderr)
        assert dev > 0 and deflated == (dev if "BVC_HOST_DEVICE_DEFLATE" in env else 0), (name, r.stderr[-2000:])
        raw[name] = open(out + ".vcf.gz", "rb").read()
        bb.walk_file(raw[name])
        text[name] = _outputs(out)
        assert text[name] == text["off"], name                            # .vcf.gz and .cvg.gz inflate to identical bytes
    print({name: len(x) for name, x in raw.items()})
    assert raw["fields"] != raw["general"] and raw["fields, dynamic"] != raw["fields"]
    assert raw["fields alone"] == raw["off"]                              # the knob acts only with BVC_HOST_DEVICE_DEFLATE=1
