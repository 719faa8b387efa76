"""bvc_bam_pileup_bgzf_deflate, bvc_bam_pileup_text_bgzf_deflate and bvc_bam_pileup_deflate_fetch (include/bvc_bam_deflate.h; GPU), and
tuning key "bgzf_cuts".  On the pileup catalogue, the text form's cases, the seeded random cases and the 100 test BAMs, in both forms: every
block walks (tests/bgzf_blocks.py), each piece's blocks inflate to the slice of what bvc_bam_pileup[_text]_bgzf returns for the same inputs,
piece_bytes / out_off / sample_status / the return code are what that call implies, and `out` is byte for byte what bvc_bgzf_deflate
writes for those slices -- under all eight values of "bgzf_codes" x "bgzf_parse" x "bgzf_cuts".  With cuts 1 every block is the model's
encoding (tests/bgzf_fields_model.py with DELIMITERS a space and a newline); cuts 0 is a context that never set the key; with parse 0 the
key changes nothing.  Pieces of exact sizes around a block's 65280 bytes, empty pieces, more blocks than workgroups; the two-step protocol,
guard bytes, the refusals, no allocation in a second call."""
import zlib

import numpy as np
import pytest

from tests import bam_deflate_cases as zc
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import bam_text_model as tm
from tests import bgzf_blocks as bb
from tests import bgzf_dynamic_model as dm
from tests import bgzf_fields_cases as fc
from tests import bgzf_fields_model as fm

pytestmark = pytest.mark.gpu

GUARD = 64
FORMS = [False, True]
FORM_IDS = ["bin", "text"]
CASES = bc.catalogue() + tm.cases() + [bc.random_case(seed) for seed in bc.RANDOM_SEEDS]
KEYS = [(codes, parse, cuts) for codes in (0, 1) for parse in (0, 1) for cuts in (0, 1)]


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def tuned(ctx, codes, parse, cuts):
    ctx.set_tuning("bgzf_codes", codes)
    ctx.set_tuning("bgzf_parse", parse)
    ctx.set_tuning("bgzf_cuts", cuts)


def call_args(inputs, c):
    comp, table, bam_bytes, off, end, eof, rid, pos, ref = inputs
    from basevarc_amd import lib as bl
    return [comp, np.array(table, dtype=bl.BLOCK_DTYPE), bam_bytes, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref]


def reference(ctx, text, args):
    """What the existing call returns for the same inputs: (rc or the BvcError's status, bytes, rec_start, status)."""
    from basevarc_amd.lib import BvcError
    try:
        rc, data, rs, st, _ = (ctx.bam_pileup_text_bgzf if text else ctx.bam_pileup_bgzf)(*args)
    except BvcError as e:
        return e.status, None, None, None
    return rc, data.tobytes(), [int(x) for x in rs], [int(x) for x in st[:len(args[6])]]


def deflate(ctx, text, args, piece_pos, room, cap=None):
    """One call with guarded outputs: (rc or the BvcError's status, out with GUARD bytes on either side of `room`, out_off, piece_bytes,
    sample_status -- each with GUARD elements behind it --, needed)."""
    from basevarc_amd.lib import BvcError
    k, n = len(piece_pos) - 1, len(args[6])
    whole = np.full(GUARD + room + GUARD, 0xCD, dtype=np.uint8)
    out_off = np.full(k + 1 + GUARD, -0x3232323232323233, dtype=np.int64)
    piece_bytes = np.full(k + GUARD, -0x3232323232323233, dtype=np.int64)
    status = np.full(n + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    try:
        rc, _, _, _, _, need = ctx.bam_pileup_bgzf_deflate(*args, piece_pos, text=text, out=whole[GUARD:GUARD + room], out_cap=room if cap is None else cap,
                                                          out_off=out_off, piece_bytes=piece_bytes, sample_status=status)
    except BvcError as e:
        rc, need = e.status, None
    return rc, whole, out_off, piece_bytes, status, need


def untouched(a):
    return bool((a == (0xCD if a.dtype == np.uint8 else 0xCDCDCDCD if a.dtype == np.uint32 else -0x3232323232323233)).all())


def slices_of(data, rec_start, piece_pos):
    return [data[rec_start[a]:rec_start[b]] for a, b in zip(piece_pos[:-1], piece_pos[1:])]


def encoder(ctx, pieces):
    """bvc_bgzf_deflate of the pieces on the same context: (bytes, comp_off)."""
    data = np.frombuffer(b"".join(pieces) + b"\0", dtype=np.uint8)
    lens = [len(p) for p in pieces]
    comp, off = ctx.bgzf_deflate(data, np.cumsum([0] + lens[:-1]), lens)
    return comp[:int(off[-1])].tobytes(), [int(x) for x in off]


def check_ok(ctx, name, got, pieces, n, walk=True):
    """A BVC_OK call against the pieces the existing call implies and against the encoder on the same context."""
    rc, whole, out_off, piece_bytes, status, need = got
    k = len(pieces)
    assert rc == bm.OK, (name, rc)
    assert [int(x) for x in piece_bytes[:k]] == [len(p) for p in pieces], name
    off = [int(x) for x in out_off[:k + 1]]
    assert off[0] == 0 and off[-1] == need and all(a <= b for a, b in zip(off[:-1], off[1:])), (name, off, need)
    assert untouched(out_off[k + 1:]) and untouched(piece_bytes[k:]) and untouched(status[n:]), name
    assert untouched(whole[:GUARD]) and untouched(whole[GUARD + need:]), name
    out = whole[GUARD:GUARD + need].tobytes()
    if walk:
        for i, p in enumerate(pieces):
            bb.walk_piece(out[off[i]:off[i + 1]], p)                      # (a piece of no bytes: no block)
    enc, enc_off = encoder(ctx, pieces)
    assert off == enc_off and out == enc, (name, off[-1], enc_off[-1])
    return out, off


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_every_case_round_trips_and_is_the_encoders_bytes(ctx, text):
    from basevarc_amd.lib import bgzf_bound
    tuned(ctx, 0, 0, 0)
    seen = set()
    for index, c in enumerate(CASES):
        args = call_args(zc.bgzf_inputs(c), c)
        n, P = len(c["samples"]), len(c["positions"])
        lname, piece_pos = zc.layout_of(index, P)
        rc, data, rs, st = reference(ctx, text, args)
        if rc != bm.OK:
            got = deflate(ctx, text, args, piece_pos, 256)
            assert got[0] == rc and got[5] in (None, 0), (c["name"], got[0], rc)
            assert untouched(got[1]) and untouched(got[2]) and untouched(got[3]), c["name"]
            if rc == bm.BAM_MORE:                                          # (a sample of status 2: the statuses are delivered, as by the existing call)
                assert [int(x) for x in got[4][:n]] == st and 2 in st, c["name"]
            seen.add(rc)
            continue
        pieces = slices_of(data, rs, piece_pos)
        got = deflate(ctx, text, args, piece_pos, sum(bgzf_bound(len(p)) for p in pieces))
        check_ok(ctx, (c["name"], lname), got, pieces, n)
        assert [int(x) for x in got[4][:n]] == st, c["name"]
        seen.add((lname, any(len(p) == 0 for p in pieces)))
    assert {bm.BAM_MORE, bm.ERR_DATA} <= seen and {name for name, _ in zc.layouts(8)} == {s[0] for s in seen if isinstance(s, tuple)}


# ---- the 100 test BAMs ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bams():
    """The _bgzf calls' inputs for the 100 test BAMs' own blocks, every 29th position of the region: (args, n_samples, n_positions)."""
    import os
    from basevarc_amd import lib as bl
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    from tests.test_gpu_bam_pileup import bgzf_blocks_of
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    pv = pv[::29]
    data = bam_data_bytes()
    comp, table, off, end = bytearray(), [], [], []
    files = [l.strip().replace("data/", "", 1) for l in open(os.path.join(hostref.DATA, "bam.list")) if l.strip()]
    out_at = 0
    for f, (d, first, _) in zip(files, data):
        raw = open(os.path.join(hostref.DATA, f), "rb").read()
        off.append(out_at + first)
        for co, cl, isz, crc in bgzf_blocks_of(raw):
            table.append((len(comp) + co, out_at, cl, isz, crc, 1))
            out_at += isz
        end.append(out_at)
        comp += raw
    rid = np.array([refs.index(contig) for _, _, refs in data], dtype=np.int32)
    args = [np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8), np.array(table, dtype=bl.BLOCK_DTYPE), out_at, np.array(off, dtype=np.int64),
            np.array(end, dtype=np.int64), np.ones(len(data), dtype=np.uint8), rid, beg0, end0, mapq, np.array(pv, dtype=np.int32), rg_s,
            np.frombuffer(refseq.encode(), dtype=np.uint8)]
    return args, len(data), len(pv)


@pytest.fixture(scope="module")
def bam_pieces(ctx, bams):
    """{text: (piece_pos, the pieces the existing call implies, its statuses)}: computed once."""
    args, n, P = bams
    out = {}
    for text in FORMS:
        rc, data, rs, st = reference(ctx, text, args)
        assert rc == bm.OK and len(data) > (300000 if text else 30000)
        piece_pos = zc.layouts(P)[1][1]
        out[text] = (piece_pos, slices_of(data, rs, piece_pos), st)
    return out


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_the_bams_under_every_value_of_the_three_keys(ctx, bams, bam_pieces, text):
    from basevarc_amd.lib import bgzf_bound
    args, n, _ = bams
    piece_pos, pieces, st = bam_pieces[text]
    room = sum(bgzf_bound(len(p)) for p in pieces)
    outs = {}
    try:
        for key in KEYS:
            tuned(ctx, *key)
            got = deflate(ctx, text, args, piece_pos, room)
            outs[key] = check_ok(ctx, ("test BAMs", key), got, pieces, n)[0]
            assert [int(x) for x in got[4][:n]] == st
    finally:
        tuned(ctx, 0, 0, 0)
    for codes in (0, 1):
        assert outs[(codes, 0, 0)] == outs[(codes, 0, 1)]                  # with "bgzf_parse" 0 the key changes nothing
        assert len({outs[(codes, 0, 0)], outs[(codes, 1, 0)], outs[(codes, 1, 1)]}) == 3
    sizes = {key: len(o) for key, o in outs.items()}
    print(f"{'text' if text else 'bin'}: {sum(len(p) for p in pieces)} bytes; packed (codes, parse, cuts): {sizes}; "
          f"zlib 1 / 6 of the whole: {len(zlib.compress(b''.join(pieces), 1))} / {len(zlib.compress(b''.join(pieces), 6))}")


def model_payloads(piece, codes):
    """The model's payload of every block of a piece (fm.DELIMITERS as the caller set them)."""
    out = []
    for data in fm.blocks_of(piece):
        m = dm.encode(fm.symbols(data))
        out.append(m["data"] if codes else m["fixed"] if len(m["fixed"]) <= len(data) + 5 else m["stored"])
    return out


@pytest.mark.parametrize("codes", (0, 1))
def test_with_cuts_1_every_block_is_the_models_encoding(ctx, bams, bam_pieces, monkeypatch, codes):
    """The text pieces of the test BAMs through the new call, and the field catalogue (as it is, and with its tabs and colons turned into
    spaces and newlines so that the parse finds its fields) through bvc_bgzf_deflate."""
    from basevarc_amd.lib import bgzf_bound
    monkeypatch.setattr(fm, "DELIMITERS", (0x20, 0x0A))
    args, n, _ = bams
    piece_pos, pieces, _ = bam_pieces[True]
    swap = bytes.maketrans(b"\t: \n", b" \n\t:")
    cat = fc.catalogue()
    others = [(name, piece.translate(swap)) for name, piece in cat] + cat[::7]
    try:
        tuned(ctx, codes, 1, 1)
        got = deflate(ctx, True, args, piece_pos, sum(bgzf_bound(len(p)) for p in pieces))
        assert got[0] == bm.OK
        off = [int(x) for x in got[2][:len(pieces) + 1]]
        out = got[1][GUARD:GUARD + got[5]].tobytes()
        comp, coff = encoder(ctx, [p for _, p in others])
    finally:
        tuned(ctx, 0, 0, 0)
    coded = 0
    for i, p in enumerate(pieces):
        blocks = bb.walk_piece(out[off[i]:off[i + 1]], p)
        for (data, payload, _), want in zip(blocks, model_payloads(p, codes)):
            assert payload == want, ("test BAMs, piece", i, len(data), len(payload), len(want))
            coded += (payload[0] & 6) != 0
    assert coded >= len(pieces)
    for i, (name, p) in enumerate(others):
        blocks = bb.walk_piece(comp[coff[i]:coff[i + 1]], p)
        for (data, payload, _), want in zip(blocks, model_payloads(p, codes)):
            assert payload == want, (name, len(data), len(payload), len(want))


def test_the_key_takes_0_and_1_only_and_0_is_a_context_that_never_set_it(ctx, bam_pieces):
    from basevarc_amd import Context
    from basevarc_amd.lib import BvcError
    for value in (-1, 2):
        with pytest.raises(BvcError) as e:
            ctx.set_tuning("bgzf_cuts", value)
        assert e.value.status == bm.ERR_ARG
    pieces = bam_pieces[True][1] + [p for _, p in fc.catalogue()[::5]]
    never, zero = Context(0), Context(0)
    try:
        for c in (never, zero):
            c.set_tuning("bgzf_parse", 1)
        zero.set_tuning("bgzf_cuts", 1)
        zero.set_tuning("bgzf_cuts", 0)                                    # (it was 1: back to 0)
        assert encoder(never, pieces) == encoder(zero, pieces)
        zero.set_tuning("bgzf_cuts", 1)
        assert encoder(never, pieces) != encoder(zero, pieces)
    finally:
        never.close()
        zero.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def no_sample_args(P):
    """No sample at all: every line is a newline, every record its four-byte length word."""
    c = bc.case("no samples", [], list(range(1001, 1001 + P)))
    return call_args(zc.bgzf_inputs(c), c)


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_pieces_of_exact_sizes_around_a_blocks_input(ctx, text):
    from basevarc_amd.lib import bgzf_bound
    tuned(ctx, 0, 0, 0)
    P, piece_pos, sizes = zc.exact_pieces(text)
    pieces = [(b"\n" if text else b"\0\0\0\0") * (s if text else s // 4) for s in sizes]
    got = deflate(ctx, text, no_sample_args(P), piece_pos, sum(bgzf_bound(s) for s in sizes))
    out, off = check_ok(ctx, "exact sizes", got, pieces, 0)
    assert [len(bb.walk(out[off[i]:off[i + 1]])) for i in range(5)] == [1, 1, 1, 2, 2]


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_more_blocks_than_workgroups_of_the_encoders_grid(ctx, text):
    from basevarc_amd.lib import bgzf_bound
    tuned(ctx, 0, 0, 0)
    k = zc.GRID + 45
    piece_pos = [0]
    for i in range(k):
        piece_pos.append(piece_pos[-1] + (0 if i % 50 == 7 else 1 + i % 3))  # (and an empty piece now and then)
    unit = b"\n" if text else b"\0\0\0\0"
    pieces = [unit * (b - a) for a, b in zip(piece_pos[:-1], piece_pos[1:])]
    got = deflate(ctx, text, no_sample_args(piece_pos[-1]), piece_pos, sum(bgzf_bound(len(p)) for p in pieces))
    out, _ = check_ok(ctx, "301 pieces", got, pieces, 0)
    assert len(bb.walk(out)) == sum(1 for p in pieces if p) > zc.GRID


# ---- the protocol ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_a_cap_too_small_keeps_the_blocks_and_the_fetch_delivers_them(ctx, bams, bam_pieces, text):
    from basevarc_amd import Context
    from basevarc_amd.lib import BvcError, bgzf_bound
    tuned(ctx, 0, 0, 0)
    args, n, _ = bams
    piece_pos, pieces, st = bam_pieces[text]
    k = len(pieces)
    one_call = deflate(ctx, text, args, piece_pos, sum(bgzf_bound(len(p)) for p in pieces))
    want, want_off = check_ok(ctx, "one call", one_call, pieces, n)
    with pytest.raises(BvcError) as e:                                     # the call before was BVC_OK: nothing is kept
        ctx.bam_pileup_deflate_fetch(len(want))
    assert e.value.status == bm.ERR_ARG
    for cap in (0, len(want) - 1):
        rc, whole, out_off, piece_bytes, status, need = deflate(ctx, text, args, piece_pos, len(want), cap=cap)
        assert rc == bm.BAM_MORE and need == len(want) and untouched(whole), cap
        assert [int(x) for x in out_off[:k + 1]] == want_off and [int(x) for x in piece_bytes[:k]] == [len(p) for p in pieces]
        assert untouched(out_off[k + 1:]) and untouched(piece_bytes[k:]) and [int(x) for x in status[:n]] == st and untouched(status[n:])
        small = np.full(len(want) + GUARD, 0xCD, dtype=np.uint8)
        with pytest.raises(BvcError) as e:                                 # too small a cap: refused, and what is kept stays
            ctx.bam_pileup_deflate_fetch(0, out=small, out_cap=len(want) - 1)
        assert e.value.status == bm.ERR_ARG and untouched(small)
        for _ in range(2):                                                 # (the fetch may be repeated)
            ctx.bam_pileup_deflate_fetch(0, out=small, out_cap=len(want))
            assert small[:len(want)].tobytes() == want and untouched(small[len(want):])
    # the binding's own two steps (no buffer given)
    rc, out, out_off, piece_bytes, _, need = ctx.bam_pileup_bgzf_deflate(*args, piece_pos, text=text)
    assert rc == 0 and out.tobytes() == want and [int(x) for x in out_off] == want_off and need == len(want)
    fresh = Context(0)
    try:
        with pytest.raises(BvcError) as e:                                 # no call yet
            fresh.bam_pileup_deflate_fetch(16)
        assert e.value.status == bm.ERR_ARG
    finally:
        fresh.close()


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_the_refusals_a_short_sample_a_damaged_block_and_a_failing_crc(ctx, bams, bam_pieces, text):
    tuned(ctx, 0, 0, 0)
    args, n, P = bams
    piece_pos, pieces, st = bam_pieces[text]

    def refused(code, args, piece_pos, status_written=False):
        rc, whole, out_off, piece_bytes, status, need = deflate(ctx, text, args, piece_pos, 4096)
        assert rc == code and need in (None, 0), (rc, code, need)
        assert untouched(whole) and untouched(out_off) and untouched(piece_bytes) and (status_written or untouched(status))
        return status
    for name, bad in zc.bad_layouts(P):
        refused(bm.ERR_ARG, args, bad)
    # sample 3 ends inside its records and is not said to end its file: more bytes are wanted
    short = list(args)
    short[4], short[5] = args[4].copy(), args[5].copy()
    short[4][3], short[5][3] = args[3][3] + 5000, 0
    assert refused(bm.BAM_MORE, short, piece_pos, status_written=True)[3] == 2
    # one payload byte of a block in the middle flipped; good bytes under a CRC32 that is not theirs
    tab = args[1]
    k = len(tab) // 2
    damaged = list(args)
    damaged[0] = args[0].copy()
    damaged[0][int(tab[k]["comp_off"]) + int(tab[k]["comp_len"]) // 2] ^= 0x5A
    refused(bm.ERR_DATA, damaged, piece_pos, status_written=True)
    crc = list(args)
    crc[1] = tab.copy()
    crc[1][k]["crc32"] ^= 1
    refused(bm.ERR_DATA, crc, piece_pos, status_written=True)
    from basevarc_amd.lib import bgzf_bound                               # the context stays usable
    check_ok(ctx, "after the refusals", deflate(ctx, text, args, piece_pos, sum(bgzf_bound(len(p)) for p in pieces)), pieces, n)


@pytest.mark.parametrize("text", FORMS, ids=FORM_IDS)
def test_a_second_call_of_the_same_shape_allocates_nothing_and_gives_the_same_bytes(ctx, bams, bam_pieces, text):
    import torch
    from basevarc_amd.lib import bgzf_bound
    tuned(ctx, 0, 0, 0)
    args, n, _ = bams
    piece_pos, pieces, _ = bam_pieces[text]
    room = sum(bgzf_bound(len(p)) for p in pieces)
    free, outs = [], []
    for _ in range(3):
        got = deflate(ctx, text, args, piece_pos, room)
        assert got[0] == bm.OK
        ctx.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        outs.append(got[1].tobytes())
    # the library allocates device memory of its own (not torch's pool): what is free on the device after the first call stays free
    assert free[1] == free[0] == free[2], free
    assert outs[0] == outs[1] == outs[2]
