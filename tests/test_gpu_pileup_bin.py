"""bvc_pileup_begin_bin (GPU): a tile of binary temp-batch RECORDS (basevarc_amd/host/pileup.h: `--tmp-format bin` / `raw`) parsed on
the device must give what the CPU parser of that form gives (parse_pileup_bin, basevarc_amd/host/pileup.cpp) -- which is what the
reference's position loop builds from the text form of the same tokens (src/BaseVarC.cpp:403-441): entries in sample order, N bases
dropped, base & 7 / strand & 1, indel entries inheriting the fields of the last base entry before them across records, positions and
tiles -- the tallies bt_f takes and the records of bvc_lrt_csr on those columns.

Oracles: the Python restatement of the reference's parser (oracle/emit_oracle.py Parser) on the text lines of the same tokens; the
text call (bvc_pileup_begin) byte for byte; the host library's own parse_pileup_bin for the 2000-batch tile.  Malformed records are
REFUSED (BVC_ERR_DATA), never followed.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import emit_oracle as eo
from tests.test_gpu_round5 import random_token, reference_columns, tile_of

pytestmark = pytest.mark.gpu

BVC_ERR_ARG, BVC_ERR_DATA = -1, -5


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    _, lib = b.build_host()
    L = C.CDLL(lib)
    L.bvchost_reset_parser.restype = None
    L.bvchost_site_parse_bin.restype = C.c_void_p
    L.bvchost_site_parse_bin.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_int32]
    L.bvchost_site_free.restype = None
    L.bvchost_site_free.argtypes = [C.c_void_p]
    L.bvchost_site_size.restype = C.c_int32
    L.bvchost_site_size.argtypes = [C.c_void_p]
    L.bvchost_site_field.restype = C.c_int32
    L.bvchost_site_field.argtypes = [C.c_void_p, C.c_int32, C.c_int]
    return L


# ------------------------------------------------------------------------------------------------ the same tokens in both forms
def entry_bytes(j, tok, junk=0xA5):
    """One token of sample-in-batch j as a binary entry (b'' for '.').  The base .. rpr bytes and the strand bit of an INDEL entry are
    not read by the parser: they carry junk here, so that an implementation that reads them shows."""
    if tok == ".":
        return b""
    if tok[0] in "+-N":
        t = tok.encode()
        return struct.pack("<IBBBBBH", j, junk & 0xFF, junk ^ 0x11, junk ^ 0x22, junk ^ 0x33, 2 | (j & 1), len(t)) + t
    f = [int(x) for x in tok.split(",")]
    return struct.pack("<IBBBBB", j, f[0] & 0xFF, f[1] & 0xFF, f[2] & 0xFF, f[3] & 0xFF, f[4] & 1)


def encode(batch_tokens):
    """batch_tokens[b][t] = the tokens of position t of batch b, one per sample of the batch.  Returns (batch_lines for tile_of,
    records, rec_start [nb, T + 1], stats of the input): batches start at every alignment (pad bytes between them, as tile_of does)."""
    nb, T = len(batch_tokens), len(batch_tokens[0]) if batch_tokens else 0
    lines = [["".join(tok + " " for tok in toks) for toks in per_pos] for per_pos in batch_tokens]
    rec = bytearray()
    rs = np.zeros((nb, T + 1), dtype=np.uint32)
    stats = dict(indel_first=0, indel_after_n=0, indel_run=0, over_64_entries=0, indel_past_576=0)
    for b, per_pos in enumerate(batch_tokens):
        while len(rec) % 16 != (b * 5 + 3) % 16:
            rec += b"\xEE"
        for t, toks in enumerate(per_pos):
            payload = bytearray()
            kinds = []                                           # per entry: 'b' base, 'n' N base, 'i' indel
            for j, tok in enumerate(toks):
                e = entry_bytes(j, tok)
                if not e:
                    continue
                is_ind = tok[0] in "+-N"
                if is_ind and len(payload) > 576:
                    stats["indel_past_576"] += 1
                kinds.append("i" if is_ind else ("n" if int(tok.split(",")[0]) & 7 == 4 else "b"))
                payload += e
            k = "".join(kinds)
            stats["indel_first"] += k.startswith("i")
            stats["indel_after_n"] += "ni" in k
            stats["indel_run"] += "ii" in k
            stats["over_64_entries"] += len(k) > 64
            rs[b, t] = len(rec)
            rec += struct.pack("<I", len(payload)) + payload
        rs[b, T] = len(rec)
    return lines, bytes(rec), rs, stats


def sample0_of(n_in_batch):
    n = np.asarray(n_in_batch, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32) if len(n) else np.zeros(0, np.int32)


def fields(e):
    return tuple(int(e[f]) for f in ("base", "mapq", "qual", "rpr", "strand", "is_indel"))


def check_columns(ctx, out, records, cols, ref, min_af, where):
    """out (a pileup_tile_bin dict) against cols = [(aiv, sample)] per position; returns the (bases, quals) of the sites."""
    T = len(cols)
    eoff = out["entry_off"]
    assert eoff[0] == 0 and eoff[T] == len(out["entries"]) == sum(len(a) for a, _ in cols), where
    texts = {int(r["entry"]): records[int(r["text_off"]):int(r["text_off"]) + int(r["len"])].decode() for r in out["indels"]}
    assert len(texts) == len(out["indels"]), where
    sites = []
    for t, (aiv, sample) in enumerate(cols):
        e = out["entries"][eoff[t]:eoff[t + 1]]
        assert len(e) == len(aiv), (where, t)
        assert out["samples"][eoff[t]:eoff[t + 1]].tolist() == list(sample), (where, t)
        tally = np.zeros(32, dtype=np.int64)
        for k, a in enumerate(aiv):
            assert fields(e[k]) == (a["base"], a["mapq"], a["qual"], a["rpr"], a["strand"], a["is_indel"]), (where, t, k, fields(e[k]), a)
            tally[(16 if a["is_indel"] else 0) + (a["strand"] << 3 | a["base"])] += 1
            if a["is_indel"] and a.get("indel") is not None:
                assert texts[int(eoff[t]) + k] == a["indel"], (where, t, k)
        assert out["tally"][t].tolist() == tally.tolist(), (where, t)
        sites.append((np.array([a["base"] for a in aiv if not a["is_indel"]], dtype=np.int8),
                      np.array([a["qual"] for a in aiv if not a["is_indel"]], dtype=np.uint8).astype(np.int8),
                      np.array([s for a, s in zip(aiv, sample) if not a["is_indel"]], dtype=np.int32)))
    assert set(texts) == {int(eoff[t]) + k for t, (aiv, _) in enumerate(cols) for k, a in enumerate(aiv) if a["is_indel"]}, where
    offs = np.concatenate([[0], np.cumsum([len(b) for b, _, _ in sites])]).astype(np.int64)
    allb = np.concatenate([b for b, _, _ in sites] + [np.zeros(0, np.int8)])
    allq = np.concatenate([q for _, q, _ in sites] + [np.zeros(0, np.int8)])
    alls = np.concatenate([s for _, _, s in sites] + [np.zeros(0, np.int32)])
    one = np.zeros(1, np.int8)
    want = ctx.lrt_csr(offs, allb if len(allb) else one, allq if len(allq) else one, ref, min_af)
    assert out["results"].tobytes() == want.tobytes(), where
    return offs, allb, allq, alls


def check_called_only(full, co, where):
    """bvc_pileup_finish_called on the same tile: everything the same, the entries of the called positions only."""
    T = len(full["entry_off"]) - 1
    eoff = full["entry_off"]
    for key in ("entry_off", "tally", "results", "indels"):
        assert co[key].tobytes() == full[key].tobytes(), (where, key)
    assert co["carry_out"] == full["carry_out"], where
    coff, called = co["called_off"], full["results"]["called"]
    assert coff[0] == 0 and coff[T] == len(co["entries"]) == len(co["samples"]) == sum(int(eoff[t + 1] - eoff[t]) for t in range(T) if called[t])
    for t in range(T):
        n_t = int(eoff[t + 1] - eoff[t]) if called[t] else 0
        assert coff[t + 1] - coff[t] == n_t, (where, t)
        assert co["entries"][coff[t]:coff[t + 1]].tobytes() == full["entries"][eoff[t]:eoff[t] + n_t].tobytes(), (where, t)
        assert co["samples"][coff[t]:coff[t + 1]].tolist() == full["samples"][eoff[t]:eoff[t] + n_t].tolist(), (where, t)


def check_bin_tile(ctx, batch_tokens, n_in_batch, ref, min_af, parser, carry_in, where=""):
    lines, records, rs, stats = encode(batch_tokens)
    s0 = sample0_of(n_in_batch)
    out = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, min_af, carry_in=carry_in)
    cols = reference_columns(lines, parser)
    check_columns(ctx, out, records, cols, ref, min_af, where)
    ai = parser.ai
    assert out["carry_out"] == [ai["base"], ai["mapq"], ai["qual"], ai["rpr"], ai["strand"]], where
    co = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, min_af, carry_in=carry_in, called_only=True)
    check_called_only(out, co, where)
    return out, stats


def wide_token(rng, p_data, p_indel):
    """Every byte field 0..255, the base byte 0..255 (base = byte & 7), strand values beyond one bit."""
    if rng.random() < p_data:
        return f"{rng.integers(0, 256)},{rng.integers(0, 256)},{rng.integers(0, 256)},{rng.integers(0, 256)},{rng.integers(0, 10)}"
    return random_token(rng, 0.0, p_indel / max(1e-9, 1.0 - p_data))


SHAPES = {"sparse": (0.08, 0.004), "dense": (0.9, 0.02), "indel_heavy": (0.2, 0.3), "wide": (0.5, 0.05), "tiny_batches": (0.3, 0.05)}
# for the comparison with the text call: the wide tokens of the text form's own fuzz (tests/test_gpu_round5.py: a base of one digit,
# the other fields up to 999 -- the text parser wraps them to a byte, the records hold the wrapped byte)
TEXT_SHAPES = dict(SHAPES, wide_text=(0.5, 0.05))
# what each shape's input must hold, so that the inherit and the multi-step paths of the record walk cannot be skipped silently
MUST_HOLD = {"sparse": (), "dense": ("indel_first", "indel_run", "over_64_entries", "indel_past_576"),
             "indel_heavy": ("indel_first", "indel_after_n", "indel_run", "over_64_entries", "indel_past_576"),
             "wide": ("indel_first", "indel_after_n", "indel_run", "over_64_entries", "indel_past_576"),
             "tiny_batches": ("indel_first", "indel_after_n", "indel_run")}


def fuzz_tiles(shape):
    rng = np.random.default_rng({"sparse": 11, "dense": 12, "indel_heavy": 13, "wide": 14, "tiny_batches": 15, "wide_text": 16}[shape])
    p_data, p_indel = TEXT_SHAPES[shape]
    n_in_batch = np.array({"tiny_batches": [1, 2, 1, 3, 1, 1, 7, 1]}.get(shape, [700, 37, 1, 300]), dtype=np.int32)
    tiles = []
    for tile in range(3):
        T = [13, 1, 40][tile]
        tok = (lambda p: wide_token(rng, p, p_indel)) if shape == "wide" else (lambda p: random_token(rng, p, p_indel, shape == "wide_text"))
        tiles.append(([[[tok(p_data if (t + tile) % 7 else 0.0) for _ in range(n)] for t in range(T)] for n in n_in_batch],
                      rng.integers(0, 4, T).astype(np.int8)))
    return n_in_batch, tiles


@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_parse_of_fuzzed_records_equals_the_restated_parser(ctx, shape):
    """Records of every kind the writer can produce, batches at every alignment: entries crossing the 8-byte words, records of more
    than 64 entries (several steps of the walk), indel entries first in a record / after an N base / in runs / deep in a long
    record, byte fields over their whole range, batches of one sample, empty positions; three tiles share one parser state."""
    n_in_batch, tiles = fuzz_tiles(shape)
    parser = eo.Parser()
    carry = [0, 0, 0, 0, 0]
    total = dict()
    for i, (batch_tokens, ref) in enumerate(tiles):
        out, stats = check_bin_tile(ctx, batch_tokens, n_in_batch, ref, 0.001, parser, carry, where=f"{shape} tile {i}")
        carry = out["carry_out"]
        for k, v in stats.items():
            total[k] = total.get(k, 0) + int(v)
    for key in MUST_HOLD[shape]:
        assert total[key] >= 1, (shape, key, total)


@pytest.mark.parametrize("shape", ["dense", "indel_heavy", "wide_text", "tiny_batches"])
def test_the_binary_call_and_the_text_call_agree_byte_for_byte(ctx, shape):
    """The same tokens as text lines through bvc_pileup_begin and as records through bvc_pileup_begin_bin: entry_off, tally, entries,
    samples, records and carry identical, the indel records agree in entry and text; also with 5 groups (some samples in none) and in
    the called-only form."""
    n_in_batch, tiles = fuzz_tiles(shape)
    n = int(n_in_batch.sum())
    rng = np.random.default_rng(99)
    group = rng.integers(0, 5, n).astype(np.uint8)
    group[rng.random(n) < 0.1] = 255
    s0 = sample0_of(n_in_batch)
    carry = [0, 0, 0, 0, 0]
    for i, (batch_tokens, ref) in enumerate(tiles):
        lines, records, rs, _ = encode(batch_tokens)
        text, ls = tile_of(lines)
        for kw in (dict(), dict(group_of_sample=group, n_groups=5), dict(group_of_sample=group, n_groups=5, called_only=True)):
            a = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, **kw)
            b = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, **kw)
            assert a is not None
            keys = ["entry_off", "tally", "entries", "samples", "results"] + (["grp_results"] if kw else []) + (["called_off"] if "called_only" in kw else [])
            for key in keys:
                assert a[key].tobytes() == b[key].tobytes(), (shape, i, sorted(kw), key)
            assert a["carry_out"] == b["carry_out"]
            assert a["indels"]["entry"].tolist() == b["indels"]["entry"].tolist()
            ta = [text[int(r["text_off"]):int(r["text_off"]) + int(r["len"])] for r in a["indels"]]
            tb = [records[int(r["text_off"]):int(r["text_off"]) + int(r["len"])] for r in b["indels"]]
            assert ta == tb, (shape, i)
        carry = b["carry_out"]


def test_device_parse_of_the_reference_test_data_as_records(ctx):
    """The temp batches of the reference's test data (100 BAMs, chr17:41197700-41276155, -q 20; batch = 30 samples) re-encoded as
    records: every tile of 2048 positions against the restated parser, records against bvc_lrt_csr."""
    from tests import hostref
    P = hostref.Pipeline(mapq=20, batch=30, thread=1)
    files = P.batch_files()
    nb = 1 + (P.n - 1) // P.batch
    per_batch = [[l.split(" ")[:-1] for l in files[(0, ib)].split("\n")[1:-1]] for ib in range(nb)]
    n_in_batch = np.array([min(P.batch, P.n - ib * P.batch) for ib in range(nb)], dtype=np.int32)
    assert all(len(pb) == len(P.pv) for pb in per_batch)
    assert all(len(toks) == n_in_batch[ib] for ib, pb in enumerate(per_batch) for toks in pb[:50])
    parser = eo.Parser()
    carry = [0, 0, 0, 0, 0]
    n_entries = 0
    for t0 in range(0, len(P.pv), 2048)[:12]:
        t1 = min(len(P.pv), t0 + 2048)
        ref = np.array(["ACGT".index(P.refseq[p - P.rg_s]) for p in P.pv[t0:t1]], dtype=np.int8)
        out, _ = check_bin_tile(ctx, [pb[t0:t1] for pb in per_batch], n_in_batch, ref, P.min_af, parser, carry, where=f"test data tile {t0}")
        carry = out["carry_out"]
        n_entries += len(out["entries"])
    assert n_entries > 100000


@pytest.mark.parametrize("k_groups", [0, 5])
def test_a_tile_of_2000_batches_equals_the_host_parser(ctx, H, k_groups):
    """The shape of N = 1e6 with --batch 500: 2000 batches of 500 samples in ONE tile of 16 positions, coverage 1 %, a few indels.
    Oracle: the host library's own parse_pileup_bin, position after position in one process (its carry is process state: reset, then
    the positions in order, as the device takes them position-major with carry_in = 0)."""
    nb, n_in, T, cov = 2000, 500, 16, 0.01
    rng = np.random.default_rng(2000 + k_groups)
    n_in_batch = np.full(nb, n_in, dtype=np.int32)
    s0 = sample0_of(n_in_batch)
    rec = bytearray()
    rs = np.zeros((nb, T + 1), dtype=np.uint32)
    payloads = [[None] * nb for _ in range(T)]
    for b in range(nb):
        for t in range(T):
            js = np.flatnonzero(rng.random(n_in) < cov)
            p = bytearray()
            for j in js:
                if rng.random() < 0.01:
                    txt = ("+" + "ACGT"[int(rng.integers(4))] * int(rng.integers(1, 9))).encode()
                    p += struct.pack("<IBBBBBH", int(j), 0, 0, 0, 0, 2, len(txt)) + txt
                else:
                    p += struct.pack("<IBBBBB", int(j), int(rng.integers(0, 5)), int(rng.integers(0, 61)), int(rng.integers(0, 42)),
                                     int(rng.integers(0, 100)), int(rng.integers(0, 2)))
            payloads[t][b] = bytes(p)
            rs[b, t] = len(rec)
            rec += struct.pack("<I", len(p)) + p
        rs[b, T] = len(rec)
    records = bytes(rec)
    ref = rng.integers(0, 4, T).astype(np.int8)
    group = None
    if k_groups:
        group = rng.integers(0, k_groups, nb * n_in).astype(np.uint8)
        group[rng.random(nb * n_in) < 0.1] = 255
    out = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 1e-4, group_of_sample=group, n_groups=k_groups)
    H.bvchost_reset_parser()
    cols = []
    n_ind = 0
    for t in range(T):
        blob = b"".join(struct.pack("<II", n_in, len(p)) + p for p in payloads[t])
        h = H.bvchost_site_parse_bin(blob, len(blob), nb, t)
        assert h
        aiv, sample = [], []
        for k in range(H.bvchost_site_size(h)):
            f = [H.bvchost_site_field(h, k, i) for i in range(7)]
            aiv.append(dict(base=f[0], mapq=f[1], qual=f[2], rpr=f[3], strand=f[4], is_indel=f[5], indel=None))
            sample.append(f[6])
            n_ind += f[5]
        H.bvchost_site_free(h)
        cols.append((aiv, sample))
    assert n_ind > 100 and sum(len(a) for a, _ in cols) > 100000
    offs, allb, allq, alls = check_columns(ctx, out, records, cols, ref, 1e-4, f"2000 batches, {k_groups} groups")
    if k_groups:
        res, gres = ctx.lrt_csr_groups(offs, allb, allq, alls, ref, 1e-4, group, k_groups)
        assert out["results"].tobytes() == res.tobytes() and out["grp_results"].tobytes() == gres.tobytes()


# ------------------------------------------------------------------------------------------------ refusals and edges
def base_entry(j, base=1, mapq=30, qual=25, rpr=7, strand=1):
    return struct.pack("<IBBBBB", j, base, mapq, qual, rpr, strand)


def one_batch(payloads, pad=0):
    """records + rec_start [1, T + 1] of one batch whose payloads are given as they are (well-formed or not)."""
    rec = bytearray(b"\xEE" * pad)
    rs = [0] * (len(payloads) + 1)
    for t, p in enumerate(payloads):
        rs[t] = len(rec)
        rec += struct.pack("<I", len(p)) + p
    rs[len(payloads)] = len(rec)
    return bytes(rec), np.array([rs], dtype=np.uint32)


def status_of(call):
    from basevarc_amd.lib import BvcError
    with pytest.raises(BvcError) as ei:
        call()
    return ei.value.status


def test_malformed_records_are_refused_not_followed(ctx):
    """What parse_pileup_bin refuses, and a sample index that is not below the batch's size: BVC_ERR_DATA, the context stays usable,
    the tile is not begun.  Every bad record is the LAST of its buffer and its bad length points far past the buffer's end: a walk
    that followed it would read outside (the kernel compares with the record's end first)."""
    n_in = np.array([4], dtype=np.int32)
    good = [base_entry(0) + base_entry(3, base=2), struct.pack("<IBBBBBH", 1, 0, 0, 0, 0, 2, 3) + b"+AC"]
    ref = np.zeros(2, dtype=np.int8)

    def run(payloads, nib=n_in, pad=0):
        records, rs = one_batch(payloads, pad)
        return ctx.pileup_tile_bin(records, rs, [0], nib, ref, 0.001)
    ok = run(good)
    assert len(ok["entries"]) == 3 and [fields(e) for e in ok["entries"]] == [(1, 30, 25, 7, 1, 0), (2, 30, 25, 7, 1, 0), (2, 30, 25, 7, 1, 1)]
    bad = [base_entry(0) + base_entry(1)[:5]]                                               # cut in the middle of an entry
    bad += [base_entry(0)[:n] for n in range(1, 9)]                                         # payloads of 1..8 bytes
    bad += [base_entry(0) + struct.pack("<IBBBBBH", 1, 0, 0, 0, 0, 2, 65535) + b"+A",      # indel text far past the payload's end
            struct.pack("<IBBBBBH", 1, 0, 0, 0, 0, 2, 3) + b"+A",                           # ... one byte past it
            base_entry(0) + struct.pack("<IBBBBB", 1, 0, 0, 0, 0, 2),                       # indel entry with 9 bytes left
            base_entry(0) + struct.pack("<IBBBBB", 1, 0, 0, 0, 0, 2) + b"\xFF",             # ... with 10
            base_entry(4),                                                                  # sample index = n_in_batch
            struct.pack("<IBBBBBH", 4, 0, 0, 0, 0, 2, 1) + b"N",                            # ... of an indel entry
            base_entry(0xFFFFFFFF)]
    for i, p in enumerate(bad):
        for pad in (0, 3):
            assert status_of(lambda: run([good[0], p], pad=pad)) == BVC_ERR_DATA, (i, pad)
        assert status_of(lambda: run([p, good[1]])) == BVC_ERR_DATA, i
    # a finish after a refused begin has no tile
    assert status_of(lambda: run([good[0], bad[0]])) == BVC_ERR_DATA
    assert status_of(lambda: ctx._pileup_finish(2, 0, 0, 0, ref, 0.001, [0] * 5, None, 0)) == BVC_ERR_ARG
    again = run(good)                                            # the context is as usable as before
    for key in ("entry_off", "tally", "entries", "samples", "results"):
        assert again[key].tobytes() == ok[key].tobytes(), key
    # a batch of no samples: any entry of it is out of range, empty records are fine
    records, rs = one_batch([b"", b""])
    assert len(ctx.pileup_tile_bin(records, rs, [0], [0], ref, 0.001)["entries"]) == 0
    records, rs = one_batch([b"", base_entry(0)])
    assert status_of(lambda: ctx.pileup_tile_bin(records, rs, [0], [0], ref, 0.001)) == BVC_ERR_DATA


def test_a_record_table_that_does_not_fit_the_records_is_an_argument_error(ctx):
    n_in = np.array([4], dtype=np.int32)
    ref = np.zeros(2, dtype=np.int8)
    records, rs = one_batch([base_entry(0) + base_entry(3), base_entry(2)])
    assert len(ctx.pileup_tile_bin(records, rs, [0], n_in, ref, 0.001)["entries"]) == 3

    def run(table, data=records):
        return ctx.pileup_tile_bin(data, np.array([table], dtype=np.uint32), [0], n_in, ref, 0.001)
    a, b, c = (int(x) for x in rs[0])
    assert status_of(lambda: run([a, b - 9, c])) == BVC_ERR_ARG                    # disagrees with the length words
    assert status_of(lambda: run([a, b, c + 9])) == BVC_ERR_ARG                    # past records_bytes
    assert status_of(lambda: run([b, a, c])) == BVC_ERR_ARG                        # descending
    assert status_of(lambda: run([a, b, b])) == BVC_ERR_ARG                        # a record without its length word
    assert status_of(lambda: run([a, b, c], records[:-1])) == BVC_ERR_ARG          # the buffer ends inside the last record
    lying = bytearray(records)
    lying[b:b + 4] = struct.pack("<I", 0x7FFFFFF0)                                  # a length word far past the buffer
    assert status_of(lambda: run([a, b, c], bytes(lying))) == BVC_ERR_ARG
    assert len(run([a, b, c])["entries"]) == 3


def test_edges_of_the_record_form(ctx):
    ref3 = np.zeros(3, dtype=np.int8)
    # no positions; no batches (with and without positions)
    out = ctx.pileup_tile_bin(b"", np.zeros((2, 1), dtype=np.uint32), [0, 4], [4, 4], np.zeros(0, dtype=np.int8), 0.001, carry_in=[3, 9, 8, 7, 1])
    assert out["entry_off"].tolist() == [0] and out["carry_out"] == [3, 9, 8, 7, 1]
    out = ctx.pileup_tile_bin(b"", np.zeros((0, 1), dtype=np.uint32), [], [], np.zeros(0, dtype=np.int8), 0.001, carry_in=[3, 9, 8, 7, 1])
    assert out["entry_off"].tolist() == [0] and out["carry_out"] == [3, 9, 8, 7, 1]
    out = ctx.pileup_tile_bin(b"", np.zeros((0, 4), dtype=np.uint32), [], [], ref3, 0.001, carry_in=[3, 9, 8, 7, 1])
    assert out["entry_off"].tolist() == [0, 0, 0, 0] and out["results"]["called"].tolist() == [0, 0, 0] and out["carry_out"] == [3, 9, 8, 7, 1]
    # every payload empty, one batch of no samples
    lines, records, rs, _ = encode([[["."] * 3] * 3, [[]] * 3])
    out = ctx.pileup_tile_bin(records, rs, [0, 3], [3, 0], ref3, 0.001, carry_in=[2, 50, 33, 6, 1])
    assert out["entry_off"].tolist() == [0, 0, 0, 0] and out["tally"].sum() == 0 and out["carry_out"] == [2, 50, 33, 6, 1]
    # nothing, an N base only (dropped, but it IS the last base entry), an indel: as the text form's test of the same
    lines, records, rs, _ = encode([[[".", ".", "."], ["4,1,1,1,1", ".", "."], [".", "N", "."]]])
    out = ctx.pileup_tile_bin(records, rs, [5], [3], ref3, 0.001, carry_in=[2, 50, 33, 6, 1])
    assert out["entry_off"].tolist() == [0, 0, 0, 1] and out["samples"].tolist() == [6]
    assert fields(out["entries"][0]) == (4, 1, 1, 1, 1, 1) and out["carry_out"] == [4, 1, 1, 1, 1]
    # ... the indel first in the tile: the carry of the tile before
    lines, records, rs, _ = encode([[[".", "N", "."]]])
    out = ctx.pileup_tile_bin(records, rs, [5], [3], np.zeros(1, dtype=np.int8), 0.001, carry_in=[2, 50, 33, 6, 1])
    assert fields(out["entries"][0]) == (2, 50, 33, 6, 1, 1)
    assert out["tally"][0][16 + (1 << 3 | 2)] == 1 and out["tally"][0].sum() == 1 and out["carry_out"] == [2, 50, 33, 6, 1]
    # records of exactly 64 and 65 base entries (one step of the walk and one entry more), 63 + an indel, 64 + an indel
    parser = eo.Parser()
    rng = np.random.default_rng(6)
    tok = lambda: f"{rng.integers(0, 4)},{rng.integers(0, 61)},{rng.integers(0, 42)},{rng.integers(0, 100)},{rng.integers(0, 2)}"
    toks = [[tok() for _ in range(64)] + ["."] * 6, [tok() for _ in range(65)] + ["."] * 5, [tok() for _ in range(63)] + ["-ACG"] + ["."] * 6,
            [tok() for _ in range(64)] + ["+T"] + ["."] * 5, ["."] * 5 + [tok() for _ in range(65)]]
    out, _ = check_bin_tile(ctx, [toks], np.array([70], dtype=np.int32), rng.integers(0, 4, 5).astype(np.int8), 0.001, parser, [0] * 5, "64 / 65")
    assert np.diff(out["entry_off"]).tolist() == [64, 65, 64, 65, 65]
    # an indel text of 65535 bytes (the longest the form holds) between two base entries, and one of 0 bytes
    long_text = "+" + "ACGT" * 16383 + "AC"
    assert len(long_text) == 65535
    parser = eo.Parser()
    out, _ = check_bin_tile(ctx, [[["1,2,3,4,1", long_text, "2,9,8,7,0"], [".", "-A", "."]]], np.array([3], dtype=np.int32), np.zeros(2, dtype=np.int8),
                            0.001, parser, [0] * 5, "65535")
    assert out["indels"]["len"].tolist() == [65535, 2]
    payload = base_entry(0) + struct.pack("<IBBBBBH", 1, 9, 9, 9, 9, 2, 0) + base_entry(2, base=3, strand=0)
    records, rs = one_batch([payload], pad=5)
    out = ctx.pileup_tile_bin(records, rs, [10], [3], np.zeros(1, dtype=np.int8), 0.001)
    assert [fields(e) for e in out["entries"]] == [(1, 30, 25, 7, 1, 0), (1, 30, 25, 7, 1, 1), (3, 30, 25, 7, 0, 0)]
    assert out["samples"].tolist() == [10, 11, 12] and out["indels"]["len"].tolist() == [0] and out["carry_out"] == [3, 30, 25, 7, 0]
