"""GPU: the text parser's kernels on the hand-built catalogue (tests/pileup_lines.py), whose census (tests/test_pileup_lines.py)
says that every path of pileup_parse_kernel, pileup_scan_kernel, pileup_patch_kernel, called_scan_kernel / called_gather_kernel and
of region_lines_kernel / region_scan_kernel is taken.

Regular tiles go through Context.pileup_tile and tests/test_gpu_round5.py's check_tile: entries, samples, tallies, indel records and
texts, the carry, the records byte for byte against bvc_lrt_csr on the same columns, and the called-only form -- against the
restated parser (oracle/emit_oracle.py), which tests/test_pileup_lines.py holds against a strict split.  Irregular tiles must come
back as None with their regular twin accepted.  Every comparison is integer or byte equality.

Not covered, by decision: more than 262,144 SEGMENTS in one bvc_pileup_begin_bgzf call (the second trip of region_lines_kernel's
loop needs 256 MiB of text in one call).
"""
import zlib

import numpy as np
import pytest

from oracle import emit_oracle as eo
from tests import pileup_lines as S
from tests import pileup_model as M
from tests import test_gpu_round5 as r5

pytestmark = pytest.mark.gpu
MIN_AF = 0.001


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def by_name():
    return {c.name: c for c in S.regular()}


def tile(ctx, c, **kw):
    text, ls = S.layout(c.batch_lines, c.align)
    return ctx.pileup_tile(text, ls, S.sample0_of(c.n_in_batch), c.n_in_batch, c.ref, MIN_AF, carry_in=c.carry_in, **kw)


def check(ctx, monkeypatch, c):
    """check_tile on the case's own layout (the case says where every batch starts; check_tile's tile_of has one fixed stride)."""
    text, ls = S.layout(c.batch_lines, c.align)
    monkeypatch.setattr(r5, "tile_of", lambda batch_lines: (text, ls))
    out, _ = r5.check_tile(ctx, c.batch_lines, c.n_in_batch, c.ref, MIN_AF, S.parser_for(c), c.carry_in, where=c.name)
    return out


def test_base_token_of_every_length_at_every_alignment(ctx, monkeypatch, by_name):
    """Every token length 10..20 at every p % 16, each pair in a tile of its own first (so that a refusal names its pair), then all of
    them in one tile against the restated parser; fields that wrap their bit fields.  Before parse_base_token read a fourth word this
    failed at exactly the pairs with p % 8 + length - 1 >= 24: (18, 7), (19, 6), (19, 7), (20, 5), (20, 6), (20, 7) -- the token's
    last bytes were taken with a 64-bit shift by 64 or more, which the hardware counts modulo 64."""
    refused = sorted({(L, a % 8) for L in range(10, 21) for a in range(16) if tile(ctx, S.base_length_tile(L, a)) is None})
    print("refused (length, p % 8):", refused)
    assert refused == []
    check(ctx, monkeypatch, by_name["base_lengths"])
    check(ctx, monkeypatch, by_name["field_wrap"])


def test_lines_at_every_start_and_end_lanes_steps_and_counters(ctx, monkeypatch, by_name):
    for name in ("line_edges", "long_lines", "step_edges", "counters"):
        check(ctx, monkeypatch, by_name[name])


def test_indel_tokens_and_where_their_fields_come_from(ctx, monkeypatch, by_name):
    for name in ("indel_lengths", "indel_sources", "patch_far"):
        check(ctx, monkeypatch, by_name[name])
    a = check(ctx, monkeypatch, by_name["chain_a"])                  # three consecutive tiles share the carry
    assert a["carry_out"] == by_name["chain_b"].carry_in
    b = check(ctx, monkeypatch, by_name["chain_b"])
    assert b["carry_out"] == by_name["chain_c"].carry_in
    c = check(ctx, monkeypatch, by_name["chain_c"])
    e = c["entries"][0]                                              # "-G": chain_a's N base token, two tiles back
    assert [int(e[k]) for k in ("base", "mapq", "qual", "rpr", "strand", "is_indel")] == [4, 21, 22, 23, 0, 1]


@pytest.mark.parametrize("which", ["small", "4095_4096", "4097_8191", "8193"])
def test_line_counts_of_the_scan_and_patch_kernels(ctx, monkeypatch, by_name, which):
    """n_lines 1..9, 255, 256, 512 / 4095, 4096 / 4097, 8191 / 8193 in batches of 1, 3, 5 and 7 one-sample lines."""
    want = {"small": (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 512), "4095_4096": (4095, 4096), "4097_8191": (4097, 8191), "8193": (8193,)}[which]
    for n in want:
        check(ctx, monkeypatch, by_name["lines_%d" % n])


@pytest.mark.parametrize("T", [1023, 1024, 1025, 2049])
def test_called_positions_on_both_sides_of_a_scan_step(ctx, monkeypatch, by_name, T):
    """called_scan_kernel / called_gather_kernel: which positions are called is read from the records (check_tile holds them against
    bvc_lrt_csr on the reference columns), and there must be some on each side of position 1024 where the tile has both sides."""
    out = check(ctx, monkeypatch, by_name["called_%d" % T])
    called = np.nonzero(out["results"]["called"])[0]
    print("called positions:", called.tolist())
    assert len(called) and called.min() < 1024
    if T > 1024:
        assert called.max() >= 1024


def test_label_writes_of_the_write_pass(ctx, by_name):
    """n_groups = 5: the write pass leaves every observation's group in obs_label; the group records must be those of bvc_lrt_csr_groups
    on the restated parser's columns.  sample0 is shifted by 3, so the last three samples lie beyond the label vector: in no group."""
    beyond = ran = 0
    for name in ("base_lengths", "step_edges", "counters", "indel_sources", "called_1025"):
        c = by_name[name]
        text, ls = S.layout(c.batch_lines, c.align)
        n = int(c.n_in_batch.sum())
        labels = (np.arange(n) * 7 % 6).astype(np.uint8)               # 5 = n_groups: "in no group", as 255
        labels[::13] = 255
        out = ctx.pileup_tile(text, ls, S.sample0_of(c.n_in_batch) + 3, c.n_in_batch, c.ref, MIN_AF, carry_in=c.carry_in,
                              group_of_sample=labels, n_groups=5)
        assert out is not None, name
        cols = r5.reference_columns(c.batch_lines, S.parser_for(c))
        offs, bb, qq, ss = [0], [], [], []
        for aiv, sample in cols:
            for a, j in zip(aiv, sample):
                if not a["is_indel"]:
                    bb.append(a["base"]); qq.append(a["qual"]); ss.append(j + 3)
            offs.append(len(bb))
        beyond += sum(j >= n for j in ss)
        res, gres = ctx.lrt_csr_groups(np.array(offs, np.int64), np.array(bb, np.int8), np.array(qq, np.uint8).astype(np.int8),
                                       np.array(ss, np.int32), c.ref, MIN_AF, labels, 5)
        assert out["results"].tobytes() == res.tobytes() and out["grp_results"].tobytes() == gres.tobytes(), name
        ran += int(gres["ran"].sum())
    assert beyond > 0 and ran > 0


def test_irregular_tiles_are_reported_beside_their_regular_twins(ctx, by_name):
    """Everything tests/test_gpu_round5.py's test of irregular lines holds, with the byte that spoils the line on the first and last byte
    of a lane, of a step, in the second step, and on a token across the step edge: None, the twin accepted, and a regular tile accepted
    afterwards on the same context."""
    wrong = []
    for bad, twin in S.irregular():
        if tile(ctx, bad) is not None:
            wrong.append(bad.name + " accepted")
        if tile(ctx, twin) is None:
            wrong.append(twin.name + " reported")
    assert not wrong, wrong
    assert tile(ctx, by_name["indel_sources"]) is not None


def test_large_tile_second_trip_of_the_line_loop(ctx):
    """5 x 52,500 one-sample lines = 262,500 lines: the parse kernel's 65,536 workgroups of 4 lines make a second trip, the per-wavefront
    LDS tally must be zero again between lines of different positions.  Compared with vectorised numpy (tests/pileup_lines.py, held
    against the strict split on the CPU)."""
    c = S.large()
    x = S.large_expected()
    text, ls = S.layout(c.batch_lines, c.align)
    assert ls.shape[0] * (ls.shape[1] - 1) > M.TRIP_LINES
    out = tile(ctx, c)
    assert out is not None
    for k in ("base", "mapq", "qual", "rpr", "strand", "is_indel"):
        assert np.array_equal(out["entries"][k].astype(np.int64), x[k]), k
    assert np.array_equal(out["samples"], x["samples"]) and np.array_equal(out["entry_off"], x["entry_off"])
    assert np.array_equal(out["tally"], x["tally"]) and out["carry_out"] == x["carry_out"]
    ind = out["indels"]
    assert np.array_equal(ind["entry"], np.nonzero(x["is_indel"])[0]) and (ind["len"] == 1).all()
    assert (np.frombuffer(text, dtype=np.uint8)[ind["text_off"]] == ord("N")).all()
    want = ctx.lrt_csr(x["obs_off"], x["obs_base"], x["obs_qual"], c.ref, MIN_AF)
    assert out["results"].tobytes() == want.tobytes()
    co = tile(ctx, c, called_only=True)
    for key in ("entry_off", "tally", "results", "indels"):
        assert co[key].tobytes() == out[key].tobytes(), key
    n_t = np.diff(out["entry_off"]) * (out["results"]["called"] != 0)
    assert np.array_equal(co["called_off"], np.concatenate([[0], np.cumsum(n_t)]))
    keep = np.repeat(out["results"]["called"] != 0, np.diff(out["entry_off"]))
    assert co["entries"].tobytes() == out["entries"][keep].tobytes() and np.array_equal(co["samples"], out["samples"][keep])


@pytest.mark.parametrize("feed", S.feeds(), ids=lambda f: f.name)
def test_compressed_tiles_with_their_segment_edges_where_intended(ctx, feed):
    """bvc_pileup_begin_bgzf with blocks cut where the catalogue says (inside a token, on a newline): newlines on bytes 1023, 1024 and
    1025 of a region, regions that start at every % 16, a partial line of more than 1 KiB carried into the next tile, a region of more
    than 64 segments beside regions of a few bytes and an empty one, a batch without a new block, max_positions one less than, equal to
    and one more than the whole lines there are.  The model says how many positions every call must find."""
    streams = S.feed_streams(feed)
    nb = len(streams)
    sample0 = S.sample0_of(feed.n_in_batch)
    _, Ts = M.region_census(streams, feed.skip, feed.calls)
    sent, parser, carry, done, first = [0] * nb, eo.Parser(), [0] * 5, 0, True
    for (pieces, max_pos), T_want in zip(feed.calls, Ts):
        comp, blocks, bob = bytearray(), [], []
        for b in range(nb):
            for n in pieces[b]:
                chunk = streams[b][sent[b]:sent[b] + n]
                sent[b] += n
                co = zlib.compressobj(6, zlib.DEFLATED, -15)
                z = co.compress(chunk) + co.flush()
                blocks.append((len(comp), len(z), len(chunk)))
                comp += z
            bob.append(len(pieces[b]))
        r = ctx.pileup_begin_bgzf(bytes(comp), blocks, bob, feed.skip if first else None, sample0, feed.n_in_batch, max_pos, first)
        first = False
        assert r["rc"] == 0, (feed.name, r)
        T = r["T"]
        assert T == T_want, (feed.name, done, r)
        if T == 0:
            continue
        ref = np.zeros(T, dtype=np.int8)
        out = ctx._pileup_finish(T, r["n_entries"], r["n_indels"], r["indel_text_bytes"], ref, MIN_AF, carry, None, 0)
        cols = [parser.parse([feed.batch_lines[b][done + t] for b in range(nb)]) for t in range(T)]
        r5._columns_check(out, cols, ref, MIN_AF, ctx, "%s positions %d..%d" % (feed.name, done, done + T))
        ai = parser.ai
        assert out["carry_out"] == [ai["base"], ai["mapq"], ai["qual"], ai["rpr"], ai["strand"]]
        carry = out["carry_out"]
        done += T
    assert done == len(feed.batch_lines[0]) and all(sent[b] == len(streams[b]) for b in range(nb))
    r = ctx.pileup_begin_bgzf(b"", [], [0] * nb, None, sample0, feed.n_in_batch, 10, False)
    assert r["rc"] == 0 and r["T"] == 0 and r["lines"].tolist() == [0] * nb
