"""The sample columns behind the producer calls (bvc_pileup_finish_called_text + bvc_pileup_sample_text; GPU).

Tiles go through bvc_pileup_begin, _begin_bin and _begin_bgzf on two contexts: one finishes with bvc_pileup_finish_called_stats (the
twin), the other with bvc_pileup_finish_called_text.  Everything both deliver must be the same bytes; the text of the second is compared
with the host program's columns (bvchost_vcf_samples) and the Python model, built from the entries the TWIN downloaded."""
import numpy as np
import pytest

from tests import vcf_samples_cases as vc
from tests.test_gpu_pileup_bin import encode, fuzz_tiles, sample0_of
from tests.test_gpu_round5 import _bgzf_payloads, tile_of

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
GUARD = 0xA7
SAME = ("entry_off", "tally", "indels", "indel_text", "results", "grp_results", "stats", "carry_out")


@pytest.fixture(scope="module")
def pair():
    from basevarc_amd import Context
    a, b = Context(0), Context(0)
    yield a, b
    a.close(); b.close()


@pytest.fixture(scope="module")
def host():
    return vc.host_library()


def groups_of(n, n_groups):
    if not n_groups:
        return dict()
    rng = np.random.default_rng(99)
    group = rng.integers(0, 5, n).astype(np.uint8)
    group[rng.random(n) < 0.1] = 255
    return dict(group_of_sample=group, n_groups=5)


def check_tile(host, ctx, twin, mine, ref, n, where, text_slack=48):
    """twin: the dict of finish_called_stats; mine: the dict of finish_called_text on ctx, whose tile is still resident."""
    from basevarc_amd.lib import vcf_samples_need, vcf_samples_slot
    assert twin is not None and mine is not None, where
    for key in SAME:
        a, b = mine[key], twin[key]
        if key in ("indels", "indel_text") and len(twin["indel_text"]):
            # texts gathered on the device lie in the buffer in any order: the records agree in entry and length, and in the text they name
            assert a is not None and len(mine["indels"]) == len(twin["indels"]), (where, key)
            assert mine["indels"]["entry"].tolist() == twin["indels"]["entry"].tolist(), where
            assert mine["indels"]["len"].tolist() == twin["indels"]["len"].tolist(), where
            texts = [[d["indel_text"][int(r["text_off"]):int(r["text_off"]) + int(r["len"])] for r in d["indels"]] for d in (mine, twin)]
            assert texts[0] == texts[1], where
            continue
        if a is None or b is None:
            assert a is None and b is None, (where, key)
        elif isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, key)
        else:
            assert a == b, (where, key)
    assert len(mine["entries"]) == 0 and len(mine["samples"]) == 0, where
    T = len(ref)
    res, eoff, coff = twin["results"], twin["entry_off"], twin["called_off"]
    need = vcf_samples_need(n, eoff, res)
    text = np.full(need + text_slack, GUARD, dtype=np.uint8)
    text, off, ln = ctx.pileup_sample_text(T, n, text, text_cap=need)
    at = called = 0
    for t in range(T):
        assert int(off[t]) == at, (where, t)
        if not int(res[t]["called"]):
            assert int(ln[t]) == 0, (where, t)
            continue
        e, s = twin["entries"][coff[t]:coff[t + 1]], twin["samples"][coff[t]:coff[t + 1]]
        assert len(e) == eoff[t + 1] - eoff[t]
        want = vc.host_columns(host, n, s, e, int(ref[t]), res[t])
        assert want == vc.model_columns(n, s, e, int(ref[t]), res[t]["n_alt"], res[t]["alt_base"]), (where, t)
        assert int(ln[t]) == len(want), (where, t)
        assert text[at:at + len(want)].tobytes() == want, (where, t)
        at += vcf_samples_slot(n, len(e))
        called += 1
    assert int(off[T]) == at == need and (text[at:] == GUARD).all(), where
    return called


@pytest.mark.parametrize("n_groups", [0, 5])
@pytest.mark.parametrize("form", ["text", "bin", "bgzf"])
def test_three_tiles_through_every_begin_call(pair, host, form, n_groups):
    mine_ctx, twin_ctx = pair
    shape = "wide_text" if form != "bin" else "wide"
    n_in_batch, tiles = fuzz_tiles(shape)
    n = int(n_in_batch.sum())
    kw = groups_of(n, n_groups)
    s0 = sample0_of(n_in_batch)
    carry, called = [0, 0, 0, 0, 0], 0
    rng = np.random.default_rng(7)
    for i, (batch_tokens, ref) in enumerate(tiles):
        lines, records, rs, _ = encode(batch_tokens)
        where = f"{form} groups {n_groups} tile {i}"
        if form == "text":
            text, ls = tile_of(lines)
            twin = twin_ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True, stats=True, **kw)
            mine = mine_ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, sample_text=True, **kw)
        elif form == "bin":
            twin = twin_ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True, stats=True, **kw)
            mine = mine_ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, sample_text=True, **kw)
        else:
            comp, blocks, bob = bytearray(), [], []
            for b in range(len(n_in_batch)):
                data = "".join(l + "\n" for l in lines[b]).encode()
                pl = _bgzf_payloads(data, rng, [65280, 3000, 500])
                for c, isz in pl:
                    blocks.append((len(comp), len(c), isz))
                    comp += c
                bob.append(len(pl))
            outs = []
            for c in (twin_ctx, mine_ctx):
                r = c.pileup_begin_bgzf(bytes(comp), blocks, bob, [0] * len(bob), s0, n_in_batch, 1000, i == 0)
                assert r["rc"] == 0 and r["T"] == len(ref), (where, r)
                g = kw.get("group_of_sample")
                outs.append(c._pileup_finish(r["T"], r["n_entries"], r["n_indels"], r["indel_text_bytes"], ref, 0.001, carry, g, n_groups,
                                             **(dict(called_only=True, stats=True) if c is twin_ctx else dict(sample_text=True))))
            twin, mine = outs
        called += check_tile(host, mine_ctx, twin, mine, ref, n, where)
        carry = twin["carry_out"]
    assert called > 0, (form, n_groups)                            # (the text was asked about real records)


def test_calls_out_of_place_and_short_buffers_are_refused(pair, host):
    from basevarc_amd.lib import BvcError, vcf_samples_need
    ctx, twin_ctx = pair
    n_in_batch, tiles = fuzz_tiles("dense")
    n = int(n_in_batch.sum())
    s0 = sample0_of(n_in_batch)
    batch_tokens, ref = tiles[0]
    lines, records, rs, _ = encode(batch_tokens)
    text, ls = tile_of(lines)
    T = len(ref)
    buf = np.full(64, GUARD, dtype=np.uint8)

    def refused(call):
        with pytest.raises(BvcError) as err:
            call()
        assert err.value.status == BVC_ERR_ARG
        return str(err.value)
    # a finish that is not finish_called_text leaves nothing to format
    ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, called_only=True, stats=True)
    refused(lambda: ctx.pileup_sample_text(T, n, buf))
    twin = twin_ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, called_only=True, stats=True)
    mine = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, sample_text=True)
    need = vcf_samples_need(n, twin["entry_off"], twin["results"])
    assert need > 64
    # a short buffer: refused with the need named, nothing written, nothing consumed -- the larger buffer then gets the text, twice
    big = np.full(need + 48, GUARD, dtype=np.uint8)
    assert str(need) in refused(lambda: ctx.pileup_sample_text(T, n, big, text_cap=need - 1))
    assert (big == GUARD).all()
    refused(lambda: ctx.pileup_sample_text(T, -1, big))
    assert check_tile(host, ctx, twin, mine, ref, n, "after a short buffer") > 0
    assert check_tile(host, ctx, twin, mine, ref, n, "a second time") > 0
    # page-locked text
    addr, pinned = ctx.host_alloc(need + 16)
    try:
        pinned[:] = GUARD
        t2, off, ln = ctx.pileup_sample_text(T, n, pinned, text_cap=need)
        assert t2[:need].tobytes() == ctx.pileup_sample_text(T, n, big, text_cap=need)[0][:need].tobytes() and (t2[need:] == GUARD).all()
    finally:
        ctx.host_free(addr)
    # the next begin ends it, whether or not that tile is finished
    r = ctx._pileup_begin(ctx._L.bvc_pileup_begin_bin, records, np.ascontiguousarray(rs, dtype=np.uint32), s0, n_in_batch)
    assert r[0] == 0
    refused(lambda: ctx.pileup_sample_text(T, n, big))
    out = ctx._pileup_finish(r[1], r[2], r[3], 0, ref, 0.001, (0, 0, 0, 0, 0), None, 0, called_only=True)
    assert out["results"].tobytes() == twin["results"].tobytes()
    refused(lambda: ctx.pileup_sample_text(T, n, big))
