"""The sample columns behind the producer calls as BGZF blocks (bvc_pileup_sample_bgzf; GPU).  On the tiles tests/
test_gpu_pileup_sample_text.py builds, each called position's blocks walk clean (tests/bgzf_blocks.py) and inflate to exactly the
bytes bvc_pileup_sample_text returns for the same tile; a position that is not called has an empty range; the two calls work in either
order and repeated; a short buffer consumes nothing; out of sequence the call is refused."""
import numpy as np
import pytest

from tests import bgzf_blocks as bb
from tests.test_gpu_pileup_bin import encode, fuzz_tiles, sample0_of
from tests.test_gpu_round5 import tile_of

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
GUARD = 0xA7


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def comp_need(n, out):
    from basevarc_amd.lib import bgzf_bound, vcf_samples_slot
    eoff, res = out["entry_off"], out["results"]
    return sum(bgzf_bound(vcf_samples_slot(n, int(eoff[t + 1] - eoff[t]))) for t in range(len(res)) if int(res[t]["called"]))


def text_of(ctx, T, n, out):
    from basevarc_amd.lib import vcf_samples_need
    need = vcf_samples_need(n, out["entry_off"], out["results"])
    text, off, ln = ctx.pileup_sample_text(T, n, np.zeros(max(1, need), dtype=np.uint8))
    return [text[int(off[t]):int(off[t]) + int(ln[t])].tobytes() for t in range(T)], ln


def check_blocks(T, out, want, comp, off, ln, want_ln, where):
    assert int(off[0]) == 0 and [int(x) for x in ln] == [int(x) for x in want_ln], where
    called = 0
    for t in range(T):
        piece = comp[int(off[t]):int(off[t + 1])].tobytes()
        if not int(out["results"][t]["called"]):
            assert piece == b"" and want[t] == b"", (where, t)
            continue
        bb.walk_piece(piece, want[t])
        called += 1
    return called


@pytest.mark.parametrize("form,first", [("text", "text"), ("bin", "bgzf")])
def test_blocks_inflate_to_the_text_in_either_order_and_repeated(ctx, form, first):
    n_in_batch, tiles = fuzz_tiles("wide_text" if form == "text" else "wide")
    n = int(n_in_batch.sum())
    s0 = sample0_of(n_in_batch)
    carry, called = [0, 0, 0, 0, 0], 0
    for i, (batch_tokens, ref) in enumerate(tiles):
        lines, records, rs, _ = encode(batch_tokens)
        if form == "text":
            text, ls = tile_of(lines)
            out = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, sample_text=True)
        else:
            out = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, sample_text=True)
        T = len(ref)
        need = comp_need(n, out)
        if first == "text":
            want, want_ln = text_of(ctx, T, n, out)
        comp = np.full(need + 32, GUARD, dtype=np.uint8)
        comp, off, ln = ctx.pileup_sample_bgzf(T, n, comp, comp_cap=need)
        if first != "text":
            want, want_ln = text_of(ctx, T, n, out)
        where = f"{form} tile {i}"
        called += check_blocks(T, out, want, comp, off, ln, want_ln, where)
        assert (comp[int(off[T]):] == GUARD).all(), where
        # again: the same bytes
        comp2, off2, ln2 = ctx.pileup_sample_bgzf(T, n, np.zeros(need + 32, dtype=np.uint8), comp_cap=need)
        assert (off2 == off).all() and comp2[:int(off[T])].tobytes() == comp[:int(off[T])].tobytes(), where
        carry = out["carry_out"]
    assert called > 0


def test_calls_out_of_place_and_short_buffers_are_refused(ctx):
    from basevarc_amd.lib import BvcError
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
    # a finish that is not finish_called_text leaves nothing to deflate
    ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, called_only=True, stats=True)
    refused(lambda: ctx.pileup_sample_bgzf(T, n, buf))
    out = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, sample_text=True)
    need = comp_need(n, out)
    assert need > 64
    # a short buffer: refused with the need named, nothing written, nothing consumed
    big = np.full(need + 48, GUARD, dtype=np.uint8)
    assert str(need) in refused(lambda: ctx.pileup_sample_bgzf(T, n, big, comp_cap=need - 1))
    assert (big == GUARD).all()
    refused(lambda: ctx.pileup_sample_bgzf(T, -1, big))
    want, want_ln = text_of(ctx, T, n, out)
    comp, off, ln = ctx.pileup_sample_bgzf(T, n, big, comp_cap=need)
    assert check_blocks(T, out, want, comp, off, ln, want_ln, "after a short buffer") > 0
    # the next begin ends it
    r = ctx._pileup_begin(ctx._L.bvc_pileup_begin_bin, records, np.ascontiguousarray(rs, dtype=np.uint32), s0, n_in_batch)
    assert r[0] == 0
    refused(lambda: ctx.pileup_sample_bgzf(T, n, big))
    ctx._pileup_finish(r[1], r[2], r[3], 0, ref, 0.001, (0, 0, 0, 0, 0), None, 0, called_only=True)
    refused(lambda: ctx.pileup_sample_bgzf(T, n, big))
