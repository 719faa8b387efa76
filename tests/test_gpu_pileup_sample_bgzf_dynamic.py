"""bvc_pileup_sample_bgzf with tuning key "bgzf_codes" at 1 (GPU): on one small tile of tests/test_gpu_pileup_sample_bgzf.py each called
position's blocks walk clean and inflate to the bytes bvc_pileup_sample_text returns, they are not larger than the blocks the same call
gives at key 0, and the call may be repeated and follow its twin."""
import numpy as np
import pytest

from tests.test_gpu_pileup_bin import encode, fuzz_tiles, sample0_of
from tests.test_gpu_pileup_sample_bgzf import GUARD, check_blocks, comp_need, text_of

pytestmark = pytest.mark.gpu


def test_the_blocks_at_key_1_inflate_to_the_text_and_are_not_larger():
    from basevarc_amd import Context
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
        for key in (0, 1, 1):                                             # (the key acts from the next call on; the last one repeats)
            ctx.set_tuning("bgzf_codes", key)
            want, want_ln = text_of(ctx, T, n, out)                       # the twin first
            comp = np.full(need + 32, GUARD, dtype=np.uint8)
            comp, off, ln = ctx.pileup_sample_bgzf(T, n, comp, comp_cap=need)
            assert check_blocks(T, out, want, comp, off, ln, want_ln, f"key {key}") > 0
            assert (comp[int(off[T]):] == GUARD).all()
            if key in got:
                assert (off == got[key][1]).all() and comp[:int(off[T])].tobytes() == got[key][0][:int(off[T])].tobytes()
            got[key] = (comp, off)
    off0, off1 = got[0][1], got[1][1]
    sizes0, sizes1 = np.diff(off0), np.diff(off1)
    print(f"bytes of the called positions' blocks: key 0 {int(off0[T])}, key 1 {int(off1[T])}")
    assert (sizes1 <= sizes0).all() and int(off1[T]) <= int(off0[T])
