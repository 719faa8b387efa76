"""Temp batches kept on the device (include/bvc_store.h; bvc_store.hip, store_kernel.hip; GPU).

1. Kept bytes: bvc_bam_pileup_bgzf_store then bvc_store_get gives bvc_bam_pileup_bgzf's records and rec_start byte for byte, with its
   statuses and return code, for the catalogue of tests/bam_pileup_cases.py and the 100 test BAMs; after every failure nothing is kept.
2. Tiles: bvc_pileup_begin_store of batches that were put, against bvc_pileup_begin_bin on the host-sliced concatenation of the same
   positions in another context -- every array the finish calls deliver -- and, through bvc_pileup_text, against the model of the tile
   buffer (tests/store_model.py): every slice where the model puts it, the table row for row.
3. The shapes that send the gather kernel down every path.  4. Puts from four threads.  5. The refusals.  6. No allocation in a second
   call of the same shape.
(Guard bytes behind the tile buffer's used part cannot be read back through the ABI -- bvc_pileup_text delivers the used part -- so that
check of the issue is left out; the model comparison covers every byte in use, pads excluded.)"""
import threading
import zlib

import numpy as np
import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import store_model as sm

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ALLOC, ERR_DATA = -1, -4, -5
MIN_AF = 0.001


@pytest.fixture(scope="module")
def ctxs():
    from basevarc_amd import Context
    cs = [Context(0) for _ in range(2)]
    yield cs
    for c in cs:
        c.close()


def new_store(n_positions, n_batches, budget=0):
    from basevarc_amd import Store
    return Store(0, n_positions, n_batches, budget)


def filled(ctx, batches, n_in, order=None):
    """A sealed store of batches = [(records, rec_start)] with n_in[b] samples each."""
    st = new_store(len(batches[0][1]) - 1, len(batches))
    for b in (order if order is not None else range(len(batches))):
        st.put(ctx, b, n_in[b], batches[b][0], batches[b][1])
    st.seal(ctx)
    return st


def sample0_of(n_in):
    return np.concatenate([[0], np.cumsum(n_in)[:-1]]).astype(np.int32)


def check_layout(ctx, st, batches, t0, T, where):
    """After a begin_store of (t0, T) on ctx: the tile buffer and its table against the model."""
    text, rows = ctx.pileup_text(len(batches), T)
    places, want_rows, used = sm.gathered(batches, t0, T)
    assert len(text) == used, (where, len(text), used)
    assert (rows == want_rows).all(), where
    for b, (dst, data) in enumerate(places):
        assert text[dst:dst + len(data)] == data, (where, b)


def indel_texts(out, data):
    """{entry: text} of a finish call's indel records, their text_off read in `data`."""
    return {int(r["entry"]): data[int(r["text_off"]):int(r["text_off"]) + int(r["len"])] for r in out["indels"]}


def check_two_ways(ctxs, st, batches, n_in, t0, T, n_groups, called, where, layout=True):
    """The tile (t0, T) through the store in one context and through bvc_pileup_begin_bin in the other: everything equal."""
    a, b = ctxs
    rng = np.random.default_rng(t0 * 1000 + T)
    ref = rng.integers(0, 4, size=T).astype(np.int8)
    n_samples = int(sum(n_in))
    groups = (np.arange(n_samples) % (n_groups + 1)).astype(np.uint8) if n_groups else None      # (label n_groups: in no group)
    carry = (2, 31, 17, 5, 1)
    kw = dict(carry_in=carry, group_of_sample=groups, n_groups=n_groups, called_only=called, stats=called)
    got = a.pileup_tile_store(st, t0, T, ref, MIN_AF, **kw)
    if layout:
        check_layout(a, st, batches, t0, T, where)
    data, rows = sm.sliced(batches, t0, T)
    want = b.pileup_tile_bin(data, rows, sample0_of(n_in), np.asarray(n_in, dtype=np.int32), ref, MIN_AF, **kw)
    for k in ("entry_off", "tally", "entries", "samples", "results", "carry_out") + (("called_off", "stats") if called else ()) + (("grp_results",) if n_groups else ()):
        g, w = got[k], want[k]
        assert (g.tobytes() == w.tobytes()) if hasattr(g, "tobytes") else (g == w), (where, k)
    gi, wi = got["indels"], want["indels"]
    assert len(gi) == len(wi) and gi["entry"].tolist() == wi["entry"].tolist() and gi["len"].tolist() == wi["len"].tolist(), where
    assert indel_texts(got, got["indel_text"]) == indel_texts(want, data), where
    return got


# ---- 1. kept bytes --------------------------------------------------------------------------------------------------------------------
def bgzf_of(bam):
    """bam as BGZF payloads of at most 65280 bytes: (comp uint8, BLOCK_DTYPE table with the CRC32 checked)."""
    from basevarc_amd import lib as bl
    comp, table = bytearray(), []
    for at in range(0, len(bam), 65280):
        piece = bam[at:at + 65280]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        c = z.compress(piece) + z.flush()
        table.append((len(comp), at, len(c), len(piece), zlib.crc32(piece), 1))
        comp += c
        comp += b"\0" * (-len(comp) % 4)
    return np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8), np.array(table, dtype=bl.BLOCK_DTYPE) if table else np.zeros(0, dtype=bl.BLOCK_DTYPE)


def both_calls(ctx, st, batch, args):
    """(rc, status, need, records, rec_start) of bvc_bam_pileup_bgzf and of the _store call with bvc_store_get behind it."""
    from basevarc_amd.lib import BvcError
    out = []
    for stored in (False, True):
        try:
            if stored:
                rc, status, need = ctx.bam_pileup_bgzf_store(*args, st, batch)
                rec, rs = st.get(ctx, batch) if rc == 0 else (None, None)
            else:
                rc, rec, rs, status, need = ctx.bam_pileup_bgzf(*args)
                rec = rec.tobytes() if rc == 0 else None
        except BvcError as e:
            rc, status, need, rec, rs = e.status, None, 0, None, None
        out.append((rc, status, need, rec, rs))
    return out


def test_the_catalogue_batches_are_kept_byte_for_byte_and_failures_keep_nothing(ctxs):
    ctx = ctxs[0]
    seen = set()
    for c in bc.catalogue():
        bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
        comp, tab = bgzf_of(bam)
        args = (comp, tab, len(bam), off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], c["positions"], c["rg_s"],
                np.frombuffer(c["refseq"].encode(), dtype=np.uint8))
        st = new_store(len(c["positions"]), 2)
        (rc0, st0, need0, rec0, rs0), (rc1, st1, need1, rec1, rs1) = both_calls(ctx, st, 1, args)
        exp = bc.expected(c)
        assert rc0 == rc1 == exp["rc"], (c["name"], rc0, rc1, exp["rc"])
        n = len(c["samples"])
        if rc0 != ERR_DATA:
            assert list(st0[:n]) == list(st1[:n]) == exp["status"], c["name"]
        seen.add((rc0, tuple(sorted(set(exp["status"]) & {2, 3, 4}))))
        if rc0 == 0:
            assert need0 == need1 == len(rec0) and rec1 == rec0 == exp["records"] and list(rs1) == list(rs0[:len(rs1)]) == exp["rec_start"], c["name"]
            assert st.bytes()[0] == sm.row_bytes(len(c["positions"])) + (len(rec0) or 16), c["name"]
        else:
            assert need1 == 0 and st.bytes()[0] == 0, c["name"]
            with pytest.raises(Exception):
                st.get(ctx, 1)
        st.close()
    rcs = {rc for rc, _ in seen}
    assert rcs == {0, bm.BAM_MORE, ERR_DATA} and any(3 in s for _, s in seen) and any(4 in s for _, s in seen), seen


def test_the_test_bams_are_kept_byte_for_byte_and_a_damaged_block_keeps_nothing(ctxs):
    import os
    from basevarc_amd import lib as bl
    from basevarc_amd.lib import BvcError
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    from tests.test_gpu_bam_pileup import bgzf_blocks_of
    ctx = ctxs[0]
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    pv = pv[::13]
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
    tab = np.array(table, dtype=bl.BLOCK_DTYPE)
    rid = [refs.index(contig) for _, _, refs in data]
    eof = np.ones(len(data), dtype=np.uint8)
    ref = np.frombuffer(refseq.encode(), dtype=np.uint8)
    comp = np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8)
    args = lambda comp, tab, end, eof: (comp, tab, out_at, off, end, eof, rid, beg0, end0, mapq, pv, rg_s, ref)
    st = new_store(len(pv), 1)
    (rc0, st0, need0, rec0, rs0), (rc1, st1, need1, rec1, rs1) = both_calls(ctx, st, 0, args(comp, tab, end, eof))
    assert rc0 == rc1 == 0 and need0 == need1 == len(rec0) > 100000 and rec1 == rec0 and list(rs1) == list(rs0) and list(st0) == list(st1)
    assert st.bytes()[0] == sm.row_bytes(len(pv)) + len(rec0)
    st.close()
    # one payload byte of a block in the middle flipped; a sample cut short without its end of file: the codes of the plain call, nothing kept
    k = len(tab) // 2
    bad = comp.copy()
    bad[int(tab[k]["comp_off"]) + int(tab[k]["comp_len"]) // 2] ^= 0x5A
    short_end, short_eof = list(end), eof.copy()
    short_end[3], short_eof[3] = off[3] + 5000, 0
    for a, want_rc in ((args(bad, tab, end, eof), ERR_DATA), (args(comp, tab, short_end, short_eof), bm.BAM_MORE)):
        st = new_store(len(pv), 1)
        (rc0, _, _, _, _), (rc1, st1, need1, _, _) = both_calls(ctx, st, 0, a)
        assert rc0 == rc1 == want_rc and need1 == 0 and st.bytes()[0] == 0
        if want_rc == bm.BAM_MORE:
            assert st1[3] == 2
        with pytest.raises(BvcError):
            st.seal(ctx)
        st.close()


# ---- 2. tiles equal the staged call ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_batches():
    rng = np.random.default_rng(20261020)
    n_in = [3, 1, 7, 4, 2]
    return [sm.random_batch(rng, n, 9, density=0.6, indel_rate=0.15, filler=int(rng.integers(0, 40))) for n in n_in], n_in


@pytest.mark.parametrize("n_groups, called", [(0, False), (5, False), (0, True), (5, True)])
def test_every_tile_of_a_small_grid_equals_the_staged_call(ctxs, grid_batches, n_groups, called):
    batches, n_in = grid_batches
    st = filled(ctxs[0], batches, n_in)
    P = 9
    n_indels = 0
    for t0 in range(P):
        for T in range(1, P - t0 + 1):
            if (t0 + T) % 2 and T not in (1, P) and t0 + T != P:
                continue                                         # (half of the inner tiles; both ends and both extremes of T always)
            n_indels += len(check_two_ways(ctxs, st, batches, n_in, t0, T, n_groups, called, (t0, T))["indels"])
    assert n_indels > 20
    cum = sm.cum_of([rs for _, rs in batches])
    for t0, mp, mb in ((0, P, 1 << 30), (0, P, 300), (3, 4, 500), (P - 1, P, 0), (2, P, int(cum[6] - cum[2]) + 80), (2, P, int(cum[6] - cum[2]) + 79)):
        assert st.tile(t0, mp, mb) == sm.tile(cum, len(batches), t0, mp, mb), (t0, mp, mb)
    st.close()


# ---- 3. the shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_batches", [1, 2, 63, 64, 65, 1025])
def test_batch_counts_around_a_wavefront_and_past_the_grid_cap(ctxs, n_batches):
    """1025 batches: more work items than the launcher's grid holds workgroups (every batch's slice is at least one item), and a second
    round of the plan kernel's walk."""
    from basevarc_amd import lib as bl
    rng = np.random.default_rng(n_batches)
    P = 5
    n_in = [int(rng.integers(1, 4)) for _ in range(n_batches)]
    batches = [sm.random_batch(rng, n, P, density=0.5, indel_rate=0.2, filler=int(rng.integers(0, 16))) for n in n_in]
    if n_batches > 2:
        batches[1] = sm.batch_of([sm.record([])] * P, filler=3)                  # a slice of all-empty records: 4 * T bytes
    if n_batches == 1025:
        assert n_batches > bl.STORE_GRID
    st = filled(ctxs[0], batches, n_in)
    for t0, T in ((0, P), (0, 1), (P - 1, 1), (1, 3)):
        check_two_ways(ctxs, st, batches, n_in, t0, T, 5 if n_batches == 65 else 0, n_batches == 64, (n_batches, t0, T))
    st.close()


def test_slices_around_the_chunk_size_at_every_alignment(ctxs):
    """One position a batch whose record makes the slice CHUNK - 1, CHUNK, CHUNK + 1 and 3 * CHUNK + 5 bytes; the same sizes again behind
    fillers that put the slice's start at each of the 16 alignments; an indel text of 0xffff bytes across chunk edges; a second, short
    position so that t0 = 1 starts every slice somewhere else."""
    from basevarc_amd import lib as bl
    rng = np.random.default_rng(16384)
    CH = bl.STORE_CHUNK
    sizes = [CH - 1, CH, CH + 1, 3 * CH + 5]
    batches, n_in = [], []
    for f in range(16):
        rec, n = sm.sized_record(rng, sizes[f % 4] if f else CH)              # (filler 0 with exactly a chunk: no head, no tail)
        batches.append(sm.batch_of([rec, sm.record([(0, sm.base_entry(rng))])], filler=f))
        n_in.append(n)
        assert int(batches[-1][1][1]) - int(batches[-1][1][0]) == (sizes[f % 4] if f else CH)
    for size in sizes:                                                         # and each size from an aligned start
        rec, n = sm.sized_record(rng, size)
        batches.append(sm.batch_of([rec, sm.record([])]))
        n_in.append(n)
    rec, n = sm.sized_record(rng, 2 * CH, indel_at=CH - 100, indel_text=0xffff)
    assert len(rec) > 5 * CH - 200
    batches.append(sm.batch_of([rec, sm.record([(1, sm.base_entry(rng))])], filler=7))
    n_in.append(n)
    st = filled(ctxs[0], batches, n_in)
    for t0, T in ((0, 1), (0, 2), (1, 1)):
        got = check_two_ways(ctxs, st, batches, n_in, t0, T, 0, False, (t0, T))
        if t0 == 0:
            assert max(got["indels"]["len"]) == 0xffff
    st.close()


# ---- 4. concurrency -------------------------------------------------------------------------------------------------------------------
def test_four_threads_put_sixteen_batches_in_scrambled_order(ctxs):
    from basevarc_amd import Context
    rng = np.random.default_rng(4)
    P, nb = 12, 16
    n_in = [int(rng.integers(1, 6)) for _ in range(nb)]
    batches = [sm.random_batch(rng, n, P, density=0.7, filler=int(rng.integers(0, 16))) for n in n_in]
    st = new_store(P, nb)
    order = [int(x) for x in rng.permutation(nb)]
    errors = []

    def work(k):
        try:
            with Context(0) as c:
                for b in order[k::4]:
                    st.put(c, b, n_in[b], batches[b][0], batches[b][1])
        except Exception as e:                                   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    st.seal(ctxs[0])
    in_order = filled(ctxs[1], batches, n_in)
    assert st.bytes() == in_order.bytes()
    cum = sm.cum_of([rs for _, rs in batches])
    for t0, T in ((0, P), (3, 5), (P - 1, 1)):
        assert st.tile(t0, P, 1 << 30) == in_order.tile(t0, P, 1 << 30) == sm.tile(cum, nb, t0, P, 1 << 30)
        ref = np.zeros(T, dtype=np.int8)
        a = ctxs[0].pileup_tile_store(st, t0, T, ref, MIN_AF)
        ta = ctxs[0].pileup_text(nb, T)
        b = ctxs[1].pileup_tile_store(in_order, t0, T, ref, MIN_AF)
        tb = ctxs[1].pileup_text(nb, T)
        # the same table and as many bytes in use; the slices' bytes below, against the model (the pad bytes between them belong to nobody)
        assert len(ta[0]) == len(tb[0]) and (ta[1] == tb[1]).all()
        check_layout(ctxs[1], in_order, batches, t0, T, ("in order", t0, T))
        for k in ("entry_off", "tally", "entries", "samples", "results"):
            assert a[k].tobytes() == b[k].tobytes(), k
        # (where a token's text lies in indel_text is the gathering kernel's choice: the records are compared through it)
        assert a["indels"]["entry"].tolist() == b["indels"]["entry"].tolist() and indel_texts(a, a["indel_text"]) == indel_texts(b, b["indel_text"])
        check_layout(ctxs[0], st, batches, t0, T, (t0, T))
    for b in range(nb):
        assert st.get(ctxs[0], b)[0] == batches[b][0] and (st.get(ctxs[0], b)[1] == batches[b][1]).all()
    st.close()
    in_order.close()


# ---- 5. the refusals ------------------------------------------------------------------------------------------------------------------
def test_the_refusals_leave_the_store_and_the_context_usable(ctxs):
    import ctypes as C
    from basevarc_amd.lib import BvcError
    ctx = ctxs[0]
    rng = np.random.default_rng(5)
    P = 6
    n_in = [2, 3, 4]
    batches = [sm.random_batch(rng, n, P, density=0.8, indel_rate=0.3) for n in n_in]
    st = new_store(P, 3)

    def refused(code, match, fn):
        with pytest.raises(BvcError, match=match) as e:
            fn()
        assert e.value.status == code

    def good_tile(store=None):
        s = store if store is not None else good
        check_two_ways(ctxs, s, batches, n_in, 1, 4, 0, False, "good tile", layout=False)
    good = filled(ctx, batches, n_in)
    st.put(ctx, 0, n_in[0], *batches[0])
    refused(ERR_ARG, "sealed", lambda: ctx.pileup_begin_store(st, 0, 1))                      # begin before seal
    good_tile()
    with pytest.raises(ValueError):
        st.tile(0, 1, 100)                                                                    # (tile before seal too)
    refused(ERR_ARG, "put already", lambda: st.put(ctx, 0, n_in[0], *batches[0]))             # double put
    refused(ERR_ARG, "outside the store", lambda: st.put(ctx, 3, 1, *batches[1]))
    refused(ERR_ARG, "outside the store", lambda: st.put(ctx, -1, 1, *batches[1]))
    refused(ERR_ARG, "batch 1 has not been put", lambda: st.seal(ctx))                        # a batch missing: named
    good_tile()
    # a rec_start that disagrees with a length word; one that leaves the records
    rs = batches[1][1].copy()
    k = next(t for t in range(P) if rs[t + 1] - rs[t] > 4)
    rs[k + 1:] += 1
    refused(ERR_ARG, "length word", lambda: st.put(ctx, 1, n_in[1], batches[1][0] + b"\0", rs))
    rs = batches[1][1].copy()
    rs[P] += 8
    refused(ERR_ARG, "rec_start", lambda: st.put(ctx, 1, n_in[1], batches[1][0], rs))
    assert st.bytes()[0] == sm.row_bytes(P) + len(batches[0][0])
    st.put(ctx, 1, n_in[1], *batches[1])
    st.put(ctx, 2, n_in[2], *batches[2])
    st.seal(ctx)
    refused(ERR_ARG, "sealed", lambda: st.put(ctx, 2, n_in[2], *batches[2]))                  # put after seal
    refused(ERR_ARG, "outside the store", lambda: ctx.pileup_begin_store(st, 3, 4))
    refused(ERR_ARG, "outside the store", lambda: ctx.pileup_begin_store(st, -1, 2))
    good_tile(st)
    # finish without indel_text: the tile's text is on the device only
    ne, ni, nt = ctx.pileup_begin_store(st, 0, P)
    assert ni > 0 and nt > 0
    refused(ERR_ARG, "indel_text", lambda: ctx._pileup_finish(P, ne, ni, 0, np.zeros(P, dtype=np.int8), MIN_AF, (0, 0, 0, 0, 0), None, 0))
    good_tile(st)
    st.close()
    # the budget: a put over it names both numbers and keeps nothing; a smaller one then succeeds
    need = [sm.row_bytes(P) + len(r) for r, _ in batches]
    small, big = (0, 2) if need[0] < need[2] else (2, 0)
    st = new_store(P, 3, budget=need[big] - 1)
    refused(ERR_ALLOC, f"{need[big] - 1} bytes.*{need[big]}", lambda: st.put(ctx, big, n_in[big], *batches[big]))
    assert st.bytes() == (0, need[big] - 1)
    st.put(ctx, small, n_in[small], *batches[small])
    assert st.bytes()[0] == need[small] and st.get(ctx, small)[0] == batches[small][0]
    st.close()
    good_tile()
    good.close()


def test_a_tile_over_the_32_bit_limit_is_refused_from_the_cumulative_sizes_alone(ctxs):
    """Five batches of one position, each a record of 0x34000000 bytes (only its length word is ever looked at by a put): together
    they pass 0xFFFFFF00, bvc_store_tile reports the one position a tile always has with its bytes, and bvc_pileup_begin_store refuses it
    before anything is launched.  A tile of the first batch's store alone still runs."""
    from basevarc_amd.lib import BvcError
    ctx = ctxs[0]
    size = 0x34000000
    rec = np.zeros(size, dtype=np.uint8)
    rec[:4] = np.frombuffer(np.uint32(size - 4).tobytes(), dtype=np.uint8)
    rs = np.array([0, size], dtype=np.uint32)
    st = new_store(1, 5)
    for b in range(5):
        st.put(ctx, b, 1, rec, rs)
    st.seal(ctx)
    assert 5 * size + 80 > sm.LIMIT and st.tile(0, 1, 1 << 20) == (1, 5 * size + 80)
    with pytest.raises(BvcError, match="use fewer positions") as e:
        ctx.pileup_begin_store(st, 0, 1)
    assert e.value.status == ERR_ARG
    st.close()
    small = sm.batch_of([sm.record([(0, sm.base_entry(np.random.default_rng(1)))])])
    st = filled(ctx, [small], [1])
    assert ctx.pileup_begin_store(st, 0, 1)[0] == 1
    st.close()


# ---- 6. no allocation ---------------------------------------------------------------------------------------------------------------
def test_a_second_begin_of_the_same_shape_allocates_nothing(ctxs):
    import torch
    ctx = ctxs[0]
    rng = np.random.default_rng(6)
    P, nb = 300, 40
    n_in = [3] * nb
    batches = [sm.random_batch(rng, 3, P, density=0.5) for _ in range(nb)]
    st = filled(ctx, batches, n_in)
    ref = np.zeros(P, dtype=np.int8)
    free, outs = [], []
    torch.cuda.mem_get_info()                                    # (whatever the first look itself brings up is up before the two that count)
    for _ in range(2):
        outs.append(ctx.pileup_tile_store(st, 0, P, ref, MIN_AF))
        ctx.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    # the library allocates device memory of its own (not torch's pool): what is free on the device after the first call stays free
    assert free[1] == free[0], free
    for k in ("entry_off", "tally", "entries", "samples", "results"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    st.close()
