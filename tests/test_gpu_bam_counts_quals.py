"""bvc_bam_counts_quals and the accumulator's third kind on the device (bam_counts_kernel.hip, bvc_bam_counts.hip; GPU), word for word
against the plain model (tests/bam_counts_quals_model.py: the wide call's counts cut to the first n_quals quality columns of each base, the
ninth header's depth rows, sample status 5).

1. Every case of tests/bam_pileup_cases.py with 4, 40, 124 and 128 quality columns and 0, 5 and 32 groups, from host and from device
   pointers: the return code and statuses are the model's, and the arrays -- pre-filled with random words, guard words in front and behind
   -- hold the old words plus the model's, modulo 2^32, after BVC_OK and exactly the old words after anything else (a sample of status 2,
   3, 4 or 5, a bad argument).  One hand-built batch holds the qualities 39, 40, 127, 128 and 255 at 40 columns.
2. The shapes: positions around a wavefront and past the grid's 1024 chunks, samples around a workgroup's four, none of either.
3. Expansion: an accumulator of 128 columns holds a wide one's bytes; bvc_site_acc_get at odd rows into a guarded destination;
   bvc_site_acc_lrt byte for byte a wide accumulator's, also across the boundary of the pieces it expands.
4. The accumulator: four threads' contexts adding into one, a damaged block, a short sample and a quality without a column adding nothing,
   no allocation in a second call."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import bam_counts_model as cm
from tests import bam_counts_quals_model as qm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests.test_gpu_bam_counts import (CATALOGUE, ERR_ALLOC, ERR_ARG, ERR_DATA, GUARD, GUARD_WORD, MIN_AF, TW, acc_args, arrays, bgzf_args, guarded,
                                       span_case, bams100)  # noqa: F401  (bams100: that module's fixture of the 100 test BAMs)
from tests.test_gpu_bam_group_depth import labels_of

pytestmark = pytest.mark.gpu

QUALS = (4, 40, 124, 128)
GROUPS = (0, 5, 32)
EXPAND_ROWS = 32768                              # csrc/bvc_bam_counts.hip, kExpandRows: the rows a call expands at a time


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def model_of(c, n_quals, n_groups=0, labels=None):
    return qm.expected(None, None, None, None, c["positions"], None, None, n_quals, labels, n_groups, exp=bc.expected(c))


def run(ctx, c, device, n_quals, n_groups, labels, exp):
    """One bvc_bam_counts_quals call on guarded, pre-filled arrays.  Returns (rc or the BvcError's status, its message, sample_status with
    its guard, [(buffer, its old words, the model's words or None)] for counts, tally and -- with groups -- depth)."""
    from basevarc_amd.lib import BvcError
    bam, off, end, eof, rid, pos = arrays(c)
    n, P = len(rid), len(pos)
    rng = np.random.default_rng(len(bam) + 7 * P + n_groups + n_quals)
    sizes = (P * 4 * n_quals, P * TW, P * n_groups * 4) if n else (0, 0, 0)
    wants = (exp["counts"], None if exp["tally"] is None else exp["tally"].view(np.uint32), exp["depth"])
    if not n_groups:
        sizes, wants = sizes[:2], wants[:2]
    bufs = [guarded(rng, np.zeros(size, dtype=np.uint32) if w is None else w) for size, w in zip(sizes, wants)]
    status = np.full(n + GUARD, GUARD_WORD, dtype=np.uint32)
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        d_bufs, d_s = [dev(b) for b, _ in bufs], dev(status)
        args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], len(c["refseq"]), n_quals]
        out = [d[GUARD:GUARD + len(pre)] for d, (_, pre) in zip(d_bufs, bufs)]
        kw = dict(group_of_sample=dev(labels) if n_groups else None, n_groups=n_groups, sample_status=d_s)
    else:
        args = [bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"]), n_quals]
        out = [b[GUARD:GUARD + len(pre)] for b, pre in bufs]
        kw = dict(group_of_sample=labels if n_groups else None, n_groups=n_groups, sample_status=status)
    message = ""
    try:
        rc, _ = ctx.bam_counts_quals(*args, *out, **kw)
    except BvcError as e:
        rc, message = e.status, str(e)
    if device:
        ctx.synchronize()
        status = d_s.cpu().numpy().view(np.uint32)
        bufs = [(d.cpu().numpy().view(np.uint32), pre) for d, (_, pre) in zip(d_bufs, bufs)]
    return rc, message, status, [(b, pre, w) for (b, pre), w in zip(bufs, wants)]


def check(c, got, exp, n_quals):
    """What a call left, against the model: old + model (mod 2^32) after BVC_OK, the old words otherwise, the guards as they were; a call
    refused for status 5 alone names the first such sample and n_quals."""
    rc, message, status, bufs = got
    n = len(c["samples"])
    assert rc == exp["rc"], (c["name"], n_quals, rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], n_quals, list(status[:n]), exp["status"])
    assert (status[n:] == GUARD_WORD).all(), c["name"]
    if rc == ERR_DATA and not set(exp["status"]) & {3, 4}:
        assert f"sample {exp['status'].index(5)}:" in message and f"n_quals = {n_quals}" in message, (c["name"], message)
    for which, (buf, pre, want) in zip(("counts", "tally", "depth"), bufs):
        assert (buf[:GUARD] == GUARD_WORD).all() and (buf[GUARD + len(pre):] == GUARD_WORD).all(), (c["name"], n_quals, which)
        body = buf[GUARD:GUARD + len(pre)]
        if rc == bm.OK and want is not None and len(pre):
            w = want.reshape(-1)
            bad = np.flatnonzero(body != pre + w)           # (uint32 arithmetic wraps)
            assert bad.size == 0, (c["name"], n_quals, which, bad[:8], body[bad[:8]], pre[bad[:8]], w[bad[:8]])
        else:
            assert (body == pre).all(), (c["name"], n_quals, which)


def both_forms(ctx, c, n_quals, n_groups=0, labels=None):
    exp = model_of(c, n_quals, n_groups, labels)
    for device in (False, True):
        check(c, run(ctx, c, device, n_quals, n_groups, labels, exp), exp, n_quals)
    return exp


# ---- 1. the catalogue and the quality edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_catalogue_case(ctx, c):
    """The catalogue's default qualities run from 2 to 41: four columns refuse nearly every batch that the existing verdict passes, forty
    some, 124 and 128 none; its samples of status 2, 3 and 4 keep their codes in front of status 5."""
    for k, n_groups in enumerate(GROUPS):
        labels = labels_of(c, n_groups, k) if n_groups else None
        for n_quals in QUALS:
            both_forms(ctx, c, n_quals, n_groups, labels)


def test_the_catalogue_holds_every_verdict_at_every_width():
    seen = {}
    for n_quals in QUALS:
        seen[n_quals] = {(model_of(c, n_quals)["rc"], s) for c in CATALOGUE for s in set(model_of(c, n_quals)["status"])}
    for n_quals in (4, 40):
        assert {(bm.OK, 0), (ERR_DATA, 5), (ERR_DATA, 4), (ERR_DATA, 3), (bm.BAM_MORE, 2)} <= seen[n_quals], (n_quals, seen[n_quals])
    for n_quals in (124, 128):
        assert not any(s == 5 for _, s in seen[n_quals]) and (bm.OK, 0) in seen[n_quals]
    # statuses 3 and 5 in one batch, and the call's code is the existing verdict's
    assert any(model_of(c, 4)["rc"] == ERR_DATA and {3, 5} <= set(model_of(c, 4)["status"]) for c in CATALOGUE)
    assert any(model_of(c, 4)["rc"] == bm.BAM_MORE and 5 in model_of(c, 4)["status"] for c in CATALOGUE)


def edge_case(name, quals_of_samples):
    """One read of four bases a sample at 1010..1013, its quality bytes as given."""
    return bc.case(name, [bc.sample([bc.R(1009, "4M", seq="ACGT", qual=q, flag=16 * (s % 2))]) for s, q in enumerate(quals_of_samples)], bc.span(1008, 1016))


@pytest.mark.parametrize("n_groups", [0, 5])
def test_the_qualities_either_side_of_forty_columns(ctx, n_groups):
    labels = np.array([0, 4, 255, 1], dtype=np.uint8)
    # 39 is counted; 128 and 255 are tallied, not counted and -- alone -- not refused
    c = edge_case("qualities 39, 128 and 255", [[39, 128, 255, 0], [255, 39, 39, 128]])
    exp = both_forms(ctx, c, 40, n_groups, labels[:2])
    t0 = c["positions"].index(1010)
    assert exp["rc"] == 0 and exp["status"] == [0, 0] and int(exp["counts"].sum()) == 4 and int(exp["counts"][:, :, 39].sum()) == 3
    assert exp["tally"]["strand_base"][t0:t0 + 4].sum() == 8
    if n_groups:
        assert int(exp["depth"].sum()) == 4
    # 40 and 127 have no column: each refuses its sample with status 5, and not a word changes
    for name, bad, where in (("quality 40", [39, 40, 39, 39], 1), ("quality 127", [1, 2, 3, 127], 2), ("qualities 40 and 127", [127, 128, 255, 40], 3)):
        rows = [[39, 128, 255, 0], [255, 39, 39, 128], [5, 6, 7, 8], [0, 0, 0, 0]]
        rows[where] = bad
        c = edge_case(name, rows)
        exp = both_forms(ctx, c, 40, n_groups, labels)
        assert exp["rc"] == ERR_DATA and exp["status"] == [5 if s == where else 0 for s in range(4)], name
        # the same batch at 128 columns is added whole
        assert both_forms(ctx, c, 128, n_groups, labels)["rc"] == 0
    # an N of quality 40 and an insertion's anchor of quality 40 are no counted observations: no refusal
    c = bc.case("an N and an indel entry of quality 40", [bc.sample([bc.R(1009, "4M", seq="ANGT", qual=[1, 40, 2, 3])]),
                                                          bc.sample([bc.R(1009, "2M2I2M", seq="ACGGTT", qual=[1, 40, 40, 40, 2, 3])])], bc.span(1008, 1016))
    exp = both_forms(ctx, c, 40, n_groups, labels[:2])
    assert exp["rc"] == 0 and exp["tally"]["n_other"].sum() == 1 and exp["tally"]["n_indel"].sum() == 1


def test_status_four_outranks_status_five_in_one_sample(ctx):
    """The out-of-range rule at 1016 and a base of quality 30 at 1012, eight columns: the sample's status is 4 whichever lane comes first."""
    c = next(x for x in CATALOGUE if x["name"] == "a query offset past the sequence")
    for _ in range(3):
        exp = both_forms(ctx, c, 8)
    assert exp["rc"] == ERR_DATA and exp["status"] == [4]
    # without the position that is out of range, the quality alone refuses it
    d = bc.case("a query offset inside the sequence", c["samples"], [1012])
    exp = both_forms(ctx, d, 8)
    assert exp["rc"] == ERR_DATA and exp["status"] == [5]


def test_a_bad_argument_leaves_the_arrays_as_they_were(ctx):
    c = next(x for x in CATALOGUE if x["name"] == "2 samples")
    bam, off, end, eof, rid, pos = arrays(c)
    P, Q = len(pos), 44
    labels = np.array([0, 1], dtype=np.uint8)
    counts, tally, depth = np.full(P * 4 * Q, 3, dtype=np.uint32), np.full(P * TW, 5, dtype=np.uint32), np.full(P * 2 * 4, 7, dtype=np.uint32)
    st = np.zeros(2, dtype=np.uint32)
    p = lambda x: C.c_void_p(x.ctypes.data)
    good = [ctx._h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), c["beg0"], c["end0"], c["min_mapq"], P, p(pos), c["rg_s"], len(c["refseq"]), p(labels), 2,
            Q, p(counts), p(tally), p(depth), p(st), 0]
    for i in (2, 4, 5, 6, 7, 12, 15, 18, 19, 20, 21):           # each pointer null with work present
        bad = list(good)
        bad[i] = None
        assert ctx._L.bvc_bam_counts_quals(*bad) == ERR_ARG, i
    for i, v in ((1, -1), (3, -1), (11, -1), (14, -1), (16, 33), (16, -1), (17, 0), (17, 2), (17, 42), (17, 132), (17, -4)):
        bad = list(good)
        bad[i] = v
        assert ctx._L.bvc_bam_counts_quals(*bad) == ERR_ARG, (i, v)
    assert b"n_quals must be a multiple of 4 in 4..128" in ctx._L.bvc_last_error(ctx._h)
    assert (counts == 3).all() and (tally == 5).all() and (depth == 7).all()
    # and the call still works: the model's words on top of the old ones; without groups the labels and the depths may be null
    exp = model_of(c, Q, 2, labels)
    assert ctx._L.bvc_bam_counts_quals(*good) == 0
    assert (counts == 3 + exp["counts"].reshape(-1)).all() and (tally == 5 + exp["tally"].view(np.uint32)).all() and (depth == 7 + exp["depth"].reshape(-1)).all()
    plain = list(good)
    plain[15], plain[16], plain[20] = None, 0, None
    assert ctx._L.bvc_bam_counts_quals(*plain) == 0
    assert (counts == 3 + 2 * exp["counts"].reshape(-1)).all() and (depth == 7 + exp["depth"].reshape(-1)).all() and int(exp["depth"].sum()) > 0


# ---- 2. the shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 65537])
def test_positions_around_a_wavefront_and_past_the_grids_chunks(ctx, P):
    """65,537 positions: 1025 chunks of 64 for a grid of 1024, so the last position is reached in the stride loop's second trip.  The
    spans' qualities stop at 41: 44 columns hold them."""
    c = span_case(P)
    labels = np.array([0, 1, 255, 1, 2], dtype=np.uint8)         # (two groups: label 2 is outside them)
    exp = both_forms(ctx, c, 44, 2, labels)
    assert exp["rc"] == 0 and exp["counts"][0].sum() > 0 and exp["counts"][P - 1].sum() > 0 and exp["depth"][P - 1].sum() > 0
    plain = both_forms(ctx, c, 44)
    assert (plain["counts"] == exp["counts"]).all() and plain["depth"] is None
    if P > 20:
        assert both_forms(ctx, c, 40)["rc"] == ERR_DATA          # (a quality of 40 or 41 somewhere)
    bc._EXPECTED.pop(c["name"], None)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_samples_either_side_of_a_workgroups_four_and_one_sample(ctx, n):
    c = span_case(100, n)
    labels = (np.arange(n) % 3).astype(np.uint8)
    exp = both_forms(ctx, c, 44, 3, labels)
    assert exp["rc"] == 0 and all(exp["depth"][:, g].sum() > 0 for g in range(min(n, 3)))
    both_forms(ctx, c, 44)
    bc._EXPECTED.pop(c["name"], None)


def test_no_samples_and_no_positions_are_no_ops(ctx):
    some = span_case(10, 3)
    for c in (bc.case("no samples here", [], some["positions"]), bc.case("no positions here", some["samples"], [])):
        for n_groups in (0, 2):
            exp = both_forms(ctx, c, 44, n_groups, np.zeros(len(c["samples"]), dtype=np.uint8))
            assert exp["rc"] == 0
        bc._EXPECTED.pop(c["name"], None)
    # no samples, but arrays to leave alone: not a word of them changes
    counts, tally = np.full(10 * 4 * 44, 7, dtype=np.uint32), np.full(10 * TW, 9, dtype=np.uint32)
    pos = np.arange(1, 11, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert ctx._L.bvc_bam_counts_quals(ctx._h, 0, None, 0, None, None, None, None, 0, 100, 20, 10, p(pos), 1, 50, None, 0, 44, p(counts), p(tally), None, None, 0) == 0
    assert (counts == 7).all() and (tally == 9).all()


# ---- 3. expansion -------------------------------------------------------------------------------------------------------------------------
def test_an_accumulator_of_128_columns_holds_a_wide_ones_bytes(ctx, bams100):
    from basevarc_amd import SiteAcc
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    G = 5
    labels = (np.arange(n) % 7).astype(np.uint8)
    with SiteAcc.create_quals(0, P, 128) as acc, SiteAcc(0, P) as wide, SiteAcc.create_quals(0, P, 128, G) as accg, SiteAcc.create_depth(0, P, G) as wideg:
        assert acc.bytes() == wide.bytes() == (qm.acc_bytes(P, 128), 0) and accg.bytes() == wideg.bytes() == (qm.acc_bytes(P, 128, G), 0)
        assert (acc.n_quals, wide.n_quals, accg.n_quals, wideg.n_quals) == (128, 128, 128, 128)
        for a in (acc, wide):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), a)[0] == 0
        for a in (accg, wideg):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), a, group_of_sample=labels)[0] == 0
        (c1, t1), (c2, t2), (c3, t3), (c4, t4) = (a.get(ctx) for a in (acc, wide, accg, wideg))
        assert c1.tobytes() == c2.tobytes() == c3.tobytes() == c4.tobytes() and t1.tobytes() == t2.tobytes() == t3.tobytes() == t4.tobytes()
        assert c1.sum() > 30000 and accg.get_depth(ctx).tobytes() == wideg.get_depth(ctx).tobytes()
        # the refusals of get_depth: no depth rows without groups
        from basevarc_amd.lib import BvcError
        with pytest.raises(BvcError, match="keeps no group depths") as e:
            acc.get_depth(ctx)
        assert e.value.status == ERR_ARG


@pytest.fixture(scope="module")
def narrow100(ctx, bams100):
    """The 100 test BAMs added once into an accumulator of 40 columns with five groups' depths, and into a wide one."""
    from basevarc_amd import SiteAcc
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    labels = (np.arange(n) % 7).astype(np.uint8)
    with SiteAcc.create_quals(0, P, 40, 5) as acc, SiteAcc(0, P) as wide:
        rc, st = ctx.bam_counts_bgzf_acc(*acc_args(b), acc, group_of_sample=labels)
        assert rc == 0 and list(st[:n]) == b["exp"]["status"]
        assert ctx.bam_counts_bgzf_acc(*acc_args(b), wide)[0] == 0
        yield acc, wide, labels


def test_the_fetched_rows_are_the_wide_layout_with_zeros_behind_the_columns(ctx, bams100, narrow100):
    acc, wide, labels = narrow100
    b = bams100
    P = len(b["pv"])
    assert acc.n_quals == 40 and acc.bytes() == (qm.acc_bytes(P, 40, 5), 0)
    want_c, want_t = cm.fold(b["exp"]["maps"], b["pv"])
    want_c = want_c.reshape(P, 512)
    counts, tally = acc.get(ctx)
    assert counts.shape == (P, 512) and (counts == want_c).all() and tally.tobytes() == want_t.tobytes() and counts.sum() > 30000
    assert not counts.reshape(P, 4, 128)[:, :, 40:].any() and (qm.expand(qm.narrow(counts, 40)) == counts).all()
    assert (acc.get_depth(ctx) == qm.gm.fold_maps(b["exp"]["maps"], b["pv"], labels, 5)[2]).all()
    # rows at odd places into a pre-filled destination with guards: exactly n rows are written
    p = lambda a: C.c_void_p(a.ctypes.data)
    for t0, n in ((1233, 0), (1233, 1), (77, 2), (4001, 65), (P - 1, 1), (P, 0)):
        dst = np.full(2 * GUARD + n * 512, GUARD_WORD, dtype=np.uint32)
        tl = np.full(2 * GUARD + n * TW, GUARD_WORD, dtype=np.uint32)
        assert ctx._L.bvc_site_acc_get(ctx._h, acc._h, t0, n, p(dst[GUARD:]), p(tl[GUARD:])) == 0
        assert (dst[:GUARD] == GUARD_WORD).all() and (dst[GUARD + n * 512:] == GUARD_WORD).all() and (tl[:GUARD] == GUARD_WORD).all() and (tl[GUARD + n * TW:] == GUARD_WORD).all()
        assert (dst[GUARD:GUARD + n * 512].reshape(n, 512) == want_c[t0:t0 + n]).all() and tl[GUARD:GUARD + n * TW].tobytes() == want_t[t0:t0 + n].tobytes()
    none, some = acc.get(ctx, 17, 40, counts=False)
    assert none is None and some.tobytes() == want_t[17:57].tobytes()
    from basevarc_amd.lib import BvcError
    for t0, n in ((1, P), (-1, 1), (0, P + 1)):
        with pytest.raises(BvcError, match="outside the accumulator"):
            acc.get(ctx, t0, n)


def test_stage_two_on_narrow_rows_is_a_wide_accumulators_byte_for_byte(ctx, bams100, narrow100):
    acc, wide, _ = narrow100
    b = bams100
    P = len(b["pv"])
    for t0, T in ((0, P), (1233, 777), (P - 1, 1)):
        ref = b["ref_base"][t0:t0 + T]
        res, want = acc.lrt(ctx, ref, MIN_AF, t0), wide.lrt(ctx, ref, MIN_AF, t0)
        assert res.tobytes() == want.tobytes(), (t0, T)
        if T == P:
            assert 0 < int((res["called"] != 0).sum()) < P // 10
    assert acc.lrt(ctx, np.zeros(0, dtype=np.int8), MIN_AF, 5).shape == (0,)


def test_a_call_of_one_row_more_than_a_piece_crosses_the_boundary(ctx):
    """32,769 rows of a mostly empty accumulator: reads at both ends and in the middle of the span, so the rows on both sides of the
    boundary -- the last one is the second piece's only row -- hold counts."""
    from basevarc_amd import SiteAcc
    P = EXPAND_ROWS + 1
    c = span_case(P)
    exp = model_of(c, 44)
    assert exp["rc"] == 0 and exp["counts"][P - 1].sum() > 0 and exp["counts"][0].sum() > 0 and exp["counts"][EXPAND_ROWS - 1].sum() > 0
    ref = (np.arange(P) % 4).astype(np.int8)
    with SiteAcc.create_quals(0, P, 44) as acc, SiteAcc(0, P) as wide:
        for a in (acc, wide):
            for _ in range(3):
                assert ctx.bam_counts_bgzf_acc(*bgzf_args(c), a)[0] == 0
        counts, tally = acc.get(ctx)
        assert (counts == 3 * qm.expand(exp["counts"])).all() and (tally.view(np.uint32) == 3 * exp["tally"].view(np.uint32)).all()
        assert counts.tobytes() == wide.get(ctx)[0].tobytes()
        res, want = acc.lrt(ctx, ref, MIN_AF), wide.lrt(ctx, ref, MIN_AF)
        assert res.tobytes() == want.tobytes() and res["called"][P - 1] == want["called"][P - 1]
        assert int((res["called"] != 0).sum()) > 0
        # the last two rows alone, and the first piece alone
        assert acc.lrt(ctx, ref[P - 2:], MIN_AF, P - 2).tobytes() == want[P - 2:].tobytes()
        assert acc.lrt(ctx, ref[:EXPAND_ROWS], MIN_AF).tobytes() == want[:EXPAND_ROWS].tobytes()
    bc._EXPECTED.pop(c["name"], None)


# ---- 4. the accumulator -----------------------------------------------------------------------------------------------------------------
def test_four_threads_contexts_add_into_one_narrow_accumulator(ctx):
    from basevarc_amd import Context, SiteAcc
    P, Q, G = 300, 44, 3
    base = span_case(P, 6)
    batches, seed = [], 40
    while len(batches) < 4:                                      # (random reads now and then leave the rule's range: batches that pass)
        rng = np.random.default_rng(seed)
        lo = base["positions"][0]
        samples = [bc.sample([bc.random_read(rng, int(p)) for p in np.sort(rng.integers(lo - 20, lo + P, 30))]) for _ in range(7 + len(batches))]
        c = bc.case(f"narrow thread batch {seed}", samples, base["positions"], rg_s=1000, refseq="A" * 80000)
        if bc.expected(c)["rc"] == 0:
            batches.append(c)
        else:
            bc._EXPECTED.pop(c["name"], None)
        seed += 1
    labels = [labels_of(c, G, k) for k, c in enumerate(batches)]
    want_c, want_t, want_d = np.zeros((P, 4, Q), dtype=np.uint32), np.zeros(P * TW, dtype=np.uint32), np.zeros((P, G, 4), dtype=np.uint32)
    for c, g in zip(batches, labels):
        exp = model_of(c, Q, G, g)
        assert exp["rc"] == 0                                    # (random qualities stop at 41)
        want_c += exp["counts"]
        want_t += exp["tally"].view(np.uint32)
        want_d += exp["depth"]
        bc._EXPECTED.pop(c["name"], None)
    assert want_c.sum() > 2000 and want_c.max() > 1 and want_d.sum() > 500
    errors = []
    with SiteAcc.create_quals(0, P, Q, G) as acc:
        def work(k):
            try:
                with Context(0) as c2:
                    for _ in range(3):                           # (three times each: twelve adds in flight between them)
                        rc, _ = c2.bam_counts_bgzf_acc(*bgzf_args(batches[k]), acc, group_of_sample=labels[k])
                        assert rc == 0
            except Exception as e:                               # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        counts, tally = acc.get(ctx)
        assert (counts == 3 * qm.expand(want_c)).all() and (tally.view(np.uint32) == 3 * want_t).all() and (acc.get_depth(ctx) == 3 * want_d).all()


def test_a_damaged_block_a_short_sample_and_a_quality_without_a_column_add_nothing(ctx, bams100):
    from basevarc_amd import SiteAcc
    from basevarc_amd.lib import BvcError
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    want = qm.expected(None, None, None, None, b["pv"], None, None, 36, exp=b["exp"])
    assert want["rc"] == ERR_DATA and want["status"].count(5) > 50
    with SiteAcc.create_quals(0, P, 40) as acc, SiteAcc.create_quals(0, P, 36) as tight:
        assert ctx.bam_counts_bgzf_acc(*acc_args(b), acc)[0] == 0
        counts, tally = acc.get(ctx)
        assert counts.sum() > 30000
        k = len(b["tab"]) // 2
        bad = b["comp"].copy()
        bad[int(b["tab"][k]["comp_off"]) + int(b["tab"][k]["comp_len"]) // 2] ^= 0x5A
        short_end, short_eof = list(b["end"]), b["eof"].copy()
        short_end[3], short_eof[3] = b["off"][3] + 5000, 0
        for a in (acc, tight):
            with pytest.raises(BvcError, match="BGZF block") as e:
                ctx.bam_counts_bgzf_acc(*acc_args(b, comp=bad), a)
            assert e.value.status == ERR_DATA
            rc, st = ctx.bam_counts_bgzf_acc(*acc_args(b, end=short_end, eof=short_eof), a)
            assert rc == bm.BAM_MORE and st[3] == 2              # (the existing verdict goes first, whatever the qualities)
        # 36 columns: the test BAMs hold qualities up to 39
        status = np.zeros(n, dtype=np.uint32)
        with pytest.raises(BvcError, match=f"sample {want['status'].index(5)}: .*n_quals = 36") as e:
            ctx.bam_counts_bgzf_acc(*acc_args(b), tight, sample_status=status)
        assert e.value.status == ERR_DATA and list(status) == want["status"]
        again, tally2 = acc.get(ctx)
        assert (again == counts).all() and tally2.tobytes() == tally.tobytes()
        nothing, no_tally = tight.get(ctx)
        assert not nothing.any() and not no_tally.view(np.uint32).any()
        # the accumulators and the context still work: the batch once more into the one that holds it
        assert ctx.bam_counts_bgzf_acc(*acc_args(b), acc)[0] == 0
        assert (acc.get(ctx)[0] == 2 * counts).all()
    # a budget one byte short of the arrays: refused, and one of exactly their size is made
    need = qm.acc_bytes(P, 40, 5)
    with pytest.raises(BvcError) as e:
        SiteAcc.create_quals(0, P, 40, 5, need - 1)
    assert e.value.status == ERR_ALLOC
    with SiteAcc.create_quals(0, P, 40, 5, need) as exact:
        assert exact.bytes() == (need, need)


def test_a_second_call_of_the_same_shape_allocates_nothing(ctx, bams100):
    import torch
    from basevarc_amd import SiteAcc
    b = bams100
    P = len(b["pv"])
    c = next(x for x in CATALOGUE if x["name"] == "300 samples")
    Q = 44
    bam, off, end, eof, rid, pos = arrays(c)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    d_args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], len(c["refseq"]), Q]
    d_counts = torch.zeros(len(pos) * 4 * Q, dtype=torch.int32, device="cuda")
    d_tally = torch.zeros(len(pos) * TW, dtype=torch.int32, device="cuda")
    d_status = torch.zeros(len(rid), dtype=torch.int32, device="cuda")
    counts, tally = np.zeros(len(pos) * 4 * Q, dtype=np.uint32), np.zeros(len(pos), dtype=cm.TALLY)
    with SiteAcc.create_quals(0, P, 40) as acc:
        free = []
        torch.cuda.mem_get_info()
        for _ in range(2):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), acc)[0] == 0
            acc.lrt(ctx, b["ref_base"], MIN_AF)
            acc.get(ctx)
            assert ctx.bam_counts_quals(*d_args, d_counts, d_tally, sample_status=d_status)[0] == 0
            assert ctx.bam_counts_quals(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"]), Q, counts, tally)[0] == 0
            ctx.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
        # the library allocates device memory of its own (not torch's pool): what is free on the device after the first round stays free
        assert free[1] == free[0], free
    want = model_of(c, Q)
    assert want["rc"] == 0
    assert (d_counts.cpu().numpy().view(np.uint32) == 2 * want["counts"].reshape(-1)).all() and (counts == 2 * want["counts"].reshape(-1)).all()
