"""bvc_bam_counts_depth, bvc_site_acc_create_depth and bvc_site_acc_get_depth on the device (bam_counts_kernel.hip, bvc_bam_counts.hip; GPU)
against the plain model (tests/bam_group_depth_model.py: what tests/bam_counts_model.py says the grouped call adds, folded into one slot of
counts and the groups' depths per base).

1. Every case of tests/bam_pileup_cases.py and 50 seeded random batches with 1, 5 and 32 groups, labels inside the groups, just outside
   them and 255, from host and from device pointers: the return code and statuses are the model's, and the three arrays -- pre-filled with
   random words, 0xFFFFFFFF wherever the model adds among them, guard words in front and behind -- hold the old words plus the model's,
   modulo 2^32, after BVC_OK and exactly the old words after anything else (a sample of status 2, 3 or 4, a bad argument).
2. The shapes: positions around a wavefront and past the grid's 1024 chunks, samples around a workgroup's four, one sample, a sample
   without a kept read.
3. The accumulator of the second kind on the 100 test BAMs' blocks, four threads adding at once and a damaged block in between, held to an
   accumulator of the first kind with the same groups (depth = its slots' sums per base, counts = the sum of its slots) and to one without
   groups (bvc_site_acc_lrt's records byte for byte); bvc_site_acc_get_depth refuses the first kind."""
import threading

import numpy as np
import pytest

from tests import bam_group_depth_model as gm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests.test_gpu_bam_counts import (CATALOGUE, ERR_ALLOC, ERR_ARG, ERR_DATA, GUARD, GUARD_WORD, MIN_AF, TW, acc_args, arrays, guarded, span_case,
                                       bams100)  # noqa: F401  (bams100: that module's fixture of the 100 test BAMs)

pytestmark = pytest.mark.gpu

GROUPS = (1, 5, 32)


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def labels_of(c, n_groups, seed=0):
    """One label per sample: 0 .. n_groups + 2 (the last three lie outside the groups), every fifth sample the program's 255."""
    g = np.random.default_rng(3000 + seed).integers(0, n_groups + 3, size=len(c["samples"])).astype(np.uint8)
    g[seed % 5::5] = 255
    return g


def model_of(c, n_groups, labels):
    return gm.expected(None, None, None, None, c["positions"], None, None, labels, n_groups, exp=bc.expected(c))


def run(ctx, c, device, n_groups, labels, exp):
    """One bvc_bam_counts_depth call on guarded, pre-filled arrays.  Returns (rc or the BvcError's status, sample_status with its guard,
    [(buffer, its old words, the model's words or None)] for counts, tally and depth)."""
    from basevarc_amd.lib import BvcError
    bam, off, end, eof, rid, pos = arrays(c)
    n, P = len(rid), len(pos)
    rng = np.random.default_rng(len(bam) + 7 * P + n_groups)
    sizes = (P * 512, P * TW, P * n_groups * 4) if n else (0, 0, 0)
    wants = (exp["counts"], None if exp["tally"] is None else exp["tally"].view(np.uint32), exp["depth"])
    bufs = [guarded(rng, np.zeros(size, dtype=np.uint32) if w is None else w) for size, w in zip(sizes, wants)]
    status = np.full(n + GUARD, GUARD_WORD, dtype=np.uint32)
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        d_bufs, d_s = [dev(b) for b, _ in bufs], dev(status)
        args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], len(c["refseq"])]
        out = [d[GUARD:GUARD + len(pre)] for d, (_, pre) in zip(d_bufs, bufs)]
        kw = dict(group_of_sample=dev(labels), n_groups=n_groups, sample_status=d_s)
    else:
        args = [bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"])]
        out = [b[GUARD:GUARD + len(pre)] for b, pre in bufs]
        kw = dict(group_of_sample=labels, n_groups=n_groups, sample_status=status)
    try:
        rc, _ = ctx.bam_counts_depth(*args, *out, **kw)
    except BvcError as e:
        rc = e.status
    if device:
        ctx.synchronize()
        status = d_s.cpu().numpy().view(np.uint32)
        bufs = [(d.cpu().numpy().view(np.uint32), pre) for d, (_, pre) in zip(d_bufs, bufs)]
    return rc, status, [(b, pre, w) for (b, pre), w in zip(bufs, wants)]


def check(c, got, exp):
    """What a call left, against the model: old + model (mod 2^32) after BVC_OK, the old words otherwise, the guards as they were."""
    rc, status, bufs = got
    n = len(c["samples"])
    assert rc == exp["rc"], (c["name"], rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], list(status[:n]), exp["status"])
    assert (status[n:] == GUARD_WORD).all(), c["name"]
    for which, (buf, pre, want) in zip(("counts", "tally", "depth"), bufs):
        assert (buf[:GUARD] == GUARD_WORD).all() and (buf[GUARD + len(pre):] == GUARD_WORD).all(), (c["name"], which)
        body = buf[GUARD:GUARD + len(pre)]
        if rc == bm.OK and want is not None and len(pre):
            w = want.reshape(-1)
            bad = np.flatnonzero(body != pre + w)           # (uint32 arithmetic wraps)
            assert bad.size == 0, (c["name"], which, bad[:8], body[bad[:8]], pre[bad[:8]], w[bad[:8]])
        else:
            assert (body == pre).all(), (c["name"], which)


def both_forms(ctx, c, n_groups, labels):
    exp = model_of(c, n_groups, labels)
    for device in (False, True):
        check(c, run(ctx, c, device, n_groups, labels, exp), exp)
    return exp


# ---- 1. the catalogue and the random batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_catalogue_case(ctx, c):
    """With 1, 5 and 32 groups, from host and from device pointers.  The catalogue holds samples of status 2, 3 and 4
    (tests/test_gpu_bam_counts.py, test_the_catalogue_holds_every_verdict): after those calls not a word of the three arrays has changed."""
    for k, n_groups in enumerate(GROUPS):
        both_forms(ctx, c, n_groups, labels_of(c, n_groups, k))


RANDOM_SEEDS = tuple(range(20271000, 20271050))


@pytest.mark.parametrize("n_groups", GROUPS)
def test_fifty_seeded_random_batches(ctx, n_groups):
    rcs, depth = set(), 0
    for seed in RANDOM_SEEDS:
        c = bc.random_case(seed)
        exp = both_forms(ctx, c, n_groups, labels_of(c, n_groups, seed))
        rcs.add(exp["rc"])
        if exp["rc"] == 0:
            depth += int(exp["depth"].sum())
            assert int(exp["depth"].sum()) <= int(exp["counts"].sum()) <= int(exp["tally"]["strand_base"].sum())
        bc._EXPECTED.pop(c["name"], None)                    # (the catalogue's cache is not for one-off cases)
    assert rcs == {bm.OK, bm.BAM_MORE, ERR_DATA} and depth > 1000, (rcs, depth)


def test_a_bad_argument_leaves_the_three_arrays_as_they_were(ctx):
    import ctypes as C
    c = next(x for x in CATALOGUE if x["name"] == "2 samples")
    bam, off, end, eof, rid, pos = arrays(c)
    P = len(pos)
    labels = np.array([0, 1], dtype=np.uint8)
    counts, tally, depth = np.full(P * 512, 3, dtype=np.uint32), np.full(P * TW, 5, dtype=np.uint32), np.full(P * 2 * 4, 7, dtype=np.uint32)
    st = np.zeros(2, dtype=np.uint32)
    p = lambda x: C.c_void_p(x.ctypes.data)
    good = [ctx._h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), c["beg0"], c["end0"], c["min_mapq"], P, p(pos), c["rg_s"], len(c["refseq"]), p(labels), 2,
            p(counts), p(tally), p(depth), p(st), 0]
    for i in (2, 4, 5, 6, 7, 12, 15, 17, 18, 19, 20):           # each pointer null with work present
        bad = list(good)
        bad[i] = None
        assert ctx._L.bvc_bam_counts_depth(*bad) == ERR_ARG, i
    for i, v in ((1, -1), (3, -1), (11, -1), (14, -1), (16, 0), (16, 33), (16, -1)):      # each size negative; n_groups outside 1..32
        bad = list(good)
        bad[i] = v
        assert ctx._L.bvc_bam_counts_depth(*bad) == ERR_ARG, (i, v)
    assert (counts == 3).all() and (tally == 5).all() and (depth == 7).all()
    # and the call still works: the model's words on top of the old ones
    exp = model_of(c, 2, labels)
    assert ctx._L.bvc_bam_counts_depth(*good) == 0
    assert (counts == 3 + exp["counts"].reshape(-1)).all() and (tally == 5 + exp["tally"].view(np.uint32)).all() and (depth == 7 + exp["depth"].reshape(-1)).all()
    assert int(exp["depth"].sum()) > 0


# ---- 2. the shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 64, 65, 65537])
def test_positions_around_a_wavefront_and_past_the_grids_chunks(ctx, P):
    """65,537 positions: 1025 chunks of 64 for a grid of 1024, so the last position is reached in the stride loop's second trip."""
    c = span_case(P)
    labels = np.array([0, 1, 255, 1, 2], dtype=np.uint8)         # (two groups: label 2 is outside them)
    exp = both_forms(ctx, c, 2, labels)
    assert exp["rc"] == 0 and exp["depth"][0].sum() > 0 and exp["depth"][P - 1].sum() > 0 and exp["depth"][:, 1].sum() > exp["depth"][:, 0].sum() > 0
    assert exp["depth"].sum() < exp["counts"].sum()
    bc._EXPECTED.pop(c["name"], None)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_samples_either_side_of_a_workgroups_four_and_one_sample(ctx, n):
    c = span_case(100, n)
    labels = (np.arange(n) % 3).astype(np.uint8)
    exp = both_forms(ctx, c, 3, labels)
    assert exp["rc"] == 0 and all(exp["depth"][:, g].sum() > 0 for g in range(min(n, 3)))
    bc._EXPECTED.pop(c["name"], None)


def test_a_sample_without_a_kept_read_adds_nothing(ctx):
    some = span_case(70, 3)
    c = bc.case("a sample without a kept read", [some["samples"][0], bc.sample([bc.R(900, "20M", mapq=3)]), some["samples"][1], bc.sample([])],
                some["positions"], rg_s=1000, refseq="A" * 80000)
    labels = np.array([1, 0, 1, 0], dtype=np.uint8)
    exp = both_forms(ctx, c, 2, labels)
    assert exp["rc"] == 0 and exp["status"] == [0, 1, 0, 1] and not exp["depth"][:, 0].any() and exp["depth"][:, 1].sum() > 0
    bc._EXPECTED.pop(c["name"], None)


# ---- 3. the accumulator -----------------------------------------------------------------------------------------------------------------
def test_the_second_kind_on_the_test_bams_against_the_first_kind(ctx, bams100):
    from basevarc_amd import Context, SiteAcc
    from basevarc_amd.lib import BvcError
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    G = 5
    labels = (np.arange(n) % 7).astype(np.uint8)                 # (labels 5 and 6 are in no group)
    labels[::11] = 255
    errors = []
    with SiteAcc.create_depth(0, P, G) as acc, SiteAcc(0, P, G) as grouped, SiteAcc(0, P) as plain:
        assert acc.bytes() == (P * (2048 + 48 + 16 * G), 0) and acc.depth_groups == G
        assert not acc.get_depth(ctx).any()

        def work():
            try:
                with Context(0) as c2:
                    rc, st = c2.bam_counts_bgzf_acc(*acc_args(b), acc, group_of_sample=labels)
                    assert rc == 0 and list(st[:n]) == b["exp"]["status"]
            except Exception as e:                               # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work) for _ in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        counts, tally = acc.get(ctx)
        depth = acc.get_depth(ctx)
        assert counts.shape == (P, 512) and depth.shape == (P, G, 4)
        # a damaged block, a sample cut short, no labels: the codes of the first kind, and not a word changes
        k = len(b["tab"]) // 2
        bad = b["comp"].copy()
        bad[int(b["tab"][k]["comp_off"]) + int(b["tab"][k]["comp_len"]) // 2] ^= 0x5A
        with pytest.raises(BvcError, match="BGZF block") as e:
            ctx.bam_counts_bgzf_acc(*acc_args(b, comp=bad), acc, group_of_sample=labels)
        assert e.value.status == ERR_DATA
        short_end, short_eof = list(b["end"]), b["eof"].copy()
        short_end[3], short_eof[3] = b["off"][3] + 5000, 0
        rc, st = ctx.bam_counts_bgzf_acc(*acc_args(b, end=short_end, eof=short_eof), acc, group_of_sample=labels)
        assert rc == bm.BAM_MORE and st[3] == 2
        with pytest.raises(BvcError, match="null group_of_sample") as e:
            ctx.bam_counts_bgzf_acc(*acc_args(b), acc)
        assert e.value.status == ERR_ARG
        again, tally2 = acc.get(ctx)
        assert (again == counts).all() and tally2.tobytes() == tally.tobytes() and (acc.get_depth(ctx) == depth).all()
        # 1. the first kind with the same groups, fed the same batch four times
        for _ in range(4):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), grouped, group_of_sample=labels)[0] == 0
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), plain)[0] == 0
        gcounts, gtally = grouped.get(ctx)
        want_c, want_d = gm.fold(gcounts, G)
        assert (counts == want_c).all() and (depth == want_d).all() and tally.tobytes() == gtally.tobytes()
        assert all(depth[:, g].sum() > 10000 for g in range(G)) and depth.sum() < counts.sum()
        # ... which is four times the model's
        mc, md = gm.fold(gm.cm.fold(b["exp"]["maps"], b["pv"], labels, G)[0], G)
        assert (counts == 4 * mc).all() and (depth == 4 * md).all()
        # rows from the middle
        assert (acc.get_depth(ctx, 17, 40) == depth[17:57]).all() and acc.get_depth(ctx, P, 0).shape[0] == 0
        # 2. the first kind without groups: stage 2 where the rows lie, byte for byte
        for t0, T in ((0, P), (1234, 777)):
            ref = b["ref_base"][t0:t0 + T]
            res, want = acc.lrt(ctx, ref, MIN_AF, t0), plain.lrt(ctx, ref, MIN_AF, t0)
            assert res.tobytes() == want.tobytes(), (t0, T)
            if T == P:
                assert 0 < int((res["called"] != 0).sum()) < P // 10
        # the refusals of the new call
        for a, match in ((grouped, "keeps no group depths"), (plain, "keeps no group depths")):
            with pytest.raises(BvcError, match=match) as e:
                a.get_depth(ctx)
            assert e.value.status == ERR_ARG
        for t0, T in ((1, P), (-1, 1), (0, P + 1)):
            with pytest.raises(BvcError, match="outside the accumulator") as e:
                acc.get_depth(ctx, t0, T)
            assert e.value.status == ERR_ARG
        assert ctx._L.bvc_site_acc_get_depth(ctx._h, acc._h, 0, 1, None) == ERR_ARG
        if ctx._L.bvc_device_count() > 1:
            with Context(1) as far, pytest.raises(BvcError, match="another device"):
                acc.get_depth(far)
    # a budget one byte short of the three arrays: refused, and one of exactly their size is made
    need = P * (2048 + 48 + 16 * G)
    with pytest.raises(BvcError) as e:
        SiteAcc.create_depth(0, P, G, need - 1)
    assert e.value.status == ERR_ALLOC
    with SiteAcc.create_depth(0, P, G, need) as exact:
        assert exact.bytes() == (need, need)
