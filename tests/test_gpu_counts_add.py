"""Counts accumulated over chunks of a cohort's samples (GPU): bvc_counts_add_dense[_packed], bvc_counts_add_csr[_packed],
bvc_counts_add_dense_groups, bvc_counts_add_csr_group_labels, bvc_lrt_hist_groups, bvc_counts_merge.

Class counts are integers and add over samples, so every comparison here is equality of words (with the one-piece histogram call and with
the oracle's counts) or of the raw record bytes (with the one-piece bvc_lrt_* call).  No tolerance appears anywhere.

Shapes: the dense tile is 37 sites x 6000 samples cut by columns into chunks of 1, 63, 64, 500, 4097 and the remaining 1275 (rows
that start on and off a 16-byte boundary, with a row stride that is and is not a multiple of 16); the ragged columns are ~200 sites of total depths 0 .. 9000
dealt to 7 chunks by sample range, among them sites whose depth in ONE chunk is exactly 63, 64 and 65 -- the two sides of the cut-over
between hist_csr_scatter_kernel and hist_csr_add_kernel when "csr_scatter_max" is 64.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu

BVC_OK, BVC_ERR_ARG = 0, -1
HOST, DEVICE = 0, 1
MIN_AF = 0.001
NS, N = 37, 6000
CHUNK_SIZES = [1, 63, 64, 500, 4097]
N_RAGGED_SAMPLES, N_RAGGED_CHUNKS = 7000, 7


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                     # (a copy: the cached cases are read-only)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def zeros(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.int32, device="cuda")


def offset_view(a, shift):
    """The bytes of `a` on the device, `shift` bytes behind the start of their own allocation."""
    import torch
    t = torch.zeros(len(a) + 8, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    v = t[shift:shift + len(a)]
    v.copy_(torch.from_numpy(np.array(a)))
    return v


# ------------------------------------------------------------------------------------------------ the dense tile
@functools.lru_cache(maxsize=None)
def dense_case(packable):
    """(bases, quals, ref, column ranges in shuffled order); ~30 % uncovered; qualities 0..127 (packable: 0..62).  Never modified."""
    rng = np.random.default_rng(11 + packable)
    ref = rng.integers(0, 4, NS).astype(np.int8)
    alt = (ref + 1 + rng.integers(0, 3, NS)) % 4
    af = rng.choice([0.0, 0.01, 0.2, 0.5], NS)
    b = np.where(rng.random((NS, N)) < af[:, None], alt[:, None], ref[:, None]).astype(np.int8)
    q = rng.integers(5, 42, (NS, N)).astype(np.int8)
    wide = rng.random((NS, N)) < 0.1
    q[wide] = rng.integers(0, 63 if packable else 128, int(wide.sum()))
    err = rng.random((NS, N)) < 10.0 ** (-np.maximum(q, 3) / 10.0)
    b[err] = (b[err] + 1 + rng.integers(0, 3, int(err.sum()))) % 4
    b[rng.random((NS, N)) < 0.3] = -1
    if not packable:
        b[rng.random((NS, N)) < 0.001] = 5                           # no A/C/G/T
        q[rng.random((NS, N)) < 0.001] = -3                          # no quality
    bounds = np.concatenate([[0], np.cumsum(CHUNK_SIZES), [N]])
    ranges = [(int(bounds[i]), int(bounds[i + 1])) for i in range(len(bounds) - 1)]
    order = np.random.default_rng(5).permutation(len(ranges))
    ranges = tuple(ranges[i] for i in order)
    for a in (b, q, ref):
        a.setflags(write=False)
    return b, q, ref, ranges


@functools.lru_cache(maxsize=None)
def dense_oracle_counts(packable):
    b, q, _, _ = dense_case(packable)
    out = np.stack([orc.dense_hist(b[s], q[s]) for s in range(NS)])
    out.setflags(write=False)
    return out


def strided(a, stride):
    """`a` on the device in rows `stride` bytes apart."""
    import torch
    t = torch.full((a.shape[0], stride), -1, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    t[:, :a.shape[1]] = dev(a)
    return t[:, :a.shape[1]]


def pack(b, q):
    covered = (b >= 0) & (b < 4) & (q >= 0) & (q < 63)
    return np.where(covered, (b.astype(np.int32) << 6) | (q.astype(np.int32) & 63), 0xFF).astype(np.uint8)


@pytest.mark.parametrize("stride", [N, N + 7])
def test_dense_chunks_add_up_to_the_whole_tile(ctx, stride):
    b, q, _, ranges = dense_case(False)
    bt, qt = strided(b, stride), strided(q, stride)
    whole = words(ctx.hist_dense_device(bt, qt))
    assert np.array_equal(whole, dense_oracle_counts(False))
    counts = zeros(NS, 512)
    for lo, hi in ranges:
        ctx.counts_add_dense_device(bt[:, lo:hi], qt[:, lo:hi], counts)
    ctx.synchronize()
    assert np.array_equal(words(counts), whole)


def test_dense_chunks_add_to_what_the_counts_held(ctx):
    b, q, _, ranges = dense_case(False)
    bt, qt = dev(b), dev(q)
    prefill = np.random.default_rng(3).integers(0, 1 << 32, (NS, 512), dtype=np.uint64).astype(np.uint32)
    counts = dev(prefill.view(np.int32))
    for lo, hi in ranges:
        ctx.counts_add_dense_device(bt[:, lo:hi], qt[:, lo:hi], counts)
    ctx.synchronize()
    assert np.array_equal(words(counts), prefill + dense_oracle_counts(False))       # (uint32: wraps like the library)


@pytest.mark.parametrize("stride", [N, N + 7])
def test_packed_dense_chunks_add_up_to_the_whole_tile(ctx, stride):
    b, q, _, ranges = dense_case(True)
    pt = strided(pack(b, q), stride)
    whole = words(ctx.hist_dense_packed_device(pt))
    assert np.array_equal(whole, dense_oracle_counts(True))
    prefill = np.random.default_rng(4).integers(0, 1 << 32, (NS, 512), dtype=np.uint64).astype(np.uint32)
    counts, filled = zeros(NS, 512), dev(prefill.view(np.int32))
    for lo, hi in ranges:
        ctx.counts_add_dense_packed_device(pt[:, lo:hi], counts)
        ctx.counts_add_dense_packed_device(pt[:, lo:hi], filled)
    ctx.synchronize()
    assert np.array_equal(words(counts), whole)
    assert np.array_equal(words(filled), prefill + whole)


def accumulated_dense(ctx):
    b, q, _, ranges = dense_case(False)
    bt, qt = dev(b), dev(q)
    counts = zeros(NS, 512)
    for lo, hi in ranges:
        ctx.counts_add_dense_device(bt[:, lo:hi], qt[:, lo:hi], counts)
    return bt, qt, counts


def record_bytes(ctx, *tensors):
    ctx.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def test_records_of_accumulated_counts_are_those_of_the_whole_tile(ctx):
    _, _, ref, _ = dense_case(False)
    bt, qt, counts = accumulated_dense(ctx)
    rt = dev(ref)
    got, = record_bytes(ctx, ctx.lrt_hist_device(counts, rt, MIN_AF))
    want, = record_bytes(ctx, ctx.lrt_dense_device(bt, qt, rt, MIN_AF))
    assert len(want) == NS * 120 and got == want


# ------------------------------------------------------------------------------------------------ ragged columns
@functools.lru_cache(maxsize=None)
def ragged_case():
    """~200 sites as (offsets, bases, quals, sample of each observation, ref) with qualities <= 62, plus the per-chunk columns.
    Total depths 0, 1, 63, 64, 65, 4095, 4096, 9000 and random ones up to 300; three sites lie in ONE chunk with 63, 64 and 65
    observations.  A site's observations are in sample order; chunk c holds samples [1000 c, 1000 (c + 1))."""
    rng = np.random.default_rng(21)
    depths = [0, 1, 63, 64, 65, 4095, 4096, 9000, 0, 0] + rng.integers(0, 301, 186).tolist()
    sites = []
    for n in depths:
        sites.append(np.sort(rng.integers(0, N_RAGGED_SAMPLES, n)).astype(np.int32))
    for n in (63, 64, 65):                                            # exactly this deep in chunk 2 and in no other
        sites.append(np.sort(rng.integers(2000, 3000, n)).astype(np.int32))
    total = sum(len(s) for s in sites)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in sites])]).astype(np.int64)
    smp = np.concatenate(sites).astype(np.int32)
    ref = rng.integers(0, 4, len(sites)).astype(np.int8)
    site_of = np.repeat(np.arange(len(sites)), np.diff(offs))
    b = ref[site_of].copy()
    alt = rng.random(total) < 0.05
    b[alt] = (b[alt] + 1 + rng.integers(0, 3, int(alt.sum()))) % 4
    q = rng.integers(5, 42, total).astype(np.int8)
    q[rng.random(total) < 0.05] = 62
    chunks = []
    for c in range(N_RAGGED_CHUNKS):
        take = (smp >= 1000 * c) & (smp < 1000 * (c + 1))
        co = np.concatenate([[0], np.cumsum(np.bincount(site_of[take], minlength=len(sites)))]).astype(np.int64)
        chunks.append((co, b[take], q[take], smp[take]))
    assert sorted(np.diff(chunks[2][0])[-3:].tolist()) == [63, 64, 65] and any((np.diff(co) == 0).sum() > 10 for co, _, _, _ in chunks)
    for a in (offs, b, q, smp, ref):
        a.setflags(write=False)
    return offs, b, q, smp, ref, tuple(chunks)


def two_byte_ragged():
    """The ragged case with what only two bytes can say: qualities of 63 and more, entries that are no base or no quality."""
    offs, b, q, smp, ref, chunks = ragged_case()
    rng = np.random.default_rng(22)

    def widen(bb, qq):
        bb, qq = bb.copy(), qq.copy()
        if len(bb):
            qq[rng.random(len(qq)) < 0.05] = 93
            qq[rng.random(len(qq)) < 0.01] = -1
            bb[rng.random(len(bb)) < 0.01] = 4
        return bb, qq
    return [(co,) + widen(cb, cq) + (cs,) for co, cb, cq, cs in chunks]


def ragged_whole_counts(chunks, n_sites):
    """The counts of all observations of all chunks, by the oracle's histogram of each site's concatenated columns."""
    out = np.zeros((n_sites, 512), dtype=np.uint32)
    for s in range(n_sites):
        sb = np.concatenate([cb[co[s]:co[s + 1]] for co, cb, _, _ in chunks])
        sq = np.concatenate([cq[co[s]:co[s + 1]] for co, _, cq, _ in chunks])
        out[s] = orc.dense_hist(sb, sq)
    return out


SHIFTS = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (3, 2), (2, 0)]       # byte offsets of a chunk's arrays: agreeing and not


def add_ragged(c, chunks, packed):
    n_sites = len(chunks[0][0]) - 1
    counts = zeros(n_sites, 512)
    for i, (co, cb, cq, _) in enumerate(chunks):
        sb, sq = SHIFTS[i % len(SHIFTS)]
        if packed:
            c.counts_add_csr_packed_device(dev(co), offset_view(pack(cb, cq), sb), counts)
        else:
            c.counts_add_csr_device(dev(co), offset_view(cb, sb), offset_view(cq, sq), counts)
    c.synchronize()
    return words(counts)


@pytest.mark.parametrize("packed", [False, True])
def test_ragged_chunks_add_up_whatever_the_cut_over(packed):
    from basevarc_amd import Context
    chunks = ragged_case()[5] if packed else two_byte_ragged()
    want = ragged_whole_counts(chunks, len(chunks[0][0]) - 1)
    assert want.sum() > 20000
    for cut in (None, 0, 64, 1 << 30):                               # None: the context's default
        with Context(0) as c:
            if cut is not None:
                c.set_tuning("csr_scatter_max", cut)
            assert np.array_equal(add_ragged(c, chunks, packed), want), cut


def test_ragged_chunks_equal_the_one_piece_call(ctx):
    offs, b, q, _, ref, chunks = ragged_case()
    got = add_ragged(ctx, chunks, False)
    rt = dev(ref)
    a, = record_bytes(ctx, ctx.lrt_hist_device(dev(got.view(np.int32)), rt, MIN_AF))
    w, = record_bytes(ctx, ctx.lrt_csr_device(dev(offs), dev(b), dev(q), rt, MIN_AF))
    assert a == w


# ------------------------------------------------------------------------------------------------ groups
def labels_for(k, n, seed):
    """One label per sample: groups 0..k-1 with some left EMPTY (k >= 5), ~10 % of the samples in no group (255, or k itself)."""
    rng = np.random.default_rng(seed)
    used = [g for g in range(k) if k < 5 or g not in (3, k - 1)]
    lab = rng.choice(used, n).astype(np.uint8)
    none = rng.random(n) < 0.1
    lab[none] = rng.choice([255, k], int(none.sum())).astype(np.uint8)
    return lab


@pytest.mark.parametrize("k", [1, 5, 32])
def test_dense_group_chunks_then_stage_two(ctx, k):
    b, q, ref, _ = dense_case(False)
    bt, qt, rt = dev(b), dev(q), dev(ref)
    lab = labels_for(k, N, 30 + k)
    gt = dev(lab)
    grp = zeros(NS, k + 1, 512)
    for lo, hi in ((4597, N), (0, 500), (500, 4597)):
        ctx.counts_add_dense_groups_device(bt[:, lo:hi], qt[:, lo:hi], gt[lo:hi], k, grp)
    ctx.synchronize()
    g = words(grp)
    assert np.array_equal(g.sum(axis=1, dtype=np.uint32), dense_oracle_counts(False))
    for s in (0, NS - 1):                                            # slot n_groups holds the samples in no group
        assert np.array_equal(g[s, k], orc.dense_hist(b[s][lab >= k], q[s][lab >= k]))
        assert np.array_equal(g[s, 0], orc.dense_hist(b[s][lab == 0], q[s][lab == 0]))
    before = g.copy()
    got = record_bytes(ctx, *ctx.lrt_hist_groups_device(grp, rt, MIN_AF, k))
    want = record_bytes(ctx, *ctx.lrt_dense_groups_device(bt, qt, rt, MIN_AF, gt, k))
    assert len(want[1]) == NS * k * 48 and got == want
    assert np.array_equal(words(grp), before)


@pytest.mark.parametrize("k", [1, 5, 32])
def test_ragged_label_chunks_then_stage_two(k):
    from basevarc_amd import Context
    with Context(0) as ctx:                                          # a context of its own: the key it sets reaches no other test
        ragged_label_chunks_then_stage_two(ctx, k)


def ragged_label_chunks_then_stage_two(ctx, k):
    offs, b, q, smp, ref, _ = ragged_case()
    chunks = two_byte_ragged()
    lab = labels_for(k, N_RAGGED_SAMPLES, 40 + k)
    n_sites = len(ref)
    ctx.set_tuning("csr_scatter_max", 64)
    grp = zeros(n_sites, k + 1, 512)
    for i, (co, cb, cq, cs) in enumerate(chunks):
        sb, sq = SHIFTS[i % len(SHIFTS)]
        ctx.counts_add_csr_group_labels_device(dev(co), offset_view(cb, sb), offset_view(cq, sq), offset_view(lab[cs], sb), k, grp)
    ctx.synchronize()
    before = words(grp).copy()
    assert np.array_equal(before.sum(axis=1, dtype=np.uint32), ragged_whole_counts(chunks, n_sites))
    rt = dev(ref)
    got = record_bytes(ctx, *ctx.lrt_hist_groups_device(grp, rt, MIN_AF, k))
    # the whole columns: every site's observations of all chunks, chunk after chunk
    cat = lambda j: np.concatenate([np.concatenate([c[j][c[0][s]:c[0][s + 1]] for c in chunks]) for s in range(n_sites)])
    wb, wq, ws = cat(1), cat(2), cat(3)
    want = record_bytes(ctx, *ctx.lrt_csr_group_labels_device(dev(offs), dev(wb), dev(wq), dev(lab[ws]), rt, MIN_AF, k))
    assert got == want
    assert np.array_equal(words(grp), before)


# ------------------------------------------------------------------------------------------------ host pointers, overlap mode
def test_host_pointers_give_the_counts_and_records_of_device_pointers(ctx):
    b, q, ref, ranges = dense_case(False)
    counts = np.zeros((NS, 512), dtype=np.uint32)
    for lo, hi in ranges:
        ctx.counts_add_dense(b[:, lo:hi], q[:, lo:hi], counts)
    assert np.array_equal(counts, dense_oracle_counts(False))
    bt, qt, dcounts = accumulated_dense(ctx)
    want, = record_bytes(ctx, ctx.lrt_hist_device(dcounts, dev(ref), MIN_AF))
    assert ctx.lrt_hist(counts, ref, MIN_AF).tobytes() == want
    pb, pq, _, _ = dense_case(True)
    pcounts = np.zeros((NS, 512), dtype=np.uint32)
    for lo, hi in ranges:
        ctx.counts_add_dense_packed(pack(pb, pq)[:, lo:hi], pcounts)
    assert np.array_equal(pcounts, dense_oracle_counts(True))
    # ragged, plain and packed
    chunks = ragged_case()[5]
    want_r = ragged_whole_counts(chunks, len(chunks[0][0]) - 1)
    for packed in (False, True):
        rc = np.zeros_like(want_r)
        for co, cb, cq, _ in chunks:
            if packed:
                ctx.counts_add_csr_packed(co, pack(cb, cq), rc)
            else:
                ctx.counts_add_csr(co, cb, cq, rc)
        assert np.array_equal(rc, want_r), packed


def test_host_pointer_group_calls(ctx):
    k = 5
    b, q, ref, _ = dense_case(False)
    lab = labels_for(k, N, 30 + k)
    grp = np.zeros((NS, k + 1, 512), dtype=np.uint32)
    for lo, hi in ((4597, N), (0, 500), (500, 4597)):
        ctx.counts_add_dense_groups(b[:, lo:hi], q[:, lo:hi], lab[lo:hi], k, grp)
    res, gres = ctx.lrt_hist_groups(grp, ref, MIN_AF, k)
    wres, wgres = ctx.lrt_dense_groups(b, q, ref, MIN_AF, lab, k)
    assert res.tobytes() == wres.tobytes() and gres.tobytes() == wgres.tobytes()
    chunks = two_byte_ragged()
    rlab = labels_for(k, N_RAGGED_SAMPLES, 40 + k)
    n_sites = len(chunks[0][0]) - 1
    rgrp, dgrp = np.zeros((n_sites, k + 1, 512), dtype=np.uint32), zeros(n_sites, k + 1, 512)
    for co, cb, cq, cs in chunks:
        ctx.counts_add_csr_group_labels(co, cb, cq, rlab[cs], k, rgrp)
        ctx.counts_add_csr_group_labels_device(dev(co), dev(cb), dev(cq), dev(rlab[cs]), k, dgrp)
    ctx.synchronize()
    assert np.array_equal(rgrp, words(dgrp))


def test_overlap_mode_leaves_the_records_unchanged(ctx):
    _, _, ref, _ = dense_case(False)
    bt, qt, counts = accumulated_dense(ctx)
    rt = dev(ref)
    want, = record_bytes(ctx, ctx.lrt_hist_device(counts, rt, MIN_AF))
    whole, = record_bytes(ctx, ctx.lrt_dense_device(bt, qt, rt, MIN_AF))
    ctx.set_overlap(True)
    keep = []                                                        # everything handed to the library stays alive and untouched until join()
    try:
        keep.append(ctx.lrt_dense_device(bt, qt, rt, MIN_AF))        # its stage 2 runs on a side stream while the chunks are added
        keep.append(accumulated_dense(ctx))
        again = keep[-1][2]
        res = ctx.lrt_hist_device(again, rt, MIN_AF)
        keep.append(res)
        ctx.join()
        got, under = record_bytes(ctx, res, keep[0])
    finally:
        ctx.synchronize()
        ctx.set_overlap(False)
    assert got == want
    assert under == whole                                            # and the call that ran beside them is what it is alone
    del keep


# ------------------------------------------------------------------------------------------------ merge
def test_two_half_cohorts_in_two_contexts_merge_to_the_whole(ctx):
    from basevarc_amd import Context
    b, q, _, ranges = dense_case(False)
    bt, qt = dev(b), dev(q)
    parts = [zeros(NS, 512), zeros(NS, 512)]
    with Context(0) as other:
        for i, (lo, hi) in enumerate(ranges):
            (ctx, other)[i % 2].counts_add_dense_device(bt[:, lo:hi], qt[:, lo:hi], parts[i % 2])
        other.synchronize()
    ctx.counts_merge_device(parts[0], parts[1])
    ctx.synchronize()
    assert np.array_equal(words(parts[0]), dense_oracle_counts(False))


def test_merge_wraps_at_two_to_the_32(ctx):
    dst = np.array([0xFFFFFFFF, 5, 0x80000000, 1, 2, 3, 4], dtype=np.uint32)
    src = np.array([1, 7, 0x80000000, 1, 1, 1, 0xFFFFFFFF], dtype=np.uint32)
    want = dst + src
    assert want[0] == 0 and want[2] == 0 and want[6] == 3
    got = dst.copy()
    ctx.counts_merge(got, src)
    assert np.array_equal(got, want)
    # device arrays off the 16-byte boundary, a word count that is no multiple of four
    big = np.random.default_rng(9).integers(0, 1 << 32, (2, 4099), dtype=np.uint64).astype(np.uint32)
    for shift in (0, 1):
        d, s = offset_view(big[0].view(np.int32), shift), offset_view(big[1].view(np.int32), shift)
        ctx.counts_merge_device(d, s)
        ctx.synchronize()
        assert np.array_equal(words(d), big[0] + big[1])


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_and_the_context_stays_usable(ctx):
    L, h = ctx._L, ctx._h
    b = np.zeros((2, 8), dtype=np.int8)
    q = np.full((2, 8), 30, dtype=np.int8)
    lab = np.zeros(8, dtype=np.uint8)
    counts = np.zeros((2, 33, 512), dtype=np.uint32)
    offs = np.array([0, 8, 16], dtype=np.int64)
    ref = np.zeros(2, dtype=np.int8)
    res = np.zeros(2 * 120, dtype=np.uint8)
    gres = np.zeros(2 * 32 * 48, dtype=np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    db, dq, dl, dc, do = dev(b), dev(q), dev(lab), zeros(2, 33, 512), dev(offs)
    d = lambda t: C.c_void_p(t.data_ptr())
    bad_offsets = [np.array([1, 8, 16], dtype=np.int64), np.array([0, 9, 8], dtype=np.int64)]
    refused = {
        # null pointers with work present
        "dense null bases": lambda: L.bvc_counts_add_dense(h, 2, 8, 8, None, p(q), p(counts), HOST),
        "dense null quals": lambda: L.bvc_counts_add_dense(h, 2, 8, 8, d(db), None, d(dc), DEVICE),
        "dense null counts": lambda: L.bvc_counts_add_dense(h, 2, 8, 8, p(b), p(q), None, HOST),
        "packed null rows": lambda: L.bvc_counts_add_dense_packed(h, 2, 8, 8, None, p(counts), HOST),
        "packed null counts": lambda: L.bvc_counts_add_dense_packed(h, 2, 8, 8, d(db), None, DEVICE),
        "csr null offsets": lambda: L.bvc_counts_add_csr(h, 2, None, p(b), p(q), p(counts), HOST),
        "csr null bases": lambda: L.bvc_counts_add_csr(h, 2, p(offs), None, p(q), p(counts), HOST),
        "csr null quals device": lambda: L.bvc_counts_add_csr(h, 2, d(do), d(db), None, d(dc), DEVICE),
        "csr null counts": lambda: L.bvc_counts_add_csr(h, 2, p(offs), p(b), p(q), None, HOST),
        "csr packed null": lambda: L.bvc_counts_add_csr_packed(h, 2, p(offs), None, p(counts), HOST),
        "groups null labels": lambda: L.bvc_counts_add_dense_groups(h, 2, 8, 8, p(b), p(q), None, 5, p(counts), HOST),
        "groups null counts": lambda: L.bvc_counts_add_dense_groups(h, 2, 8, 8, d(db), d(dq), d(dl), 5, None, DEVICE),
        "labels null labels": lambda: L.bvc_counts_add_csr_group_labels(h, 2, p(offs), p(b), p(q), None, 5, p(counts), HOST),
        "labels null labels device": lambda: L.bvc_counts_add_csr_group_labels(h, 2, d(do), d(db), d(dq), None, 5, d(dc), DEVICE),
        "hist_groups null counts": lambda: L.bvc_lrt_hist_groups(h, 2, None, p(ref), MIN_AF, 5, p(res), p(gres), HOST),
        "hist_groups null ref": lambda: L.bvc_lrt_hist_groups(h, 2, p(counts), None, MIN_AF, 5, p(res), p(gres), HOST),
        "hist_groups null results": lambda: L.bvc_lrt_hist_groups(h, 2, p(counts), p(ref), MIN_AF, 5, None, p(gres), HOST),
        "hist_groups null group results": lambda: L.bvc_lrt_hist_groups(h, 2, p(counts), p(ref), MIN_AF, 5, p(res), None, HOST),
        "merge null src": lambda: L.bvc_counts_merge(h, 8, p(counts), None, HOST),
        "merge null dst": lambda: L.bvc_counts_merge(h, 8, None, d(dc), DEVICE),
        # negative sizes
        "dense n_sites < 0": lambda: L.bvc_counts_add_dense(h, -1, 8, 8, p(b), p(q), p(counts), HOST),
        "dense n_samples < 0": lambda: L.bvc_counts_add_dense(h, 2, -1, 8, p(b), p(q), p(counts), HOST),
        "dense stride < n_samples": lambda: L.bvc_counts_add_dense(h, 2, 8, 7, p(b), p(q), p(counts), HOST),
        "packed n_samples < 0": lambda: L.bvc_counts_add_dense_packed(h, 2, -1, 8, p(b), p(counts), HOST),
        "csr n_sites < 0": lambda: L.bvc_counts_add_csr(h, -1, p(offs), p(b), p(q), p(counts), HOST),
        "csr packed n_sites < 0": lambda: L.bvc_counts_add_csr_packed(h, -1, p(offs), p(b), p(counts), HOST),
        "groups n_samples < 0": lambda: L.bvc_counts_add_dense_groups(h, 2, -1, 8, p(b), p(q), p(lab), 5, p(counts), HOST),
        "labels n_sites < 0": lambda: L.bvc_counts_add_csr_group_labels(h, -1, p(offs), p(b), p(q), p(b), 5, p(counts), HOST),
        "hist_groups n_sites < 0": lambda: L.bvc_lrt_hist_groups(h, -1, p(counts), p(ref), MIN_AF, 5, p(res), p(gres), HOST),
        "merge n_words < 0": lambda: L.bvc_counts_merge(h, -1, p(counts), p(counts), HOST),
    }
    for k in (0, 33, -1):                                            # n_groups outside 1..32
        refused[f"groups n_groups {k}"] = lambda k=k: L.bvc_counts_add_dense_groups(h, 2, 8, 8, p(b), p(q), p(lab), k, p(counts), HOST)
        refused[f"labels n_groups {k}"] = lambda k=k: L.bvc_counts_add_csr_group_labels(h, 2, p(offs), p(b), p(q), p(b), k, p(counts), HOST)
        refused[f"labels n_groups {k} device"] = lambda k=k: L.bvc_counts_add_csr_group_labels(h, 2, d(do), d(db), d(dq), d(db), k, d(dc), DEVICE)
        refused[f"hist_groups n_groups {k}"] = lambda k=k: L.bvc_lrt_hist_groups(h, 2, p(counts), p(ref), MIN_AF, k, p(res), p(gres), HOST)
    for i, o in enumerate(bad_offsets):                              # host offsets that do not start at 0 / that decrease
        refused[f"csr offsets {i}"] = lambda o=o: L.bvc_counts_add_csr(h, 2, p(o), p(b), p(q), p(counts), HOST)
        refused[f"csr packed offsets {i}"] = lambda o=o: L.bvc_counts_add_csr_packed(h, 2, p(o), p(b), p(counts), HOST)
        refused[f"labels offsets {i}"] = lambda o=o: L.bvc_counts_add_csr_group_labels(h, 2, p(o), p(b), p(q), p(b), 5, p(counts), HOST)
    for name, call in refused.items():
        assert call() == BVC_ERR_ARG, name
        assert L.bvc_last_error(h), name
    assert not counts.any() and not words(dc).any()
    # nothing to do is not an error: no sites, no columns, no observations, no words
    assert L.bvc_counts_add_dense(h, 0, 8, 8, None, None, None, HOST) == BVC_OK
    assert L.bvc_counts_add_dense(h, 2, 0, 0, None, None, p(counts), HOST) == BVC_OK
    assert L.bvc_counts_add_csr(h, 2, p(np.zeros(3, dtype=np.int64)), None, None, p(counts), HOST) == BVC_OK
    assert L.bvc_counts_merge(h, 0, None, None, HOST) == BVC_OK
    # and the context still works
    flat = counts[:, 0, :].copy()
    ctx.counts_add_dense(b, q, flat)
    assert flat[0, 30] == 8 and flat[1, 30] == 8 and flat.sum() == 16
