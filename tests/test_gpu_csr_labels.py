"""bvc_lrt_csr_group_labels / bvc_lrt_csr_group_labels_packed (GPU): the ragged group call with ONE label byte per observation.

Every comparison is byte identity of the records with bvc_lrt_csr_groups on the same observations with
group_of_obs[i] = group_of_sample[sample_of_obs[i]]; tests/test_gpu_round5.py ties that call to the dense group call and to the
oracle's group loop.  No tolerance appears anywhere.  hist_csr_labels_kernel reads a site with aligned 4-byte loads where the three
arrays agree on the alignment of the site's first byte (two steps of 512 x 4 observations in flight, then single steps, up to three
observations in front and behind) and with byte loads where they do not (four steps of 512 in flight, then single steps): the site
lengths and the alignments below walk through every one of those boundaries on both paths.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import emit_oracle as eo
from tests.test_gpu_pileup_bin import encode, sample0_of
from tests.test_gpu_round5 import random_token, reference_columns, tile_of

pytestmark = pytest.mark.gpu

BVC_OK, BVC_ERR_ARG = 0, -1
BVC_PTR_HOST = 0
MIN_AF = 0.001
N_SAMPLES = 6000
LENGTHS = [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 0, 7]


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def site_obs(rng, n):
    """One site's observations as tests/test_gpu_round5.py ragged_group_case draws them, the samples with repetition."""
    who = rng.integers(0, N_SAMPLES, n).astype(np.int32)
    ref = int(rng.integers(0, 4))
    af = float(rng.choice([0.0, 0.0, 0.02, 0.3]))
    alt = (ref + 1 + int(rng.integers(0, 3))) % 4
    b = np.where(rng.random(n) < af, alt, ref).astype(np.int8)
    q = rng.integers(5, 42, n).astype(np.int8)
    err = rng.random(n) < 10.0 ** (-q / 10.0)
    b[err] = (b[err] + 1 + rng.integers(0, 3, int(err.sum()))) % 4
    return who, b, q, ref


def columns(sites):
    offs = np.concatenate([[0], np.cumsum([len(w) for w, _, _, _ in sites])]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([s[i] for s in sites] + [np.zeros(0, dt)]).astype(dt)
    return offs, cat(1, np.int8), cat(2, np.int8), cat(0, np.int32), np.array([r for _, _, _, r in sites], dtype=np.int8)


def labels_of(k, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, k, N_SAMPLES).astype(np.uint8)
    labels[rng.random(N_SAMPLES) < 0.1] = 255
    return labels


@functools.lru_cache(maxsize=None)
def boundary_case(k):
    """(offsets, bases, quals, samples, ref, group_of_sample, group_of_obs) of case 1; never modified by its users."""
    rng = np.random.default_rng(500 + k)
    sites = [site_obs(rng, n) for n in LENGTHS + rng.integers(0, 301, 40).tolist()]
    offs, b, q, smp, ref = columns(sites)
    for v in (4, 5, -1):                                             # entries that are no A/C/G/T, qualities that are none
        b[rng.integers(0, len(b), 9)] = v
    q[rng.integers(0, len(q), 9)] = -1
    labels = labels_of(k, 600 + k)
    out = (offs, b, q, smp, ref, labels, labels[smp])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def boundary_reference(ctx, k):
    """bvc_lrt_csr_groups on case 1, computed once per k: (results bytes, group results bytes, results, group results)."""
    offs, b, q, smp, ref, labels, _ = boundary_case(k)
    res, gres = ctx.lrt_csr_groups(offs, b, q, smp, ref, MIN_AF, labels, k)
    return res.tobytes(), gres.tobytes(), res, gres


def device(*arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


def device_bytes(ctx, res_t, gres_t):
    from basevarc_amd.lib import results_from_tensor
    ctx.synchronize()
    return results_from_tensor(res_t).tobytes(), gres_t.cpu().numpy().tobytes()


def offset_view(a, shift):
    """The bytes of `a` on the device, `shift` bytes behind the start of their own allocation."""
    import torch
    t = torch.zeros(len(a) + 4, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    v = t[shift:shift + len(a)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() == t.data_ptr() + shift
    return v


# ------------------------------------------------------------------------------------------------ 1. every loop boundary
@pytest.mark.parametrize("k", [1, 5, 32])
def test_site_lengths_around_every_loop_boundary(ctx, k):
    offs, b, q, smp, ref, labels, lab = boundary_case(k)
    want_r, want_g, res, gres = boundary_reference(ctx, k)
    assert int(res["called"].sum()) > 5 and int(gres["ran"].sum()) > 5          # not a comparison of empty records
    got, ggot = ctx.lrt_csr_group_labels(offs, b, q, lab, ref, MIN_AF, k)
    assert got.tobytes() == want_r and ggot.tobytes() == want_g
    # device pointers, each form against its twin
    d = device(offs, b, q, smp, ref, labels, lab)
    twin = device_bytes(ctx, *ctx.lrt_csr_groups_device(d[0], d[1], d[2], d[3], d[4], MIN_AF, d[5], k))
    assert twin == (want_r, want_g)
    assert device_bytes(ctx, *ctx.lrt_csr_group_labels_device(d[0], d[1], d[2], d[6], d[4], MIN_AF, k)) == twin


# ------------------------------------------------------------------------------------------------ 2. every alignment
def test_every_alignment_of_a_sites_start_and_of_the_three_arrays(ctx):
    k = 5
    rng = np.random.default_rng(7)
    labels = labels_of(k, 8)
    body = [site_obs(rng, 513), site_obs(rng, 2049)]
    lead = site_obs(rng, 16)
    called = 0
    for a in range(17):
        sites = [tuple(x[:a] if isinstance(x, np.ndarray) else x for x in lead)] + body
        offs, b, q, smp, ref = columns(sites)
        lab = labels[smp]
        res, gres = ctx.lrt_csr_groups(offs, b, q, smp, ref, MIN_AF, labels, k)
        want = (res.tobytes(), gres.tobytes())
        called += int(res["called"].sum())
        got, ggot = ctx.lrt_csr_group_labels(offs, b, q, lab, ref, MIN_AF, k)
        assert (got.tobytes(), ggot.tobytes()) == want, a
        # arrays allocated alike: the sites start at byte a, 513 + a, ... of all three (the 4-byte loads, every head and tail)
        d = device(offs, ref, b, q, lab)
        assert device_bytes(ctx, *ctx.lrt_csr_group_labels_device(d[0], d[2], d[3], d[4], d[1], MIN_AF, k)) == want, a
        # arrays 1, 2 and 3 bytes behind their allocations: no common alignment (the byte loads)
        vb, vq, vl = offset_view(b, 1), offset_view(q, 2), offset_view(lab, 3)
        assert device_bytes(ctx, *ctx.lrt_csr_group_labels_device(d[0], vb, vq, vl, d[1], MIN_AF, k)) == want, a
        # the packed form has two arrays: alike, and one byte apart
        pk = (b.astype(np.uint8) << 6 | q.astype(np.uint8)).astype(np.uint8)
        dp = device(pk)[0]
        assert device_bytes(ctx, *ctx.lrt_csr_group_labels_packed_device(d[0], dp, d[4], d[1], MIN_AF, k)) == want, a
        assert device_bytes(ctx, *ctx.lrt_csr_group_labels_packed_device(d[0], offset_view(pk, 2), vl, d[1], MIN_AF, k)) == want, a
    assert called > 5


# ------------------------------------------------------------------------------------------------ 3. label values
@pytest.mark.parametrize("k", [2, 32])
def test_every_label_of_n_groups_and_above_is_in_no_group(ctx, k):
    """As test_csr_groups_sample_indices_outside_the_label_vector_are_in_no_group: depths written out by hand."""
    offs = np.array([0, 6], dtype=np.int64)
    b = np.array([0, 0, 1, 1, 0, 1], dtype=np.int8); q = np.full(6, 30, dtype=np.int8)
    lab = np.array([0, k - 1, k, k + 1, 254, 255], dtype=np.uint8)
    pk = (b.astype(np.uint8) << 6 | 30).astype(np.uint8)
    for res, gres in (ctx.lrt_csr_group_labels(offs, b, q, lab, np.zeros(1, np.int8), MIN_AF, k),
                      ctx.lrt_csr_group_labels_packed(offs, pk, lab, np.zeros(1, np.int8), MIN_AF, k)):
        assert res[0]["depth"].tolist() == [3, 3, 0, 0]
        assert gres[0, 0]["depth"].tolist() == [1, 0, 0, 0] and gres[0, k - 1]["depth"].tolist() == [1, 0, 0, 0]
        assert gres[0, 1:k - 1]["depth"].sum() == 0 and gres[0]["depth"].sum() == 2


# ------------------------------------------------------------------------------------------------ 4. the packed form
def test_packed_form_gives_the_records_of_the_unpacked_form(ctx):
    k = 5
    offs, b, q, smp, ref, labels, lab = boundary_case(k)
    want_r, want_g, res, _ = boundary_reference(ctx, k)
    skipped = (b < 0) | (b > 3) | (q < 0)
    qc = np.minimum(q, 62)                                           # (the case's qualities are below 42: the records do not change)
    pk = np.where(skipped, 0xFF, (b.astype(np.uint8) << 6) | qc.astype(np.uint8)).astype(np.uint8)
    assert skipped.sum() > 20
    got, ggot = ctx.lrt_csr_group_labels_packed(offs, pk, lab, ref, MIN_AF, k)
    assert got.tobytes() == want_r and ggot.tobytes() == want_g
    d = device(offs, pk, lab, ref)
    assert device_bytes(ctx, *ctx.lrt_csr_group_labels_packed_device(d[0], d[1], d[2], d[3], MIN_AF, k)) == (want_r, want_g)
    # quality bits 63 = no observation: one covered observation less in that site, every other site as before
    site = LENGTHS.index(513)
    at = int(offs[site]) + 100
    while skipped[at]:
        at += 1
    pk2 = pk.copy(); pk2[at] |= 63
    got2, _ = ctx.lrt_csr_group_labels_packed(offs, pk2, lab, ref, MIN_AF, k)
    assert int(got2[site]["depth"].sum()) == int(res[site]["depth"].sum()) - 1
    others = np.arange(len(res)) != site
    assert got2[others].tobytes() == res[others].tobytes()


# ------------------------------------------------------------------------------------------------ 5. the producer
@pytest.mark.parametrize("form", ["text", "bin"])
def test_device_parse_with_groups_equals_the_label_call_on_its_columns(ctx, form):
    """bvc_pileup_finish with n_groups > 0 = the parse + the ragged group call on its columns.  The device parser writes the label
    byte of every observation itself and finishes with the label form; this test holds for either form behind the
    producer, since both give the same records: it would pass unchanged with the producer on the sample-index path."""
    rng = np.random.default_rng(9)
    n_in_batch = np.array([200, 200, 77], dtype=np.int32)
    N = int(n_in_batch.sum())
    labels = rng.integers(0, 4, N).astype(np.uint8); labels[::13] = 255
    T = 60
    batch_tokens = [[[random_token(rng, 0.5, 0.02) for _ in range(n)] for _ in range(T)] for n in n_in_batch]
    lines, records, rs, _ = encode(batch_tokens)
    ref = rng.integers(0, 4, T).astype(np.int8)
    s0 = sample0_of(n_in_batch)
    if form == "text":
        text, ls = tile_of(lines)
        run = lambda g: ctx.pileup_tile(text, ls, s0, n_in_batch, ref, MIN_AF, group_of_sample=g, n_groups=3)
    else:
        run = lambda g: ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, MIN_AF, group_of_sample=g, n_groups=3)
    offs, bb, qq, ss = [0], [], [], []
    for aiv, sample in reference_columns(lines, eo.Parser()):
        for a, j in zip(aiv, sample):
            if not a["is_indel"]:
                bb.append(a["base"]); qq.append(a["qual"]); ss.append(j)
        offs.append(len(bb))
    offs, bb, qq, ss = np.array(offs, np.int64), np.array(bb, np.int8), np.array(qq, np.int8), np.array(ss, np.int32)
    out = run(labels)
    res, gres = ctx.lrt_csr_group_labels(offs, bb, qq, labels[ss], ref, MIN_AF, 3)
    assert out["results"].tobytes() == res.tobytes() and out["grp_results"].tobytes() == gres.tobytes()
    assert res["called"].sum() > 5 and gres["ran"].sum() > 5
    # a label vector of 300 samples: the third batch's samples lie outside it and are in no group
    out = run(labels[:300])
    res2, gres2 = ctx.lrt_csr_groups(offs, bb, qq, ss, ref, MIN_AF, labels[:300], 3)
    assert (ss >= 300).sum() > 100 and gres2.tobytes() != gres.tobytes()
    assert out["results"].tobytes() == res2.tobytes() and out["grp_results"].tobytes() == gres2.tobytes()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refused_arguments_leave_the_context_usable(ctx):
    from basevarc_amd.lib import GROUP_DTYPE, SITE_DTYPE
    L, h = ctx._L, ctx._h
    offs = np.array([0, 6], dtype=np.int64)
    b = np.array([0, 0, 1, 1, 0, 1], dtype=np.int8); q = np.full(6, 30, dtype=np.int8)
    pk = (b.astype(np.uint8) << 6 | 30).astype(np.uint8)
    lab = np.array([0, 1, 2, 3, 254, 255], dtype=np.uint8)
    ref = np.zeros(1, np.int8)
    res = np.zeros(1, dtype=SITE_DTYPE); gres = np.zeros((1, 33), dtype=GROUP_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def unpacked(n_sites=1, o=offs, labels=p(lab), k=2, g=p(gres)):
        return L.bvc_lrt_csr_group_labels(h, n_sites, p(o), p(b), p(q), labels, p(ref), MIN_AF, k, p(res), g, BVC_PTR_HOST)

    def packed(n_sites=1, o=offs, labels=p(lab), k=2, g=p(gres)):
        return L.bvc_lrt_csr_group_labels_packed(h, n_sites, p(o), p(pk), labels, p(ref), MIN_AF, k, p(res), g, BVC_PTR_HOST)

    def still_right():
        for r, g in (ctx.lrt_csr_group_labels(offs, b, q, lab, ref, MIN_AF, 2), ctx.lrt_csr_group_labels_packed(offs, pk, lab, ref, MIN_AF, 2)):
            assert r[0]["depth"].tolist() == [3, 3, 0, 0]
            assert g[0, 0]["depth"].tolist() == [1, 0, 0, 0] and g[0, 1]["depth"].tolist() == [1, 0, 0, 0]

    still_right()
    for call in (unpacked, packed):
        for bad in (dict(k=0), dict(k=33), dict(labels=None), dict(g=None), dict(o=np.array([1, 7], dtype=np.int64))):
            assert call(**bad) == BVC_ERR_ARG, (call.__name__, sorted(bad))
            still_right()
        assert call(n_sites=0, o=np.array([0], dtype=np.int64)) == BVC_OK
        assert call() == BVC_OK
    still_right()
