"""The VCF sample columns formatted on the device (bvc_vcf_samples_csr; GPU).

Every byte of every called site's text is compared `==` with the plain Python model of tests/vcf_samples_cases.py and with the host
program's own columns (bvchost_vcf_samples); the offsets and lengths with the slot formula of include/bvc.h.  The text buffers are
prefilled with a guard byte: nothing outside the slots may change.  The `results` records are made by the tests (called, n_alt,
alt_base): nothing here depends on the LRT."""
import ctypes as C

import numpy as np
import pytest

from tests import vcf_samples_cases as vc

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1
GUARD = 0xA7


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    return vc.host_library()


@pytest.fixture(scope="module")
def catalogue(host):
    """n -> (sites, packed arrays, the model's text per site); the model is held against the host program's columns once, here."""
    out = {}
    for n in vc.SIZES:
        sites = vc.sites_of(n)
        want = vc.model_of(n, sites)
        for s, w in zip(sites[::5], want[::5]):                    # (every site: tests/test_vcf_samples_abi.py, without a device)
            if int(s[4]["called"]) and vc.host_defined(s[4]):
                assert vc.host_columns(host, n, s[1], s[2], s[3], s[4]) == w, (n, s[0])
        out[n] = (sites, vc.pack(sites), want)
    return out


def check_text(n, arrays, want, text, off, ln, where):
    """Offsets, lengths, every called site's bytes, and the guard behind the slots."""
    from basevarc_amd.lib import vcf_samples_slot
    offsets, _, _, _, results = arrays
    text = np.asarray(text)
    at = 0
    for s in range(len(want)):
        assert int(off[s]) == at, (where, s)
        if int(results[s]["called"]):
            assert int(ln[s]) == len(want[s]), (where, s, int(ln[s]), len(want[s]))
            got = text[at:at + len(want[s])].tobytes()
            if got != want[s]:
                first = next(i for i in range(len(got)) if got[i] != want[s][i])
                raise AssertionError((where, s, first, got[max(0, first - 20):first + 20], want[s][max(0, first - 20):first + 20]))
            at += vcf_samples_slot(n, int(offsets[s + 1] - offsets[s]))
        else:
            assert int(ln[s]) == 0, (where, s)
    assert int(off[len(want)]) == at, where
    assert (text[at:] == GUARD).all(), (where, "bytes behind the slots were written")
    return at


def device_call(ctx, n, arrays, shift=0, slack=64, cap=None):
    """bvc_vcf_samples_csr with BVC_PTR_DEVICE on torch memory; entries and samples start `shift` elements into their allocations."""
    import torch
    from basevarc_amd.lib import vcf_samples_need
    offsets, entries, samples, refs, results = arrays

    def raw(a, pad):
        b = np.concatenate([np.zeros(pad, dtype=np.uint8), np.frombuffer(a.tobytes(), dtype=np.uint8)])
        return torch.from_numpy(b.copy()).to("cuda:0")[pad:]
    need = vcf_samples_need(n, offsets, results)
    o_t = torch.from_numpy(offsets.copy()).to("cuda:0")
    e_t, s_t = raw(entries, 8 * shift), raw(samples, 4 * shift)
    r_t, res_t = raw(refs, shift), raw(results, 8 * shift)
    text_t = torch.full((need + slack,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert text_t.data_ptr() % 16 == 0
    text_t, off_t, len_t = ctx.vcf_samples_csr_device(o_t, e_t, s_t, r_t, res_t, n, text_t, text_cap=cap)
    ctx.synchronize()
    return text_t.cpu().numpy(), off_t.cpu().numpy(), len_t.cpu().numpy()[:len(refs)]


# ------------------------------------------------------------------------------------------------------------------ the catalogue
@pytest.mark.parametrize("n", vc.SIZES)
def test_the_catalogue_with_host_pointers(ctx, catalogue, n):
    from basevarc_amd.lib import vcf_samples_need
    sites, arrays, want = catalogue[n]
    need = vcf_samples_need(n, arrays[0], arrays[4])
    text = np.full(need + 64, GUARD, dtype=np.uint8)
    text, off, ln = ctx.vcf_samples_csr(*arrays[:4], arrays[4], n, text=text, text_cap=need)       # (exactly the sum of the slots)
    assert check_text(n, arrays, want, text, off, ln, f"host n={n}") == need


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [5, vc.T - 1, vc.T + 1, 2 * vc.T + 1])
def test_the_catalogue_with_device_pointers_at_any_element(ctx, catalogue, n, shift):
    sites, arrays, want = catalogue[n]
    text, off, ln = device_call(ctx, n, arrays, shift)
    check_text(n, arrays, want, text, off, ln, f"device n={n} shift={shift}")


@pytest.mark.parametrize("n", [1, 2, 3, 4, vc.T, 2 * vc.T])
def test_the_catalogue_with_device_pointers(ctx, catalogue, n):
    sites, arrays, want = catalogue[n]
    text, off, ln = device_call(ctx, n, arrays)
    check_text(n, arrays, want, text, off, ln, f"device n={n}")


def test_page_locked_and_pageable_text_buffers_hold_the_same_bytes(ctx, catalogue):
    from basevarc_amd.lib import vcf_samples_need
    n = vc.T + 1
    sites, arrays, want = catalogue[n]
    need = vcf_samples_need(n, arrays[0], arrays[4])
    addr, pinned = ctx.host_alloc(need + 64)
    try:
        pinned[:] = GUARD
        text, off, ln = ctx.vcf_samples_csr(*arrays[:4], arrays[4], n, text=pinned, text_cap=need)
        assert text.ctypes.data == addr
        check_text(n, arrays, want, text, off, ln, "page-locked text")
        # entries and samples from page-locked memory too
        e_addr, e_mem = ctx.host_alloc(max(1, arrays[1].nbytes))
        s_addr, s_mem = ctx.host_alloc(max(1, arrays[2].nbytes))
        try:
            e_mem[:arrays[1].nbytes] = np.frombuffer(arrays[1].tobytes(), dtype=np.uint8)
            s_mem[:arrays[2].nbytes] = np.frombuffer(arrays[2].tobytes(), dtype=np.uint8)
            e = e_mem[:arrays[1].nbytes].view(arrays[1].dtype)
            s = s_mem[:arrays[2].nbytes].view(np.int32)
            pinned[:] = GUARD
            text, off, ln = ctx.vcf_samples_csr(arrays[0], e, s, arrays[3], arrays[4], n, text=pinned, text_cap=need)
            check_text(n, arrays, want, text, off, ln, "page-locked everything")
        finally:
            ctx.host_free(e_addr); ctx.host_free(s_addr)
    finally:
        ctx.host_free(addr)


# ------------------------------------------------------------------------------------------------------------------ the larger calls
def random_sites(rng, n, n_sites, coverage, called_p):
    """n_sites sites of n samples at the given coverage; the uncalled ones carry poison (entries 0xFF, samples out of order)."""
    from basevarc_amd.lib import SITE_DTYPE
    sites = []
    for s in range(n_sites):
        if rng.random() < called_p:
            k = int(rng.binomial(n, coverage))
            at = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
            res = vc.make_result(1, int(rng.integers(0, 4)), tuple(int(x) for x in rng.integers(0, 4, 3)))
            sites.append((f"site {s}", at, vc.make_entries(k, rng), int(rng.integers(-1, 5)), res))
        else:
            k = int(rng.integers(0, 9))
            poison = np.frombuffer(b"\xff" * (8 * k), dtype=vc.make_entries(0).dtype).copy()
            sites.append((f"uncalled {s}", np.full(k, 2 ** 31 - 1, dtype=np.int32), poison, 0, vc.make_result(0, 3, (1, 2, 3))))
    return sites


def test_three_thousand_sites_so_the_grid_strides(ctx, host):
    n = 257
    rng = np.random.default_rng(3000)
    sites = random_sites(rng, n, 3000, 0.3, 0.8)
    arrays = vc.pack(sites)
    want = vc.model_of(n, sites)
    for s, w in list(zip(sites, want))[::100]:
        if int(s[4]["called"]):
            assert vc.host_columns(host, n, s[1], s[2], s[3], s[4]) == w
    text, off, ln = device_call(ctx, n, arrays)
    check_text(n, arrays, want, text, off, ln, "3000 sites, device")
    htext = np.full(int(off[-1]) + 16, GUARD, dtype=np.uint8)
    htext, hoff, hln = ctx.vcf_samples_csr(*arrays[:4], arrays[4], n, text=htext)
    check_text(n, arrays, want, htext, hoff, hln, "3000 sites, host")


def test_one_site_of_a_million_and_three_samples(ctx, host):
    n = 1_000_003
    rng = np.random.default_rng(1000003)
    at = np.flatnonzero(rng.random(n) < 0.1).astype(np.int32)
    at = np.union1d(at, [0, n - 1]).astype(np.int32)
    e = vc.make_entries(len(at), rng)
    res = vc.make_result(1, 2, (2, 3, -1))
    sites = [("poison in front", np.full(3, -1, np.int32), vc.make_entries(3, rng), 1, vc.make_result(0)), ("the site", at, e, 0, res)]
    arrays = vc.pack(sites)
    # the reference here is the host program's text (the Python model walks a million fields: the catalogue is where it is held to it)
    want = [b"", vc.host_columns(host, n, at, e, 0, res)]
    assert len(want[1]) == 4 * n + 13 * len(at) - 1 and want[1].startswith(b"0/.:" if int(e["base"][0]) & 7 == 0 else b"./")
    text, off, ln = device_call(ctx, n, arrays, shift=1)
    check_text(n, arrays, want, text, off, ln, "a million samples")


# ------------------------------------------------------------------------------------------------------------------ calls the library refuses
def test_refusals_leave_the_context_usable(ctx, catalogue):
    import torch
    from basevarc_amd.lib import BvcError, vcf_samples_need
    n = vc.T + 1
    sites, arrays, want = catalogue[n]
    offsets, entries, samples, refs, results = arrays
    ns = len(refs)
    need = vcf_samples_need(n, offsets, results)
    text = np.full(need + 64, GUARD, dtype=np.uint8)
    off, ln = np.zeros(ns + 1, np.int64), np.zeros(ns, np.int64)
    L, h = ctx._L, ctx._h
    p = lambda a: C.c_void_p(a.ctypes.data)
    good = [p(offsets), p(entries), p(samples), p(refs), p(results), n, p(text), need, p(off), p(ln)]
    for k in (0, 1, 2, 3, 4, 6, 8, 9):                             # every null pointer with work present
        args = list(good)
        args[k] = None
        assert L.bvc_vcf_samples_csr(h, ns, *args, 0) == BVC_ERR_ARG, k
        assert L.bvc_vcf_samples_csr(h, ns, *args, 1) == BVC_ERR_ARG, k
    for flags in (0, 1):
        assert L.bvc_vcf_samples_csr(h, -1, *good, flags) == BVC_ERR_ARG
        args = list(good); args[5] = -1
        assert L.bvc_vcf_samples_csr(h, ns, *args, flags) == BVC_ERR_ARG
        args = list(good); args[7] = -1
        assert L.bvc_vcf_samples_csr(h, ns, *args, flags) == BVC_ERR_ARG
    bad = offsets.copy(); bad[3] = bad[2] - 1
    assert L.bvc_vcf_samples_csr(h, ns, p(bad), *good[1:], 0) == BVC_ERR_ARG
    bad = offsets.copy(); bad[0] = 1
    assert L.bvc_vcf_samples_csr(h, ns, p(bad), *good[1:], 0) == BVC_ERR_ARG
    # one byte short: refused, the need is named, nothing is written
    args = list(good); args[7] = need - 1
    assert L.bvc_vcf_samples_csr(h, ns, *args, 0) == BVC_ERR_ARG
    assert str(need).encode() in L.bvc_last_error(h)
    assert (text == GUARD).all()
    with pytest.raises(BvcError) as err:
        device_call(ctx, n, arrays, cap=need - 1)
    assert err.value.status == BVC_ERR_ARG and str(need) in str(err.value)
    # device text off a 16-byte boundary
    t = torch.full((need + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    o_t = torch.from_numpy(offsets.copy()).to("cuda:0")
    with pytest.raises(BvcError):
        ctx.vcf_samples_csr_device(o_t, o_t, o_t, o_t, o_t, n, t[1:])
    assert L.bvc_vcf_samples_csr(h, 0, None, None, None, None, None, n, None, 0, p(off), None, 0) == 0      # no work: only text_off[0]
    assert off[0] == 0
    text, off, ln = ctx.vcf_samples_csr(*arrays[:4], arrays[4], n, text=text, text_cap=need)
    check_text(n, arrays, want, text, off, ln, "after the refusals")
    text, off, ln = device_call(ctx, n, arrays)
    check_text(n, arrays, want, text, off, ln, "after the refusals, device")


def test_overlap_mode_after_join(catalogue):
    """The records come from an LRT of the same context in overlap mode: after bvc_join the call reads them complete."""
    import torch
    from basevarc_amd import Context
    from basevarc_amd.lib import SITE_DTYPE, vcf_samples_need
    n = 300
    rng = np.random.default_rng(11)
    with Context(0) as c:
        c.set_overlap(True)
        bases = rng.choice([0, 1, -1], (6, n), p=[0.25, 0.15, 0.6]).astype(np.int8)
        bases[4:] = np.where(bases[4:] == 1, 0, bases[4:])         # two sites without an alternative allele: not called
        quals = np.full((6, n), 35, dtype=np.int8)
        ref = np.zeros(6, dtype=np.int8)
        b_t, q_t, r_t = (torch.from_numpy(x).to("cuda:0") for x in (bases, quals, ref))
        res_t = c.lrt_dense_device(b_t, q_t, r_t, 0.001)
        c.join()
        sites = []
        for s in range(6):
            at = np.flatnonzero(bases[s] >= 0).astype(np.int32)
            sites.append((f"site {s}", at, vc.make_entries(len(at), rng, base=bases[s][at], qual=35), 0, None))
        offsets = np.concatenate([[0], np.cumsum([len(s[1]) for s in sites])]).astype(np.int64)
        entries = np.concatenate([s[2] for s in sites])
        samples = np.concatenate([s[1] for s in sites])
        o_t, s_t = torch.from_numpy(offsets).to("cuda:0"), torch.from_numpy(samples).to("cuda:0")
        e_t = torch.from_numpy(np.frombuffer(entries.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
        text_t = torch.full((6 * (4 * n + 13 * n + 16) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        text_t, off_t, len_t = c.vcf_samples_csr_device(o_t, e_t, s_t, r_t, res_t, n, text_t)
        c.synchronize()
        results = np.frombuffer(res_t.cpu().numpy().tobytes(), dtype=SITE_DTYPE)
        assert results["called"][:4].all()
        full = [(s[0], s[1], s[2], 0, results[i]) for i, s in enumerate(sites)]
        arrays = (offsets, entries, samples, ref, results)
        assert int(off_t[-1]) == vcf_samples_need(n, offsets, results)
        check_text(n, arrays, vc.model_of(n, full), text_t.cpu().numpy(), off_t.cpu().numpy(), len_t.cpu().numpy()[:6], "overlap mode")
