"""The called sites' rank-sum and strand statistics on the device (bvc_site_stats_csr, bvc_pileup_finish_called_stats; GPU).

Every field of every record is compared `==` with an integer model: the ref / alt classification of include/bvc.h in numpy, one
`bincount` per field and class, a descending cumulative sum and Python integers for 2 x rankR1 = sum r[v] (2 lo + r[v] + a[v] + 1).
The tests make the `results` records themselves (called, n_alt, alt_base): nothing here depends on the LRT, except the producer tests,
which take the records the tile's own LRT wrote."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_pileup_bin import encode, fuzz_tiles, sample0_of
from tests.test_gpu_round5 import tile_of

pytestmark = pytest.mark.gpu

BVC_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------ the model
def rank2_model(ref, alt):
    r = np.bincount(ref.astype(np.int64), minlength=256)[::-1]
    a = np.bincount(alt.astype(np.int64), minlength=256)[::-1]
    m = r + a
    lo = np.cumsum(m) - m
    return sum(int(r[i]) * (2 * int(lo[i]) + int(r[i]) + int(a[i]) + 1) for i in np.nonzero(r)[0])


def model_site(e, ref, res):
    """The record of one site as a tuple (rank2 x 3, n_ref, n_alt, ref_fwd, ref_rev, alt_fwd, alt_rev, valid)."""
    if not int(res["called"]):
        return (0,) * 10
    base = e["base"].astype(np.int64)
    counted = (e["is_indel"] != 1) & (base <= 3)
    is_ref = counted & (base == int(ref)) if 0 <= int(ref) <= 3 else np.zeros(len(e), bool)
    alts = [int(res["alt_base"][i]) for i in range(min(int(res["n_alt"]), 3))]
    is_alt = counted & ~is_ref & np.isin(base, [a for a in alts if 0 <= a <= 3])
    fwd = e["strand"] == 1
    ranks = tuple(rank2_model(e[f][is_ref], e[f][is_alt]) for f in ("mapq", "qual", "rpr"))
    return ranks + (int(is_ref.sum()), int(is_alt.sum()), int((is_ref & fwd).sum()), int((is_ref & ~fwd).sum()),
                    int((is_alt & fwd).sum()), int((is_alt & ~fwd).sum()), 1)


def record_tuple(s):
    return tuple(int(x) for x in s["rank2"]) + tuple(int(s[f]) for f in ("n_ref", "n_alt", "ref_fwd", "ref_rev", "alt_fwd", "alt_rev", "valid"))


def check_stats(stats, offsets, entries, refs, results, where=""):
    from basevarc_amd.lib import STATS_DTYPE
    assert stats.dtype == STATS_DTYPE and len(stats) == len(refs)
    for s in range(len(refs)):
        want = model_site(entries[offsets[s]:offsets[s + 1]], refs[s], results[s])
        assert record_tuple(stats[s]) == want, (where, s, int(offsets[s + 1] - offsets[s]))
        if not int(results[s]["called"]):
            assert stats[s].tobytes() == bytes(64), (where, s)
        assert bytes(stats[s]["pad"]) == bytes(15), (where, s)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def random_entries(rng, n, kind="random"):
    from basevarc_amd.lib import ENTRY_DTYPE
    e = np.zeros(n, dtype=ENTRY_DTYPE)
    # bases 0..3, N (4) and the two codes beyond; a tenth of the entries are indel entries; both strands
    e["base"] = rng.choice([0, 1, 2, 3, 4, 5, 7], n, p=[0.4, 0.2, 0.15, 0.15, 0.05, 0.03, 0.02])
    e["strand"] = rng.integers(0, 2, n)
    e["is_indel"] = rng.random(n) < 0.1
    if kind == "equal":
        e["mapq"] = 60; e["qual"] = 60; e["rpr"] = 60
    elif kind == "all_values":
        for f in ("mapq", "qual", "rpr"):
            e[f] = rng.permutation(np.arange(n) % 256)
    else:
        e["mapq"] = np.where(rng.random(n) < 0.8, 60, rng.integers(0, 256, n))     # mostly one value, as mapping qualities are
        e["qual"] = rng.integers(0, 256, n)
        e["rpr"] = rng.integers(0, 256, n)
        if n >= 2:
            e["mapq"][0] = 0; e["mapq"][1] = 255; e["rpr"][0] = 255; e["qual"][1] = 0
    e["pad"] = rng.integers(0, 65536, n)                           # (nobody reads it)
    return e


def big_case(parity):
    """Called sites of every length at which the kernel takes another path, each starting at an entry index of the given parity; in
    front of each an UNCALLED site (random entries that must not be read into any record) that sets that parity."""
    from basevarc_amd.lib import SITE_DTYPE, SITE_STATS_TRIP as W
    rng = np.random.default_rng(1000 + parity)
    sizes = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 70001]
    plan = [(n, "random") for n in sizes] + [(50000, "equal"), (50000, "all_values"), (300, "no_ref"), (300, "no_alt"), (300, "ref_none")]
    parts, lens, refs = [], [], []
    res = np.zeros(2 * len(plan), dtype=SITE_DTYPE)
    at = 0
    for k, (n, kind) in enumerate(plan):
        fill = int(rng.integers(0, 40)) * 2 + ((at + parity) & 1)  # the called site then starts at an index of `parity`
        parts.append(random_entries(rng, fill)); lens.append(fill); refs.append(int(rng.integers(0, 4)))
        res[2 * k]["n_alt"] = 2; res[2 * k]["alt_base"] = (1, 2, 3)    # an uncalled record may say anything
        at += fill
        assert (at & 1) == parity
        e = random_entries(rng, n, kind if kind in ("equal", "all_values") else "random")
        r = res[2 * k + 1]
        r["called"] = 1 + (k % 3)                                  # any non-zero byte
        ref = k % 4
        n_alt = 1 + k % 3
        alt = [(ref + 1 + i) % 4 for i in range(3)]
        if kind == "no_ref":
            e["base"][e["base"] == ref] = alt[0]
        elif kind == "no_alt":
            n_alt = 1
            e["base"][e["base"] == alt[0]] = ref
        elif kind == "ref_none":
            ref = -1
        if k == 5:
            n_alt = 5                                              # read as 3
        r["n_alt"] = n_alt
        r["alt_base"] = alt if n_alt >= 3 else alt[:n_alt] + [-1] * (3 - n_alt)
        parts.append(e); lens.append(n); refs.append(ref)
        at += n
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offsets, np.concatenate(parts), np.array(refs, dtype=np.int8), res


@pytest.fixture(scope="module")
def cases():
    return {p: big_case(p) for p in (0, 1)}


@pytest.mark.parametrize("pointers", ["host", "device", "device_shifted"])
@pytest.mark.parametrize("parity", [0, 1])
def test_every_field_equals_the_integer_model(ctx, cases, parity, pointers):
    from basevarc_amd.lib import SITE_STATS_TRIP as W
    offsets, entries, refs, results = cases[parity]
    lens = np.diff(offsets)[results["called"] != 0]
    assert {0, 1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 70001} <= set(int(x) for x in lens)
    assert all((int(offsets[s]) & 1) == parity for s in range(len(refs)) if results[s]["called"])
    if pointers == "host":
        stats = ctx.site_stats_csr(offsets, entries, refs, results)
    else:
        stats = device_call(ctx, offsets, entries, refs, results, 1 if pointers == "device_shifted" else 0)
    check_stats(stats, offsets, entries, refs, results, where=f"{pointers} parity {parity}")
    called = results["called"] != 0
    assert stats["valid"][called].all() and (stats["n_ref"][called] > 0).any() and (stats["n_alt"][called] > 0).any()


STATS_COPIES_DEFAULT = 2                            # tuning key "stats_copies_log2" (include/bvc.h): 2^n copies of a workgroup's counters


class copies:
    """The shared context with stats_copies_log2 = n, and the default again afterwards.  3 and 4 take more than 48 KB of LDS a workgroup
    (site_stats_lds_bytes: 6,416 bytes + 6,144 x 2^n), the branch of launch_site_stats that raises the kernel's limit first."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n

    def __enter__(self):
        self.ctx.set_tuning("stats_copies_log2", self.n)

    def __exit__(self, *exc):
        self.ctx.set_tuning("stats_copies_log2", STATS_COPIES_DEFAULT)


@pytest.mark.parametrize("log2c", [0, 1, 3, 4])
@pytest.mark.parametrize("parity", [0, 1])
def test_every_field_equals_the_integer_model_with_other_numbers_of_counter_copies(ctx, cases, parity, log2c):
    """test_every_field_equals_the_integer_model (host pointers) with 1, 2, 8 and 16 copies of the counters: the records are integers and
    do not depend on how many copies the votes were spread over."""
    with copies(ctx, log2c):
        test_every_field_equals_the_integer_model(ctx, cases, parity, "host")


@pytest.mark.parametrize("log2c", [0, 4])
def test_more_called_sites_than_workgroups_with_one_and_sixteen_counter_copies(ctx, log2c):
    """The fold leaves every copy zero for the workgroup's next site: with one copy and with sixteen"""
    with copies(ctx, log2c):
        test_more_called_sites_than_workgroups(ctx)


def device_call(ctx, offsets, entries, refs, results, shift):
    """bvc_site_stats_csr with BVC_PTR_DEVICE on torch memory (the binding's site_stats_csr_device takes typed tensors: int64 offsets)."""
    import torch
    from basevarc_amd.lib import STATS_DTYPE

    def raw(a, pad):
        b = np.concatenate([np.zeros(pad, dtype=np.uint8), np.frombuffer(a.tobytes(), dtype=np.uint8)])
        return torch.from_numpy(b.copy()).to("cuda:0")[pad:]
    # int64 offsets need an 8-byte aligned address: they stay at the start of their allocation; the entries move by ONE entry, the
    # reference bases by one byte, the records by eight
    o_t = torch.from_numpy(offsets.copy()).to("cuda:0")
    e_t = raw(entries, 8 * shift)
    r_t = raw(refs, shift)
    res_t = raw(results, 8 * shift)
    out_t = torch.full((len(refs) * 64 + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")[64 * shift:64 * shift + len(refs) * 64]
    st = ctx.site_stats_csr_device(o_t, e_t, r_t, res_t, stats_t=out_t)
    assert st.data_ptr() == out_t.data_ptr()
    ctx.synchronize()
    return np.frombuffer(st.cpu().numpy().tobytes(), dtype=STATS_DTYPE)


def test_more_called_sites_than_workgroups(ctx):
    """4,000 small sites twice in one call: a workgroup takes several sites, and the second copy of a site must get the first copy's
    record -- counters that were not zeroed between two sites of a workgroup would show in it."""
    from basevarc_amd.lib import SITE_DTYPE
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 90, 4000)
    lens[::97] = 0
    parts = [random_entries(rng, int(n)) for n in lens]
    entries = np.concatenate(parts + parts)
    offsets = np.concatenate([[0], np.cumsum(np.concatenate([lens, lens]))]).astype(np.int64)
    refs = np.tile(rng.integers(-1, 4, 4000).astype(np.int8), 2)
    res = np.zeros(4000, dtype=SITE_DTYPE)
    res["called"] = rng.random(4000) < 0.9
    res["n_alt"] = rng.integers(1, 4, 4000)
    res["alt_base"] = rng.integers(0, 4, (4000, 3))
    results = np.concatenate([res, res])
    stats = ctx.site_stats_csr(offsets, entries, refs, results)
    assert stats[:4000].tobytes() == stats[4000:].tobytes()
    check_stats(stats[:4000], offsets[:4001], entries, refs[:4000], res, where="twice")
    dev = device_call(ctx, offsets, entries, refs, results, 0)
    assert dev.tobytes() == stats.tobytes()


def test_refusals_leave_the_context_usable(ctx):
    from basevarc_amd.lib import STATS_DTYPE
    offsets, entries, refs, results = big_case(0)
    offsets, n = offsets[:9].copy(), 8
    entries, refs, results = entries[:offsets[8]], refs[:8], results[:8]
    out = np.zeros(n, dtype=STATS_DTYPE)
    L, h = ctx._L, ctx._h
    p = lambda a: C.c_void_p(a.ctypes.data)
    good = [p(offsets), p(entries), p(refs), p(results), p(out)]
    for k in range(5):                                             # every null pointer with work present
        args = list(good)
        args[k] = None
        assert L.bvc_site_stats_csr(h, n, *args, 0) == BVC_ERR_ARG, k
        if k != 1:
            assert L.bvc_site_stats_csr(h, n, *args, 1) == BVC_ERR_ARG, k
    assert L.bvc_site_stats_csr(h, -1, *good, 0) == BVC_ERR_ARG
    assert L.bvc_site_stats_csr(h, -1, *good, 1) == BVC_ERR_ARG
    bad = offsets.copy(); bad[3] = bad[2] - 1
    assert L.bvc_site_stats_csr(h, n, p(bad), *good[1:], 0) == BVC_ERR_ARG
    bad = offsets.copy(); bad[0] = 1
    assert L.bvc_site_stats_csr(h, n, p(bad), *good[1:], 0) == BVC_ERR_ARG
    assert L.bvc_site_stats_csr(h, 0, None, None, None, None, None, 0) == 0          # no work: nothing is needed
    stats = ctx.site_stats_csr(offsets, entries, refs, results)
    check_stats(stats, offsets, entries, refs, results, where="after the refusals")


# ------------------------------------------------------------------------------------------------------------------ the producer
def check_producer(with_stats, without, refs, where):
    assert with_stats is not None and without is not None, where
    for key in without:
        a, b = with_stats[key], without[key]
        if a is None or b is None:
            assert a is None and b is None, (where, key)
        elif isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (where, key)
        else:
            assert a == b, (where, key)
    assert set(with_stats) == set(without) | {"stats"}, where
    check_stats(with_stats["stats"], with_stats["called_off"], with_stats["entries"], refs, with_stats["results"], where=where)
    return int((with_stats["results"]["called"] != 0).sum())


@pytest.mark.parametrize("shape", ["dense", "indel_heavy", "wide_text"])
def test_text_tiles_deliver_the_statistics_with_everything_else_unchanged(ctx, shape):
    n_in_batch, tiles = fuzz_tiles(shape)
    s0 = sample0_of(n_in_batch)
    carry, called = [0, 0, 0, 0, 0], 0
    for i, (batch_tokens, ref) in enumerate(tiles):
        lines, _, _, _ = encode(batch_tokens)
        text, ls = tile_of(lines)
        a = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True, stats=True)
        b = ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True)
        called += check_producer(a, b, ref, f"text {shape} tile {i}")
        carry = b["carry_out"]
    assert called > 0, shape                                       # (the model was asked about real records)
    with pytest.raises(ValueError):
        ctx.pileup_tile(text, ls, s0, n_in_batch, ref, 0.001, stats=True)


@pytest.mark.parametrize("n_groups", [0, 5])
@pytest.mark.parametrize("shape", ["dense", "wide"])
def test_binary_tiles_deliver_the_statistics_with_everything_else_unchanged(ctx, shape, n_groups):
    n_in_batch, tiles = fuzz_tiles(shape)
    n = int(n_in_batch.sum())
    rng = np.random.default_rng(99)
    group = rng.integers(0, 5, n).astype(np.uint8)
    group[rng.random(n) < 0.1] = 255
    kw = dict(group_of_sample=group, n_groups=5) if n_groups else dict()
    s0 = sample0_of(n_in_batch)
    carry, called = [0, 0, 0, 0, 0], 0
    for i, (batch_tokens, ref) in enumerate(tiles):
        _, records, rs, _ = encode(batch_tokens)
        a = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True, stats=True, **kw)
        b = ctx.pileup_tile_bin(records, rs, s0, n_in_batch, ref, 0.001, carry_in=carry, called_only=True, **kw)
        called += check_producer(a, b, ref, f"bin {shape} groups {n_groups} tile {i}")
        carry = b["carry_out"]
    assert called > 0, shape
