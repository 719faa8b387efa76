"""The hand-built stage-2 catalogue (tests/lrt_sites.py) on the device (run with -m gpu on an MI355X): bvc_lrt_hist and
bvc_lrt_hist_groups against the records of the 50-digit model (tests/lrt_model.py), under every setting of the stage-2 knobs,
at every position of a region of each kernel, from host and from device pointers, and through the other entry points on the
expanded observations.

Bars: on DECISIVE cases every integer field exact, n_fits / n_passes by path_counts_match's rule, AF within 1e-6 absolute, chi and
var_qual within 1e-6 relative with floor 1e-6 -- against the high-precision values; an either-outcome case must equal ONE of the
model's outcomes in every field."""
import collections
import math

import numpy as np
import pytest

from tests import lrt_sites as S
from tests.test_gpu_parity import _pack_numpy, item_engine_takes, path_counts_match

pytestmark = pytest.mark.gpu

AF_ATOL, QUAL_RTOL, QUAL_FLOOR = 1e-6, 1e-6, 1e-6
DEFAULT_COMB = [0, 1, 2, 3]
SETTINGS = [dict(em_engine=e, em_prune=p, em_tiny_regions=t, em_wpb=w) for e in (0, 1) for p in (0, 1) for t in (0, 1) for w in (1, 4)]
DEFAULTS = dict(em_engine=0, em_prune=1, em_tiny_regions=0, em_wpb=4)


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model():
    """The model's records of every case, once (a few seconds)."""
    return S.model_results()


@pytest.fixture(scope="module")
def cases():
    return S.catalogue()


def context_with(setting):
    from basevarc_amd import Context
    c = Context(0)
    for k, v in setting.items():
        c.set_tuning(k, v)
    return c


# ---------------------------------------------------------------------------------------------------------------- running sites
Site = collections.namedtuple("Site", "counts ref min_af comb device_comb")


def site_of(case):
    return Site(S.counts512(case.counts), case.ref, case.min_af, case.comb, case.device_comb)


def comb_arrays(sites):
    cb = np.zeros((len(sites), 4), dtype=np.int8)
    nc = np.zeros(len(sites), dtype=np.uint8)
    for i, s in enumerate(sites):
        comb = DEFAULT_COMB if s.comb is None else s.comb
        cb[i, :len(comb)] = comb
        nc[i] = len(comb)
    return cb, nc


def lrt_hist_device_pointers(c, counts, ref, min_af, cb=None, nc=None):
    import torch
    from basevarc_amd.lib import results_from_tensor
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if x is not None else None
         for x in (counts.astype(np.uint32).view(np.int32), ref, cb, nc)]
    out = c._lrt_hist(True, len(ref), d[0], d[1], min_af, d[2], d[3])
    c.synchronize()
    return results_from_tensor(out).copy()


def run_sites(c, sites, null_comb=True, device=False):
    """Records of `sites` in their order.  One call per (min_af, pointer kind, base_comb given or NULL): a list with an entry
    outside 0..3 can only go through device pointers; null_comb=False hands the default list {A,C,G,T} over explicitly."""
    out = [None] * len(sites)
    calls = collections.defaultdict(list)
    for i, s in enumerate(sites):
        calls[(s.min_af, device or s.device_comb, s.comb is None and null_comb)].append(i)
    for (min_af, dev, null), idx in calls.items():
        part = [sites[i] for i in idx]
        counts = np.stack([s.counts for s in part])
        ref = np.array([s.ref for s in part], dtype=np.int8)
        cb, nc = (None, None) if null else comb_arrays(part)
        recs = lrt_hist_device_pointers(c, counts, ref, min_af, cb, nc) if dev else c.lrt_hist(counts, ref, min_af, cb, nc)
        for i, r in zip(idx, recs):
            out[i] = r
    return out


# ---------------------------------------------------------------------------------------------------------------- comparing
def same_number(a, b, rtol, floor):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= max(floor, rtol * abs(b))


def difference(rec, exp, counts):
    """First field in which the device record differs from a model outcome, or None."""
    n_alt = min(exp["n_alt"], 3)
    got = dict(status=int(rec["status"]), depth=[int(x) for x in rec["depth"]], depth_total=float(rec["depth_total"]),
               called=int(rec["called"]), n_alt=int(rec["n_alt"]), alt_base=[int(rec["alt_base"][i]) for i in range(min(int(rec["n_alt"]), 3))],
               kept=[int(rec["kept"][i]) for i in range(min(int(rec["n_kept"]), 4))])
    want = dict(status=exp["status"], depth=exp["depth"], depth_total=exp["depth_total"], called=exp["called"], n_alt=n_alt,
                alt_base=exp["alt_base"][:3], kept=exp["kept"])
    for f in got:
        if got[f] != want[f]:
            return f
    if not path_counts_match(rec, exp, counts):
        return "n_fits / n_passes"
    for i in range(n_alt):
        if not same_number(float(rec["af"][i]), exp["af"][i], 0.0, AF_ATOL):
            return "af"
    for f in ("chi", "var_qual"):
        if not same_number(float(rec[f]), exp[f], QUAL_RTOL, QUAL_FLOOR):
            return f
    return None


def assert_catalogue_matches(cases, recs, model, counts, where=""):
    worst = dict(af=(0.0, None), chi=(0.0, None), var_qual=(0.0, None))
    for c, rec in zip(cases, recs):
        g = model[c.name]
        # (min_af <= 0: uses_item_engine is false, the wave engine runs what the reference runs)
        diffs = [difference(rec, exp, counts if c.min_af > 0 else "reference") for exp in g["outcomes"]]
        assert None in diffs, (where, c.name, diffs, rec, g["outcomes"])
        if g["decisive"]:
            exp = g["outcomes"][0]
            for i in range(min(exp["n_alt"], 3)):
                if not math.isnan(exp["af"][i]):
                    worst["af"] = max(worst["af"], (abs(float(rec["af"][i]) - exp["af"][i]), c.name), key=lambda t: t[0])
            for f in ("chi", "var_qual"):
                if not math.isnan(exp[f]):
                    worst[f] = max(worst[f], (abs(float(rec[f]) - exp[f]) / max(abs(exp[f]), 1.0), c.name), key=lambda t: t[0])
    return worst


def counts_rule(setting):
    """path_counts_match: the reference's counts from the wave engine and with em_prune = 0, the pruned pair otherwise."""
    return "reference" if setting["em_engine"] == 1 or setting["em_prune"] == 0 else "default"


def reference_defined(rec):
    """The record's bytes without the two diagnostics that count what was RUN (include/bvc.h "em_prune")."""
    r = rec.copy()
    r["n_fits"] = 0
    r["n_passes"] = 0
    return r.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_catalogue_against_the_model(ctx, cases, model):
    """The whole catalogue, one call per min_af and pointer kind, a new context's settings."""
    recs = run_sites(ctx, [site_of(c) for c in cases])
    worst = assert_catalogue_matches(cases, recs, model, "default")
    print("largest error of the device against the model (af absolute; chi, var_qual relative with floor 1):", worst)


@pytest.fixture(scope="module")
def runs(cases):
    """The catalogue under each of the sixteen settings, once."""
    out = {}
    for setting in SETTINGS:
        with context_with(setting) as c:
            out[tuple(sorted(setting.items()))] = run_sites(c, [site_of(x) for x in cases])
    return out


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "engine%(em_engine)d-prune%(em_prune)d-tiny%(em_tiny_regions)d-wpb%(em_wpb)d" % s)
def test_knob_settings_against_the_model(runs, cases, model, setting):
    assert_catalogue_matches(cases, runs[tuple(sorted(setting.items()))], model, counts_rule(setting), where=str(setting))


def test_knob_settings_leave_the_reference_defined_bytes_alone(runs, cases, model):
    """Decisive cases: em_prune and em_wpb change no byte of what the reference defines (em_prune changes n_fits / n_passes, which
    count what was run); em_tiny_regions changes nothing for a site that is not in a tiny region, and like em_engine only the last
    bits of AF / chi / var_qual / lr_alt / base_frq elsewhere (include/bvc.h) -- those are held by the model comparison above."""
    def of(**kw):
        return runs[tuple(sorted(dict(DEFAULTS, **kw).items()))]

    base = of()
    decisive = [i for i, c in enumerate(cases) if model[c.name]["decisive"]]
    for engine in (0, 1):
        for tiny in (0, 1):
            ref = of(em_engine=engine, em_tiny_regions=tiny)
            for prune in (0, 1):
                for wpb in (1, 4):
                    other = of(em_engine=engine, em_tiny_regions=tiny, em_prune=prune, em_wpb=wpb)
                    for i in decisive:
                        assert reference_defined(other[i]) == reference_defined(ref[i]), (cases[i].name, engine, tiny, prune, wpb)
                    if prune == 1 or engine == 1:
                        assert all(other[i].tobytes() == ref[i].tobytes() for i in decisive), (engine, tiny, prune, wpb)
    # the wave engine knows no regions
    assert all(of(em_engine=1, em_tiny_regions=1)[i].tobytes() == of(em_engine=1)[i].tobytes() for i in decisive)
    # integer fields agree across engines and kernels
    for i in decisive:
        for other in (of(em_engine=1), of(em_tiny_regions=1)):
            for f in ("status", "depth", "depth_total", "called", "n_alt", "alt_base", "n_kept", "kept"):
                assert np.array_equal(other[i][f], base[i][f]), (cases[i].name, f)


def region_kind(need):
    """The kernel of a region whose widest taken site has `need` quality values on an allele, with em_tiny_regions = 1."""
    return 8 if need <= 8 else 32 if need <= 32 else 48


# seven of these beside a case make its region tiny, narrow or wide (unless the case itself is wider)
NEIGHBOURS = {8: {(0, 30): 50, (1, 20): 5, (0, 25): 7}, 32: {**{(0, q): 4 for q in range(10, 30)}, (2, 30): 9},
              48: {**{(3, q): 5 for q in range(3, 43)}, (0, 30): 11}}
NEIGHBOUR_NEED = {8: 2, 32: 20, 48: 40}


@pytest.fixture(scope="module")
def alone(cases):
    """Every case as a call of its own (em_tiny_regions = 1)."""
    with context_with(dict(em_tiny_regions=1)) as c:
        return {x.name: run_sites(c, [site_of(x)], null_comb=False)[0] for x in cases if not x.device_comb}


@pytest.mark.parametrize("kind", [8, 32, 48], ids=["tiny", "narrow", "wide"])
def test_record_does_not_depend_on_the_position_in_a_region(cases, model, alone, kind):
    """Every case at each of the eight positions of a region whose other seven sites send it to the tiny, the narrow or the wide
    kernel (or further up, when the case itself is wider), and alone in a call: the same bytes at every position; the same bytes as
    alone when alone it takes the same kernel or the wave engine; the narrow and the wide kernel agree byte for byte (em_items.hip:
    same lane, slot and order); whichever kernel, the record is the model's."""
    use = [c for c in cases if not c.device_comb]
    by_pos = []
    with context_with(dict(em_tiny_regions=1)) as c:
        for pos in range(8):
            sites = []
            for x in use:
                neighbour = Site(S.counts512(NEIGHBOURS[kind]), 0, x.min_af, None, False)
                sites += [neighbour] * pos + [site_of(x)] + [neighbour] * (7 - pos)
            # (run_sites keeps the order within a call, and every case brings its whole region along)
            by_pos.append(run_sites(c, sites, null_comb=False)[pos::8])
    for pos in range(8):
        assert_catalogue_matches(use, by_pos[pos], model, "default", where="kind %d, position %d" % (kind, pos))
    for i, x in enumerate(use):
        first = by_pos[0][i].tobytes()
        assert all(by_pos[pos][i].tobytes() == first for pos in range(8)), (x.name, kind)
        exp = model[x.name]["outcomes"][0]
        taken = x.min_af > 0 and item_engine_takes(exp)
        k_alone, k_region = region_kind(exp["max_quals"]), region_kind(max(exp["max_quals"], NEIGHBOUR_NEED[kind]))
        if not taken or k_alone == k_region or min(k_alone, k_region) >= 32:
            assert alone[x.name].tobytes() == first, (x.name, kind)


def test_host_and_device_pointers(ctx, cases, model):
    """base_comb / n_comb: host pointers refuse an entry outside 0..3 and n_comb > 4 (BVC_ERR_ARG, nothing runs); device pointers
    ignore the entry and read n_comb > 4 as 4 (include/bvc.h).  Every other case: the same bytes from both kinds of pointers."""
    from basevarc_amd.lib import BvcError
    plain = [c for c in cases if not c.device_comb]
    host = run_sites(ctx, [site_of(c) for c in plain])
    dev = run_sites(ctx, [site_of(c) for c in plain], device=True)
    assert all(h.tobytes() == d.tobytes() for h, d in zip(host, dev))
    bad = [c for c in cases if c.device_comb]
    assert len(bad) >= 2
    for c in bad:
        s = site_of(c)
        cb, nc = comb_arrays([s])
        with pytest.raises(BvcError):
            ctx.lrt_hist(s.counts[None], np.array([s.ref], dtype=np.int8), s.min_af, cb, nc)
        got = run_sites(ctx, [s])[0]
        clean = s._replace(comb=[b for b in s.comb if 0 <= b <= 3], device_comb=False)
        assert got.tobytes() == run_sites(ctx, [clean])[0].tobytes(), c.name
        assert difference(got, model[c.name]["outcomes"][0], "default") is None, c.name
    four = next(c for c in cases if c.name == "comb_reordered")
    s = site_of(four)
    cb, nc = comb_arrays([s])
    nc[0] = 200
    with pytest.raises(BvcError):
        ctx.lrt_hist(s.counts[None], np.array([s.ref], dtype=np.int8), s.min_af, cb, nc)
    got = lrt_hist_device_pointers(ctx, s.counts[None], np.array([s.ref], dtype=np.int8), s.min_af, cb, nc)[0]
    assert got.tobytes() == run_sites(ctx, [s])[0].tobytes()


def expand_groups(case):
    rows = [S.expand(slot) for slot in case.groups]
    b, q = np.concatenate([x[0] for x in rows]), np.concatenate([x[1] for x in rows])
    label = np.concatenate([np.full(len(x[0]), g, dtype=np.uint8) for g, x in enumerate(rows)])
    return b, q, label


@pytest.mark.parametrize("engine", [0, 1])
def test_group_cases(model, engine):
    """bvc_lrt_hist_groups on the group slots: the overall record and every group record against the model; the same bytes from
    device pointers and from bvc_lrt_dense_groups on the expanded observations."""
    import torch
    from basevarc_amd.lib import GROUP_DTYPE, results_from_tensor
    with context_with(dict(em_engine=engine)) as c:
        for case in S.group_cases():
            n_groups = len(case.groups) - 1
            slots = np.stack([S.counts512(s) for s in case.groups])[None]
            ref = np.array([case.ref], dtype=np.int8)
            res, gres = c.lrt_hist_groups(slots, ref, case.min_af, n_groups)
            g = model[case.name]
            assert difference(res[0], g["outcomes"][0], counts_rule(dict(em_engine=engine, em_prune=1))) is None, case.name
            for k, exp in enumerate(g["groups"]):
                got = gres[0][k]
                assert [int(x) for x in got["depth"]] == exp["depth"], (case.name, k)
                assert (int(got["ran"]), int(got["present"])) == (exp["ran"], exp["present"]), (case.name, k)
                assert all(same_number(float(got["af"][i]), exp["af"][i], 0.0, AF_ATOL) for i in range(3)), (case.name, k)
                assert bytes(got["pad"]) == bytes(6)
            d = c.lrt_hist_groups_device(torch.from_numpy(slots.view(np.int32)).cuda(), torch.from_numpy(ref).cuda(), case.min_af, n_groups)
            c.synchronize()
            assert results_from_tensor(d[0]).tobytes() == res.tobytes(), case.name
            assert d[1].cpu().numpy().tobytes() == gres.tobytes(), case.name
            b, q, label = expand_groups(case)
            res2, gres2 = c.lrt_dense_groups(b[None], q[None], ref, case.min_af, label, n_groups)
            assert res2.tobytes() == res.tobytes() and gres2.tobytes() == gres.tobytes(), case.name


def test_other_entry_points_give_the_same_bytes(ctx, cases, model):
    """One case of every census class (depth permitting), expanded to its observations: bvc_lrt_dense, bvc_lrt_csr and
    bvc_lrt_csr_packed return the bytes of bvc_lrt_hist."""
    sample, seen = [], set()
    for c in cases:
        new = set(c.tags) - seen
        if new and sum(c.counts.values()) <= 4000 and not c.device_comb:
            sample.append(c)
            seen |= new
    assert len(sample) >= 60
    by_min_af = collections.defaultdict(list)
    for c in sample:
        by_min_af[c.min_af].append(c)
    for min_af, part in by_min_af.items():
        want = run_sites(ctx, [site_of(c) for c in part], null_comb=False)
        obs = [S.expand(c.counts) for c in part]
        offs = np.concatenate([[0], np.cumsum([len(b) for b, _ in obs])]).astype(np.int64)
        b, q = np.concatenate([o[0] for o in obs]), np.concatenate([o[1] for o in obs])
        ref = np.array([c.ref for c in part], dtype=np.int8)
        cb, nc = comb_arrays([site_of(c) for c in part])
        got = ctx.lrt_csr(offs, b, q, ref, min_af, cb, nc)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), min_af
        plain = [i for i, c in enumerate(part) if c.comb is None]
        if not plain:
            continue
        width = max(len(obs[i][0]) for i in plain)
        B = np.full((len(plain), max(width, 1)), -1, dtype=np.int8)
        Q = np.zeros_like(B)
        for row, i in enumerate(plain):
            B[row, :len(obs[i][0])] = obs[i][0]
            Q[row, :len(obs[i][1])] = obs[i][1]
        got = ctx.lrt_dense(B, Q, ref[plain], min_af)
        assert all(g.tobytes() == want[i].tobytes() for g, i in zip(got, plain)), min_af
        packable = [i for i in plain if max([k[1] for k in part[i].counts] or [0]) <= 62]
        o2 = np.concatenate([[0], np.cumsum([len(obs[i][0]) for i in packable])]).astype(np.int64)
        pk = np.concatenate([_pack_numpy(*obs[i]) for i in packable] or [np.zeros(0, np.uint8)])
        got = ctx.lrt_csr_packed(o2, pk, ref[packable], min_af)
        assert all(g.tobytes() == want[i].tobytes() for g, i in zip(got, packable)), min_af
