"""The hand-built stage-2 catalogue (tests/lrt_sites.py) on the CPU: the 50-digit model (tests/lrt_model.py) against the C oracle in
its faithful, compensated and per-observation forms, the model's ln and chi-square tail against mpmath where that is installed, the
census of the device code's path classes, and the catalogue's two conditions.  docs/LRT_SITES.md has the counts."""
import collections
import math
import os
import re

import numpy as np
import pytest

from oracle import orc
from tests import lrt_model as M
from tests import lrt_sites as S

AF_ATOL, QUAL_RTOL, QUAL_FLOOR = 1e-6, 1e-6, 1e-6
INT_FIELDS = ("status", "depth", "depth_total", "called", "n_alt", "alt_base", "kept", "dup_candidate", "max_quals", "min_qual")
EXPAND_MAX_DEPTH = 4000
# Classes no decisive case can reach: an exact tie is what they are, and a duplicate candidate makes two subsets of a level the
# same model, which is an exact tie again.
NEVER_DECISIVE = set(M.TIES) | {"site_classes leaves the site: dup (duplicate candidate)"}


@pytest.fixture(scope="module")
def cases():
    return S.catalogue() + S.group_cases()


@pytest.fixture(scope="module")
def results(cases):
    """The model over the whole catalogue, once."""
    return S.model_results(cases)


def oracle_comb(case):
    """include/bvc.h: a candidate that is not A, C, G or T has depth 0 and falls to the min_af filter -- the oracle indexes depth[]
    by it, so it gets the list without such entries.  (min_af <= 0 would keep them: no such case.)"""
    if case.comb is None:
        return None
    assert case.min_af > 0 or all(0 <= b <= 3 for b in case.comb)
    return [b for b in case.comb if 0 <= b <= 3]


def same_number(a, b, rtol, floor):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= max(floor, rtol * abs(b))


def record_difference(got, exp, counts=True):
    """First field in which an oracle-style dict `got` differs from the model's record `exp`, or None."""
    for f in INT_FIELDS:
        if got[f] != exp[f]:
            return f
    if counts:
        pairs = [(exp["n_fits"], exp["n_passes"], exp["n_fits_pruned"], exp["n_passes_pruned"])]
        if (got["n_fits"], got["n_passes"]) != pairs[0][:2]:
            return "n_fits / n_passes"
        if exp["prune_edge"] >= M.PRUNE_BOUND and (got["n_fits_pruned"], got["n_passes_pruned"]) != pairs[0][2:]:
            return "pruned pair"
    for a, b in zip(got["af"], exp["af"]):
        if not same_number(a, b, 0.0, AF_ATOL):
            return "af"
    for f in ("chi", "var_qual"):
        if not same_number(got[f], exp[f], QUAL_RTOL, QUAL_FLOOR):
            return f
    return None


def test_renamed_letters_give_the_models_own_record(cases, results):
    """A permuted family's cases take the model's run of the family's first case with the letters renamed (tests/lrt_sites.py
    model_case).  The last case of every such family, run through the model itself: the same record."""
    last = {c.family: c for c in cases if c.perm is not None}
    assert len(last) >= 25
    for c in last.values():
        direct = S.model_case(c, orc.chisf)["outcomes"]
        renamed = results[c.name]["outcomes"]
        assert len(direct) == len(renamed), c.name
        for d, r in zip(direct, renamed):
            for k in d:
                if isinstance(d[k], float) or (isinstance(d[k], list) and d[k] and isinstance(d[k][0], float)):
                    assert np.allclose(d[k], r[k], rtol=1e-13, atol=1e-15, equal_nan=True), (c.name, k)
                else:
                    assert d[k] == r[k], (c.name, k)


def test_model_agrees_with_the_oracle(cases, results):
    """Decisive cases: every integer field, n_fits / n_passes and the pruned pair equal, AF / chi / var_qual within DESIGN.md
    section 4 -- for the faithful and the compensated histogram oracle and, up to a few thousand observations, the
    per-observation oracle.  Either-outcome cases: the oracle's record is one of the model's outcomes."""
    worst = collections.defaultdict(lambda: (0.0, None))
    checked = 0
    for c in cases:
        if c.groups is not None:
            continue
        r = results[c.name]
        comb = oracle_comb(c)
        forms = [("faithful", orc.hist_lrt(S.counts512(c.counts), c.ref, c.min_af, comb)),
                 ("compensated", orc.hist_lrt(S.counts512(c.counts), c.ref, c.min_af, comb, compensated=True))]
        if sum(c.counts.values()) <= EXPAND_MAX_DEPTH:
            b, q = S.expand(c.counts)
            forms.append(("per observation", orc.basetype_lrt(b, q, c.ref, c.min_af, comb)))
        for form, got in forms:
            diffs = [record_difference(got, exp) for exp in r["outcomes"]]
            assert None in diffs, (c.name, form, diffs, got, r["outcomes"])
            checked += 1
            if r["decisive"]:
                exp = r["outcomes"][0]
                for f in ("chi", "var_qual"):
                    if not math.isnan(exp[f]) and exp[f] != 0:
                        e = abs(got[f] - exp[f]) / max(abs(exp[f]), 1.0)
                        if e > worst[f][0]:
                            worst[f] = (e, c.name + " " + form)
                for a, b in zip(got["af"], exp["af"]):
                    if not math.isnan(b) and abs(a - b) > worst["af"][0]:
                        worst["af"] = (abs(a - b), c.name + " " + form)
    print("largest error of the C oracle against the model:", dict(worst))
    assert checked > 2 * len(cases)


def test_group_cases_agree_with_the_oracle(cases, results):
    for c in cases:
        if c.groups is None:
            continue
        n_groups = len(c.groups) - 1
        rows = [S.expand(slot) for slot in c.groups]
        b, q = np.concatenate([x[0] for x in rows]), np.concatenate([x[1] for x in rows])
        label = np.concatenate([np.full(len(x[0]), g, dtype=np.uint8) for g, x in enumerate(rows)])
        r = results[c.name]
        assert r["decisive"], c.name
        if not 0 <= c.ref <= 3:
            continue                                             # (the oracle indexes depth[] by the reference base of its list)
        ov, gd, ga, gr, gp = orc.dense_site_groups(b, q, c.ref, c.min_af, label, n_groups, use_hist=True)
        assert record_difference(ov, r["outcomes"][0]) is None, c.name
        for g, exp in enumerate(r["groups"]):
            assert list(gd[g]) == exp["depth"] and int(gr[g]) == exp["ran"] and int(gp[g]) == exp["present"], (c.name, g)
            assert np.allclose(ga[g], exp["af"], rtol=0, atol=AF_ATOL), (c.name, g)


def test_model_functions_against_mpmath(cases, results):
    """The two transcendental pieces of the model that are its own: Decimal.ln at the likelihoods of every quality the catalogue
    uses, and the chi-square tail at every chi it reaches."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    from decimal import Decimal, localcontext
    quals = sorted({q for c in cases for (_, q) in c.counts})
    with localcontext(M.CTX):
        for q in quals:
            for x in M.lik(q):
                if x > 0:
                    ref = mpmath.log(mpmath.mpf(str(x)))
                    assert abs(mpmath.mpf(str(x.ln())) - ref) <= abs(ref) * mpmath.mpf(10) ** -45 + mpmath.mpf(10) ** -48, q
    chis = sorted({o["chi"] for r in results.values() for o in r["outcomes"] if o["var_qual_kind"] in ("finite", "10000", "subnormal")})
    chis += [1e-6, 0.5, 17.9, 18.0, 18.1, 24.0, 1400.0, 3000.0]   # both branches of erfc and their seam at sqrt(chi / 2) = 3
    assert len(chis) > 50
    for chi in chis:
        ref = mpmath.erfc(mpmath.sqrt(mpmath.mpf(chi) / 2))
        got = mpmath.mpf(str(M.chisf(Decimal(chi))))
        assert abs(got - ref) <= ref * mpmath.mpf(10) ** -40, chi


def test_census_every_path_class_is_reached(cases, results):
    """Every class of tests/lrt_model.py's census is reached, and by a case that is there for it: a family DECLARES the classes it is
    there for (its tags), each of its cases must reach each of them, every class is declared by some family, and every family
    declares a class that no other family declares -- so leaving a family out empties a class, by name."""
    families = collections.defaultdict(list)
    for c in cases:
        families[c.family].append(c)
    declared = collections.defaultdict(set)
    for fam, members in families.items():
        assert len({m.tags for m in members}) == 1, fam
        for tag in members[0].tags:
            assert tag in M.ALL_CLASSES, (fam, tag)
            declared[tag].add(fam)
            for m in members:
                assert tag in results[m.name]["classes"], (m.name, "does not reach", tag)
    assert [k for k in M.ALL_CLASSES if k not in declared] == []
    assert len(set(M.ALL_CLASSES)) == len(M.ALL_CLASSES)
    for fam, members in families.items():
        own = [t for t in members[0].tags if declared[t] == {fam}]
        assert own, (fam, "could be left out without emptying a class")
    for c in cases:
        assert set(results[c.name]["classes"]) <= set(M.ALL_CLASSES)


def test_catalogue_conditions(cases, results):
    """Either-outcome cases are at most a tenth of the catalogue; every class other than the ties themselves is reached by a decisive
    case that declares it; a few hundred cases."""
    either = [c.name for c in cases if not results[c.name]["decisive"]]
    assert len(either) * 10 <= len(cases), either
    decisive_for = collections.defaultdict(list)
    for c in cases:
        if results[c.name]["decisive"]:
            for t in c.tags:
                decisive_for[t].append(c.name)
    assert [k for k in M.ALL_CLASSES if k not in NEVER_DECISIVE and not decisive_for[k]] == []
    for k in NEVER_DECISIVE:
        assert not any(k in results[c.name]["classes"] for c in cases if results[c.name]["decisive"]), k
    assert 300 <= len(cases) <= 1000
    # the searched cases are what they were searched for, at a margin far above the bound
    for c in cases:
        if c.family.startswith(("straddle_", "chi_")):
            assert results[c.name]["decisive"], c.name
    stop = min(results[c.name]["margins"].get("stop", math.inf) for c in cases if results[c.name]["decisive"])
    assert stop > 1000 * float(M.STOP_BOUND)


def test_documented_counts_are_the_catalogues(cases, results):
    """docs/LRT_SITES.md states the size of the catalogue, of the census and the share of either-outcome cases."""
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "docs", "LRT_SITES.md")).read()
    either = sum(1 for c in cases if not results[c.name]["decisive"])
    families = {c.family for c in cases}
    m = re.search(r"(\d+) cases in (\d+) families, (\d+) of them either-outcome \(([\d.]+) %\); (\d+) census classes", doc)
    assert m, "the summary line is missing"
    assert [int(m.group(i)) for i in (1, 2, 3, 5)] == [len(cases), len(families), either, len(M.ALL_CLASSES)]
    assert abs(float(m.group(4)) - 100.0 * either / len(cases)) < 0.06
