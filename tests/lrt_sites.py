"""The catalogue of hand-built stage-2 sites: sparse class counts, ref_base, min_af, an optional base_comb, an optional split into
group slots.  Nothing is random: a case is built from the definition so that one path class of tests/lrt_model.py's census is
taken, and says which (its `tag`, or the tags of its family).  A FAMILY is one case under every assignment of the four letters to
its roles (the role -- deepest, weakest, ... -- is what the case tests; the letter is what pick4, blist and kept index by).

The cases in the stop rule's straddle band and beside chi = 24 and chi = 0 were found by search_small_sites() below, a search in
double over two-allele sites of small integer counts, and are confirmed by the model (tests/test_lrt_sites.py).

model_results() runs the 50-digit model over the catalogue (once per family of permuted cases: a few seconds);
`python -m tests.lrt_sites` prints the census.
"""
import collections
import itertools
import math

import numpy as np

from tests import lrt_model as M

Case = collections.namedtuple("Case", "name family tags counts ref min_af comb device_comb groups perm", defaults=(None,))
MIN_AF = 0.001

# Classes a family is there for beside the one its own line names (the family's every case reaches them): the classes that most
# of the catalogue reaches are each pinned on one family, so that no class of the census rests on an accident.
ALSO = {'chi_above_24': ['wave engine: jump pass (|u| > 2^-6) after the first update pass'],
 'chi_below_24': ['level of n = 2: goes on'],
 'chi_negative': ['lrt_kernel<2> with 1 active slots (em_engine 1)'],
 'chi_small_positive': ['2 candidates pass the min_af filter'],
 'comb_len_1': ['n_alt = 1'],
 'comb_reordered': ['4 candidates pass the min_af filter',
                    'base_comb of length 4',
                    'level of n = 4: deepest candidate at position 2',
                    'level of n = 4: last-resort subset ruled out',
                    'n_alt = 3'],
 'group_alt_index': ['level of n = 3: deepest candidate at position 2',
                     'fit converges at its second pass',
                     'group: n_alt = 2, present = 2'],
 'group_present_2': ['region kind tiny: need <= 8 (em_items.hip region_body)',
                     'level of n = 3: deepest candidate at position 0',
                     'group: n_alt = 2, present = 0'],
 'group_present_3': ['level of n = 4: deepest candidate at position 0'],
 'group_ref_outside': ['n_alt = 2', 'group: n_alt = 2, present = 1', 'group: n_alt = 2, present = 3'],
 'largest_class': ['call_var_qual: 5000'],
 'largest_depth': ['3 candidates pass the min_af filter',
                   'level of n = 3: last-resort subset ruled out',
                   'level of n = 3: goes on'],
 'level_n2_deep0_win0': ['base_comb of length 2'],
 'level_n3_deep0_win0': ['base_comb of length 3'],
 'level_n3_deep0_win2': ['level of n = 3: last-resort subset run'],
 'level_n4_deep0_win0': ['level of n = 4: goes on'],
 'level_n4_deep0_win3': ['level of n = 4: last-resort subset run'],
 'level_n4_deep1_win0': ['level of n = 3: deepest candidate at position 1'],
 'level_n4_deep1_win1': ['level of n = 4: deepest candidate at position 1'],
 'level_n4_deep1_win2': ['fit reaches the cap of 101 passes'],
 'level_n4_deep3_win0': ['level of n = 4: deepest candidate at position 3'],
 'not_called_no_candidate': ['0 candidates pass the min_af filter'],
 'ref_outside': ['pass sure-below (hi(A) < kSureBelowHi)'],
 'values_16': ['var_qual pending then finite'],
 'values_17': ['lrt_kernel<2> with 2 active slots (em_engine 1)'],
 'values_33': ['region kind wide: need <= 48'],
 'values_48': ['lrt_kernel<4> with 3 active slots (em_engine 1)'],
 'values_49': ['site_classes leaves the site: too_wide (> 48 values on an allele)'],
 'values_64': ['lrt_kernel<4> with 4 active slots (em_engine 1)'],
 'values_65': ['lrt_kernel<8> with 6 active slots (em_engine 1)'],
 'values_8': ['pass sure-above (hi(A) >= kSureAboveHi)'],
 'values_9': ['region kind narrow: need <= 32'],
 'values_97': ['lrt_kernel<8> with 8 active slots (em_engine 1)', 'ANY remainder launch lrt_kernel<8,ANY> with 8 active slots'],
 'vq_5000_depth_10': ['1 candidates pass the min_af filter'],
 'vq_5000_depth_11': ['ref_base inside 0..3'],
 'vq_5000_r_half': ['level of n = 2: deepest candidate at position 0'],
 'vq_nan_quality_0': ['ANY remainder launch lrt_kernel<8,ANY> with 6 active slots',
                      'level of n = 2: deepest candidate at position 1']}


def _site(per_base):
    """per_base: {base: {qual: n}} -> {(base, qual): n}"""
    return {(b, q): n for b, qs in per_base.items() for q, n in qs.items() if n}


def _case(name, tag, per_base, ref, min_af=MIN_AF, comb=None, device_comb=False, family=None, groups=None, perm=None):
    tags = (tag,) if isinstance(tag, str) else tuple(tag)
    return Case(name, family or name.split("/")[0], tags + tuple(ALSO.get(family or name.split("/")[0], ())), _site(per_base), ref, min_af, comb, device_comb, groups, perm)


# ---------------------------------------------------------------------------------------------------------------- levels
STRONG = 30          # quality of the alleles that stay


def level_roles(n, p, i):
    """n candidates by position; the deepest at p; the level's winner is subset i, the one that drops position n - 1 - i.  When
    that is the deepest candidate itself (round 2: the last-resort subset wins) the deepest allele is many observations of
    quality 2, which cost little to explain as errors; otherwise the dropped one is a single observation of quality 10."""
    w = n - 1 - i
    if n == 2:
        w = 1 - i
    roles = []
    for pos in range(n):
        if p == w:
            roles.append({2: 20} if pos == p else {40: 3 + pos})
        elif pos == p:
            roles.append({STRONG: 30})
        elif pos == w:
            roles.append({10: 1})
        else:
            roles.append({STRONG: 5 + 2 * pos})
    return roles


def _permuted(name, tag, roles, ref_pos, **kw):
    """The family of a role case: every ordered choice of letters for its positions, handed over as base_comb."""
    out = []
    for letters in itertools.permutations(range(4), len(roles)):
        per_base = {b: r for b, r in zip(letters, roles)}
        ref = letters[ref_pos] if ref_pos is not None else [b for b in range(4) if b not in letters][0]
        out.append(_case("%s/%s" % (name, "".join("ACGT"[b] for b in letters)), tag, per_base, ref, comb=list(letters), family=name,
                         perm=letters + tuple(b for b in range(4) if b not in letters), **kw))
    return out


def level_cases():
    out = []
    for n in (4, 3):
        for p in range(n):
            for i in range(n):
                tag = "level of n = %d: deepest at %d, subset %d wins in round %d" % (n, p, i, 2 if i == n - 1 - p else 1)
                out += _permuted("level_n%d_deep%d_win%d" % (n, p, i), tag, level_roles(n, p, i), p)
        out += _permuted("level_n%d_all_stay" % n, "level of n = %d: ends at chi >= 24" % n,
                         [{STRONG: 10 + 3 * pos} for pos in range(n)], 0)
    for p in range(2):
        for i in range(2):
            out += _permuted("level_n2_deep%d_win%d" % (p, i), "one-allele level: deepest at %d, candidate %d wins" % (p, i), level_roles(2, p, i), 1 - i)
    out += _permuted("level_n2_both_stay", "level of n = 2: ends at chi >= 24", [{STRONG: 12}, {STRONG: 9}], 0)
    return out


# ---------------------------------------------------------------------------------------------------------------- exact ties
def tie_cases():
    """Identical count vectors on two or three alleles: their subsets' chi are equal exactly, whichever the kernel keeps is
    legitimate.  Every level, every position of the deepest candidate."""
    out = []
    same = {20: 2}
    for n in (3, 4):
        for p in range(n):
            per_base = {pos: ({STRONG: 30} if pos == p else dict(same)) for pos in range(n)}
            out.append(_case("tie_n%d/deep%d" % (n, p), "exact tie among the subsets of a level of n = %d" % n, per_base, p))
    out.append(_case("tie_n2", "exact tie among the subsets of a level of n = 2", {1: {30: 5}, 3: {30: 5}}, 1))
    out.append(_case("tie_n4/two_of_three", "exact tie among the subsets of a level of n = 4",
                     {0: {STRONG: 30}, 1: dict(same), 2: {25: 9}, 3: dict(same)}, 0))
    # equal depths in deepest_position that decide nothing: the two deepest alleles are the same, the weakest goes
    out.append(_case("deepest_tie/n3", "deepest_position with equal depths", {0: {STRONG: 30}, 1: {10: 1}, 2: {STRONG: 30}}, 0))
    out.append(_case("deepest_tie/n4", "deepest_position with equal depths", {0: {10: 1}, 1: {STRONG: 30}, 2: {25: 8}, 3: {STRONG: 30}}, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- searched cases
def _two(q1, n1, q2, n2):
    return {0: {q1: n1}, 2: {q2: n2}}


def searched_cases():
    out = []
    for q1, n1, q2, n2 in ((5, 14, 35, 7), (40, 65, 2, 5), (40, 40, 2, 5)):
        out.append(_case("straddle_converged/%d_%d_%d_%d" % (q1, n1, q2, n2), "pass in the straddle band that converged", _two(q1, n1, q2, n2), 0))
    for q1, n1, q2, n2 in ((10, 64, 10, 11), (40, 78, 10, 13), (12, 5, 23, 1)):
        out.append(_case("straddle_not/%d_%d_%d_%d" % (q1, n1, q2, n2), "pass in the straddle band that did not", _two(q1, n1, q2, n2), 0))
    for q1, n1, q2, n2 in ((2, 39, 40, 4), (20, 60, 30, 3)):
        out.append(_case("chi_below_24/%d_%d_%d_%d" % (q1, n1, q2, n2), "level goes on with chi in (23.9, 24)", _two(q1, n1, q2, n2), 0))
    for q1, n1, q2, n2 in ((40, 63, 10, 14), (2, 51, 40, 8)):
        out.append(_case("chi_above_24/%d_%d_%d_%d" % (q1, n1, q2, n2), "level ends with chi in (24, 24.1)", _two(q1, n1, q2, n2), 0))
    out.append(_case("chi_negative", ("chi in (-0.05, 0) after a level", "call_var_qual: 0 (chi <= 0)"), _two(2, 5, 40, 4), 0))
    out.append(_case("chi_small_positive", "chi in (0, 0.05) after a level", _two(2, 3, 40, 2), 0))
    return out


# ---------------------------------------------------------------------------------------------------------------- record, filter, comb
def record_cases():
    out = [
        _case("vq_5000_depth_10", "depth_total = 10 at the 5000 rule", {0: {30: 10}}, 1),
        _case("vq_5000_depth_11", "depth_total = 11 at the 5000 rule", {0: {30: 11}}, 1),
        _case("vq_5000_r_half", "r = 0.5 exactly at the 5000 rule", {0: {40: 6}, 1: {2: 6}}, 1),
        _case("vq_10000", "var_qual pending then 10000", {0: {40: 200}, 3: {40: 180}}, 0),
        _case("vq_nan_quality_0", "var_qual NaN", {0: {0: 5}, 1: {30: 10}}, 1),
        _case("not_called_no_candidate", "called 0: no candidate", {0: {30: 5}, 1: {30: 5}}, 0, min_af=0.9),
        _case("not_called_ref_only", "called 0: the accepted model is the reference base alone", {2: {30: 20}}, 2),
        _case("no_observation", "called 0: no observation", {}, 0),
        _case("ref_outside", "ref_base outside 0..3", {0: {30: 20}, 1: {30: 10}}, 4),
    ]
    above = math.nextafter(0.1, 1.0)
    out += [
        _case("min_af_equal_kept/1_10", "candidate kept at depth / depth_total == min_af", {0: {30: 9}, 1: {30: 1}}, 0, min_af=0.1),
        _case("min_af_ulp_dropped", "candidate dropped one ulp below min_af", {0: {30: 9}, 1: {30: 1}}, 0, min_af=above),
        # (7 / 25 == 0.28 in double, but 0.28 * 25 > 7: a filter rewritten as depth >= min_af * depth_total drops the base)
        _case("min_af_equal_kept/7_25", "candidate kept at depth / depth_total == min_af", {0: {30: 18}, 3: {30: 7}}, 3, min_af=0.28),
    ]
    four = {0: {30: 20}, 1: {30: 10}, 2: {30: 14}, 3: {30: 12}}
    for comb in ([], [2]):
        out.append(_case("comb_len_%d" % len(comb), "base_comb of length %d" % len(comb), four, 0, comb=comb))
    out += [
        _case("comb_reordered", "base_comb reordered", four, 1, comb=[1, 3, 0, 2]),
        _case("comb_duplicate/kept", "base_comb with a duplicate", four, 0, comb=[0, 1, 0]),
        _case("comb_duplicate_candidates", "site_classes leaves the site: dup (duplicate candidate)", four, 0, comb=[2, 2, 1, 2]),
        _case("comb_non_acgt/inside", "base_comb with a non-ACGT entry", four, 0, comb=[0, 4, 1, -1], device_comb=True),
        _case("comb_duplicate/filtered", "base_comb with a duplicate", {0: {30: 2000}, 1: {30: 1}, 2: {30: 50}}, 0, comb=[1, 0, 1, 2]),
        _case("comb_non_acgt/first", "base_comb with a non-ACGT entry", four, 0, comb=[7, 2, 0], device_comb=True),
    ]
    return out


# ---------------------------------------------------------------------------------------------------------------- engines and shapes
def _wide(k, q0=2, n=3):
    return {q0 + j: n for j in range(k)}


def shape_cases():
    out = []
    for k in M.EDGES:
        # k quality values on ONE allele only, a few observations of another
        tag = "widest allele of the site has %d quality values" % k
        out.append(_case("values_%d" % k, tag, {1: _wide(k), 2: {30: 10}}, 1))
    out += [
        _case("low_quality/not_a_candidate", "site_classes leaves the site: any_low (quality 0 or 1)", {0: {30: 3000}, 1: {1: 2}, 2: {30: 40}}, 0, min_af=0.01),
        _case("low_quality/1_candidate", "site_classes leaves the site: any_low (quality 0 or 1)", {0: {30: 30}, 1: {1: 12}, 2: {30: 4}}, 0),
        _case("low_quality/0_other_allele", "site_classes leaves the site: any_low (quality 0 or 1)", {0: {30: 30, 0: 2}, 2: {30: 9}}, 0),
        _case("min_af_nonpositive/zero", "uses_item_engine false: min_af <= 0", {0: {30: 20}, 1: {30: 10}, 2: {30: 14}, 3: {30: 12}}, 0, min_af=0.0),
        _case("zero_coverage/empty_alleles", "subset of zero coverage skipped (src/BaseType.cpp:54)", {0: {30: 5}}, 1, min_af=0.0),
        _case("min_af_nonpositive/negative", "uses_item_engine false: min_af <= 0", {0: {30: 20}, 3: {20: 3}}, 3, min_af=-1.0),
        _case("zero_coverage/skipped", "subset of zero coverage skipped (src/BaseType.cpp:54)", {0: {30: 20}}, 0, min_af=0.0, comb=[0, 2]),
        # ... and the winner is then numbered among the fitted subsets but looked up among all of them: G is "kept"
        _case("zero_coverage/winner_misnumbered", "subset of zero coverage skipped (src/BaseType.cpp:54)", {0: {30: 20}}, 0, min_af=0.0, comb=[2, 0]),
        _case("status_1", "status 1: a level without a fit", {0: {30: 5}}, 0, min_af=0.0, comb=[1]),
        _case("largest_class", "a single class of 2^31 - 1 observations", {0: {30: 2 ** 31 - 1}}, 1),
        _case("largest_depth", "depth_total = 2^31 - 1 over several classes", {0: {30: 1500000000}, 2: {25: 647483647 - 5}, 3: {12: 5}}, 0, min_af=1e-12),
    ]
    return out


# ---------------------------------------------------------------------------------------------------------------- group cases
def group_cases():
    ref, alt = {30: 20}, {30: 10}

    def slots(*per_group):
        return [_site(g) for g in per_group] + [{}]

    def total(s):
        c = collections.Counter()
        for x in s:
            c.update(x)
        return {(b, q): n for (b, q), n in c.items()}

    out = []

    def add(name, tag, s, r, **kw):
        fam = name.split("/")[0]
        tags = ((tag,) if isinstance(tag, str) else tuple(tag)) + tuple(ALSO.get(fam, ()))
        out.append(Case(name, fam, tags, total(s), r, kw.get("min_af", MIN_AF), None, False, s))

    add("group_not_called", "group: overall site not called, depths only", slots({0: ref}, {0: {25: 7}}), 0)
    add("group_zero_depth", "group: called, a group of zero depth (ran = 0)", slots({0: ref, 1: alt}, {}, {0: ref}), 0)
    for n_alt in (1, 2, 3):
        alts = [1, 2, 3][:n_alt]
        groups = []
        for mask in range(1 << n_alt):
            g = {0: ref}
            for i, b in enumerate(alts):
                if (mask >> i) & 1:
                    g[b] = {30: 10 + i}
            groups.append(g)
        add("group_present_%d/every_mask" % n_alt, ["group: n_alt = %d, present = %d" % (n_alt, m) for m in range(1 << n_alt)] if n_alt != 2 else (), slots(*groups), 0)
    add("group_alt_index", "group: its own ALT index differs from the overall one", slots({3: ref, 0: alt}, {3: ref, 2: {30: 12}}, {3: ref, 2: alt, 0: {30: 9}}), 3)
    add("group_ref_outside", "group: ref outside 0..3", slots({0: ref, 1: alt}, {1: {30: 15}}, {0: {30: 8}}), 4)
    s = slots({0: ref, 1: alt}, {0: ref})
    s[-1] = _site({2: {30: 25}})                                 # observations of no group count towards the overall site only
    add("group_present_2/unlabelled_alt", (), s, 0)
    return out


def catalogue():
    return level_cases() + tie_cases() + searched_cases() + record_cases() + shape_cases()


def counts512(counts):
    a = np.zeros(512, dtype=np.uint32)
    for (b, q), n in counts.items():
        a[b * 128 + q] = n
    return a


def expand(counts):
    """(bases, quals) of the observations, class by class."""
    b = np.concatenate([np.full(n, k[0], dtype=np.int8) for k, n in sorted(counts.items())] or [np.zeros(0, np.int8)])
    q = np.concatenate([np.full(n, k[1], dtype=np.int8) for k, n in sorted(counts.items())] or [np.zeros(0, np.int8)])
    return b, q


# ---------------------------------------------------------------------------------------------------------------- model results
def _relabel(rec, perm):
    """The record of a case whose letters are perm[0], perm[1], ... where the family's first case has 0, 1, ...: the model never
    looks at a letter except to index by it, so the record is the first case's with every letter renamed."""
    r = dict(rec)
    r["alt_base"] = [perm[b] for b in rec["alt_base"]]
    r["kept"] = [perm[b] for b in rec["kept"]]
    for k in ("depth", "base_frq"):
        r[k] = [rec[k][perm.index(b)] for b in range(4)]
    return r


def model_case(case, chisf_double, family_first=None):
    """What is kept of a case: the record of every legitimate outcome, whether the case is decisive, its census classes and its
    closest decisive margins.  A case of a permuted family takes the model's run of the family's first case (`family_first`, its
    letters in ascending order) with the letters renamed; the oracle and the device get the case itself."""
    if case.groups is not None:
        rec, tr, groups = M.group_records(case.groups, case.ref, case.min_af, chisf_double)
        outs = [(rec, tr)]
        traces = [tr] + [g["trace"] for g in groups if g["trace"]]
        classes = M.census(case.counts, case.ref, case.min_af, None, rec, tr) | M.group_census(case.ref, rec, groups)
        res = dict(decisive=all(M.is_decisive(t) for t in traces),
                   groups=[dict(depth=g["depth"], af=g["af"], ran=g["ran"], present=g["present"]) for g in groups])
    else:
        if family_first is not None:
            outs = [(_relabel(r, case.perm), tr) for r, tr in family_first["runs"]]
        else:
            outs = M.outcomes(case.counts, case.ref, case.min_af, case.comb, chisf_double)
        traces = [outs[0][1]]
        classes = set()
        for rec, tr in outs:
            classes |= M.census(case.counts, case.ref, case.min_af, case.comb, rec, tr, case.device_comb)
        res = dict(decisive=len(outs) == 1)
    res["outcomes"] = [{k: v for k, v in r.items() if k != "hp"} for r, _ in outs]
    res["runs"] = outs
    margins = {}
    for t in traces:
        for k, v in M.closest_margins(t).items():
            margins[k] = min(margins.get(k, math.inf), v)
    res.update(classes=sorted(classes, key=M.ALL_CLASSES.index), margins=margins)
    return res


def model_results(cases=None):
    """{case name: model_case}: the model over the catalogue, a few seconds."""
    from oracle import orc
    out, first = {}, {}
    for c in (cases if cases is not None else catalogue() + group_cases()):
        if c.perm is not None and c.family in first:
            out[c.name] = model_case(c, orc.chisf, first[c.family])
        else:
            out[c.name] = model_case(c, orc.chisf)
            if c.perm is not None:
                assert list(c.perm) == sorted(c.perm), c.name
                first[c.family] = out[c.name]
    return out


def census_table(results, cases):
    """{class: [names of the DECISIVE cases that reach it]} and {class: [either-outcome cases]}"""
    dec, either = collections.defaultdict(list), collections.defaultdict(list)
    for c in cases:
        r = results[c.name]
        for k in r["classes"]:
            (dec if r["decisive"] else either)[k].append(c.name)
    return dec, either


# ---------------------------------------------------------------------------------------------------------------- the search
def search_small_sites(max_n=80):
    """How the searched cases were found: every site {A: n1 x quality q1, G: n2 x quality q2} of small counts through EM in
    double; reports the passes whose A lies inside the stop rule's straddle band with the distance of delta from 1e-3, and the
    sites whose last chi lies within 0.1 of 24 or 0.05 of 0.  Prints candidates; the catalogue keeps a few of each kind."""
    a_below, a_above = float(M.A_BELOW), float(M.A_ABOVE)
    found = collections.defaultdict(list)
    for q1, q2 in ((30, 30), (20, 30), (30, 20), (40, 10), (10, 10), (2, 40), (40, 2), (5, 35), (12, 23)):
        (a1, e1), (a2, e2) = [(1 - 10 ** (-q / 10), 10 ** (-q / 10) / 3) for q in (q1, q2)]
        for n1 in range(1, max_n):
            for n2 in range(1, min(n1, 25) + 1):
                n, f, prev, ll = n1 + n2, n1 / (n1 + n2), None, 0.0
                for it in range(101):
                    m1, m2 = f * a1 + (1 - f) * e1, f * e2 + (1 - f) * a2
                    if prev:
                        delta = n1 * abs(math.log(m1) - math.log(prev[0])) + n2 * abs(math.log(m2) - math.log(prev[1]))
                        big_a = n1 * abs(m1 / prev[0] - 1) + n2 * abs(m2 / prev[1] - 1)
                        if a_below * (1 + 1e-6) < big_a < a_above * (1 - 1e-6):
                            found["straddle, converged" if delta < 1e-3 else "straddle, not converged"].append((abs(delta - 1e-3) / 1e-3, q1, n1, q2, n2, it))
                    prev, ll = (m1, m2), n1 * math.log(m1) + n2 * math.log(m2)
                    if it and delta < 1e-3:
                        break
                    f = (n1 * f * a1 / m1 + n2 * f * e2 / m2) / n
                chi = 2 * (ll - max(n1 * math.log(a1) + n2 * math.log(e2), n1 * math.log(e1) + n2 * math.log(a2)))
                if 1e-4 < abs(chi - 24) < 0.1:
                    found["chi below 24" if chi < 24 else "chi above 24"].append((abs(chi - 24), q1, n1, q2, n2))
                if 1e-5 < abs(chi) < 0.05 and n <= 10:
                    found["chi below 0" if chi < 0 else "chi above 0"].append((abs(chi), q1, n1, q2, n2))
    for k, v in sorted(found.items()):
        print(k, len(v), sorted(v)[:6])


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        search_small_sites()
    else:
        cases = catalogue() + group_cases()
        res = model_results(cases)
        dec, either = census_table(res, cases)
        print("%d cases, %d either-outcome" % (len(cases), sum(1 for c in cases if not res[c.name]["decisive"])))
        for k in M.ALL_CLASSES:
            print("%4d %3d  %s" % (len(dec.get(k, [])), len(either.get(k, [])), k))
