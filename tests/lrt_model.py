"""BaseType + SetBase + LRT() on 512 class counts at 50 significant digits, with a trace of every decision, and a census of
the paths the stage-2 kernels take for a case.

Written from the reference's source text (src/BaseType.cpp:25-139, 237-255, src/Algorithm.cpp:3-7, 69-130) and include/bvc.h;
standard library only (decimal), so it runs wherever the tests run.  Not a restatement of oracle/basetype_oracle.c: sums are plain
sums over the classes in 50-digit arithmetic, the error probability is 10^(-q/10) itself, log is Decimal.ln, and the chi-square
tail for one degree of freedom is erfc(sqrt(chi / 2)) by a series / a continued fraction of its own.

The reference's double-precision behaviour is kept only where it is behaviour and not rounding:
  * a class of quality 0 has likelihood 0 for its own allele: a model that gives that allele frequency 1 has marginal 0, log = -inf,
    posteriors 0/0 = NaN, and "NaN never converges" (the fit runs to the cap);
  * pass 0 and at most 100 update passes, the stop rule tested after each update pass;
  * depth / depth_total >= min_af, depth_first / depth_total > 0.5 and depth_total > 10 are comparisons of doubles that the reference,
    the oracle and the kernels all evaluate with the same correctly rounded division: the model does them in double too;
  * a subset of zero coverage is skipped (src/BaseType.cpp:54, only with min_af <= 0), the winner's bases are then read from the list
    of ALL subsets by its number among the FITTED ones, and a level without a fit is status 1;
  * var_qual = 10000 when chisf underflows to 0 in double, and chisf's subnormal range: both taken from the oracle's chisf (passed in
    as `chisf_double`), since they are properties of that double routine; where the tail is a normal double the model's own is used.

Every comparison the algorithm takes is logged with its MARGIN and is DECISIVE when the margin is above its rounding bound:
  stop rule: |delta - 1e-3| / 1e-3 > 1e-9;  chi against another chi, against 24, against 0: more than 1e-6 apart;
  prune test: the edge of tests/test_gpu_parity.py path_counts_match, 1e-6.
outcomes() returns the record of every legitimate outcome of a case: one when every comparison is decisive, otherwise one per way the
comparisons inside their bounds can fall.
"""
import collections
import decimal
import itertools
import math
import struct
from decimal import Decimal as D

PREC = 50
CTX = decimal.Context(prec=PREC, rounding=decimal.ROUND_HALF_EVEN, traps=[], Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)

LRT_THRESHOLD = D(24)            # src/BaseType.h:9
EM_ITERS = 100                   # src/BaseType.cpp:46
EM_EPS = D("0.001")              # src/BaseType.cpp:45

STOP_BOUND = D("1e-9")           # relative to 1e-3
CHI_BOUND = D("1e-6")
PRUNE_BOUND = 1e-6
MIN_NORMAL = 2.2250738585072014e-308

D0, D1, D3 = D(0), D(1), D(3)


def _hi(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def _from_hi(h):
    return struct.unpack("<d", struct.pack("<Q", h << 32))[0]


# csrc/em_common.h: hi(A) < kSureBelowHi converged, hi(A) >= kSureAboveHi not converged; as thresholds on A itself
A_BELOW = D(_from_hi(_hi(0.001 / (1.0 + 0.00390625))))
A_ABOVE = D(_from_hi(_hi(0.001 / (1.0 - 0.00390625)) + 1))
JUMP_U = D(2) ** -6              # kLog1pMaxU, csrc/em_kernel.hip


def _isnan(x):
    return x.is_nan()


_LIK = {}


def lik(q):
    """(a, e): likelihood of an observation of quality q under its own allele and under another one (src/BaseType.cpp:10-17)."""
    if q not in _LIK:
        with decimal.localcontext(CTX):
            eps = D(10) ** (D(-q) / D(10)) if q else D1
            _LIK[q] = (D1 - eps, eps / D3)
    return _LIK[q]


# ------------------------------------------------------------------------------------------------ chi-square tail, 1 d.o.f.
def erfc(x):
    """erfc(x), x >= 0, to about 45 digits: the all-positive series of erf below 3, the continued fraction above."""
    with decimal.localcontext(CTX) as c:
        c.prec = PREC + 20
        x = D(x)
        pi = _pi()
        if x < 3:
            term = x
            total = x
            n = 0
            x2 = 2 * x * x
            while True:
                n += 1
                term = term * x2 / (2 * n + 1)
                total += term
                if term < D(10) ** -(PREC + 18) * total or term == 0:
                    break
            r = D1 - 2 / pi.sqrt() * (-x * x).exp() * total
        else:
            t = x
            for k in range(900, 0, -1):          # x + (1/2)/(x + 1/(x + (3/2)/(x + ...)))
                t = x + (D(k) / 2) / t
            r = (-x * x).exp() / (pi.sqrt() * t)
    with decimal.localcontext(CTX):
        return +r


_PI = []


def _pi():
    if not _PI:
        with decimal.localcontext(CTX) as c:
            c.prec = PREC + 30
            # Machin: pi = 16 atan(1/5) - 4 atan(1/239)
            def atan_inv(n):
                x = D1 / n
                total, term, k, n2 = x, x, 0, n * n
                while True:
                    k += 1
                    term = -term / n2
                    t = term / (2 * k + 1)
                    total += t
                    if abs(t) < D(10) ** -(PREC + 28):
                        return total
            _PI.append(16 * atan_inv(5) - 4 * atan_inv(239))
    return _PI[0]


def chisf(chi):
    """P(X > chi) for X chi-square with one degree of freedom (src/Algorithm.cpp:3-7 with k = 1): erfc(sqrt(chi / 2))."""
    with decimal.localcontext(CTX):
        return erfc((D(chi) / 2).sqrt())


# ------------------------------------------------------------------------------------------------ decisions
class _Decider:
    def __init__(self, forced):
        self.forced = tuple(forced)
        self.open = []               # natural outcomes of the comparisons inside their bound, in the order met
        self.log = []

    def __call__(self, kind, outcome, margin, bound, where, branch=True):
        decisive = margin is None or _isnan(D(margin)) or D(margin) > D(bound)
        if not decisive and branch:
            i = len(self.open)
            self.open.append(bool(outcome))
            if i < len(self.forced):
                outcome = self.forced[i]
        self.log.append(dict(kind=kind, where=where, outcome=bool(outcome), decisive=bool(decisive),
                             margin=math.inf if margin is None else float(margin)))
        return bool(outcome)


def _subsets(n, k):
    return list(itertools.combinations(range(n), k))       # combs_: lexicographic by position (src/BaseType.cpp:237-255)


def _em(classes, nind, f, decide, where):
    """EM (src/Algorithm.cpp:115-130).  Returns (log-likelihood of the last pass's marginals, expect of the last pass, per-pass trace)."""
    def one_pass(fr):
        marg, ex = [], [D0, D0, D0, D0]
        for b, n, a, e in classes:
            l = [fr[j] * (a if j == b else e) for j in range(4)]
            m = l[0] + l[1] + l[2] + l[3]
            for j in range(4):
                ex[j] += n * (l[j] / m)
            marg.append(m)
        return marg, [x / nind for x in ex]

    marg, ex = one_pass(f)
    lnm = [m.ln() for m in marg]
    passes = [dict(it=0)]
    for it in range(1, EM_ITERS + 1):
        nxt, ex = one_pass(ex)
        lnn = [m.ln() for m in nxt]
        delta = A = umax = D0
        for (b, n, a, e), m0, m1, l0, l1 in zip(classes, marg, nxt, lnm, lnn):
            delta += n * abs(l1 - l0)
            u = abs(m1 / m0 - 1)
            A += n * u
            umax = u if (_isnan(u) or u > umax) and not _isnan(umax) else umax
        marg, lnm = nxt, lnn
        if _isnan(A) or A >= A_ABOVE:
            bracket = "above"
        elif A < A_BELOW:
            bracket = "below"
        else:
            bracket = "straddle"
        a_margin = math.inf if _isnan(A) else float(min(abs(A - A_BELOW) / A_BELOW, abs(A - A_ABOVE) / A_ABOVE))
        margin = None if _isnan(delta) else abs(delta - EM_EPS) / EM_EPS
        conv = decide("stop", (not _isnan(delta)) and delta < EM_EPS, margin, STOP_BOUND, (where, it))
        passes.append(dict(it=it, delta=delta, A=A, bracket=bracket, a_margin=a_margin, umax=umax, converged=conv))
        if conv:
            break
    ll = D0
    for (b, n, a, e), l in zip(classes, lnm):
        ll += n * l
    return ll, ex, passes


def _f(x):
    return float(x)


def lrt(counts, ref_base, min_af, base_comb=None, forced=(), chisf_double=None):
    """counts: {(base, qual): n} or 512 numbers.  Returns (record, trace).  The record has the keys of oracle.orc's dict (floats,
    rounded from the 50-digit values kept under "hp")."""
    if not isinstance(counts, dict):
        counts = {(i // 128, i % 128): int(c) for i, c in enumerate(counts) if c}
    with decimal.localcontext(CTX):
        return _lrt(counts, int(ref_base), float(min_af), base_comb, forced, chisf_double)


def _lrt(counts, ref_base, min_af, base_comb, forced, chisf_double):
    decide = _Decider(forced)
    classes = [(b, D(n), ) + lik(q) for (b, q), n in sorted(counts.items()) if n]
    depth = [sum(n for (b, q), n in counts.items() if b == j) for j in range(4)]
    total_i = sum(depth)
    nind = D(total_i)
    depth_total = float(total_i)
    quals = [[q for (b, q), n in counts.items() if b == j and n] for j in range(4)]
    rec = dict(called=0, n_alt=0, alt_base=[], af=[], var_qual=0.0, chi=0.0, depth_total=depth_total, depth=list(depth), kept=[],
               base_frq=[0.0] * 4, lr_alt=0.0, n_fits=0, n_passes=0, status=0, tie_gap=math.inf, n_fits_pruned=0, n_passes_pruned=0,
               prune_edge=math.inf, max_quals=max(len(x) for x in quals), min_qual=min([q for x in quals for q in x] or [127]),
               dup_candidate=0, var_qual_kind="none")
    trace = dict(fits=[], levels=[], filter=[], log=decide.log, open=decide.open, record=[])
    hp = rec["hp"] = dict(chi=D0, af=[], var_qual=D0, lr_alt=D0)
    if total_i == 0:                                           # :75
        return rec, trace
    comb = [0, 1, 2, 3] if base_comb is None else [int(b) for b in base_comb]
    bases = []
    for b in comb:                                             # :77-83
        d = depth[b] if 0 <= b <= 3 else 0                     # (a candidate that is no base has no observations)
        r = float(d) / depth_total
        keep = r >= min_af
        decide("min_af", keep, None, 0, b)
        trace["filter"].append(dict(base=b, depth=d, ratio=r, kept=keep,
                                    equal=r == min_af, one_ulp_below=math.nextafter(r, 2.0) == min_af))
        if keep:
            if b in bases:
                rec["dup_candidate"] = 1
            bases.append(b)
    n = len(bases)
    if n == 0:                                                 # :84
        return rec, trace
    if n > 4:
        rec["status"] = 2
        return rec, trace
    lle = [sum(D(c) * lik(q)[1].ln() for (b, q), c in counts.items() if b == j and c) for j in range(4)]
    counters = dict(fits=0, passes=0)

    def update_f(cur, k, level):                               # UpdateF, :41-71
        combs = [tuple(cur[p] for p in pos) for pos in _subsets(len(cur), k)]
        fitted = []
        for ci, c in enumerate(combs):
            s = sum(depth[b] for b in c if 0 <= b <= 3)
            f = [D0] * 4
            if s > 0:
                for b in c:
                    f[b] = D(depth[b]) / D(s)                  # (a repeated base keeps one entry, as the reference's array does)
            if sum(f) == 0:
                continue                                       # :54
            ll, ex, passes = _em(classes, nind, f, decide, (level, ci))
            counters["fits"] += 1
            counters["passes"] += len(passes)
            trace["fits"].append(dict(level=level, k=k, subset=c, index=ci, passes=passes, n_passes=len(passes), ll=ll))
            fitted.append(dict(ll=ll, ex=ex, n_passes=len(passes), index=ci))
        return combs, fitted

    combs, fitted = update_f(bases, n, 0)                      # :88
    if not fitted:
        rec["status"] = 1
        rec["n_fits"] = rec["n_fits_pruned"] = counters["fits"]
        rec["n_passes"] = rec["n_passes_pruned"] = counters["passes"]
        return rec, trace
    frq, lr_alt, chi = fitted[0]["ex"], fitted[0]["ll"], D0
    skipped_fits = skipped_passes = 0
    level = 0
    for k in range(n - 1, 0, -1):                              # :93-110
        level += 1
        n_in = len(bases)
        combs, fitted = update_f(bases, k, level)
        if not fitted:
            rec["status"] = 1
            break
        chis = [2 * (lr_alt - x["ll"]) for x in fitted]
        i_min = 0
        for i in range(1, len(chis)):                          # std::min_element: first minimum, '<'
            a, b = chis[i], chis[i_min]
            nan = _isnan(a) or _isnan(b)
            if decide("min", (not nan) and a < b, None if nan else abs(a - b), CHI_BOUND, (level, i)):
                i_min = i
        lv = dict(level=level, n=n_in, k=k, chis=chis, i_min=i_min, all_fitted=len(fitted) == len(combs), bases=list(bases),
                  p_deepest=None, c_last=None, ruled_out=None, deep_tie=False, prune_bound=None, prune_best=None)
        others = [c for j, c in enumerate(chis) if j != i_min and not _isnan(c) and not _isnan(chis[i_min])]
        if others:
            rec["tie_gap"] = min(rec["tie_gap"], float(min(others) - chis[i_min]))
        p_deep = 0
        for j in range(1, n_in):
            if depth[bases[j]] > depth[bases[p_deep]]:
                p_deep = j
        lv["p_deepest"] = p_deep
        lv["deep_tie"] = sum(1 for b in bases if depth[b] == depth[bases[p_deep]]) > 1
        if len(fitted) == len(combs) and len(fitted) >= 2 and k >= 2:
            # what the level need not have run (csrc/em_items.hip site_decide): the subset without the deepest candidate
            c_last = n_in - 1 - p_deep
            best_other = min(c for j, c in enumerate(chis) if j != c_last) if not any(_isnan(c) for c in chis) else D("NaN")
            u_c = sum(lle[b] for b in range(4) if b not in combs[c_last])
            bound = 2 * (lr_alt - u_c)
            slack = D1 + D("1e-6") * abs(u_c)
            lv.update(c_last=c_last, prune_bound=bound, prune_best=best_other)
            if _isnan(bound) or _isnan(best_other):
                edge, ruled = 0.0, False
            else:
                ruled = bound > best_other + slack and bound.is_finite()
                edge = float(abs(bound - (best_other + slack)) / max(abs(bound), D1))
            decide("prune", ruled, D(edge), PRUNE_BOUND, level, branch=False)
            lv["ruled_out"] = ruled
            rec["prune_edge"] = min(rec["prune_edge"], edge)
            if ruled:
                skipped_fits += 1
                skipped_passes += fitted[c_last]["n_passes"]
        lr_alt, chi = fitted[i_min]["ll"], chis[i_min]
        nan = _isnan(chi)
        goes_on = decide("chi<24", (not nan) and chi < LRT_THRESHOLD, None if nan else abs(chi - LRT_THRESHOLD), CHI_BOUND, level)
        lv["goes_on"] = goes_on
        trace["levels"].append(lv)
        if not goes_on:
            break
        bases = list(combs[i_min])                             # bc[i_min] although lr / bp skip zero-coverage subsets
        frq = fitted[i_min]["ex"]
    n = len(bases)
    rec["kept"] = list(bases)
    rec["base_frq"] = [_f(x) for x in frq]
    rec["lr_alt"], hp["lr_alt"] = _f(lr_alt), lr_alt
    rec["chi"], hp["chi"] = _f(chi), chi
    rec["n_fits"], rec["n_passes"] = counters["fits"], counters["passes"]
    rec["n_fits_pruned"], rec["n_passes_pruned"] = counters["fits"] - skipped_fits, counters["passes"] - skipped_passes
    for b in bases:                                            # :111-116
        if b != ref_base:
            rec["alt_base"].append(b)
            rec["af"].append(_f(frq[b]))
            hp["af"].append(frq[b])
    rec["n_alt"] = len(rec["alt_base"])
    if rec["n_alt"]:                                           # :117-135
        rec["called"] = 1
        r = float(depth[bases[0]]) / depth_total
        one = n == 1
        big = decide("depth_total>10", depth_total > 10, None, 0, "record")
        major = decide("r>0.5", r > 0.5, None, 0, "record")
        trace["record"] = dict(one=one, depth_total=depth_total, r=r)
        if one and big and major:
            rec["var_qual"], rec["var_qual_kind"] = 5000.0, "5000"
        elif _isnan(chi):
            rec["var_qual"], rec["var_qual_kind"] = math.nan, "nan"
        elif decide("chi<=0", chi <= 0, abs(chi) if level else None, CHI_BOUND, "record"):   # (no level run: chi is the literal 0 of :73)
            rec["var_qual"], rec["var_qual_kind"] = 0.0, "zero"
        else:
            p_double = chisf_double(float(chi)) if chisf_double else float(chisf(chi))
            if p_double == 0:
                rec["var_qual"], rec["var_qual_kind"] = 10000.0, "10000"
            elif p_double < MIN_NORMAL:
                rec["var_qual"], rec["var_qual_kind"] = -10 * math.log10(p_double), "subnormal"
            else:
                vq = -10 * chisf(chi).log10()
                rec["var_qual"], rec["var_qual_kind"], hp["var_qual"] = _f(vq), "finite", vq
            if rec["var_qual"] == 0:
                rec["var_qual"] = 0.0
    return rec, trace


def outcomes(counts, ref_base, min_af, base_comb=None, chisf_double=None, limit=16):
    """[(record, trace)] of every legitimate outcome; the natural one (every comparison as the 50-digit values fall) first."""
    done, todo = [], [()]
    while todo:
        f = todo.pop(0)
        rec, tr = lrt(counts, ref_base, min_af, base_comb, f, chisf_double)
        if len(tr["open"]) > len(f):
            nat = tr["open"][len(f)]
            todo[:0] = [f + (nat,), f + (not nat,)]
            if len(done) + len(todo) > limit:
                raise ValueError("more than %d outcomes: not a case for a catalogue" % limit)
        else:
            done.append((rec, tr))
    return done


def is_decisive(trace):
    return not trace["open"]


def closest_margins(trace):
    """{kind: smallest margin among the DECISIVE comparisons of that kind} (stop: relative to 1e-3; the chi kinds: absolute)."""
    out = {}
    for e in trace["log"]:
        if e["decisive"] and e["margin"] != math.inf:
            out[e["kind"]] = min(out.get(e["kind"], math.inf), e["margin"])
    return out


def group_records(grp_counts, ref_base, min_af, chisf_double=None):
    """The caller's --group loop (src/BaseVarC.cpp:617-661) on slots [n_groups + 1] of {(base, qual): n}; the last slot holds the
    observations of no group.  Returns (overall record, overall trace, [group dict(depth, af, ran, present, rec)])."""
    total = collections.Counter()
    for slot in grp_counts:
        total.update(slot)
    rec, tr = lrt(dict(total), ref_base, min_af, None, (), chisf_double)
    comb = [ref_base] + rec["alt_base"][:3]                    # :614-615
    groups = []
    for slot in grp_counts[:-1]:
        d = [sum(n for (b, q), n in slot.items() if b == j) for j in range(4)]
        g = dict(depth=d, af=[0.0, 0.0, 0.0], ran=0, present=0, rec=None, trace=None)
        if rec["called"] and sum(d) > 0:                       # :633-636, :641
            grec, gtr = lrt(dict(slot), ref_base, min_af, comb, (), chisf_double)
            g.update(ran=1, rec=grec, trace=gtr)
            for i, alt in enumerate(rec["alt_base"][:3]):      # :646-652
                for t, galt in enumerate(grec["alt_base"]):
                    if galt == alt:
                        g["af"][i] = grec["af"][t]
                        g["present"] |= 1 << i
        groups.append(g)
    return rec, tr, groups


# ------------------------------------------------------------------------------------------------ census
# Classes are named after the line of the device code they stand for.
REGION = ["region kind tiny: need <= 8 (em_items.hip region_body)", "region kind narrow: need <= 32", "region kind wide: need <= 48"]
LEAVE = ["site_classes leaves the site: too_wide (> 48 values on an allele)", "site_classes leaves the site: any_low (quality 0 or 1)",
         "site_classes leaves the site: dup (duplicate candidate)", "uses_item_engine false: min_af <= 0"]
WAVE = ["lrt_kernel<%d> with %d active slots (em_engine 1)" % p for p in ((2, 1), (2, 2), (4, 3), (4, 4), (8, 6), (8, 8))] + \
       ["ANY remainder launch lrt_kernel<8,ANY> with %d active slots" % a for a in (6, 8)]
EDGES = (8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 96, 97)        # both sides of every capacity of a kernel or of an active-slot count
WIDTH = ["widest allele of the site has %d quality values" % k for k in EDGES]
CAND = ["%d candidates pass the min_af filter" % i for i in range(5)] + \
       ["candidate kept at depth / depth_total == min_af", "candidate dropped one ulp below min_af",
        "ref_base inside 0..3", "ref_base outside 0..3"] + \
       ["base_comb of length %d" % i for i in range(5)] + ["base_comb reordered", "base_comb with a duplicate", "base_comb with a non-ACGT entry"]
LEVEL = ["level of n = %d: deepest candidate at position %d" % (n, p) for n in (2, 3, 4) for p in range(n)] + \
        ["level of n = %d: deepest at %d, subset %d wins in round %d" % (n, p, i, 2 if i == n - 1 - p else 1)
         for n in (3, 4) for p in range(n) for i in range(n)] + \
        ["level of n = %d: last-resort subset %s" % (n, w) for n in (3, 4) for w in ("ruled out", "run")] + \
        ["level of n = %d: %s" % (n, w) for n in (2, 3, 4) for w in ("ends at chi >= 24", "goes on")] + \
        ["one-allele level: deepest at %d, candidate %d wins" % (p, i) for p in (0, 1) for i in (0, 1)] + \
        ["level goes on with chi in (23.9, 24)", "level ends with chi in (24, 24.1)", "deepest_position with equal depths"]
STOP = ["fit converges at its second pass", "fit reaches the cap of 101 passes", "pass sure-below (hi(A) < kSureBelowHi)",
        "pass sure-above (hi(A) >= kSureAboveHi)", "pass in the straddle band that converged", "pass in the straddle band that did not",
        "wave engine: jump pass (|u| > 2^-6) after the first update pass"]
QUIRK = ["status 1: a level without a fit", "subset of zero coverage skipped (src/BaseType.cpp:54)"]
RECORD = ["call_var_qual: 5000", "call_var_qual: 0 (chi <= 0)", "var_qual pending then finite", "var_qual pending then 10000", "var_qual NaN",
          "called 0: no candidate", "called 0: the accepted model is the reference base alone", "called 0: no observation"] + \
         ["n_alt = %d" % i for i in (1, 2, 3)] + ["depth_total = 10 at the 5000 rule", "depth_total = 11 at the 5000 rule", "r = 0.5 exactly at the 5000 rule",
                                                  "a single class of 2^31 - 1 observations", "depth_total = 2^31 - 1 over several classes",
                                                  "chi in (-0.05, 0) after a level", "chi in (0, 0.05) after a level"]
GROUP = ["group: overall site not called, depths only", "group: called, a group of zero depth (ran = 0)"] + \
        ["group: n_alt = %d, present = %d" % (n, m) for n in (1, 2, 3) for m in range(1 << n)] + \
        ["group: its own ALT index differs from the overall one", "group: ref outside 0..3"]
TIES = ["exact tie among the subsets of a level of n = %d" % n for n in (2, 3, 4)]
ALL_CLASSES = REGION + LEAVE + WAVE + WIDTH + CAND + LEVEL + STOP + QUIRK + RECORD + GROUP + TIES


def census(counts, ref_base, min_af, base_comb, rec, trace, device_comb=False):
    """The classes a case reaches (a set of names from ALL_CLASSES), from the case and the model's trace."""
    with decimal.localcontext(CTX):
        return _census(ref_base, min_af, base_comb, rec, trace, device_comb)


def _census(ref_base, min_af, base_comb, rec, trace, device_comb):
    out = set()
    need = rec["max_quals"]
    nslots = (need + 15) >> 4
    if need in EDGES:
        out.add(WIDTH[EDGES.index(need)])
    out.add(WAVE[0 if nslots <= 1 else 1 if nslots == 2 else 2 if nslots == 3 else 3 if nslots == 4 else 4 if nslots <= 6 else 5])
    left = []
    if min_af <= 0:
        left.append(LEAVE[3])
    else:
        if need > 48:
            left.append(LEAVE[0])
        if rec["min_qual"] < 2:
            left.append(LEAVE[1])
        if rec["dup_candidate"]:
            left.append(LEAVE[2])
    out.update(left)
    if left:
        out.add(WAVE[6 if nslots <= 6 else 7])
    else:
        out.add(REGION[0 if need <= 8 else 1 if need <= 32 else 2])
    if rec["depth_total"] > 0:
        n_cand = sum(1 for f in trace["filter"] if f["kept"])
        if n_cand <= 4:
            out.add(CAND[n_cand])
        for f in trace["filter"]:
            if f["kept"] and f["equal"] and min_af > 0:
                out.add(CAND[5])
            if not f["kept"] and f["one_ulp_below"] and f["depth"] > 0:
                out.add(CAND[6])
    out.add(CAND[7 if 0 <= ref_base <= 3 else 8])
    if base_comb is not None:
        comb = list(base_comb)
        out.add(CAND[9 + len(comb)])
        acgt = [b for b in comb if 0 <= b <= 3]
        if acgt != sorted(acgt):
            out.add(CAND[14])
        if len(set(acgt)) < len(acgt):
            out.add(CAND[15])
        if len(acgt) < len(comb) and device_comb:
            out.add(CAND[16])
    if rec["status"] == 1:
        out.add(QUIRK[0])
    for lv in trace["levels"]:
        n = lv["n"]
        if not lv["all_fitted"]:
            out.add(QUIRK[1])
            continue
        out.add("level of n = %d: deepest candidate at position %d" % (n, lv["p_deepest"]))
        if lv["deep_tie"]:
            out.add(LEVEL[-1])
        chis = lv["chis"]
        tie = any(j != lv["i_min"] and not _isnan(c) and abs(c - chis[lv["i_min"]]) <= CHI_BOUND for j, c in enumerate(chis))
        if tie:
            out.add("exact tie among the subsets of a level of n = %d" % n)
        if n >= 3:
            i = lv["i_min"]
            out.add("level of n = %d: deepest at %d, subset %d wins in round %d" % (n, lv["p_deepest"], i, 2 if i == lv["c_last"] else 1))
            out.add("level of n = %d: last-resort subset %s" % (n, "ruled out" if lv["ruled_out"] else "run"))
        else:
            out.add("one-allele level: deepest at %d, candidate %d wins" % (lv["p_deepest"], lv["i_min"]))
        if not _isnan(chis[lv["i_min"]]) and abs(chis[lv["i_min"]] - LRT_THRESHOLD) < D("0.1"):
            out.add("level goes on with chi in (23.9, 24)" if lv["goes_on"] else "level ends with chi in (24, 24.1)")
        out.add("level of n = %d: %s" % (n, "goes on" if lv["goes_on"] else "ends at chi >= 24"))
    for fit in trace["fits"]:
        if fit["k"] < 2:
            continue                                           # one-allele models: closed form in the item engine
        if fit["n_passes"] == 2:
            out.add(STOP[0])
        if fit["n_passes"] == EM_ITERS + 1 and not fit["passes"][-1]["converged"]:
            out.add(STOP[1])
        for p in fit["passes"][1:]:
            if p["a_margin"] <= 1e-9:
                continue
            if p["bracket"] == "below":
                out.add(STOP[2])
            elif p["bracket"] == "above":
                out.add(STOP[3])
            else:
                out.add(STOP[4 if p["converged"] else 5])
            if p["it"] >= 2 and not _isnan(p["umax"]) and p["umax"] > JUMP_U * D("1.000001"):
                out.add(STOP[6])
    if rec["depth_total"] == 2.0 ** 31 - 1:
        out.add(RECORD[14 if max(rec["depth"]) == 2 ** 31 - 1 and rec["max_quals"] == 1 else 15])
    if trace["levels"] and rec["called"] and rec["chi"] != 0 and abs(rec["chi"]) < 0.05:
        out.add(RECORD[16 if rec["chi"] < 0 else 17])
    kind = rec["var_qual_kind"]
    if kind in ("5000", "zero", "finite", "10000", "nan"):
        out.add(RECORD[("5000", "zero", "finite", "10000", "nan").index(kind)])
    if not rec["called"]:
        out.add(RECORD[7] if rec["depth_total"] == 0 else RECORD[5] if not rec["kept"] else RECORD[6])
    elif 1 <= rec["n_alt"] <= 3:
        out.add("n_alt = %d" % rec["n_alt"])
    if rec["called"] and len(rec["kept"]) == 1:
        r = trace["record"]
        if r["depth_total"] == 10 and r["r"] > 0.5:
            out.add(RECORD[11])
        if r["depth_total"] == 11 and r["r"] > 0.5:
            out.add(RECORD[12])
        if r["depth_total"] > 10 and r["r"] == 0.5:
            out.add(RECORD[13])
    return out


def group_census(ref_base, rec, groups):
    out = set()
    if not 0 <= ref_base <= 3:
        out.add(GROUP[-1])
    for g in groups:
        if not rec["called"]:
            out.add(GROUP[0])
            continue
        if not g["ran"]:
            out.add(GROUP[1])
            continue
        n_alt = min(rec["n_alt"], 3)
        out.add("group: n_alt = %d, present = %d" % (n_alt, g["present"]))
        for i, alt in enumerate(rec["alt_base"][:3]):
            if alt in g["rec"]["alt_base"] and g["rec"]["alt_base"].index(alt) != i:
                out.add(GROUP[-2])
    return out
