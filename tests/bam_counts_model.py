"""Plain Python / numpy model of bvc_bam_counts (include/bvc_bam_counts.h), no device: the entries of tests/bam_pileup_model.py folded into
class counts, group counts and tallies; and revisit(), the rule that says which positions a run that piled phase 1 into counts must read
again entry by entry (host/pileup.h, counts_revisit)."""
import numpy as np

from tests import bam_pileup_model as bm

NCLASS = 512
TALLY = np.dtype([("strand_base", "<u4", (8,)), ("n_other", "<u4"), ("n_indel", "<u4"), ("pad", "<u4", (2,))])
CALLED, INDEL, CARRY = 1, 2, 4
assert TALLY.itemsize == 48


def slots_of(n_groups):
    return n_groups + 1 if n_groups else 1


def fold(maps, positions, group_of_sample=None, n_groups=0):
    """maps: [{pos: entry}] per sample (bam_pileup_model.expected()["maps"]).  (counts uint32 [P, slots, 512], tally TALLY [P]): what a call
    that returns BVC_OK adds."""
    P = len(positions)
    counts = np.zeros((P, slots_of(n_groups), NCLASS), dtype=np.uint32)
    tally = np.zeros(P, dtype=TALLY)
    at = {int(p): t for t, p in enumerate(positions)}
    for s, m in enumerate(maps):
        slot = min(int(group_of_sample[s]), n_groups) if n_groups else 0
        for p, e in m.items():
            t = at[int(p)]
            if e["is_indel"]:
                tally["n_indel"][t] += 1
            elif e["base"] > 3:
                tally["n_other"][t] += 1
            else:
                tally["strand_base"][t, (e["strand"] & 1) << 2 | e["base"]] += 1
                if e["qual"] < 128:
                    counts[t, slot, e["base"] * 128 + e["qual"]] += 1
    return counts, tally


def expected(samples, beg0, end0, min_mapq, positions, rg_s, refseq_len, group_of_sample=None, n_groups=0, exp=None):
    """dict(rc, status, counts, tally): what bvc_bam_counts returns, writes to sample_status and ADDS; counts and tally are None unless rc
    is OK.  Only the reference's length reaches the call: the model's rule takes a text of that length.  exp: bam_pileup_model.expected() of
    the same inputs where the caller has it."""
    if exp is None:
        exp = bm.expected(samples, beg0, end0, min_mapq, positions, rg_s, "N" * refseq_len)
    if exp["rc"] != bm.OK:
        return dict(rc=exp["rc"], status=exp["status"], counts=None, tally=None)
    counts, tally = fold(exp["maps"], positions, group_of_sample, n_groups)
    return dict(rc=bm.OK, status=exp["status"], counts=counts, tally=tally)


def thread_window(psize, thread, i):
    """host/pileup.cpp, thread_window"""
    window = psize % thread + psize // thread
    lo = min(psize, i * window)
    return lo, (psize if i == thread - 1 else min(psize, (i + 1) * window))


def revisit(tally, called, thread, carry=True):
    """flags uint8 [P] (CALLED | INDEL | CARRY; 0: the position's CVG line is made from its tally).  carry=False: the rule without its
    third part (the tests show that it is then not sufficient)."""
    P = len(tally)
    flags = np.zeros(P, dtype=np.uint8)
    bases = tally["strand_base"].astype(np.int64).sum(axis=1) + tally["n_other"].astype(np.int64)
    for i in range(thread):
        lo, hi = thread_window(P, thread, i)
        last = None
        for t in range(lo, hi):
            if called[t]:
                flags[t] |= CALLED
            if tally["n_indel"][t] > 0:
                flags[t] |= INDEL
                if carry and last is not None:
                    flags[last] |= CARRY
            if bases[t] > 0:
                last = t
    return flags
