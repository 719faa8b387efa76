"""Plain Python / numpy model of bvc_bam_counts_quals and of the accumulator's third kind (include/bvc_site_acc_quals.h), no device: what
tests/bam_counts_model.py says bvc_bam_counts adds without groups, cut to the first n_quals quality columns of each base --
narrow[t, b, q] = wide[t, 0, b * 128 + q] for q < n_quals --, the depth rows of tests/bam_group_depth_model.py, sample status 5 with the
precedence the header states (a sample of status 4 stays 4), the return code, and expand(), the way back to the [512] layout."""
import numpy as np

from tests import bam_counts_model as cm
from tests import bam_group_depth_model as gm
from tests import bam_pileup_model as bm

NCLASS = cm.NCLASS


def quals_ok(n_quals):
    return 4 <= n_quals <= 128 and n_quals % 4 == 0


def acc_bytes(n_positions, n_quals, n_groups=0):
    """What bvc_site_acc_bytes reports for an accumulator of the third kind."""
    return n_positions * (16 * n_quals + 48 + 16 * n_groups)


def narrow(wide, n_quals):
    """uint32 [P, 512] or [P, 1, 512] -> [P, 4, n_quals]: the first n_quals quality columns of each base."""
    P = wide.shape[0]
    return np.ascontiguousarray(wide.reshape(P, 4, 128)[:, :, :n_quals])


def expand(rows):
    """uint32 [P, 4, n_quals] -> [P, 512], zeros in the columns >= n_quals: what bvc_site_acc_get delivers."""
    P, four, Q = rows.shape
    assert four == 4 and quals_ok(Q)
    wide = np.zeros((P, 4, 128), dtype=np.uint32)
    wide[:, :, :Q] = rows
    return wide.reshape(P, NCLASS)


def counted_qualities(maps):
    """The quality bytes of every entry that adds a class count in the wide call: base 0..3, quality 0..127."""
    return [e["qual"] for m in maps for e in m.values() if not e["is_indel"] and e["base"] <= 3 and e["qual"] < 128]


def statuses(exp, n_quals):
    """bam_pileup_model.expected()'s statuses with status 5: a sample of status 0 that holds a counted observation of quality
    n_quals..127.  A sample the model gave status 4 has no entries left and stays 4 -- the header's precedence."""
    out = list(exp["status"])
    for s, m in enumerate(exp["maps"]):
        if out[s] == 0 and any(q >= n_quals for q in counted_qualities([m])):
            out[s] = 5
    return out


def expected(samples, beg0, end0, min_mapq, positions, rg_s, refseq_len, n_quals, group_of_sample=None, n_groups=0, exp=None):
    """dict(rc, status, counts [P, 4, n_quals], tally, depth [P, n_groups, 4] or None): what bvc_bam_counts_quals returns, writes to
    sample_status and ADDS; the arrays are None unless rc is OK.  The existing verdict (statuses 2, 3, 4) goes first; a call it would pass
    is ERR_DATA when a sample has status 5."""
    assert quals_ok(n_quals) and 0 <= n_groups <= 32
    if exp is None:
        exp = bm.expected(samples, beg0, end0, min_mapq, positions, rg_s, "N" * refseq_len)
    status = statuses(exp, n_quals)
    rc = exp["rc"] if exp["rc"] != bm.OK else bm.ERR_DATA if 5 in status else bm.OK
    if rc != bm.OK:
        return dict(rc=rc, status=status, counts=None, tally=None, depth=None)
    if n_groups:
        wide, tally, depth = gm.fold_maps(exp["maps"], positions, group_of_sample, n_groups)
    else:
        (wide, tally), depth = cm.fold(exp["maps"], positions), None
    return dict(rc=rc, status=status, counts=narrow(wide, n_quals), tally=tally, depth=depth)
