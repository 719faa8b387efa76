"""Plain Python / numpy model of bvc_bam_counts_depth (include/bvc_bam_group_depth.h), no device: what tests/bam_counts_model.py says
bvc_bam_counts adds with the same labels, folded once more -- the depth of group g per base is the sum over the 128 quality classes of that
base in slot g (slot n_groups, "in no group", is left out), and the one slot of counts is the sum of all slots.  And group_map(), the rule
by which the host program labels samples and finds its columns' depth rows (host/pileup.h, counts_group_map)."""
import numpy as np

from tests import bam_counts_model as cm

NCLASS = cm.NCLASS


def fold(grouped_counts, n_groups):
    """grouped_counts uint32 [P, n_groups + 1, 512] -> (counts uint32 [P, 512], depth uint32 [P, n_groups, 4])."""
    P = grouped_counts.shape[0]
    assert n_groups >= 1 and grouped_counts.shape == (P, n_groups + 1, NCLASS)
    depth = grouped_counts[:, :n_groups].reshape(P, n_groups, 4, 128).sum(axis=3, dtype=np.uint32)
    return grouped_counts.sum(axis=1, dtype=np.uint32), depth


def fold_maps(maps, positions, group_of_sample, n_groups):
    """The same from the entries themselves (bam_counts_model.fold's loop), without the grouped counts in between -- for position lists whose
    [P, n_groups + 1, 512] would not fit.  (counts [P, 512], tally TALLY [P], depth [P, n_groups, 4])."""
    counts, tally = cm.fold(maps, positions)
    depth = np.zeros((len(positions), n_groups, 4), dtype=np.uint32)
    at = {int(p): t for t, p in enumerate(positions)}
    for s, m in enumerate(maps):
        g = int(group_of_sample[s])
        if g >= n_groups:
            continue
        for p, e in m.items():
            if not e["is_indel"] and e["base"] <= 3 and e["qual"] < 128:
                depth[at[int(p)], g, e["base"]] += 1
    return counts.reshape(len(positions), NCLASS), tally, depth


def expected(samples, beg0, end0, min_mapq, positions, rg_s, refseq_len, group_of_sample, n_groups, exp=None):
    """dict(rc, status, counts [P, 512], tally, depth [P, n_groups, 4]): what bvc_bam_counts_depth returns, writes to sample_status and
    ADDS; the three arrays are None unless rc is OK."""
    e = cm.expected(samples, beg0, end0, min_mapq, positions, rg_s, refseq_len, group_of_sample, n_groups, exp=exp)
    if e["counts"] is None:
        return dict(rc=e["rc"], status=e["status"], counts=None, tally=None, depth=None)
    counts, depth = fold(e["counts"], n_groups)
    return dict(rc=e["rc"], status=e["status"], counts=counts, tally=e["tally"], depth=depth)


def group_map(lines, samples):
    """lines: [(sample id, group name)] of the group file in order; samples: the sample names.  (names: the file's distinct group names,
    sorted; label per sample: its group's index among them, 255 when the file does not list it -- a sample listed twice keeps its first
    line; column_file_index: per group that has a sample, in sorted order, its index among names)."""
    names = sorted({g for _, g in lines})
    first = {}
    for i, g in lines:
        first.setdefault(i, names.index(g))
    label = [first.get(s, 255) if first.get(s, 255) < 255 else 255 for s in samples]
    present = {first[s] for s in samples if s in first}
    return names, label, sorted(present)
