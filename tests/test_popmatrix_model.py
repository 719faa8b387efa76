"""The two forms of popmatrix's rule (tests/popmatrix_model.py) against each other, no device: FetchAlleleType's stateful loop -- what the
host program's CPU path follows -- and the stateless per-position form the device computes.  They agree wherever the positions do not
descend (duplicates included); a hand-built descending list shows them apart, which is why the device path refuses such a position file."""
import numpy as np

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import popmatrix_model as pm

N_SAMPLES = 2400


def random_sample(seed):
    """(kept reads sorted by start, [(pos, ref, alt)] not descending with duplicates, refseq, rg_s)"""
    rng = np.random.default_rng(seed)
    rg_s = int(rng.integers(1000, 1100))
    n_span = int(rng.integers(40, 300))
    refseq = "".join(rng.choice(list("ACGT"), n_span + 60))
    starts = np.sort(rng.integers(rg_s - 30, rg_s + n_span, int(rng.integers(0, 25))))
    rv = [bc.random_read(rng, int(p)) for p in starts]
    rv = [r for r in rv if not (r["flag"] & 0x404)]
    pv = []
    for p in range(rg_s - 5, rg_s + n_span + 5):
        for _ in range(int(rng.choice([0, 1, 1, 1, 1, 1, 2, 3]))):       # gaps, and a site on two or three lines
            ref, alt = rng.choice(list("ACGTN="), 2)
            pv.append((p, str(ref), str(alt)))
    return rv, pv, refseq, rg_s


def test_the_stateful_loop_is_the_stateless_form_where_positions_do_not_descend():
    cells = {"0": 0, "1": 0, ".": 0}
    ops, raised, dup, fell = set(), 0, 0, 0
    for seed in range(20261101, 20261101 + N_SAMPLES):
        rv, pv, refseq, rg_s = random_sample(seed)
        assert all(a[0] <= b[0] for a, b in zip(pv, pv[1:]))
        dup += sum(1 for a, b in zip(pv, pv[1:]) if a[0] == b[0])
        for r in rv:
            ops.update(op for op, _ in r["cigar"])
        try:
            a = pm.fetch_allele_type(rv, pv, refseq, rg_s)
        except IndexError:
            a = None
        try:
            b = pm.stateless_row(rv, pv, refseq, rg_s)
        except IndexError:
            b = None
        assert a == b, (seed, a, b)
        if a is None:
            raised += 1
            continue
        assert len(a) == len(pv)
        for ch in a:
            cells[ch] += 1
        # a character from a read behind the first one that has not ended in front of the position: the fall-through on D / N
        for (pos, _, _), ch in zip(pv, a):
            first = next((r for r in rv if bm.tp.end_pos(r) >= pos), None)
            if ch != "." and first is not None and any(o in "DN" for o, _ in first["cigar"]):
                k = bm.tp.find_snp_at_pos([first], [pos], refseq=bm.Checked(refseq), rg_s=rg_s).get(pos)
                fell += k is None
    assert N_SAMPLES >= 2000 and set("MIDNSHP=X") <= ops, sorted(ops)
    assert cells["0"] > 5000 and cells["1"] > 5000 and cells["."] > 50000 and dup > 10000 and fell > 0, (cells, dup, fell, raised)


def test_a_descending_list_tells_the_two_forms_apart():
    """Two reads, 1010-1019 and 1030-1039.  Asked for 1035 and then for 1012, the reference's cursor already stands on the second read,
    which starts behind 1012: a dot.  The stateless form finds the first read again."""
    rv = [bm.make_read(1009, "10M", seq="A" * 10), bm.make_read(1029, "10M", seq="C" * 10)]
    refseq = "A" * 100
    down = [(1035, "C", "A"), (1012, "A", "C")]
    assert pm.fetch_allele_type(rv, down, refseq, 1000) == "0."
    assert pm.stateless_row(rv, down, refseq, 1000) == "00"
    up = sorted(down)
    assert pm.fetch_allele_type(rv, up, refseq, 1000) == pm.stateless_row(rv, up, refseq, 1000) == "00"


def test_the_characters_are_compared_not_the_classes():
    """A read's N is the character N: it matches a REF of N, not a REF of '=' or of lowercase n; REF is tried before ALT."""
    rv = [bm.make_read(1009, "4M", seq="ANGA")]
    pv = [(1010, "A", "A"), (1011, "N", "A"), (1011, "=", "N"), (1011, "n", "a"), (1012, "g", "G"), (1013, "C", "T")]
    for form in (pm.fetch_allele_type, pm.stateless_row):
        assert form(rv, pv, "A" * 50, 1000) == "001.1."
