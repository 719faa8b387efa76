"""bvc_bam_counts, bvc_bam_counts_bgzf_acc and bvc_site_acc_* on the device (bam_counts_kernel.hip, bvc_bam_counts.hip; GPU) against the plain
model (tests/bam_counts_model.py: the entries of tests/bam_pileup_model.py folded into counts and tallies).

1. Every case of tests/bam_pileup_cases.py and 200 seeded random batches, from host and from device pointers: the return code and statuses
   are the model's (for the failing catalogue cases also bvc_bam_pileup's own), and both arrays -- pre-filled with random words, 0xFFFFFFFF
   wherever the model adds among them, guard words in front and behind -- hold the old words plus the model's, modulo 2^32, after BVC_OK
   and exactly the old words after anything else.
2. The shapes that send the kernel down every path: positions around a wavefront and past the grid's 1024 chunks, samples around a
   workgroup's four, none of either, quality bytes 127 / 128 / 255.
3. Groups against bvc_counts_add_csr_group_labels / bvc_counts_add_csr on the entries of bvc_bam_pileup's records of the same batch.
4. The accumulator: four threads' contexts adding into one, the 100 test BAMs through the _bgzf_acc form, a damaged block, the refusals,
   bvc_site_acc_lrt against bvc_lrt_hist[_groups] and against the bin path's called flags, no allocation in a second call."""
import threading

import numpy as np
import pytest

from tests import bam_counts_model as cm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

pytestmark = pytest.mark.gpu

GUARD = 64
GUARD_WORD = 0xCDCDCDCD
ERR_ARG, ERR_ALLOC, ERR_DATA = -1, -4, -5
MIN_AF = 0.001
CATALOGUE = bc.catalogue()
TW = cm.TALLY.itemsize // 4                     # words of a tally


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def arrays(c):
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    return (np.frombuffer(bam, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(end, dtype=np.int64), np.array(eof, dtype=np.uint8),
            np.array(rid, dtype=np.int32), np.array(c["positions"], dtype=np.int32))


def labels_of(c, n_groups, seed=0):
    """One label per sample, 0 .. n_groups + 2: the last three are labels outside the groups."""
    return np.random.default_rng(1000 + seed).integers(0, n_groups + 3, size=len(c["samples"])).astype(np.uint8) if n_groups else None


_MODEL = {}


def model_of(c, n_groups=0, labels=None):
    """The model's result for a case, folded once."""
    key = (c["name"], n_groups, None if labels is None else labels.tobytes())
    if key not in _MODEL:
        if len(_MODEL) > 8:
            _MODEL.clear()
        _MODEL[key] = cm.expected(None, None, None, None, c["positions"], None, None, labels, n_groups, exp=bc.expected(c))
    return _MODEL[key]


def guarded(rng, want):
    """GUARD words, the array pre-filled with random words (0xFFFFFFFF at half of the places the model adds to, and at a few others), GUARD
    words.  want: the model's words, or None."""
    n = 0 if want is None else want.size
    buf = np.full(n + 2 * GUARD, GUARD_WORD, dtype=np.uint32)
    pre = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        hot = np.flatnonzero(want.reshape(-1))
        pre[hot[::2]] = 0xFFFFFFFF
        pre[rng.integers(0, n, size=min(n, 16))] = 0xFFFFFFFF
    buf[GUARD:GUARD + n] = pre
    return buf, pre


def run(ctx, c, device, n_groups=0, labels=None):
    """One bvc_bam_counts call on guarded, pre-filled arrays.  Returns (rc or the BvcError's status, sample_status with its guard, counts
    buffer, its old words, tally buffer, its old words)."""
    from basevarc_amd.lib import BvcError
    exp = model_of(c, n_groups, labels)
    bam, off, end, eof, rid, pos = arrays(c)
    n, P = len(rid), len(pos)
    rng = np.random.default_rng(len(bam) + 7 * P + n_groups)
    shape = np.zeros(P * cm.slots_of(n_groups) * cm.NCLASS if n else 0, dtype=np.uint32), np.zeros(P * TW if n else 0, dtype=np.uint32)
    wc = exp["counts"] if exp["counts"] is not None else shape[0]
    wt = exp["tally"].view(np.uint32) if exp["tally"] is not None else shape[1]
    cbuf, cpre = guarded(rng, wc)
    tbuf, tpre = guarded(rng, wt)
    status = np.full(n + GUARD, GUARD_WORD, dtype=np.uint32)
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        d_c, d_t, d_s = dev(cbuf), dev(tbuf), dev(status)
        args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], len(c["refseq"])]
        out = (d_c[GUARD:GUARD + len(cpre)], d_t[GUARD:GUARD + len(tpre)])
        kw = dict(group_of_sample=dev(labels) if labels is not None else None, n_groups=n_groups, sample_status=d_s)
    else:
        args = [bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"])]
        out = (cbuf[GUARD:GUARD + len(cpre)], tbuf[GUARD:GUARD + len(tpre)])
        kw = dict(group_of_sample=labels, n_groups=n_groups, sample_status=status)
    try:
        rc, _ = ctx.bam_counts(*args, *out, **kw)
    except BvcError as e:
        rc = e.status
    if device:
        ctx.synchronize()
        cbuf, tbuf, status = (x.cpu().numpy().view(np.uint32) for x in (d_c, d_t, d_s))
    return rc, status, cbuf, cpre, tbuf, tpre


def check(c, got, n_groups=0, labels=None):
    """What a call left, against the model: old + model (mod 2^32) after BVC_OK, the old words otherwise, the guards as they were."""
    exp = model_of(c, n_groups, labels)
    rc, status, cbuf, cpre, tbuf, tpre = got
    n = len(c["samples"])
    assert rc == exp["rc"], (c["name"], rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], list(status[:n]), exp["status"])
    assert (status[n:] == GUARD_WORD).all(), c["name"]
    for buf, pre, want in ((cbuf, cpre, exp["counts"]), (tbuf, tpre, exp["tally"])):
        assert (buf[:GUARD] == GUARD_WORD).all() and (buf[GUARD + len(pre):] == GUARD_WORD).all(), c["name"]
        body = buf[GUARD:GUARD + len(pre)]
        if rc == bm.OK and want is not None and len(pre):
            w = want.view(np.uint32).reshape(-1)
            bad = np.flatnonzero(body != pre + w)           # (uint32 arithmetic wraps)
            assert bad.size == 0, (c["name"], bad[:8], body[bad[:8]], pre[bad[:8]], w[bad[:8]])
        else:
            assert (body == pre).all(), c["name"]


# ---- 1. the catalogue and the random batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_catalogue_case(ctx, c, device):
    from basevarc_amd.lib import BvcError
    got = run(ctx, c, device)
    check(c, got)
    if got[0] != bm.OK and not device:
        # a data verdict: the code and the statuses are bvc_bam_pileup's own for the same inputs
        bam, off, end, eof, rid, pos = arrays(c)
        try:
            rc, _, _, st, _ = ctx.bam_pileup(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"],
                                             np.frombuffer(c["refseq"].encode(), dtype=np.uint8))
        except BvcError as e:
            rc, st = e.status, None
        assert rc == got[0]
        if st is not None:
            assert list(st[:len(rid)]) == list(got[1][:len(rid)])


def test_the_catalogue_holds_every_verdict():
    seen = {(bc.expected(c)["rc"], s) for c in CATALOGUE for s in set(bc.expected(c)["status"]) & {2, 3, 4}}
    assert {rc for rc, _ in seen} == {bm.BAM_MORE, ERR_DATA} and {s for _, s in seen} == {2, 3, 4}, seen


RANDOM_SEEDS = tuple(range(20270000, 20270200))


@pytest.mark.parametrize("part", range(4))
def test_two_hundred_seeded_random_batches(ctx, part):
    """Each from host and from device pointers; every other one with three groups and labels outside them."""
    rcs = set()
    for seed in RANDOM_SEEDS[part * 50:(part + 1) * 50]:
        c = bc.random_case(seed)
        n_groups = 3 if seed % 2 else 0
        labels = labels_of(c, n_groups, seed)
        for device in (False, True):
            got = run(ctx, c, device, n_groups, labels)
            check(c, got, n_groups, labels)
        rcs.add(got[0])
        bc._EXPECTED.pop(c["name"], None)                    # (the catalogue's cache is not for two hundred one-off cases)
    assert rcs == {bm.OK, bm.BAM_MORE, ERR_DATA}, rcs


# ---- 2. the shapes ----------------------------------------------------------------------------------------------------------------------
def span_case(P, n_samples=5):
    """P consecutive positions ending inside the samples' last reads; reads at both ends of the list (and in the middle of a long one),
    an insertion and a deletion among them, so that the first and the last position hold entries."""
    hi = 70000 + 40
    lo = hi - P + 1
    samples = []
    for s in range(n_samples):
        reads = [bc.R(lo - 1 - s % 3, "6M2I8M" if s % 2 else "5M1D9M", mapq=30 + s)]
        if P > 200:
            reads.append(bc.R(lo + P // 2 + s, "30M", mapq=25 + s))
        if P > 20:
            reads.append(bc.R(hi - 12 - s, "4M1I20M" if s % 2 == 0 else "30M", mapq=40 + s))
        samples.append(bc.sample(reads))
    return bc.case(f"span {P} x {n_samples}", samples, range(lo, hi + 1), rg_s=1000, refseq="A" * 80000)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 65537])
def test_positions_around_a_wavefront_and_past_the_grids_chunks(ctx, P):
    """65,537 positions: 1025 chunks of 64 for a grid of 1024, so the last position is reached in the stride loop's second trip."""
    c = span_case(P)
    exp = model_of(c)
    assert exp["rc"] == 0 and exp["tally"]["strand_base"][0].sum() > 0 and exp["tally"]["strand_base"][P - 1].sum() > 0
    if P > 20:
        assert exp["tally"]["n_indel"].sum() > 0
    for device in (False, True):
        check(c, run(ctx, c, device))
    bc._EXPECTED.pop(c["name"], None)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_samples_either_side_of_a_workgroups_four(ctx, n):
    c = span_case(100, n)
    labels = labels_of(c, 2, n)
    for device in (False, True):
        check(c, run(ctx, c, device, 2, labels), 2, labels)
    bc._EXPECTED.pop(c["name"], None)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_samples_and_no_positions_are_no_ops(ctx, device):
    some = span_case(10, 3)
    for c in (bc.case("no samples here", [], some["positions"]), bc.case("no positions here", some["samples"], [])):
        got = run(ctx, c, device)
        assert got[0] == 0
        check(c, got)
        bc._EXPECTED.pop(c["name"], None)
    # no samples, but arrays to leave alone: not a word of them changes
    import ctypes as C
    counts, tally = np.full(10 * 512, 7, dtype=np.uint32), np.full(10 * TW, 9, dtype=np.uint32)
    pos = np.arange(1, 11, dtype=np.int32)
    if not device:
        p = lambda a: C.c_void_p(a.ctypes.data)
        assert ctx._L.bvc_bam_counts(ctx._h, 0, None, 0, None, None, None, None, 0, 100, 20, 10, p(pos), 1, 50, None, 0, p(counts), p(tally), None, 0) == 0
        assert (counts == 7).all() and (tally == 9).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_quality_bytes_127_128_and_255_are_tallied_and_counted_only_at_127(ctx, device):
    quals = [0, 126, 127, 128, 129, 254, 255, 40]
    c = bc.case("quality bytes", [bc.sample([bc.R(1010, "8M", seq="ACGTACGT", qual=quals)]), bc.sample([bc.R(1010, "8M", seq="TTTTTTTT", qual=quals[::-1], flag=16)])],
                bc.span(1008, 1022))
    exp = model_of(c)
    t0 = c["positions"].index(1011)
    assert exp["tally"]["strand_base"][t0:t0 + 8].sum() == 16 and exp["counts"][t0:t0 + 8].sum() == 8
    assert [int(exp["counts"][t0 + i].sum()) for i in range(8)] == [2, 1, 1, 0, 0, 1, 1, 2]
    check(c, run(ctx, c, device))


# ---- 3. groups: the library's own counts of the same batch's entries ------------------------------------------------------------------
def entries_of_records(records, rec_start, P):
    """(offsets int64 [P + 1], bases, quals, sample of each observation) of the base entries of a batch's binary records."""
    offsets, bases, quals, samples = [0], [], [], []
    data = bytes(records)
    for t in range(P):
        at, end = int(rec_start[t]) + 4, int(rec_start[t + 1])
        while at < end:
            s = int.from_bytes(data[at:at + 4], "little")
            base, _, qual, _, flags = data[at + 4:at + 9]
            at += 9
            if flags & 2:
                at += 2 + int.from_bytes(data[at:at + 2], "little")
                continue
            bases.append(base); quals.append(qual); samples.append(s)
        offsets.append(len(bases))
    return np.array(offsets, dtype=np.int64), np.array(bases, dtype=np.uint8).view(np.int8), np.array(quals, dtype=np.uint8).view(np.int8), np.array(samples, dtype=np.int64)


@pytest.mark.parametrize("n_groups", [0, 1, 5, 32])
def test_the_counts_are_the_librarys_own_of_the_pileups_entries(ctx, n_groups):
    names = ("300 samples", "every CIGAR operation", "positions over two tiles", "0, 1, 63, 64, 65 and 200 reads a sample")
    quality = bc.case("quality bytes and groups", [bc.sample([bc.R(1010, "8M", seq="ACGTNCGT", qual=[0, 126, 127, 128, 129, 254, 255, 40])]) for _ in range(9)],
                      bc.span(1008, 1022))
    for c in [x for x in CATALOGUE if x["name"] in names] + [quality]:
        bam, off, end, eof, rid, pos = arrays(c)
        n, P = len(rid), len(pos)
        labels = labels_of(c, n_groups, n_groups)
        rc, rec, rs, _, _ = ctx.bam_pileup(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], np.frombuffer(c["refseq"].encode(), dtype=np.uint8))
        assert rc == 0
        offsets, bases, quals, samples = entries_of_records(rec, rs, P)
        assert len(bases) > 0
        slots = cm.slots_of(n_groups)
        want = np.zeros((P, slots, 512) if n_groups else (P, 512), dtype=np.uint32)
        if n_groups:
            ctx.counts_add_csr_group_labels(offsets, bases, quals, labels[samples], n_groups, want)
        else:
            ctx.counts_add_csr(offsets, bases, quals, want)
        counts, tally = np.zeros(P * slots * 512, dtype=np.uint32), np.zeros(P, dtype=cm.TALLY)
        rc, _ = ctx.bam_counts(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"]), counts, tally,
                               group_of_sample=labels, n_groups=n_groups)
        assert rc == 0 and (counts == want.reshape(-1)).all(), c["name"]
        # and the tallies say what the records hold: the entries of base 0..3 (whatever their quality), of class 4, and the indel entries
        assert int(tally["strand_base"].sum()) == int((bases >= 0).sum() - (bases > 3).sum()) and int(tally["n_other"].sum()) == int((bases > 3).sum()), c["name"]
    bc._EXPECTED.pop(quality["name"], None)


# ---- 4. the accumulator -----------------------------------------------------------------------------------------------------------------
def bgzf_args(c, refseq_len=None):
    from tests.test_gpu_store import bgzf_of
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    comp, tab = bgzf_of(bam)
    return (comp, tab, len(bam), off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], c["positions"], c["rg_s"], len(c["refseq"]) if refseq_len is None else refseq_len)


def test_the_catalogue_through_the_bgzf_form_and_failures_add_nothing(ctx):
    from basevarc_amd import SiteAcc
    from basevarc_amd.lib import BvcError
    seen = set()
    for i, c in enumerate(CATALOGUE):
        n_groups = (0, 4)[i % 2]
        labels = labels_of(c, n_groups, i)
        exp = model_of(c, n_groups, labels)
        P = len(c["positions"])
        with SiteAcc(0, P, n_groups) as acc:
            assert acc.bytes() == (P * (cm.slots_of(n_groups) * 2048 + 48), 0)
            rcs = []
            for _ in range(2):                                   # twice: the second call adds the same again, or nothing again
                try:
                    rc, st = ctx.bam_counts_bgzf_acc(*bgzf_args(c), acc, group_of_sample=labels)
                    assert list(st[:len(c["samples"])]) == exp["status"], c["name"]
                except BvcError as e:
                    rc = e.status
                rcs.append(rc)
            assert rcs == [exp["rc"]] * 2, (c["name"], rcs)
            counts, tally = acc.get(ctx)
            if exp["rc"] == 0:
                assert (counts.reshape(exp["counts"].shape) == 2 * exp["counts"]).all(), c["name"]
                assert (tally.view(np.uint32) == 2 * exp["tally"].view(np.uint32)).all(), c["name"]
            else:
                assert not counts.any() and not tally.view(np.uint32).any(), c["name"]
            seen.add(exp["rc"])
    assert seen == {0, bm.BAM_MORE, ERR_DATA}


def test_four_threads_contexts_add_into_one_accumulator(ctx):
    from basevarc_amd import Context, SiteAcc
    P = 300
    base = span_case(P, 6)
    batches, seed = [], 40
    while len(batches) < 4:                                      # (random reads now and then leave the rule's range: batches that pass)
        rng = np.random.default_rng(seed)
        lo = base["positions"][0]
        samples = [bc.sample([bc.random_read(rng, int(p)) for p in np.sort(rng.integers(lo - 20, lo + P, 30))]) for _ in range(7 + len(batches))]
        c = bc.case(f"thread batch {seed}", samples, base["positions"], rg_s=1000, refseq="A" * 80000)
        if bc.expected(c)["rc"] == 0:
            batches.append(c)
        else:
            bc._EXPECTED.pop(c["name"], None)
        seed += 1
    n_groups = 3
    labels = [labels_of(c, n_groups, k) for k, c in enumerate(batches)]
    want_c = np.zeros((P, n_groups + 1, 512), dtype=np.uint32)
    want_t = np.zeros(P * TW, dtype=np.uint32)
    for c, g in zip(batches, labels):
        exp = model_of(c, n_groups, g)
        assert exp["rc"] == 0
        want_c += exp["counts"]
        want_t += exp["tally"].view(np.uint32)
        bc._EXPECTED.pop(c["name"], None)
    assert want_c.sum() > 2000 and want_c.max() > 1
    errors = []
    with SiteAcc(0, P, n_groups) as acc:
        def work(k):
            try:
                with Context(0) as c2:
                    for _ in range(3):                           # (three times each: twelve adds in flight between them)
                        rc, _ = c2.bam_counts_bgzf_acc(*bgzf_args(batches[k]), acc, group_of_sample=labels[k])
                        assert rc == 0
            except Exception as e:                               # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        counts, tally = acc.get(ctx)
        assert (counts == 3 * want_c).all() and (tally.view(np.uint32) == 3 * want_t).all()
        # rows from the middle, the tallies alone
        none, some = acc.get(ctx, 17, 40, counts=False)
        assert none is None and some.tobytes() == tally[17:57].tobytes()


@pytest.fixture(scope="module")
def bams100():
    """The 100 test BAMs' compressed bytes and block table, every 13th position of the region, and the model's entries for them."""
    import os
    from basevarc_amd import lib as bl
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    from tests.test_gpu_bam_pileup import bgzf_blocks_of
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    pv = pv[::13]
    data = bam_data_bytes()
    comp, table, off, end = bytearray(), [], [], []
    files = [l.strip().replace("data/", "", 1) for l in open(os.path.join(hostref.DATA, "bam.list")) if l.strip()]
    out_at = 0
    for f, (d, first, _) in zip(files, data):
        raw = open(os.path.join(hostref.DATA, f), "rb").read()
        off.append(out_at + first)
        for co, cl, isz, crc in bgzf_blocks_of(raw):
            table.append((len(comp) + co, out_at, cl, isz, crc, 1))
            out_at += isz
        end.append(out_at)
        comp += raw
    rid = [refs.index(contig) for _, _, refs in data]
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    assert exp["rc"] == 0
    ref_base = np.array(["ACGT".index(refseq[p - rg_s]) for p in pv], dtype=np.int8)
    return dict(comp=np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8), tab=np.array(table, dtype=bl.BLOCK_DTYPE), bam_bytes=out_at, off=off, end=end,
                eof=np.ones(len(data), dtype=np.uint8), rid=rid, beg0=beg0, end0=end0, mapq=mapq, pv=pv, rg_s=rg_s, refseq=refseq, exp=exp, ref_base=ref_base)


def acc_args(b, comp=None, end=None, eof=None):
    return (b["comp"] if comp is None else comp, b["tab"], b["bam_bytes"], b["off"], b["end"] if end is None else end, b["eof"] if eof is None else eof, b["rid"],
            b["beg0"], b["end0"], b["mapq"], b["pv"], b["rg_s"], len(b["refseq"]))


def test_the_test_bams_through_the_bgzf_form_and_a_damaged_block_adds_nothing(ctx, bams100):
    from basevarc_amd import SiteAcc
    from basevarc_amd.lib import BvcError
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    n_groups = 5
    labels = (np.arange(n) % 7).astype(np.uint8)
    want_c, want_t = cm.fold(b["exp"]["maps"], b["pv"], labels, n_groups)
    assert want_c.sum() > 30000 and want_t["n_indel"].sum() > 0
    with SiteAcc(0, P, n_groups) as acc:
        rc, st = ctx.bam_counts_bgzf_acc(*acc_args(b), acc, group_of_sample=labels)
        assert rc == 0 and list(st[:n]) == b["exp"]["status"]
        counts, tally = acc.get(ctx)
        assert (counts == want_c).all() and tally.tobytes() == want_t.tobytes()
        # one payload byte of a block in the middle flipped (it fails to inflate or fails its CRC32); a sample cut short without its end of
        # file: the codes of the plain call, and not a word changes
        k = len(b["tab"]) // 2
        bad = b["comp"].copy()
        bad[int(b["tab"][k]["comp_off"]) + int(b["tab"][k]["comp_len"]) // 2] ^= 0x5A
        with pytest.raises(BvcError, match="BGZF block") as e:
            ctx.bam_counts_bgzf_acc(*acc_args(b, comp=bad), acc, group_of_sample=labels)
        assert e.value.status == ERR_DATA
        short_end, short_eof = list(b["end"]), b["eof"].copy()
        short_end[3], short_eof[3] = b["off"][3] + 5000, 0
        rc, st = ctx.bam_counts_bgzf_acc(*acc_args(b, end=short_end, eof=short_eof), acc, group_of_sample=labels)
        assert rc == bm.BAM_MORE and st[3] == 2
        again, tally2 = acc.get(ctx)
        assert (again == want_c).all() and tally2.tobytes() == want_t.tobytes()


def test_the_refusals_leave_the_accumulator_and_the_context_usable(ctx):
    import ctypes as C
    from basevarc_amd import SiteAcc
    from basevarc_amd.lib import BvcError
    c = next(x for x in CATALOGUE if x["name"] == "2 samples")
    P = len(c["positions"])
    exp = model_of(c)

    def refused(code, match, fn):
        with pytest.raises(BvcError, match=match) as e:
            fn()
        assert e.value.status == code
    with SiteAcc(0, P) as acc, SiteAcc(0, P + 1) as other, SiteAcc(0, P, 2) as grouped:
        a = bgzf_args(c)
        refused(ERR_ARG, "n_positions is not the accumulator's", lambda: ctx.bam_counts_bgzf_acc(*a, other))
        refused(ERR_ARG, "null group_of_sample", lambda: ctx.bam_counts_bgzf_acc(*a, grouped))
        refused(ERR_ARG, "strictly ascending", lambda: ctx.bam_counts_bgzf_acc(*a[:10], c["positions"][::-1], *a[11:], acc))
        refused(ERR_ARG, "one behind the other", lambda: ctx.bam_counts_bgzf_acc(*a[:3], a[3][::-1], a[4][::-1], *a[5:], acc))
        refused(ERR_ARG, "outside the accumulator", lambda: acc.get(ctx, 1, P))
        refused(ERR_ARG, "outside the accumulator", lambda: acc.get(ctx, -1, 1))
        refused(ERR_ARG, "outside the accumulator", lambda: acc.lrt(ctx, np.zeros(P + 1, dtype=np.int8), MIN_AF))
        assert ctx._L.bvc_site_acc_lrt(ctx._h, grouped._h, 0, 1, C.c_void_p(np.zeros(1, dtype=np.int8).ctypes.data), MIN_AF,
                                       C.c_void_p(np.zeros(200, dtype=np.uint8).ctypes.data), None) == ERR_ARG      # groups, no group records
        # the context of another device, where the machine has one
        if ctx._L.bvc_device_count() > 1:
            from basevarc_amd import Context
            with Context(1) as far:
                refused(ERR_ARG, "another device", lambda: far.bam_counts_bgzf_acc(*a, acc))
                refused(ERR_ARG, "another device", lambda: acc.get(far))
        # the plain call's own
        bam, off, end, eof, rid, pos = arrays(c)
        counts, tally = np.zeros(P * 512, dtype=np.uint32), np.zeros(P, dtype=cm.TALLY)
        call = lambda **kw: ctx.bam_counts(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"]), counts, tally, **kw)
        refused(ERR_ARG, "n_groups must be 0..32", lambda: call(n_groups=33, group_of_sample=np.zeros(2, dtype=np.uint8)))
        refused(ERR_ARG, "n_groups must be 0..32", lambda: call(n_groups=-1))
        refused(ERR_ARG, "null group_of_sample", lambda: call(n_groups=2))
        p = lambda x: C.c_void_p(x.ctypes.data)
        st = np.zeros(2, dtype=np.uint32)
        good = [ctx._h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), c["beg0"], c["end0"], c["min_mapq"], P, p(pos), c["rg_s"], len(c["refseq"]), None, 0,
                p(counts), p(tally.view(np.uint32)), p(st), 0]
        for i in (2, 4, 5, 6, 7, 12, 17, 18, 19):                   # each pointer null with work present
            bad = list(good)
            bad[i] = None
            assert ctx._L.bvc_bam_counts(*bad) == ERR_ARG, i
        for i in (1, 3, 11, 14):                                     # each size negative
            bad = list(good)
            bad[i] = -1
            assert ctx._L.bvc_bam_counts(*bad) == ERR_ARG, i
        assert not counts.any() and not tally.view(np.uint32).any()
        # a budget one byte short of the accumulator: refused, and one of exactly its size is made
        need = P * (2048 + 48)
        with pytest.raises(BvcError) as e:
            SiteAcc(0, P, 0, need - 1)
        assert e.value.status == ERR_ALLOC
        with SiteAcc(0, P, 0, need) as exact:
            assert exact.bytes() == (need, need)
        # everything still works
        rc, _ = ctx.bam_counts_bgzf_acc(*a, acc)
        assert rc == 0 and (acc.get(ctx)[0] == exp["counts"].reshape(P, 512)).all()
        assert ctx._L.bvc_bam_counts(*good) == 0 and (counts == exp["counts"].reshape(-1)).all()


@pytest.mark.parametrize("n_groups", [0, 5])
def test_the_accumulators_stage_two_is_the_librarys_on_the_fetched_counts(ctx, bams100, n_groups):
    """bvc_site_acc_lrt on rows where they lie: byte for byte bvc_lrt_hist / bvc_lrt_hist_groups on what bvc_site_acc_get delivers, for all
    rows and for a window of them; and its called flags are the bin path's on bvc_bam_pileup_bgzf's records of the same batch."""
    from basevarc_amd import SiteAcc
    b = bams100
    P, n = len(b["pv"]), len(b["rid"])
    labels = (np.arange(n) % 7).astype(np.uint8) if n_groups else None
    with SiteAcc(0, P, n_groups) as acc:
        rc, _ = ctx.bam_counts_bgzf_acc(*acc_args(b), acc, group_of_sample=labels)
        assert rc == 0
        counts, _ = acc.get(ctx)
        for t0, T in ((0, P), (1234, 777), (P - 1, 1)):
            ref = b["ref_base"][t0:t0 + T]
            if n_groups:
                res, gres = acc.lrt(ctx, ref, MIN_AF, t0)
                want, gwant = ctx.lrt_hist_groups(counts[t0:t0 + T], ref, MIN_AF, n_groups)
                assert gres.tobytes() == gwant.tobytes(), (t0, T)
            else:
                res = acc.lrt(ctx, ref, MIN_AF, t0)
                want = ctx.lrt_hist(counts[t0:t0 + T], ref, MIN_AF)
            assert res.tobytes() == want.tobytes(), (t0, T)
            if T == P:
                everything = res
    assert 0 < int((everything["called"] != 0).sum()) < P // 10
    rc, rec, rs, _, _ = ctx.bam_pileup_bgzf(b["comp"], b["tab"], b["bam_bytes"], b["off"], b["end"], b["eof"], b["rid"], b["beg0"], b["end0"], b["mapq"], b["pv"],
                                            b["rg_s"], np.frombuffer(b["refseq"].encode(), dtype=np.uint8))
    assert rc == 0
    tile = ctx.pileup_tile_bin(rec.tobytes(), rs[None, :P + 1], [0], [n], b["ref_base"], MIN_AF, group_of_sample=labels, n_groups=n_groups)
    assert (tile["results"]["called"] == everything["called"]).all()


def test_a_second_call_of_the_same_shape_allocates_nothing(ctx, bams100):
    import torch
    from basevarc_amd import SiteAcc
    b = bams100
    P = len(b["pv"])
    c = next(x for x in CATALOGUE if x["name"] == "300 samples")
    bam, off, end, eof, rid, pos = arrays(c)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    d_args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], len(c["refseq"])]
    d_counts = torch.zeros(len(pos) * 512, dtype=torch.int32, device="cuda")
    d_tally = torch.zeros(len(pos) * TW, dtype=torch.int32, device="cuda")
    d_status = torch.zeros(len(rid), dtype=torch.int32, device="cuda")
    counts, tally = np.zeros(len(pos) * 512, dtype=np.uint32), np.zeros(len(pos), dtype=cm.TALLY)
    with SiteAcc(0, P) as acc:
        free = []
        torch.cuda.mem_get_info()
        for _ in range(2):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), acc)[0] == 0
            acc.lrt(ctx, b["ref_base"], MIN_AF)
            acc.get(ctx)
            assert ctx.bam_counts(*d_args, d_counts, d_tally, sample_status=d_status)[0] == 0
            assert ctx.bam_counts(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], len(c["refseq"]), counts, tally)[0] == 0
            ctx.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
        # the library allocates device memory of its own (not torch's pool): what is free on the device after the first round stays free
        assert free[1] == free[0], free
    want = model_of(c)
    assert (d_counts.cpu().numpy().view(np.uint32) == 2 * want["counts"].reshape(-1)).all() and (counts == 2 * want["counts"].reshape(-1)).all()
