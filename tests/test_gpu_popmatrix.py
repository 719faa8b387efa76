"""bvc_bam_popmatrix on the device (bam_popmatrix_kernel.hip; GPU) against the plain Python model (tests/popmatrix_model.py, which
tests/test_popmatrix_model.py and tests/test_popmatrix_host.py hold to the reference's rule and to the CPU path): every byte of the
matrix, every status and every return code -- the hand-built catalogue of bvc_bam_pileup, the REF / ALT characters, the smallest shapes
at which the kernel can go wrong, a row stride with guard bytes, host and device pointers, the refusals, 200 seeded random cases and the
100 test BAMs from their BGZF blocks."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import popmatrix_model as pm

pytestmark = pytest.mark.gpu

GUARD = 64
CATALOGUE = bc.catalogue()
_EXPECTED = {}


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def lines_of(c):
    """The case's positions as position-file lines (its own "pv" where it has one)."""
    return c["pv"] if "pv" in c else pm.refalt(c["positions"], c["rg_s"], c["refseq"])


def expected(c):
    if c["name"] not in _EXPECTED:
        _EXPECTED[c["name"]] = pm.expected(c["samples"], c["beg0"], c["end0"], c["min_mapq"], lines_of(c), c["rg_s"], len(c["refseq"]))
    return _EXPECTED[c["name"]]


def run(ctx, c, device, pad=0):
    """One call with guard bytes in front of and behind the matrix and `pad` bytes between the rows: (rc or the BvcError's status,
    the whole matrix buffer, the status buffer, row_stride)."""
    from basevarc_amd.lib import BvcError
    pv = lines_of(c)
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    n, P = len(rid), len(pv)
    stride = P + pad
    arrs = [np.frombuffer(bam, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(end, dtype=np.int64), np.array(eof, dtype=np.uint8),
            np.array(rid, dtype=np.int32)]
    pos = np.array([p for p, _, _ in pv], dtype=np.int32)
    ref = np.array([ord(r) for _, r, _ in pv], dtype=np.uint8)
    alt = np.array([ord(a) for _, _, a in pv], dtype=np.uint8)
    buf = np.full(GUARD + n * stride + GUARD, 0xCD, dtype=np.uint8)
    status = np.full(n + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        arrs, pos, ref, alt, d_buf, d_status = [dev(a) for a in arrs], dev(pos), dev(ref), dev(alt), dev(buf), dev(status)
        out = (d_buf[GUARD:], d_status)
    else:
        out = (buf[GUARD:], status)
    try:
        rc, _, _ = ctx.bam_popmatrix(*arrs, c["beg0"], c["end0"], c["min_mapq"], pos, ref, alt, c["rg_s"], len(c["refseq"]), matrix=out[0],
                                     row_stride=stride, sample_status=out[1])
    except BvcError as e:
        rc = e.status
    if device:
        ctx.synchronize()
        buf, status = d_buf.cpu().numpy(), d_status.cpu().numpy().view(np.uint32)
    return rc, buf, status, stride


def check(c, got):
    """What a call left, against the model: the return code, every status, every byte of the rows the header defines, and nothing
    written in front of the matrix, behind it or between a row's end and the next row."""
    exp = expected(c)
    rc, buf, status, stride = got
    n, P = len(c["samples"]), len(lines_of(c))
    assert rc == exp["rc"], (c["name"], rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], list(status[:n]), exp["status"])
    assert (status[n:] == 0xCDCDCDCD).all(), c["name"]
    assert (buf[:GUARD] == 0xCD).all() and (buf[GUARD + n * stride:] == 0xCD).all(), c["name"]
    rows = buf[GUARD:GUARD + n * stride].reshape(n, stride) if n and stride else np.zeros((n, 0), dtype=np.uint8)
    assert (rows[:, P:] == 0xCD).all(), c["name"]
    for s, want in enumerate(exp["rows"]):
        if want is not None:
            assert rows[s, :P].tobytes().decode("latin1") == want, (c["name"], s)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_catalogue_case(ctx, c, device):
    check(c, run(ctx, c, device, pad=0 if len(c["samples"]) > 1000 else 7))


def test_the_catalogue_holds_every_status_character_and_return_code():
    seen, chars, rcs = set(), set(), set()
    for c in CATALOGUE:
        e = expected(c)
        seen.update(e["status"])
        rcs.add(e["rc"])
        chars.update(ch for r in e["rows"] if r for ch in r)
    assert seen == {0, 1, 2, 3, 4} and rcs == {pm.OK, pm.BAM_MORE, pm.ERR_DATA} and chars == set("01."), (seen, rcs, chars)


# ---- the characters -------------------------------------------------------------------------------------------------------------------
def character_cases():
    seq = "ACGTN" * 4
    reads = [bm.make_read(1009, "20M", seq=seq), bm.make_read(1019, "10M", seq="ACGTNACGTN")]
    span = list(range(1008, 1032))
    out = []
    letters = "ACGTN="
    out.append(bc.case("REF and ALT from ACGTN=", [bc.sample(reads)], span))
    out[-1]["pv"] = [(p, letters[(p + k) % 6], letters[(p + 2 * k + 1) % 6]) for p in span for k in range(3)]       # every position on three lines
    out.append(bc.case("lowercase REF and ALT", [bc.sample(reads)], span))
    out[-1]["pv"] = [(p, "acgtn"[p % 5], "ACGTN"[p % 5]) for p in span]                  # the first read's base at p is "ACGTN"[p % 5]
    out.append(bc.case("REF equal to ALT", [bc.sample(reads)], span))
    out[-1]["pv"] = [(p, "ACGTN"[(p + k) % 5], "ACGTN"[(p + k) % 5]) for p in span for k in range(2)]
    # a read's bases outside ACGTN keep their own characters: M R W ... against themselves
    amb = "=ACMGRSVTWYHKDBN"
    out.append(bc.case("every base code against its own character", [bc.sample([bm.make_read(1009, "16M", seq=amb)])], list(range(1010, 1026))))
    out[-1]["pv"] = [(1010 + i, amb[i], "A") for i in range(16)] + [(1025, "n", "N")]
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_ref_and_alt_characters(ctx, device):
    cases = character_cases()
    for c in cases:
        check(c, run(ctx, c, device, pad=3))
    assert expected(cases[3])["rows"][0] == "0" * 16 + "1"
    assert set(expected(cases[1])["rows"][0]) == {"1", "."} and "0" in expected(cases[2])["rows"][0] and "1" not in expected(cases[2])["rows"][0]


# ---- the smallest shapes ---------------------------------------------------------------------------------------------------------------
def shape_cases():
    many = lambda n, at=1010: [bc.R(at + 2 * i, "6M1D3M" if i % 5 == 0 else "7M", mapq=20 + i % 40) for i in range(n)]
    out = []
    for ns in (1, 3, 4, 5):                          # either side of the four wavefronts of a workgroup
        for P in (0, 1, 63, 64, 65, 129):            # either side of a wavefront's 64 lanes, and a third step
            out.append(bc.case(f"{ns} samples, {P} positions", [bc.sample(many(30 + 7 * s, at=1010 + s)) for s in range(ns)], bc.span(1012, 1012 + P)))
    # 63 / 64 / 65 kept reads: the index kernel's chunk and the ends of the binary search (the first, the last read; behind the last)
    for n in (63, 64, 65):
        reads = many(n)
        pos = sorted({1005, reads[0]["pos"] + 1, bm.tp.end_pos(reads[0]), reads[-1]["pos"] + 1, bm.tp.end_pos(reads[-1]), bm.tp.end_pos(reads[-1]) + 1,
                      reads[62]["pos"] + 1, bm.tp.end_pos(reads[62]), 1010 + n, 1010 + 2 * n - 3})
        out.append(bc.case(f"{n} kept reads, positions at the reads' first and last bases", [bc.sample(reads)], pos))
    dup = bc.case("duplicate positions, three lines a site over two wavefront steps", [bc.sample(many(40)), bc.sample([bc.R(1010, "200M")])], bc.span(1012, 1060))
    dup["pv"] = [(p, r, "ACGT"[(i + k) % 4]) for i, (p, r, _) in enumerate(pm.refalt(dup["positions"], dup["rg_s"], dup["refseq"])) for k in range(3)]
    out.append(dup)
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_smallest_shapes(ctx, device):
    for c in shape_cases():
        check(c, run(ctx, c, device, pad=5))


def test_odd_addresses_of_bam_and_a_wide_stride(ctx):
    c = next(x for x in CATALOGUE if x["name"] == "every CIGAR operation")
    for lead in (1, 2, 3):
        d = dict(c, lead=lead, name=f"{c['name']}, lead {lead}")
        _EXPECTED[d["name"]] = expected(c)
        check(d, run(ctx, d, False, pad=1000))
        check(d, run(ctx, d, True, pad=1))


def test_statuses_alone_and_mixed_leave_the_guards_and_the_good_rows(ctx):
    """Each failing status alone in a batch, then all five in one: the rows of the samples with status 0 and 1 are the model's whatever
    the call returns."""
    good, rec = bc.R(1010, "10M", mapq=25), bm.pack_record(bc.R(1010, "10M", mapq=25))
    kinds = {1: bc.sample([bc.R(1008, "10M", flag=4)]), 2: bc.sample([good], eof=False), 3: bc.sample([good, bm.pack_record(good, l_seq=1000)]),
             4: bc.sample([bc.R(1010, "10M", seq="ACGTA", qual=[30] * 5)])}
    assert len(rec) > 36
    for st, smp in kinds.items():
        for mix in ([smp], [bc.sample([good]), smp, bc.sample([good])]):
            c = bc.case(f"status {st} in a batch of {len(mix)}", mix, bc.span(1005, 1030))
            assert st in expected(c)["status"]
            for device in (False, True):
                check(c, run(ctx, c, device, pad=9))
    c = bc.case("all five statuses", [bc.sample([good])] + [kinds[k] for k in (1, 2, 3, 4)] + [bc.sample([good])], bc.span(1005, 1030))
    assert expected(c)["status"] == [0, 1, 2, 3, 4, 0] and expected(c)["rc"] == pm.ERR_DATA
    for device in (False, True):
        check(c, run(ctx, c, device, pad=9))
    # the reference builds an indel's text before it looks at its length: a zero-length I / D whose text would start past its source
    # throws there (status 4), one whose text starts inside it is no token at all
    c = bc.case("zero-length I and D past their source", [bc.sample([bc.R(1010, "5M0I5M", seq="ACG", qual=[30] * 3)]), bc.sample([bc.R(1040, "5M0D5M")]),
                                                          bc.sample([bc.R(1010, "5M0I5M")]), bc.sample([bc.R(1020, "5M0D5M")])],
                [1012, 1015, 1025, 1045], refseq=bc.REFSEQ[:30])
    assert expected(c)["status"] == [4, 4, 0, 0]
    for device in (False, True):
        check(c, run(ctx, c, device, pad=9))
    c = bc.case("statuses 0, 1 and 2", [bc.sample([good]), kinds[1], kinds[2]], bc.span(1005, 1030))
    assert expected(c)["rc"] == pm.BAM_MORE
    for device in (False, True):
        check(c, run(ctx, c, device, pad=9))


def test_the_last_error_names_the_first_failing_sample(ctx):
    from basevarc_amd.lib import BvcError
    for name, msg in (("block_size 31 and its kin", "sample 0: truncated or corrupt BAM record"),
                      ("an empty sequence", "sample 0: index offset is out of range of the sequence")):
        c = next(x for x in CATALOGUE if x["name"] == name)
        bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
        pv = lines_of(c)
        with pytest.raises(BvcError, match=msg):
            ctx.bam_popmatrix(np.frombuffer(bam, dtype=np.uint8), off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], [p for p, _, _ in pv],
                              [ord(r) for _, r, _ in pv], [ord(a) for _, _, a in pv], c["rg_s"], len(c["refseq"]))


def test_the_refusals(ctx):
    c = next(x for x in CATALOGUE if x["name"] == "2 samples")
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    pv = lines_of(c)
    bam, off, end = np.frombuffer(bam, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(end, dtype=np.int64)
    eof, rid = np.array(eof, dtype=np.uint8), np.array(rid, dtype=np.int32)
    pos = np.array([p for p, _, _ in pv], dtype=np.int32)
    ref, alt = np.array([ord(r) for _, r, _ in pv], dtype=np.uint8), np.array([ord(a) for _, _, a in pv], dtype=np.uint8)
    P = len(pos)
    mat, st = np.full(2 * P + GUARD, 0xCD, dtype=np.uint8), np.zeros(2, dtype=np.uint32)
    L, h = ctx._L, ctx._h
    p = lambda a: C.c_void_p(a.ctypes.data)
    good = [h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), 0, 1 << 30, 20, P, p(pos), p(ref), p(alt), c["rg_s"], len(c["refseq"]), p(mat), P, p(st), 0]
    assert L.bvc_bam_popmatrix(*good) == pm.OK
    rows = mat[:2 * P].tobytes().decode("latin1")
    assert [rows[:P], rows[P:]] == expected(c)["rows"] and (mat[2 * P:] == 0xCD).all()
    for i in (2, 4, 5, 6, 7, 12, 13, 14, 17, 19):                     # each pointer null with work present
        bad = list(good)
        bad[i] = None
        assert L.bvc_bam_popmatrix(*bad) == pm.ERR_ARG, i
    for i in (1, 3, 11, 16):                                          # each size negative
        bad = list(good)
        bad[i] = -1
        assert L.bvc_bam_popmatrix(*bad) == pm.ERR_ARG, i
    for stride in (P - 1, 0, -1):                                     # rows that would overlap
        bad = list(good)
        bad[18] = stride
        assert L.bvc_bam_popmatrix(*bad) == pm.ERR_ARG, stride

    def with_arrays(**kw):
        a = dict(off=off, end=end, pos=pos)
        a.update(kw)
        bad = list(good)
        bad[4], bad[5], bad[12] = p(a["off"]), p(a["end"]), p(a["pos"])
        return L.bvc_bam_popmatrix(*bad)
    assert with_arrays(pos=pos[::-1].copy()) == pm.ERR_ARG             # descending positions
    assert with_arrays(pos=np.concatenate([pos[:5], pos[3:5], pos[5:]])[:P].copy()) == pm.ERR_ARG
    assert with_arrays(pos=np.repeat(pos[:(P + 1) // 2], 2)[:P].copy()) == pm.OK      # duplicates are legal
    assert with_arrays(off=off[::-1].copy(), end=end[::-1].copy()) == pm.ERR_ARG
    assert with_arrays(end=end + 1) == pm.ERR_ARG and with_arrays(off=off - 1) == pm.ERR_ARG and with_arrays(off=end, end=off) == pm.ERR_ARG
    assert (mat[2 * P:] == 0xCD).all()
    assert L.bvc_bam_popmatrix(*good) == pm.OK                         # the context stays usable


# ---- the seeded random cases ------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = tuple(range(20261019, 20261019 + 200))


def random_popmatrix_case(seed):
    """tests/bam_pileup_cases.random_case with position-file lines of its positions: some sites on two or three lines, REF / ALT from
    ACGTN with the reference's base twice as likely."""
    c = bc.random_case(seed)
    rng = np.random.default_rng(seed + 7)
    pv = []
    for p in c["positions"]:
        for _ in range(int(rng.choice([1, 1, 1, 1, 2, 3]))):
            at = c["refseq"][p - c["rg_s"]]
            ref, alt = (str(x) for x in rng.choice(list("ACGTN") + [at] * 5, 2))
            pv.append((p, ref, alt))
    return dict(c, name=f"popmatrix seed {seed}", pv=pv)


def test_the_seeded_random_cases(ctx):
    tot = {}
    for seed in RANDOM_SEEDS:
        c = random_popmatrix_case(seed)
        check(c, run(ctx, c, device=seed % 2 == 1, pad=seed % 5))
        e = expected(c)
        for s in e["status"]:
            tot[f"status{s}"] = tot.get(f"status{s}", 0) + 1
        tot[f"rc{e['rc']}"] = tot.get(f"rc{e['rc']}", 0) + 1
        for r in e["rows"]:
            for ch in r or "":
                tot[ch] = tot.get(ch, 0) + 1
        _EXPECTED.pop(c["name"])
    assert len(RANDOM_SEEDS) == 200 and all(tot.get(f"status{s}", 0) > 0 for s in range(5)) and all(tot.get(f"rc{r}", 0) > 0 for r in (0, 2, -5)), tot
    assert tot["0"] > 1000 and tot["1"] > 1000 and tot["."] > 1000, tot


# ---- the 100 test BAMs, from their BGZF blocks ----------------------------------------------------------------------------------------
def test_the_test_bams_from_their_blocks_and_a_damaged_block(ctx):
    from basevarc_amd import lib as bl
    from basevarc_amd.lib import BvcError
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    from tests.test_gpu_bam_pileup import bgzf_blocks_of
    contig, beg0, end0, mapq, positions, rg_s, refseq = bam_data_call()
    pv = pm.refalt(positions[::13], rg_s, refseq)
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
    tab = np.array(table, dtype=bl.BLOCK_DTYPE)
    rid = [refs.index(contig) for _, _, refs in data]
    exp = pm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, len(refseq))
    assert exp["rc"] == 0 and set("".join(exp["rows"])) == set("01.")
    args = (off, end, np.ones(len(data), dtype=np.uint8), rid, beg0, end0, mapq, [p for p, _, _ in pv], [ord(r) for _, r, _ in pv],
            [ord(a) for _, _, a in pv], rg_s, len(refseq))
    comp = np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8)
    rc, matrix, status = ctx.bam_popmatrix_bgzf(comp, tab, out_at, *args)
    assert rc == 0 and list(status) == exp["status"]
    assert [row.tobytes().decode("latin1") for row in matrix] == exp["rows"]
    # one payload byte of a block in the middle flipped: the block fails to inflate or fails its CRC32
    bad = comp.copy()
    k = len(tab) // 2
    bad[int(tab[k]["comp_off"]) + int(tab[k]["comp_len"]) // 2] ^= 0x5A
    with pytest.raises(BvcError, match=f"BGZF block {k}: ") as e:
        ctx.bam_popmatrix_bgzf(bad, tab, out_at, *args)
    assert e.value.status == pm.ERR_DATA
    rc, matrix, _ = ctx.bam_popmatrix_bgzf(comp, tab, out_at, *args)           # the context stays usable
    assert rc == 0 and [row.tobytes().decode("latin1") for row in matrix] == exp["rows"]
