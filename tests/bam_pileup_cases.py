"""Hand-built catalogue for bvc_bam_pileup: the smallest inputs at which each path of the filter, the per-position rule, the entry
encoding and the transposition can go wrong (tests/bam_pileup_model.py writes the bytes and says what must come out), and the seeded
random cases of the differential run.  Plain Python, no device."""
import struct

import numpy as np

from tests import bam_pileup_model as bm

RG_S = 1000
REFSEQ = "".join("ACGT"[(i * 7 + i // 5) % 4] for i in range(1400))
TILE = 1024                  # positions per tile of the kernels (csrc/bvc_internal.h, bam_pileup_tile): a call of more takes the loop again
WIDE = 4100                  # samples from which on the tile shrinks (4 Mi cells): 960 positions at this width


def R(pos, cigar, **kw):
    return bm.make_read(pos, cigar, **kw)


def sample(reads, eof=True, rid=0, tail=b""):
    """(bytes, eof, rid) of a sample holding these reads (dicts, or bytes taken as they are) and `tail` behind them."""
    return (b"".join(r if isinstance(r, bytes) else bm.pack_record(r) for r in reads) + tail, eof, rid)


def case(name, samples, positions, beg0=0, end0=1 << 30, min_mapq=20, rg_s=RG_S, refseq=REFSEQ, lead=0):
    return dict(name=name, samples=samples, positions=[int(p) for p in positions], beg0=beg0, end0=end0, min_mapq=min_mapq, rg_s=rg_s,
                refseq=refseq, lead=lead)


def span(lo, hi, step=1):
    return list(range(lo, hi, step))


STOP_BY_REF = bm.pack_record(R(5, "10M", ref_id=1))
STOP_BY_POS = bm.pack_record(R(5000, "10M"))
GARBAGE = bytes((i * 37 + 11) & 0xFF for i in range(97))


def catalogue():
    c = []
    every_op = "2H3S5M2I4M3D5M2N3M1P2M4=3X2S1H"
    c.append(case("one sample, one read", [sample([R(1010, "10M")])], span(1005, 1030)))
    c.append(case("every CIGAR operation", [sample([R(1010, every_op)])], span(1000, 1060)))
    c.append(case("the last base in front of I, D, P and zero-length I / D",
                  [sample([R(1010, cg)]) for cg in ("5M2I5M", "5M2D5M", "5M1P5M", "5M0I5M", "5M0D5M", "5M1P2I5M")], span(1008, 1030)))
    c.append(case("D and N at the position, the next read covering it or not",
                  [sample([R(1010, "5M5D5M", mapq=31), R(1012, "20M", mapq=32)]), sample([R(1010, "5M5N5M", mapq=33), R(1040, "3M", mapq=34)]),
                   sample([R(1010, "5M5D5M", mapq=35)]), sample([R(1010, "5M5N5M"), R(1018, "9M", mapq=36)])], span(1005, 1050)))
    c.append(case("a fall-through chain over three reads",
                  [sample([R(1010, "5M10D5M", mapq=41), R(1013, "2M10D5M", mapq=42), R(1014, "30M", mapq=43)]),
                   sample([R(1010, "5M10D5M", mapq=41), R(1013, "2M10N5M", mapq=42), R(1014, "3M12D4M", mapq=43)])], span(1008, 1050)))
    c.append(case("a short read inside a long one, first sticking at the last read",
                  [sample([R(1010, "50M", mapq=50), R(1020, "5M", mapq=51), R(1070, "10M", mapq=52)])], span(1005, 1100)))
    c.append(case("soft clips at either end, = beside M and X", [sample([R(1010, "3S10M4S")]), sample([R(1010, "3M4=3X2I3M2D4=")]),
                                                                  sample([R(1010, "4S3=2I3X5S")])], span(1005, 1040)))
    c.append(case("an empty sequence", [sample([R(1010, "10M", seq="", qual=[])]), sample([R(1010, "10M")])], span(1005, 1025)))
    c.append(case("an insertion that starts past the sequence", [sample([R(1010, "5M3I5M", seq="ACG", qual=[30, 30, 30])])], [1015]))
    c.append(case("a query offset past the sequence", [sample([R(1010, "10M", seq="ACGTA", qual=[30] * 5)])], [1012, 1016]))
    c.append(case("an indel entry first, and one behind another read's base entry",
                  [sample([R(1010, "5M2I5M", mapq=44)]), sample([R(1000, "8M", mapq=33), R(1010, "5M2D5M", mapq=44)])], [1004, 1015, 1016]))
    c.append(case("a deletion longer than what is left of the reference", [sample([R(1010, "5M50D5M")]), sample([R(1024, "5M3D5M")])],
                  span(1010, 1032), refseq=REFSEQ[:30]))
    c.append(case("a deletion that starts past the reference", [sample([R(1040, "5M3D5M")])], [1045], refseq=REFSEQ[:30]))
    good = R(1010, "10M", mapq=25)
    c.append(case("each filtered kind of read", [
        sample([R(1008, "10M", flag=4), good]), sample([bm.pack_record(R(1008, "10M"), n_cigar=0), good]), sample([R(900, "20M"), good]),
        sample([R(1008, "10M", flag=0x400), good]), sample([R(1008, "10M", mapq=19), good]), sample([R(1008, "10M", ref_id=0), good], rid=1),
        sample([R(1008, "10M", ref_id=-1), R(1009, "10M", ref_id=0)], rid=1), sample([R(1008, "10M", flag=4)]),
        sample([R(1010, "10M", ref_id=0)], rid=-1)], span(1000, 1030), beg0=950, min_mapq=20))
    for eof in (False, True):
        c.append(case(f"a stop by ref_id and a stop by pos, garbage behind them, eof {int(eof)}",
                      [sample([R(1010, "10M"), STOP_BY_REF], eof=eof, tail=GARBAGE), sample([R(1010, "10M"), STOP_BY_POS], eof=eof, tail=GARBAGE),
                       sample([STOP_BY_POS], eof=eof, tail=GARBAGE[:3]), sample([R(1010, "10M"), R(1015, "10M")], eof=eof, tail=STOP_BY_POS[:-1] + b"\0")],
                      span(1005, 1030), end0=2000))
    rec = bm.pack_record(good)
    c.append(case("block_size 31 and its kin", [
        sample([good, struct.pack("<i", 31) + rec[4:]]), sample([good, struct.pack("<i", -5) + rec[4:]]),
        sample([good, struct.pack("<i", (1 << 28) + 1) + rec[4:]]), sample([good])], span(1005, 1025)))
    c.append(case("fields that overrun their block", [
        sample([good, bm.pack_record(good, l_seq=1000)]), sample([good, bm.pack_record(good, n_cigar=60000)]),
        sample([good, bm.pack_record(good, l_read_name=255)]), sample([good, bm.pack_record(good, l_seq=-1)]),
        sample([bm.pack_record(good, l_seq=1000), STOP_BY_POS]), sample([STOP_BY_POS, bm.pack_record(good, l_seq=1000)])], span(1005, 1025), end0=2000))
    last = bm.pack_record(R(1012, "4M1I3M"))
    for eof in (False, True):
        c.append(case(f"the last record cut at every byte, eof {int(eof)}", [sample([good], eof=eof, tail=last[:k]) for k in range(len(last) + 1)],
                      span(1005, 1025)))
    many = lambda n, at=1010: [R(at + 2 * i, "6M1D3M" if i % 5 == 0 else "7M", mapq=20 + i % 40) for i in range(n)]
    c.append(case("0, 1, 63, 64, 65 and 200 reads a sample", [sample(many(n)) for n in (0, 1, 63, 64, 65, 200)], span(1000, 1300, 1) + span(1300, 1420, 3)))
    for n in (0, 1, 63, 64, 65):
        c.append(case(f"{n} listed positions", [sample(many(40)), sample([R(1010, "200M")])], span(1012, 1012 + n)))
    c.append(case("a read over more than 64 listed positions, a position list with gaps",
                  [sample([R(1010, "200M")]), sample([R(1010, "90M2I90M"), R(1100, "150M")])], span(1000, 1120, 1) + span(1120, 1300, 3)))
    for n in (1, 2, 64, 65, 300):
        c.append(case(f"{n} samples", [sample([R(1010 + (s * 3) % 50, "4M1I4M2D6M" if s % 4 == 0 else "12M", mapq=20 + s % 41)] +
                                              ([R(1030 + s % 7, "9M", mapq=21 + s % 30)] if s % 3 == 0 else [])) for s in range(n)], span(1005, 1080)))
    c.append(case("samples with no bytes at all, sample_off at odd addresses",
                  [sample([]), sample([R(1010, "9M")]), sample([]), sample([R(1011, "3M2I4M")]), sample([])], span(1005, 1030), lead=1))
    c.append(case("samples with no bytes and no end of file", [sample([], eof=False), sample([R(1010, "9M")])], span(1005, 1030), lead=3))
    c.append(case("no samples", [], span(1005, 1010)))
    c.append(case("no samples and no positions", [], []))
    # more positions than a tile: the indel entry behind the boundary shows the mapq of the base entry in front of it
    c.append(case("positions over two tiles", [sample([R(1100, "200M", mapq=37), R(1000 + TILE + 80, "5M2I5M", mapq=38)]),
                                               sample([R(1000 + TILE - 10, "12M3D12M", mapq=39)]), sample(many(100, at=1900))],
                  span(1090, 1090 + TILE + 130), refseq=REFSEQ * 2))
    c.append(case("a batch so wide that the tile shrinks", [sample([R(1010 + (s * 13) % 900, "5M1I4M" if s % 9 == 0 else "8M", mapq=20 + s % 40)])
                                                            for s in range(WIDE)], span(1005, 1005 + 965)))
    return c


# ---- the seeded random cases ------------------------------------------------------------------------------------------------------
def random_read(rng, pos):
    """tests/test_host.py's _random_read with rich CIGARs."""
    ops = []
    if rng.random() < 0.2:
        ops.append(("H", int(rng.integers(1, 6))))
    if rng.random() < 0.4:
        ops.append(("S", int(rng.integers(1, 9))))
    ops.append((str(rng.choice(list("M=X"))), int(rng.integers(1, 30))))
    for _ in range(int(rng.integers(0, 6))):
        op = str(rng.choice(list("MIDNP=X")))
        if op == ops[-1][0]:
            continue
        ops.append((op, int(rng.integers(1, 12 if op in "MX=" else 5))))
    if ops[-1][0] not in "M=X":
        ops.append(("M", int(rng.integers(1, 20))))
    if rng.random() < 0.3:
        ops.append(("S", int(rng.integers(1, 9))))
    if rng.random() < 0.15:
        ops.append(("H", int(rng.integers(1, 6))))
    qlen = bm.query_length(ops)
    seq = "".join(rng.choice(list("ACGTN"), qlen, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    qual = [int(x) for x in rng.integers(2, 42, qlen)]
    flag = int(rng.choice([0, 16, 32, 99, 147, 163, 4, 0x400 | 99]))
    return bm.make_read(pos, ops, flag=flag, mapq=int(rng.integers(10, 61)), seq=seq, qual=qual)


RANDOM_SEEDS = tuple(range(20261019, 20261019 + 40))


def random_case(seed):
    """1-12 samples of random reads; every fifth case spoils one sample (cut short, a malformed record, or a sequence too short)."""
    rng = np.random.default_rng(seed)
    rg_s = int(rng.integers(1000, 1100))
    n_span = int(rng.integers(50, 400))
    refseq = "".join(rng.choice(list("ACGT"), n_span + 1200))
    samples = []
    n_samples = int(rng.integers(1, 13))
    spoil = int(rng.integers(0, n_samples)) if seed % 5 == 0 else -1
    for s in range(n_samples):
        n_reads = int(rng.integers(0, 25))
        starts = np.sort(rng.integers(rg_s - 30, rg_s + n_span, n_reads))
        reads = [random_read(rng, int(p)) for p in starts]
        eof = bool(rng.random() < 0.5)
        tail = b"" if eof else STOP_BY_REF + GARBAGE[:int(rng.integers(0, 40))]
        data = sample(reads, eof=eof, tail=tail)
        if s == spoil:
            kind = (seed // 5) % 3
            if kind == 0:
                data = (data[0][:max(1, len(data[0]) - len(tail) - 7)], False, 0)
            elif kind == 1:
                data = (bm.pack_record(random_read(rng, rg_s), l_seq=5000) + data[0], eof, 0)
            else:
                r = bm.make_read(rg_s + 5, "30M", seq="ACGT", qual=[30] * 4, mapq=60)
                data = sample([r], eof=True)
        samples.append(data)
    positions = [p for p in range(rg_s, rg_s + n_span) if rng.random() < 0.9]
    return case(f"seed {seed}", samples, positions, beg0=max(0, rg_s - 1 - 20), end0=rg_s + n_span + 20, min_mapq=20, rg_s=rg_s, refseq=refseq,
                lead=int(rng.integers(0, 4)))


def reads_text(rv):
    """The kept reads of a sample in the line form bvchost_pileup_tokens reads."""
    return "".join(f"{r['pos']} {r['flag']} {r['mapq']} " + "".join(f"{l}{o}" for o, l in r["cigar"]) + f" {r['seq']} " +
                   ",".join(str(int(q)) for q in r["qual"]) + "\n" for r in rv)


_EXPECTED = {}


def expected(c):
    """The model's result for a case, computed once."""
    if c["name"] not in _EXPECTED:
        _EXPECTED[c["name"]] = bm.expected(c["samples"], c["beg0"], c["end0"], c["min_mapq"], c["positions"], c["rg_s"], c["refseq"])
    return _EXPECTED[c["name"]]
