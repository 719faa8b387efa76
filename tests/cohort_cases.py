"""Hand-built cohorts for the host program's file-level tests: BAM files, indexes and a three-contig reference generated from read dicts
(tests/bam_files.py), small enough for the Python pipeline (tests/hostref.Pipeline) to run in seconds.  Plain Python, no device; nothing
is committed, everything is a function of the seeds below.

  rule   phase 1: the fetch, its filters and the per-position rule -- reads of tests/bam_pileup_cases.catalogue() moved into the region,
         indel tokens at the starts of thread ranges and of position windows, the fall-through triple across window cuts, reads around the
         padded region's two ends, every filter, three block layouts, two empty samples.
  calls  stage 2 and the VCF line: seeded reads that copy the reference but for planted content.
  fail   two samples that end the run (find_snp_at_pos's std::out_of_range) beside a good one.

All three share the contigs and the region: chrS:31500-34000 on the middle contig of three, so rid is 1, reads on chrR and chrT meet both
ref_id filters, and the region crosses coordinate 32768, the edge of a 16 kbp window of the linear index."""
import functools
import os
import random

from tests import bam_files as bf
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import hostref
from tests.test_store_windows import store_window_ranges, store_windows

CONTIGS = [("chrR", 5000), ("chrS", 60000), ("chrT", 4000)]
REGION = "chrS:31500-34000"
RID = 1
RG_S, RG_E = 31500, 33999                            # splitrg's end - 1
BEG0, END0 = RG_S - 1 - 1000, RG_E + 1000             # the fetch range, 0-based
N_RUNS = [(32100, 5), (32766, 4), (33333, 3), (34200, 6)]   # runs of N on chrS (1-based start, length); the last lies in the fetched tail
MAPQ = 20
WINDOWS = [(1, 3), (2, 3)]                            # the (T, K) of the windows tests


def sequences(seed):
    rng = random.Random(seed)
    seqs = {n: "".join(rng.choice("ACGT") for _ in range(l)) for n, l in CONTIGS}
    s = list(seqs["chrS"])
    for start, n in N_RUNS:
        s[start - 1:start - 1 + n] = "N" * n
    seqs["chrS"] = "".join(s)
    return seqs


def positions(ref):
    """pv: the region's positions whose reference base is one of ACGT"""
    return [p for p in range(RG_S, RG_E + 1) if ref[p - 1] in "ACGT"]


def R(pos, cigar, **kw):
    kw.setdefault("ref_id", RID)
    return bm.make_read(pos, cigar, **kw)


def from_ref(ref, pos, cigar, rng, **kw):
    """A read whose aligned bases copy the reference (A where it has N); inserted and clipped bases are random."""
    seq = []
    at = pos
    for op, l in bm.parse_cigar(cigar):
        if op in "M=X":
            seq += [c if c in "ACGT" else "A" for c in ref[at:at + l]]
            at += l
        elif op in "IS":
            seq += [rng.choice("ACGT") for _ in range(l)]
        elif op in "DN":
            at += l
    kw.setdefault("qual", [30] * len(seq))
    return R(pos, cigar, seq="".join(seq), **kw)


def query_index(r, p):
    """Index into the read's sequence of the base aligned to 1-based position p, or None"""
    at, q = r["pos"], 0
    for op, l in r["cigar"]:
        if op in "M=X":
            if at < p <= at + l:
                return q + (p - 1 - at)
            at += l
            q += l
        elif op in "IS":
            q += l
        elif op in "DN":
            at += l
    return None


def covers(r, p):
    return r["ref_id"] == RID and r["pos"] < p <= bm.tp.end_pos(r)


def set_base(r, p, base=None, qual=None):
    k = query_index(r, p)
    if k is None:
        return
    if base is not None:
        r["seq"] = r["seq"][:k] + base + r["seq"][k + 1:]
    if qual is not None:
        r["qual"][k] = qual


def in_file_order(reads):
    """coordinate-sorted: by reference, then position; reads without a reference last (a stable sort keeps ties as given)"""
    return sorted(reads, key=lambda r: (r["ref_id"] if r["ref_id"] >= 0 else 1 << 30, r["pos"]))


def excluded_by(r):
    """The filter of BamFile::fetch that drops the read, in its order, or None: what the census counts"""
    if r["ref_id"] < 0:
        return "no reference"
    if r["ref_id"] < RID:
        return "earlier reference"
    if r["ref_id"] > RID:
        return "later reference"
    if r["pos"] >= END0:
        return "at or behind the range's end"
    if r["flag"] & 0x4:
        return "unmapped"
    if bm.tp.end_pos(r) <= BEG0:
        return "ends in front of the range"
    if r["flag"] & 0x400:
        return "duplicate"
    if r["mapq"] < MAPQ:
        return "low mapq"
    return None


FILTERS = ("no reference", "earlier reference", "later reference", "at or behind the range's end", "unmapped", "ends in front of the range",
           "duplicate", "low mapq")


def window_cuts(pv, T, K):
    """The 0-based coordinates at which the windows of (T, K) cut the fetch range (store_window_ranges' wbeg[1:])"""
    a, b = store_windows(len(pv), T, K)
    return store_window_ranges(pv, a, b, BEG0, END0)[0][1:]


def triple(c):
    """The reads of DESIGN 3.17's open case around the cut c: at the positions behind c the first covering read has a deletion, the read
    between it and the next covering one ended in front of c"""
    return [R(c - 10, "5M20D5M", mapq=31), R(c - 8, "3M", mapq=32), R(c - 6, "30M", mapq=33)]


# ---- cohort `rule` ---------------------------------------------------------------------------------------------------------------------
REUSED = ("every CIGAR operation", "the last base in front of I, D, P and zero-length I / D",
          "D and N at the position, the next read covering it or not", "a fall-through chain over three reads",
          "a short read inside a long one, first sticking at the last read", "soft clips at either end, = beside M and X",
          "an indel entry first, and one behind another read's base entry")
RULE_SNPS = (33100, 33200)


@functools.lru_cache(maxsize=None)
def rule_spec():
    seqs = sequences(20261021)
    ref = seqs["chrS"]
    pv = positions(ref)
    rng = random.Random(7)
    samples, plan = [], {}

    def S(tag, reads, payload=0xff00):
        plan.setdefault(tag, []).append(len(samples))
        samples.append(dict(reads=in_file_order(reads), payload=payload))
    # the catalogue's well-formed reads, each case moved to a place of its own in the region
    cat = {c["name"]: c for c in bc.catalogue()}
    for k, name in enumerate(REUSED):
        shift = 31700 + 130 * k - bc.RG_S
        for data, _, _ in cat[name]["samples"]:
            st, rv = bm.scan_sample(data, True, 0, 0, 1 << 30, 0)
            assert st == 0
            S("catalogue", [dict(r, pos=r["pos"] + shift, ref_id=RID, name=b"r\0", seq=str(r["seq"]), qual=list(r["qual"])) for r in rv])
    # an indel token as the first entry of a thread range (-t 3, -t 6) and so of a window of (1, 3) and (2, 3): the last M base in front
    # of the insertion is the range's first position.  (The two sets of starts lie two positions apart: a sample each.)
    for n in (3, 6):
        starts = [pv[hostref.thread_window(len(pv), n, j)[0]] for j in range(1, n)]
        S(f"indel first, -t {n}", [R(p - 5, "5M2I5M", mapq=40 + j) for j, p in enumerate(starts)])
        plan[f"range starts, -t {n}"] = starts
    # the triple, twice in one sample: across cut 2 of (1, 3) -- a plain -t 3 range start too, and four positions in front of cut 2 of
    # (2, 3), which it straddles as well -- and across cut 1 of (2, 3)
    cuts = {tk: window_cuts(pv, *tk) for tk in WINDOWS}
    plan["cuts"] = cuts
    plan["triple at"] = [cuts[(1, 3)][1], cuts[(2, 3)][0]]
    S("triple", [r for c in plan["triple at"] for r in triple(c)])
    # the padded region's two ends
    S("edge", [R(30300, "100M"), R(30450, "40M1060N60M"), R(30480, "50M")])            # ends in front of BEG0; skips into the region; in the pad
    S("edge", [R(30400, "1300M", seq="ACGT" * 325, qual=[33] * 1300)])                  # starts in front of BEG0 and reaches 31700
    S("edge", [R(33950, "80M"), R(END0 - 1, "10M"), R(END0, "10M"), R(35200, "10M")])  # the last read kept, the read that stops the fetch
    # every filter, a good read behind the filtered one
    g = 33400
    good = lambda: R(g + 2, "10M", mapq=25)
    S("filter", [R(g, "10M", flag=0x400), good()])
    S("filter", [R(g, "10M", flag=0x4), good()])
    S("filter", [R(g, "10M", mapq=MAPQ - 1), good()])
    S("filter", [good(), R(-1, "10M", ref_id=-1, flag=0x4)])
    S("filter", [R(100, "50M", ref_id=0), good(), R(200, "50M", ref_id=2)])
    # eight samples that tile 33000 .. 33330 with reads copying the reference, five of them with another base at two positions (so that
    # the cohort calls something); one in 300-byte blocks, one in a block a record
    for s in range(8):
        reads = [from_ref(ref, p, "60M", rng, mapq=30 + s, flag=(0, 16)[(s + k) % 2], qual=[20 + (s * 7 + i) % 21 for i in range(60)])
                 for k, p in enumerate(range(32990 + 3 * s, 33280, 30))]
        for p in RULE_SNPS:
            if s < 5:
                alt = "ACGT"[("ACGT".index(ref[p - 1]) + 1) % 4]
                for r in reads:
                    set_base(r, p, alt)
        S("tiled", reads, payload={0: 300, 1: bf.ONE_RECORD}.get(s, 0xff00))
    plan["blocks of 300"], plan["a block a record"] = plan["tiled"][0], plan["tiled"][1]
    # two samples the run reports as empty: reads outside the fetch range only, and no read at all
    S("empty", [R(100, "50M", ref_id=0), R(1000, "50M"), R(300, "50M", ref_id=2)])
    S("empty", [])
    return dict(name="rule", seqs=seqs, samples=samples, plan=plan)


# ---- cohort `calls` --------------------------------------------------------------------------------------------------------------------
N_CALLS = 32
IUPAC = "MRSVWYHKDB"
# planted positions (1-based), a hundred or more apart and away from the runs of N and the ranges' starts
SITES = dict(bi=31650, tri=31800, quad=32000, alt_major=32250, skew=32450, ranks=32600, indel_beside=32900, depth10=33620, depth11=33720,
             long_deletion=33995)
MORE_BI = (31560, 32700, 33050, 33150, 33260, 33450, 33530, 33850)


def alt_of(ref, p, k=1):
    return "ACGT"[("ACGT".index(ref[p - 1]) + k) % 4]


@functools.lru_cache(maxsize=None)
def calls_spec():
    seqs = sequences(20261022)
    ref = seqs["chrS"]
    rng = random.Random(20261020)
    planted = sorted(list(SITES.values()) + list(MORE_BI))
    assert all(ref[p - 1] in "ACGT" for p in planted)
    near = lambda lo, hi: any(lo - 8 <= p <= hi + 8 for p in planted)
    samples = []
    for s in range(N_CALLS):
        reads, pos = [], 30600 + rng.randrange(60)
        while pos < 34900:
            kind = rng.random()
            if near(pos, pos + 110) or kind < 0.88:
                cigar = "100M"
            elif kind < 0.92:
                a = rng.randrange(10, 80)
                cigar = f"{a}M{rng.randrange(1, 4)}I{100 - a - 3}M"
            elif kind < 0.96:
                a = rng.randrange(10, 80)
                cigar = f"{a}M{rng.randrange(1, 6)}D{100 - a}M"
            elif kind < 0.98:
                cigar = "6S94M"
            else:
                cigar = "50=50X"
            r = from_ref(ref, pos, cigar, rng, flag=rng.choice([0, 65, 16, 83, 99]), mapq=rng.randrange(MAPQ, 61))
            r["qual"] = [rng.randrange(94) for _ in r["seq"]]
            reads.append(r)
            pos += rng.randrange(40, 90)
        # (a few reads every filter drops, and reads on the other contigs)
        reads += [from_ref(ref, 32000 + 37 * s, "100M", rng, flag=0x400), from_ref(ref, 33000 + 41 * s, "100M", rng, mapq=rng.randrange(MAPQ)),
                  R(50 + s, "80M", ref_id=0), R(70 + s, "80M", ref_id=2)]
        # depth_total 10 and 11: samples 10 .. (11 ..) have no read over the site
        for first_without, p in ((10, SITES["depth10"]), (11, SITES["depth11"])):
            if s >= first_without:
                reads = [r for r in reads if not covers(r, p)]
        samples.append(reads)
    # N and IUPAC codes, away from the planted positions
    for reads in samples:
        for r in reads:
            seq = list(r["seq"])
            for k in range(len(seq)):
                x = rng.random()
                if x < 0.014 and all(abs(r["pos"] + k - q) > 12 for q in planted):
                    seq[k] = "N" if x < 0.01 else rng.choice(IUPAC)
            r["seq"] = "".join(seq)

    def plant(p, carriers, k=1, qual=None):
        for s in carriers:
            for r in samples[s]:
                if covers(r, p):
                    set_base(r, p, alt_of(ref, p, k), qual)
    plant(SITES["bi"], range(0, 12))
    plant(SITES["tri"], range(0, 8), 1); plant(SITES["tri"], range(8, 15), 2)
    plant(SITES["quad"], range(0, 6), 1); plant(SITES["quad"], range(6, 12), 2); plant(SITES["quad"], range(12, 18), 3)
    plant(SITES["alt_major"], range(0, 26))
    plant(SITES["depth10"], range(0, 4)); plant(SITES["depth11"], range(0, 4))
    for j, p in enumerate(MORE_BI):
        plant(p, rng.sample(range(N_CALLS), 3 + 2 * j))
    # strand skew: the other base on reverse reads only
    p = SITES["skew"]
    for s in range(N_CALLS):
        for r in samples[s]:
            if covers(r, p) and excluded_by(r) is None:
                r["flag"] = 16 if s < 10 else 0
    plant(p, range(0, 10))
    # the three rank sums: the other base mostly where the first covering read has the position late in the read, with mostly lower mapq
    # and quality -- the two sides' values overlap, each in its own way, so that the three sums differ
    p = SITES["ranks"]
    late = []
    for s in range(N_CALLS):
        first = next(r for r in in_file_order(samples[s]) if covers(r, p) and excluded_by(r) is None)
        is_late = (p - 1 - first["pos"] >= 50) != (s % 6 == 0)
        late += [s] if is_late else []
        for r in samples[s]:
            if covers(r, p) and excluded_by(r) is None:
                r["mapq"] = 21 + (s * 5) % 30 if is_late else 38 + s % 20
                set_base(r, p, qual=3 + (s * 7) % 40 if is_late else 25 + (s * 3) % 60)
    assert 6 <= len(late) <= N_CALLS - 6
    plant(p, late)
    # insertions and deletions beside a called SNP: the first covering read of five samples has the position as the last base in front
    p = SITES["indel_beside"]
    plant(p, range(0, 12))
    for s, cigar in ((20, "50M2I48M"), (21, "50M2I48M"), (22, "50M1I49M"), (23, "50M3D50M"), (24, "50M3D50M")):
        samples[s] = [r for r in samples[s] if not covers(r, p)] + [from_ref(ref, p - 50, cigar, rng, mapq=50 + s % 10)]
    # a deletion that runs past the end of the fetched reference (RG_E + 1000): its text is cut where the reference ends
    p = SITES["long_deletion"]
    samples[31] = [r for r in samples[31] if r["ref_id"] != RID or bm.tp.end_pos(r) < p - 25] + [from_ref(ref, p - 20, "20M1100D10M", rng, mapq=44)]
    return dict(name="calls", seqs=seqs, samples=[dict(reads=in_file_order(r), payload=0xff00 if s % 8 else 4000) for s, r in enumerate(samples)],
                plan=dict(sites=dict(SITES), more_bi=MORE_BI, late=late))


# ---- cohort `fail` ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fail_spec():
    """A good sample and two that end the run with find_snp_at_pos's std::out_of_range: a sequence shorter than its CIGAR, and an
    insertion that starts past the sequence.  (The rule's third out-of-range case, a deletion that starts past the fetched reference, cannot
    be written as a file: a deletion's text starts at most one base behind a listed position, the listed positions end 1000 bases in
    front of the fetched reference's end, so the start never passes it.  bvc_bam_pileup's own catalogue reaches it through the library.)"""
    seqs = sequences(20261023)
    rng = random.Random(3)
    reads = [[from_ref(seqs["chrS"], p, "80M", rng) for p in range(31480, 33900, 60)],
             [R(31600, "30M", seq="ACGT", qual=[30] * 4, mapq=60)],
             [R(31700, "5M3I5M", seq="ACG", qual=[30] * 3)]]
    return dict(name="fail", seqs=seqs, samples=[dict(reads=r, payload=0xff00) for r in reads], plan={})


FAIL_LINE = "index offset is out of range of the sequence"


# ---- writing ---------------------------------------------------------------------------------------------------------------------------
def write_cohort(spec, directory, bai=True):
    """The cohort's files under `directory`: <sample>.bam (and .bam.bai), ref.fa, ref.fa.fai, bam.list.  Returns the hostref.Cohort, with
    .fa, .list, .names and .voffs ([per sample: the records' virtual offsets]) beside what the pipeline reads."""
    os.makedirs(directory, exist_ok=True)
    bams, names, voffs = [], [], []
    for s, sm in enumerate(spec["samples"]):
        name = f"{spec['name']}{s:02d}"
        path = os.path.join(str(directory), name + ".bam")
        voffs.append(bf.write_bam(path, name, CONTIGS, sm["reads"], block_payload=sm["payload"]))
        if bai:
            bf.write_bai(path + ".bai", path)
        bams.append(path)
        names.append(name)
    c = hostref.Cohort(directory, bams, REGION, CONTIGS, spec["seqs"])
    c.fa = hostref.write_fasta(os.path.join(str(directory), "ref.fa"), c)
    c.list = hostref.write_bam_list(os.path.join(str(directory), "bam.list"), c)
    c.names, c.voffs, c.spec = names, voffs, spec
    return c


def groups_of(names):
    """{sample: group}: three groups, every seventh sample in none"""
    return {n: ["EAS", "AFR", "EUR"][i % 3] for i, n in enumerate(names) if i % 7 != 5}
