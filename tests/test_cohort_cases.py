"""The census of tests/cohort_cases.py (no device): the generated cohorts hold what they are for.  Every count is one of the Python
pipeline's own output (tests/hostref.Pipeline) or of the read dicts -- a condition on the test data, not a measurement of the product."""
import gzip
import struct

import pytest

from tests import bam_files as bf
from tests import bam_pileup_model as bm
from tests import cohort_cases as cc
from tests import hostref
from tests.test_store_windows import store_window_ranges, store_windows


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("cohort_cases")
    out = {}
    for spec in (cc.rule_spec(), cc.calls_spec()):
        c = cc.write_cohort(spec, d / spec["name"])
        pipe = hostref.Pipeline(mapq=cc.MAPQ, batch=7, thread=1, cohort=c)
        vcf, cvg = pipe.outputs()
        out[spec["name"]] = dict(cohort=c, pipe=pipe, vcf=[l.split("\t") for l in vcf.split("\n") if l], cvg=[l.split("\t") for l in cvg.split("\n") if l])
    return out


def info_of(fields):
    return dict(kv.split("=") for kv in fields[7].split(";"))


def test_the_shape_both_cohorts_share(built):
    for name, b in built.items():
        c, pipe = b["cohort"], b["pipe"]
        assert 24 <= pipe.n <= 40 and [n for n, _ in c.contigs].index(pipe.chr) == cc.RID == 1
        assert (pipe.rg_s, pipe.rg_e) == (cc.RG_S, cc.RG_E) and pipe.rg_s < 32768 < pipe.rg_e and 2000 < len(pipe.pv) < 2600
        # runs of N in the region: those positions are not listed
        n_in_region = [p for p in range(cc.RG_S, cc.RG_E + 1) if c.sequences["chrS"][p - 1] == "N"]
        assert len(n_in_region) >= 10 and not set(n_in_region) & set(pipe.pv) and len(pipe.pv) + len(n_in_region) == cc.RG_E - cc.RG_S + 1
        # reads on the earlier and on the later contig
        refs = {r["ref_id"] for sm in c.spec["samples"] for r in sm["reads"]}
        assert {0, 1, 2} <= refs, name


def test_calls_holds_the_planted_sites(built):
    b = built["calls"]
    called = {int(f[1]): f for f in b["vcf"]}
    sites = cc.SITES
    assert len(called) >= 12
    for key in ("bi", "tri", "quad", "alt_major", "skew", "ranks", "indel_beside", "depth10", "depth11"):
        assert sites[key] in called, key
    n_alt = lambda p: len(called[p][4].split(","))
    assert n_alt(sites["bi"]) == 1 and n_alt(sites["tri"]) == 2 and n_alt(sites["quad"]) == 3
    assert all(int(info_of(called[sites[k]])["CM_DP"]) >= 11 for k in ("bi", "tri", "quad"))
    assert int(info_of(called[sites["depth10"]])["CM_DP"]) == 10 and int(info_of(called[sites["depth11"]])["CM_DP"]) == 11
    # the other allele is the major one
    assert float(info_of(called[sites["alt_major"]])["CM_AF"]) > 0.5
    # strand skew: every observation of the other base on the reverse strand, none of the reference base
    skew = info_of(called[sites["skew"]])
    assert skew["SB_ALT"].split(",")[0] == "0" and skew["SB_REF"].split(",")[1] == "0" and float(skew["FS"]) > 30
    # the three rank sums differ from zero and from each other
    ranks = info_of(called[sites["ranks"]])
    sums = [abs(float(ranks[k])) for k in ("MQRankSum", "BaseQRankSum", "ReadPosRankSum")]
    assert all(x > 1.0 for x in sums) and len(set(sums)) == 3, sums
    # a called position with insertions and deletions in its CVG line, and the deletion cut at the end of the fetched reference
    cvg = {int(f[1]): f for f in b["cvg"]}
    beside = cvg[sites["indel_beside"]][8]
    assert "+" in beside and "-" in beside, beside
    longest = cvg[sites["long_deletion"]][8]
    assert longest.startswith("-") and longest.endswith("|1") and len(longest) - 3 == cc.RG_E + 1000 - sites["long_deletion"] < 1100
    # N and IUPAC codes among the reads, all dropped: some listed position has fewer observations than samples with a read over it
    letters = set("".join(r["seq"] for sm in b["cohort"].spec["samples"] for r in sm["reads"]))
    assert "N" in letters and letters & set(cc.IUPAC)
    # qualities over the whole printable range, so that tiles of one byte an observation do not fit
    quals = [e["qual"] for m in b["pipe"].maps for e in m.values() if not e["is_indel"]]
    assert min(quals) == 0 and max(quals) == 93 and sum(1 for q in quals if q >= 63) > 1000


def test_rule_holds_the_planted_reads(built):
    b = built["rule"]
    c, pipe, plan = b["cohort"], b["pipe"], b["cohort"].spec["plan"]
    reads = [r for sm in c.spec["samples"] for r in sm["reads"]]
    ops = set(op for r in reads for op, _ in r["cigar"])
    assert ops == set("MIDNSHP=X")
    assert any(op in "ID" and l == 0 for r in reads for op, l in r["cigar"])
    # every filter of the fetch drops at least one read
    dropped = [cc.excluded_by(r) for r in reads]
    assert all(dropped.count(f) >= 1 for f in cc.FILTERS), {f: dropped.count(f) for f in cc.FILTERS}
    # reads that start in front of the padded region and reach into it, and a read that is the last one kept
    assert any(r["pos"] < cc.BEG0 and bm.tp.end_pos(r) > cc.RG_S and cc.excluded_by(r) is None for r in reads)
    assert any(r["pos"] == cc.END0 - 1 for r in reads) and any(r["pos"] == cc.END0 for r in reads)
    # two samples reported empty: one with reads outside the range only, one without a read
    assert pipe.empty == [c.names[s] for s in plan["empty"]] and len(pipe.empty) == 2
    assert [len(c.spec["samples"][s]["reads"]) for s in plan["empty"]] == [3, 0]
    # an indel token is the first entry of every thread range of -t 3 and -t 6, and so of every window of (1, 3) and (2, 3)
    for n in (3, 6):
        (s,) = plan[f"indel first, -t {n}"]
        starts = [pipe.pv[hostref.thread_window(len(pipe.pv), n, j)[0]] for j in range(1, n)]
        assert starts == plan[f"range starts, -t {n}"]
        for p in starts:
            assert pipe.maps[s][p]["is_indel"] and not pipe.maps[s][p - 1]["is_indel"]
    for T, K in cc.WINDOWS:
        a, _ = store_windows(len(pipe.pv), T, K)
        assert all(pipe.pv[x] in plan[f"range starts, -t {T * K}"] for x in a[1:])
    # something is called, so that the VCF has lines
    called = {int(f[1]) for f in b["vcf"]}
    assert set(cc.RULE_SNPS) <= called


def test_rule_has_records_that_straddle_blocks(built):
    c, plan = built["rule"]["cohort"], built["rule"]["cohort"].spec["plan"]

    def blocks(path):
        raw, at, out = open(path, "rb").read(), 0, []
        while at < len(raw):
            bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
            out.append((at, struct.unpack_from("<I", raw, at + bsize - 4)[0]))
            at += bsize
        return out
    # 300-byte payloads: a record's end lies in another block than its start
    s = plan["blocks of 300"]
    isize = dict(blocks(c.bams[s]))
    assert max(isize.values()) == 300
    v = c.voffs[s]
    straddling = sum(1 for v0, v1 in zip(v, v[1:]) if (v1 >> 16) != (v0 >> 16) and (v1 & 0xffff) != 0)
    assert straddling >= 1
    # a block a record: every record begins at offset 0 of a block of its own
    s = plan["a block a record"]
    v = c.voffs[s]
    assert len(v) > 5 and all(x & 0xffff == 0 for x in v) and len(set(x >> 16 for x in v)) == len(v)
    assert gzip.open(c.bams[s]).read()[:4] == b"BAM\x01"


@pytest.mark.parametrize("T, K", cc.WINDOWS)
def test_the_triple_has_teeth(built, T, K):
    """For the sample with the planted triple: a window piled up from reads filtered by the WINDOW's start (what the host program did
    before the fix) differs from the whole region's pile-up at the positions behind the cut; filtered by the REGION's start, over the
    records from the window's index offset on (what it does now), it is the whole region's."""
    b = built["rule"]
    c, pipe, plan = b["cohort"], b["pipe"], b["cohort"].spec["plan"]
    (s,) = plan["triple"]
    data = gzip.open(c.bams[s]).read()
    _, recs = bf.walk_bam(c.bams[s])
    first_record = len(bf.header_bytes(c.names[s], cc.CONTIGS))
    starts = {r[4]: r[6] for r in recs}                        # virtual offset -> the record's offset in the inflated stream
    assert min(starts.values()) == first_record
    lin = bf.read_bai_linear(c.bams[s] + ".bai")[cc.RID]
    refseq = pipe.refseq
    whole = bm.expected([(data[first_record:], True, cc.RID)], cc.BEG0, cc.END0, cc.MAPQ, pipe.pv, pipe.rg_s, refseq)["maps"][0]
    a, bb = store_windows(len(pipe.pv), T, K)
    wbeg, wend = store_window_ranges(pipe.pv, a, bb, cc.BEG0, cc.END0)
    differing = 0
    for w in range(K):
        pos = pipe.pv[a[w]:bb[w]]
        want = {p: e for p, e in whole.items() if p in set(pos)}
        old = bm.expected([(data[first_record:], True, cc.RID)], wbeg[w], wend[w], cc.MAPQ, pos, pipe.rg_s, refseq)["maps"][0]
        differing += sum(1 for p in pos if (p in old) != (p in want))
        from_index = starts[lin[min(wbeg[w] >> 14, len(lin) - 1)]]
        new = bm.expected([(data[from_index:], True, cc.RID)], cc.BEG0, wend[w], cc.MAPQ, pos, pipe.rg_s, refseq)["maps"][0]
        strip = lambda m: {p: {k: v for k, v in e.items() if not (e["is_indel"] and k == "mapq")} for p, e in m.items()}
        assert strip(new) == strip(want), w
    assert differing >= 10, differing
