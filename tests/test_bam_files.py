"""tests/bam_files.py held to what the project already has (no device): the reads it writes come back from the BAM reader of
tests/golden/make_testdata_pileup.py field for field; the linear index it builds from a BAM's own records is the committed .bam.bai of every
fixture; the virtual offsets it returns are those a walk of the blocks finds; and `BaseVarC basetype --load` -- the CPU path through
BamFile::fetch, with the index and without -- writes the batch files the Python pipeline gives for the generated cohorts."""
import glob
import gzip
import os
import subprocess

import pytest

from tests import bam_files as bf
from tests import cohort_cases as cc
from tests import hostref
from tests.golden import make_testdata_pileup as tp

FIXTURES = sorted(glob.glob(os.path.join(hostref.DATA, "bam100", "*.bam")))


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_files")
    return {(spec["name"], bai): cc.write_cohort(spec, d / f"{spec['name']}_{int(bai)}", bai=bai)
            for spec in (cc.rule_spec(), cc.calls_spec()) for bai in (True, False)}


@pytest.mark.parametrize("name", ["rule", "calls"])
def test_the_written_reads_come_back_field_for_field(cohorts, name):
    c = cohorts[(name, True)]
    n_reads = 0
    for path, sample, sm in zip(c.bams, c.names, c.spec["samples"]):
        header, recs = tp.read_bam(path)
        assert "SO:coordinate" in header and tp.sample_name(header) == sample
        assert [l.split("\t")[1:] for l in header.split("\n") if l.startswith("@SQ")] == [[f"SN:{n}", f"LN:{l}"] for n, l in cc.CONTIGS]
        assert len(recs) == len(sm["reads"])
        for got, r in zip(recs, sm["reads"]):
            want = dict(bf.read_fields(r), ref=cc.CONTIGS[r["ref_id"]][0] if r["ref_id"] >= 0 else "*")
            assert got == want, (sample, r["pos"])
        n_reads += len(recs)
    assert n_reads > 100
    # the stream ends with the 28-byte EOF block
    assert all(open(p, "rb").read()[-28:] == bf.EOF_BLOCK for p in c.bams)


@pytest.mark.parametrize("name", ["rule", "calls"])
def test_the_returned_virtual_offsets_are_those_of_a_walk_and_the_index_is_the_records(cohorts, name):
    c = cohorts[(name, True)]
    for path, voffs, sm in zip(c.bams, c.voffs, c.spec["samples"]):
        n_ref, recs = bf.walk_bam(path)
        assert n_ref == 3 and [r[4] for r in recs] == voffs[:-1] and [r[5] for r in recs] == voffs[1:]
        assert [(r[0], r[1], r[3]) for r in recs] == [(x["ref_id"], x["pos"], x["flag"]) for x in sm["reads"]]
        lin = bf.read_bai_linear(path + ".bai")
        # by the specification's words, from the read dicts: per window the smallest offset of a mapped alignment overlapping it
        for ref_id in range(3):
            mine = [(x["pos"] >> 14, (max(tp.end_pos(x), x["pos"] + 1) - 1) >> 14, v) for x, v in zip(sm["reads"], voffs)
                    if x["ref_id"] == ref_id and not x["flag"] & 4]
            n = 1 + max([hi for _, hi, _ in mine], default=-1)
            assert len(lin[ref_id]) == n
            want = [min([v for lo, hi, v in mine if lo <= w <= hi], default=None) for w in range(n)]
            for w in range(n - 2, -1, -1):
                want[w] = want[w + 1] if want[w] is None else want[w]
            assert lin[ref_id] == want, (path, ref_id)
    # the region crosses a window edge: some sample's index names another offset behind 32768 than in front of it
    assert any(len(l[1]) > 2 and l[1][1] != l[1][2] for l in (bf.read_bai_linear(p + ".bai") for p in c.bams))


@pytest.mark.parametrize("bam", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_the_linear_index_of_a_fixture_is_rebuilt_from_its_records(bam):
    """n_intv and every ioffset of the committed .bam.bai, for every reference"""
    n_ref, recs = bf.walk_bam(bam)
    want = bf.read_bai_linear(bam + ".bai")
    got = bf.linear_index(recs, n_ref)
    assert len(got) == len(want) == n_ref and sum(len(l) for l in want) > 1000
    for r in range(n_ref):
        assert len(got[r]) == len(want[r]) and got[r] == want[r], r


def test_there_are_the_hundred_fixtures():
    assert len(FIXTURES) == 100


@pytest.mark.parametrize("bai", [True, False], ids=["bai", "no_bai"])
@pytest.mark.parametrize("name", ["rule", "calls"])
def test_load_writes_the_pipelines_batch_files_with_the_index_and_without(cohorts, tmp_path, name, bai):
    from basevarc_amd import build as b
    exe, _ = b.build_host()
    c = cohorts[(name, bai)]
    assert all(os.path.exists(p + ".bai") == bai for p in c.bams)
    thread, batch = 3, 7
    out = str(tmp_path / "load")
    r = subprocess.run([exe, "basetype", "--load", "-q", "20", "-t", str(thread), "-b", str(batch), "-i", c.list, "-s", c.region, "-r", c.fa, "-o", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    pipe = hostref.Pipeline(mapq=20, batch=batch, thread=thread, cohort=c)
    want = pipe.batch_files()
    assert len(want) == thread * (1 + (pipe.n - 1) // batch)
    for (t, ib), text in want.items():
        assert gzip.decompress(open(f"{out}.tmp.thread.{t}/batch.{ib}", "rb").read()).decode() == text, (t, ib)
    assert sorted(l for l in r.stderr.split("\n") if "is empty." in l) == sorted(f"warning: {n} region {c.region} is empty." for n in pipe.empty)
