"""The host program with --tmp-format counts --group and BVC_HOST_COUNTS_GROUPS=1 (the counts pass keeps the groups' depths per base beside
one slot of class counts: bvc_site_acc_create_depth, bvc_site_acc_get_depth; the "<group>_AF" values come from the second pile-up's store;
GPU) against the same run with --tmp-format bin --group: the .vcf.gz and the .cvg.gz inflate to the same bytes on the generated cohorts
`rule` and `calls` of tests/cohort_cases.py -- their groups file with two samples more that no BAM holds, whose groups sort in front of and
behind the others -- for 1 and 3 threads, and on the 100 test BAMs with three groups and seven samples in none; the profile line's
accumulator bytes are the three arrays'; nothing but the two outputs is on disk; without the knob the refusal is what it was."""
import glob
import gzip
import os
import re
import subprocess

import pytest

from tests import cohort_cases as cc
from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu

KNOB = "BVC_HOST_COUNTS_GROUPS"
BATCH = 7
TIMEOUT = 120


def clean_env(extra=None):
    """The environment without any of the host program's knobs, then `extra`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BVC_HOST_")}
    env.update(extra or {})
    return env


def inflated(prefix):
    return {k: gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}


def on_disk(prefix):
    return sorted(os.path.basename(f) for f in glob.glob(str(prefix) + "*"))


# ---- the generated cohorts --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    from basevarc_amd import build as b
    d = tmp_path_factory.mktemp("host_counts_groups")
    exe, _ = b.build_host()
    made = {}
    for name, spec in (("rule", cc.rule_spec()), ("calls", cc.calls_spec())):
        c = cc.write_cohort(spec, d / name, bai=True)
        groups = d / f"{name}.groups"
        # (the file's first and last sorted group names have no sample: the present groups' rows are the middle ones)
        groups.write_text("".join(f"{k} {v}\n" for k, v in cc.groups_of(c.names).items()) + "nobody_1 AAA\nnobody_2 ZZZ\n")
        made[name] = (c, str(groups))
    return exe, made


def cohort_run(exe, c, groups, out, thread, fmt, env=None):
    cmd = [exe, "basetype", "-q", str(cc.MAPQ), "-t", str(thread), "-b", str(BATCH), "-i", c.list, "-s", c.region, "-r", c.fa, "-o", str(out), "--tmp-format", fmt,
           "-g", groups]
    return subprocess.run(cmd, capture_output=True, text=True, env=clean_env(env), timeout=TIMEOUT)


@pytest.mark.parametrize("thread", [1, 3])
@pytest.mark.parametrize("name", ["rule", "calls"])
def test_a_cohorts_outputs_are_those_of_the_binary_temp_batches(cohorts, tmp_path, name, thread):
    exe, made = cohorts
    c, groups = made[name]
    want_p, got_p = tmp_path / "bin", tmp_path / "counts"
    r0 = cohort_run(exe, c, groups, want_p, thread, "bin")
    r1 = cohort_run(exe, c, groups, got_p, thread, "counts", {KNOB: "1", "BVC_HOST_PROFILE": "1"})
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(str(want_p)), inflated(str(got_p))
    for k in want:
        assert want[k] == got[k], k
    # not an empty run, and the group columns are there: the three groups that have samples, not the file's five
    cvg = got[".cvg.gz"].decode().split("\n")
    head = next(l for l in cvg if l.startswith("#CHROM"))
    assert head.split("\t")[-3:] == ["AFR", "EAS", "EUR"] and "AAA" not in head and "ZZZ" not in head
    rows = [l.split("\t") for l in cvg if l and l[0] != "#"]
    assert len(rows) > 500 and all(re.fullmatch(r"\d+:\d+:\d+:\d+", x) for r in rows for x in r[-3:])
    assert any(r[-3:] != ["0:0:0:0"] * 3 for r in rows)
    assert sum(1 for l in got[".vcf.gz"].decode().split("\n") if l and l[0] != "#" and "EAS_AF=" in l) >= 12
    assert sorted(l for l in r0.stderr.split("\n") if "is empty." in l) == sorted(l for l in r1.stderr.split("\n") if "is empty." in l)
    assert on_disk(got_p) == ["counts.cvg.gz", "counts.vcf.gz"]
    # the revisit set is a part of the region: most group columns above came from the depth rows, not from the store
    m = re.search(r"counts pass: (\d+) positions, (\d+) revisited .*accumulator (\d+) bytes", r1.stderr)
    assert m and int(m.group(3)) == int(m.group(1)) * (2048 + 48 + 16 * 5) and int(m.group(2)) < int(m.group(1)), r1.stderr[-1000:]


# ---- the 100 test BAMs ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_counts_groups_bams")
    exe, _ = b.build_host()
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))      # 7 samples left ungrouped
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), groups=str(gf))


def test_the_test_bams_outputs_are_those_of_the_binary_temp_batches(tmp_path, inputs):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = ["-g", inputs["groups"]]
    want_p, got_p = str(tmp_path / "bin"), str(tmp_path / "counts")
    r0 = _run(exe, want_p, lst, fa, ["--tmp-format", "bin"] + extra, clean_env(), thread=4, batch=7)
    r1 = _run(exe, got_p, lst, fa, ["--tmp-format", "counts"] + extra, clean_env({KNOB: "1", "BVC_HOST_PROFILE": "1"}), thread=4, batch=7)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(want_p), inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30 and want[".cvg.gz"].count(b"\n") > 60000 and b"EUR_AF=" in want[".vcf.gz"]
    assert sorted(l for l in r0.stderr.split("\n") if "is empty." in l) == sorted(l for l in r1.stderr.split("\n") if "is empty." in l)
    assert on_disk(got_p) == ["counts.cvg.gz", "counts.vcf.gz"]
    m = re.search(r"\[profile\] main: counts pass: (\d+) positions, (\d+) revisited \((\d+) called, (\d+) with indel entries, (\d+) for the carry\), "
                  r"accumulator (\d+) bytes, store (\d+) bytes", r1.stderr)
    assert m, r1.stderr[-2000:]
    P, S, called, _, _, acc_bytes, _ = (int(x) for x in m.groups())
    assert P == 66615 and called == 76 and S <= P // 10
    assert acc_bytes == 66615 * (2048 + 48 + 16 * 3)


def test_over_the_budget_the_line_counts_the_depth_bytes(tmp_path, inputs):
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts", "-g", inputs["groups"]],
             clean_env({KNOB: "1", "BVC_HOST_STORE_GB": "0.000001"}), thread=2, batch=25)
    lines = [l for l in r.stderr.split("\n") if "--tmp-format bin" in l]
    assert r.returncode == 1 and len(lines) == 1 and "BVC_HOST_STORE_GB allows 1073" in lines[0] and str(66615 * (2096 + 48)) in lines[0], r.stderr[-1000:]
    assert glob.glob(out + "*") == []


@pytest.mark.parametrize("knob", [None, "0"])
def test_without_the_knob_the_refusal_is_what_it_was(tmp_path, inputs, knob):
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts", "--group", inputs["groups"]], clean_env({KNOB: knob} if knob else None))
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and "--tmp-format counts with --group" in r.stderr and "--tmp-format mem" in r.stderr, r.stderr[-1000:]
    assert glob.glob(out + "*") == []
