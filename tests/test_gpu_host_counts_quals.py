"""The host program with --tmp-format counts and BVC_HOST_COUNTS_QUALS=Q (the counts pass keeps Q quality columns for each base:
bvc_site_acc_create_quals, include/bvc_site_acc_quals.h; GPU) against the same run with --tmp-format bin: the .vcf.gz and the .cvg.gz
inflate to the same bytes on the 100 test BAMs at 40 columns (their qualities stop at 39), without and with --group, and on the generated
cohorts `rule` and `calls` of tests/cohort_cases.py at the smallest multiple of 4 above their highest counted quality -- taken from the
model --; four columns fewer end the run with one line that names a BAM, the width and BVC_HOST_COUNTS_QUALS=128.  A budget the wide
counts do not fit holds the narrow ones; a bad value is refused before any file is made; with the knob at 128 or unset the run is what it
was."""
import glob
import os
import re
import subprocess

import pytest

from tests import bam_counts_quals_model as qm
from tests import bam_pileup_model as bm
from tests import cohort_cases as cc
from tests.test_gpu_host import _run
from tests.test_gpu_host_counts_groups import clean_env, inflated, on_disk

pytestmark = pytest.mark.gpu

KNOB = "BVC_HOST_COUNTS_QUALS"
BATCH = 7
TIMEOUT = 120
PROFILE = re.compile(r"\[profile\] main: counts pass: (\d+) positions, (\d+) revisited \((\d+) called, (\d+) with indel entries, (\d+) for the carry\), "
                     r"accumulator (\d+) bytes, store (\d+) bytes")


# ---- the 100 test BAMs ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_counts_quals_bams")
    exe, _ = b.build_host()
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))      # 7 samples left ungrouped
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), groups=str(gf))


@pytest.fixture(scope="module")
def bin_runs(tmp_path_factory, inputs):
    """--tmp-format bin -t 4 -b 7 on the test BAMs, without and with the groups file: the inflated outputs and the "is empty" lines"""
    d = tmp_path_factory.mktemp("host_counts_quals_bin")
    made = {}
    for grouped in (False, True):
        out = str(d / f"bin{int(grouped)}")
        r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "bin"] + (["-g", inputs["groups"]] if grouped else []), clean_env(), thread=4, batch=7)
        assert r.returncode == 0, r.stderr[-1000:]
        made[grouped] = (inflated(out), sorted(l for l in r.stderr.split("\n") if "is empty." in l))
    return made


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
def test_forty_columns_on_the_test_bams_give_the_outputs_of_the_binary_temp_batches(tmp_path, inputs, bin_runs, grouped):
    got_p = str(tmp_path / "counts")
    extra = ["-g", inputs["groups"]] if grouped else []
    env = {KNOB: "40", "BVC_HOST_PROFILE": "1"}
    if grouped:
        env["BVC_HOST_COUNTS_GROUPS"] = "1"
    r = _run(inputs["exe"], got_p, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"] + extra, clean_env(env), thread=4, batch=7)
    assert r.returncode == 0, r.stderr[-1000:]
    want, empty = bin_runs[grouped]
    got = inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30 and want[".cvg.gz"].count(b"\n") > 60000 and (b"EUR_AF=" in want[".vcf.gz"]) == grouped
    assert sorted(l for l in r.stderr.split("\n") if "is empty." in l) == empty
    assert on_disk(got_p) == ["counts.cvg.gz", "counts.vcf.gz"]
    m = PROFILE.search(r.stderr)
    assert m, r.stderr[-2000:]
    P, S, called, indel, _, acc_bytes, _ = (int(x) for x in m.groups())
    G = 3 if grouped else 0
    assert P == 66615 and called == 76 and indel == 45 and S <= P // 10
    assert acc_bytes == 66615 * (640 + 48 + 16 * G) == qm.acc_bytes(66615, 40, G)


def test_thirty_six_columns_on_the_test_bams_end_the_run_with_the_line(tmp_path, inputs):
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], clean_env({KNOB: "36"}), thread=4, batch=7)
    lines = [l for l in r.stderr.split("\n") if KNOB in l]
    assert r.returncode == 1 and len(lines) == 1, r.stderr[-1000:]
    assert "a base quality of 36 or more in " in lines[0] and ".bam" in lines[0] and lines[0].endswith("BVC_HOST_COUNTS_QUALS=128"), lines[0]
    assert glob.glob(out + "*") == []


@pytest.mark.parametrize("knob", [None, "128"])
def test_with_the_knob_at_128_or_unset_the_run_is_what_it_was(tmp_path, inputs, bin_runs, knob):
    got_p = str(tmp_path / "counts")
    env = {"BVC_HOST_PROFILE": "1"}
    if knob:
        env[KNOB] = knob
    r = _run(inputs["exe"], got_p, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], clean_env(env), thread=4, batch=7)
    assert r.returncode == 0, r.stderr[-1000:]
    want, _ = bin_runs[False]
    got = inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    m = PROFILE.search(r.stderr)
    assert m and int(m.group(1)) == 66615 and int(m.group(6)) == 66615 * (2048 + 48), r.stderr[-2000:]


def test_a_budget_the_wide_counts_do_not_fit_holds_forty_columns(tmp_path, inputs):
    """0.1 GB are 107,374,182 bytes: the region's wide counts take 139.6 MB, forty columns 45.8 MB.  (This stands in for a chromosome on
    a device's memory, which no test can hold.)"""
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], clean_env({"BVC_HOST_STORE_GB": "0.1"}), thread=2, batch=25)
    lines = [l for l in r.stderr.split("\n") if "--tmp-format bin" in l]
    assert r.returncode == 1 and len(lines) == 1 and "BVC_HOST_STORE_GB allows 107374182" in lines[0] and "take 139625040 bytes" in lines[0], r.stderr[-1000:]
    assert glob.glob(out + "*") == []
    # the same budget at 44 columns is refused with the narrow bytes, not the wide ones ...
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], clean_env({"BVC_HOST_STORE_GB": "0.04", KNOB: "44"}), thread=2, batch=25)
    lines = [l for l in r.stderr.split("\n") if "--tmp-format bin" in l]
    assert r.returncode == 1 and len(lines) == 1 and f"take {66615 * (704 + 48)} bytes" in lines[0], r.stderr[-1000:]
    # ... and 0.1 GB hold forty columns, and afterwards the second pile-up's batches
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"],
             clean_env({"BVC_HOST_STORE_GB": "0.1", KNOB: "40", "BVC_HOST_PROFILE": "1"}), thread=2, batch=25)
    m = PROFILE.search(r.stderr)
    assert r.returncode == 0 and m and int(m.group(6)) == 45831120, r.stderr[-1000:]
    assert on_disk(out) == ["counts.cvg.gz", "counts.vcf.gz"]


@pytest.mark.parametrize("knob", ["42", "0", "132", "forty"])
def test_a_bad_value_is_refused_before_any_file_is_made(tmp_path, inputs, knob):
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], clean_env({KNOB: knob}))
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and "BVC_HOST_COUNTS_QUALS must be a multiple of 4 in 4..128" in r.stderr, r.stderr[-1000:]
    assert glob.glob(out + "*") == [] and "basetype start" not in r.stdout


# ---- the generated cohorts --------------------------------------------------------------------------------------------------------------
def highest_counted_quality(spec):
    """(the highest quality byte of a counted observation over the cohort, per sample its own) from the model on the records the files hold"""
    ref = spec["seqs"]["chrS"]
    pv = cc.positions(ref)
    samples = [(b"".join(bm.pack_record(r) for r in sm["reads"]), True, cc.RID) for sm in spec["samples"]]
    exp = bm.expected(samples, cc.BEG0, cc.END0, cc.MAPQ, pv, cc.RG_S, ref[cc.RG_S - 1:cc.RG_E + 1000])
    assert exp["rc"] == 0
    each = [max(qm.counted_qualities([m]), default=-1) for m in exp["maps"]]
    return max(each), each


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    from basevarc_amd import build as b
    d = tmp_path_factory.mktemp("host_counts_quals")
    exe, _ = b.build_host()
    made = {}
    for name, spec in (("rule", cc.rule_spec()), ("calls", cc.calls_spec())):
        c = cc.write_cohort(spec, d / name, bai=True)
        groups = d / f"{name}.groups"
        groups.write_text("".join(f"{k} {v}\n" for k, v in cc.groups_of(c.names).items()))
        made[name] = (c, str(groups), highest_counted_quality(spec))
    return exe, made


def cohort_run(exe, c, out, thread, fmt, env=None, groups=None):
    cmd = [exe, "basetype", "-q", str(cc.MAPQ), "-t", str(thread), "-b", str(BATCH), "-i", c.list, "-s", c.region, "-r", c.fa, "-o", str(out), "--tmp-format", fmt]
    return subprocess.run(cmd + (["-g", groups] if groups else []), capture_output=True, text=True, env=clean_env(env), timeout=TIMEOUT)


def test_the_cohorts_highest_qualities_are_what_the_tests_below_rest_on(cohorts):
    _, made = cohorts
    assert made["rule"][2][0] == 41 and made["calls"][2][0] == 93                # (`calls` draws its qualities from 0..93)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("name", ["rule", "calls"])
def test_a_cohort_at_the_smallest_width_that_holds_it(cohorts, tmp_path, name, grouped):
    exe, made = cohorts
    c, groups, (highest, _) = made[name]
    Q = (highest // 4 + 1) * 4
    assert highest < Q <= highest + 4 and qm.quals_ok(Q)
    want_p, got_p = tmp_path / "bin", tmp_path / "counts"
    env = {KNOB: str(Q), "BVC_HOST_PROFILE": "1"}
    if grouped:
        env["BVC_HOST_COUNTS_GROUPS"] = "1"
    r0 = cohort_run(exe, c, want_p, 3, "bin", groups=groups if grouped else None)
    r1 = cohort_run(exe, c, got_p, 3, "counts", env, groups=groups if grouped else None)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(str(want_p)), inflated(str(got_p))
    for k in want:
        assert want[k] == got[k], k
    rows = [l for l in got[".cvg.gz"].decode().split("\n") if l and l[0] != "#"]
    assert len(rows) > 500 and sum(1 for l in got[".vcf.gz"].decode().split("\n") if l and l[0] != "#") >= 2
    assert sorted(l for l in r0.stderr.split("\n") if "is empty." in l) == sorted(l for l in r1.stderr.split("\n") if "is empty." in l)
    assert on_disk(got_p) == ["counts.cvg.gz", "counts.vcf.gz"]
    m = PROFILE.search(r1.stderr)
    assert m and int(m.group(6)) == qm.acc_bytes(int(m.group(1)), Q, 3 if grouped else 0) and int(m.group(2)) < int(m.group(1)), r1.stderr[-1000:]


@pytest.mark.parametrize("name", ["rule", "calls"])
def test_a_cohort_at_four_columns_fewer_ends_the_run_with_the_line(cohorts, tmp_path, name):
    exe, made = cohorts
    c, _, (highest, each) = made[name]
    Q = (highest // 4 + 1) * 4 - 4
    assert Q <= highest
    out = tmp_path / "counts"
    r = cohort_run(exe, c, out, 3, "counts", {KNOB: str(Q)})
    lines = [l for l in r.stderr.split("\n") if KNOB in l]
    assert r.returncode == 1 and len(lines) == 1, r.stderr[-1000:]
    m = re.fullmatch(rf"ERROR: a base quality of {Q} or more in (\S+): the counts keep {Q} quality columns, run with BVC_HOST_COUNTS_QUALS=128", lines[0])
    assert m, lines[0]
    # the BAM it names is one whose sample the model refuses at this width
    refused = {os.path.basename(b) for b, q in zip(c.bams, each) if q >= Q}
    assert os.path.basename(m.group(1)) in refused and 0 < len(refused)
    assert on_disk(out) == []
