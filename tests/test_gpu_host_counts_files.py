"""The host program's counts files (BVC_HOST_COUNTS_SAVE / BVC_HOST_COUNTS_LOAD with --tmp-format counts; host/counts_file.cpp,
bvc_site_acc_pack / bvc_site_acc_add_packed; GPU): partial counts saved by jobs over parts of the cohort and loaded by the final run give
the .vcf.gz and .cvg.gz of a plain --tmp-format counts run, compared as inflated bytes -- on the 100 test BAMs with -t 4 -b 7 (two halves,
one half with a mixed batch, chained files, files of 128 and of 40 columns, with --group), on the generated cohorts `rule` and `calls`
(tests/cohort_cases.py) with 1 and 3 threads, and on `rule` cut to a region without calls or indels, where nothing is revisited and the
sample names come from the files alone; and every refusal is one line that names the file and the field."""
import glob
import gzip
import os
import re
import subprocess

import pytest

from tests import cohort_cases as cc
from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu

TIMEOUT = 180


def clean_env(extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BVC_HOST_")}
    env.update(extra or {})
    return env


def inflated(prefix):
    return {k: gzip.decompress(open(str(prefix) + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}


def on_disk(prefix):
    return sorted(os.path.basename(f) for f in glob.glob(str(prefix) + "*"))


def files_line(r):
    m = re.search(r"\[profile\] main: counts files: (\d+) loaded \((\d+) entries added, (\d+) bytes\), (\d+) BAMs skipped, (\d+) of (\d+) batches piled up in pass 1, "
                  r"(\d+) saved \((\d+) entries written, (\d+) bytes\), accumulator (\d+) bytes", r.stderr)
    assert m, r.stderr[-2000:]
    return dict(zip(("loaded", "added", "load_bytes", "skipped", "piled", "batches", "saved", "written", "save_bytes", "acc_bytes"), (int(x) for x in m.groups())))


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """The 100 test BAMs: the plain run's outputs, and the files a (BAMs 0..39) and b (40..99), made once."""
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_counts_files")
    exe, _ = b.build_host()
    fa, lst = hostref.write_fasta(str(d / "chr17.fa")), hostref.write_bam_list(str(d / "bam.list"))
    lines = [l for l in open(lst).read().split("\n") if l]
    assert len(lines) == 100

    def sub_list(name, lo, hi):
        (d / name).write_text("".join(l + "\n" for l in lines[lo:hi]))
        return str(d / name)
    S = dict(exe=exe, fa=fa, lst=lst, d=d, sub_list=sub_list, lines=lines)

    def run(out, lst_, env=None, extra=()):
        return _run(exe, str(out), lst_, fa, ["--tmp-format", "counts"] + list(extra), clean_env(dict(env or {}, BVC_HOST_PROFILE="1")), thread=4, batch=7)
    S["run"] = run
    r = run(d / "plain", lst)
    assert r.returncode == 0, r.stderr[-1000:]
    S["want"] = inflated(d / "plain")
    assert S["want"][".vcf.gz"].count(b"\n") > 30 and S["want"][".cvg.gz"].count(b"\n") > 60000
    for name, lo, hi in (("a", 0, 40), ("b", 40, 100)):
        r = run(d / ("job_" + name), sub_list(name + ".list", lo, hi), {"BVC_HOST_COUNTS_SAVE": str(d / (name + ".counts"))})
        assert r.returncode == 0, r.stderr[-1000:]
        # a saving job ends with status 0 and one line, and writes no VCF or CVG
        assert on_disk(d / ("job_" + name)) == [] and r.stdout.count("basetype counts saved -- ") == 1 and "basetype computing done" not in r.stdout
        line = files_line(r)
        assert line["saved"] == 1 and line["piled"] == line["batches"] and line["skipped"] == 0 and line["written"] > 100000
        assert line["save_bytes"] == os.path.getsize(str(d / (name + ".counts"))) < line["acc_bytes"] == 66615 * 2096
        S[name] = str(d / (name + ".counts"))
    return S


def same_outputs(S, out):
    got = inflated(out)
    for k in S["want"]:
        assert got[k] == S["want"][k], k
    assert on_disk(out) == [os.path.basename(str(out)) + ".cvg.gz", os.path.basename(str(out)) + ".vcf.gz"]


def test_both_halves_loaded_no_batch_is_piled_up_in_pass_one(bams, tmp_path):
    S = bams
    r = S["run"](tmp_path / "all", S["lst"], {"BVC_HOST_COUNTS_LOAD": S["a"] + ":" + S["b"]})
    assert r.returncode == 0, r.stderr[-1000:]
    same_outputs(S, tmp_path / "all")
    line = files_line(r)
    assert line["loaded"] == 2 and line["skipped"] == 100 and line["piled"] == 0 and line["batches"] == 15 and line["saved"] == 0
    assert line["load_bytes"] == os.path.getsize(S["a"]) + os.path.getsize(S["b"]) and line["added"] > 200000
    assert "counts pass: 66615 positions" in r.stderr


def test_one_half_loaded_a_mixed_batch_piles_up_only_the_others(bams, tmp_path):
    S = bams
    r = S["run"](tmp_path / "half", S["lst"], {"BVC_HOST_COUNTS_LOAD": S["a"]})
    assert r.returncode == 0, r.stderr[-1000:]
    same_outputs(S, tmp_path / "half")
    line = files_line(r)
    assert line["loaded"] == 1 and line["skipped"] == 40 and line["piled"] == 15 - 5           # batches 0..4 hold BAMs 0..34; 35..41 is mixed


def test_chained_files_hold_the_sum_and_the_union(bams, tmp_path):
    S = bams
    c = str(tmp_path / "c.counts")
    r = S["run"](tmp_path / "job_c", S["sub_list"]("c.list", 0, 70), {"BVC_HOST_COUNTS_LOAD": S["a"], "BVC_HOST_COUNTS_SAVE": c})
    assert r.returncode == 0 and on_disk(tmp_path / "job_c") == [], r.stderr[-1000:]
    line = files_line(r)
    assert line["loaded"] == 1 and line["saved"] == 1 and line["skipped"] == 40 and line["written"] >= line["added"]
    r = S["run"](tmp_path / "all", S["lst"], {"BVC_HOST_COUNTS_LOAD": c})
    assert r.returncode == 0, r.stderr[-1000:]
    same_outputs(S, tmp_path / "all")
    assert files_line(r)["skipped"] == 70


def test_files_of_128_columns_into_40_and_the_other_way_round(bams, tmp_path):
    """The test BAMs' highest counted quality is 39: 40 columns hold every count, 36 do not."""
    S = bams
    r = S["run"](tmp_path / "narrow", S["lst"], {"BVC_HOST_COUNTS_LOAD": S["a"] + ":" + S["b"], "BVC_HOST_COUNTS_QUALS": "40"})
    assert r.returncode == 0, r.stderr[-1000:]
    same_outputs(S, tmp_path / "narrow")
    a40 = str(tmp_path / "a40.counts")
    r = S["run"](tmp_path / "job_a40", S["sub_list"]("a.list", 0, 40), {"BVC_HOST_COUNTS_SAVE": a40, "BVC_HOST_COUNTS_QUALS": "40"})
    assert r.returncode == 0, r.stderr[-1000:]
    narrow, wide = open(a40, "rb").read(), open(S["a"], "rb").read()
    assert narrow[:20] == wide[:20] and narrow[24:] == wide[24:] and narrow[20] == 40 and wide[20] == 128      # (the cells are logical: only n_quals differs)
    r = S["run"](tmp_path / "wide", S["lst"], {"BVC_HOST_COUNTS_LOAD": a40 + ":" + S["b"]})
    assert r.returncode == 0, r.stderr[-1000:]
    same_outputs(S, tmp_path / "wide")
    r = S["run"](tmp_path / "tight", S["lst"], {"BVC_HOST_COUNTS_LOAD": S["a"] + ":" + S["b"], "BVC_HOST_COUNTS_QUALS": "36"})
    assert r.returncode == 1 and r.stderr.count("ERROR") == 1 and on_disk(tmp_path / "tight") == [], r.stderr[-1000:]
    line = next(l for l in r.stderr.split("\n") if "ERROR" in l)
    assert S["a"] in line and re.search(r"base quality 3[6-9] ", line) and "36 quality columns" in line and "BVC_HOST_COUNTS_QUALS=128" in line, line


def test_with_groups_saved_and_loaded(bams, tmp_path):
    from tests import hostref
    S = bams
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = tmp_path / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))      # 7 samples left ungrouped
    env, extra = {"BVC_HOST_COUNTS_GROUPS": "1"}, ["-g", str(gf)]
    r = S["run"](tmp_path / "plain_g", S["lst"], env, extra)
    assert r.returncode == 0, r.stderr[-1000:]
    want = inflated(tmp_path / "plain_g")
    assert b"EUR_AF=" in want[".vcf.gz"]
    files = []
    for name, lo, hi in (("ga", 0, 40), ("gb", 40, 100)):
        files.append(str(tmp_path / (name + ".counts")))
        r = S["run"](tmp_path / name, S["sub_list"](name + ".list", lo, hi), dict(env, BVC_HOST_COUNTS_SAVE=files[-1]), extra)
        assert r.returncode == 0, r.stderr[-1000:]
    r = S["run"](tmp_path / "all_g", S["lst"], dict(env, BVC_HOST_COUNTS_LOAD=":".join(files)), extra)
    assert r.returncode == 0 and files_line(r)["piled"] == 0, r.stderr[-1000:]
    got = inflated(tmp_path / "all_g")
    for k in want:
        assert got[k] == want[k], k
    # a file saved without groups is refused
    r = S["run"](tmp_path / "mixed", S["lst"], dict(env, BVC_HOST_COUNTS_LOAD=S["a"] + ":" + files[1]), extra)
    assert r.returncode == 1 and on_disk(tmp_path / "mixed") == [], r.stderr[-1000:]
    line = next(l for l in r.stderr.split("\n") if "ERROR" in l)
    assert S["a"] in line and "depth_groups" in line, line


def test_the_refusals_one_run_each(bams, tmp_path):
    S = bams
    from tests import hostref
    both = S["a"] + ":" + S["b"]

    def refused(name, lst, load, *words, args=None, budget=None):
        out = tmp_path / name
        env = clean_env({"BVC_HOST_COUNTS_LOAD": load})
        if budget:
            env["BVC_HOST_STORE_GB"] = budget
        cmd = [S["exe"], "basetype", "-q", "20", "-t", "4", "-b", "7", "-i", lst, "-s", hostref.REGION, "-r", S["fa"], "-o", str(out), "--tmp-format", "counts"]
        for k, v in (args or {}).items():
            cmd[cmd.index(k) + 1] = v
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=TIMEOUT)
        lines = [l for l in r.stderr.split("\n") if "ERROR" in l]
        assert r.returncode == 1 and len(lines) == 1 and all(w in lines[0] for w in words) and on_disk(out) == [], (name, r.stderr[-1000:])
        assert "is empty." not in r.stderr or budget                          # (refused before anything is piled up)
    chrom, span = hostref.REGION.split(":")
    lo, hi = (int(x) for x in span.split("-"))
    refused("region", S["lst"], both, S["a"], "range", args={"-s": f"{chrom}:{lo}-{hi - 100}"})
    refused("mapq", S["lst"], both, S["a"], "-q", "20", args={"-q": "21"})
    refused("twice", S["lst"], S["a"] + ":" + S["a"], S["a"], "BAM list", "records too")
    refused("dropped", S["sub_list"]("dropped.list", 1, 100), both, S["a"], "BAM list", S["lines"][0], "not in --input")
    (tmp_path / "twice.list").write_text("".join(l + "\n" for l in S["lines"] + S["lines"][:1]))
    refused("listed_twice", str(tmp_path / "twice.list"), both, "--input lists", S["lines"][0], "twice")
    cut = tmp_path / "b_short.counts"
    cut.write_bytes(open(S["b"], "rb").read()[:-1])
    refused("cut", S["lst"], S["a"] + ":" + str(cut), str(cut), "truncated")
    # BVC_HOST_STORE_GB still caps the accumulator with LOAD set
    refused("budget", S["lst"], both, "BVC_HOST_STORE_GB allows", "--tmp-format bin", budget="0.000001")


# ---- the generated cohorts --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    from basevarc_amd import build as b
    d = tmp_path_factory.mktemp("host_counts_files_cohorts")
    exe, _ = b.build_host()
    return exe, d, {name: cc.write_cohort(spec, d / name, bai=True) for name, spec in (("rule", cc.rule_spec()), ("calls", cc.calls_spec()))}


def cohort_run(exe, lst, c, out, thread, env=None, region=None):
    cmd = [exe, "basetype", "-q", str(cc.MAPQ), "-t", str(thread), "-b", "2", "-i", lst, "-s", region or c.region, "-r", c.fa, "-o", str(out), "--tmp-format", "counts"]
    return subprocess.run(cmd, capture_output=True, text=True, env=clean_env(dict(env or {}, BVC_HOST_PROFILE="1")), timeout=TIMEOUT)


def halves_then_all(exe, d, c, tag, thread, region=None):
    lines = [l for l in open(c.list).read().split("\n") if l]
    k = len(lines) // 2
    r = cohort_run(exe, c.list, c, d / (tag + "_plain"), thread, region=region)
    assert r.returncode == 0, r.stderr[-1000:]
    files = []
    for name, part in (("lo", lines[:k]), ("hi", lines[k:])):
        lst = d / f"{tag}_{name}.list"
        lst.write_text("".join(l + "\n" for l in part))
        files.append(str(d / f"{tag}_{name}.counts"))
        r = cohort_run(exe, str(lst), c, d / f"{tag}_{name}", thread, {"BVC_HOST_COUNTS_SAVE": files[-1]}, region)
        assert r.returncode == 0 and not glob.glob(str(d / f"{tag}_{name}") + ".*.gz"), r.stderr[-1000:]
    r = cohort_run(exe, c.list, c, d / (tag + "_all"), thread, {"BVC_HOST_COUNTS_LOAD": ":".join(files)}, region)
    assert r.returncode == 0, r.stderr[-1000:]
    line = files_line(r)
    assert line["piled"] == 0 and line["skipped"] == len(lines)          # (no batch is opened in pass 1: the names the outputs need come from the files)
    want, got = inflated(d / (tag + "_plain")), inflated(d / (tag + "_all"))
    for key in want:
        assert want[key] == got[key], key
    return want, r


@pytest.mark.parametrize("thread", [1, 3])
@pytest.mark.parametrize("name", ["rule", "calls"])
def test_a_cohorts_halves_saved_and_loaded(cohorts, tmp_path, name, thread):
    exe, _, made = cohorts
    want, _ = halves_then_all(exe, tmp_path, made[name], name, thread)
    assert want[".cvg.gz"].count(b"\n") > 500


QUIET = "chrS:33020-33090"      # (70 positions as the program cuts a region) of `rule`: the tiled samples' reads alone, copies of the reference -- no call, no indel entry (the SNPs are 33100 and 33200)


def test_without_a_revisited_position_the_names_come_from_the_files_alone(cohorts, tmp_path):
    """`rule` cut to a region without calls or indels: pass 2 piles nothing up, no batch is opened at all, and the sample names of the VCF
    header come from the files' BAM lists."""
    exe, _, made = cohorts
    c = made["rule"]
    assert cc.REGION.split(":")[0] == "chrS" and not any(33020 <= p <= 33090 for p in cc.RULE_SNPS)
    for thread in (1, 3):
        want, r = halves_then_all(exe, tmp_path, c, f"quiet{thread}", thread, region=QUIET)
        m = re.search(r"counts pass: (\d+) positions, (\d+) revisited", r.stderr)
        assert m and int(m.group(1)) == 70 and int(m.group(2)) == 0, r.stderr[-1000:]
        assert files_line(r)["piled"] == 0
        cvg = [l.split("\t") for l in want[".cvg.gz"].decode().split("\n") if l and l[0] != "#"]
        assert len(cvg) == 70 and all(int(row[3]) > 0 and row[8] == "." for row in cvg)                     # covered, and no indel
        assert not [l for l in want[".vcf.gz"].decode().split("\n") if l and l[0] != "#"]
        head = next(l for l in want[".vcf.gz"].decode().split("\n") if l.startswith("#CHROM"))
        assert set(c.names) <= set(head.split("\t")) and len(head.split("\t")) >= 9 + len(c.names)
