"""The host program's matrix of paths on generated cohorts (GPU): `BaseVarC basetype` with every --tmp-format, every feed knob, position
windows and --group, on the cohorts of tests/cohort_cases.py -- `rule` for phase 1 (the fetch, its filters, the per-position rule, block
layouts, empty samples) and `calls` for stage 2 and the VCF line (multi-allelic sites, qualities up to 93, rank sums, strand skew, indel
tokens beside called positions) -- against the Python pipeline (tests/hostref.Pipeline with the cohort).

Per configuration and cohort one test of two host runs, -t 1 and -t 3, both with -b 7.  Each run must exit 0, write a .cvg.gz that inflates
to the pipeline's bytes and a .vcf.gz that equals the pipeline's line for line but for float fields within hostref.compare_vcf's bars,
inflate to exactly the bytes of the `text` run of the same cohort, -t and groups, print the pipeline's "is empty." lines and leave
nothing but the two outputs on disk.  The windows tests hold (mem, -t T, K windows) to (bin, -t T*K) byte for byte on both cohorts; `rule`
plants the reads that tell a window's own start from the region's as the read filter (tests/test_cohort_cases.py shows it with the
model).  A third cohort holds samples that end the run: exit 1, the CPU path's message, no output file."""
import glob
import gzip
import os
import subprocess
import time

import pytest

from tests import cohort_cases as cc
from tests import hostref

pytestmark = pytest.mark.gpu

BATCH = 7
THREADS = (1, 3)
TIMEOUT = 120

P = "BVC_HOST_DEVICE_"
TEXT_PILEUP = {P + "PILEUP_TEXT": "1"}
TEXT_PILEUP_DEFLATE = dict(TEXT_PILEUP, **{P + "PILEUP_DEFLATE": "1"})
BIN_PILEUP = {P + "PILEUP": "1"}
BIN_PILEUP_DEFLATE = dict(BIN_PILEUP, **{P + "PILEUP_DEFLATE": "1"})
DEFLATE = {P + "DEFLATE": "1"}
# name: (--tmp-format, environment, with --group)
CONFIGS = {
    "text": ("text", {}, False),
    "text, cpu parse": ("text", {P + "PARSE": "0"}, False),
    "text, cpu inflate": ("text", {P + "INFLATE": "0"}, False),
    "text, device pileup": ("text", TEXT_PILEUP, False),
    "text, device pileup, deflate": ("text", TEXT_PILEUP_DEFLATE, False),
    "text, device pileup, deflate, tokens": ("text", dict(TEXT_PILEUP_DEFLATE, **{P + "PILEUP_DEFLATE_TOKENS": "1"}), False),
    "bin": ("bin", {}, False),
    "bin, device pileup": ("bin", BIN_PILEUP, False),
    "bin, device pileup, deflate": ("bin", BIN_PILEUP_DEFLATE, False),
    "bin, device pileup, deflate, codes": ("bin", dict(BIN_PILEUP_DEFLATE, **{P + "PILEUP_DEFLATE_CODES": "1"}), False),
    "raw": ("raw", {}, False),
    "raw, device pileup": ("raw", BIN_PILEUP, False),
    "mem": ("mem", {}, False),
    "counts": ("counts", {}, False),
    "cpu stats": ("text", {P + "STATS": "0"}, False),
    "cpu samples": ("text", {P + "SAMPLES": "0"}, False),
    "every position's entries": ("text", {"BVC_HOST_CALLED_ONLY": "0"}, False),
    "device deflate": ("text", DEFLATE, False),
    "device deflate, codes, fields": ("text", dict(DEFLATE, **{P + "DEFLATE_CODES": "1", P + "DEFLATE_FIELDS": "1"}), False),
    "two-byte tiles": ("text", {"BVC_HOST_TWO_BYTE_TILES": "1"}, False),
    "two-byte tiles, cpu parse": ("text", {"BVC_HOST_TWO_BYTE_TILES": "1", P + "PARSE": "0"}, False),
    # --group on every form that takes it (counts refuses it), and on the CPU parser's dense group tiles
    "text, groups": ("text", {}, True),
    "text, cpu parse, groups": ("text", {P + "PARSE": "0"}, True),
    "two-byte tiles, cpu parse, groups": ("text", {"BVC_HOST_TWO_BYTE_TILES": "1", P + "PARSE": "0"}, True),
    "bin, groups": ("bin", {}, True),
    "bin, device pileup, groups": ("bin", BIN_PILEUP, True),
    "raw, groups": ("raw", {}, True),
    "mem, groups": ("mem", {}, True),
}
NO_BAI = ("text", "bin, device pileup", "mem")
COHORTS = ("rule", "calls")


def clean_env(extra=None):
    """The environment without any of the host program's knobs, then `extra`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BVC_HOST_")}
    env.update(extra or {})
    return env


class Runs:
    """The cohorts on disk (with .bai and without), the pipeline's outputs and the `text` runs, each made once"""

    def __init__(self, directory):
        from basevarc_amd import build as b
        self.exe, _ = b.build_host()
        self.dir = directory
        specs = {"rule": cc.rule_spec(), "calls": cc.calls_spec(), "fail": cc.fail_spec()}
        self.cohort = {(n, bai): cc.write_cohort(s, directory / f"{n}_{int(bai)}", bai=bai) for n, s in specs.items() for bai in (True, False)}
        self.groups = {}
        for n in COHORTS:
            c = self.cohort[(n, True)]
            self.groups[n] = cc.groups_of(c.names)
            (directory / f"{n}.groups").write_text("".join(f"{k} {v}\n" for k, v in self.groups[n].items()))
        self._want, self._text, self.slowest = {}, {}, (0.0, None)

    def want(self, name, thread, grouped):
        """(vcf text, cvg text, the empty samples' warning lines) of the Python pipeline"""
        key = (name, thread, grouped)
        if key not in self._want:
            c = self.cohort[(name, True)]
            pipe = hostref.Pipeline(mapq=cc.MAPQ, batch=BATCH, thread=thread, cohort=c)
            group_of = self.groups[name] if grouped else None
            vcf, cvg = pipe.outputs(group_of)
            vh, ch = hostref.headers(c.fa, pipe.names, sorted(set(group_of.values())) if grouped else (), cohort=c)
            self._want[key] = (vh + vcf, ch + cvg, sorted(f"warning: {n} region {c.region} is empty." for n in pipe.empty))
        return self._want[key]

    def host(self, name, out, thread, fmt="text", env=None, grouped=False, bai=True, what=None):
        """One run of the host program; the reference is always the indexed cohort's file, so that the header's ##reference line is one"""
        c = self.cohort[(name, True)]
        cmd = [self.exe, "basetype", "-q", str(cc.MAPQ), "-t", str(thread), "-b", str(BATCH), "-i", self.cohort[(name, bai)].list, "-s", c.region,
               "-r", c.fa, "-o", str(out)]
        cmd += ["--tmp-format", fmt] if fmt != "text" else []
        cmd += ["-g", str(self.dir / f"{name}.groups")] if grouped else []
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, env=clean_env(env), timeout=TIMEOUT)
        dt = time.time() - t0
        if dt > self.slowest[0]:
            self.slowest = (dt, (name, what or fmt, thread))
        print(f"host run {name} / {what or fmt} / -t {thread}: {dt:.2f} s (the slowest so far: {self.slowest[0]:.2f} s, {self.slowest[1]})")
        return r

    def text(self, name, thread, grouped):
        """The inflated outputs of the `text` run with default knobs"""
        key = (name, thread, grouped)
        if key not in self._text:
            out = self.dir / f"text_{name}_{thread}_{int(grouped)}"
            r = self.host(name, out, thread, grouped=grouped, what="text (the run the others are held to)")
            assert r.returncode == 0, r.stderr[-2000:]
            self._text[key] = inflated(str(out))
        return self._text[key]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("host_cohorts"))


def inflated(prefix):
    return {k: gzip.decompress(open(prefix + k, "rb").read()).decode() for k in (".vcf.gz", ".cvg.gz")}


def empty_lines(r):
    return sorted(l for l in r.stderr.split("\n") if "is empty." in l)


def on_disk(prefix):
    return sorted(os.path.basename(f) for f in glob.glob(str(prefix) + "*"))


def check_run(runs, r, out, name, thread, grouped):
    assert r.returncode == 0, r.stderr[-2000:]
    want_vcf, want_cvg, want_empty = runs.want(name, thread, grouped)
    got = inflated(str(out))
    assert got[".cvg.gz"] == want_cvg
    assert got[".vcf.gz"].split("\n")[:30] == want_vcf.split("\n")[:30]              # (the header, shown short when it differs)
    hostref.compare_vcf(got[".vcf.gz"], want_vcf)
    assert empty_lines(r) == want_empty
    base = os.path.basename(str(out))
    assert on_disk(out) == [base + ".cvg.gz", base + ".vcf.gz"]
    return got


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", COHORTS)
def test_a_configuration_writes_the_pipelines_outputs_and_the_text_runs_bytes(runs, tmp_path, name, config):
    fmt, env, grouped = CONFIGS[config]
    for thread in THREADS:
        out = tmp_path / f"t{thread}"
        r = runs.host(name, out, thread, fmt, env, grouped, what=config)
        got = check_run(runs, r, out, name, thread, grouped)
        text = runs.text(name, thread, grouped)
        for k in got:
            assert got[k] == text[k], (k, thread)
        # the cohort is not an empty run: lines in both outputs
        assert got[".cvg.gz"].count("\n") > 500 and sum(1 for l in got[".vcf.gz"].split("\n") if l and l[0] != "#") >= 12


@pytest.mark.parametrize("config", NO_BAI)
@pytest.mark.parametrize("name", COHORTS)
def test_without_the_index_the_outputs_are_the_same(runs, tmp_path, name, config):
    fmt, env, grouped = CONFIGS[config]
    assert not any(os.path.exists(b + ".bai") for b in runs.cohort[(name, False)].bams)
    for thread in THREADS:
        out = tmp_path / f"t{thread}"
        r = runs.host(name, out, thread, fmt, env, grouped, bai=False, what=config + ", no .bai")
        got = check_run(runs, r, out, name, thread, grouped)
        assert got == runs.text(name, thread, grouped), thread


@pytest.mark.parametrize("overlap", ["0", "1"])
@pytest.mark.parametrize("T, K", cc.WINDOWS)
@pytest.mark.parametrize("name", COHORTS)
def test_windows_write_the_bytes_of_the_binary_batches_with_t_times_k_threads(runs, tmp_path, name, T, K, overlap):
    """(mem, -t T, BVC_HOST_STORE_WINDOWS=K) against (bin, -t T*K), the specification of tests/test_gpu_host_mem_windows.py.  On `rule`
    this is the case that differed up to the fix of the windows' read filter: the planted reads end in front of a cut, lie between a
    read whose deletion covers the window's first positions and the next covering read, and were missing from the window's list."""
    want_p, got_p = tmp_path / "bin", tmp_path / "mem"
    r0 = runs.host(name, want_p, T * K, "bin", what="bin for the windows")
    r1 = runs.host(name, got_p, T, "mem", {"BVC_HOST_STORE_WINDOWS": str(K), "BVC_HOST_STORE_OVERLAP": overlap}, what=f"mem, {K} windows, overlap {overlap}")
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(str(want_p)), inflated(str(got_p))
    for k in want:
        if want[k] != got[k]:
            wl, gl = want[k].split("\n"), got[k].split("\n")
            first = next((i for i, (a, b) in enumerate(zip(wl, gl)) if a != b), min(len(wl), len(gl)))
            raise AssertionError((k, first, wl[first:first + 1], gl[first:first + 1]))
    assert empty_lines(r0) == empty_lines(r1) == runs.want(name, 1, False)[2]
    assert on_disk(got_p) == ["mem.cvg.gz", "mem.vcf.gz"]
    # and both are the pipeline's outputs for -t T*K
    check_run(runs, r0, want_p, name, T * K, False)


@pytest.mark.parametrize("config", ["text", "bin, device pileup", "mem", "counts"])
def test_a_failing_sample_ends_the_run_with_the_cpu_paths_message(runs, tmp_path, config):
    """Two of the three samples end find_snp_at_pos with std::out_of_range (cohort_cases.fail_spec): exit 1, the CPU path's line on stderr
    whichever path met the sample, and no output file -- no .vcf.gz or .cvg.gz, merged or a thread's (the temp batches of the forms that
    write files stay, as after any failed run, for --rerun)."""
    fmt, env, _ = CONFIGS[config]
    out = tmp_path / "fail"
    r = runs.host("fail", out, 1, fmt, env, what=config)
    assert r.returncode == 1, (r.returncode, r.stderr[-1000:])
    assert cc.FAIL_LINE in r.stderr, r.stderr[-1000:]
    assert [f for f in glob.glob(str(out) + "*") if f.endswith((".vcf.gz", ".cvg.gz"))] == []
    if fmt in ("mem", "counts"):
        assert glob.glob(str(out) + "*") == []
