"""The host program with --tmp-format mem (phase 1's records stay on the device: bvc_bam_pileup_bgzf_store, bvc_pileup_begin_store; GPU)
against the same run with --tmp-format bin, on the 100 test BAMs: the .vcf.gz and the .cvg.gz inflate to the same bytes for 1 and 4
threads, batches of 7 and 100, with and without --group, with the sample columns deflated on the host and on the device; no temp directory
is ever made; --rerun is ignored and said so; a batch over BVC_HOST_STORE_GB ends the run with a line that names --tmp-format bin."""
import glob
import gzip
import os

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_mem")
    exe, _ = b.build_host()
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))      # 7 samples left ungrouped
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), groups=str(gf))


def inflated(prefix):
    return {k: gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}


@pytest.mark.parametrize("deflate", ["0", "1"])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("batch", [7, 100])
@pytest.mark.parametrize("thread", [1, 4])
def test_the_outputs_are_those_of_the_binary_temp_batches(tmp_path, inputs, thread, batch, grouped, deflate):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = dict(os.environ, BVC_HOST_DEVICE_DEFLATE=deflate, BVC_HOST_PROFILE="1")
    extra = ["-g", inputs["groups"]] if grouped else []
    want_p, got_p = str(tmp_path / "bin"), str(tmp_path / "mem")
    r0 = _run(exe, want_p, lst, fa, ["--tmp-format", "bin"] + extra, env, thread=thread, batch=batch)
    r1 = _run(exe, got_p, lst, fa, ["--tmp-format", "mem"] + extra, env, thread=thread, batch=batch)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    n_batches = 1 + (100 - 1) // batch
    assert f"load phase on the device, {n_batches} batches kept there" in r1.stderr, r1.stderr[-2000:]
    want, got = inflated(want_p), inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30 and want[".cvg.gz"].count(b"\n") > 60000
    # the same warnings of phase 1, and nothing but the two outputs on disk: no temp directory, no sub-file
    assert sorted(l for l in r0.stderr.split("\n") if "is empty." in l) == sorted(l for l in r1.stderr.split("\n") if "is empty." in l)
    assert sorted(os.path.basename(f) for f in glob.glob(got_p + "*")) == ["mem.cvg.gz", "mem.vcf.gz"]


def test_rerun_is_ignored_and_said_so_once(tmp_path, inputs):
    out = str(tmp_path / "mem")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "mem", "--rerun"], thread=2, batch=25)
    assert r.returncode == 0 and r.stderr.count("--rerun has nothing to reuse with --tmp-format mem") == 1, r.stderr[-1000:]
    assert sorted(os.path.basename(f) for f in glob.glob(out + "*")) == ["mem.cvg.gz", "mem.vcf.gz"]


@pytest.mark.parametrize("extra, line", [(["--load"], "--tmp-format mem with --load"), (["--keep_tmp"], "--tmp-format mem with --keep_tmp"),
                                         (["--gpus", "2"], "--tmp-format mem with --gpus above 1")])
def test_the_refusals_of_the_options(tmp_path, inputs, extra, line):
    out = str(tmp_path / "mem")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "mem"] + extra)
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and line in r.stderr, r.stderr[-1000:]
    assert glob.glob(out + "*") == []


def test_a_batch_over_the_budget_names_the_way_out(tmp_path, inputs):
    """BVC_HOST_STORE_GB counts GB and takes a fraction: 1e-6 GB is about a kilobyte, which no batch of the 100 test BAMs fits; a budget of
    1 GB holds them all and the run reports what it used."""
    out = str(tmp_path / "mem")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "mem"], dict(os.environ, BVC_HOST_STORE_GB="0.000001"), thread=2, batch=25)
    lines = [l for l in r.stderr.split("\n") if "--tmp-format bin" in l]
    assert r.returncode == 1 and len(lines) == 1 and "budget is 1073 bytes" in lines[0], r.stderr[-1000:]
    assert glob.glob(out + "*") == []
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "mem"], dict(os.environ, BVC_HOST_STORE_GB="1", BVC_HOST_PROFILE="1"),
             thread=2, batch=25)
    assert r.returncode == 0 and "4 batches kept there" in r.stderr, r.stderr[-1000:]
