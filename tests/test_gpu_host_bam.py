"""The host program with phase 1 on the device (BVC_HOST_DEVICE_PILEUP=1: bvc_bam_pileup_bgzf; GPU) against the same run with the knob at
0, on the 100 test BAMs: every temp batch, the .vcf.gz and the .cvg.gz inflate to the same bytes, for --tmp-format bin and raw, batches of
7 and 100, 1 and 4 threads; a BAM cut mid-record ends both runs with the same message and exit code 1; a sample whose region is empty
prints the warning in both."""
import glob
import gzip
import os
import re
import shutil

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu

ON = dict(BVC_HOST_DEVICE_PILEUP="1", BVC_HOST_PROFILE="1")
OFF = dict(BVC_HOST_DEVICE_PILEUP="0", BVC_HOST_PROFILE="1")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_bam")
    exe, _ = b.build_host()
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), dir=d)


def device_batches(stderr):
    m = re.search(r"load phase on the device, (\d+) batches", stderr)
    return int(m.group(1)) if m else 0


def inflated(prefix, thread):
    out = {k: gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}
    for t in range(thread):
        for f in sorted(glob.glob(f"{prefix}.tmp.thread.{t}/batch.*")):
            out[f[len(prefix):]] = gzip.decompress(open(f, "rb").read())
    return out


@pytest.mark.parametrize("thread", [1, 4])
@pytest.mark.parametrize("batch", [7, 100])
@pytest.mark.parametrize("fmt", ["bin", "raw"])
def test_the_device_load_phase_writes_what_the_cpu_load_phase_writes(tmp_path, inputs, fmt, batch, thread):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = ["--tmp-format", fmt, "--keep_tmp"]
    cpu, dev = str(tmp_path / "cpu"), str(tmp_path / "dev")
    r0 = _run(exe, cpu, lst, fa, extra, dict(os.environ, **OFF), thread=thread, batch=batch)
    r1 = _run(exe, dev, lst, fa, extra, dict(os.environ, **ON), thread=thread, batch=batch)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    n_batches = 1 + (100 - 1) // batch
    assert device_batches(r0.stderr) == 0 and device_batches(r1.stderr) == n_batches, r1.stderr[-2000:]
    want, got = inflated(cpu, thread), inflated(dev, thread)
    assert len(want) == 2 + thread * n_batches and set(want) == set(got)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30


def test_the_text_form_ignores_the_knob(tmp_path, inputs):
    r = _run(inputs["exe"], str(tmp_path / "t"), inputs["lst"], inputs["fa"], ["--load"], dict(os.environ, **ON), thread=1, batch=100)
    assert r.returncode == 0 and device_batches(r.stderr) == 0


def test_a_bam_cut_mid_record_and_an_empty_region(tmp_path, inputs):
    """Three samples: a whole BAM, one whose file ends inside a record (its last BGZF blocks dropped and the rest re-blocked so that the
    stream still frames), and -- in a second run -- the whole BAMs with a region no read of them reaches."""
    from tools.host_bench import _bgzf_write
    paths = [l.strip() for l in open(inputs["lst"]) if l.strip()][:3]
    d = tmp_path / "bams"
    d.mkdir()
    local = []
    for i, p in enumerate(paths):
        q = str(d / os.path.basename(p))
        if i == 1:
            data = gzip.open(p).read()
            open(q + ".cut", "wb").write(data[:len(data) - 37])      # ends inside its last record; no index beside it
            _bgzf_write(q + ".cut", q)
        else:
            shutil.copy(p, q)
            shutil.copy(p + ".bai", q + ".bai")
        local.append(q)
    lst = str(tmp_path / "cut.list")
    open(lst, "w").write("".join(q + "\n" for q in local))
    msgs = []
    for env in (OFF, ON):
        r = _run(inputs["exe"], str(tmp_path / f"cut{env['BVC_HOST_DEVICE_PILEUP']}"), lst, inputs["fa"], ["--tmp-format", "bin", "--load"],
                 dict(os.environ, **env), thread=1, batch=3)
        assert r.returncode == 1, r.stderr[-1000:]
        msgs.append([l for l in r.stderr.split("\n") if "truncated or corrupt BAM record" in l])
    assert msgs[0] and msgs[0] == msgs[1], msgs
    # a region of the same contig that the test BAMs hold no read of: the warning for every sample, from both paths
    lst2 = str(tmp_path / "whole.list")
    open(lst2, "w").write("".join(p + "\n" for p in paths))
    warn = []
    for env in (OFF, ON):
        import subprocess
        r = subprocess.run([inputs["exe"], "basetype", "--load", "--tmp-format", "raw", "-q", "20", "-t", "1", "-b", "3", "-i", lst2, "-s",
                            "chr17:41190000-41190050", "-r", inputs["fa"], "-o", str(tmp_path / f"empty{env['BVC_HOST_DEVICE_PILEUP']}")],
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-1000:]
        warn.append(sorted(l for l in r.stderr.split("\n") if "is empty." in l))
    assert len(warn[0]) == 3 and warn[0] == warn[1], warn
