"""The host program with phase 1 on the device for the text temp batches (BVC_HOST_DEVICE_PILEUP_TEXT=1: bvc_bam_pileup_text_bgzf; GPU)
against the same run with the knob at 0, on the 100 test BAMs with --tmp-format text: every temp batch, the .vcf.gz and the .cvg.gz
inflate to the same bytes and stderr carries the same warnings, for batches of 7 and 100 and 1 and 3 threads; with --tmp-format bin the
knob changes nothing."""
import os

import pytest

from tests.test_gpu_host import _run
from tests.test_gpu_host_bam import device_batches, inflated

pytestmark = pytest.mark.gpu

ON = dict(BVC_HOST_DEVICE_PILEUP_TEXT="1", BVC_HOST_PROFILE="1")
OFF = dict(BVC_HOST_DEVICE_PILEUP_TEXT="0", BVC_HOST_PROFILE="1")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_bam_text")
    exe, _ = b.build_host()
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), dir=d)


def warnings(stderr):
    return sorted(l for l in stderr.split("\n") if l.startswith("warning"))


@pytest.mark.parametrize("thread", [1, 3])
@pytest.mark.parametrize("batch", [7, 100])
def test_the_device_load_phase_writes_the_text_batches_the_cpu_load_phase_writes(tmp_path, inputs, batch, thread):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = ["--tmp-format", "text", "--keep_tmp"]
    cpu, dev = str(tmp_path / "cpu"), str(tmp_path / "dev")
    r0 = _run(exe, cpu, lst, fa, extra, dict(os.environ, **OFF), thread=thread, batch=batch)
    r1 = _run(exe, dev, lst, fa, extra, dict(os.environ, **ON), thread=thread, batch=batch)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    n_batches = 1 + (100 - 1) // batch
    assert device_batches(r0.stderr) == 0 and device_batches(r1.stderr) == n_batches, r1.stderr[-2000:]
    assert "bvc_bam_pileup_text_bgzf" in r1.stderr and "extracted on the CPU" not in r1.stderr
    assert warnings(r0.stderr) == warnings(r1.stderr)
    want, got = inflated(cpu, thread), inflated(dev, thread)
    assert len(want) == 2 + thread * n_batches and set(want) == set(got)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30
    # text batches they are: the names line, then a line a position
    first = want[".tmp.thread.0/batch.0"]
    assert first.split(b"\n", 1)[0].count(b"\t") == min(batch, 100) and not first.startswith(b"BVCBAT1")


def test_the_binary_form_ignores_the_knob(tmp_path, inputs):
    out = {}
    for name, env in (("off", OFF), ("on", ON)):
        r = _run(inputs["exe"], str(tmp_path / name), inputs["lst"], inputs["fa"], ["--tmp-format", "bin", "--load", "--keep_tmp"], dict(os.environ, **env),
                 thread=1, batch=100)
        assert r.returncode == 0 and device_batches(r.stderr) == 0, r.stderr[-1000:]
        out[name] = open(str(tmp_path / name) + ".tmp.thread.0/batch.0", "rb").read()
    assert out["on"] == out["off"] and len(out["on"]) > 1000
