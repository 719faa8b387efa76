"""The host program with --tmp-format counts (phase 1 added into class counts: bvc_bam_counts_bgzf_acc, bvc_site_acc_lrt; only the called
positions, those with indel entries and their predecessors piled up a second time; GPU) against the same run with --tmp-format bin, on the
100 test BAMs: the .vcf.gz and the .cvg.gz inflate to the same bytes for 1 and 4 threads, batches of 7 and 100, with the sample columns
deflated on the host and on the device; nothing but the two outputs is on disk; the same "is empty" lines; the profile line's revisit set
is small; --rerun is ignored and said so; --group, --load, --keep_tmp and --gpus above 1 are refused; a budget the class counts do not fit
ends the run with a line that names --tmp-format bin and leaves no file."""
import glob
import gzip
import os
import re

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_counts")
    exe, _ = b.build_host()
    gf = d / "groups.txt"
    gf.write_text("S1 EAS\n")
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), groups=str(gf))


def inflated(prefix):
    return {k: gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}


@pytest.mark.parametrize("deflate", ["0", "1"])
@pytest.mark.parametrize("batch", [7, 100])
@pytest.mark.parametrize("thread", [1, 4])
def test_the_outputs_are_those_of_the_binary_temp_batches(tmp_path, inputs, thread, batch, deflate):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = dict(os.environ, BVC_HOST_DEVICE_DEFLATE=deflate, BVC_HOST_PROFILE="1", BVC_HOST_STORE_WINDOWS="3")     # (the windows' knob is mem's: ignored)
    want_p, got_p = str(tmp_path / "bin"), str(tmp_path / "counts")
    r0 = _run(exe, want_p, lst, fa, ["--tmp-format", "bin"], env, thread=thread, batch=batch)
    r1 = _run(exe, got_p, lst, fa, ["--tmp-format", "counts"], env, thread=thread, batch=batch)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(want_p), inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    assert want[".vcf.gz"].count(b"\n") > 30 and want[".cvg.gz"].count(b"\n") > 60000
    # the same warnings of phase 1, once each, and nothing but the two outputs on disk: no temp directory, no sub-file
    assert sorted(l for l in r0.stderr.split("\n") if "is empty." in l) == sorted(l for l in r1.stderr.split("\n") if "is empty." in l)
    assert sorted(os.path.basename(f) for f in glob.glob(got_p + "*")) == ["counts.cvg.gz", "counts.vcf.gz"]
    assert r1.stdout.count("basetype loading done") == 1
    # the revisit set: every called position is in it, and it is a small part of the region -- a run that revisited everything would
    # pass the comparison above too
    m = re.search(r"\[profile\] main: counts pass: (\d+) positions, (\d+) revisited \((\d+) called, (\d+) with indel entries, (\d+) for the carry\), "
                  r"accumulator (\d+) bytes, store (\d+) bytes", r1.stderr)
    assert m, r1.stderr[-2000:]
    P, S, called, indel, carry, acc_bytes, store_bytes = (int(x) for x in m.groups())
    assert P == 66615 and 76 <= S <= P // 10, (P, S)
    assert called == 76 and indel == 45 and 0 < carry <= 45 and S <= called + indel + carry
    assert acc_bytes == P * (2048 + 48) and 0 < store_bytes < acc_bytes


def test_rerun_is_ignored_and_said_so_once(tmp_path, inputs):
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts", "--rerun"], thread=2, batch=25)
    assert r.returncode == 0 and r.stderr.count("--rerun has nothing to reuse with --tmp-format counts") == 1, r.stderr[-1000:]
    assert sorted(os.path.basename(f) for f in glob.glob(out + "*")) == ["counts.cvg.gz", "counts.vcf.gz"]


@pytest.mark.parametrize("extra, line", [(["--load"], "--tmp-format counts with --load"), (["--keep_tmp"], "--tmp-format counts with --keep_tmp"),
                                         (["--gpus", "2"], "--tmp-format counts with --gpus above 1"), (["--group", "GROUPS"], "--tmp-format mem")])
def test_the_refusals_of_the_options(tmp_path, inputs, extra, line):
    out = str(tmp_path / "counts")
    extra = [inputs["groups"] if x == "GROUPS" else x for x in extra]
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"] + extra)
    assert r.returncode == 1 and r.stderr.count("\n") == 1 and line in r.stderr and "--tmp-format counts with" in r.stderr, r.stderr[-1000:]
    assert glob.glob(out + "*") == []


def test_class_counts_over_the_budget_name_the_way_out(tmp_path, inputs):
    """BVC_HOST_STORE_GB counts GB and takes a fraction: 1e-6 GB is about a kilobyte, which the class counts of no region fit; a budget of
    1 GB holds them, and afterwards the second pile-up's batches."""
    out = str(tmp_path / "counts")
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], dict(os.environ, BVC_HOST_STORE_GB="0.000001"), thread=2, batch=25)
    lines = [l for l in r.stderr.split("\n") if "--tmp-format bin" in l]
    assert r.returncode == 1 and len(lines) == 1 and "BVC_HOST_STORE_GB allows 1073" in lines[0] and str(66615 * 2096) in lines[0], r.stderr[-1000:]
    assert glob.glob(out + "*") == []
    r = _run(inputs["exe"], out, inputs["lst"], inputs["fa"], ["--tmp-format", "counts"], dict(os.environ, BVC_HOST_STORE_GB="1", BVC_HOST_PROFILE="1"),
             thread=2, batch=25)
    assert r.returncode == 0 and "counts pass: 66615 positions" in r.stderr, r.stderr[-1000:]
