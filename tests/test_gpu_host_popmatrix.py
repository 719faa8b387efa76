"""`BaseVarC popmatrix` with the rows made on the device (BVC_HOST_DEVICE_POPMATRIX=1: bvc_bam_popmatrix_bgzf; GPU) against the same run
with the knob at 0 (the CPU path, which tests/test_popmatrix_host.py holds to the model) on the 100 test BAMs: the matrix inflates to the
same bytes for batches of 7 and 100; an unsorted position file takes the CPU path; a BAM cut mid-record ends both runs alike."""
import gzip
import os
import re
import shutil
import subprocess

import pytest

from tests import hostref
from tests import popmatrix_model as pm
from tests.golden import make_testdata_pileup as tp

pytestmark = pytest.mark.gpu

ON = dict(BVC_HOST_DEVICE_POPMATRIX="1", BVC_HOST_PROFILE="1")
OFF = dict(BVC_HOST_DEVICE_POPMATRIX="0", BVC_HOST_PROFILE="1")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    d = tmp_path_factory.mktemp("host_popmatrix")
    exe, _ = b.build_host()
    _, start, _, refseq = hostref.region_fixture()
    _, s, e = tp.REGION
    pv = pm.refalt([p for p in range(s, e, 10) if refseq[p - start] in "ACGT"], start, refseq)
    pv = [x for i, x in enumerate(pv) for _ in range(2 if i % 50 == 9 else 1)]          # some sites on two lines
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), dir=d, pv=pv)


def write_posfile(path, pv):
    with open(path, "w") as f:
        for p, ref, alt in pv:
            f.write(f"{tp.REGION[0]}\t{p}\t{ref}\t{alt}\n")
    return path


def run(inputs, out, posfile, env, lst=None, extra=()):
    return subprocess.run([inputs["exe"], "popmatrix", "-q", "20", "-i", lst or inputs["lst"], "-p", posfile, "-r", inputs["fa"], "-o", out, *extra],
                          capture_output=True, text=True, env=dict(os.environ, **env))


def device_batches(stderr):
    m = re.search(r"popmatrix on the device, (\d+) batches", stderr)
    return int(m.group(1)) if m else -1


def inflated(path):
    return gzip.decompress(open(path, "rb").read())


@pytest.fixture(scope="module")
def cpu(inputs):
    pos = write_posfile(str(inputs["dir"] / "sites.pos"), inputs["pv"])
    r = run(inputs, str(inputs["dir"] / "cpu.gz"), pos, OFF)
    assert r.returncode == 0 and device_batches(r.stderr) == 0, r.stderr[-2000:]
    text = inflated(str(inputs["dir"] / "cpu.gz"))
    assert text.count(b"0") > 1000 and text.count(b"1") > 500
    return pos, text


@pytest.mark.parametrize("batch", [7, 100, None])
def test_the_device_rows_are_the_cpu_rows(inputs, cpu, batch):
    pos, want = cpu
    out = str(inputs["dir"] / f"dev{batch}.gz")
    r = run(inputs, out, pos, ON, extra=() if batch is None else ("-b", str(batch)))
    assert r.returncode == 0, r.stderr[-2000:]
    assert device_batches(r.stderr) == 1 + (100 - 1) // (batch or 100), r.stderr[-2000:]
    assert inflated(out) == want


def test_an_unsorted_position_file_takes_the_cpu_path(inputs):
    pv = inputs["pv"]
    inner = pv[1:-1]
    order = sorted(range(len(inner)), key=lambda i: (i * 7919) % len(inner))
    pos = write_posfile(str(inputs["dir"] / "unsorted.pos"), [pv[0]] + [inner[i] for i in order] + [pv[-1]])
    outs = []
    for k, env in enumerate((OFF, ON)):
        out = str(inputs["dir"] / f"unsorted{k}.gz")
        r = run(inputs, out, pos, env)
        assert r.returncode == 0 and device_batches(r.stderr) == 0, r.stderr[-2000:]
        assert ("the position file is not sorted, the rows are made on the CPU" in r.stderr) == (env is ON)
        outs.append(inflated(out))
    assert outs[0] == outs[1] and outs[0].count(b"\n") == 101


def test_a_bam_cut_mid_record_ends_both_runs_alike(inputs, cpu, tmp_path):
    """Three samples, the second one's file ending inside its last record (re-blocked so that the stream still frames), as
    tests/test_gpu_host_bam.py cuts it."""
    from tools.host_bench import _bgzf_write
    paths = [l.strip() for l in open(inputs["lst"]) if l.strip()][:3]
    local = []
    for i, p in enumerate(paths):
        q = str(tmp_path / os.path.basename(p))
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
        r = run(inputs, str(tmp_path / f"cut{env['BVC_HOST_DEVICE_POPMATRIX']}.gz"), cpu[0], env, lst=lst)
        assert r.returncode == 1, r.stderr[-1000:]
        msgs.append([l for l in r.stderr.split("\n") if "truncated or corrupt BAM record" in l])
    assert msgs[0] and msgs[0] == msgs[1], msgs
