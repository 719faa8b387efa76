"""The host program with the called positions' rank-sum and strand statistics computed on the device (BVC_HOST_DEVICE_STATS=1,
bvc_pileup_finish_called_stats) and on the CPU (=0, vcf_line's own tallies and three sorts): `BaseVarC basetype` on the reference's 100
test BAMs writes the same VCF and CVG, byte for byte, either way -- text feed and `--tmp-format raw`, with and without `--group`, one
thread and three.  The 76 called positions carry real spreads of mapq, qual and rpr."""
import gzip
import os
import re

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


def _outputs(prefix):
    return [gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")]


def _tiles(stderr):
    return (sum(int(x) for x in re.findall(r"parsed on the device (\d+)", stderr)),
            sum(int(x) for x in re.findall(r"statistics from the device (\d+)", stderr)))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_stats")
    exe, _ = b.build_host()
    fa = hostref.write_fasta(str(d / "chr17.fa"))
    lst = hostref.write_bam_list(str(d / "bam.list"))
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))
    return dict(exe=exe, fa=fa, lst=lst, groups=str(gf))


@pytest.mark.parametrize("fmt,grouped,thread", [("text", False, 1), ("text", True, 3), ("raw", False, 3), ("raw", True, 1)])
def test_device_statistics_write_what_host_statistics_write(tmp_path, inputs, fmt, grouped, thread):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = (["--tmp-format", fmt] if fmt != "text" else []) + (["-g", inputs["groups"]] if grouped else []) + ["--keep_tmp"]
    out = str(tmp_path / "out")
    r = _run(exe, out, lst, fa, extra, dict(os.environ, BVC_HOST_DEVICE_STATS="0", BVC_HOST_PROFILE="1"), thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, with_stats = _tiles(r.stderr)
    assert dev > 0 and with_stats == 0, r.stderr[-2000:]
    want = _outputs(out)
    assert sum(1 for l in want[0].split(b"\n") if l and l[:1] != b"#") == 76
    r = _run(exe, out, lst, fa, extra + ["--rerun"], dict(os.environ, BVC_HOST_DEVICE_STATS="1", BVC_HOST_PROFILE="1"), thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, with_stats = _tiles(r.stderr)
    assert dev > 0 and with_stats == dev, r.stderr[-2000:]        # every device-parsed tile took the statistics from the device
    got = _outputs(out)
    assert got[0] == want[0] and got[1] == want[1]
    assert any(re.search(rb"MQRankSum=(?!0\.000|nan|10000)", l) for l in want[0].split(b"\n"))    # (the statistic is not trivial here)
