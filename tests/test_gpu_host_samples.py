"""The host program with the called positions' sample columns formatted on the device (BVC_HOST_DEVICE_SAMPLES=1:
bvc_pileup_finish_called_text + bvc_pileup_sample_text, no entry of a device-parsed tile comes to the CPU) and on the CPU (=0, vcf_line's
sample loop): `BaseVarC basetype` on the reference's 100 test BAMs writes the same VCF and CVG, byte for byte, either way -- text, `bin`
and `raw` batches, with and without `--group`, one thread and three, tiles of 1 and 37 positions and the default.  With the knob on and
the CPU parser (BVC_HOST_DEVICE_PARSE=0) nothing changes either: the knob acts on device-parsed tiles only."""
import gzip
import os
import re

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


def _outputs(prefix):
    return [gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")]


def _tiles(stderr):
    return tuple(sum(int(x) for x in re.findall(pat + r" (\d+)", stderr))
                 for pat in ("parsed on the device", "statistics from the device", "sample columns from the device"))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_samples")
    exe, _ = b.build_host()
    fa = hostref.write_fasta(str(d / "chr17.fa"))
    lst = hostref.write_bam_list(str(d / "bam.list"))
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))
    return dict(exe=exe, fa=fa, lst=lst, groups=str(gf))


@pytest.mark.parametrize("fmt,grouped,thread,tile,cpu_parser_too", [
    ("text", False, 1, 0, True), ("text", True, 3, 37, False), ("text", False, 3, 1, False),
    ("bin", True, 1, 0, True), ("bin", False, 3, 37, False),
    ("raw", True, 3, 1, False), ("raw", False, 1, 0, False)])
def test_device_sample_columns_write_what_host_sample_columns_write(tmp_path, inputs, fmt, grouped, thread, tile, cpu_parser_too):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = (["--tmp-format", fmt] if fmt != "text" else []) + (["-g", inputs["groups"]] if grouped else []) + ["--keep_tmp"]
    out = str(tmp_path / "out")
    r = _run(exe, out, lst, fa, extra, dict(os.environ, BVC_HOST_DEVICE_SAMPLES="0", BVC_HOST_PROFILE="1"), thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, _, with_text = _tiles(r.stderr)
    assert dev > 0 and with_text == 0, r.stderr[-2000:]
    want = _outputs(out)
    assert sum(1 for l in want[0].split(b"\n") if l and l[:1] != b"#") == 76
    on = dict(os.environ, BVC_HOST_DEVICE_SAMPLES="1", BVC_HOST_PROFILE="1")
    r = _run(exe, out, lst, fa, extra + ["--rerun"] + (["--tile", str(tile)] if tile else []), on, thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, with_stats, with_text = _tiles(r.stderr)
    assert dev > 0 and with_text == dev and with_stats == dev, r.stderr[-2000:]   # every device-parsed tile; the knob implies the statistics
    got = _outputs(out)
    assert got[0] == want[0] and got[1] == want[1]
    # the columns are not trivial here: called positions carry covered samples of both kinds
    body = [l for l in want[0].split(b"\n") if l and l[:1] != b"#"]
    assert any(b"\t0/.:" in l and b"\t./1:" in l and b"\t./.\t" in l for l in body)
    if cpu_parser_too:
        r = _run(exe, out, lst, fa, extra + ["--rerun"], dict(on, BVC_HOST_DEVICE_PARSE="0"), thread=thread)
        assert r.returncode == 0, r.stderr[-2000:]
        assert _tiles(r.stderr) == (0, 0, 0), r.stderr[-2000:]
        got = _outputs(out)
        assert got[0] == want[0] and got[1] == want[1]
