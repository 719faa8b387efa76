"""The host program with the called positions' sample columns deflated on the device (BVC_HOST_DEVICE_DEFLATE=1:
bvc_pileup_sample_bgzf + BgzfWriter::write_blocks): `BaseVarC basetype` on the reference's 100 test BAMs writes a .vcf.gz that walks
clean as BGZF and inflates, as the .cvg.gz does, to the bytes of the run with the knob off.  The profile counts every device-parsed tile
as deflated on the device.  With the CPU parser, or without the device's sample columns, the knob changes nothing."""
import gzip
import os
import re

import pytest

from tests import bgzf_blocks as bb
from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


def _outputs(prefix):
    return [gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")]


def _tiles(stderr):
    return tuple(sum(int(x) for x in re.findall(pat + r" (\d+)", stderr))
                 for pat in ("parsed on the device", "sample columns from the device", "columns deflated on the device"))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_deflate")
    exe, _ = b.build_host()
    fa = hostref.write_fasta(str(d / "chr17.fa"))
    lst = hostref.write_bam_list(str(d / "bam.list"))
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))
    return dict(exe=exe, fa=fa, lst=lst, groups=str(gf))


@pytest.mark.parametrize("fmt,grouped,thread,tile,knob_off_too", [
    ("text", False, 1, 0, True), ("bin", True, 3, 37, False), ("raw", False, 3, 1, False)])
def test_device_deflated_columns_inflate_to_what_the_writer_deflates(tmp_path, inputs, fmt, grouped, thread, tile, knob_off_too):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = (["--tmp-format", fmt] if fmt != "text" else []) + (["-g", inputs["groups"]] if grouped else []) + ["--keep_tmp"]
    out = str(tmp_path / "out")
    r = _run(exe, out, lst, fa, extra, dict(os.environ, BVC_HOST_PROFILE="1"), thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, with_text, deflated = _tiles(r.stderr)
    assert dev > 0 and with_text == dev and deflated == 0, r.stderr[-2000:]          # the knob is off by default
    want = _outputs(out)
    raw_off = open(out + ".vcf.gz", "rb").read()
    assert sum(1 for l in want[0].split(b"\n") if l and l[:1] != b"#") == 76
    on = dict(os.environ, BVC_HOST_DEVICE_DEFLATE="1", BVC_HOST_PROFILE="1")
    r = _run(exe, out, lst, fa, extra + ["--rerun"] + (["--tile", str(tile)] if tile else []), on, thread=thread)
    assert r.returncode == 0, r.stderr[-2000:]
    dev, with_text, deflated = _tiles(r.stderr)
    assert dev > 0 and deflated == dev and with_text == dev, r.stderr[-2000:]
    raw = open(out + ".vcf.gz", "rb").read()
    blocks = bb.walk_file(raw)
    assert len(blocks) >= 2 * 76 and raw != raw_off                # a called position: the text in front of its columns, their blocks
    got = _outputs(out)
    assert got[0] == want[0] and got[1] == want[1]
    if knob_off_too:
        for off in ("BVC_HOST_DEVICE_PARSE", "BVC_HOST_DEVICE_SAMPLES"):
            r = _run(exe, out, lst, fa, extra + ["--rerun"], dict(on, **{off: "0"}), thread=thread)
            assert r.returncode == 0, r.stderr[-2000:]
            assert _tiles(r.stderr)[2] == 0, r.stderr[-2000:]
            assert open(out + ".vcf.gz", "rb").read() == raw_off and _outputs(out)[1] == want[1], off
