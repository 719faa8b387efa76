"""The host program on binary temp batches (`--tmp-format bin` and `raw`) with the records parsed on the DEVICE
(bvc_pileup_begin_bin): the same VCF and CVG, byte for byte, as the CPU feed of the same files (BVC_HOST_DEVICE_PARSE=0, the parser
parse_pileup_bin) and as the text form of the same run, whatever the tile size; a record that does not add up is an error."""
import gzip
import os
import re
import struct

import pytest

from tests.test_gpu_host import _run

pytestmark = pytest.mark.gpu


def _outputs(prefix):
    return [gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")]


def _counts(stderr):
    return (sum(int(x) for x in re.findall(r"parsed on the device (\d+)", stderr)),
            sum(int(x) for x in re.findall(r"handed back to the CPU parser (\d+)", stderr)))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_bin")
    exe, _ = b.build_host()
    fa = hostref.write_fasta(str(d / "chr17.fa"))
    lst = hostref.write_bam_list(str(d / "bam.list"))
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))
    text = {}
    for grouped in (False, True):                                # the text form of the same run: what every binary run must write
        out = str(d / f"text_{int(grouped)}")
        r = _run(exe, out, lst, fa, ["-g", str(gf)] if grouped else [])
        assert r.returncode == 0, r.stderr[-2000:]
        text[grouped] = _outputs(out)
        assert text[grouped][0].count(b"\n") > 30
    return dict(exe=exe, fa=fa, lst=lst, groups=str(gf), text=text)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("fmt", ["bin", "raw"])
def test_device_parsed_records_write_what_cpu_parsed_records_write(tmp_path, inputs, fmt, grouped):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = ["--tmp-format", fmt] + (["-g", inputs["groups"]] if grouped else [])
    base = str(tmp_path / "base")
    r = _run(exe, base, lst, fa, extra + ["--keep_tmp"], dict(os.environ, BVC_HOST_DEVICE_PARSE="0", BVC_HOST_PROFILE="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert _counts(r.stderr) == (0, 0), r.stderr[-2000:]
    want = _outputs(base)
    assert want == inputs["text"][grouped]
    for tile in (0, 37, 1):
        rr = _run(exe, base, lst, fa, extra + ["--keep_tmp", "--rerun"] + (["--tile", str(tile)] if tile else []),
                  dict(os.environ, BVC_HOST_DEVICE_PARSE="1", BVC_HOST_PROFILE="1"))
        assert rr.returncode == 0, rr.stderr[-2000:]
        dev, cpu = _counts(rr.stderr)
        assert _outputs(base) == want, (fmt, grouped, tile)
        assert dev > 0 and cpu == 0, (fmt, grouped, tile, dev, cpu)
    # tiles sized by bytes: many calls
    rr = _run(exe, base, lst, fa, extra + ["--keep_tmp", "--rerun"], dict(os.environ, BVC_HOST_DEVICE_PARSE="1", BVC_HOST_PROFILE="1", BVC_HOST_TILE_MB="1"))
    assert rr.returncode == 0 and _outputs(base) == want and _counts(rr.stderr)[0] > 0
    # the test hook that shifts qualities keeps forcing the CPU feed
    rr = _run(exe, base, lst, fa, extra + ["--keep_tmp", "--rerun"], dict(os.environ, BVC_HOST_DEVICE_PARSE="1", BVC_HOST_PROFILE="1", BVC_HOST_QUAL_SHIFT="1"))
    assert rr.returncode == 0 and _counts(rr.stderr) == (0, 0)


def test_a_record_whose_indel_overruns_its_payload_is_an_error(tmp_path, inputs):
    """One batch file rewritten with an indel length that runs past its record's payload (the record's length word kept consistent, so
    the stream still frames): exit code 1, `malformed temp batch` on stderr, the temp files kept -- with the device feed and with
    the CPU feed."""
    from tools.host_bench import _bgzf_write
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    extra = ["--tmp-format", "bin", "--keep_tmp"]
    out = str(tmp_path / "bad")
    r = _run(exe, out, lst, fa, extra + ["--load"])
    assert r.returncode == 0, r.stderr[-1000:]
    victim = f"{out}.tmp.thread.1/batch.2"
    raw = bytearray(gzip.decompress(open(victim, "rb").read()))
    assert raw[:8] == b"BVCBAT1\n"
    off = 16 + struct.unpack_from("<I", raw, 12)[0]
    hit = None
    while off < len(raw) and hit is None:                        # the first indel entry of the file
        (n,) = struct.unpack_from("<I", raw, off)
        p, end = off + 4, off + 4 + n
        while p < end:
            if raw[p + 8] & 2:
                hit = p
                break
            p += 9
        off = end
    assert hit is not None, "the victim batch has no indel entry"
    struct.pack_into("<H", raw, hit + 9, 60000)
    tmp = str(tmp_path / "bad.raw")
    open(tmp, "wb").write(bytes(raw))
    _bgzf_write(tmp, victim)
    for parse in ("1", "0"):
        r = _run(exe, out, lst, fa, extra + ["--rerun"], dict(os.environ, BVC_HOST_DEVICE_PARSE=parse))
        assert r.returncode == 1, (parse, r.returncode, r.stderr[-500:])
        assert "malformed temp batch" in r.stderr, (parse, r.stderr[-500:])
        assert os.path.exists(victim)
