"""The host program with phase 1's temp batches deflated on the device (BVC_HOST_DEVICE_PILEUP_DEFLATE=1 beside BVC_HOST_DEVICE_PILEUP on
--tmp-format bin, beside BVC_HOST_DEVICE_PILEUP_TEXT on text: bvc_bam_pileup[_text]_bgzf_deflate; GPU), on the 100 test BAMs at 1 and 4
threads and batches of 7 and 100.  With the knob on -- alone, with _CODES, and for text with _TOKENS -- every batch file is a BGZF file
(tests/bgzf_blocks.py walks it: the end-of-file block last, no empty block before it) that inflates to the bytes it has with the knob off;
a later run with every knob off reuses the files (--rerun) and writes the same .vcf.gz and .cvg.gz, through the default BGZF feed, with
--group, and with BVC_HOST_DEVICE_INFLATE=0; raw and mem ignore the knob."""
import glob
import gzip
import os

import pytest

from tests import bgzf_blocks as bb
from tests.test_gpu_host import _run
from tests.test_gpu_host_bam import device_batches

pytestmark = pytest.mark.gpu

PILEUP = {"bin": "BVC_HOST_DEVICE_PILEUP", "text": "BVC_HOST_DEVICE_PILEUP_TEXT"}
CALL = {"bin": "bvc_bam_pileup_bgzf", "text": "bvc_bam_pileup_text_bgzf"}
# every knob of this path off, whatever the environment of the test run holds
ALL_OFF = dict(BVC_HOST_DEVICE_PILEUP="0", BVC_HOST_DEVICE_PILEUP_TEXT="0", BVC_HOST_DEVICE_PILEUP_DEFLATE="0", BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES="0",
               BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS="0", BVC_HOST_PROFILE="1")


def variants(fmt):
    """[(name, environment)] of the knob on: alone, with _CODES, and for text with _TOKENS (and with both)."""
    on = dict(ALL_OFF, **{PILEUP[fmt]: "1", "BVC_HOST_DEVICE_PILEUP_DEFLATE": "1"})
    out = [("alone", on), ("codes", dict(on, BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES="1"))]
    if fmt == "text":
        out += [("tokens", dict(on, BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS="1")),
                ("codes and tokens", dict(on, BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES="1", BVC_HOST_DEVICE_PILEUP_DEFLATE_TOKENS="1"))]
    return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from basevarc_amd import build as b
    from tests import hostref
    d = tmp_path_factory.mktemp("host_bam_deflate")
    exe, _ = b.build_host()
    names = hostref.Pipeline(mapq=20, batch=25, thread=1).names
    gf = d / "groups.txt"
    gf.write_text("".join(f"{n} {['EAS', 'AFR', 'EUR'][i % 3]}\n" for i, n in enumerate(names) if i % 14 != 5))
    return dict(exe=exe, fa=hostref.write_fasta(str(d / "chr17.fa")), lst=hostref.write_bam_list(str(d / "bam.list")), groups=str(gf))


def batch_files(prefix, thread):
    """{name behind the prefix: the file's bytes} of every temp batch."""
    return {f[len(prefix):]: open(f, "rb").read() for t in range(thread) for f in sorted(glob.glob(f"{prefix}.tmp.thread.{t}/batch.*"))}


def outputs(prefix):
    return {k: gzip.decompress(open(prefix + k, "rb").read()) for k in (".vcf.gz", ".cvg.gz")}


@pytest.mark.parametrize("thread", [1, 4])
@pytest.mark.parametrize("batch", [7, 100])
@pytest.mark.parametrize("fmt", ["bin", "text"])
def test_the_batch_files_inflate_to_the_same_bytes_and_a_run_with_every_knob_off_reuses_them(tmp_path, inputs, fmt, batch, thread):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    n_batches = 1 + (100 - 1) // batch
    base = ["--tmp-format", fmt, "--keep_tmp"]
    # the parent's device path: the pileup knob alone, a whole run
    off = str(tmp_path / "off")
    r = _run(exe, off, lst, fa, base, dict(os.environ, **dict(ALL_OFF, **{PILEUP[fmt]: "1"})), thread=thread, batch=batch)
    assert r.returncode == 0 and device_batches(r.stderr) == n_batches and f"({CALL[fmt]})" in r.stderr, r.stderr[-2000:]
    want = {k: gzip.decompress(v) for k, v in batch_files(off, thread).items()}
    want_out = outputs(off)
    assert len(want) == thread * n_batches and want_out[".vcf.gz"].count(b"\n") > 30
    sizes = {"level 6": sum(len(v) for v in batch_files(off, thread).values())}
    for name, env in variants(fmt):
        on = str(tmp_path / name.replace(" ", "_"))
        r = _run(exe, on, lst, fa, base + ["--load"], dict(os.environ, **env), thread=thread, batch=batch)
        assert r.returncode == 0 and device_batches(r.stderr) == n_batches and f"({CALL[fmt]}_deflate)" in r.stderr, r.stderr[-2000:]
        assert "extracted on the CPU" not in r.stderr
        got = batch_files(on, thread)
        assert set(got) == set(want)
        for k, raw in got.items():
            blocks = bb.walk_file(raw)                                      # the end-of-file block --rerun probes for, and no empty block before it
            assert b"".join(b[0] for b in blocks) == want[k] == gzip.decompress(raw), (name, k)
            # the names line (the binary header) is a block of its own: the device's blocks begin behind it
            head = want[k].split(b"\n", 1)[0] + b"\n" if fmt == "text" else None
            assert fmt != "text" or blocks[0][0] == head, (name, k)
        sizes[name] = sum(len(v) for v in got.values())
    print(f"{fmt}, {thread} threads, batches of {batch}: bytes of the batch files {sizes}")
    # the files of the last variant, read by a run with every knob off: nothing is extracted again, and the outputs are the same
    r = _run(exe, on, lst, fa, base + ["--rerun"], dict(os.environ, **ALL_OFF), thread=thread, batch=batch)
    assert r.returncode == 0 and "begin to extract reads from bam" not in r.stderr and device_batches(r.stderr) == 0, r.stderr[-2000:]
    assert outputs(on) == want_out
    assert {k: gzip.decompress(v) for k, v in batch_files(on, thread).items()} == want


@pytest.mark.parametrize("fmt", ["bin", "text"])
def test_the_other_feeds_and_group_read_the_files(tmp_path, inputs, fmt):
    """4 threads, batches of 7: the deflated files under --group, and (text) under BVC_HOST_DEVICE_INFLATE=0, the CPU's inflater."""
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    base = ["--tmp-format", fmt, "--keep_tmp"]
    grouped = ["-g", inputs["groups"]]
    name, env = variants(fmt)[-1]
    on = str(tmp_path / "on")
    r = _run(exe, on, lst, fa, base + ["--load"], dict(os.environ, **env), thread=4, batch=7)
    assert r.returncode == 0 and device_batches(r.stderr) == 15, r.stderr[-2000:]
    for label, extra, more in (("group", grouped, {}), ("host inflate", [], dict(BVC_HOST_DEVICE_INFLATE="0")),
                               ("cpu parser", [], dict(BVC_HOST_DEVICE_PARSE="0"))):
        off = str(tmp_path / ("off_" + label.replace(" ", "_")))
        r0 = _run(exe, off, lst, fa, ["--tmp-format", fmt] + extra, dict(os.environ, **dict(ALL_OFF, **more)), thread=4, batch=7)
        r1 = _run(exe, on, lst, fa, base + ["--rerun"] + extra, dict(os.environ, **dict(ALL_OFF, **more)), thread=4, batch=7)
        assert r0.returncode == 0 and r1.returncode == 0, (label, r0.stderr[-1000:], r1.stderr[-1000:])
        assert "begin to extract reads from bam" not in r1.stderr and outputs(on) == outputs(off), label


def test_raw_and_mem_ignore_the_knob(tmp_path, inputs):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    files = {}
    for name, deflate in (("off", "0"), ("on", "1")):
        env = dict(os.environ, **dict(ALL_OFF, BVC_HOST_DEVICE_PILEUP="1", BVC_HOST_DEVICE_PILEUP_DEFLATE=deflate, BVC_HOST_DEVICE_PILEUP_DEFLATE_CODES=deflate))
        r = _run(exe, str(tmp_path / name), lst, fa, ["--tmp-format", "raw", "--load", "--keep_tmp"], env, thread=2, batch=100)
        assert r.returncode == 0 and device_batches(r.stderr) == 1 and "(bvc_bam_pileup_bgzf)" in r.stderr, r.stderr[-1000:]
        files[name] = batch_files(str(tmp_path / name), 2)
        r = _run(exe, str(tmp_path / ("mem_" + name)), lst, fa, ["--tmp-format", "mem"], env, thread=2, batch=100)
        assert r.returncode == 0 and "1 batches kept there (bvc_bam_pileup_bgzf_store)" in r.stderr, r.stderr[-1000:]
    assert files["on"] == files["off"] and len(files["on"]) == 2             # stored blocks, byte for byte
    assert outputs(str(tmp_path / "mem_on")) == outputs(str(tmp_path / "mem_off"))
