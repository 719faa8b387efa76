"""`BaseVarC popmatrix` and `BaseVarC concat` (host/popmatrix.cpp, fetch_allele_type of host/bam.cpp; the CPU path, knob at 0) on the
100 test BAMs against the plain Python model of the reference's FetchAlleleType (tests/popmatrix_model.py): the matrix byte for byte for
a sorted and for an unsorted position file, two halves put together by concat, and the commands' errors.  No device."""
import gzip
import os
import subprocess

import pytest

from tests import hostref
from tests import popmatrix_model as pm
from tests.golden import make_testdata_pileup as tp

MAPQ = 20
CONTIG, START, END = tp.REGION


@pytest.fixture(scope="module")
def exe():
    from basevarc_amd import build as b
    return b.build_host()[0]


@pytest.fixture(scope="module")
def bams():
    """[(path, sample name, every read of the file on CONTIG that passes the flag and mapq filter)] in the list's order."""
    out = []
    for line in open(os.path.join(hostref.DATA, "bam.list")):
        if line.strip():
            path = os.path.join(hostref.DATA, line.strip().replace("data/", "", 1))
            header, recs = tp.read_bam(path)
            rv = [r for r in recs if r["ref"] == CONTIG and not (r["flag"] & 0x404) and r["cigar"] and r["mapq"] >= MAPQ]
            out.append((path, tp.sample_name(header), rv))
    return out


def model_matrix(bams, pv):
    """The file the reference writes for these lines: the region is first line + last line, split as splitrg splits it."""
    rg_s, rg_e = pv[0][0], pv[-1][0] - 1
    beg0, end0 = max(0, rg_s - 1 - 1000), rg_e + 1000
    refseq = "N" * max(0, rg_e + 1000 - rg_s + 1)
    rows = []
    for _, _, reads in bams:
        rv = [r for r in reads if tp.end_pos(r) > beg0 and r["pos"] < end0]
        rows.append(pm.fetch_allele_type(rv, pv, refseq, rg_s))
    return f"{len(bams)}\t{len(pv)}\n" + "".join(r + "\n" for r in rows)


@pytest.fixture(scope="module")
def sites(bams):
    """Lines made from the model's own coverage: every 7th position of the region that some sample covers, every 50th that nobody
    covers.  REF is the reference's base; on every third line REF and ALT change places (the covering reads then mostly say '1'), every
    fifth line asks for lowercase letters (nothing matches) and every 40th line stands twice with another ALT (a multi-allelic site)."""
    _, start, _, refseq = hostref.region_fixture()
    cov = {}
    for _, _, reads in bams:
        for r in reads:
            for p in range(r["pos"] + 1, tp.end_pos(r) + 1):
                cov[p] = cov.get(p, 0) + 1
    pv = []
    for p in range(START, END):
        ref = refseq[p - start]
        if ref not in "ACGT" or (p % 7 if p in cov else p % 50):
            continue
        n = len(pv)
        alt = "ACGT"[("ACGT".index(ref) + 1 + n % 3) % 4]
        if n % 3 == 1:
            ref, alt = alt, ref
        if n % 5 == 4:
            ref, alt = ref.lower(), alt.lower()
        pv.append((p, ref, alt))
        if n % 40 == 7:
            pv.append((p, ref, "N"))
    return pv


def write_posfile(path, pv, chrom=CONTIG):
    with open(path, "w") as f:
        for p, ref, alt in pv:
            f.write(f"{chrom}\t{p}\t{ref}\t{alt}\n")
    return path


def popmatrix(exe, out, lst, posfile, fa, extra=(), env=None):
    return subprocess.run([exe, "popmatrix", "-q", str(MAPQ), "-i", lst, "-p", posfile, "-r", fa, "-o", out, *extra], capture_output=True, text=True,
                          env=dict(os.environ, BVC_HOST_DEVICE_POPMATRIX="0") if env is None else env)


def inflated(path):
    return gzip.decompress(open(path, "rb").read()).decode()


@pytest.fixture(scope="module")
def whole(exe, bams, sites, tmp_path_factory):
    """The one-posfile run on the 100 BAMs: (directory, fasta, bam list, the output's text)."""
    d = tmp_path_factory.mktemp("popmatrix")
    fa, lst = hostref.write_fasta(str(d / "chr17.fa")), hostref.write_bam_list(str(d / "bam.list"))
    r = popmatrix(exe, str(d / "whole.gz"), lst, write_posfile(str(d / "sites.pos"), sites), fa)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "popmatrix start" in r.stderr and "popmatrix done" in r.stderr and "elapsed secs" in r.stdout
    return d, fa, lst, inflated(str(d / "whole.gz"))


def test_the_matrix_is_the_models_and_each_character_fills_its_share(whole, bams, sites):
    text = whole[3]
    want = model_matrix(bams, sites)
    assert text == want
    lines = text.split("\n")
    assert lines[0] == f"100\t{len(sites)}" and len(lines) == 102 and all(len(l) == len(sites) for l in lines[1:101])
    body = "".join(lines[1:])
    share = {ch: body.count(ch) / len(body) for ch in "01."}
    print("shares of the matrix:", share, "lines:", len(sites))
    # low-pass data: a covered site is covered by a few samples of the hundred, so most of the matrix is dots; of the lines, 8 in 15
    # ask for the reference's base as REF and 4 in 15 as ALT (the rest is lowercase), so '0' should fill about twice the share of '1'
    assert len(sites) > 1000 and len({p for p, _, _ in sites}) < len(sites)
    assert share["0"] > 0.002 and share["1"] > 0.001 and share["."] > 0.9 and body.count("0") > 500 and body.count("1") > 250, share


def test_an_unsorted_position_file_gets_the_stateful_answer(exe, whole, bams, sites):
    d, fa, lst, _ = whole
    inner = sites[1:-1]
    order = sorted(range(len(inner)), key=lambda i: (i * 7919) % len(inner))      # a fixed shuffle; the first and last line stay
    pv = [sites[0]] + [inner[i] for i in order] + [sites[-1]]
    assert any(a[0] > b[0] for a, b in zip(pv, pv[1:]))
    r = popmatrix(exe, str(d / "unsorted.gz"), lst, write_posfile(str(d / "unsorted.pos"), pv), fa)
    assert r.returncode == 0, r.stderr[-2000:]
    got = inflated(str(d / "unsorted.gz"))
    want = model_matrix(bams, pv)
    assert got == want
    # and it is not the sorted answer permuted: the cursor never goes back
    stateless = [pm.stateless_row([x for x in reads if tp.end_pos(x) > max(0, pv[0][0] - 1001) and x["pos"] < pv[-1][0] + 999], pv, "N" * (END - START + 1000), pv[0][0])
                 for _, _, reads in bams[:20]]
    assert stateless != want.split("\n")[1:21]


def test_two_halves_and_concat_are_the_whole(exe, whole, sites):
    d, fa, lst, text = whole
    half = len(sites) // 2
    outs = []
    for k, part in enumerate((sites[:half], sites[half:])):
        out = str(d / f"half{k}.gz")
        r = popmatrix(exe, out, lst, write_posfile(str(d / f"half{k}.pos"), part), fa)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    open(d / "halves.list", "w").write("".join(o + "\n" for o in outs))
    r = subprocess.run([exe, "concat", "-i", str(d / "halves.list"), "-o", str(d / "joined.gz")], capture_output=True, text=True)
    assert r.returncode == 0 and "concat done" in r.stdout, r.stderr[-2000:]
    joined = inflated(str(d / "joined.gz"))
    assert joined.split("\n")[0] == f"100\t{len(sites)}"
    # (a half's region is its own first and last line: the reads fetched differ, the characters do not)
    assert joined == text


def test_concat_refuses_files_that_disagree_or_run_out(exe, tmp_path):
    from tools.host_bench import _bgzf_write

    def matrix(name, n, m, rows):
        p = str(tmp_path / name)
        open(p + ".txt", "w").write(f"{n}\t{m}\n" + "".join(r + "\n" for r in rows))
        _bgzf_write(p + ".txt", p)
        return p
    a, b, c = matrix("a.gz", 2, 3, ["010", "1.0"]), matrix("b.gz", 3, 2, ["01", "10", ".."]), matrix("c.gz", 2, 2, ["01"])
    ok = matrix("ok.gz", 2, 1, ["1", "."])

    def concat(files):
        lst = str(tmp_path / "m.list")
        open(lst, "w").write("".join(f + "\n" for f in files))
        return subprocess.run([exe, "concat", "-i", lst, "-o", str(tmp_path / "out.gz")], capture_output=True, text=True)
    r = concat([a, b])
    assert r.returncode == 1 and "ERROR: the number of samples among the inputs are different!" in r.stderr
    r = concat([a, c])
    assert r.returncode == 1 and f"ERROR: empty in the 1 line of {c}" in r.stderr
    r = concat([a, ok])
    assert r.returncode == 0 and inflated(str(tmp_path / "out.gz")) == "2\t4\n0101\n1.0.\n"
    # an input that is not BGZF is refused by name, not read as an empty matrix
    with gzip.open(tmp_path / "plain.gz", "wb") as f:
        f.write(b"2\t1\n0\n1\n")
    r = concat([a, str(tmp_path / "plain.gz")])
    assert r.returncode == 1 and "plain.gz" in r.stderr


def test_the_commands_errors(exe, whole, bams, sites, tmp_path):
    from tools.host_bench import _bgzf_write
    d, fa, lst, _ = whole
    pos = str(d / "sites.pos")
    # no -p: the usage text, exit code 1
    r = subprocess.run([exe, "popmatrix", "-i", lst, "-r", fa, "-o", str(tmp_path / "x.gz")], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage   : BaseVarC popmatrix [options]" in r.stderr and "--posfile" in r.stderr
    r = subprocess.run([exe, "popmatrix", "-i", lst, "-p", pos, "-o", str(tmp_path / "x.gz")], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage   : BaseVarC popmatrix [options]" in r.stderr
    # a BAM whose header has no SM tag, behind a good one
    raw = gzip.open(bams[1][0]).read()
    assert raw.count(b"SM:") >= 1
    open(tmp_path / "nosm.raw", "wb").write(raw.replace(b"SM:", b"XM:"))
    _bgzf_write(str(tmp_path / "nosm.raw"), str(tmp_path / "nosm.bam"))
    open(tmp_path / "nosm.list", "w").write(bams[0][0] + "\n" + str(tmp_path / "nosm.bam") + "\n")
    r = popmatrix(exe, str(tmp_path / "nosm.gz"), str(tmp_path / "nosm.list"), pos, fa)
    assert r.returncode == 1 and "ERROR: No SM tag can be found. Please make sure there is SM tag in the bam header" in r.stderr
    # a contig the BAMs' headers do not have: the reference's line per sample on stderr, rows of dots
    with open(tmp_path / "q.fa", "w") as f:
        f.write(">chrQ\n" + "ACGT" * 500 + "\n")
    open(tmp_path / "q.fa.fai", "w").write("chrQ\t2000\t6\t2000\t2001\n")
    qpos = write_posfile(str(tmp_path / "q.pos"), [(10, "A", "C"), (20, "C", "G"), (50, "G", "T")], chrom="chrQ")
    open(tmp_path / "three.list", "w").write("".join(b[0] + "\n" for b in bams[:3]))
    r = popmatrix(exe, str(tmp_path / "q.gz"), str(tmp_path / "three.list"), qpos, str(tmp_path / "q.fa"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert [l for l in r.stderr.split("\n") if "is empty." in l] == [f"{b[1]}: region chrQ:10-50 is empty." for b in bams[:3]]
    assert inflated(str(tmp_path / "q.gz")) == "3\t3\n...\n...\n...\n"
