"""The host program with --tmp-format mem in position windows (BVC_HOST_STORE_WINDOWS=K|auto, BVC_HOST_STORE_OVERLAP; GPU) on the 100 test
BAMs.  The specification is one sentence: the outputs of (mem, -t T, K windows) inflate to the bytes of (--tmp-format bin, -t T*K, the same
-b, -q, -g) -- window w is the ranges of threads wT .. wT+T-1 of a run with T*K threads, and its compute thread i works as thread wT+i of
it.  Also: the warnings are the bin run's, nothing but the two outputs is left on disk, K = 1 is the knob unset, windows without positions,
a budget that the whole region passes and a window fits, `auto` under that budget, and the next window loaded beside this one's threads."""
import glob
import os
import re

import pytest

from tests.test_gpu_host import _run
from tests.test_gpu_host_mem import inflated, inputs                     # noqa: F401  (the fixture's recipe)

pytestmark = pytest.mark.gpu

WINDOW_LINE = re.compile(r"\[profile\] main: window (\d+) of (\d+): positions \[(\d+), (\d+)\), fetch range \[(\d+), (\d+)\), (\d+) batches kept, (\d+) bytes, "
                         r"load ([0-9.e+-]+) s, compute ([0-9.e+-]+) s")
WHOLE_LINE = re.compile(r"batches kept there \(bvc_bam_pileup_bgzf_store\), (\d+) bytes")
LARGEST_LINE = re.compile(r"\[profile\] main: (\d+) windows, the largest store held (\d+) bytes")
ALIVE_LINE = re.compile(r"\[profile\] main: windows (\d+) and (\d+) alive together: (\d+) \+ (\d+) = (\d+) bytes \(budget (\d+)\)")


def empty_lines(r):
    return sorted(l for l in r.stderr.split("\n") if "is empty." in l)


def on_disk(prefix):
    return sorted(os.path.basename(f) for f in glob.glob(prefix + "*"))


def mem_against_bin(tmp_path, inputs, T, K, batch, extra=(), env=None, windows=None):
    """(mem, -t T, BVC_HOST_STORE_WINDOWS=windows or K) against (bin, -t T*K): returns the mem run"""
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = dict(os.environ, BVC_HOST_PROFILE="1", **(env or {}))
    want_p, got_p = str(tmp_path / "bin"), str(tmp_path / "mem")
    r0 = _run(exe, want_p, lst, fa, ["--tmp-format", "bin"] + list(extra), env, thread=T * K, batch=batch)
    r1 = _run(exe, got_p, lst, fa, ["--tmp-format", "mem"] + list(extra), dict(env, BVC_HOST_STORE_WINDOWS=str(windows or K)), thread=T, batch=batch)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    want, got = inflated(want_p), inflated(got_p)
    for k in want:
        assert want[k] == got[k], k
    assert empty_lines(r0) == empty_lines(r1)
    assert on_disk(got_p) == ["mem.cvg.gz", "mem.vcf.gz"]
    return r1, want


# (2, 61, 100): position 47214 of the list is where thread 86 of 122 starts, and its first entry is an indel entry, which inherits the
# parser's carry -- zeros at a range start.  A run that ignored the knob would differ from bin -t 122 there at the latest.
@pytest.mark.parametrize("T, K, batch, grouped, deflate", [(1, 2, 25, False, "0"), (1, 2, 25, True, "0"), (2, 3, 7, False, "0"), (2, 3, 7, True, "0"),
                                                          (2, 3, 7, False, "1"), (2, 3, 7, True, "1"), (4, 2, 100, False, "0"), (4, 2, 100, True, "0"),
                                                          (2, 61, 100, False, "0")])
def test_the_outputs_are_those_of_the_binary_temp_batches_with_t_times_k_threads(tmp_path, inputs, T, K, batch, grouped, deflate):
    r, want = mem_against_bin(tmp_path, inputs, T, K, batch, ["-g", inputs["groups"]] if grouped else [], dict(BVC_HOST_DEVICE_DEFLATE=deflate))
    assert want[".vcf.gz"].count(b"\n") > 30 and want[".cvg.gz"].count(b"\n") > 60000
    lines = WINDOW_LINE.findall(r.stderr)
    n_batches = 1 + (100 - 1) // batch
    assert [int(l[0]) for l in lines] == list(range(K)) and all(int(l[1]) == K and int(l[6]) == n_batches for l in lines), r.stderr[-2000:]
    # the windows follow each other through the position list and the fetch ranges through the region
    assert int(lines[0][2]) == 0 and all(lines[w][3] == lines[w + 1][2] and lines[w][5] == lines[w + 1][4] for w in range(K - 1))
    largest = LARGEST_LINE.search(r.stderr)
    assert largest and int(largest.group(1)) == K and int(largest.group(2)) == max(int(l[7]) for l in lines)
    assert "batches kept there" not in r.stderr                         # (the line of one window, K = 1)


def test_one_window_given_explicitly_is_the_knob_unset(tmp_path, inputs):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = {k: v for k, v in os.environ.items() if k not in ("BVC_HOST_STORE_WINDOWS", "BVC_HOST_PROFILE")}
    # (one thread: the progress lines of two compute threads are written piece by piece and end up inside each other)
    r0 = _run(exe, str(tmp_path / "unset"), lst, fa, ["--tmp-format", "mem"], env, thread=1, batch=25)
    r1 = _run(exe, str(tmp_path / "one"), lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_WINDOWS="1"), thread=1, batch=25)
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr[-1000:], r1.stderr[-1000:])
    assert sorted(r0.stderr.split("\n")) == sorted(r1.stderr.split("\n")) and "begin to load data and run basetype" in r0.stderr
    assert inflated(str(tmp_path / "unset")) == inflated(str(tmp_path / "one"))
    # and the knob is ignored, whatever it says, by the forms that write files
    r2 = _run(exe, str(tmp_path / "bin"), lst, fa, ["--tmp-format", "bin"], dict(env, BVC_HOST_STORE_WINDOWS="x"), thread=1, batch=25)
    assert r2.returncode == 0 and "BVC_HOST_STORE_WINDOWS" not in r2.stderr, r2.stderr[-1000:]
    assert inflated(str(tmp_path / "bin")) == inflated(str(tmp_path / "one"))


def test_more_windows_than_the_positions_fill(tmp_path, inputs):
    """A region of 3001 coordinates cut for 400 threads: the ranges are psize % 400 + psize // 400 positions long, so a few threads have
    some and most windows of four threads each have none -- no store is made for those, and their sub-files are those of bin -t 400's
    idle threads."""
    from tests import hostref
    r, want = mem_against_bin(tmp_path, inputs, 4, 100, 100, ["-s", "chr17:41197700-41200701"])
    lines = WINDOW_LINE.findall(r.stderr)
    psize = int(lines[-1][3])
    assert len(lines) == 100 and psize > 1000 and want[".cvg.gz"].count(b"\n") > 500
    ranges = [hostref.thread_window(psize, 400, j) for j in range(400)]
    assert [(int(l[2]), int(l[3])) for l in lines] == [(ranges[4 * w][0], ranges[4 * w + 3][1]) for w in range(100)]
    held = [int(l[3]) - int(l[2]) for l in lines]
    n_held = sum(1 for h in held if h > 0)
    assert 2 <= n_held < 100 and held[n_held:] == [0] * (100 - n_held), held[:8]
    assert all(int(l[6]) == 1 for l in lines[:n_held])
    assert all(int(l[6]) == 0 and int(l[7]) == 0 for l in lines[n_held:])          # no batch kept, no byte held


@pytest.fixture(scope="module")
def budget(tmp_path_factory, inputs):
    """Nothing is fixed in advance: the windows' bytes u_w (K = 4) and the whole store's U (K = 1) are read from the profile lines of two
    runs without a budget, and the budget lies half way between the largest window and the whole."""
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    d = tmp_path_factory.mktemp("budget")
    env = dict(os.environ, BVC_HOST_PROFILE="1")
    r4 = _run(exe, str(d / "k4"), lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_WINDOWS="4"), thread=2, batch=25)
    r1 = _run(exe, str(d / "k1"), lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_WINDOWS="1"), thread=2, batch=25)
    assert r4.returncode == 0 and r1.returncode == 0, (r4.stderr[-1000:], r1.stderr[-1000:])
    u = [int(l[7]) for l in WINDOW_LINE.findall(r4.stderr)]
    U = int(WHOLE_LINE.search(r1.stderr).group(1))
    assert len(u) == 4 and 0 < max(u) < U, (u, U)
    nbytes = (max(u) + U) // 2
    return dict(u=u, U=U, bytes=nbytes, gb=repr(nbytes / 1073741824.0))


def test_a_budget_that_the_region_passes_and_a_window_fits(tmp_path, inputs, budget):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = {k: v for k, v in os.environ.items() if k != "BVC_HOST_STORE_WINDOWS"}
    out = str(tmp_path / "mem")
    r = _run(exe, out, lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_GB=budget["gb"]), thread=2, batch=25)
    assert r.returncode == 1 and r.stderr.count("ERROR") == 1, r.stderr[-1000:]
    line = next(l for l in r.stderr.split("\n") if "ERROR" in l)
    proposed = re.search(r"BVC_HOST_STORE_WINDOWS=(\d+)", line)
    assert "--tmp-format bin" in line and proposed and int(proposed.group(1)) >= 2, line
    assert glob.glob(out + "*") == []
    r, _ = mem_against_bin(tmp_path, inputs, 2, 4, 25, env=dict(BVC_HOST_STORE_GB=budget["gb"]))
    largest = int(LARGEST_LINE.search(r.stderr).group(2))
    assert largest == max(budget["u"]) and largest < budget["bytes"], (largest, budget)
    # one window given explicitly: the line as it was, without a proposal
    r = _run(exe, out, lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_GB=budget["gb"], BVC_HOST_STORE_WINDOWS="1"), thread=2, batch=25)
    assert r.returncode == 1 and "--tmp-format bin" in r.stderr and "BVC_HOST_STORE_WINDOWS" not in r.stderr, r.stderr[-1000:]


def test_auto_finds_windows_that_fit_the_budget(tmp_path, inputs, budget):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    out = str(tmp_path / "auto")
    env = dict(os.environ, BVC_HOST_PROFILE="1", BVC_HOST_STORE_GB=budget["gb"], BVC_HOST_STORE_WINDOWS="auto")
    r = _run(exe, out, lst, fa, ["--tmp-format", "mem"], env, thread=2, batch=25)
    assert r.returncode == 0, r.stderr[-1000:]
    chose = re.search(r"\[profile\] main: BVC_HOST_STORE_WINDOWS=auto chose (\d+) windows", r.stderr)
    assert chose and int(chose.group(1)) >= 2, r.stderr[-2000:]
    K = int(chose.group(1))
    r0 = _run(exe, str(tmp_path / "bin"), lst, fa, ["--tmp-format", "bin"], None, thread=2 * K, batch=25)
    assert r0.returncode == 0 and inflated(str(tmp_path / "bin")) == inflated(out)
    assert int(LARGEST_LINE.search(r.stderr).group(2)) < budget["bytes"]
    # without a budget the device's free memory is one: these batches fit it whole
    r = _run(exe, out, lst, fa, ["--tmp-format", "mem"], dict(os.environ, BVC_HOST_PROFILE="1", BVC_HOST_STORE_WINDOWS="auto"), thread=2, batch=25)
    assert r.returncode == 0 and "BVC_HOST_STORE_WINDOWS=auto chose 1 windows" in r.stderr, r.stderr[-2000:]


def test_the_next_window_loaded_beside_this_ones_threads(tmp_path, inputs):
    exe, fa, lst = inputs["exe"], inputs["fa"], inputs["lst"]
    env = dict(os.environ, BVC_HOST_PROFILE="1", BVC_HOST_STORE_WINDOWS="3")
    one, two = str(tmp_path / "serial"), str(tmp_path / "overlap")
    r0 = _run(exe, one, lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_OVERLAP="0"), thread=2, batch=7)
    assert r0.returncode == 0 and not ALIVE_LINE.search(r0.stderr), r0.stderr[-1000:]
    u = [int(l[7]) for l in WINDOW_LINE.findall(r0.stderr)]
    # each of the two stores gets half of the budget: twice the largest window (and a page) lets every window in
    nbytes = 2 * max(u) + 8192
    r1 = _run(exe, two, lst, fa, ["--tmp-format", "mem"], dict(env, BVC_HOST_STORE_OVERLAP="1", BVC_HOST_STORE_GB=repr(nbytes / 1073741824.0)), thread=2, batch=7)
    assert r1.returncode == 0, r1.stderr[-1000:]
    assert inflated(one) == inflated(two) and empty_lines(r0) == empty_lines(r1)
    assert [int(l[7]) for l in WINDOW_LINE.findall(r1.stderr)] == u
    alive = [tuple(int(x) for x in m) for m in ALIVE_LINE.findall(r1.stderr)]
    assert [(m[0], m[1]) for m in alive] == [(0, 1), (1, 2)], r1.stderr[-2000:]
    for w0, w1, x, y, z, b in alive:
        assert (x, y) == (u[w0], u[w1]) and z == x + y and 0 < z <= nbytes and abs(b - nbytes) <= 1
    assert on_disk(two) == ["overlap.cvg.gz", "overlap.vcf.gz"]
