"""The census of stage 1 (no GPU): which kernel instance of csrc/hist_kernel.hip every case of tests/hist_cases.py reaches.

hist_model.plan restates the launchers; the compiler's own list of instances comes from tools/isa_report.py.  Every counting instance
is either reached by a case or named in UNREACHABLE with the launcher's reason, which a loop over every k and every tuning proves.
tests/test_gpu_hist_cases.py runs the same catalogue on the device.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402
from tests import hist_cases as HC  # noqa: E402
from tests import hist_model as M  # noqa: E402

# Instances the compiler emits and no call can reach, with the launcher's reason (test_unreachable_is_proved).
UNREACHABLE = {
    "hist_dense_groups_kernel<5, true>": "plan_group_copies: 32 copies of two 512-class histograms (k = 1) are 128 KiB, twice kLdsWords",
    "hist_dense_groups_kernel<5, false>": "plan_group_copies: 32 copies of two 512-class histograms (k = 1) are 128 KiB, twice kLdsWords",
}


@pytest.fixture(scope="module")
def instances():
    """The counting kernels of hist_kernel.hip as the compiler emitted them."""
    rows = isa_report.kernels_of(isa_report.assembly("hist_kernel.hip"))
    return {k["pretty"] for k in rows} - set(M.NOT_COUNTING)


@pytest.fixture(scope="module")
def census():
    reached = {}
    for c in HC.CASES:
        for name in HC.plan_of(c):
            reached.setdefault(name, []).append(c.name)
    return reached


def test_plan_names_are_the_compilers(instances):
    # a new instance fails here until hist_model.plan can name it (and test_every_instance_is_reached until a case reaches it)
    assert M.all_names() == instances, (sorted(M.all_names() - instances), sorted(instances - M.all_names()))


def test_every_case_reaches_what_it_is_meant_to():
    bad = [(c.name, c.want, HC.plan_of(c)) for c in HC.CASES if tuple(HC.plan_of(c)) != c.want]
    assert not bad, bad


def test_every_instance_is_reached(instances, census, capsys):
    with capsys.disabled():
        print(f"\nstage-1 census: {len(HC.CASES)} cases, {len(instances)} instances")
        for name in sorted(instances):
            cases = census.get(name, [])
            shown = ", ".join(cases[:4]) + (f", ... ({len(cases)})" if len(cases) > 4 else "")
            print(f"  {name:46s} -> {shown if cases else 'UNREACHABLE: ' + UNREACHABLE.get(name, '?')}")
    assert set(census) <= instances
    assert instances - set(census) == set(UNREACHABLE), sorted(instances - set(census) ^ set(UNREACHABLE))


def every_group_plan():
    """plan of the group entries for every k, tuning, alignment and order of the labels (row length on either side of the H16 bound)."""
    for entry in M.GROUP_ENTRIES + M.PACKED_GROUP_ENTRIES:
        arrays = 1 if entry in M.PACKED_GROUP_ENTRIES else 2
        for k in range(1, M.MAX_GROUPS + 1):
            for tuning in M.all_tunings():
                for align in ((0,) * arrays, (1,) * arrays):
                    for ordered in (False, True):
                        for n in (1000, M.H16_MAX_SAMPLES + 16):
                            yield M.plan(entry, 7, n, n + 8, align, k, ordered, tuning, 256)


def test_unreachable_is_proved(instances):
    seen = set()
    for names in every_group_plan():
        seen.update(names)
    assert not seen & set(UNREACHABLE), sorted(seen & set(UNREACHABLE))
    # ... and the loop is wide enough to find every other instance of the group launchers
    group_instances = {n for n in instances if "groups" in n or "ranges" in n}
    assert group_instances - seen == set(UNREACHABLE), sorted(group_instances - seen)
    # the reason: the plan's copies for two-byte rows stop at 16 (k = 1), whatever the tuning
    assert max(M.plan_group_copies(t, k + 1, M.NCLASS, 16)[0] for k in range(1, 33) for t in M.all_tunings()) == 4
    assert M.plan_group_copies({}, 2, M.PACKED_SLOTS, 0)[0] == 5


def test_plan_steps():
    """The steps of plan_group_copies the catalogue sits on, worked by hand from kLdsWords = 16384 and kBigLdsBytes = 144 KiB."""
    two_byte = {k: M.plan_group_copies({}, k + 1, M.NCLASS, 16) for k in range(1, 33)}
    packed = {k: M.plan_group_copies({}, k + 1, M.PACKED_SLOTS, 0) for k in range(1, 33)}
    assert [two_byte[k][0] for k in (1, 2, 3, 4, 7, 8, 15, 16, 32)] == [4, 3, 3, 2, 2, 1, 1, 0, 0]
    assert [packed[k][0] for k in (1, 2, 3, 4, 7, 8, 15, 16, 31, 32)] == [5, 4, 4, 3, 3, 2, 2, 1, 1, 0]
    # k = 8: sixteen copies of nine 256-slot histograms are 9 * 16384 bytes = 144 KiB exactly; the two-byte form's 16-byte tail does not fit
    assert packed[8][1] == 4 and two_byte[8][1] == 3 and two_byte[7][1] == 4
    assert [two_byte[k][1] for k in (16, 17, 32)] == [3, 2, 2] and [packed[k][1] for k in (17, 18, 32)] == [3, 2, 2]
    assert M.choose_hist_split({}, 3, 65536, 256) == 2 and M.choose_hist_split({}, 3, 65535, 256) == 1
    assert M.choose_hist_split({}, 1024, 1 << 20, 256) == 1 and M.choose_hist_split({}, 1, 1 << 22, 256) == 64
    assert M.choose_hist_split({"hist_split": 5}, 1, 1, 256) == 5


def test_edges_of_the_issue_are_in_the_catalogue():
    """Shapes the launchers and kernels treat specially, each checked on the case that is meant to hold it."""
    by = HC.by_name
    items = lambda c: M.work_items(c.entry, c.n_sites, c.n, c.k, HC.labels_of(c), dict(c.tuning), 256)  # noqa: E731
    for name in ("dense_4097_sites", "packed_4097_sites", "ranges_4097_items", "packed_ranges_4097_items", "ranges_prefetch_large",
                 "packed_ranges_large", "slots_4097_sites_flag_alt", "groups_4097_sites", "packed_groups_4097_sites"):
        assert items(by(name)) > M.GRID_CAP, name
    # the prefetch across work items: every range holds a whole load block of whole chunks
    for name, block in (("ranges_prefetch_large", M.BLOCK_SAMPLES), ("packed_ranges_large", M.PACKED_BLOCK_SAMPLES)):
        c = by(name)
        g = HC.labels_of(c).astype(np.int64)
        edges = [0] + [int(i) + 1 for i in np.flatnonzero(np.diff(g))] + [c.n]
        assert all(((s0 + 15) >> 4) + block // 16 <= (s1 >> 4) for s0, s1 in zip(edges, edges[1:])), name
    # the 16-bit counters: at the bound a copy's counter takes 62,512 samples of one (label, class); beyond it the launcher keeps 16 copies
    c = by("h16_bound")
    assert c.n == M.H16_MAX_SAMPLES and by("h16_past_bound").n == c.n + 16 and not M.labels_ordered(HC.labels_of(c), c.k)
    chunks = c.n // 16
    assert max(len(range(copy, chunks, 32)) for copy in range(32)) * 16 == 62512 < 65536
    # the wave kernel's threshold and its grid loop
    assert by("wave_n16384").n == M.WAVE_ROW_MAX and by("wave_n16384").n_sites == 256 * 2 * M.CSR_WAVES
    assert by("csr_65539_sites").n_sites > M.WAVE_GRID_CAP * M.CSR_WAVES
    for tag in ("csr", "csr_packed"):
        for name in (f"{tag}_residues_short", f"{tag}_residues_long"):
            o = np.concatenate([[0], np.cumsum(by(name).n)])[:-1]
            assert set(int(x) % 16 for x in o) == set(range(16)), name


SMALL = [c for c in HC.CASES if c.gen != "device" and c.n_sites <= 100 and (isinstance(c.n, tuple) or c.n <= 100000)]


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.build()
    return o


def test_model_equals_the_oracle_on_the_catalogue(orc):
    """hist_model.counts against orc.dense_hist and the oracle's group loop (which keeps a group's samples by their label)."""
    checked = 0
    for c in SMALL:
        if c.entry in M.CSR_ENTRIES:
            continue
        t = HC.tile(c)
        b, q = M.unpack(t["packed"]) if HC.is_packed(c) else (t["bases"], t["quals"])
        b, q = b.view(np.int8), q.view(np.int8)
        got = HC.model_counts(c, t)
        for s in range(c.n_sites):
            if c.k == 0:
                assert np.array_equal(got[s], orc.dense_hist(b[s], q[s])), (c.name, s)
            else:
                for g in range(c.k):
                    assert np.array_equal(got[s, g], orc.dense_hist(b[s], q[s], t["labels"], g)), (c.name, s, g)
                assert np.array_equal(got[s].sum(axis=0, dtype=np.uint32), orc.dense_hist(b[s], q[s])), (c.name, s)
            checked += 1
    assert checked > 500


def test_ragged_model_equals_the_dense_model():
    for c in SMALL:
        if c.entry not in M.CSR_ENTRIES:
            continue
        t = HC.tile(c)
        got = HC.model_counts(c, t)
        o = t["offsets"]
        for s in range(c.n_sites):
            row = slice(int(o[s]), int(o[s + 1]))
            want = M.counts_packed(t["packed"][None, row]) if HC.is_packed(c) else M.counts(t["bases"][None, row], t["quals"][None, row])
            assert np.array_equal(got[s], want[0]), (c.name, s)


def test_packed_model_is_the_two_byte_model_without_wide_qualities():
    for c in SMALL:
        if HC.is_packed(c) or c.entry in M.CSR_ENTRIES:
            continue
        t = HC.tile(c)
        want = M.counts(t["bases"], t["quals"], t.get("labels"), c.k).reshape(-1, 4, 128).copy()
        want[:, :, 63:] = 0
        got = M.counts_packed(M.pack(t["bases"], t["quals"]), t.get("labels"), c.k)
        assert np.array_equal(got.reshape(-1, 4, 128), want), c.name
    # the four no-observation bytes, and every other byte in its class
    every = np.arange(256, dtype=np.uint8)[None, :]
    got = M.counts_packed(every)[0].reshape(4, 128)
    assert got[:, :63].min() == 1 and got[:, :63].max() == 1 and got[:, 63:].max() == 0 and got.sum() == 252


def test_bytes_of_the_catalogue():
    t = HC.tile(HC.by_name("dense_bytes_all"))
    b, q = t["bases"].view(np.uint8), t["quals"].view(np.uint8)
    assert len(set(zip(b[0].tolist(), q[0].tolist()))) == 65536                # every base byte with every qual byte: -128..127 both
    c = M.counts(t["bases"], t["quals"])
    assert c[0].min() == 1 and c[0].max() == 1 and c[1].sum() == 0 and c[2].max() == 65536 == c[2].sum()
    t = HC.tile(HC.by_name("packed_bytes_all"))
    assert set(t["packed"][0].tolist()) == set(range(256)) and set(t["packed"][1].tolist()) == {0x3F, 0x7F, 0xBF, 0xFF}
    c = M.counts_packed(t["packed"])
    assert c[1].sum() == 0 and c[2].max() == 4096
    # flagged and unflagged sites alternate: an odd site holds one covered sample of quality 63, 64 or 127
    case = HC.by_name("slots_4097_sites_flag_alt")
    wide = M.counts(*[HC.tile(case)[x] for x in ("bases", "quals")]).reshape(-1, 4, 128)[:, :, 63:].sum(axis=(1, 2))
    assert np.array_equal(wide, np.arange(case.n_sites) % 2)


def moved(counts512):
    """The counts with a single observation moved to the neighbouring quality class (None: the site has no observation to move)."""
    c = np.array(counts512, np.uint32).reshape(4, 128)
    for b, q in zip(*np.nonzero(c[:, :62])):
        c[b, q] -= 1
        c[b, q + 1] += 1
        return c.reshape(512)
    return None


def test_probe_sites_have_teeth(orc):
    """Every records-only case names a site whose records change when one observation moves to the next quality class (checked here
    on the CPU oracle's stage 2; the device test asserts it on the device's)."""
    for c in HC.RECORD_CASES:
        if c.gen == "device":
            continue
        t = HC.tile(c)
        cnt = HC.model_counts(c, t)[c.probe]
        site = cnt.sum(axis=0, dtype=np.uint32) if c.k else cnt
        other = moved(site)
        assert other is not None, c.name
        ref = int(t["ref"][c.probe])
        assert orc.hist_lrt(site, ref, HC.MIN_AF) != orc.hist_lrt(other, ref, HC.MIN_AF), c.name
