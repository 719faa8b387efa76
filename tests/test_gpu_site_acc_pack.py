"""bvc_site_acc_pack and bvc_site_acc_add_packed on the device (acc_pack_kernel.hip, bvc_bam_counts.hip; GPU), word for word against the plain
model (tests/acc_pack_model.py: dense arrays <-> logical rows <-> entries).

1. add_packed against the existing read path: model entries into a zeroed accumulator of every kind, then bvc_site_acc_get / get_depth
   equal the dense model; into a filled one the sum modulo 2^32.
2. pack against the model, from host and device pointers, guard words round every output, the two-step protocol, no second allocation.
3. Sub-ranges; 4. kind independence on the test BAMs and the catalogue; 5. every refusal leaves the accumulator as it was; 6. four threads'
   contexts; 7. stage 2 on an accumulator rebuilt from its own pieces."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import acc_pack_model as pm
from tests import bam_counts_model as cm
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests.test_gpu_bam_counts import CATALOGUE, MIN_AF, acc_args, bgzf_args, span_case, bams100  # noqa: F401  (bams100: that module's fixture)

pytestmark = pytest.mark.gpu

GUARD = 64
ROWS = (0, 1, 63, 64, 65, 3000)                  # 3,000: more rows than one grid round (704 workgroups of four rows)
# (name, n_groups, depth_groups, n_quals): wide without and with groups (33 slots: the longest row, 66 rounds of count pieces), the depth kind,
# narrow rows at every width with 0, 5 and 32 groups
KINDS = ([("wide", 0, 0, None), ("wide g1", 1, 0, None), ("wide g32", 32, 0, None), ("depth g5", 0, 5, None), ("depth g32", 0, 32, None)] +
         [(f"narrow q{q} g{g}", 0, g, q) for q in (4, 40, 124, 128) for g in (0, 5, 32)])
p = lambda a: C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def make_acc(kind, P):
    from basevarc_amd import SiteAcc
    _, ng, dg, q = kind
    if q is not None:
        return SiteAcc.create_quals(0, P, q, dg)
    return SiteAcc.create_depth(0, P, dg) if dg else SiteAcc(0, P, ng)


def shape_of(kind):
    """(slots, depth_groups, W, the logical cells the kind has a word for, the logical cell of every STORED word in piece order -- -1: a pad)."""
    _, ng, dg, q = kind
    slots = ng + 1 if ng else 1
    W = pm.row_words(slots, dg)
    cols = 128 if q is None else q
    count_cells = np.array([s * 512 + b * 128 + k for s in range(slots) for b in range(4) for k in range(cols)])
    stored = np.concatenate([count_cells, slots * 512 + np.array(list(range(10)) + [-1 - slots * 512] * 2), slots * 512 + 10 + np.arange(4 * dg)])
    return slots, dg, W, stored[stored >= 0], stored


def make_rows(kind, n, seed=0):
    """Logical rows [n, W]: the rows the issue lists, cyclically at the front and again at the end, sparse random rows between them."""
    slots, dg, W, valid, stored = shape_of(kind)
    cc = slots * 512
    rng = np.random.default_rng(1000 * seed + n + W)
    rows = np.zeros((n, W), dtype=np.uint32)

    def special(k, row):
        if k == 1:                                # word 0 and word 3 of a 16-byte piece: of the first count piece and of the tally's second
            row[[0, 3, cc + 4, cc + 7]] = [5, 6, 7, 8]
        elif k == 2:                              # the stored words 255 and 256: the edge between two rounds of 64 lanes
            edge = [c for c in stored[255:257] if c >= 0] if len(stored) > 256 else [valid[len(valid) // 2]]
            row[edge] = 9
        elif k == 3:                              # every word the kind stores
            row[valid] = rng.integers(1, 1 << 32, len(valid), dtype=np.uint64).astype(np.uint32)
        elif k == 4:                              # only the last depth word (the last word of the row)
            row[valid[-1]] = 11
        elif k == 5:                              # only tally word 9
            row[cc + 9] = 12
        elif k == 6:                              # counts of 1, 0xFFFF, 0x10000 and 0xFFFFFFFF
            row[[valid[0], valid[1], valid[2], cc + 1]] = [1, 0xFFFF, 0x10000, 0xFFFFFFFF]
    for t in range(n):
        if t < 14 or t >= n - 7:
            special((t if t < 14 else t - (n - 7)) % 7, rows[t])      # (row 0 and the first of the last seven: empty)
        else:
            k = int(rng.integers(0, 12))
            at = rng.choice(valid, size=min(k, len(valid)), replace=False)
            rows[t, at] = rng.integers(1, 1 << 32, len(at), dtype=np.uint64).astype(np.uint32)
    return rows


def read_back(ctx, acc, kind, t0=0, n=None):
    """The accumulator's rows through the EXISTING read path, as logical rows."""
    counts, tally = acc.get(ctx, t0, n)
    depth = acc.get_depth(ctx, t0, n) if kind[2] else None
    return pm.logical_rows(counts, tally, depth)


def pack_host(ctx, acc, t0, n):
    """Both steps from host pointers into guarded arrays.  Returns (rc of the first step, row_start, cell, count)."""
    L = ctx._L
    rs = np.full(n + 1 + 2 * GUARD, -0x3232323232323233, dtype=np.int64)
    need = C.c_int64(-1)
    rc1 = L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, p(rs[GUARD:]), None, None, 0, C.byref(need), 0)
    assert rc1 in (0, pm.ACC_MORE), (rc1, L.bvc_last_error(ctx._h))
    ne = need.value
    assert (rc1 == pm.ACC_MORE) == (ne > 0) and rs[GUARD] == 0 and rs[GUARD + n] == ne
    assert (rs[:GUARD] == rs[0]).all() and (rs[GUARD + n + 1:] == rs[0]).all() and rs[0] < 0
    cell = np.full(ne + 2 * GUARD, 0xCDCD, dtype=np.uint16)
    count = np.full(ne + 2 * GUARD, 0xCDCDCDCD, dtype=np.uint32)
    if ne > 0:
        # a cap one too small: BVC_ACC_MORE, row_start written in full, cell and count untouched
        first = rs.copy()
        rs[GUARD:GUARD + n + 1] = -7
        assert L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, p(rs[GUARD:]), p(cell[GUARD:]), p(count[GUARD:]), ne - 1, C.byref(need), 0) == pm.ACC_MORE
        assert need.value == ne and (rs == first).all() and (cell == 0xCDCD).all() and (count == 0xCDCDCDCD).all()
    assert L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, p(rs[GUARD:]), p(cell[GUARD:]), p(count[GUARD:]), ne, C.byref(need), 0) == 0 and need.value == ne
    for g, word in ((cell, 0xCDCD), (count, 0xCDCDCDCD)):
        assert (g[:GUARD] == word).all() and (g[GUARD + ne:] == word).all()
    assert (rs[:GUARD] == rs[0]).all() and (rs[GUARD + n + 1:] == rs[0]).all()
    return rc1, rs[GUARD:GUARD + n + 1].copy(), cell[GUARD:GUARD + ne].copy(), count[GUARD:GUARD + ne].copy()


def pack_device(ctx, acc, t0, n):
    """Both steps from device pointers into guarded tensors."""
    import torch
    L = ctx._L
    rs = torch.full((n + 1 + 2 * GUARD,), -5, dtype=torch.int64, device="cuda")
    need = C.c_int64(-1)
    at = lambda t, k: C.c_void_p(t.data_ptr() + k * t.element_size())
    rc1 = L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, at(rs, GUARD), None, None, 0, C.byref(need), 1)
    assert rc1 in (0, pm.ACC_MORE)
    ne = need.value
    cell = torch.full((ne + 2 * GUARD,), -13108, dtype=torch.int16, device="cuda")           # 0xCCCC
    count = torch.full((ne + 2 * GUARD,), -858993460, dtype=torch.int32, device="cuda")     # 0xCCCCCCCC
    if ne > 0:
        assert L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, at(rs, GUARD), at(cell, GUARD), at(count, GUARD), ne - 1, C.byref(need), 1) == pm.ACC_MORE
        ctx.synchronize()
        assert need.value == ne and bool((cell == -13108).all()) and bool((count == -858993460).all())
    assert L.bvc_site_acc_pack(ctx._h, acc._h, t0, n, at(rs, GUARD), at(cell, GUARD), at(count, GUARD), ne, C.byref(need), 1) == 0 and need.value == ne
    ctx.synchronize()
    rs, cell, count = rs.cpu().numpy(), cell.cpu().numpy().view(np.uint16), count.cpu().numpy().view(np.uint32)
    assert (rs[:GUARD] == -5).all() and (rs[GUARD + n + 1:] == -5).all()
    for g, word in ((cell, 0xCCCC), (count, 0xCCCCCCCC)):
        assert (g[:GUARD] == word).all() and (g[GUARD + ne:] == word).all()
    return rs[GUARD:GUARD + n + 1], cell[GUARD:GUARD + ne], count[GUARD:GUARD + ne]


def add_device(ctx, acc, rs, cell, count, t0=0):
    import torch
    d_rs = torch.from_numpy(np.ascontiguousarray(rs, dtype=np.int64)).cuda()
    d_cell = torch.from_numpy(np.ascontiguousarray(cell, dtype=np.uint16).view(np.int16).copy()).cuda()
    d_count = torch.from_numpy(np.ascontiguousarray(count, dtype=np.uint32).view(np.int32).copy()).cuda()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    rc = ctx._L.bvc_site_acc_add_packed(ctx._h, acc._h, t0, len(rs) - 1, C.c_void_p(d_rs.data_ptr()), ptr(d_cell), ptr(d_count), len(cell), 1)
    ctx.synchronize()
    return rc


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. add_packed against the existing read path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k[0])
def test_add_packed_against_the_existing_read_path(ctx, kind):
    for n in ROWS:
        rows, more = make_rows(kind, n), make_rows(kind, n, seed=1)
        if n > 6:
            more[6][rows[6] == 0xFFFFFFFF] = 1        # 0xFFFFFFFF + 1 wraps
        with make_acc(kind, n) as acc:
            assert acc.row_words() == (rows.shape[1], shape_of(kind)[0], kind[2])
            acc.add_packed(ctx, *pm.entries(rows))
            assert np.array_equal(read_back(ctx, acc, kind), rows), (kind, n)
            if n <= 65:
                assert add_device(ctx, acc, *pm.entries(more)) == 0
            else:
                acc.add_packed(ctx, *pm.entries(more))
            got = read_back(ctx, acc, kind)
            assert np.array_equal(got, rows + more), (kind, n)            # (uint32 arithmetic wraps)
            if n > 6:
                assert got[6][rows[6] == 0xFFFFFFFF].tolist() == [0]
            # an entry with count 0 is legal and adds nothing
            rs = np.zeros(n + 1, dtype=np.int64)
            rs[1:] = 1 if n else 0
            acc.add_packed(ctx, rs, np.array([3] if n else [], dtype=np.uint16), np.array([0] if n else [], dtype=np.uint32))
            assert np.array_equal(read_back(ctx, acc, kind), got)


# ---- 2. pack against the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k[0])
def test_pack_against_the_model_from_host_and_device_pointers(ctx, kind):
    for n in ROWS:
        rows = make_rows(kind, n)
        want = pm.entries(rows)
        with make_acc(kind, n) as acc:
            acc.add_packed(ctx, *want)
            rc1, *got = pack_host(ctx, acc, 0, n)
            assert same(got, want), (kind, n)
            assert same(pack_device(ctx, acc, 0, n), want), (kind, n)
            assert same(acc.pack(ctx), want)
            assert got[1].dtype == np.uint16 and (np.diff(got[0]) <= rows.shape[1]).all()


def test_the_model_rows_hold_what_the_issue_lists():
    for kind in KINDS:
        slots, dg, W, valid, stored = shape_of(kind)
        rows = make_rows(kind, 65)
        rs, cell, count = pm.entries(rows)
        assert rs[1] == 0 and rs[8] == rs[7] and rs[4] - rs[3] == len(valid)                     # an empty row, a full row
        assert cell[rs[1]:rs[2]].tolist() == [0, 3, slots * 512 + 4, slots * 512 + 7]
        assert cell[rs[5]:rs[6]].tolist() == [slots * 512 + 9] and cell[rs[4]:rs[5]].tolist() == [W - 1 if dg else valid[-1]]
        assert sorted(count[rs[6]:rs[7]].tolist()) == [1, 0xFFFF, 0x10000, 0xFFFFFFFF]
        if kind[3] is None:
            assert cell[rs[2]:rs[3]].tolist() == [255, 256]
        assert pm.verdict(rs, cell, count, 65, W, kind[3] or 128) is None
    assert pm.row_words(33, 0) == 33 * 512 + 10 and len(shape_of(KINDS[2])[4]) // 4 == 66 * 64 + 3


def test_a_second_call_of_the_same_shape_allocates_nothing(ctx):
    import torch
    kind = KINDS[9]                                  # narrow q40 g5
    rows = make_rows(kind, 3000)
    want = pm.entries(rows)
    with make_acc(kind, 3000) as acc:
        free = []
        torch.cuda.mem_get_info()
        for _ in range(2):
            acc.add_packed(ctx, *want)
            assert add_device(ctx, acc, *want) == 0
            acc.pack(ctx)
            pack_device(ctx, acc, 0, 3000)
            ctx.synchronize()
            torch.cuda.empty_cache()
            free.append(torch.cuda.mem_get_info()[0])
        assert free[1] == free[0], free
        assert np.array_equal(read_back(ctx, acc, kind), rows * np.uint32(4))


# ---- 3. sub-ranges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [KINDS[0], KINDS[9], KINDS[4]], ids=lambda k: k[0])
def test_sub_ranges_concatenate_to_the_whole(ctx, kind):
    n = 3000
    rows = make_rows(kind, n)
    whole = pm.entries(rows)
    with make_acc(kind, n) as acc:
        # the pieces go in one by one, each at its t0
        cuts = [0, 1, 64, 65, 1233, 2010, 2999, 3000]
        for a, b in zip(cuts, cuts[1:]):
            acc.add_packed(ctx, *pm.entries(rows[a:b]), t0=a)
        assert np.array_equal(read_back(ctx, acc, kind), rows)
        for t0, m in ((1233, 777), (2999, 1), (3000, 0), (64, 1), (17, 0)):
            assert same(acc.pack(ctx, t0, m), pm.entries(rows[t0:t0 + m])), (t0, m)
            assert same(pack_device(ctx, acc, t0, m), pm.entries(rows[t0:t0 + m])), (t0, m)
        for cuts in ([0, 1500, 3000], [0, 63, 64, 129, 2817, 3000]):
            assert same(pm.concat([acc.pack(ctx, a, b - a) for a, b in zip(cuts, cuts[1:])]), whole)


# ---- 4. kind independence -------------------------------------------------------------------------------------------------------------------
def test_a_wide_and_a_forty_column_accumulator_give_the_same_pieces(ctx, bams100):
    from basevarc_amd import SiteAcc
    b = bams100
    P = len(b["pv"])
    want_c, want_t = cm.fold(b["exp"]["maps"], b["pv"])
    want = pm.entries(pm.logical_rows(want_c.reshape(P, 512), want_t))
    with SiteAcc(0, P) as wide, SiteAcc.create_quals(0, P, 40) as narrow, SiteAcc.create_quals(0, P, 40) as into_narrow, SiteAcc(0, P) as into_wide:
        for a in (wide, narrow):
            assert ctx.bam_counts_bgzf_acc(*acc_args(b), a)[0] == 0
        pw, pn = wide.pack(ctx), narrow.pack(ctx)
        assert same(pw, pn) and same(pw, want) and len(pw[1]) > 30000
        # either piece added into the other kind reproduces it
        into_narrow.add_packed(ctx, *pw)
        into_wide.add_packed(ctx, *pn)
        for a in (into_narrow, into_wide):
            c, t = a.get(ctx)
            assert c.tobytes() == wide.get(ctx)[0].tobytes() and t.tobytes() == want_t.tobytes()
        assert same(into_narrow.pack(ctx), want) and same(into_wide.pack(ctx), want)


def test_the_catalogues_batches_through_both_kinds(ctx):
    from basevarc_amd import SiteAcc
    from tests import bam_counts_quals_model as qm
    done = 0
    for c in CATALOGUE:
        exp = qm.expected(None, None, None, None, c["positions"], None, None, 40, exp=bc.expected(c))
        if exp["rc"] != 0 or not len(c["samples"]) or not len(c["positions"]) or not exp["counts"].any():
            continue
        P = len(c["positions"])
        want = pm.entries(pm.logical_rows(exp["counts"], exp["tally"]))
        with SiteAcc(0, P) as wide, SiteAcc.create_quals(0, P, 40) as narrow:
            for a in (wide, narrow):
                assert ctx.bam_counts_bgzf_acc(*bgzf_args(c), a)[0] == 0
            assert same(wide.pack(ctx), want) and same(narrow.pack(ctx), want), c["name"]
        done += 1
        if done == 8:
            break
    assert done >= 3


# ---- 5. the refusals --------------------------------------------------------------------------------------------------------------------------
def faulty_pieces(rows, W, narrow):
    """[(what, row_start, cell, count, n_entries or None)] built from a sound piece of `rows`."""
    rs, cell, count = pm.entries(rows)
    n = len(rs) - 1
    full = [t for t in range(n) if rs[t + 1] - rs[t] >= 3]
    k, k2 = full[1], full[-1]
    out = []

    def variant(what, f, ne=None):
        r, c, v = rs.copy(), cell.copy(), count.copy()
        f(r, c, v)
        out.append((what, r, c, v, ne))
    variant("row_start does not start at 0", lambda r, c, v: r.__setitem__(0, 1))
    variant("row_start decreases", lambda r, c, v: r.__setitem__(k + 1, r[k] - 1))
    variant("row_start negative", lambda r, c, v: r.__setitem__(k, -3))
    variant("a row_start word far outside the entries", lambda r, c, v: r.__setitem__(k2, 1 << 40))
    variant("row_start does not end at n_entries", lambda r, c, v: None, ne=len(cell) - 1)
    variant("row_start ends before n_entries", lambda r, c, v: r.__setitem__(n, r[n] - 1))
    variant("a cell of W", lambda r, c, v: c.__setitem__(r[k + 1] - 1, W))
    variant("a cell of 0xFFFF", lambda r, c, v: c.__setitem__(r[k2], 0xFFFF))
    variant("equal cells", lambda r, c, v: c.__setitem__(r[k] + 1, c[r[k]]))
    variant("descending cells", lambda r, c, v: c.__setitem__(slice(r[k], r[k] + 2), c[r[k]:r[k] + 2][::-1].copy()))
    variant("two faults: the first row is named", lambda r, c, v: (c.__setitem__(r[k2], 0xFFFF), c.__setitem__(r[k] + 1, c[r[k]])))
    if narrow:
        variant("quality 40", lambda r, c, v: c.__setitem__(r[k], 128 + 40))
        variant("quality 127 of the last base", lambda r, c, v: c.__setitem__(r[k], 511))
    return out


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[9], KINDS[2]], ids=lambda k: k[0])
def test_every_refusal_leaves_the_accumulator_as_it_was(ctx, kind):
    from basevarc_amd.lib import BvcError
    n = 200
    L = ctx._L
    slots, dg, W, valid, _ = shape_of(kind)
    narrow = kind[3] is not None
    rows = make_rows(kind, n, seed=3)
    if narrow:
        for base in range(4):                                   # (quality 0 alone in the count cells: a cell to turn into quality 40)
            rows[:, base * 128 + 1:(base + 1) * 128] = 0
        rows[20:30, 0] = 7
    sound = pm.entries(rows)
    with make_acc(kind, n) as acc:
        acc.add_packed(ctx, *sound)
        before = [x.tobytes() for x in acc.get(ctx)] + ([acc.get_depth(ctx).tobytes()] if dg else [])
        unchanged = lambda: [x.tobytes() for x in acc.get(ctx)] + ([acc.get_depth(ctx).tobytes()] if dg else []) == before
        for what, rs, cell, count, ne in faulty_pieces(rows, W, narrow):
            ne = len(cell) if ne is None else ne
            t, fault = pm.verdict(rs, cell[:ne], count[:ne], n, W, kind[3] or 128, slots * 512)
            for device in (False, True):
                if device:
                    rc = add_device(ctx, acc, rs, cell[:ne], count[:ne])
                else:
                    rc = L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, n, p(rs), p(cell), p(count), ne, 0)
                msg = L.bvc_last_error(ctx._h).decode()
                assert rc == pm.ERR_DATA and msg.startswith(f"row {t}:"), (what, device, rc, msg, t)
                assert ("n_quals = 40" in msg) == (fault == pm.FAULT_QUAL), (what, msg)
                assert unchanged(), (what, device)
        if narrow:
            # quality 39 is accepted where quality 40 is refused
            acc.add_packed(ctx, [0, 1], [128 + 39], [2], t0=5)
            with pytest.raises(BvcError, match="row 0: .*n_quals = 40") as e:
                acc.add_packed(ctx, [0, 1], [128 + 40], [2], t0=5)
            assert e.value.status == pm.ERR_DATA
            rows[5, 128 + 39] += 2
            assert np.array_equal(read_back(ctx, acc, kind), rows)
            before = [x.tobytes() for x in acc.get(ctx)] + ([acc.get_depth(ctx).tobytes()] if dg else [])
        # bad arguments: rows outside the accumulator, null pointers, negative sizes
        rs, cell, count = sound
        ne = len(cell)
        for t0, m in ((-1, 1), (0, n + 1), (n, 1), (1, n), (0, -1)):
            assert L.bvc_site_acc_add_packed(ctx._h, acc._h, t0, m, p(rs), p(cell), p(count), ne, 0) == pm.ERR_ARG, (t0, m)
            assert b"outside the accumulator" in L.bvc_last_error(ctx._h)
            need = C.c_int64(-9)
            assert L.bvc_site_acc_pack(ctx._h, acc._h, t0, m, p(rs.copy()), None, None, 0, C.byref(need), 0) == pm.ERR_ARG and need.value == -9
        assert L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, n, None, p(cell), p(count), ne, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, n, p(rs), None, p(count), ne, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, n, p(rs), p(cell), None, ne, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, n, p(rs), p(cell), p(count), -1, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(ctx._h, None, 0, n, p(rs), p(cell), p(count), ne, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(None, acc._h, 0, n, p(rs), p(cell), p(count), ne, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_add_packed(ctx._h, acc._h, 0, 0, p(rs), p(cell), p(count), 1, 0) == pm.ERR_DATA
        need = C.c_int64(-9)
        out = rs.copy()
        assert L.bvc_site_acc_pack(ctx._h, acc._h, 0, n, None, None, None, 0, C.byref(need), 0) == pm.ERR_ARG
        assert L.bvc_site_acc_pack(ctx._h, acc._h, 0, n, p(out), None, None, 0, None, 0) == pm.ERR_ARG
        assert L.bvc_site_acc_pack(ctx._h, acc._h, 0, n, p(out), None, None, -1, C.byref(need), 0) == pm.ERR_ARG
        assert L.bvc_site_acc_pack(ctx._h, acc._h, 0, n, p(out), None, None, ne + 8, C.byref(need), 0) == pm.ERR_ARG     # room, and nowhere to put them
        assert L.bvc_site_acc_pack(None, acc._h, 0, n, p(out), None, None, 0, C.byref(need), 0) == pm.ERR_ARG
        assert L.bvc_site_acc_pack(ctx._h, None, 0, n, p(out), None, None, 0, C.byref(need), 0) == pm.ERR_ARG
        assert unchanged()
        # and the calls still work
        assert same(acc.pack(ctx), pm.entries(rows))


# ---- 6. four threads, four contexts -----------------------------------------------------------------------------------------------------------
def test_four_threads_contexts_add_pieces_and_a_batch_into_one_accumulator(ctx):
    from basevarc_amd import Context
    from tests import bam_counts_quals_model as qm
    P, Q = 300, 44
    kind = ("narrow q44 g0", 0, 0, Q)
    batch = span_case(P, 6)
    exp = qm.expected(None, None, None, None, batch["positions"], None, None, Q, exp=bc.expected(batch))
    assert exp["rc"] == 0
    parts = [make_rows(kind, P, seed=10 + k) for k in range(4)]
    want = pm.logical_rows(exp["counts"], exp["tally"]) * np.uint32(3)
    for r in parts:
        want = want + r * np.uint32(3)
    errors = []
    with make_acc(kind, P) as acc:
        def work(k):
            try:
                with Context(0) as c2:
                    for _ in range(3):
                        for a, b in ((0, 150), (150, P)):
                            acc.add_packed(c2, *pm.entries(parts[k][a:b]), t0=a)
                        if k == 2:
                            assert c2.bam_counts_bgzf_acc(*bgzf_args(batch), acc)[0] == 0
            except Exception as e:                               # noqa: BLE001
                errors.append(e)
        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert np.array_equal(read_back(ctx, acc, kind), want)
    bc._EXPECTED.pop(batch["name"], None)


# ---- 7. stage 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_stage_two_on_an_accumulator_rebuilt_from_its_own_pieces(ctx, bams100):
    from basevarc_amd import SiteAcc
    b = bams100
    P = len(b["pv"])
    with SiteAcc(0, P) as wide, SiteAcc(0, P) as again, SiteAcc.create_quals(0, P, 40) as narrow:
        assert ctx.bam_counts_bgzf_acc(*acc_args(b), wide)[0] == 0
        want = wide.lrt(ctx, b["ref_base"], MIN_AF)
        cuts = [0, 1000, 1001, 4000, P]
        for a, e in zip(cuts, cuts[1:]):
            piece = wide.pack(ctx, a, e - a)
            again.add_packed(ctx, *piece, t0=a)
            narrow.add_packed(ctx, *piece, t0=a)
        assert again.lrt(ctx, b["ref_base"], MIN_AF).tobytes() == want.tobytes() and narrow.lrt(ctx, b["ref_base"], MIN_AF).tobytes() == want.tobytes()
        assert 0 < int((want["called"] != 0).sum()) < P // 10
