"""The stage-1 catalogue (tests/hist_cases.py) on the device, against the plain model (tests/hist_model.py).  No tolerance anywhere.

Per case: the plan at the real device's CU count must still name the instances the case is meant for; the entry points that return
counts must return the model's, word for word; those that return only records must return the bytes stage 2 makes of the model's
counts in the same context (and the named probe site's records must change when one observation moves to the next quality class,
so that the comparison is known to have teeth).  Input arrays sit inside allocations of covered-looking bytes, so a read past a
row's end is counted; the output has a guard site in front and one behind.
"""
import numpy as np
import pytest

from tests import hist_cases as HC
from tests import hist_model as M

pytestmark = pytest.mark.gpu

FILL_BASE, FILL_QUAL, FILL_PACKED = 1, 30, 0x5E               # what a read outside the tile finds: a covered sample
GUARD_WORD, GUARD_BYTE = 0x5A5A5A5A, 0xA5
ADD_TO = 7                                                    # what the counts_add_* calls find in the caller's counts
SITE_BYTES, GROUP_BYTES = 120, 48
TAIL = 64                                                     # guard bytes behind the last row


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def contexts(torch):
    """One context per tuning set, made on first use and closed at the end of the module."""
    from basevarc_amd import Context
    made = {}

    def get(tuning):
        if tuning not in made:
            ctx = Context(0, stream=torch.cuda.current_stream())
            for key, value in tuning:
                ctx.set_tuning(key, value)
            made[tuning] = ctx
        return made[tuning]
    yield get
    for ctx in made.values():
        ctx.close()


def place_rows(torch, rows, off, stride, fill):
    """rows [n_sites][n] (numpy) at byte `off` of an allocation filled with `fill`, `stride` bytes apart: the strided view."""
    ns, n = rows.shape
    t = torch.from_numpy(rows)
    alloc = torch.full((off + ns * stride + TAIL,), fill, dtype=t.dtype, device="cuda:0")
    view = alloc[off:].as_strided((ns, n), (stride, 1))
    if n:
        view.copy_(t.to("cuda:0"))
    return view


def place_flat(torch, a, off, fill):
    t = torch.from_numpy(a)
    alloc = torch.full((off + len(a) + TAIL,), fill, dtype=t.dtype, device="cuda:0")
    alloc[off:off + len(a)].copy_(t.to("cuda:0"))
    return alloc[off:off + len(a)]


def guarded(torch, n_items, item, fill, dtype):
    """[1 guard][n_items][1 guard] items of `item` elements: (whole buffer, the view of the real items)."""
    buf = torch.full(((n_items + 2) * item,), fill, dtype=dtype, device="cuda:0")
    return buf, buf[item:(n_items + 1) * item]


def guards_intact(buf, item, fill):
    return bool((buf[:item] == fill).all()) and bool((buf[-item:] == fill).all())


def on_device(torch, case):
    """(device tensors, host arrays) of the case's tile."""
    packed = HC.is_packed(case)
    if case.gen == "device":
        d = {key: v[:, :case.n] for key, v in HC.device_tile(case, torch, "cuda:0").items()}
        h = {key: v.cpu().numpy() for key, v in d.items()}
        h["ref"] = ((np.arange(case.n_sites) + 1) % 4).astype(np.int8)
        if case.k:
            h["labels"] = HC.labels_of(case)
    else:
        h = HC.tile(case)
        fills = {"packed": FILL_PACKED, "bases": FILL_BASE, "quals": FILL_QUAL}
        keys = ("packed",) if packed else ("bases", "quals")
        if case.entry in M.CSR_ENTRIES:
            d = {key: place_flat(torch, h[key], off, fills[key]) for key, off in zip(keys, case.offs)}
            d["offsets"] = torch.from_numpy(h["offsets"]).to("cuda:0")
        else:
            d = {key: place_rows(torch, h[key], off, case.stride, fills[key]) for key, off in zip(keys, case.offs)}
    for key, off in zip(("packed",) if packed else ("bases", "quals"), case.offs):
        assert d[key].data_ptr() % 16 == off % 16, (case.name, key)          # the alignment the case is about
    if case.k:
        d["labels"] = place_flat(torch, h["labels"], case.offs[-1], 0)
    d["ref"] = torch.from_numpy(h["ref"]).to("cuda:0")
    return d, h


def run_counts(torch, ctx, case, d):
    """The entry points that return counts: (guarded buffer, the real sites as uint32 numpy, what the call found in them)."""
    n_hist = case.k + 1 if case.k else 1
    buf, real = guarded(torch, case.n_sites, n_hist * M.NCLASS, GUARD_WORD, torch.int32)
    adds = case.entry.startswith("counts_add")
    real.fill_(ADD_TO if adds else 0x77777777)               # the hist_* calls overwrite every word
    if case.entry == "hist_dense":
        ctx.hist_dense_device(d["bases"], d["quals"], real)
    elif case.entry == "hist_dense_packed":
        ctx.hist_dense_packed_device(d["packed"], real)
    elif case.entry == "counts_add_dense":
        ctx.counts_add_dense_device(d["bases"], d["quals"], real)
    elif case.entry == "counts_add_dense_packed":
        ctx.counts_add_dense_packed_device(d["packed"], real)
    else:
        assert case.entry == "counts_add_dense_groups", case.entry
        ctx.counts_add_dense_groups_device(d["bases"], d["quals"], d["labels"], case.k, real)
    got = real.cpu().numpy().view(np.uint32).reshape(case.n_sites, n_hist, M.NCLASS)
    return buf, got, ADD_TO if adds else 0


def stage2(torch, ctx, case, counts, ref_t):
    """(site record bytes, group record bytes) that stage 2 makes of `counts` (numpy uint32) in this context."""
    c = torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).to("cuda:0")
    if case.k:
        res, gres = ctx.lrt_hist_groups_device(c, ref_t, HC.MIN_AF, case.k)
        return res.cpu().numpy().tobytes(), gres.cpu().numpy().tobytes()
    return ctx.lrt_hist_device(c, ref_t, HC.MIN_AF).cpu().numpy().tobytes(), b""


def run_records(torch, ctx, case, d):
    """The entry points that return only records: (guarded buffers, site record bytes, group record bytes)."""
    ns = case.n_sites
    rbuf, res = guarded(torch, ns, SITE_BYTES, GUARD_BYTE, torch.uint8)
    if case.entry == "lrt_csr":
        ctx.lrt_csr_device(d["offsets"], d["bases"], d["quals"], d["ref"], HC.MIN_AF, res)
        return [(rbuf, SITE_BYTES)], res.cpu().numpy().tobytes(), b""
    if case.entry == "lrt_csr_packed":
        ctx.lrt_csr_packed_device(d["offsets"], d["packed"], d["ref"], HC.MIN_AF, res)
        return [(rbuf, SITE_BYTES)], res.cpu().numpy().tobytes(), b""
    assert case.entry == "lrt_dense_groups_packed", case.entry
    gbuf, gres = guarded(torch, ns, case.k * GROUP_BYTES, GUARD_BYTE, torch.uint8)
    ctx.lrt_dense_groups_packed_device(d["packed"], d["ref"], HC.MIN_AF, d["labels"], case.k, res, gres)
    return [(rbuf, SITE_BYTES), (gbuf, case.k * GROUP_BYTES)], res.cpu().numpy().tobytes(), gres.cpu().numpy().tobytes()


def move_one(counts_site):
    """A site's counts ([512] or [n_hist][512]) with a single observation moved to the neighbouring quality class."""
    c = np.array(counts_site, np.uint32).reshape(-1, 4, 128)
    h, b, q = [int(x[0]) for x in np.nonzero(c[:, :, :62])]
    c[h, b, q] -= 1
    c[h, b, q + 1] += 1
    return c.reshape(np.shape(counts_site))


@pytest.mark.parametrize("case", HC.CASES, ids=[c.name for c in HC.CASES])
def test_case(case, torch, contexts):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    planned = tuple(HC.plan_of(case, n_cu))
    assert planned == case.want, f"{case.name}: with {n_cu} CUs this shape no longer reaches {case.want}, it reaches {planned}"
    ctx = contexts(case.tuning)
    d, h = on_device(torch, case)
    model = HC.model_counts(case, h)
    if HC.returns_counts(case):
        buf, got, base = run_counts(torch, ctx, case, d)
        want = (model.reshape(got.shape) + np.uint32(base)).astype(np.uint32)
        if not np.array_equal(got, want):
            s, hh, cls = [int(x[0]) for x in np.nonzero(got != want)]
            raise AssertionError(f"{case.name}: {int((got != want).sum())} words differ; first at site {s} histogram {hh} class {cls} "
                                 f"(base {cls >> 7}, qual {cls & 127}): got {int(got[s, hh, cls]) - base}, model {int(want[s, hh, cls]) - base}")
        assert guards_intact(buf, (case.k + 1 if case.k else 1) * M.NCLASS, GUARD_WORD), f"{case.name}: a guard site of the counts was written"
        return
    bufs, res, gres = run_records(torch, ctx, case, d)
    want_res, want_gres = stage2(torch, ctx, case, model, d["ref"])
    if res != want_res or gres != want_gres:
        a = np.frombuffer(res, np.uint8).reshape(case.n_sites, -1) != np.frombuffer(want_res, np.uint8).reshape(case.n_sites, -1)
        bad = np.flatnonzero(a.any(axis=1))
        raise AssertionError(f"{case.name}: the records differ from stage 2 of the model's counts: {len(bad)} site records (first: {bad[:5]}), "
                             f"group records {'differ' if gres != want_gres else 'equal'}")
    for buf, item in bufs:
        assert guards_intact(buf, item, GUARD_BYTE), f"{case.name}: a guard record was written"
    # the comparison has teeth: one observation of the probe site in the neighbouring quality class gives other records
    p = slice(case.probe, case.probe + 1)
    one, other = model[p], move_one(model[case.probe])[None]
    assert stage2(torch, ctx, case, one, d["ref"][p]) != stage2(torch, ctx, case, other, d["ref"][p]), f"{case.name}: probe site {case.probe} is insensitive"
