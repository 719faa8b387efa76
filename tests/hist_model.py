"""Stage 1 restated in plain numpy: what the histogram kernels of csrc/hist_kernel.hip must count, and which of them counts a call.

counts / counts_packed / counts_csr are the definition (hist_kernel.hip's header comment): integer arithmetic only, no
library of the project involved.  plan restates the launchers (choose_hist_split, plan_group_copies, launch_hist_dense,
launch_hist_packed, launch_hist_packed_groups, launch_hist_csr) and returns kernel names spelled as tools/isa_report.py prints them.
"""
import itertools

import numpy as np

NCLASS = 512
MAX_GROUPS = 32

# ---- the constants of hist_kernel.hip that the launchers and the catalogue's shapes depend on
HIST_THREADS = 512
UNROLL = 2                                   # kUnroll
PACKED_UNROLL = 4                            # kPackedUnroll
BLOCK_SAMPLES = UNROLL * HIST_THREADS * 16           # one load block of a two-byte row: 16384 samples
PACKED_BLOCK_SAMPLES = PACKED_UNROLL * HIST_THREADS * 16    # of a packed row: 32768
BLOCK_SAMPLES_1024 = 2 * 1024 * 16                   # of the 1024-thread kernels: 32768
WAVE_ROW_MAX = 16384                         # kWaveRowMax
CSR_LONG = 4096                              # kCsrLong
CSR_WAVES = HIST_THREADS // 64               # kCsrWaves
GRID_CAP = 4096                              # grid_cap()
WAVE_GRID_CAP = 8192
H16_MAX_SAMPLES = 2000000                    # kH16MaxSamples
LDS_WORDS = NCLASS * 32                      # kLdsWords
BIG_LDS_BYTES = 144 * 1024                   # kBigLdsBytes
PACKED_SLOTS = 256

TUNING_DEFAULTS = {"hist_split": 0, "group_pipe": 1, "group_copies_log2": -1, "group_big_lds": 1, "group_h16": 0}


def _u8(a):
    a = np.asarray(a)
    assert a.dtype.itemsize == 1, a.dtype
    return a.view(np.uint8)


def _accumulate(out, site, hist, cls, keep):
    """out[site][hist][cls] += 1 for the kept observations (flat integer index, np.bincount without weights)."""
    n_hist = out.shape[1]
    idx = (site.astype(np.int64) * n_hist + hist) * NCLASS + cls
    out += np.bincount(idx[keep], minlength=out.size).astype(np.uint32).reshape(out.shape)


def _hist_of(labels, n, n_groups):
    if labels is None:
        return np.zeros(n, np.int64)
    g = _u8(labels).astype(np.int64)
    assert g.shape == (n,)
    return np.minimum(g, n_groups)


def counts(bases, quals, labels=None, n_groups=0):
    """[site][n_groups + 1][512] uint32 (or [site][512] without labels) of a two-byte tile [site][sample]: an observation counts when
    0 <= base < 4 and 0 <= qual < 128 (both bytes read as unsigned), its class is base * 128 + qual, its histogram min(label, n_groups)."""
    b, q = _u8(bases), _u8(quals)
    assert b.ndim == 2 and b.shape == q.shape
    ns, n = b.shape
    out = np.zeros((ns, n_groups + 1 if labels is not None else 1, NCLASS), np.uint32)
    h = _hist_of(labels, n, n_groups)
    step = max(1, (1 << 24) // max(n, 1))               # rows per pass: bounded temporaries for the large tiles
    for s0 in range(0, ns, step):
        bb, qq = b[s0:s0 + step].astype(np.int64), q[s0:s0 + step].astype(np.int64)
        site = np.broadcast_to(np.arange(bb.shape[0])[:, None], bb.shape)
        _accumulate(out[s0:s0 + step], site, np.broadcast_to(h[None, :], bb.shape), (bb & 3) * 128 + (qq & 127), (bb < 4) & (qq < 128))
    return out if labels is not None else out[:, 0]


def unpack(packed):
    """packed byte -> (base, qual) as the two-byte kernels see them: qual bits 63 (0x3F, 0x7F, 0xBF, 0xFF) = no observation (base 255)."""
    p = _u8(packed)
    q = p & 63
    b = np.where(q == 63, 255, p >> 6).astype(np.uint8)
    return b, q.astype(np.uint8)


def pack(bases, quals):
    """(base, qual) -> base << 6 | qual; a sample that is not covered, or whose quality does not fit (63..127), becomes 0xFF."""
    b, q = _u8(bases), _u8(quals)
    return np.where((b < 4) & (q < 63), (b << 6) | (q & 63), 0xFF).astype(np.uint8)


def counts_packed(packed, labels=None, n_groups=0):
    """counts of a packed tile [site][sample] (byte = base << 6 | qual; quality bits 63 = no observation; qualities 63..127 stay zero)."""
    b, q = unpack(packed)
    return counts(b, q, labels, n_groups)


def counts_csr(offsets, bases, quals=None):
    """[site][512] of ragged sites: site s owns elements offsets[s] .. offsets[s + 1]; quals None = packed observations in `bases`."""
    o = np.asarray(offsets, np.int64)
    b, q = unpack(bases) if quals is None else (_u8(bases), _u8(quals))
    ns = len(o) - 1
    out = np.zeros((ns, 1, NCLASS), np.uint32)
    b, q = b[o[0]:o[ns]].astype(np.int64), q[o[0]:o[ns]].astype(np.int64)
    site = np.repeat(np.arange(ns), np.diff(o))
    _accumulate(out, site, np.zeros(len(b), np.int64), (b & 3) * 128 + (q & 127), (b < 4) & (q < 128))
    return out[:, 0]


def labels_ordered(labels, n_groups):
    """group_bounds_kernel's test: the labels clamped to n_groups never decrease."""
    h = _hist_of(labels, len(labels), n_groups)
    return bool(np.all(h[1:] >= h[:-1]))


# ---- the launchers restated --------------------------------------------------------------------------------------------------------
def _b(x):
    return "true" if x else "false"


def name_dense(aligned): return f"hist_dense_kernel<{_b(aligned)}>"
def name_packed(aligned): return f"hist_packed_kernel<{_b(aligned)}>"
def name_wave(aligned, dense, packed): return f"hist_wave_kernel<{_b(aligned)}, {_b(dense)}, {_b(packed)}>"
def name_csr_block(aligned, packed): return f"hist_csr_block_kernel<{_b(aligned)}, {_b(packed)}>"
def name_ranges(aligned): return f"hist_dense_ranges_kernel<{_b(aligned)}>"
def name_packed_ranges(aligned): return f"hist_packed_ranges_kernel<{_b(aligned)}>"
def name_groups(log2c, pipe): return f"hist_dense_groups_kernel<{log2c}, {_b(pipe)}>"
def name_slots(log2c): return f"hist_dense_groups_slots_kernel<{log2c}>"
def name_packed_groups(log2c, aligned, threads): return f"hist_packed_groups_kernel<{log2c}, {_b(aligned)}, {threads}>"


NAME_BYTES = "hist_dense_groups_bytes_kernel"
NAME_H16 = "hist_packed_groups_h16_kernel"
NOT_COUNTING = ("group_bounds_kernel", "pack_dense_kernel", "stream_read_kernel")


def all_names():
    """Every instance the launchers' tables and conditionals can name (whether or not a call can reach it)."""
    tf = (True, False)
    names = {NAME_BYTES, NAME_H16}
    names |= {f(a) for f in (name_dense, name_packed, name_ranges, name_packed_ranges) for a in tf}
    names |= {name_wave(a, True, False) for a in tf} | {name_wave(a, False, p) for a in tf for p in tf}
    names |= {name_csr_block(a, p) for a in tf for p in tf}
    names |= {name_groups(l, p) for l in range(6) for p in tf} | {name_slots(l) for l in (2, 3, 4)}
    names |= {name_packed_groups(l, a, 512) for l in range(6) for a in tf} | {name_packed_groups(l, True, 1024) for l in (2, 3, 4)}
    return names


def tuning_of(tuning):
    t = dict(TUNING_DEFAULTS)
    t.update(tuning or {})
    assert set(t) == set(TUNING_DEFAULTS), sorted(t)
    return t


def choose_hist_split(tuning, n_sites, n_samples, n_cu):
    t = tuning_of(tuning)
    if t["hist_split"] > 0:
        return t["hist_split"]
    want = n_cu * 4
    if n_sites >= want or n_samples < (1 << 16):
        return 1
    split = min((want + n_sites - 1) // n_sites, n_samples // (1 << 15))
    return int(min(max(split, 1), 64))


def plan_group_copies(tuning, n_hist, slots, big_tail):
    """(log2c, big): copies of the 64 KiB form, copies of the one-workgroup-per-CU form (-1: not used)."""
    t = tuning_of(tuning)
    log2c = 0
    while log2c < 5 and n_hist * slots * (2 << log2c) <= LDS_WORDS:
        log2c += 1
    if 0 <= t["group_copies_log2"] < log2c:
        log2c = t["group_copies_log2"]
    def big_bytes(l): return ((n_hist * PACKED_SLOTS) << l) * 4 + big_tail
    big = 4
    while big > 2 and big_bytes(big) > BIG_LDS_BYTES:
        big -= 1
    if not t["group_big_lds"] or big_bytes(big) > BIG_LDS_BYTES:
        big = -1
    return log2c, big


DENSE_ENTRIES = ("hist_dense", "counts_add_dense", "lrt_dense")
PACKED_ENTRIES = ("hist_dense_packed", "counts_add_dense_packed", "lrt_dense_packed")
GROUP_ENTRIES = ("counts_add_dense_groups", "lrt_dense_groups")
PACKED_GROUP_ENTRIES = ("lrt_dense_groups_packed",)
CSR_ENTRIES = ("lrt_csr", "lrt_csr_packed")
ENTRIES = DENSE_ENTRIES + PACKED_ENTRIES + GROUP_ENTRIES + PACKED_GROUP_ENTRIES + CSR_ENTRIES


def plan(entry, n_sites, n_samples, row_stride, align, k, ordered, tuning, n_cu):
    """Names of the kernel instances that count the call, in launch order.

    entry: one of ENTRIES.  n_samples: the row length; for the ragged entries the sequence of site lengths.  align: the residue mod 16
    of each array's address, (bases, quals) or (packed,).  k: n_groups (0 without groups).  ordered: labels_ordered() of the call's
    labels.  Where the launcher enqueues two kernels and one returns at once (ranges against any-order) only the one that counts is
    named; the slots kernel and the kernel that redoes its flagged sites are both named."""
    t = tuning_of(tuning)
    if n_sites <= 0:
        return []
    ptr_ok = all(a % 16 == 0 for a in align)
    if entry in CSR_ENTRIES:
        packed = entry == "lrt_csr_packed"
        lens = np.asarray(n_samples, np.int64)
        assert lens.shape == (n_sites,)
        names = []
        if np.any(lens < CSR_LONG):
            names.append(name_wave(ptr_ok, False, packed))
        if np.any(lens >= CSR_LONG):
            names.append(name_csr_block(ptr_ok, packed))
        return names
    aligned = ptr_ok and row_stride % 16 == 0
    assert row_stride >= n_samples >= 0
    if entry in DENSE_ENTRIES or entry in PACKED_ENTRIES:
        if n_samples == 0 and entry.startswith("counts_add"):
            return []                                            # nothing to add: no launch
        split = choose_hist_split(t, n_sites, n_samples, n_cu)
        if entry in PACKED_ENTRIES:
            return [name_packed(aligned)]
        if split == 1 and n_samples <= WAVE_ROW_MAX and n_sites >= n_cu * 2 * CSR_WAVES:
            return [name_wave(aligned, True, False)]
        return [name_dense(aligned)]
    assert 1 <= k <= MAX_GROUPS, k
    if n_samples == 0:
        return []                                                # hipMemsetAsync (or, adding, nothing at all)
    n_hist = k + 1
    if entry in GROUP_ENTRIES:
        if ordered:
            return [name_ranges(aligned)]
        log2c, big = plan_group_copies(t, n_hist, NCLASS, 16)
        if not aligned:
            return [NAME_BYTES]
        names = [name_slots(big)] if big >= 0 and log2c < 3 else []
        return names + [name_groups(log2c, t["group_pipe"])]
    assert entry in PACKED_GROUP_ENTRIES, entry
    if ordered:
        return [name_packed_ranges(aligned)]
    log2c, big = plan_group_copies(t, n_hist, PACKED_SLOTS, 0)
    if (t["group_h16"] and t["group_big_lds"] and aligned and log2c < 4 and n_hist * 128 * 32 * 4 <= BIG_LDS_BYTES
            and n_samples <= H16_MAX_SAMPLES):
        return [NAME_H16]
    if big >= 0 and aligned and log2c < big:
        return [name_packed_groups(big, True, 1024)]
    return [name_packed_groups(log2c, aligned, 512)]


def work_items(entry, n_sites, n_samples, k, labels, tuning, n_cu):
    """Work items of the call's grid loop (sites x parts, or sites x non-empty ranges): above GRID_CAP a workgroup takes several."""
    if entry in DENSE_ENTRIES or entry in PACKED_ENTRIES:
        return n_sites * choose_hist_split(tuning, n_sites, n_samples, n_cu)
    if labels is not None and labels_ordered(labels, k):
        return n_sites * len(np.unique(_hist_of(labels, len(labels), k)))
    return n_sites


def all_tunings():
    """Every value of the five tuning keys the launchers read (hist_split only matters to the plain entries: 0 and three fixed values)."""
    for pipe, log2c, big, h16 in itertools.product((0, 1), range(-1, 6), (0, 1), (0, 1)):
        yield {"group_pipe": pipe, "group_copies_log2": log2c, "group_big_lds": big, "group_h16": h16}
