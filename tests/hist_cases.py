"""Hand-built catalogue of stage-1 calls: every shape, alignment, label vector and tuning at which csrc/hist_kernel.hip takes another
path, each with the kernel instances it is meant to reach (hist_model.plan at 256 CUs restates the launchers; tests/test_hist_cases.py
holds the census, tests/test_gpu_hist_cases.py runs the catalogue on the device against hist_model.counts).

A case is: a name; the entry point; the tile (built from `seed` by `gen`); the byte offset of each array inside its allocation
(bases, quals, labels -- or packed, labels); the row stride; the labels and k; the tuning keys; `want`, the instances that count it.
Shapes are the smallest at which a path can still go wrong; only the cases with large=True exceed a few MB (they are generated on
the device).
"""
import collections

import numpy as np

from tests import hist_model as M

Case = collections.namedtuple("Case", "name entry n_sites n stride offs k labels tuning gen seed want probe large")

CASES = []
MIN_AF = 0.001
FLAG_QUALS = (63, 64, 127)                   # a covered sample of such a quality has no slot in the 256-slot forms: the site is redone


def up16(n):
    return (n + 15) // 16 * 16


def aligned_stride(n):
    return up16(n) + 16                      # a gap after every row: a read past a row's end meets covered-looking guard bytes


def odd_stride(n):
    return up16(n) + 19


def add(name, entry, n_sites, n, want, *, stride=None, offs=None, k=0, labels=None, tuning=(), gen="mix", probe=0, large=False):
    ragged = entry in M.CSR_ENTRIES
    arrays = 1 if entry in M.PACKED_ENTRIES + M.PACKED_GROUP_ENTRIES + ("lrt_csr_packed",) else 2
    if offs is None:
        offs = (0,) * (arrays + (k > 0))
    assert len(offs) == arrays + (k > 0), name
    if stride is None:
        stride = 0 if ragged else aligned_stride(n)
    assert not any(c.name == name for c in CASES), name
    CASES.append(Case(name, entry, n_sites, tuple(n) if ragged else n, stride, tuple(offs), k, labels, tuple(sorted(dict(tuning).items())),
                      gen, len(CASES) + 1, tuple(want), probe, large))


def by_name(name):
    return next(c for c in CASES if c.name == name)


def is_packed(case):
    return case.entry in M.PACKED_ENTRIES + M.PACKED_GROUP_ENTRIES + ("lrt_csr_packed",)


def returns_counts(case):
    return case.entry in ("hist_dense", "hist_dense_packed", "counts_add_dense", "counts_add_dense_packed", "counts_add_dense_groups")


# ---- labels ------------------------------------------------------------------------------------------------------------------------
def runs(*pairs):
    """('runs', ((label, count), ...)): consecutive runs; count None = the rest of the row."""
    return ("runs", tuple(pairs))


def rand(*values):
    """('rand', values): every sample one of `values`, drawn from the case's seed."""
    return ("rand", tuple(values))


def labels_of(case):
    if case.k == 0:
        return None
    kind, arg = case.labels[0], case.labels[1]
    n = case.n
    if kind == "rand":
        rng = np.random.default_rng(1000 + case.seed)
        g = np.asarray(arg, np.uint8)[rng.integers(0, len(arg), n)]
    else:
        g = np.zeros(n, np.uint8)
        at = 0
        for label, count in arg:
            count = n - at if count is None else count
            g[at:at + count] = label
            at += count
        assert at == n, (case.name, at, n)
    if len(case.labels) > 2:                 # ('runs', ..., last): the last element replaced
        g[-1] = case.labels[2]
    return g


# ---- tiles -------------------------------------------------------------------------------------------------------------------------
def _fill_two_byte(rng, b, q, mode):
    """One site's samples (views b, q of uint8) by mode: 0 covered, qualities below 63 (the wave-wide fast paths); 1 the same with three
    samples in ten not covered; 2 covered, qualities 0..127; 3 any byte in either array."""
    n = len(b)
    b[:] = rng.integers(0, 4, n)
    q[:] = rng.integers(0, 63, n)
    if mode == 1:
        hole = rng.random(n) < 0.3
        b[hole] = rng.integers(4, 256, n)[hole]
        far = rng.random(n) < 0.05
        q[far] = rng.integers(128, 256, n)[far]
    elif mode == 2:
        q[:] = rng.integers(0, 128, n)
    elif mode == 3:
        b[:] = rng.integers(0, 256, n)
        q[:] = rng.integers(0, 256, n)
        near = rng.random(n) < 0.5               # half of them bases, so that the wide qualities are counted too
        b[near] &= 3


def _fill_packed(rng, p, mode):
    """0 / 2: every byte an observation; 1: three in ten one of the four no-observation bytes; 3: any byte."""
    n = len(p)
    p[:] = rng.integers(0, 4, n) << 6 | rng.integers(0, 63, n)
    if mode == 1:
        hole = rng.random(n) < 0.3
        p[hole] = np.asarray([0x3F, 0x7F, 0xBF, 0xFF], np.uint8)[rng.integers(0, 4, n)][hole]
    elif mode == 3:
        p[:] = rng.integers(0, 256, n)


def tile(case):
    """The case's arrays as numpy: {'bases', 'quals'} or {'packed'}, 'labels' (k > 0), 'offsets' (ragged), 'ref'.  Dense arrays are
    [n_sites][n]; the device test lays them out at the case's stride and offsets.  Not for gen == 'device' (see device_tile)."""
    assert case.gen != "device", case.name
    rng = np.random.default_rng(case.seed)
    ns, packed = case.n_sites, is_packed(case)
    out = {"ref": ((np.arange(ns) + 1) % 4).astype(np.int8)}
    if case.entry in M.CSR_ENTRIES:
        lens = np.asarray(case.n, np.int64)
        o = np.zeros(ns + 1, np.int64)
        o[1:] = np.cumsum(lens)
        out["offsets"] = o
        rows = [(int(o[s]), int(o[s + 1])) for s in range(ns)]
        total = max(int(o[ns]), 1)
        shape = (total,)
    else:                                                      # (one_class: the tile of the longer row, cut to this case's n)
        rows, shape = None, (ns, max(case.n, M.H16_MAX_SAMPLES + 16) if case.gen == "one_class" else case.n)
    b, q = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for s in range(ns):
        vb, vq = (b[rows[s][0]:rows[s][1]], q[rows[s][0]:rows[s][1]]) if rows else (b[s], q[s])
        n = len(vb)
        if case.gen == "mix":
            mode = s % 4
        elif case.gen == "clean":
            mode = 0
        else:
            mode = {"flag_alt": 0, "bytes_all": 3, "one_class": 1}[case.gen]
        if packed:
            _fill_packed(rng, vb, mode)
        else:
            _fill_two_byte(rng, vb, vq, mode)
        if case.gen == "flag_alt" and s % 2 == 1:            # one covered sample of quality 63, 64 or 127
            at = (s * 7) % n
            if packed:
                vb[at] = 0x7F                                 # (a packed row has no such quality: one no-observation byte instead)
            else:
                vb[at], vq[at] = s % 4, FLAG_QUALS[(s // 2) % 3]
        if case.gen == "bytes_all":
            if s == 0 and packed:                             # every byte 0..255, sixteen times over
                vb[:] = rng.permutation(np.arange(n) % 256)
            elif s == 0:                                      # every (base byte, qual byte) pair
                assert n == 65536
                perm = rng.permutation(65536)
                vb[:], vq[:] = perm >> 8, perm & 255
            elif s == 1 and packed:                           # entirely uncovered
                vb[:] = np.asarray([0x3F, 0x7F, 0xBF, 0xFF], np.uint8)[np.arange(n) % 4]
            elif s == 1:
                vb[:] = rng.integers(4, 256, n)
            elif s == 2:                                      # all one class
                vb[:] = 0x9A if packed else 2
                vq[:] = 37
        if case.gen == "one_class" and s == 0:
            vb[:] = 0x85 if packed else 2
            vq[:] = 5
    if not rows:
        b, q = np.ascontiguousarray(b[:, :case.n]), np.ascontiguousarray(q[:, :case.n])
    if packed:
        out["packed"] = b
    else:
        out["bases"], out["quals"] = b.view(np.int8), q.view(np.int8)
    if case.k:
        out["labels"] = labels_of(case)
    return out


def device_tile(case, torch, device):
    """gen == 'device': the tile as [n_sites][stride] tensors made on the device from the case's seed (the model is computed from
    their copy on the host).  Every byte of a row's gap is a covered-looking sample too."""
    g = torch.Generator(device=device)
    g.manual_seed(case.seed)
    shape = (case.n_sites, case.stride)
    if is_packed(case):
        return {"packed": torch.randint(0, 256, shape, generator=g, device=device, dtype=torch.uint8)}
    b = torch.randint(0, 4, shape, generator=g, device=device, dtype=torch.int8)
    q = torch.randint(0, 128, shape, generator=g, device=device, dtype=torch.int8)
    b[:, 5::997] = -1                                         # a sprinkle of samples that are not covered, by either byte
    q[1::3, 11::1013] = -128
    return {"bases": b, "quals": q}


def model_counts(case, t):
    """hist_model's counts of the case's tile t (numpy arrays as tile() returns them)."""
    if case.entry in M.CSR_ENTRIES:
        return M.counts_csr(t["offsets"], t["packed"] if is_packed(case) else t["bases"], None if is_packed(case) else t["quals"])
    if is_packed(case):
        return M.counts_packed(t["packed"], t.get("labels"), case.k)
    return M.counts(t["bases"], t["quals"], t.get("labels"), case.k)


def plan_of(case, n_cu=256):
    """hist_model.plan of the case."""
    g = labels_of(case)
    return M.plan(case.entry, case.n_sites, case.n, case.stride, case.offs[:1 if is_packed(case) else 2], case.k,
                  g is not None and M.labels_ordered(g, case.k), dict(case.tuning), n_cu)


# ====================================================================================================================================
# The catalogue
# ====================================================================================================================================
D, P, W, B = M.name_dense, M.name_packed, M.name_wave, M.name_csr_block
R, PR, G, S, PG = M.name_ranges, M.name_packed_ranges, M.name_groups, M.name_slots, M.name_packed_groups
BLK, PBLK, BLK1024 = M.BLOCK_SAMPLES, M.PACKED_BLOCK_SAMPLES, M.BLOCK_SAMPLES_1024
STEPS = (0, 1, 15, 16, 17)                                    # around the loop steps of every family


def lengths(block):
    """0, 1, 15, 16, 17; one load block - 1 chunk, one block, one block + 1 chunk; two blocks and a ragged tail."""
    return STEPS + (block - 16, block, block + 16, 2 * block + 3 * 16 + 5)


# ---- plain dense, two bytes per sample: hist_dense_kernel<ALIGNED> -----------------------------------------------------------------
for n in lengths(BLK):
    add(f"dense_n{n}", "hist_dense", 5, n, [D(True)])
    add(f"dense_add_n{n}", "counts_add_dense", 5, n, [] if n == 0 else [D(True)])
for off, tag in (((1, 1), "off1"), ((15, 15), "off15"), ((0, 1), "q_off1"), ((16, 0), "off16")):
    for n in (17, BLK + 16, 2 * BLK + 53):
        add(f"dense_{tag}_n{n}", "hist_dense", 5, n, [D(off == (16, 0))], offs=off)
for n in (17, BLK, 2 * BLK + 53):
    add(f"dense_odd_stride_n{n}", "hist_dense", 5, n, [D(False)], stride=odd_stride(n))
# parts of a row: hist_split by tuning (at 64 parts and three blocks, parts 3..62 own no chunk and the last takes the tail alone)
for split in (1, 2, 5, 64):
    for n in (17, BLK + 16, 2 * BLK + 53):
        add(f"dense_split{split}_n{n}", "hist_dense", 3, n, [D(True)], tuning={"hist_split": split})
    add(f"dense_split{split}_unaligned", "counts_add_dense", 3, 2 * BLK + 53, [D(False)], offs=(1, 1), tuning={"hist_split": split})
# every (base byte, qual byte) pair; a site entirely uncovered; a site all one class.  65536 samples and three sites: the automatic split (2)
add("dense_bytes_all", "hist_dense", 3, 65536, [D(True)], gen="bytes_all")
add("dense_bytes_all_add", "counts_add_dense", 3, 65536, [D(True)], gen="bytes_all")
add("dense_bytes_all_unaligned", "hist_dense", 3, 65536, [D(False)], gen="bytes_all", offs=(15, 1))
# more work items than the grid cap: 4097 sites in two parts each (with one part they would be the wave kernel's); odd sites flagged
add("dense_4097_sites", "hist_dense", 4097, 40, [D(True)], tuning={"hist_split": 2}, gen="flag_alt")
add("dense_4097_sites_unaligned", "hist_dense", 4097, 40, [D(False)], tuning={"hist_split": 2}, gen="flag_alt", offs=(1, 0))

# ---- short dense rows, one wavefront per site: hist_wave_kernel<ALIGNED, true> (n_sites >= 16 * CUs, split 1, n <= 16384) ----------
for n in (1, 17, 63, 64, 65):
    add(f"wave_n{n}", "hist_dense", 4096, n, [W(True, True, False)])
    add(f"wave_unaligned_n{n}", "hist_dense", 4096, n, [W(False, True, False)], offs=(1, 1))
add("wave_add_n65", "counts_add_dense", 4099, 65, [W(True, True, False)])
add("wave_one_site_short", "hist_dense", 4095, 65, [D(True)])          # one site fewer: the block kernel
add("wave_n16384", "hist_dense", 4096, 16384, [W(True, True, False)], stride=16400, gen="device", large=True)
add("wave_n16385", "hist_dense", 4096, 16385, [D(True)], stride=16400, gen="device", large=True)    # the same tile, one sample more
CASES[-1] = CASES[-1]._replace(seed=CASES[-2].seed)

# ---- plain dense, one byte per sample: hist_packed_kernel<ALIGNED> -----------------------------------------------------------------
for n in lengths(PBLK):
    add(f"packed_n{n}", "hist_dense_packed", 5, n, [P(True)])
for n in (0, 17, PBLK + 16):
    add(f"packed_add_n{n}", "counts_add_dense_packed", 5, n, [] if n == 0 else [P(True)])
for off in (1, 15):
    for n in (17, PBLK + 16, 2 * PBLK + 53):
        add(f"packed_off{off}_n{n}", "hist_dense_packed", 5, n, [P(False)], offs=(off,))
add("packed_odd_stride", "hist_dense_packed", 5, PBLK + 16, [P(False)], stride=odd_stride(PBLK + 16))
for split in (2, 5, 64):
    add(f"packed_split{split}", "hist_dense_packed", 3, 2 * PBLK + 53, [P(True)], tuning={"hist_split": split})
    add(f"packed_split{split}_unaligned", "counts_add_dense_packed", 3, 2 * PBLK + 53, [P(False)], offs=(1,), tuning={"hist_split": split})
add("packed_bytes_all", "hist_dense_packed", 3, 4096, [P(True)], gen="bytes_all")
add("packed_bytes_all_unaligned", "hist_dense_packed", 3, 4096, [P(False)], gen="bytes_all", offs=(1,))
add("packed_auto_split", "hist_dense_packed", 3, 65536 + 21, [P(True)])
add("packed_4097_sites", "hist_dense_packed", 4097, 40, [P(True)], gen="flag_alt")
add("packed_4097_sites_unaligned", "hist_dense_packed", 4097, 40, [P(False)], gen="flag_alt", offs=(15,))

# ---- labels ordered by group: hist_dense_ranges_kernel / hist_packed_ranges_kernel -------------------------------------------------
ORDERED = [
    # range edges inside one 16-sample chunk (s0 = 3, s1 = 8: c0 = 1 > c1 = 0); a range of exactly one chunk [16, 32)
    ("edges_in_chunk", 3, 100, runs((0, 3), (1, 5), (2, 8), (3, None))),      # and [8, 16): c0 = c1 = 1, no whole chunk either
    ("one_chunk", 3, 100, runs((0, 16), (1, 16), (2, 16), (3, None))),
    ("head_and_tail", 2, 100, runs((0, 20), (1, 10), (2, None))),             # [0, 20): one chunk and a tail; [20, 30): c0 = 2 > c1 = 1
    ("empty_first_middle_last", 5, 3 * 16 + 7, runs((1, 20), (3, None))),     # groups 0, 2, 4 and "no group" are empty
    ("all_no_group", 4, 77, runs((4, 30), (5, 30), (255, None))),             # labels k, k + 1 and 255: every sample in "no group"
    ("labels_k_k1_255", 4, 16 * 9 + 3, runs((0, 33), (3, 40), (4, 20), (255, 20), (5, None))),
    ("k1", 1, BLK + 40, runs((0, BLK + 8), (1, None))),
    ("k32", 32, 32 * 21 + 9, runs(*[(g, 21) for g in range(32)], (32, None))),
    ("one_group_only", 5, 2 * BLK + 53, runs((2, None))),                     # a single non-empty range: n_real = 1
    ("blocks", 3, 3 * BLK + 16 * 5 + 9, runs((0, BLK + 8), (1, BLK - 16 + 3), (2, 37), (3, None))),
    ("n1", 2, 1, runs((1, None))),
    ("n17", 2, 17, runs((0, 16), (2, None))),
]
for tag, k, n, g in ORDERED:
    add(f"ranges_{tag}", "counts_add_dense_groups", 5, n, [R(True)], k=k, labels=g, offs=(0, 0, 3))
    add(f"ranges_unaligned_{tag}", "counts_add_dense_groups", 5, n, [R(False)], k=k, labels=g, offs=(1, 15, 0))
    add(f"packed_ranges_{tag}", "lrt_dense_groups_packed", 5, n, [PR(True)], k=k, labels=g, offs=(0, 3))
    add(f"packed_ranges_unaligned_{tag}", "lrt_dense_groups_packed", 5, n, [PR(False)], k=k, labels=g, offs=(1, 0))
add("packed_ranges_blocks2", "lrt_dense_groups_packed", 5, 3 * PBLK + 91, [PR(True)], k=2, gen="mix",
    labels=runs((0, PBLK + 8), (1, PBLK - 16 + 3), (2, None)))
add("ranges_odd_stride", "counts_add_dense_groups", 5, 100, [R(False)], k=3, labels=ORDERED[0][3], stride=odd_stride(100))
# ordered except for the last element: the any-order kernels
add("ranges_last_out_of_order", "counts_add_dense_groups", 5, 100, [G(3, True)], k=3, labels=ORDERED[1][3] + (0,))
add("packed_ranges_last_out_of_order", "lrt_dense_groups_packed", 5, 100, [PG(4, True, 512)], k=3, labels=ORDERED[1][3] + (0,))
# more work items than the grid cap (sites x non-empty ranges): small ranges, then -- large -- every range at least one load block long,
# so that the next item's first block is prefetched before the fold of the current one (`have` in hist_dense_ranges_kernel)
add("ranges_4097_items", "counts_add_dense_groups", 1400, 50, [R(True)], k=3, labels=runs((0, 13), (1, 20), (3, None)), gen="flag_alt")
add("packed_ranges_4097_items", "lrt_dense_groups_packed", 1400, 50, [PR(True)], k=3, labels=runs((0, 13), (1, 20), (3, None)), gen="clean")
add("ranges_prefetch_large", "counts_add_dense_groups", 2049, 2 * BLK + 32, [R(True)], k=1, stride=2 * BLK + 32,
    labels=runs((0, BLK + 24), (1, None)), gen="device", large=True)
add("packed_ranges_large", "lrt_dense_groups_packed", 2049, 2 * PBLK + 32, [PR(True)], k=1, stride=2 * PBLK + 32,
    labels=runs((0, PBLK + 24), (1, None)), gen="device", large=True, probe=7)

# ---- labels in any order, two bytes per sample -------------------------------------------------------------------------------------
def any_labels(k):
    return rand(*range(k), k, k + 1, 255)


for n in (15, 16, 17, BLK - 16, BLK, BLK + 16, 2 * BLK + 53):              # a trip of either sample loop is one block (2 * 512 chunks)
    add(f"groups_k3_n{n}", "counts_add_dense_groups", 5, n, [G(3, True)], k=3, labels=any_labels(3))
    add(f"groups_k3_nopipe_n{n}", "counts_add_dense_groups", 5, n, [G(3, False)], k=3, labels=any_labels(3), tuning={"group_pipe": 0})
for n in (15, 16, 17, BLK1024 - 16, BLK1024, BLK1024 + 16, 2 * BLK1024 + 53):       # the slots kernel's block: 2 * 1024 chunks
    add(f"slots_k5_n{n}", "counts_add_dense_groups", 5, n, [S(4), G(2, True)], k=5, labels=any_labels(5), offs=(0, 0, 5))
    add(f"bytes_k5_n{n}", "counts_add_dense_groups", 5, n, [M.NAME_BYTES], k=5, labels=any_labels(5), offs=(1, 1, 0))
add("bytes_odd_stride", "counts_add_dense_groups", 5, 200, [M.NAME_BYTES], k=5, labels=any_labels(5), stride=odd_stride(200))
add("bytes_q_off1_k32", "counts_add_dense_groups", 5, 200, [M.NAME_BYTES], k=32, labels=any_labels(32), offs=(0, 1, 0))
add("bytes_k1", "counts_add_dense_groups", 5, 200, [M.NAME_BYTES], k=1, labels=any_labels(1), offs=(15, 15, 1))
NA = 2 * BLK + 53
GROUPS_BY_K = {1: [G(4, True)], 2: [G(3, True)], 3: [G(3, True)], 4: [S(4), G(2, True)], 7: [S(4), G(2, True)], 8: [S(3), G(1, True)],
               9: [S(3), G(1, True)], 16: [S(3), G(0, True)], 17: [S(2), G(0, True)], 31: [S(2), G(0, True)], 32: [S(2), G(0, True)]}
for k, want in GROUPS_BY_K.items():
    add(f"groups_k{k}", "counts_add_dense_groups", 5, NA, want, k=k, labels=any_labels(k))
for k, l in ((1, 4), (3, 3), (4, 2), (8, 1), (32, 0)):                      # without the slots kernel and without the pipeline
    add(f"groups_k{k}_plain", "counts_add_dense_groups", 5, NA, [G(l, False)], k=k, labels=any_labels(k), tuning={"group_pipe": 0, "group_big_lds": 0})
add("groups_k7_no_big_lds", "counts_add_dense_groups", 5, NA, [G(2, True)], k=7, labels=any_labels(7), tuning={"group_big_lds": 0})
for l in range(-1, 6):                                                      # group_copies_log2 caps the copies: below 3 the slots kernel goes first
    want = [G(4, True)] if l in (-1, 4, 5) else ([G(3, True)] if l == 3 else [S(4), G(l, True)])
    add(f"groups_k1_log2c{l}", "counts_add_dense_groups", 5, 4 * 16 * 41 + 7, want, k=1, labels=any_labels(1), tuning={"group_copies_log2": l})
# 4097 sites; the odd ones hold one covered sample of quality 63, 64 or 127: a workgroup of the slots kernel takes a flagged and an
# unflagged site in turn (its flag and its LDS are cleared in between) and the redo kernel skips every other site
add("slots_4097_sites_flag_alt", "counts_add_dense_groups", 4097, 48, [S(4), G(2, True)], k=5, labels=any_labels(5), gen="flag_alt")
add("groups_4097_sites", "counts_add_dense_groups", 4097, 48, [G(3, True)], k=2, labels=any_labels(2), gen="flag_alt")
add("slots_one_flagged_site", "counts_add_dense_groups", 5, BLK1024 + 16 + 9, [S(3), G(1, False)], k=9, labels=any_labels(9), gen="flag_alt",
    tuning={"group_pipe": 0})

# ---- labels in any order, one byte per sample (records only) -----------------------------------------------------------------------
PACKED_BY_K = {1: PG(5, True, 512), 2: PG(4, True, 512), 3: PG(4, True, 512), 4: PG(4, True, 1024), 7: PG(4, True, 1024),
               8: PG(4, True, 1024), 9: PG(3, True, 1024), 16: PG(3, True, 1024), 17: PG(3, True, 1024), 31: PG(2, True, 1024),
               32: PG(2, True, 1024)}
for k, want in PACKED_BY_K.items():
    add(f"packed_groups_k{k}", "lrt_dense_groups_packed", 5, 2 * BLK1024 + 53, [want], k=k, labels=any_labels(k), offs=(0, 5))
for k, l in ((1, 5), (2, 4), (4, 3), (8, 2), (16, 1), (32, 0)):
    add(f"packed_groups_k{k}_no_big_lds", "lrt_dense_groups_packed", 5, NA, [PG(l, True, 512)], k=k, labels=any_labels(k), tuning={"group_big_lds": 0})
    add(f"packed_groups_k{k}_unaligned", "lrt_dense_groups_packed", 5, NA, [PG(l, False, 512)], k=k, labels=any_labels(k), offs=(1, 0))
add("packed_groups_odd_stride", "lrt_dense_groups_packed", 5, 300, [PG(3, False, 512)], k=5, labels=any_labels(5), stride=odd_stride(300))
for n in (15, 16, 17, BLK - 16, BLK, BLK + 16):                             # the 512-thread form's block: 2 * 512 chunks
    add(f"packed_groups_k2_n{n}", "lrt_dense_groups_packed", 5, n, [PG(4, True, 512)], k=2, labels=any_labels(2))
for n in (15, 16, 17, BLK1024 - 16, BLK1024, BLK1024 + 16):                 # the 1024-thread forms' block: 2 * 1024 chunks
    add(f"packed_groups_k5_n{n}", "lrt_dense_groups_packed", 5, n, [PG(4, True, 1024)], k=5, labels=any_labels(5))
    add(f"h16_k5_n{n}", "lrt_dense_groups_packed", 5, n, [M.NAME_H16], k=5, labels=any_labels(5), tuning={"group_h16": 1})
add("packed_groups_k1_log2c2", "lrt_dense_groups_packed", 5, NA, [PG(4, True, 1024)], k=1, labels=any_labels(1), tuning={"group_copies_log2": 2})
add("h16_k8", "lrt_dense_groups_packed", 5, NA, [M.NAME_H16], k=8, labels=any_labels(8), tuning={"group_h16": 1})
add("h16_k9_does_not_fit", "lrt_dense_groups_packed", 5, NA, [PG(3, True, 1024)], k=9, labels=any_labels(9), tuning={"group_h16": 1})
add("h16_unaligned", "lrt_dense_groups_packed", 5, NA, [PG(3, False, 512)], k=5, labels=any_labels(5), tuning={"group_h16": 1}, offs=(15, 0))
add("packed_groups_4097_sites", "lrt_dense_groups_packed", 4097, 48, [PG(4, True, 512)], k=2, labels=any_labels(2), gen="flag_alt")
# The 16-bit counters at their bound: 2,000,000 samples, site 0 all one class and (but for the last sample, which makes the vector
# any-order) all one label, so a copy's counter of that class reaches 62,512.  Sixteen samples more and the launcher must keep the
# sixteen-copy kernel.
H16_LABELS = runs((2, None)) + (1,)
add("h16_bound", "lrt_dense_groups_packed", 2, M.H16_MAX_SAMPLES, [M.NAME_H16], k=5, labels=H16_LABELS, tuning={"group_h16": 1},
    gen="one_class", stride=M.H16_MAX_SAMPLES + 16, probe=1)
add("h16_past_bound", "lrt_dense_groups_packed", 2, M.H16_MAX_SAMPLES + 16, [PG(4, True, 1024)], k=5, labels=H16_LABELS, tuning={"group_h16": 1},
    gen="one_class", stride=M.H16_MAX_SAMPLES + 16, probe=1)
CASES[-1] = CASES[-1]._replace(seed=CASES[-2].seed)

# ---- ragged sites (records only): hist_wave_kernel<ALIGNED, false, PACKED> below 4096 observations, hist_csr_block_kernel from there ---
CSR_LENS = (0, 1, 63, 64, 65, 4095, 4096, 4097, BLK - 16, 0, BLK, BLK + 16, 20000, 2 * BLK + 53, 3)
for entry, tag in (("lrt_csr", "csr"), ("lrt_csr_packed", "csr_packed")):
    pk = entry == "lrt_csr_packed"
    for off in (0, 1):
        offs = (off,) if pk else (off, off)
        ut = "" if off == 0 else "_unaligned"
        add(f"{tag}_lengths{ut}", entry, len(CSR_LENS), CSR_LENS, [W(off == 0, False, pk), B(off == 0, pk)], offs=offs, probe=4)
    # a site's first element at every residue mod 16: lengths of 1 mod 16, short (the wave kernel) and long (the block kernel)
    add(f"{tag}_residues_short", entry, 33, (81,) * 33, [W(True, False, pk)], probe=4)
    add(f"{tag}_residues_long", entry, 17, (4113,) * 17, [B(True, pk)], probe=4)
    add(f"{tag}_residues_long_blocks", entry, 17, (BLK + 16 + 1,) * 17, [B(True, pk)], probe=4)
    # more than 8 * 8192 sites: the wave kernel's grid loops
    add(f"{tag}_65539_sites", entry, 65539, (3,) * 65539, [W(True, False, pk)], probe=4)
add("csr_q_off1", "lrt_csr", len(CSR_LENS), CSR_LENS, [W(False, False, False), B(False, False)], offs=(0, 1), probe=4)

RECORD_CASES = [c for c in CASES if not returns_counts(c)]
