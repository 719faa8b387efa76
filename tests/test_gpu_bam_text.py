"""bvc_bam_pileup_text on the device (bam_text_kernel.hip; GPU) against the plain Python model (tests/bam_text_model.py, which
tests/test_bam_text_abi.py holds to the CPU path): the binary call's catalogue, the cases the text form adds and the seeded random run,
from host and from device pointers -- every byte of text, line_start, sample_status, *text_needed and the return code, with guard bytes
around the outputs and bam / text at odd addresses; the two-step output; the refusals; no allocation in a second call of the same shape;
the _bgzf form on the 100 test BAMs' own blocks."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm
from tests import bam_text_model as tm

pytestmark = pytest.mark.gpu

GUARD = 64
CATALOGUE = bc.catalogue()
TEXT_CASES = tm.cases()


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


def arrays(c):
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    return (np.frombuffer(bam, dtype=np.uint8), np.array(off, dtype=np.int64), np.array(end, dtype=np.int64), np.array(eof, dtype=np.uint8), np.array(rid, dtype=np.int32),
            np.array(c["positions"], dtype=np.int32), np.frombuffer(c["refseq"].encode(), dtype=np.uint8))


def run(ctx, c, device, cap=None, room=None, shift=0):
    """One call with guarded output buffers: (rc or the BvcError's status, the text buffer with GUARD + shift bytes in front of the text and
    GUARD behind its room, the line_start buffer, the sample_status buffer, needed).  cap: the text_cap told to the library (default: the
    room); room: bytes of text between the guards (default: the model's size); shift 1: bam and text begin at odd addresses."""
    from basevarc_amd.lib import BvcError
    exp = tm.expected(c)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    n, P = len(rid), len(pos)
    want = len(exp["text"]) if exp["text"] is not None else 0
    room = want if room is None else room
    front = GUARD + shift
    whole = np.full(front + room + GUARD, 0xCD, dtype=np.uint8)
    line_start = np.full(P + 1 + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    status = np.full(n + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    cap = room if cap is None else cap
    shifted = np.concatenate([np.full(shift, 0x5A, dtype=np.uint8), bam])
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        d_bam, d_whole = dev(shifted), dev(whole)
        assert d_bam.data_ptr() % 2 == 0 and d_whole.data_ptr() % 2 == 0
        args = [d_bam[shift:]] + [dev(a) for a in (off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], dev(ref)]
        out = [d_whole[front:], dev(line_start), dev(status)]
    else:
        assert shifted.ctypes.data % 2 == 0 and whole.ctypes.data % 2 == 0
        args = [shifted[shift:], off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref]
        out = [whole[front:], line_start, status]
    try:
        rc, _, _, _, need = ctx.bam_pileup_text(*args, text=out[0], text_cap=cap, line_start=out[1], sample_status=out[2])
    except BvcError as e:
        rc, need = e.status, None
    if device:
        ctx.synchronize()
        whole, line_start, status = d_whole.cpu().numpy(), out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint32)
    return rc, whole, line_start, status, need, front


def check(c, got):
    """What a call left, against the model: everything the model names, and nothing written anywhere else."""
    exp = tm.expected(c)
    rc, whole, line_start, status, need, front = got
    n, P = len(c["samples"]), len(c["positions"])
    assert rc == exp["rc"], (c["name"], rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], list(status[:n]), exp["status"])
    assert (status[n:] == 0xCDCDCDCD).all() and (line_start[P + 1:] == 0xCDCDCDCD).all(), c["name"]
    assert (whole[:front] == 0xCD).all(), c["name"]
    if rc == bm.OK:
        want = exp["text"]
        assert need == len(want), (c["name"], need, len(want))
        assert list(line_start[:P + 1]) == exp["line_start"], c["name"]
        got_text = whole[front:front + len(want)].tobytes()
        if got_text != want:
            at = next(i for i in range(len(want)) if got_text[i] != want[i])
            raise AssertionError((c["name"], at, got_text[max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))
        assert (whole[front + len(want):] == 0xCD).all(), c["name"]
    else:
        assert (whole == 0xCD).all() and (line_start == 0xCDCDCDCD).all(), c["name"]
        assert need in (None, 0), (c["name"], need)


def room_of(c):
    return None if tm.expected(c)["rc"] == bm.OK else 256


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_case_of_the_binary_catalogue(ctx, c, device):
    check(c, run(ctx, c, device, room=room_of(c)))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("c", TEXT_CASES, ids=lambda c: c["name"])
def test_every_case_of_the_text_form(ctx, c, device):
    check(c, run(ctx, c, device, shift=1))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_seeded_random_cases(ctx, device):
    assert len(bc.RANDOM_SEEDS) == 40
    for seed in bc.RANDOM_SEEDS:
        c = bc.random_case(seed)
        check(c, run(ctx, c, device, room=room_of(c), shift=seed % 2))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_two_step_call(ctx, device):
    """text_cap 0 reports the size and writes nothing; the reported size then takes the lines; a byte less is refused again."""
    c = next(x for x in TEXT_CASES if x["name"] == "text: 129 samples")
    exp = tm.expected(c)
    for cap in (0, len(exp["text"]) - 1):
        rc, whole, line_start, status, need, _ = run(ctx, c, device, cap=cap, shift=1)
        assert rc == bm.BAM_MORE and need == len(exp["text"])
        assert (whole == 0xCD).all() and (line_start == 0xCDCDCDCD).all()
        assert list(status[:len(c["samples"])]) == exp["status"]
    check(c, run(ctx, c, device, cap=need, shift=1))
    # and the binding's own two calls (no buffer given)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    rc, text, ls, st, need = ctx.bam_pileup_text(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref)
    assert rc == 0 and text.tobytes() == exp["text"] and list(ls) == exp["line_start"] and need == len(exp["text"])


def test_the_refusals_leave_text_and_line_start_untouched(ctx):
    c = next(x for x in TEXT_CASES if x["name"] == "an insertion on an odd and on an even nibble")
    exp = tm.expected(c)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    L, h = ctx._L, ctx._h
    need = C.c_int64(0)
    text = np.full(len(exp["text"]) + GUARD, 0xCD, dtype=np.uint8)
    ls = np.full(len(pos) + 1, 0xCDCDCDCD, dtype=np.uint32)
    st = np.zeros(2, dtype=np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    good = [h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), c["beg0"], c["end0"], c["min_mapq"], len(pos), p(pos), c["rg_s"], p(ref), len(ref), p(text),
            len(exp["text"]), C.byref(need), p(ls), p(st), 0]
    untouched = lambda: (text == 0xCD).all() and (ls == 0xCDCDCDCD).all()
    for i in (2, 4, 5, 6, 7, 12, 14, 16, 18, 19, 20):               # each pointer null with work present
        bad = list(good)
        bad[i] = None
        assert L.bvc_bam_pileup_text(*bad) == bm.ERR_ARG and untouched(), i
    for i in (1, 3, 11, 15, 17):                                    # each size negative
        bad = list(good)
        bad[i] = -1
        assert L.bvc_bam_pileup_text(*bad) == bm.ERR_ARG and untouched(), i
    for k, arr in ((12, pos[::-1].copy()), (12, np.concatenate([pos[:3], pos[2:-1]])), (4, off[::-1].copy()), (5, end + 1)):
        bad = list(good)                                            # positions that do not strictly ascend, sample ranges out of order / past the buffer
        bad[k] = p(arr)
        assert L.bvc_bam_pileup_text(*bad) == bm.ERR_ARG and untouched(), k
    assert L.bvc_bam_pileup_text(*good) == bm.OK and need.value == len(exp["text"])       # the context stays usable
    assert text[:need.value].tobytes() == exp["text"] and (text[need.value:] == 0xCD).all() and list(ls) == exp["line_start"]


def test_a_second_call_of_the_same_shape_allocates_nothing_and_gives_the_same_bytes(ctx):
    import torch
    c = next(x for x in TEXT_CASES if x["name"] == "text: 1025 positions")
    exp = tm.expected(c)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], dev(ref)]
    outs = [(torch.zeros(len(exp["text"]), dtype=torch.uint8, device="cuda"), torch.zeros(len(pos) + 1, dtype=torch.int32, device="cuda"),
             torch.zeros(len(rid), dtype=torch.int32, device="cuda")) for _ in range(2)]
    free = []
    for text, ls, st in outs:
        rc = ctx.bam_pileup_text(*args, text=text, line_start=ls, sample_status=st)[0]
        ctx.synchronize()
        assert rc == 0
        free.append(torch.cuda.mem_get_info()[0])
    # the library allocates device memory of its own (not torch's pool): what is free on the device after the first call stays free
    assert free[1] == free[0], free
    for text, ls, _ in outs:
        assert text.cpu().numpy().tobytes() == exp["text"] and list(ls.cpu().numpy().view(np.uint32)) == exp["line_start"]


# ---- the 100 test BAMs, from their BGZF blocks ----------------------------------------------------------------------------------------
def test_the_test_bams_from_their_blocks_a_damaged_block_a_failing_crc_and_a_short_sample(ctx):
    """Every 13th position of the region, the 100 test BAMs' own BGZF blocks: the lines are the model's, byte for byte.  A payload byte
    flipped and a CRC32 that does not match are BVC_ERR_DATA naming the block; a sample cut short without its end of file is BVC_BAM_MORE."""
    from basevarc_amd import lib as bl
    from basevarc_amd.lib import BvcError
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
    from tests.test_gpu_bam_pileup import bgzf_blocks_of
    contig, beg0, end0, mapq, pv, rg_s, refseq = bam_data_call()
    pv = pv[::13]
    data = bam_data_bytes()
    comp, table, off, end = bytearray(), [], [], []
    files = [l.strip().replace("data/", "", 1) for l in open(os.path.join(hostref.DATA, "bam.list")) if l.strip()]
    out_at = 0
    for f, (d, first, _) in zip(files, data):
        raw = open(os.path.join(hostref.DATA, f), "rb").read()
        off.append(out_at + first)
        for co, cl, isz, crc in bgzf_blocks_of(raw):
            table.append((len(comp) + co, out_at, cl, isz, crc, 1))
            out_at += isz
        end.append(out_at)
        comp += raw
    tab = np.array(table, dtype=bl.BLOCK_DTYPE)
    rid = [refs.index(contig) for _, _, refs in data]
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    assert exp["rc"] == 0
    want, want_ls = tm.lines(exp["maps"], pv)
    assert len(want) > 1000000
    eof = np.ones(len(data), dtype=np.uint8)
    ref = np.frombuffer(refseq.encode(), dtype=np.uint8)
    comp = np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8)
    call = lambda comp, tab, end, eof: ctx.bam_pileup_text_bgzf(comp, tab, out_at, off, end, eof, rid, beg0, end0, mapq, pv, rg_s, ref)
    rc, text, ls, st, need = call(comp, tab, end, eof)
    assert rc == 0 and need == len(want) and list(st[:len(data)]) == exp["status"]
    assert text.tobytes() == want and list(ls) == want_ls
    # one payload byte of a block in the middle flipped: the block fails to inflate or fails its CRC32
    k = len(tab) // 2
    bad = comp.copy()
    bad[int(tab[k]["comp_off"]) + int(tab[k]["comp_len"]) // 2] ^= 0x5A
    with pytest.raises(BvcError, match=f"BGZF block {k}: ") as e:
        call(bad, tab, end, eof)
    assert e.value.status == bm.ERR_DATA
    # good bytes under a CRC32 that is not theirs
    bad_tab = tab.copy()
    bad_tab[k]["crc32"] ^= 1
    with pytest.raises(BvcError, match=f"BGZF block {k}: CRC32 mismatch") as e:
        call(comp, bad_tab, end, eof)
    assert e.value.status == bm.ERR_DATA
    # sample 3 ends inside its records and is not said to end its file: more bytes are wanted, nothing is written
    short_end, short_eof = list(end), eof.copy()
    short_end[3], short_eof[3] = off[3] + 5000, 0
    guard = np.full(len(want), 0xCD, dtype=np.uint8)
    guard_ls = np.full(len(pv) + 1, 0xCDCDCDCD, dtype=np.uint32)
    rc, _, _, st, need = ctx.bam_pileup_text_bgzf(comp, tab, out_at, off, short_end, short_eof, rid, beg0, end0, mapq, pv, rg_s, ref, text=guard,
                                                  line_start=guard_ls)
    assert rc == bm.BAM_MORE and need == 0 and st[3] == 2 and (guard == 0xCD).all() and (guard_ls == 0xCDCDCDCD).all()
    rc, text, ls, _, _ = call(comp, tab, end, eof)                  # the context stays usable
    assert rc == 0 and text.tobytes() == want and list(ls) == want_ls
