"""bvc_bam_pileup on the device (bam_pileup_kernel.hip; GPU) against the plain Python model (tests/bam_pileup_model.py, which
tests/test_bam_pileup_abi.py holds to the CPU path): every case of the hand-built catalogue and of the seeded random run, from host and
from device pointers -- records, rec_start, sample_status and the return code, with guard bytes behind the outputs; the two-step output;
the refusals; the 100 test BAMs inflated with bvc_inflate_blocks and chained through device pointers; the output through
bvc_pileup_begin_bin."""
import os
import struct

import numpy as np
import pytest

from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

pytestmark = pytest.mark.gpu

GUARD = 64
CATALOGUE = bc.catalogue()


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


def run(ctx, c, device, cap=None, room=None):
    """One call with guarded output buffers: (rc or the BvcError's status, records buffer, rec_start buffer, sample_status, needed).
    cap: the records_cap told to the library (default: the model's size); room: bytes of the records buffer in front of its guard."""
    from basevarc_amd.lib import BvcError
    exp = bc.expected(c)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    n, P = len(rid), len(pos)
    want = len(exp["records"]) if exp["records"] is not None else 0
    room = want if room is None else room
    records = np.full(room + GUARD, 0xCD, dtype=np.uint8)
    rec_start = np.full(P + 1 + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    status = np.full(n + GUARD, 0xCDCDCDCD, dtype=np.uint32)
    cap = room if cap is None else cap
    if device:
        import torch
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).cuda()
        args = [dev(a) for a in (bam, off, end, eof, rid)] + [c["beg0"], c["end0"], c["min_mapq"], dev(pos), c["rg_s"], dev(ref)]
        out = [dev(records), dev(rec_start), dev(status)]
    else:
        args = [bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref]
        out = [records, rec_start, status]
    try:
        rc, _, _, _, need = ctx.bam_pileup(*args, records=out[0], records_cap=cap, rec_start=out[1], sample_status=out[2])
    except BvcError as e:
        rc, need = e.status, None
    if device:
        ctx.synchronize()
        records, rec_start, status = out[0].cpu().numpy(), out[1].cpu().numpy().view(np.uint32), out[2].cpu().numpy().view(np.uint32)
    return rc, records, rec_start, status, need


def check(c, got):
    """What a call left, against the model: everything the model names, and nothing written anywhere else."""
    exp = bc.expected(c)
    rc, records, rec_start, status, need = got
    n, P = len(c["samples"]), len(c["positions"])
    assert rc == exp["rc"], (c["name"], rc, exp["rc"])
    assert list(status[:n]) == exp["status"], (c["name"], list(status[:n]), exp["status"])
    assert (status[n:] == 0xCDCDCDCD).all() and (rec_start[P + 1:] == 0xCDCDCDCD).all(), c["name"]
    if rc == bm.OK:
        want = exp["records"]
        assert need == len(want), (c["name"], need, len(want))
        assert list(rec_start[:P + 1]) == exp["rec_start"], c["name"]
        assert records[:len(want)].tobytes() == want, c["name"]
        assert (records[len(want):] == 0xCD).all(), c["name"]
    else:
        assert (records == 0xCD).all() and (rec_start == 0xCDCDCDCD).all(), c["name"]
        assert need in (None, 0), (c["name"], need)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("c", CATALOGUE, ids=lambda c: c["name"])
def test_every_catalogue_case(ctx, c, device):
    check(c, run(ctx, c, device, room=None if bc.expected(c)["rc"] == bm.OK else 256))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_seeded_random_cases(ctx, device):
    for seed in bc.RANDOM_SEEDS:
        c = bc.random_case(seed)
        check(c, run(ctx, c, device, room=None if bc.expected(c)["rc"] == bm.OK else 256))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_cap_one_byte_short_writes_nothing_and_the_retry_succeeds(ctx, device):
    c = next(x for x in CATALOGUE if x["name"] == "300 samples")
    want = bc.expected(c)["records"]
    rc, records, rec_start, status, need = run(ctx, c, device, cap=len(want) - 1)
    assert rc == bm.BAM_MORE and need == len(want)
    assert (records == 0xCD).all() and (rec_start == 0xCDCDCDCD).all()
    assert list(status[:len(c["samples"])]) == bc.expected(c)["status"]
    check(c, run(ctx, c, device, cap=need))
    # and the binding's own two calls (no buffer given)
    bam, off, end, eof, rid, pos, ref = arrays(c)
    rc, rec, rs, st, need = ctx.bam_pileup(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref)
    assert rc == 0 and rec.tobytes() == want and list(rs) == bc.expected(c)["rec_start"]


def test_the_same_call_twice_gives_identical_bytes(ctx):
    for name in ("300 samples", "positions over two tiles", "0, 1, 63, 64, 65 and 200 reads a sample"):
        c = next(x for x in CATALOGUE if x["name"] == name)
        a, b = run(ctx, c, True), run(ctx, c, True)
        check(c, a)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def test_the_refusals(ctx):
    from basevarc_amd.lib import BvcError
    c = next(x for x in CATALOGUE if x["name"] == "2 samples")
    bam, off, end, eof, rid, pos, ref = arrays(c)

    def refused(**kw):
        a = dict(bam=bam, off=off, end=end, eof=eof, rid=rid, pos=pos, ref=ref)
        a.update(kw)
        with pytest.raises(BvcError) as e:
            ctx.bam_pileup(a["bam"], a["off"], a["end"], a["eof"], a["rid"], c["beg0"], c["end0"], c["min_mapq"], a["pos"], c["rg_s"], a["ref"])
        assert e.value.status == bm.ERR_ARG, e.value
    refused(off=off[::-1].copy(), end=end[::-1].copy())             # the second sample in front of the first
    refused(end=end + 1)                                            # ends past the buffer (and in the next sample)
    refused(off=off - 1)                                            # starts in front of the buffer
    refused(off=end, end=off)                                       # ends in front of its start
    refused(pos=pos[::-1].copy())
    refused(pos=np.concatenate([pos[:3], pos[2:]]))                 # not strictly ascending
    L, h = ctx._L, ctx._h
    import ctypes as C
    need = C.c_int64(0)
    rs = np.zeros(len(pos) + 1, dtype=np.uint32)
    st = np.zeros(2, dtype=np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    good = [h, 2, p(bam), len(bam), p(off), p(end), p(eof), p(rid), 0, 1 << 30, 20, len(pos), p(pos), c["rg_s"], p(ref), len(ref), None, 0, C.byref(need),
            p(rs), p(st), 0]
    assert L.bvc_bam_pileup(*good) == bm.BAM_MORE and need.value == len(bc.expected(c)["records"])   # the size query itself is fine
    for i in (2, 4, 5, 6, 7, 12, 14, 18, 19, 20):                      # each pointer null with work present
        bad = list(good)
        bad[i] = None
        assert L.bvc_bam_pileup(*bad) == bm.ERR_ARG, i
    for i in (1, 3, 11, 15, 17):                                    # each size negative
        bad = list(good)
        bad[i] = -1
        assert L.bvc_bam_pileup(*bad) == bm.ERR_ARG, i
    bad = list(good)
    bad[17] = 100                                                   # room claimed for records, none given
    assert L.bvc_bam_pileup(*bad) == bm.ERR_ARG
    check(c, run(ctx, c, False))                                    # the context stays usable


def test_the_last_error_names_the_first_failing_sample(ctx):
    from basevarc_amd.lib import BvcError
    c = next(x for x in CATALOGUE if x["name"] == "block_size 31 and its kin")
    bam, off, end, eof, rid, pos, ref = arrays(c)
    with pytest.raises(BvcError, match="sample 0: truncated or corrupt BAM record"):
        ctx.bam_pileup(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref)
    c = next(x for x in CATALOGUE if x["name"] == "an empty sequence")
    bam, off, end, eof, rid, pos, ref = arrays(c)
    with pytest.raises(BvcError, match="sample 0: index offset is out of range of the sequence"):
        ctx.bam_pileup(bam, off, end, eof, rid, c["beg0"], c["end0"], c["min_mapq"], pos, c["rg_s"], ref)


# ---- the 100 test BAMs, inflated on the device -------------------------------------------------------------------------------------
def bgzf_blocks_of(raw):
    """[(payload offset, payload bytes, isize, crc32)] of a BGZF file's blocks (the empty end-of-file block left out)."""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 14] == b"BC"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        if isize:
            out.append((at + 18, bsize - 26, isize, crc))
        at += bsize
    return out


def test_the_test_bams_inflated_on_the_device_and_chained_through_device_pointers(ctx):
    """The compressed bytes of the 100 test BAMs go up once; bvc_inflate_blocks (CRC checked) leaves every file's bytes on the device --
    header and all -- and bvc_bam_pileup reads the records there, each sample from its first record to its file's end.  Every 13th
    position of the region: the records are the model's, byte for byte, and bvc_pileup_begin_bin takes them."""
    import ctypes as C
    import torch
    from basevarc_amd import lib as bl
    from tests import hostref
    from tests.test_bam_pileup_abi import bam_data_bytes, bam_data_call
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
        assert end[-1] - off[-1] == len(d) - first
    tab = np.array(table, dtype=bl.BLOCK_DTYPE)
    dev = lambda a: torch.from_numpy(a).cuda()
    d_comp = dev(np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8).copy())
    d_out = torch.zeros(out_at, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(len(tab), dtype=torch.int32, device="cuda")
    ctx._call(ctx._L.bvc_inflate_blocks, True, (d_comp, len(comp), dev(tab.view(np.uint8).copy()), len(tab), d_out, out_at, d_st))
    rid = [refs.index(contig) for _, _, refs in data]
    exp = bm.expected([(d[first:], True, r) for (d, first, _), r in zip(data, rid)], beg0, end0, mapq, pv, rg_s, refseq)
    assert exp["rc"] == 0 and len(exp["records"]) > 100000
    rc, rec, rs, st, need = ctx.bam_pileup(d_out, dev(np.array(off, dtype=np.int64)), dev(np.array(end, dtype=np.int64)),
                                           torch.ones(len(data), dtype=torch.uint8, device="cuda"), dev(np.array(rid, dtype=np.int32)), beg0, end0,
                                           mapq, dev(np.array(pv, dtype=np.int32)), rg_s, dev(np.frombuffer(refseq.encode(), dtype=np.uint8).copy()))
    ctx.synchronize()
    assert rc == 0 and (d_st.cpu().numpy() == 0).all()
    assert list(st.cpu().numpy()) == exp["status"]
    h_rec, h_rs = rec.cpu().numpy(), np.ascontiguousarray(rs.cpu().numpy().view(np.uint32))
    assert h_rec.tobytes() == exp["records"] and list(h_rs) == exp["rec_start"]
    # and the parser of the binary temp batches takes them
    ne, ni = C.c_int64(0), C.c_int64(0)
    s0, nib = np.zeros(1, dtype=np.int32), np.array([len(data)], dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert ctx._L.bvc_pileup_begin_bin(ctx._h, p(h_rec), len(h_rec), p(h_rs), p(s0), p(nib), 1, len(pv), C.byref(ne), C.byref(ni)) == 0
    assert ne.value == sum(1 for m in exp["maps"] for e in m.values() if e["is_indel"] or e["base"] != 4)
    assert ni.value == sum(1 for m in exp["maps"] for e in m.values() if e["is_indel"])
