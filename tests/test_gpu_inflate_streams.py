"""GPU: csrc/inflate_kernel.hip (inflate_kernel and crc32_kernel) on the hand-built deflate streams of tests/deflate_streams.py.

What zlib's compressor never emits, and what the kernel's hand-written symbol loop must still take or refuse: see the catalogue
and its census (tests/test_deflate_streams.py demands that the valid streams reach every path class of the kernel).  All through
Context.inflate_blocks (host pointers).  The times in the comments are one run on an MI355X: a budget, not a criterion.
"""
import zlib

import numpy as np
import pytest

from tests import deflate_streams as S
from tests import deflate_writer as W

pytestmark = pytest.mark.gpu

ERR_CRC = 10


@pytest.fixture(scope="module")
def ctx():
    from basevarc_amd import Context
    c = Context(0)
    yield c
    c.close()


class Payloads:
    """Payloads laid into one buffer at chosen alignments, with chosen bytes between them."""

    def __init__(self):
        self.comp = bytearray()
        self.blocks = []

    def add(self, comp, isize, crc=None, lead=None, filler=b"\xA5"):
        """lead: the payload's offset modulo 4 (None: wherever the buffer ends); filler: the byte in front of and behind it."""
        if lead is not None:
            self.comp += filler * ((lead - len(self.comp)) % 4)
        self.blocks.append((len(self.comp), len(comp), isize) if crc is None else (len(self.comp), len(comp), isize, crc))
        self.comp += comp
        self.comp += filler * 5                                   # (the words the kernel loads behind a payload hold these)

    def run(self, ctx):
        got, status = ctx.inflate_blocks(bytes(self.comp), self.blocks)
        return got, [int(v) for v in status]


def crc_of(data):
    return zlib.crc32(data) & 0xFFFFFFFF


def test_valid_streams_at_every_payload_alignment(ctx):
    """Every valid stream, at each of the four alignments of its payload, gives status 0 and exactly its data; two blocks in three
    carry their CRC32."""
    # 543 streams (24 of them random, up to 40 KiB: deflate_streams.N_RANDOM) x 4 alignments = 2172 blocks, 10.5 MB of output: 1.1 s
    p, want = Payloads(), []
    for s in S.valid():
        for lead in range(4):
            p.add(s.comp, s.isize, crc_of(s.data) if len(p.blocks) % 3 else None, lead=lead, filler=b"\xFF" if lead & 1 else b"\x00")
            want.append(s)
    got, status = p.run(ctx)
    bad = [(s.name, i % 4, st) for i, (s, g, st) in enumerate(zip(want, got, status)) if st != 0 or g != s.data]
    assert not bad, (len(bad), bad[:12])
    assert len(want) > 2000


def test_refused_streams_and_their_neighbours(ctx):
    """Every stream to be refused comes back with a non-zero status -- the kernel's own code where it has one unambiguous code for
    the reason -- at every alignment and with 0x00 and 0xFF behind it, and the good blocks between them stay byte-exact."""
    # 74 streams x 4 alignments x 2 fillers, a good block after every one: 1184 blocks: 1.1 s
    good = [s for s in S.valid() if 0 < s.isize <= 2000]
    p, want = Payloads(), []
    for s in S.refused():
        for lead in range(4):
            for filler in (b"\x00", b"\xFF"):
                p.add(s.comp, s.isize, crc_of(s.data) if s.data is not None and len(s.data) == s.isize else None, lead=lead, filler=filler)
                want.append(s)
                g = good[len(want) % len(good)]
                p.add(g.comp, g.isize, crc_of(g.data), filler=filler)
                want.append(g)
    got, status = p.run(ctx)
    bad = []
    for s, g, st in zip(want, got, status):
        if s.reason is None:
            if st != 0 or g != s.data:
                bad.append((s.name, "good neighbour", st))
        elif st == 0 or (s.err is not None and st != s.err):
            bad.append((s.name, s.reason, st, s.err))
    assert not bad, (len(bad), bad[:12])


def test_truncated_streams_against_zero_and_nonzero_neighbours(ctx):
    """Every byte prefix of four streams, followed in the buffer by 0x00 bytes and by 0xFF bytes (the words the kernel loads hold the
    neighbour's bytes inside the payload's last word, zeros behind it), at every alignment: never status 0."""
    # 557 prefixes x 2 fillers x 4 alignments = 4456 blocks and a good one after every eighth: 1.1 s
    good = [s for s in S.valid() if 0 < s.isize <= 2000]
    p, want = Payloads(), []
    for name, prefix, isize in S.truncations():
        for filler in (b"\x00", b"\xFF"):
            for lead in range(4):
                p.add(prefix, isize, lead=lead, filler=filler)
                want.append((name, None))
                if len(want) % 8 == 0:
                    g = good[len(want) % len(good)]
                    p.add(g.comp, g.isize, crc_of(g.data), filler=filler)
                    want.append((g.name, g.data))
    got, status = p.run(ctx)
    bad = [(name, i, st) for i, ((name, data), g, st) in enumerate(zip(want, got, status))
           if (st == 0 if data is None else (st != 0 or g != data))]
    assert not bad, (len(bad), bad[:12])


def test_second_trip_of_the_block_loop(ctx):
    """One call of 65536 + 4096 blocks: the launch has 65536 workgroups, so the wavefront of block i decodes block i + 65536 next --
    with whatever the first left in its registers, its ring and its tables.  For the first 4096 indices the two are, in turn,
    valid then valid, valid then refused, refused then valid and refused then refused; every block's status and bytes are
    compared, CRC checks on (crc32_kernel makes the same second trip)."""
    # 69632 blocks of at most 64 bytes of output, 177 valid and 57 refused streams cycled, 2.7 MB of payload: 1.2 s
    V, R = S.small()
    assert len(V) >= 150 and len(R) >= 50
    n = 65536 + 4096
    p, want = Payloads(), []
    for i in range(n):
        j = i - 65536
        if i < 4096:
            s = V[(i * 7) % len(V)] if i % 4 in (0, 1) else R[(i * 5) % len(R)]
        elif j >= 0:
            s = V[(j * 11 + 3) % len(V)] if j % 4 in (0, 2) else R[(j * 3 + 1) % len(R)]
        else:
            s = V[i % len(V)] if i % 3 else R[i % len(R)]
        p.add(s.comp, s.isize, crc_of(s.data) if s.reason is None else 0, lead=(i // 4 + i // 65536) % 4, filler=b"\xFF" if i & 1 else b"\x00")
        want.append(s)
    got, status = p.run(ctx)
    bad = []
    for i, (s, g, st) in enumerate(zip(want, got, status)):
        if s.reason is None:
            if st != 0 or g != s.data:
                bad.append((i, s.name, st))
        elif st == 0 or (s.err is not None and st != s.err):
            bad.append((i, s.name, st, s.err))
    assert not bad, (len(bad), bad[:12])
    orders = {(want[i].reason is None, want[i + 65536].reason is None) for i in range(4096)}
    assert len(orders) == 4


CRC_SIZES = list(range(0, 131)) + list(range(1008, 1041)) + list(range(4080, 4113)) + list(range(65520, 65537))


def _crc_layout(cases):
    """cases: (isize, residue of out_off modulo 16, crc xor).  Stored blocks, each behind a filler block of 1..15 bytes (its own CRC
    right) where that is needed to bring out_off to the residue.  Returns (Payloads, [(data or None for a filler's, crc xor)])."""
    rng = np.random.default_rng(3)
    payload = {}                                                  # one payload per size: (offset, length, data)
    p = Payloads()

    def stream_of(n):
        if n not in payload:
            data = rng.bytes(n) if n else b""
            s = W.build("stored", [W.stored(data[:65535])] + ([W.stored(data[65535:])] if n > 65535 else []))
            assert s.data == data
            payload[n] = (len(p.comp), len(s.comp), data)
            p.comp += s.comp + b"\0" * 3
        return payload[n]
    at, want = 0, []
    for n, residue, flip in cases:
        f = (residue - at) % 16
        if f:
            off, length, data = stream_of(f)
            p.blocks.append((off, length, f, crc_of(data)))
            want.append((data, 0))
            at += f
        assert at % 16 == residue                                 # (outputs lie one after the other: this is the block's out_off)
        off, length, data = stream_of(n)
        p.blocks.append((off, length, n, crc_of(data) ^ flip))
        want.append((data, flip))
        at += n
    return p, want


def _check_crc(ctx, cases):
    p, want = _crc_layout(cases)
    got, status = p.run(ctx)
    bad = [(len(data), flip, st) for (data, flip), g, st in zip(want, got, status) if st != (ERR_CRC if flip else 0) or g != data]
    assert not bad, (len(bad), bad[:12])


def test_crc32_kernel_right_crc_at_every_residue(ctx):
    """Stored blocks of 0..130, 1008..1040, 4080..4112 and 65520..65536 bytes with out_off at every residue modulo 16 (the kernel cuts
    a block into slices at absolute 16-byte boundaries): the right CRC32 gives status 0; ISIZE 0 with CRC 0 is accepted."""
    # 214 sizes x 16 residues and their fillers, 20 MB of output: 0.04 s
    _check_crc(ctx, [(n, r, 0) for n in CRC_SIZES for r in range(16)])


def test_crc32_kernel_any_flipped_bit_is_status_10(ctx):
    """The same with one bit of the CRC32 flipped: status 10, whichever bit -- all 32 for every size up to 130, the bit changing from
    block to block for the rest (every residue up to 4112 bytes, four of them for the 64 KiB blocks)."""
    # 4192 + 3220 blocks and their fillers, 7 MB of output: 0.11 s
    cases = [(n, n % 16, 1 << bit) for n in range(0, 131) for bit in range(32)]
    k = 0
    for n in CRC_SIZES:
        for r in (range(16) if n < 65520 else (0, 1, 8, 15)):
            cases.append((n, r, 1 << (k % 32)))
            k += 1
    _check_crc(ctx, cases)
