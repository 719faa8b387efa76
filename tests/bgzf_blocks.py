"""A plain Python walker over BGZF blocks (SAM specification 4.1): every header field, the BSIZE chain, each block inflated on its own
with zlib -- the deflate data must end exactly at the trailer, nothing unused -- CRC32 and ISIZE.  An empty block is the end-of-file
marker: walk() fails on one, walk_file() wants exactly one, as the file's last block.  Nothing here needs a device."""
import struct
import zlib

EOF_MARKER = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
BLOCK_INPUT = 65280


def walk(buf, allow_empty=False):
    """buf: whole blocks, one after the other.  Returns [(input bytes, payload, block size)] per block."""
    buf = bytes(buf)
    out, at = [], 0
    while at < len(buf):
        assert len(buf) - at >= 26, ("a block is at least 26 bytes", at, len(buf))
        id1, id2, cm, flg, mtime, xfl, os_, xlen = struct.unpack_from("<BBBBIBBH", buf, at)
        assert (id1, id2, cm, flg) == (0x1f, 0x8b, 8, 4), (at, id1, id2, cm, flg)
        assert mtime == 0 and xfl == 0 and os_ == 0xff and xlen == 6, (at, mtime, xfl, os_, xlen)
        si1, si2, slen, bsize1 = struct.unpack_from("<BBHH", buf, at + 12)
        assert (si1, si2, slen) == (ord("B"), ord("C"), 2), (at, si1, si2, slen)
        bsize = bsize1 + 1
        assert 26 <= bsize <= 65536 and at + bsize <= len(buf), (at, bsize, len(buf))
        payload = buf[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", buf, at + bsize - 8)
        d = zlib.decompressobj(-15)
        data = d.decompress(payload)
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", ("the deflate data ends at the trailer", at, len(d.unused_data))
        assert len(data) == isize and isize <= 65536, (at, len(data), isize)
        assert zlib.crc32(data) & 0xFFFFFFFF == crc, (at, hex(crc))
        assert allow_empty or isize > 0, ("an empty block", at)
        out.append((data, payload, bsize))
        at += bsize
    return out


def walk_piece(buf, want):
    """The blocks of one piece: all but the last of exactly 65280 input bytes, none empty, together `want`."""
    blocks = walk(buf)
    assert len(blocks) == (len(want) + BLOCK_INPUT - 1) // BLOCK_INPUT, (len(blocks), len(want))
    assert all(len(b[0]) == BLOCK_INPUT for b in blocks[:-1])
    got = b"".join(b[0] for b in blocks)
    if got != want:
        first = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError(("the blocks inflate to other bytes", len(got), len(want), first))
    return blocks


def walk_file(raw):
    """A whole BGZF file: no empty block but the end-of-file marker, and that one last.  Returns the blocks in front of it."""
    raw = bytes(raw)
    assert raw[-28:] == EOF_MARKER
    return walk(raw[:-28])


def is_stored(payload):
    return (payload[0] >> 1) & 3 == 0


LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def fixed_symbols(payload):
    """The symbols of a payload that is ONE deflate block in the fixed code (RFC 1951, 3.2.6), as written: an int per literal, a
    (length, distance, length symbol, distance symbol) per match.  Fails on anything else; stops at the end-of-block symbol."""
    at = 0

    def bits(n, msb_first=False):
        nonlocal at
        v = 0
        for i in range(n):
            b = (payload[at >> 3] >> (at & 7)) & 1
            v = (v << 1) | b if msb_first else v | (b << i)
            at += 1
        return v
    assert bits(1) == 1 and bits(2) == 1, "BFINAL and the fixed code"
    out = []
    while True:
        c = bits(7, True)
        if c <= 0x17:
            sym = 256 + c
        else:
            c = (c << 1) | bits(1)
            if 0x30 <= c <= 0xBF:
                sym = c - 0x30
            elif 0xC0 <= c <= 0xC7:
                sym = 280 + c - 0xC0
            else:
                c = (c << 1) | bits(1)
                assert 0x190 <= c <= 0x1FF, hex(c)
                sym = 144 + c - 0x190
        if sym < 256:
            out.append(sym)
            continue
        if sym == 256:
            assert (at + 7) // 8 == len(payload), "the end-of-block symbol lies in the payload's last byte"
            return out
        assert sym <= 285, sym
        length = LEN_BASE[sym - 257] + bits(LEN_EXTRA[sym - 257])
        ds = bits(5, True)
        assert ds <= 29, ds
        out.append((length, DIST_BASE[ds] + bits(DIST_EXTRA[ds]), sym, ds))
