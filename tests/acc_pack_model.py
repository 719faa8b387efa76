"""Plain numpy model of include/bvc_site_acc_pack.h and of docs/COUNTS_FILES.md: dense arrays of each kind of accumulator <-> logical rows
<-> (row_start, cell, count) entries, the verdict of bvc_site_acc_add_packed on a piece, and a writer and a reader of the host program's
counts files written from the document alone.  No device, no library."""
import struct

import numpy as np

TW = 12                                            # words of a bvc_bam_site_tally; the first 10 are part of the logical row
OK, ERR_ARG, ERR_DATA, ACC_MORE = 0, -1, -5, 2
FAULT_ROW_START, FAULT_CELL, FAULT_ORDER, FAULT_QUAL = 1, 2, 3, 4


def row_words(slots=1, depth_groups=0):
    """W of the logical row."""
    return slots * 512 + 10 + 4 * depth_groups


def logical_rows(counts, tally, depth=None):
    """Dense arrays -> uint32 [n, W].  counts: [n, 512] or [n, slots, 512] (wide), or [n, 4, n_quals] (narrow); tally: anything that views
    as [n, 12] words; depth: [n, depth_groups, 4] or None."""
    counts = np.asarray(counts, dtype=np.uint32)
    n = counts.shape[0]
    if counts.ndim == 3 and counts.shape[1] == 4 and counts.shape[2] <= 128 and counts.shape[2] != 512:
        wide = np.zeros((n, 4, 128), dtype=np.uint32)
        wide[:, :, :counts.shape[2]] = counts
        c = wide.reshape(n, 512)
    else:
        c = counts.reshape(n, int(np.prod(counts.shape[1:])))
    assert c.shape[1] % 512 == 0
    t = np.ascontiguousarray(tally).view(np.uint32).reshape(n, TW)[:, :10]
    parts = [c, t]
    if depth is not None:
        depth = np.asarray(depth, dtype=np.uint32)
        parts.append(depth.reshape(n, int(np.prod(depth.shape[1:]))))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


def dense(rows, slots=1, depth_groups=0, n_quals=None):
    """Logical rows [n, W] -> (counts, tally words [n, 12], depth or None): counts [n, slots, 512] ([n, 512] for one slot), or narrow
    [n, 4, n_quals] -- a count in a column >= n_quals is a ValueError."""
    rows = np.asarray(rows, dtype=np.uint32)
    n, cc = rows.shape[0], slots * 512
    assert rows.shape[1] == row_words(slots, depth_groups)
    counts = rows[:, :cc].reshape(n, slots, 512) if slots > 1 else rows[:, :cc].copy()
    if n_quals is not None:
        wide = rows[:, :512].reshape(n, 4, 128)
        if wide[:, :, n_quals:].any():
            raise ValueError("a count in a column >= n_quals")
        counts = np.ascontiguousarray(wide[:, :, :n_quals])
    tally = np.zeros((n, TW), dtype=np.uint32)
    tally[:, :10] = rows[:, cc:cc + 10]
    depth = rows[:, cc + 10:].reshape(n, depth_groups, 4).copy() if depth_groups else None
    return np.ascontiguousarray(counts), tally, depth


def entries(rows):
    """Logical rows -> (row_start int64 [n + 1], cell uint16, count uint32): the non-zero words, rows ascending, cells ascending."""
    rows = np.asarray(rows, dtype=np.uint32)
    n = rows.shape[0]
    r, c = np.nonzero(rows)                          # (row-major: rows ascending, then cells ascending)
    row_start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=row_start[1:])
    return row_start, c.astype(np.uint16), rows[r, c].astype(np.uint32)


def verdict(row_start, cell, count, n, W, n_quals=128, count_cells=512):
    """None for a sound piece of n rows, else (first row at fault, its fault) as bvc_site_acc_add_packed judges it."""
    rs = [int(x) for x in row_start]
    ne = len(cell)
    for t in range(n):
        a, b = rs[t], rs[t + 1]
        if (t == 0 and a != 0) or a < 0 or b < a or b > ne or (t == n - 1 and b != ne):
            return t, FAULT_ROW_START
        for i in range(a, b):
            c = int(cell[i])
            if c >= W:
                return t, FAULT_CELL
            if i > a and c <= int(cell[i - 1]):
                return t, FAULT_ORDER
            if c < count_cells and (c & 127) >= n_quals:
                return t, FAULT_QUAL
    return None


def add_entries(rows, row_start, cell, count, t0=0):
    """rows [t0 + t] += the piece's entries, modulo 2^32 (a sound piece; in place)."""
    for t in range(len(row_start) - 1):
        a, b = int(row_start[t]), int(row_start[t + 1])
        np.add.at(rows[t0 + t], np.asarray(cell[a:b], dtype=np.int64), np.asarray(count[a:b], dtype=np.uint32))
    return rows


def concat(pieces):
    """Pieces of consecutive row ranges -> the piece of their union."""
    rs, at = [np.zeros(1, dtype=np.int64)], 0
    for p in pieces:
        rs.append(np.asarray(p[0][1:], dtype=np.int64) + at)
        at += int(p[0][-1])
    return np.concatenate(rs), np.concatenate([np.asarray(p[1], dtype=np.uint16) for p in pieces]), np.concatenate([np.asarray(p[2], dtype=np.uint32) for p in pieces])


# ---- the counts file, from docs/COUNTS_FILES.md ------------------------------------------------------------------------------------------
MAGIC = b"BVCCNTS\x00"
VERSION = 1
TAG_PIECE, TAG_END = 0x43454950, 0x21444E45       # "PIEC", "END!"
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def fnv1a64(data):
    h = FNV_OFFSET
    for byte in bytes(data):
        h = ((h ^ byte) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h


def positions_hash(positions):
    return fnv1a64(np.asarray(positions, dtype="<i4").tobytes())


def _s(text):
    b = text.encode() if isinstance(text, str) else bytes(text)
    return struct.pack("<I", len(b)) + b


def file_bytes(meta, pieces):
    """meta: dict(chrom, rg_s, rg_e, n_positions, pos_hash, mapq, slots, depth_groups, n_quals, groups [names], bams [(path, sample)]);
    pieces: [(t0, row_start, cell, count)]."""
    out = [MAGIC, struct.pack("<IIIIiiiiQ", VERSION, meta["slots"], meta["depth_groups"], meta["n_quals"], meta["mapq"], meta["rg_s"], meta["rg_e"],
                              meta["n_positions"], meta["pos_hash"]), _s(meta["chrom"])]
    out.append(struct.pack("<I", len(meta["groups"])))
    out += [_s(g) for g in meta["groups"]]
    out.append(struct.pack("<I", len(meta["bams"])))
    for path, sample in meta["bams"]:
        out += [_s(path), _s(sample)]
    total = 0
    for t0, rs, cell, count in pieces:
        rs, cell, count = np.asarray(rs, dtype="<i8"), np.asarray(cell, dtype="<u2"), np.asarray(count, dtype="<u4")
        out += [struct.pack("<Iiiq", TAG_PIECE, t0, len(rs) - 1, len(cell)), rs.tobytes(), cell.tobytes(), count.tobytes()]
        total += len(cell)
    out.append(struct.pack("<IIq", TAG_END, len(pieces), total))
    return b"".join(out)


class FileError(ValueError):
    pass


def parse_file(data):
    """The inverse of file_bytes: (meta, pieces).  FileError for anything the document calls truncated or damaged."""
    at = [0]

    def take(n):
        if n < 0 or at[0] + n > len(data):
            raise FileError("truncated")
        b = data[at[0]:at[0] + n]
        at[0] += n
        return b

    def string():
        (n,) = struct.unpack("<I", take(4))
        return take(n).decode()

    if take(8) != MAGIC:
        raise FileError("magic")
    version, slots, dg, nq, mapq, rg_s, rg_e, npos, h = struct.unpack("<IIIIiiiiQ", take(40))
    if version != VERSION:
        raise FileError("version")
    if not (1 <= slots <= 33 and dg <= 32 and npos >= 0):
        raise FileError("damaged: shape")
    meta = dict(slots=slots, depth_groups=dg, n_quals=nq, mapq=mapq, rg_s=rg_s, rg_e=rg_e, n_positions=npos, pos_hash=h, chrom=string())
    meta["groups"] = [string() for _ in range(struct.unpack("<I", take(4))[0])]
    meta["bams"] = [(string(), string()) for _ in range(struct.unpack("<I", take(4))[0])]
    W = row_words(slots, dg)
    pieces, total = [], 0
    while True:
        (tag,) = struct.unpack("<I", take(4))
        if tag == TAG_END:
            n_pieces, want = struct.unpack("<Iq", take(12))
            if n_pieces != len(pieces) or want != total:
                raise FileError("damaged: end mark")
            if at[0] != len(data):
                raise FileError("damaged: bytes behind the end mark")
            return meta, pieces
        if tag != TAG_PIECE:
            raise FileError("damaged: tag")
        t0, n, ne = struct.unpack("<iiq", take(16))
        if t0 < 0 or n < 0 or t0 + n > npos or ne < 0:
            raise FileError("damaged: piece header")
        rs = np.frombuffer(take((n + 1) * 8), dtype="<i8")
        cell = np.frombuffer(take(ne * 2), dtype="<u2")
        count = np.frombuffer(take(ne * 4), dtype="<u4")
        if rs[0] != 0 or rs[-1] != ne or (np.diff(rs) < 0).any() or (cell >= W).any():
            raise FileError("damaged: piece")
        pieces.append((t0, rs, cell, count))
        total += ne
