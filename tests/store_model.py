"""Plain Python models of include/bvc_store.h: bvc_store_tile's arithmetic, the layout of the tile buffer bvc_pileup_begin_store fills, and
a maker of batches of binary temp-batch records (entries through tests/bam_pileup_model.entry_bytes, the host program's bin_batch_entry)."""
import struct

import numpy as np

from tests import bam_pileup_model as bm

LIMIT = 0xFFFFFF00


def cum_of(rec_starts):
    """cum[t] = the sum over the batches of rec_start[t] (what every put adds on the device)."""
    return np.sum(np.asarray(rec_starts, dtype=np.int64), axis=0) if len(rec_starts) else None


def tile(cum, n_batches, t0, max_positions, max_bytes):
    """bvc_store_tile: (T, bytes) -- the largest T <= min(max_positions, n_positions - t0) with cum[t0 + T] - cum[t0] + 16 * n_batches <=
    max_bytes, at least 1, by plain search."""
    n_positions = len(cum) - 1
    assert 0 <= t0 < n_positions and max_positions >= 1
    best = 1
    for T in range(1, min(max_positions, n_positions - t0) + 1):
        if int(cum[t0 + T]) - int(cum[t0]) + 16 * n_batches <= max_bytes:
            best = T
    return best, int(cum[t0 + best]) - int(cum[t0]) + 16 * n_batches


def row_bytes(n_positions):
    """Bytes of a kept batch's rec_start row in its allocation: its records begin behind them, on a 16-byte boundary."""
    return ((n_positions + 1) * 4 + 15) // 16 * 16


def gathered(batches, t0, T):
    """The tile buffer and table of positions [t0, t0 + T) of batches = [(records, rec_start)]: slice b lies at the first offset behind
    slice b - 1 that is congruent mod 16 to where it lies in its batch's records (which begin on a 16-byte boundary).  Returns
    ([(dst, slice bytes)], rows [nb, T + 1] uint32, bytes in use)."""
    cursor, places = 0, []
    rows = np.zeros((len(batches), T + 1), dtype=np.uint32)
    for b, (rec, rs) in enumerate(batches):
        lo, hi = int(rs[t0]), int(rs[t0 + T])
        cursor += (lo - cursor) % 16
        places.append((cursor, bytes(rec[lo:hi])))
        rows[b] = cursor + (np.asarray(rs[t0:t0 + T + 1], dtype=np.int64) - lo)
        cursor += hi - lo
    return places, rows, cursor


def sliced(batches, t0, T):
    """The same positions as bvc_pileup_begin_bin takes them from the host: the slices one behind the other, rows [nb, T + 1]."""
    data = bytearray()
    rows = np.zeros((len(batches), T + 1), dtype=np.uint32)
    for b, (rec, rs) in enumerate(batches):
        lo, hi = int(rs[t0]), int(rs[t0 + T])
        rows[b] = len(data) + (np.asarray(rs[t0:t0 + T + 1], dtype=np.int64) - lo)
        data += rec[lo:hi]
    return bytes(data), rows


def base_entry(rng):
    return dict(base=int(rng.integers(0, 5)), mapq=int(rng.integers(0, 61)), qual=int(rng.integers(0, 42)), rpr=int(rng.integers(0, 256)),
                strand=int(rng.integers(0, 2)), is_indel=0)


def indel_entry(rng, n_text):
    text = ("+" if rng.integers(0, 2) else "-") + "".join("ACGT"[i] for i in rng.integers(0, 4, size=n_text - 1))
    return dict(base=5, mapq=int(rng.integers(0, 61)), qual=int(rng.integers(0, 61)), rpr=0, strand=int(rng.integers(0, 2)), is_indel=1, indel=text)


def record(entries):
    """entries: [(sample in batch, entry dict)] in sample order -> one record."""
    payload = b"".join(bm.entry_bytes(e, s) for s, e in entries)
    return struct.pack("<I", len(payload)) + payload


def batch_of(records, filler=0):
    """(records bytes, rec_start) of a batch whose records are `records`, with `filler` bytes that no record owns in front."""
    out = bytearray(b"\xEE" * filler)
    rs = []
    for r in records:
        rs.append(len(out))
        out += r
    rs.append(len(out))
    return bytes(out), np.array(rs, dtype=np.uint32)


def random_batch(rng, n_in, T, density=0.5, indel_rate=0.1, filler=0):
    recs = []
    for _ in range(T):
        ent = []
        for s in range(n_in):
            if rng.random() < density:
                ent.append((s, indel_entry(rng, int(rng.integers(1, 12))) if rng.random() < indel_rate else base_entry(rng)))
        recs.append(record(ent))
    return batch_of(recs, filler)


def sized_record(rng, size, indel_at=None, indel_text=None):
    """One record of exactly `size` bytes (>= 4 + 9 + 12): base entries of ascending samples and one indel entry whose text makes up the
    rest -- or, with indel_at / indel_text, an indel entry of indel_text bytes of text whose entry begins indel_at bytes into the record
    (rounded down to a whole base entry) and base entries behind it up to about `size`.  Returns (record, samples it needs)."""
    ent = []
    if indel_at is None:
        k = (size - 4 - 11 - 1) // 9
        n_text = size - 4 - 11 - 9 * k
        while n_text > 0xffff:
            k += 1
            n_text -= 9
        ent = [(s, base_entry(rng)) for s in range(k)] + [(k, indel_entry(rng, n_text))]
        rec = record(ent)
        assert len(rec) == size, (len(rec), size)
        return rec, k + 1
    k = (indel_at - 4) // 9
    ent = [(s, base_entry(rng)) for s in range(k)] + [(k, indel_entry(rng, indel_text))]
    more = max(0, (size - 4 - 9 * k - 11 - indel_text) // 9)
    ent += [(k + 1 + s, base_entry(rng)) for s in range(more)]
    return record(ent), k + 1 + more
