"""What the tests of include/bvc_bam_deflate.h share: a case's inflated BAM bytes cut into BGZF blocks of its own (the _bgzf calls take
blocks, the catalogue of tests/bam_pileup_cases.py gives bytes), and the piece layouts the calls are walked over.  Nothing here needs a
device."""
import zlib

import numpy as np

from tests import bam_pileup_model as bm

B = 65280                    # input bytes of a block of the encoder (include/bvc.h, BVC_BGZF_BLOCK_INPUT)
GRID = 256                   # workgroups of the encoder's block kernels at most (csrc/bvc_internal.h, kBgzfDeflateGrid)
CHUNK = 4099                 # input bytes of the blocks made here: odd, and small enough that most cases have several


def bgzf_inputs(c):
    """The arguments of a _bgzf call for a case of tests/bam_pileup_cases.case: (comp uint8, table rows for lib.BLOCK_DTYPE, bam_bytes, off,
    end, eof, rid, positions, refseq).  The case's bytes are deflated raw in blocks of CHUNK bytes, one behind the other, CRC32 checked."""
    bam, off, end, eof, rid = bm.layout(c["samples"], c["lead"])
    comp, table = bytearray(), []
    for at in range(0, len(bam), CHUNK):
        data = bytes(bam[at:at + CHUNK])
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        payload = z.compress(data) + z.flush()
        table.append((len(comp), at, len(payload), len(data), zlib.crc32(data) & 0xFFFFFFFF, 1))
        comp += payload
    return (np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8), table, len(bam), np.array(off, dtype=np.int64), np.array(end, dtype=np.int64),
            np.array(eof, dtype=np.uint8), np.array(rid, dtype=np.int32), np.array(c["positions"], dtype=np.int32),
            np.frombuffer(c["refseq"].encode(), dtype=np.uint8))


def layouts(P):
    """[(name, piece_pos)] over P positions: one piece; four near-equal pieces; four with an empty piece first, in the middle, last."""
    q = [0, P // 4, P // 2, P - P // 4, P]
    third = [0, P // 3, P - P // 3, P]
    return [("one piece", [0, P]), ("four pieces", q), ("an empty piece first", [0, 0] + third[1:]),
            ("an empty piece in the middle", third[:2] + third[1:]), ("an empty piece last", third + [P])]


def layout_of(index, P):
    """One of layouts(P), in turn by `index`: a catalogue walked with it meets every layout."""
    all_ = layouts(P)
    return all_[index % len(all_)]


def bad_layouts(P):
    """[(name, piece_pos)] that the calls refuse (P >= 2)."""
    return [("descending", [0, P, P - 1, P]), ("not ending at n_positions", [0, P - 1]), ("past n_positions", [0, P + 1]),
            ("not starting at 0", [1, P])]


# n_samples = 0: every line of the text form is "\n" and every binary record its four-byte length word, so a piece of k positions is
# exactly k (4 k) bytes -- the pieces straddle a block's 65280 input bytes
EXACT_BYTES = (1, B - 1, B, B + 1, 2 * B)


def exact_pieces(text):
    """(n_positions, piece_pos, the pieces' bytes) with n_samples = 0: pieces of 1, 65279, 65280, 65281 and 2 x 65280 bytes of lines;
    for the binary form (records of four bytes) of 4, 65276, 65280, 65284 and 2 x 65280."""
    sizes = EXACT_BYTES if text else (4, B - 4, B, B + 4, 2 * B)
    unit = 1 if text else 4
    pos = [0]
    for s in sizes:
        pos.append(pos[-1] + s // unit)
    return pos[-1], pos, list(sizes)
