"""BAM files, their .bai indexes and an indexed reference written from read dicts (plain Python, no device; test infrastructure).
The records are tests/bam_pileup_model.pack_record's, the framing is BGZF with zlib's raw deflate, the index follows the SAM
specification 5.2 with samtools' conventions where the committed fixtures (tests/golden/testdata/bam100/*.bam.bai) show them: only mapped
reads enter the linear index, a window without alignments takes the offset of the next window that has one (the windows in front of a
reference's first read therefore hold its first read's offset, never 0), and each reference with reads carries the pseudo-bin 37450."""
import struct
import zlib

from tests import bam_pileup_model as bm
from tests.golden import make_testdata_pileup as tp

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PSEUDO_BIN = 37450
ONE_RECORD = "record"          # write_bam(block_payload=ONE_RECORD): the header in blocks of its own, then every record in one of its own


def bgzf_block(payload, level=6):
    """One BGZF block around `payload` (at most 0xff00 bytes, so that a stored block still fits the 16-bit BSIZE)."""
    assert len(payload) <= 0xff00
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    bsize = 18 + len(data) + 8
    assert bsize <= 0x10000
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + data +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def header_bytes(sample, refs):
    """magic, header text and the reference table: everything in front of the first record"""
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs) + f"@RG\tID:rg_{sample}\tSM:{sample}\n"
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, l in refs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return out


def write_bam(path, sample, refs, reads, block_payload=0xff00, level=6):
    """refs: [(name, length)]; reads: read dicts in file order (bam_pileup_model.make_read; ref_id is theirs).  The uncompressed stream is
    cut into blocks of at most block_payload bytes wherever that falls, inside a record too; ONE_RECORD cuts at the records instead.
    Returns the records' virtual offsets and, as the last element, the virtual offset behind the last record."""
    head = header_bytes(sample, refs)
    recs = [bm.pack_record(r) for r in reads]
    starts, at = [], len(head)
    for r in recs:
        starts.append(at)
        at += len(r)
    starts.append(at)
    stream = head + b"".join(recs)
    if block_payload == ONE_RECORD:
        cuts = [0] + [s for s in starts[:-1]] + [len(stream)]
        pieces = []
        for a, b in zip(cuts, cuts[1:]):
            pieces += [(k, min(b, k + 0xff00)) for k in range(a, b, 0xff00)]
    else:
        assert 1 <= block_payload <= 0xff00
        pieces = [(k, min(len(stream), k + block_payload)) for k in range(0, len(stream), block_payload)]
    block_at, ustart = [], []                       # per block: its file offset, its first byte in the stream
    with open(path, "wb") as f:
        for a, b in pieces:
            block_at.append(f.tell())
            ustart.append(a)
            f.write(bgzf_block(stream[a:b], level))
        end_of_blocks = f.tell()
        f.write(EOF_BLOCK)
    voffs, k = [], 0
    for s in starts:
        # (a record that begins where a block ends begins at offset 0 of the next one, as bgzf_tell says it after the block is flushed)
        while k + 1 < len(ustart) and ustart[k + 1] <= s:
            k += 1
        if s == len(stream) and (not pieces or pieces[-1][1] == s):
            voffs.append(end_of_blocks << 16)
        else:
            voffs.append((block_at[k] << 16) | (s - ustart[k]))
    return voffs


# ---- walking a BAM's blocks: every record with the virtual offsets around it -----------------------------------------------------------
def walk_bam(path):
    """(n_ref, [(ref_id, pos, end, flag, voff, voff_end, offset in the inflated stream)]) in file order.  voff is where the record's
    block_size word begins; a record that begins exactly at a block's end is given offset 0 of the next block, as bgzf_tell reports
    it.  end: bam_endpos (pos + 1 for an unmapped read or one without reference-consuming operations)."""
    raw = open(path, "rb").read()
    blocks, at = [], 0                                # (file offset, payload)
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 14] == b"BC"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        blocks.append((at, zlib.decompress(raw[at + 18:at + bsize - 8], -15)))
        at += bsize
    d = b"".join(p for _, p in blocks)
    ustart, u = [], 0
    for _, p in blocks:
        ustart.append(u)
        u += len(p)

    def voff_of(s, k0):
        k = k0
        while k + 1 < len(blocks) and ustart[k + 1] <= s:
            k += 1
        return (blocks[k][0] << 16) | (s - ustart[k]), k
    assert d[:4] == b"BAM\x01"
    off = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref = struct.unpack_from("<i", d, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 8 + struct.unpack_from("<i", d, off)[0]
    out, k = [], 0
    while off < len(d):
        bs = struct.unpack_from("<i", d, off)[0]
        ref_id, pos, l_rn, _mq, _bin, n_cig, flag, _l_seq = struct.unpack_from("<iiBBHHHi", d, off + 4)
        span = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", d, off + 36 + l_rn) if "MIDNSHP=X"[c & 15] in "MDN=X")
        end = pos + span if span and not flag & 4 else pos + 1
        v0, k = voff_of(off, k)
        v1, _ = voff_of(off + 4 + bs, k)
        out.append((ref_id, pos, end, flag, v0, v1, off))
        off += 4 + bs
    return n_ref, out


# ---- the index (SAM specification 5.2) -------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def linear_index(records, n_ref):
    """Per reference the ioffsets: per 16 kbp window the smallest virtual offset of a mapped alignment overlapping it, windows without one
    filled from the next window that has one; as many windows as the last covered one needs."""
    out = [[] for _ in range(n_ref)]
    for ref_id, pos, end, flag, v0, _, _ in records:
        if ref_id < 0 or flag & 4:
            continue
        lin = out[ref_id]
        lo, hi = pos >> 14, (end - 1) >> 14
        lin += [None] * (hi + 1 - len(lin))
        for w in range(lo, hi + 1):
            if lin[w] is None or v0 < lin[w]:
                lin[w] = v0
    for lin in out:
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] is None:
                lin[w] = lin[w + 1]
    return out


def bin_index(records, n_ref):
    """Per reference {bin: [(chunk_beg, chunk_end)]}: records of one bin that follow each other in the file share a chunk; placed unmapped
    reads are binned too.  The pseudo-bin holds (first offset, last offset), (mapped, unmapped)."""
    out = [dict() for _ in range(n_ref)]
    last_bin = [None] * n_ref
    for ref_id, pos, end, flag, v0, v1, _ in records:
        if ref_id < 0:
            continue
        b = reg2bin(pos, end)
        chunks = out[ref_id].setdefault(b, [])
        if last_bin[ref_id] == b and chunks and chunks[-1][1] == v0:
            chunks[-1] = (chunks[-1][0], v1)
        else:
            chunks.append((v0, v1))
        last_bin[ref_id] = b
        meta = out[ref_id].setdefault(PSEUDO_BIN, [(v0, v1), (0, 0)])
        meta[0] = (meta[0][0], v1)
        meta[1] = (meta[1][0] + (0 if flag & 4 else 1), meta[1][1] + (1 if flag & 4 else 0))
    return out


def write_bai(path, bam_path):
    """The .bai of a BAM written here (or of any coordinate-sorted BAM), from a walk of its blocks."""
    n_ref, records = walk_bam(bam_path)
    lin, bins = linear_index(records, n_ref), bin_index(records, n_ref)
    out = b"BAI\x01" + struct.pack("<i", n_ref)
    for r in range(n_ref):
        out += struct.pack("<i", len(bins[r]))
        for b, chunks in bins[r].items():
            out += struct.pack("<Ii", b, len(chunks)) + b"".join(struct.pack("<QQ", a, e) for a, e in chunks)
        out += struct.pack("<i", len(lin[r])) + b"".join(struct.pack("<Q", v) for v in lin[r])
    out += struct.pack("<Q", sum(1 for rec in records if rec[0] < 0))
    with open(path, "wb") as f:
        f.write(out)
    return lin


def read_bai_linear(path):
    """[ioffsets] per reference of a .bai file"""
    d = open(path, "rb").read()
    assert d[:4] == b"BAI\x01"
    n_ref, off, out = struct.unpack_from("<i", d, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, off)[0]
        off += 4
        for _ in range(n_bin):
            off += 8 + 16 * struct.unpack_from("<i", d, off + 4)[0]
        n_intv = struct.unpack_from("<i", d, off)[0]
        out.append(list(struct.unpack_from(f"<{n_intv}Q", d, off + 4)))
        off += 4 + 8 * n_intv
    return out


def write_reference(path, contigs):
    """contigs: [(name, sequence)].  A FASTA with every contig on one line, and its .fai, in the form hostref.write_fasta writes."""
    fai, at = [], 0
    with open(path, "w") as f:
        for name, seq in contigs:
            f.write(f">{name}\n")
            at += len(name) + 2
            f.write(seq + "\n")
            fai.append(f"{name}\t{len(seq)}\t{at}\t{len(seq)}\t{len(seq) + 1}\n")
            at += len(seq) + 1
    with open(path + ".fai", "w") as f:
        f.write("".join(fai))
    return path


def read_fields(r):
    """A read dict in the fields tp.read_bam gives back (ref by name is the caller's to add)"""
    return dict(pos=r["pos"], mapq=r["mapq"], flag=r["flag"], cigar=list(r["cigar"]), seq=r["seq"], qual=bytes(r["qual"]), md=None)


assert tp.CIGAR_OPS == bm.CIGAR_OPS
