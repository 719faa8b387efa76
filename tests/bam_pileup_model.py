"""Plain Python model of bvc_bam_pileup (include/bvc_bam.h), no device: BAM record bytes written from read dicts (the shape of
tests/test_host.py's _random_read), read_record + BamFile::fetch's filter restated over those bytes, the per-position rule taken from
tests/golden/make_testdata_pileup.find_snp_at_pos (the statement-by-statement restatement of the reference), the binary entry encoding of
bin_batch_entry and the mapq an indel entry inherits.  tests/test_bam_pileup_abi.py holds it to the CPU path (the host program's temp
batches on the 100 test BAMs, bvchost_pileup_tokens on random reads); that is what entitles it to judge the device."""
import struct

from tests.golden import make_testdata_pileup as tp

OK, BAM_MORE, ERR_ARG, ERR_DATA = 0, 2, -1, -5
CIGAR_OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
MAX_RECORD = 1 << 28


class Checked(str):
    """A string whose slices and indices fail where std::string::substr / the host's range check throw (a start past the end, a negative
    index), instead of Python's clamping and wrap-around: find_snp_at_pos then raises IndexError where the CPU path throws std::out_of_range."""

    def __getitem__(self, k):
        if isinstance(k, slice):
            start = 0 if k.start is None else k.start
            if start < 0 or start > len(self):
                raise IndexError("substr start out of range")
        elif k < 0:
            raise IndexError("negative index")
        return str.__getitem__(self, k)


def parse_cigar(text):
    """"5M2I3M" -> [("M", 5), ("I", 2), ("M", 3)]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((ch, int(n)))
            n = ""
    return out


def query_length(cigar):
    return sum(l for op, l in cigar if op in "MIS=X")


def make_read(pos, cigar, flag=0, mapq=30, seq=None, qual=None, ref_id=0, name=b"r\0"):
    """A read dict.  cigar: text or [(op, len)]; seq / qual default to a pattern of the CIGAR's query length that depends on pos."""
    cigar = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    n = query_length(cigar)
    if seq is None:
        seq = "".join("ACGTN"[(i * 3 + pos + (i // 7)) % 5] for i in range(n))
    if qual is None:
        qual = [(i * 7 + pos) % 40 + 2 for i in range(len(seq))]
    return dict(pos=pos, flag=flag, mapq=mapq, cigar=cigar, seq=seq, qual=list(qual), ref_id=ref_id, name=name)


def pack_record(r, block_size=None, l_seq=None, n_cigar=None, l_read_name=None):
    """The bytes of one alignment record (SAM specification 4.2), block_size word included.  The keyword arguments overwrite a field
    without changing the bytes behind it (malformed records)."""
    name = r.get("name", b"r\0")
    seq, qual = r["seq"], r["qual"]
    packed = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= NT16.index(ch) << (4 if i % 2 == 0 else 0)
    body = struct.pack("<iiBBHHHiiii", r.get("ref_id", 0), r["pos"], len(name) if l_read_name is None else l_read_name, r["mapq"], 4680,
                       (len(r["cigar"]) if n_cigar is None else n_cigar) & 0xFFFF, r["flag"], len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", (l << 4) | CIGAR_OPS.index(op)) for op, l in r["cigar"]) + bytes(packed) + bytes(qual)
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def scan_sample(data, eof, rid, beg0, end0, min_mapq):
    """read_record + BamFile::fetch over a sample's bytes: (status 0..3, the kept reads as dicts)."""
    off, rv = 0, []
    while True:
        left = len(data) - off
        if left == 0:
            status = 0 if eof else 2
            break
        if left < 4:
            status = 3 if eof else 2
            break
        bs = struct.unpack_from("<i", data, off)[0]
        if bs < 32 or bs > MAX_RECORD:
            status = 3
            break
        if left - 4 < bs:
            status = 3 if eof else 2
            break
        p = off + 4
        ref_id, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", data, p)
        if l_seq < 0 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            status = 3
            break
        off += 4 + bs
        if ref_id < 0 or ref_id < rid:
            continue
        if ref_id > rid or pos >= end0:
            status = 0
            break
        q = p + 32 + l_rn
        cigar = []
        for c in struct.unpack_from(f"<{n_cig}I", data, q):
            cigar.append((CIGAR_OPS[c & 15] if (c & 15) < 9 else "M", c >> 4))
        q += 4 * n_cig
        r = dict(pos=pos, flag=flag, mapq=mapq, cigar=cigar)
        if (flag & 0x4) or not cigar or tp.end_pos(r) <= beg0 or (flag & 0x400) or mapq < min_mapq:
            continue
        sb = data[q:q + (l_seq + 1) // 2]
        r["seq"] = Checked("".join(NT16[(sb[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq)))
        r["qual"] = data[q + (l_seq + 1) // 2:q + (l_seq + 1) // 2 + l_seq]
        rv.append(r)
    if status >= 2:
        return status, []
    return (0 if rv else 1), rv


def sample_entries(rv, positions, rg_s, refseq):
    """{pos: entry} of one sample, or None for the rule's out-of-range cases (status 4); the indel entries carry the mapq of the last base
    entry before them."""
    try:
        m = tp.find_snp_at_pos(rv, positions, refseq=Checked(refseq), rg_s=rg_s)
    except IndexError:
        return None
    last = 0
    for p in positions:
        e = m.get(p)
        if e is None:
            continue
        if e["is_indel"]:
            e["mapq"] = last
        else:
            last = e["mapq"]
    return m


def entry_bytes(e, sample):
    """bin_batch_entry"""
    out = struct.pack("<IBBBBB", sample, e["base"], e["mapq"], e["qual"], e["rpr"], (e["strand"] & 1) | (2 if e["is_indel"] else 0))
    if e["is_indel"]:
        text = e["indel"].encode()[:0xffff]
        out += struct.pack("<H", len(text)) + text
    return out


def expected(samples, beg0, end0, min_mapq, positions, rg_s, refseq):
    """samples: [(bytes, eof, rid)].  dict(rc, status, records, rec_start, maps): what bvc_bam_pileup returns and writes; records and
    rec_start are None unless rc is OK."""
    status, maps = [], []
    for data, eof, rid in samples:
        st, rv = scan_sample(bytes(data), eof, rid, beg0, end0, min_mapq)
        m = {}
        if st == 0:
            m = sample_entries(rv, positions, rg_s, refseq)
            if m is None:
                st, m = 4, {}
        status.append(st)
        maps.append(m)
    rc = ERR_DATA if any(s in (3, 4) for s in status) else BAM_MORE if 2 in status else OK
    if rc != OK:
        return dict(rc=rc, status=status, records=None, rec_start=None, maps=maps)
    records, rec_start = bytearray(), []
    for p in positions:
        rec_start.append(len(records))
        payload = b"".join(entry_bytes(m[p], s) for s, m in enumerate(maps) if p in m)
        records += struct.pack("<I", len(payload)) + payload
    rec_start.append(len(records))
    return dict(rc=rc, status=status, records=bytes(records), rec_start=rec_start, maps=maps)


def layout(samples, lead=0):
    """The samples' bytes one after the other, `lead` junk bytes in front of each: (bam bytes, sample_off, sample_end, sample_eof, rid)."""
    bam, off, end = bytearray(), [], []
    for data, _, _ in samples:
        bam += b"\xa5" * lead
        off.append(len(bam))
        bam += data
        end.append(len(bam))
    return bytes(bam), off, end, [1 if e else 0 for _, e, _ in samples], [r for _, _, r in samples]


def census(exp):
    """What a result exercises: base entries, indel entries, entries that come from a read behind the first covering one are counted by
    the callers that know the reads; here the statuses and the entry kinds."""
    c = dict(base=0, indel=0)
    for m in exp["maps"]:
        for e in m.values():
            c["indel" if e["is_indel"] else "base"] += 1
    for s in exp["status"]:
        c[f"status{s}"] = c.get(f"status{s}", 0) + 1
    return c
