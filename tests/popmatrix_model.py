"""Plain Python model of `BaseVarC popmatrix` and of bvc_bam_popmatrix (include/bvc_popmatrix.h), no device: BamProcess::FetchAlleleType
(src/BamProcess.cpp:96-198) restated statement by statement over the read dicts of tests/bam_pileup_model.py -- the read cursor `i`, `j`
and the `next` / `eof` flags kept across positions, so a position list that is not sorted gets the reference's answer -- raising
IndexError where the reference throws; the stateless form the device computes (per position, tests/golden/make_testdata_pileup's
find_snp_at_pos entry mapped to a character through the read's base); and what a library call returns and writes.
tests/test_popmatrix_model.py holds the two forms to each other; tests/test_popmatrix_host.py holds the host program to the first."""
from tests import bam_pileup_model as bm
from tests.golden import make_testdata_pileup as tp

OK, BAM_MORE, ERR_ARG, ERR_DATA = bm.OK, bm.BAM_MORE, bm.ERR_ARG, bm.ERR_DATA


def snp_code(r, pos, ref, alt):
    """GetSnpCode: the read's character at the position against the line's REF, then its ALT."""
    x = r["seq"][tp.get_offset(r, pos)]
    return "0" if x == ref else "1" if x == alt else "."


def fetch_allele_type(rv, pv, refseq, rg_s):
    """pv: [(pos, ref, alt)].  The row of one sample as a string.  No read at all: dots (the reference indexes an empty vector there)."""
    if not rv:
        return "." * len(pv)
    refseq = bm.Checked(refseq)
    snps = []
    i = j = 0
    eof = nxt = False
    r = rv[i]
    last = len(rv) - 1
    for pos, ref, alt in pv:
        if pos < r["pos"] + 1:
            snps.append(".")
            continue
        while pos > tp.end_pos(r):
            if i == last:
                eof = True
                break
            i += 1
            r = rv[i]
            j = i
            if pos < r["pos"] + 1:
                nxt = True
                break
        if nxt or eof:
            snps.append(".")
            eof = nxt = False
            continue
        while True:
            c = r["cigar"]
            sx, sy, sk = r["pos"], 0, None
            for k, (op, l) in enumerate(c):
                if op in "MISX":
                    sy += l
                if op in "HI":
                    continue
                sx += l
                if pos <= sx:
                    sk = k
                    break
            assert sk is not None
            op = c[sk][0]
            indel = 0
            if sx == pos and sk + 1 < len(c):
                op2, l2 = c[sk + 1]
                if op2 == "D":
                    indel = -l2
                    refseq[pos - rg_s + 1:pos - rg_s + 1 + l2]          # the token is built before it is discarded: substr throws
                elif op2 == "I":
                    indel = l2
                    bm.Checked(r["seq"])[sy:sy + l2]
                # (a pad next: the reference's scan re-reads c[sk], never an insertion, so indel stays 0)
            if indel != 0:
                snps.append(".")
                break
            if op not in "DN":
                snps.append(snp_code(r, pos, ref, alt))
                break
            elif j < last:
                j += 1
                r = rv[j]
                if pos < r["pos"] + 1 or pos > tp.end_pos(r):
                    snps.append(".")
                    break
            else:
                snps.append(".")
                break
        r = rv[i]
        j = i
    return "".join(snps)


def stateless_row(rv, pv, refseq, rg_s):
    """What the device computes: every position on its own through find_snp_at_pos (a fresh cursor each time); a base entry becomes the
    read's character against REF / ALT, anything else a dot.  The character rides in the entry's quality field."""
    if not rv:
        return "." * len(pv)
    chars = [dict(r, qual=[ord(ch) for ch in r["seq"]]) for r in rv]
    out = []
    for pos, ref, alt in pv:
        e = tp.find_snp_at_pos(chars, [pos], refseq=bm.Checked(refseq), rg_s=rg_s).get(pos)
        if e is None or e["is_indel"]:
            out.append(".")
        else:
            x = chr(e["qual"])
            out.append("0" if x == ref else "1" if x == alt else ".")
    return "".join(out)


def expected(samples, beg0, end0, min_mapq, pv, rg_s, refseq_len):
    """samples: [(bytes, eof, rid)]; pv: [(pos, ref, alt)], not descending.  dict(rc, status, rows): what bvc_bam_popmatrix returns and
    writes; a row is None where the header leaves it unspecified (status 2, 3, 4)."""
    status, rows = [], []
    for data, eof, rid in samples:
        st, rv = bm.scan_sample(bytes(data), eof, rid, beg0, end0, min_mapq)
        row = None
        if st == 0:
            try:
                row = fetch_allele_type(rv, pv, "N" * refseq_len, rg_s)
            except IndexError:
                st = 4
        elif st == 1:
            row = "." * len(pv)
        status.append(st)
        rows.append(row)
    rc = ERR_DATA if any(s in (3, 4) for s in status) else BAM_MORE if 2 in status else OK
    return dict(rc=rc, status=status, rows=rows)


def refalt(positions, rg_s, refseq, salt=0):
    """A deterministic (pos, REF, ALT) per position: REF the reference's character there (N outside it), ALT another letter -- and every
    seventh line REF and ALT swapped, every eleventh an N, so that '0', '1' and '.' all appear."""
    out = []
    for n, p in enumerate(positions):
        i = p - rg_s
        ref = refseq[i] if 0 <= i < len(refseq) else "N"
        alt = "ACGT"[("ACGTN".index(ref) + 1 + (n + salt) % 3) % 4]
        if (n + salt) % 7 == 3:
            ref, alt = alt, ref
        if (n + salt) % 11 == 5:
            alt = "N"
        out.append((p, ref, alt))
    return out
