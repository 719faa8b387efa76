"""Plain Python model of bvc_bam_pileup_text (include/bvc_bam_text.h), no device: the per-sample entries of tests/bam_pileup_model.py (which
tests/test_bam_pileup_abi.py holds to the CPU path) written as the lines of the text temp batches -- format_pileup_token of every sample
in sample order and a newline, an indel text whole -- with line_start, and the cases the binary catalogue has no reason to hold: the
decimal widths of every field, the 1-byte indel text, insertions on either nibble, a deletion past the binary entry's 0xffff bound, and
the sample and position counts around the kernels' wavefront and tile.  tests/test_bam_text_abi.py holds it to the CPU path (the host
program's text temp batches on the 100 test BAMs, bvchost_pileup_tokens on the random cases)."""
from tests import bam_pileup_cases as bc
from tests import bam_pileup_model as bm

WIDTHS = (0, 9, 10, 99, 100, 255)         # a byte's values at which its decimal form changes length, and its ends
LONG_DELETION = 70000                     # bases: past the 0xffff bytes a binary entry's text can hold


def token(e):
    """format_pileup_token (host/pileup.cpp)"""
    if e is None:
        return ". "
    return e["indel"] + " " if e["is_indel"] else f"{e['base']},{e['mapq']},{e['qual']},{e['rpr']},{e['strand']} "


def lines(maps, positions):
    """(text, line_start) of a batch: maps = the samples' {pos: entry}."""
    text, line_start = bytearray(), []
    for p in positions:
        line_start.append(len(text))
        text += ("".join(token(m.get(p)) for m in maps) + "\n").encode()
    line_start.append(len(text))
    return bytes(text), line_start


_EXPECTED = {}


def expected(c):
    """dict(rc, status, text, line_start, maps) of a case (tests/bam_pileup_cases.case): what bvc_bam_pileup_text returns and writes; text and
    line_start are None unless rc is OK.  Computed once a case."""
    if c["name"] not in _EXPECTED:
        e = bc.expected(c)
        text, line_start = lines(e["maps"], c["positions"]) if e["rc"] == bm.OK else (None, None)
        _EXPECTED[c["name"]] = dict(rc=e["rc"], status=e["status"], text=text, line_start=line_start, maps=e["maps"])
    return _EXPECTED[c["name"]]


# ---- the cases of the text form ------------------------------------------------------------------------------------------------------
ODD_INSERTION = dict(cigar="5M2I5M", seq="ACGTAGGCATGC", at=5)        # the inserted bases start at query index 5: the low nibble of byte 2
EVEN_INSERTION = dict(cigar="4M3I5M", seq="ACGTTTAGCATG", at=4)       # at query index 4: the high nibble of byte 2


def cases():
    R, sample, case, span = bc.R, bc.sample, bc.case, bc.span
    c = []
    # mapq and qual at every width; a read of 300 bases takes rpr = (uint8_t)(offset + 1) through 1 .. 255, 0, 1 .. (every width, and the
    # wrap at 256); the bases give 0 .. 4 and the flags both strands
    quals = [WIDTHS[i % 6] for i in range(300)]
    seq = "".join("ACGTN"[(i // 6) % 5] for i in range(300))
    c.append(case("every field at 0, 9, 10, 99, 100 and 255, rpr through 256",
                  [sample([R(1010, "300M", mapq=m, flag=16 if k % 2 else 0, seq=seq, qual=quals)]) for k, m in enumerate(WIDTHS)], span(1005, 1320),
                  min_mapq=0))
    c.append(case("an indel text of 1 byte", [sample([R(1024, "5M3D5M")]), sample([R(1020, "9M2D3M")])], span(1020, 1032), refseq=bc.REFSEQ[:30]))
    c.append(case("an insertion on an odd and on an even nibble",
                  [sample([R(1010, x["cigar"], seq=x["seq"])]) for x in (ODD_INSERTION, EVEN_INSERTION)], span(1008, 1024)))
    long_ref = bc.REFSEQ * (2 + LONG_DELETION // len(bc.REFSEQ))
    c.append(case("a deletion of 70,000 bases", [sample([R(1010, f"5M{LONG_DELETION}D5M", mapq=40)]), sample([R(1012, "8M")])],
                  span(1010, 1020) + span(1010 + LONG_DELETION, 1025 + LONG_DELETION), refseq=long_ref))
    c.append(case("a position no sample covers, a sample of status 1 among covered ones",
                  [sample([R(1010, "5M")]), sample([R(1008, "10M", flag=4)]), sample([R(1020, "5M2I3M")]), sample([])], span(1008, 1032)))
    for n in (1, 63, 64, 65, 129):
        c.append(case(f"text: {n} samples", [sample([R(1010 + (s * 5) % 40, "3M1I4M2D6M" if s % 3 == 0 else "11M", mapq=20 + s % 80)] if s % 7 != 6 else [])
                                             for s in range(n)], span(1005, 1070)))
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        c.append(case(f"text: {n} positions", [sample([R(1010 + 200 * i, "60M2D60M1I40M", mapq=30 + i) for i in range(6)]), sample([]),
                                               sample([R(1000, "1100M", mapq=100)])], span(1002, 1002 + n), refseq=bc.REFSEQ * 2))
    c.append(case("text: no samples", [], span(1005, 1075)))
    c.append(case("text: no samples and no positions", [], []))
    c.append(case("text: no positions", [sample([R(1010, "9M")])], []))
    return c


def census(c):
    """What a case's expected lines hold, from the model alone: token kinds, the decimal widths each field took, indel texts of 1 byte and
    past 0xffff, lines that are filler only, and the case's counts."""
    e = expected(c)
    out = dict(filler=0, base=0, indel=0, one_byte_text=0, long_text=0, empty_line=0, status1_among_covered=0)
    for p in c["positions"]:
        row = [m.get(p) for m in e["maps"]]
        out["empty_line"] += 1 if e["maps"] and all(x is None for x in row) else 0
        for x in row:
            if x is None:
                out["filler"] += 1
            elif x["is_indel"]:
                out["indel"] += 1
                out["one_byte_text"] += len(x["indel"]) == 1
                out["long_text"] += len(x["indel"]) > 0xffff
            else:
                out["base"] += 1
                for f in ("base", "mapq", "qual", "rpr", "strand"):
                    out[(f, x[f])] = out.get((f, x[f]), 0) + 1
    out["status1_among_covered"] = int(1 in e["status"] and 0 in e["status"])
    out[("n_samples", len(c["samples"]))] = 1
    out[("n_positions", len(c["positions"]))] = 1
    return out
