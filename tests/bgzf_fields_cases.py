"""The hand-built pieces the field parse of the device deflate encoder is walked over (tuning key "bgzf_parse" = 1; docs/BGZF_FIELDS.md),
beside the catalogue of tests/bgzf_deflate_cases.py: the smallest inputs at which this parse can go wrong.  Every piece is the same on
every call.  Nothing here needs a device."""
import numpy as np

from tests import bgzf_deflate_cases as dc

B = dc.B
LETTERS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789./+-"      # no tab, no colon


def letters(rng, n):
    return bytes(LETTERS[i] for i in rng.integers(0, len(LETTERS), n))


def field(rng, length):
    """A field of `length` bytes: letters and the tab that ends it."""
    return letters(rng, length - 1) + b"\t"


def catalogue():
    """[(name, bytes)]"""
    rng = np.random.default_rng(20261101)
    out = [(f"fields: length {n}", b"a\tb:c"[:n]) for n in range(6)]
    # a head of every length on either side of the keyed range 4..32, met again behind another field (a head with one candidate), and
    # three times in a row (a head and two repeats)
    for n in range(1, 35):
        f = field(rng, n)
        out.append((f"fields: head of {n} bytes met again", f + b"zz\t" + f + b"x"))
        out.append((f"fields: field of {n} bytes three times", b"zz\t" + f * 3 + b"x"))
    # repeat runs whose byte length is on either side of 4, 258, 2 x 258 and of 258 rounded down to a multiple of the field
    for n in (1, 3, 4, 17):
        f = field(rng, n)
        for reps in sorted({t // n + j for t in (4, 258, 2 * 258, 258 // n * n) for j in (-1, 0, 1)} - {0, -1}):
            out.append((f"fields: {reps} repeats of {n} bytes", b"start\t" + f * (reps + 1) + b"end"))
            out.append((f"fields: {reps} repeats of {n} bytes up to the end", b"start\t" + f * (reps + 1)))
    # rounds of 256 positions: a run across an edge, a keyed head at the last and at the first position of a round with its only candidate
    # in the round before, and one sixteen rounds on (the same way of the table)
    out.append(("fields: a run across a round's edge", field(rng, 250) + b"./.\t" * 12 + b"end"))
    head = b"HEAD\t"
    for at in (255, 256, 511, 512, 16 * 256, 16 * 256 + 255, 17 * 256):
        out.append((f"fields: a head at position {at}", head + field(rng, at - 5) + head + b"end"))
    out.append(("fields: a head at the last position of each of three rounds",
                head + field(rng, 250) + head + field(rng, 251) + head + field(rng, 251) + head + b"end"))
    # the distance's end: the only candidate at 32768 (a match) and at 32769 (none)
    for d in (32768, 32769):
        out.append((f"fields: the only candidate at distance {d}", head + field(rng, d - 5) + head + b"end"))
    # where a candidate's extension stops
    out.append(("fields: the extension stops in the middle of a field", b"AAAA\tBBBBxyz\tQ\tAAAA\tBBBBxyw\tend"))
    out.append(("fields: the extension stops in the middle of the next field", b"AAAA\tBxyz\tQ\tAAAA\tBxyw\tend"))
    out.append(("fields: the extension stops at the head's own end", b"AAAA\tB\tQ\tAAAA\tC\tend"))
    out.append(("fields: the extension stops at a cut three fields on", b"AAAA\tB:C:D\tQ\tAAAA\tB:C:E\tend"))
    out.append(("fields: the extension reaches the block's end", b"AAAA\tBBBB\tQ\tAAAA\tBBBB"))
    out.append(("fields: the extension reaches the block's end inside a field", b"AAAA\tBBBBCC\tQ\tAAAA\tBBBB"))
    out.append(("fields: the extension reaches 258 bytes inside a field", b"AAAA\t" + b"B" * 300 + b"\tQ\tAAAA\t" + b"B" * 300 + b"\tend"))
    out.append(("fields: the extension reaches 258 bytes at a cut", b"AAAAA\t" + b"./.\t" * 70 + b"Q\tAAAAA\t" + b"./.\t" * 70 + b"end"))
    # two candidates, one in each of the two rounds before the head's (a round's own candidate is its first head with the key only):
    # the longer wins, the nearer among equals
    def three_rounds(first, second, third):
        return first + field(rng, 256 - len(first)) + second + field(rng, 256 - len(second)) + third
    out.append(("fields: the farther candidate is the longer", three_rounds(b"AAAA\tB\tC\tQ\t", b"AAAA\tB\tD\tQ\t", b"AAAA\tB\tC\tend")))
    out.append(("fields: the nearer candidate is the longer", three_rounds(b"AAAA\tB\tD\tQ\t", b"AAAA\tB\tC\tQ\t", b"AAAA\tB\tC\tend")))
    out.append(("fields: the nearer of two equal candidates", three_rounds(b"AAAA\tB\tC\tQ\t", b"AAAA\tB\tC\tR\t", b"AAAA\tB\tC\tend")))
    # ... and of two heads with the key in the head's own round only the first is a candidate
    out.append(("fields: two heads with the key in the round itself", b"AAAA\tB\tD\tQ\tAAAA\tB\tC\tR\tAAAA\tB\tC\tend"))
    # a piece's cut at 65280 bytes: a field astride it, a run astride it, a head whose candidate lies in the block before (out of reach)
    out.append(("fields: a field astride a piece's cut", b"xx" + dc.periodic(b"0/.:A:+:0.999369\t", B + 100)))
    out.append(("fields: a run astride a piece's cut", b"x\t" + dc.periodic(b"./.\t", B + 100)))
    out.append(("fields: a head's twin in the block before", head + field(rng, B - 7) + head * 3 + b"end"))
    out.append(("fields: 65280 tabs", b"\t" * B))
    out.append(("fields: 65285 tabs", b"\t" * (B + 5)))
    out.append(("fields: 65280 colons and tabs in turn", dc.periodic(b":\t", B)))
    out.append(("fields: no cut, 3000 letters", letters(rng, 3000)))
    out.append(("fields: no cut, 65280 letters of four", bytes(b"ACGT"[i] for i in rng.integers(0, 4, B))))
    # many heads, many keys that meet: few letters between the delimiters
    out.append(("fields: 20000 bytes over a, b, tab and colon", bytes(b"ab\t:"[i] for i in rng.integers(0, 4, 20000))))
    out.append(("fields: 65280 bytes over six letters and a tab", bytes(b"ACGTN.\t"[i] for i in rng.integers(0, 7, B))))
    out.append(("fields: 65280 random bytes", rng.integers(0, 256, B, dtype=np.uint8).tobytes()))
    # the text the parse is for: the sample columns of one called site at three coverages, two blocks each at the most
    for coverage, seed, _ in dc.SIZE_TEXTS:
        out.append((f"fields: sample columns at coverage {coverage}", dc.sample_text(6000, coverage, seed)[:2 * B]))
    assert len({name for name, _ in out}) == len(out)
    return out
