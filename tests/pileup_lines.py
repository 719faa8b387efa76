"""The catalogue of hand-built pileup text the device parser is checked on (deterministic: no random generator decides an edge).

A Case is one tile: batch_lines[b][t] (no newline), the samples of every batch, where every batch's first line starts (mod 16),
the carry of the tile before, and whether the tile is regular by the definition at the head of csrc/pileup_kernel.hip.  Every tile
is built at the smallest size that reaches its edge; which edges the regular ones reach is counted by tests/pileup_model.py (the
census) and demanded by tests/test_pileup_lines.py.  irregular() pairs every tile that must be reported with a regular twin;
feeds() are the catalogue's text cut into compressed blocks for bvc_pileup_begin_bgzf.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name batch_lines n_in_batch align carry_in regular ref")
ZERO_CARRY = (0, 0, 0, 0, 0)


def case(name, batch_lines, n_in_batch=None, align=None, carry_in=ZERO_CARRY, regular=True, ref=None):
    if n_in_batch is None:                                             # every line of a batch holds as many tokens as its first
        n_in_batch = [len(lines[0].split(" ")) - 1 if lines[0] else 0 for lines in batch_lines]
    T = len(batch_lines[0])
    assert all(len(lines) == T for lines in batch_lines)
    if ref is None:
        ref = np.zeros(T, dtype=np.int8)
    return Case(name, batch_lines, np.array(n_in_batch, dtype=np.int32), align, list(carry_in), regular, ref)


def layout(batch_lines, align=None):
    """(text, line_start [nb, T + 1]): the lines of a batch one behind the other, batch b's first line at offset align[b] mod 16 (the
    stride of tests/test_gpu_round5.py's tile_of where align is None); '#' between the batches."""
    nb, T = len(batch_lines), len(batch_lines[0]) if batch_lines else 0
    parts, at = [], 0
    ls = np.zeros((nb, T + 1), dtype=np.uint32)
    for b, lines in enumerate(batch_lines):
        a = (b * 5) % 16 if align is None else align[b] % 16
        pad = (a - at) % 16
        parts.append(b"#" * pad)
        at += pad
        blob = "".join(l + "\n" for l in lines).encode()
        lens = np.fromiter((len(l) + 1 for l in lines), dtype=np.int64, count=T)
        ls[b, 0] = at
        ls[b, 1:] = at + np.cumsum(lens)
        parts.append(blob)
        at += len(blob)
    return b"".join(parts), ls


def sample0_of(n_in_batch):
    return np.concatenate([[0], np.cumsum(n_in_batch)[:-1]]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- tokens
def base_token(length, k):
    """A base token of `length` bytes with its space (10..20): five fields of 1..3 digits, the wide ones rotating with k so that every
    field, base and strand included, takes every width; values wrap the bit fields where the width allows."""
    assert 10 <= length <= 20
    w = [1] * 5
    for j in range(length - 10):
        w[(k + j) % 5] += 1
    f = []
    for i, wi in enumerate(w):
        f.append(str((k + i) % 10) if wi == 1 else str(10 + (k * 7 + i * 13) % 90) if wi == 2 else str(100 + (k * 37 + i * 101) % 900))
    tok = ",".join(f)
    assert len(tok) + 1 == length
    return tok


def dots(n_bytes):
    assert n_bytes % 2 == 0 and n_bytes >= 0
    return ". " * (n_bytes // 2)


def filler(n_bytes):
    """n_bytes of regular tokens: dots, with one three-byte indel token in front where n_bytes is odd."""
    if n_bytes % 2:
        assert n_bytes >= 3
        return "+A " + dots(n_bytes - 3)
    return dots(n_bytes)


# ------------------------------------------------------------------------------------------------------------ regular cases
def base_lengths():
    """Every token length at every p % 16 (so every p % 8 twice, and every way across a lane edge): the token first in its line with
    the line going on, and last in the next line.  base_length_tile(L, a) is one (length, alignment) alone."""
    lines, align = [], []
    for a in range(16):
        for L in range(10, 21):
            lines.append(base_length_lines(L, a))
            align.append(a)
    return [case("base_lengths", lines, align=align)]


def base_length_lines(L, a):
    return [base_token(L, a + L) + " . ", ". " + base_token(30 - L, a * 3 + L) + " "]


def base_length_tile(L, a):
    return case("base_%d_at_%d" % (L, a), [base_length_lines(L, a)[:1]], align=[a])


def field_wrap():
    toks = ["8,256,256,256,2", "12,999,999,999,999", "4,300,511,257,3", "999,255,0,1,998", "15,512,768,1,10", "13,257,513,769,7",
            "7,0,0,0,1", "100,100,100,100,100", "20,1,2,3,4"]
    return [case("field_wrap", [["".join(t + " " for t in toks)]], align=[9])]


def line_edges():
    """A line from every s % 16 to every e % 16 (2..17 bytes), and a batch of no samples: lines of 0 bytes."""
    lines, align = [], []
    for a in range(16):
        for em in range(16):
            k = (em - a) % 16
            if k < 2:
                k += 16
            lines.append([filler(k)])
            align.append(a)
    lines.append([""])
    align.append(4)
    lines.append([". "])
    align.append(14)
    return [case("line_edges", lines, align=align)]


def long_lines():
    """Lines that end 1024 +- 2 and 2048 +- 2 bytes behind s & ~15: the step loop's last trip holds 0, 1 or 2 bytes, or is not made."""
    lines, align = [], []
    for a in (0, 5, 15):
        for r in (1022, 1023, 1024, 1025, 1026, 2046, 2047, 2048, 2049, 2050):
            lines.append([filler(r - a)])
            align.append(a)
    return [case("long_lines", lines, align=align)]


def _at(a, x, token, tail=". 1,40,30,5,1 "):
    """A line that starts at a (mod 16) and holds `token` x bytes behind s & ~15, `tail` behind it."""
    return filler(x - a) + token + " " + tail


def step_edges():
    """The 1 KiB step boundary (1024 and 2048 bytes behind s & ~15) on a separator, on a token's first byte, inside a base token and
    inside an indel token; '.' tokens whose space is the next lane's or the next step's first byte."""
    lines, align = [], []
    for a in (0, 7):
        for x, tok in ((1024 - 13, base_token(14, 1)),               # its space is byte 1024
                       (1024, base_token(12, 2)),                     # its first byte
                       (1024 - 5, base_token(16, 3)), (1024 - 1, base_token(10, 4)), (1024 - 18, base_token(20, 5)),
                       (2048 - 5, base_token(20, 6)), (2048, base_token(11, 7)),
                       (1021, "+ACGTACGT"), (2047, "-N+"),
                       (1023, "."), (2047, "."), (95, "."), (1007, ".")):
            lines.append([_at(a, x, tok)])
            align.append(a)
        lines.append([_at(a, 111, ".", tail="")])                     # the line's last token at byte 15 of a lane
        align.append(a)
        lines.append([_at(a, 1023, ".", tail="")])                    # ... of lane 63
        align.append(a)
    return [case("step_edges", lines, align=align)]


def counters():
    """One aligned step with 512 '.' tokens, with 512 one-byte indel tokens, with the most base token starts (103); a second step
    behind each, so that the running sums are used."""
    many = "".join("%d,%d,%d,%d,%d " % (i % 4, i % 10, (i * 3) % 10, (i * 7) % 10, i & 1) for i in range(103))
    lines = [[dots(1024) + "1,2,3,4,0 N . +AC 2,60,40,9,1 "], ["N " * 512 + "3,20,30,40,1 -A N . "], [many + ". N 0,1,2,3,1 "]]
    return [case("counters", lines, align=[0, 0, 0])]


def indel_lengths():
    body = "ACGTN+-"
    toks = ["1,2,3,4,0", "N", "+" + (body * 3)[:14], "-" + (body * 3)[:15], "N" + (body * 3)[:16], "2,3,4,5,1"] + ["."] * 470 + ["+" + (body * 215)[:1499], "-A", "."]
    assert [len(t) for t in toks[1:5]] == [1, 15, 16, 17] and len(toks[-3]) == 1500 and 3 + sum(len(t) + 1 for t in toks[:-3]) == 1016
    return [case("indel_lengths", [["".join(t + " " for t in toks)]], align=[3])]


def indel_sources():
    """The three sources of an indel entry's fields in the write pass (a base token of its own lane, of an earlier lane of the step, of
    an earlier step), an N base token in front, and the entries the patch kernel fills: in lanes before the first base token's, in
    its lane, in an earlier step, in a line without a base token -- which take them from an earlier batch's line."""
    lines = [["1,30,25,7,1 N . "],
             ["2,31,26,8,0 " + dots(22) + "+AC "],
             ["3,32,27,9,1 " + dots(1012) + "-T "],
             ["4,9,9,9,1 N "],
             ["N +A " + dots(14) + "-C 0,1,2,3,0 "],
             ["N " + dots(1022) + "0,5,6,7,1 "],
             ["+A -C N "]]
    return [case("indel_sources", lines, align=[0] * 7)]


def patch_depths():
    """Indel entries that take their fields from far back: 319 lines and 159 positions behind them, and from the tile's carry_in over
    three consecutive tiles (chain_b has no base token at all: chain_c's first entry takes chain_a's last base token).  A carry_in
    of zeros is what the odd fillers of line_edges, long_lines and step_edges start from."""
    far = [["3,44,33,22,1 "] + ["N ", "-AC "] * 79 + ["N "], ["+T ", "N "] * 80]
    out = [case("patch_far", far, align=[0, 11]),
           case("chain_a", [[". 1,11,12,13,1 ", "N 4,21,22,23,0 "]], carry_in=(3, 1, 2, 3, 0)),        # an N base: dropped, but the carry
           case("chain_b", [[". . ", ". . ", ". . "]], carry_in=(4, 21, 22, 23, 0)),
           case("chain_c", [["-G 0,9,8,7,1 "]], carry_in=(4, 21, 22, 23, 0))]
    return out


ONE_SAMPLE = [".", "1,30,25,7,1", "N", ".", "+AC", "2,60,40,99,0", ".", ".", "4,5,6,7,1", "-T", "."]
LINE_COUNTS = [(1, 1), (1, 2), (3, 1), (1, 4), (5, 1), (3, 2), (7, 1), (1, 8), (3, 3), (7, 585), (1, 4096), (1, 4097), (1, 8191), (3, 2731),
               (5, 51), (1, 256), (1, 512)]


def line_counts():
    """One-sample lines in batches of 1, 3, 5 and 7: n_lines 1..9, 4095, 4096, 4097, 8191, 8193 for the scan (n_lines % 4 = 0..3) and
    255, 256, 512 for the patch kernel's last thread."""
    out = []
    for nb, T in LINE_COUNTS:
        lines = [[ONE_SAMPLE[(t * nb + b) % 11] + " " for t in range(T)] for b in range(nb)]
        out.append(case("lines_%d" % (nb * T), lines))
    return out


CALLED_AT = (0, 1022, 1023, 1024, 1025, 1026)


def called():
    """n_pos of 1023, 1024, 1025 and 2049 (called_scan_kernel takes 1024 positions a step) with positions built to be called -- 30
    samples, half reference and half not at quality 40 -- at 0, 1022..1026 and the last."""
    hot = "0,60,40,10,0 " * 15 + "1,60,40,10,1 " * 15
    out = []
    for T in (1023, 1024, 1025, 2049):
        at = {t for t in CALLED_AT if t < T} | {T - 1}
        out.append(case("called_%d" % T, [[hot if t in at else dots(60) for t in range(T)]]))
    return out


LARGE_NB, LARGE_T, LARGE_PERIOD = 5, 52500, 7
LARGE_KIND = np.array([0, 1, 0, 2, 1, 0, 1])                        # '.', base token, 'N'; by line index (position-major) mod 7


def large_columns():
    """The large case as arrays over its lines in position-major order g = t * 5 + b: kind and the five fields of a base token."""
    g = np.arange(LARGE_NB * LARGE_T, dtype=np.int64)
    kind = LARGE_KIND[g % LARGE_PERIOD]
    return g, kind, (g % 5, g % 61, (g * 7) % 42, g % 100, g & 1)     # base (4: dropped), mapq, qual, rpr, strand


@functools.lru_cache(maxsize=None)
def large():
    """5 batches x 52,500 positions of one-sample lines = 262,500 lines: the second trip of the parse kernel's line loop."""
    g, kind, (b, m, q, r, s) = large_columns()
    toks = np.where(kind == 0, ". ", np.where(kind == 2, "N ", "")).tolist()
    for i in np.nonzero(kind == 1)[0].tolist():
        toks[i] = "%d,%d,%d,%d,%d " % (b[i], m[i], q[i], r[i], s[i])
    lines = [[toks[t * LARGE_NB + bb] for t in range(LARGE_T)] for bb in range(LARGE_NB)]
    return case("large", lines)


def large_expected():
    """What the large case parses to, as arrays (vectorised: a Python loop over 262,500 lines is the slow side of its test): the
    entries' fields, samples, entry_off, tally [T, 32], the observations and their offsets."""
    g, kind, f = large_columns()
    is_base = kind == 1
    keep = (is_base & (f[0] != 4)) | (kind == 2)
    src = np.maximum.accumulate(np.where(is_base, g, -1))            # an indel entry's fields: the last base token parsed before it
    have = (src >= 0)[keep]
    at = np.maximum(src, 0)[keep]
    out = {k: np.where(have, v[at], 0) for k, v in zip(("base", "mapq", "qual", "rpr", "strand"), f)}
    out["is_indel"] = (kind == 2)[keep].astype(np.int64)
    out["samples"] = (g % LARGE_NB)[keep]
    pos = (g // LARGE_NB)[keep]
    out["entry_off"] = np.concatenate([[0], np.cumsum(np.bincount(pos, minlength=LARGE_T))])
    tally = np.zeros((LARGE_T, 32), dtype=np.int64)
    np.add.at(tally, (pos, 16 * out["is_indel"] + (out["strand"] << 3 | out["base"])), 1)
    out["tally"] = tally
    obs = out["is_indel"] == 0
    out["obs_base"], out["obs_qual"] = out["base"][obs].astype(np.int8), out["qual"][obs].astype(np.int8)
    out["obs_off"] = np.concatenate([[0], np.cumsum(np.bincount(pos[obs], minlength=LARGE_T))]).astype(np.int64)
    last = int(src[-1])
    out["carry_out"] = [int(v[last]) for v in f]
    return out


def parser_for(c):
    """The restated parser (oracle/emit_oracle.py) in the state the tile before left it in."""
    from oracle import emit_oracle as eo
    p = eo.Parser()
    p.ai.update(base=c.carry_in[0], mapq=c.carry_in[1], qual=c.carry_in[2], rpr=c.carry_in[3], strand=c.carry_in[4])
    return p


FAMILIES = (base_lengths, field_wrap, line_edges, long_lines, step_edges, counters, indel_lengths, indel_sources, patch_depths,
            line_counts, called)


@functools.lru_cache(maxsize=None)
def regular():
    """Every regular case but the large one."""
    out = [c for fam in FAMILIES for c in fam()]
    assert len({c.name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------------------- irregular cases
GOOD = "1,30,25,7,1 . . 0,60,40,12,0 "
# tests/test_gpu_round5.py::test_lines_the_writer_cannot_produce_are_reported_not_guessed, each as the regular line it spoils
BAD = [("two_spaces", "1,30,25,7,1  . . 0,60,40,12,0 "), ("leading_space", " 1,30,25,7,1 . . 0,60,40,12,0 "),
       ("no_last_space", "1,30,25,7,1 . . 0,60,40,12,0"), ("four_fields", "1,30,25,7 . . 0,60,40,12,0 "),
       ("six_fields", "1,30,25,7,1,9 . . 0,60,40,12,0 "), ("four_digits", "1,30,2555,7,1 . . 0,60,40,12,0 "),
       ("empty_field", "1,30,,7,1 . . 0,60,40,12,0 "), ("dot_with_tail", "1,30,25,7,1 .x . 0,60,40,12,0 "),
       ("unknown_token", "1,30,25,7,1 A . 0,60,40,12,0 "), ("three_tokens", "1,30,25,7,1 . 0,60,40,12,0 "),
       ("five_tokens", "1,30,25,7,1 . . . 0,60,40,12,0 "), ("letter_in_field", "1,30,2x,7,1 . . 0,60,40,12,0 ")]
# one byte put in place of another: (name, regular line, the byte's index, the byte)
SUBST = [("sub_two_spaces", "+AC . 1,2,3,4,0 ", 2, " "), ("sub_leading_space", "+- . 1,2,3,4,0 ", 0, " "),
         ("sub_four_fields", "1,30,25,7,1 . ", 9, "0"), ("sub_six_fields", "1,30,25,7,101 . ", 11, ","),
         ("sub_four_digits", "1,30,255,7,1 . ", 8, "5"), ("sub_empty_field", "1,30,25,7,1 . ", 5, ","),
         ("sub_dot_tail", ". N 1,2,3,4,0 ", 1, "x"), ("sub_unknown", "N . 1,2,3,4,0 ", 0, "A"), ("sub_letter", "1,30,25,7,1 . ", 6, "x"),
         ("sub_no_last_space", "1,2,3,4,0 +A ", 12, "A")]
# where the spoiled byte lies, in bytes behind s & ~15
PLACES = [("lane_first", 64), ("lane_last", 79), ("step_first", 1024), ("step_last", 1023), ("second_step", 1500)]


def _first_difference(a, b):
    return next(i for i in range(min(len(a), len(b)) + 1) if a[i:i + 1] != b[i:i + 1])


def irregular():
    """[(irregular case, regular twin)]: one line each.  The verbatim lines at the start of a tile, then every defect with the byte
    that makes it at the first and last byte of a lane, the first and last byte of a step and in the line's second step; a four-digit
    field and a sixth field on a token across the step edge."""
    out = []

    def pair(name, good, bad, a):
        n = len(good.split(" ")) - 1
        out.append((case(name, [[bad]], n_in_batch=[n], align=[a], regular=False), case(name + "_twin", [[good]], n_in_batch=[n], align=[a])))
    for name, bad in BAD:
        pair(name, GOOD, bad, 0)
    pair("empty_line", GOOD, "", 0)
    for k, (name, good, i, ch) in enumerate(SUBST):
        bad = good[:i] + ch + good[i + 1:]
        for place, x in PLACES:
            a = (k * 3) % 16
            front = filler(x - i - a)
            pair("%s_%s" % (name, place), front + good, front + bad, a)
    for k, (name, bad) in enumerate(BAD):
        i = _first_difference(GOOD, bad)
        for place, x in PLACES:
            a = (k * 5 + 1) % 16
            front = filler(x - i - a)
            pair("%s_%s" % (name, place), front + GOOD, front + bad, a)
    for name, good, bad in (("four_digits_across_step", "1,30,255,7,1 . ", "1,30,2555,7,1 . "), ("sixth_field_across_step", "1,30,25,7,1 . ", "1,30,25,7,1,9 . ")):
        for a in (0, 9):
            front = filler(1024 - 6 - a)
            pair("%s_%d" % (name, a), front + good, front + bad, a)
    return out


# ---------------------------------------------------------------------------------------- compressed tiles (bvc_pileup_begin_bgzf)
Feed = collections.namedtuple("Feed", "name batch_lines n_in_batch skip calls")
# calls: [(pieces, max_pos)], pieces[b] = the uncompressed byte counts of the blocks batch b gets in this call


def _stream(lines, skip):
    return ("H" * (skip - 1) + "\n" if skip else "") + "".join(l + "\n" for l in lines)


def _two_tokens(n_bytes):
    """A line of n_bytes: an indel token and a '.'."""
    return "+" + "A" * (n_bytes - 4) + " . "


def _tokens_of(batch_lines):
    return np.array([len(lines[0].split(" ")) - 1 for lines in batch_lines], dtype=np.int32)


def feed_streams(feed):
    return [_stream(lines, feed.skip[b]).encode() for b, lines in enumerate(feed.batch_lines)]


def feeds():
    """Text of the catalogue through compressed blocks: where the blocks are cut, what every call brings and how many positions it may
    take decide where the 1 KiB segments of a region fall."""
    out = []
    # newlines at bytes 1023, 1024 and 1025 of a region; region starts at every % 16 (a header line of 16..31 bytes is skipped)
    lines = [[_two_tokens((1023, 1024, 1025)[b % 3]), "N . ", "1,2,3,4,0 . ", _two_tokens(2010 + 2 * b)] for b in range(16)]
    skip = [16 + b for b in range(16)]
    f = Feed("segment_edges", lines, _tokens_of(lines), skip, None)
    streams = feed_streams(f)
    # one call with everything, cut inside a token and on a newline
    pieces = []
    for b, s in enumerate(streams):
        cut1 = s.index(b"\n", skip[b]) + 1                           # a block that ends on the first line's newline
        cut2 = s.index(b"1,2,3") + 3                                  # ... inside a base token
        pieces.append([cut1, cut2 - cut1, len(s) - cut2])
    out.append(f._replace(calls=[(pieces, 4)]))
    # max_pos one less than, equal to and one more than the whole lines available; T cut at a line a segment holds; a batch without a
    # new block in a call; a partial line of more than 1 KiB left for the next tile
    long_tail = "+" + "ACGT" * 400
    lines = [[". 1,2,3,4,1 ", "N . ", _two_tokens(1100), ". . ", long_tail + " . ", "2,3,4,5,0 . "],
             [". ", "N ", "-A ", ". ", "3,3,3,3,1 ", ". "]]
    f = Feed("max_pos_and_leftovers", lines, _tokens_of(lines), [0, 7], None)
    s0, s1 = feed_streams(f)
    cut = s0.index(long_tail.encode()) + 1300                          # the first call leaves 1300 bytes of a line without its end
    e1 = [i + 1 for i, c in enumerate(s1) if c == 10]                  # ends of batch 1's header and lines
    out.append(f._replace(calls=[([[cut], [e1[2]]], 1),                # lines available: 4 and 2 -> max_pos 1 = one less than 2
                                 ([[], [e1[3] - e1[2]]], 2),           # batch 0 gets no block; available 3 and 2 -> max_pos 2 = equal
                                 ([[len(s0) - cut], [len(s1) - e1[3]]], 4)]))      # 1 + the rest: 3 available -> max_pos 4 = one more
    # one batch of more than 64 KiB (more than 64 segments) beside batches of a few bytes
    big = [dots(1500) for _ in range(50)]
    lines = [[". "] * 50, big, ["N "] * 50]
    f = Feed("more_than_64_segments", lines, _tokens_of(lines), [0, 3, 0], None)
    ss = feed_streams(f)
    out.append(f._replace(calls=[([[len(ss[0])], [40000, len(ss[1]) - 40000], []], 64),      # batch 2's region is empty: no position
                                 ([[], [], [len(ss[2])]], 64)]))
    return out
