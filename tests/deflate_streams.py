"""The catalogue of hand-built deflate streams the block decoders are checked on (deterministic, seeded).

Every stream is built with tests/deflate_writer.py at the smallest size that reaches its edge; which edges the valid ones reach is
counted by tests/deflate_model.py (the census) and demanded by tests/test_deflate_streams.py.  catalogue() is the list of
deflate_writer.Stream; truncations() the byte prefixes of four of them.
"""
import functools
import random

from tests import deflate_writer as W
from tests.deflate_writer import build, dynamic, fixed, lit, lits, litsym, distsym, match, rawbits, reserved, stored

# the device's status codes (csrc/inflate_kernel.hip) where a refusal has one unambiguous code
ERR_TYPE, ERR_STORED, ERR_HEADER, ERR_CODES, ERR_DISTANCE = 1, 2, 3, 4, 6
N_RANDOM = 24                                                      # random valid streams (the GPU test's time budget)


def _rand(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


@functools.lru_cache(maxsize=None)
def full_codes():
    """All 286 literal/length symbols (8 and 9 bits) and all 30 distance symbols (4 and 5 bits): HLIT = 286, HDIST = 30."""
    return W.lengths_with(286, {}, list(range(286))), W.lengths_with(30, {}, list(range(30)))


# ---- code shapes
STAIR_SYMS = list(b"abcdefghijklm") + [256, 257, 265]            # thirteen literals, the end-of-block, length 3, lengths 11..12
STAIR_TOKENS = lits(b"abcdefghijklm") + [match(3, 1), match(11, 5), match(12, 6), lit(ord("a")), match(3, 13)]


def _staircases(out):
    """The staircase 1, 2, ..., 14, 15, 15 permuted: a literal, the end-of-block and a length symbol at 9, 10, 11, 12 and 15 bits; a
    distance symbol (4: distances 5..6) at 7, 8, 9 and 15 bits.  43 bytes of output each."""
    i = 0
    for sym, what in ((ord("a"), "literal"), (256, "eob"), (265, "length")):
        for bits in (9, 10, 11, 12, 15):
            dbits = (7, 8, 9, 15)[i % 4]
            i += 1
            lit_lens = W.staircase_placing(266, STAIR_SYMS, {sym: bits})
            dist_lens = W.staircase_placing(16, list(range(16)), {4: dbits})
            out.append(build("stair_%s%d_dist%d" % (what, bits, dbits), [dynamic(STAIR_TOKENS, lit_lens, dist_lens)]))
    for dbits in (7, 8, 9, 15):                                    # every long code at once, twice in a row
        lit_lens = W.staircase_placing(266, STAIR_SYMS, {ord("a"): 15, 256: 15, 265: 14})
        dist_lens = W.staircase_placing(16, list(range(16)), {4: dbits, 0: 15 if dbits != 15 else 14})
        out.append(build("stair_all_long_dist%d" % dbits, [dynamic(STAIR_TOKENS, lit_lens, dist_lens)] * 2))


SMALL_LIT = W.lengths_with(259, {}, [ord("a"), 256, ord("b"), 257, ord("c"), 258])


def _code_shapes(out):
    a, b = ord("a"), ord("b")
    out.append(build("one_dist_code_sym0", [dynamic([lit(a), lit(b), match(3, 1), match(4, 1)], SMALL_LIT, [1])]))
    out.append(build("one_dist_code_sym5", [dynamic(lits(b"abcabcab") + [match(3, 7), match(4, 8)], SMALL_LIT, [0, 0, 0, 0, 0, 1])]))
    out.append(build("one_dist_code_unused_pattern", [dynamic([lit(a), litsym(257), rawbits(1, 1)], SMALL_LIT, [1])], isize=4,
                     reason="the unused pattern of a one-code distance set"))
    out.append(build("one_dist_code_sym5_unused_pattern", [dynamic(lits(b"abcabcab") + [litsym(257), rawbits(1, 1), rawbits(0, 1)], SMALL_LIT,
                                                                   [0, 0, 0, 0, 0, 1])], isize=11,
                     reason="the unused pattern of a one-code distance set"))
    out.append(build("no_dist_code_literals", [dynamic(lits(b"abcabbca"), SMALL_LIT, [0])]))
    out.append(build("no_dist_code_match", [dynamic([lit(a), litsym(257), rawbits(0, 1)], SMALL_LIT, [0])], isize=4,
                     reason="a distance with no distance code"))
    out.append(build("eob_only_code", [dynamic([], [0] * 256 + [1], [0])]))
    out.append(build("eob_only_code_twice_then_fixed", [dynamic([], [0] * 256 + [1], [0])] * 2 + [fixed(lits(b"xyz"))]))
    lit_lens, dist_lens = full_codes()
    text = lits(b"hlit 286, hdist 30: ") + [match(5, 20), match(258, 25, alt258=True), match(258, 1)]
    out.append(build("hlit286_hdist30", [dynamic(text, lit_lens, dist_lens)]))
    out.append(build("hlit286_no_runs", [dynamic(text, lit_lens, dist_lens, runs=False)]))
    for hclen in (14, 19):
        out.append(build("hlit286_hclen%d" % hclen, [dynamic(text, lit_lens, dist_lens, hclen=hclen)]))
    # code-length codes of 7 bits (the longest there is), used and unused
    for k, forced in enumerate(({9: 7, 16: 7}, {8: 7, 9: 7}, {4: 7, 5: 6}, {16: 7, 5: 7})):
        out.append(build("cl_code_7bits_%d" % k, [dynamic(text, lit_lens, dist_lens, cl_forced=forced)]))
    out.append(build("cl_code_7bits_stair", [dynamic(STAIR_TOKENS, W.staircase_placing(266, STAIR_SYMS, {256: 9}),
                                                     W.staircase_placing(16, list(range(16)), {4: 8}), cl_forced={0: 7, 15: 7})]))
    # every run count at both ends: 16 x 3 and 6, 17 x 3 and 10, 18 x 11 and 138
    runs = [4] * 4 + [0] * 3 + [4] * 7 + [0] * 10 + [3] + [0] * 11 + [4] + [0] * 138 + [4] + [0] * 80 + [4]
    assert len(runs) == 257 and W.kraft(runs) == 1 << 15
    toks = [lit(s) for s in (0, 1, 2, 3, 7, 8, 13, 24, 36, 175, 24, 0)]
    for k in range(4):
        out.append(build("header_runs_at_both_ends_%d" % k, [fixed(lits(b"r" * k)), dynamic(toks, runs, [0])]))
    # a run of zeros from the literal/length lengths into the distance lengths (17: 3 + 3, 18: 8 + 5), and the same cut at the boundary
    for span in (True, False):
        for k in range(2):
            out.append(build("header_run17_across_boundary_span%d_%d" % (span, k),
                             [dynamic(lits(b"abcabcab"[k:]) + [match(3, 7)], SMALL_LIT + [0] * 3, [0, 0, 0, 0, 0, 1], span=span)]))
            out.append(build("header_run18_across_boundary_span%d_%d" % (span, k),
                             [dynamic(lits(b"abcabcab"[k:]) + [match(4, 7)], SMALL_LIT + [0] * 8, [0, 0, 0, 0, 0, 1], span=span)]))


# ---- matches
MATCH_LENS = (3, 4, 10, 11, 62, 63, 64, 65, 130, 131, 227, 257, 258, (258, True))


def _match_dists(length):
    return sorted({1, 2, 3, length - 1, length, length + 1, 63, 64, 65, 4095, 4096, 4097, 8192, 16384, 32767, 32768} - {0})


def _huffman(k, tokens):
    """The tokens in a fixed block (k even) or in a dynamic one with all symbols (k odd)."""
    return fixed(tokens) if k % 2 == 0 else dynamic(tokens, *full_codes())


def _matches(out, rng):
    for k, length in enumerate(MATCH_LENS):
        alt = isinstance(length, tuple)
        length = length[0] if alt else length
        toks = []
        for d in _match_dists(length):
            toks += [match(length, d, alt)] + lits(_rand(rng, d % 3))
        out.append(build("match_len%d%s_every_dist" % (length, "alt" if alt else ""), [stored(_rand(rng, 32768 + k)), _huffman(k, toks)]))
    # dist + len around W - 64 for rings of 4, 8 and 16 KiB
    for k, ring in enumerate((4096, 8192, 16384)):
        for j in range(2):
            toks = []
            for length in (3, 63, 64, 258):
                for dd in (-1, 0, 1):
                    toks += [match(length, ring - 64 - length + dd)] + lits(_rand(rng, (dd + j) % 3))
            out.append(build("ring_edge_%d_%d" % (ring, j), [stored(_rand(rng, ring + 17 + j)), _huffman(k + j, toks)]))
    # dist == o
    for k, o in enumerate((1, 2, 3, 63, 64, 65, 258, 1000, 4032, 5000)):
        for length in sorted({3, max(3, min(o, 63)), 258}):
            first = stored(_rand(rng, o)) if o > 70 else fixed(lits(_rand(rng, o)))
            out.append(build("dist_eq_o_%d_len%d" % (o, length), [first, _huffman(k + length, [match(length, o), lit(33)])]))
    # the first symbol at o = 1023, 0, 1 (mod 1024)
    for base in (1024, 2048, 4096, 8192):
        for d in (-1, 0, 1):
            for k, (length, dist) in enumerate(((3, 1), (63, 100), (258, 300), (64, 64), (10, 3))):
                toks = [match(length, dist), lit(7), match(length, dist)]
                out.append(build("offset_%d%+d_match_%d_%d" % (base, d, length, dist), [stored(_rand(rng, base + d)), _huffman(k, toks)]))
            out.append(build("offset_%d%+d_literals" % (base, d), [stored(_rand(rng, base + d)), _huffman(base + d, lits(_rand(rng, 5)))]))
    # runs of 258 over the ring's end
    for p in (4096 - 100, 8192 - 100):
        for k, d in enumerate((1, 2, 3, 4, 5, 7, 8, 16, 100, 257)):
            out.append(build("run258_dist%d_at_%d" % (d, p), [stored(_rand(rng, p)), _huffman(k, [match(258, d), lit(9), match(258, d)])]))
    # the copy left in flight: a match that reads what the match before it wrote
    for k in range(4):
        toks = []
        for la, da, lb in ((20, 100, 20), (63, 63, 63), (30, 500, 100), (100, 200, 50), (3, 3, 3), (258, 1000, 258), (40, 40, 10)):
            toks += [match(la, da), match(lb, la)] + lits(_rand(rng, k))
        for la, da, lb, db in ((30, 5000, 30, 30), (100, 5000, 40, 100), (63, 4500, 10, 20), (258, 4097, 258, 258), (20, 4013, 20, 10)):
            toks += [match(la, da), match(lb, db)] + lits(_rand(rng, k + 1))
        out.append(build("copy_in_flight_%d" % k, [stored(_rand(rng, 6000 + k)), _huffman(k, toks)]))


# ---- bit positions
X = ord("x")
SLIDE_POOL = list(b"abcdefghijkl")
# 'x' in one bit; length 258 in 3 bits, length 3 in 4; lengths 131..162 (5 extra bits) and the end-of-block in 15
SLIDE_LIT = W.lengths_with(286, {X: 1, 285: 3, 257: 4, 281: 15, 256: 15}, SLIDE_POOL, list(range(200, 256)))
# distances 25..32 in one bit; 16385..24576 (13 extra bits) in 15
SLIDE_DIST = W.lengths_with(30, {9: 1, 28: 15}, [], list(range(30)))


def _bulk(rng):
    """18 KiB of output in about 100 bytes of input: 29 random literals, then length 258 at distance 29 (a prime period)."""
    return lits(bytes(rng.choice(SLIDE_POOL) for _ in range(29))) + [match(258, 29)] * 70


def _long_pair(rng):
    """15 + 5 + 15 + 13 bits."""
    return match(131 + rng.randrange(32), 16385 + rng.randrange(1500))


def _bit_positions(out, rng):
    # k one-bit literals in front of a pair, every k a block of its own (a block's symbols start a batch: the pair starts at lane k)
    for kind in ("short", "long"):
        for k0 in range(0, 71, 18):
            blocks = [dynamic(_bulk(rng), SLIDE_LIT, SLIDE_DIST)]
            for k in range(k0, min(k0 + 18, 71)):
                pair = match(3, 25 + rng.randrange(8)) if kind == "short" else _long_pair(rng)
                blocks.append(dynamic([lit(X)] * k + [pair, lit(rng.choice(SLIDE_POOL))], SLIDE_LIT, SLIDE_DIST))
            out.append(build("slide_%s_pair_k%d" % (kind, k0), blocks))
    # ... and the ones whose pair ends at lanes 62..65 again (short: k + 5, long: k + 35)
    for j in range(3):
        blocks = [dynamic(_bulk(rng), SLIDE_LIT, SLIDE_DIST)]
        for k in (57, 58, 59, 60):
            blocks.append(dynamic([lit(X)] * k + [match(3, 25 + rng.randrange(8)), lit(rng.choice(SLIDE_POOL))], SLIDE_LIT, SLIDE_DIST))
        for k in (27, 28, 29, 30):
            blocks.append(dynamic([lit(X)] * k + [_long_pair(rng), lit(rng.choice(SLIDE_POOL))], SLIDE_LIT, SLIDE_DIST))
        out.append(build("slide_pairs_ending_at_lanes_62_to_65_%d" % j, blocks))
    # the four objects across bit 1920 and bit 2048 of the payload's first word, at every alignment of the payload
    def shape(kind, n):
        head = [lit(X)] * n
        if kind == "pair":
            return [dynamic(_bulk(random.Random(1)) + head + [_long_pair(random.Random(2)), lit(X)], SLIDE_LIT, SLIDE_DIST)]
        if kind == "eob":
            return [dynamic(lits(b"abc") + head, SLIDE_LIT, SLIDE_DIST), fixed(lits(b"after"))]
        if kind == "dynamic_header":
            return [dynamic(lits(b"abc") + head, SLIDE_LIT, SLIDE_DIST), dynamic(STAIR_TOKENS, W.staircase_placing(266, STAIR_SYMS, {256: 10}),
                                                                                   W.staircase_placing(16, list(range(16)), {4: 9}))]
        return [dynamic(lits(b"abc") + head, SLIDE_LIT, SLIDE_DIST), stored(b"stored bytes behind it")]

    def mark(s, kind):
        ms = [m for m in s.marks if m[0] == kind]
        return ms[-1] if kind in ("pair", "dynamic_header", "stored_header") else ms[0]

    for kind in ("pair", "eob", "dynamic_header", "stored_header"):
        first0, behind0 = mark(build("probe", shape(kind, 0)), kind)[1:]
        for edge in (1920, 2048):
            for lead in range(4):
                # (a stored header is 3 bits, 0..7 of padding, 32 of LEN and NLEN: at least 35)
                for inside in ((2, 12, 30) if kind == "stored_header" else (1, (behind0 - first0) // 2, behind0 - first0 - 1)):
                    n = edge - 8 * lead - inside - first0
                    s = build("%s_across_bit%d_lead%d_at%d" % (kind, edge, lead, inside), shape(kind, n))
                    m = mark(s, kind)
                    assert m[1] + 8 * lead < edge < m[2] + 8 * lead, (s.name, m)
                    out.append(s)


# ---- the host decoder's switch from its fast loop to its careful one
def _guard(out, rng):
    """The host decoder leaves its fast loop when fewer than 32 input bytes or 292 output bytes are left; cutting the same token
    sequence one token shorter each time slides that point over every kind of symbol: literals of the first level and of the
    sub-tables (12 and 15 bits), length and distance symbols of either, the end-of-block."""
    lit_lens = W.staircase_placing(266, STAIR_SYMS, {ord("a"): 15, ord("b"): 12, 265: 13, 256: 14})
    dist_lens = W.staircase_placing(16, list(range(16)), {4: 9, 7: 15})
    cycle = [lit(ord("c")), lit(ord("a")), match(3, 1), lit(ord("b")), match(11, 5), lit(ord("d")), match(12, 13), match(3, 2), lit(ord("a")),
             lit(ord("e")), match(11, 16)]
    toks = lits(b"abcdefghijklmabc") + cycle * 20
    for t in range(48):
        out.append(build("guard_cut%d" % t, [dynamic(toks[:len(toks) - t], lit_lens, dist_lens)]))
        if t % 8 == 0:
            out.append(build("guard_cut%d_two_blocks" % t, [dynamic(toks[:len(toks) - t], lit_lens, dist_lens), fixed(lits(b"tail"))]))


# ---- many blocks per stream
def _many_blocks(out, rng):
    long_lit = W.staircase_placing(266, STAIR_SYMS, {ord("a"): 15, 256: 15, 265: 11})
    long_dist = W.staircase_placing(16, list(range(16)), {4: 15})
    for j in range(4):
        blocks = []
        for k in range(100):
            if k % 2 == j % 2:
                blocks.append(dynamic(lits(b"am") + [match(11 + k % 2, 5 + k % 2)], long_lit, long_dist))
            else:
                blocks.append(dynamic(lits(b"cab"[:1 + k % 3]) + [match(3 + k % 2, 1)], SMALL_LIT, [1]))
        out.append(build("hundred_blocks_alternating_sets_%d" % j, [fixed(lits(b"0123456"[:j + 5]))] + blocks))
    # a full distance set, then a one-code set: the pattern the second leaves unused was a code of the first
    lit_lens, dist_lens = full_codes()
    first = dynamic(lits(b"abcdefgh") + [match(3, d) for d in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25)], lit_lens, dist_lens)
    out.append(build("full_dist_set_then_one_code", [first, dynamic([lit(ord("a")), match(3, 1)], SMALL_LIT, [1])]))
    for k in range(4):
        out.append(build("full_dist_set_then_unused_pattern_%d" % k,
                         [first, dynamic(lits(b"abc"[:k]) + [litsym(257), rawbits(1, 1)] + [rawbits(rng.getrandbits(8), 8)] * k, SMALL_LIT, [1])],
                         isize=64, reason="the unused pattern of a one-code distance set, a code of the block before"))


# ---- refusals a compressor cannot produce
def _refusals(out, rng):
    a, b = ord("a"), ord("b")
    toks = lits(b"abcab") + [match(3, 1), match(4, 2)]
    seq = SMALL_LIT + [1, 1]
    out.append(build("small_dynamic_valid", [dynamic(toks, SMALL_LIT, [1, 1])]))
    for f in (30, 31):
        out.append(build("hlit_field_%d" % f, [dynamic(toks, SMALL_LIT, [1, 1], hlit_field=f)], reason="HLIT > 286", err=ERR_HEADER))
        out.append(build("hdist_field_%d" % f, [dynamic(toks, SMALL_LIT, [1, 1], hdist_field=f)], reason="HDIST > 30", err=ERR_HEADER))
    out.append(build("repeat_first", [dynamic([], SMALL_LIT, [1, 1], cl_syms=[(16, 0)] + [(v, 0) for v in seq[3:]], eob=False)], isize=12,
                     reason="symbol 16 with nothing before it", err=ERR_HEADER))
    for name, tail in (("16", [(1, 0), (16, 0)]), ("17", [(17, 0)]), ("18", [(18, 127)]), ("17_by_one", [(1, 0), (17, 0)])):
        head = seq[:-2] if name != "17_by_one" else seq[:-3]
        out.append(build("repeat_%s_beyond_hlit_hdist" % name, [dynamic([], SMALL_LIT, [1, 1], cl_syms=[(v, 0) for v in head] + tail, eob=False)],
                         isize=12, reason="a repeat beyond HLIT + HDIST", err=ERR_HEADER))
    no_eob = [0] * 257
    no_eob[a] = no_eob[b] = 1
    out.append(build("no_eob_code", [dynamic([], no_eob, [1, 1], eob=False)], isize=12, reason="no end-of-block code", err=ERR_CODES))

    def lens_of(pairs, n=257):
        v = [0] * n
        for s, l in pairs.items():
            v[s] = l
        return v
    for name, lit_lens, dist_lens in (("oversubscribed_lit", lens_of({a: 1, b: 1, 256: 1}), [1, 1]),
                                      ("oversubscribed_lit_long", lens_of({a: 1, b: 2, 99: 2, 256: 15}), [1, 1]),
                                      ("oversubscribed_dist", SMALL_LIT, [1, 1, 1]),
                                      ("oversubscribed_dist_long", SMALL_LIT, [1, 2, 2, 9])):
        out.append(build(name, [dynamic([], lit_lens, dist_lens, eob=False)], isize=12, reason=name.replace("_", " "), err=ERR_CODES))
    # incomplete sets, each with symbols behind its header that a decoder which took the set would decode to ISIZE bytes
    for name, lit_lens, dist_lens, toks2 in (("incomplete_lit", lens_of({a: 2, b: 2, 256: 2}), [1, 1], lits(b"abba")),
                                             ("incomplete_lit_one_code_of_two_bits", lens_of({256: 2}), [1, 1], []),
                                             ("incomplete_lit_long", lens_of({a: 1, b: 2, 256: 15}), [1, 1], lits(b"abab")),
                                             ("incomplete_lit_with_matches", lens_of({a: 2, 256: 2, 257: 2}, 258), [1], [lit(a), match(3, 1)]),
                                             ("incomplete_dist", SMALL_LIT, [2], lits(b"ab") + [match(3, 1)]),
                                             ("incomplete_dist_two_codes", SMALL_LIT, [0, 2, 2], lits(b"abc") + [match(3, 2), match(4, 3)]),
                                             ("incomplete_dist_long", SMALL_LIT, [1, 2, 3, 15], lits(b"abcc") + [match(3, 1), match(3, 4)]),
                                             ("incomplete_dist_long_codes_only", SMALL_LIT, [0, 9, 15], lits(b"abc") + [match(3, 2), match(4, 3)]),
                                             ("incomplete_dist_unused", SMALL_LIT, [3, 3], lits(b"abcabc"))):
        s = build(name, [dynamic(toks2, lit_lens, dist_lens)], reason=name.replace("_", " "), err=ERR_CODES)
        assert s.data is not None and s.isize == len(s.data)
        out.append(s)
    used = sorted({s for s, _ in W.run_length(seq)})
    for name, l in (("oversubscribed", 1), ("incomplete", 3)):
        cl_lens = lens_of({s: l for s in used}, 19)
        assert (W.kraft(cl_lens, 7) > 128) if l == 1 else (W.kraft(cl_lens, 7) < 128)
        out.append(build(name + "_code_length_set", [dynamic([], SMALL_LIT, [1, 1], cl_lens=cl_lens, eob=False)], isize=12,
                         reason=name + " code-length set", err=ERR_CODES))
    out.append(build("one_code_length_code", [dynamic([], [0] * 256 + [1], [1], cl_lens=lens_of({1: 1}, 19), cl_syms=[], eob=False)], isize=0,
                     reason="incomplete code-length set (one code)", err=ERR_CODES))
    for s in (286, 287):
        out.append(build("fixed_symbol_%d" % s, [fixed([lit(a), litsym(s)])], isize=12, reason="literal/length symbol %d" % s))
        out.append(build("fixed_symbol_%d_far_in" % s, [fixed(lits(b"abcdefghijkl" * 6) + [litsym(s)])], isize=80,
                         reason="literal/length symbol %d" % s))
    for d in (30, 31):
        out.append(build("fixed_distance_%d" % d, [fixed(lits(b"abc") + [litsym(257), distsym(d)])], isize=12, reason="distance symbol %d" % d))
        out.append(build("fixed_distance_%d_long_match" % d, [fixed(lits(b"abc") + [litsym(285), distsym(d)])], isize=300,
                         reason="distance symbol %d" % d))
    out.append(build("block_type_3", [reserved()], isize=0, reason="block type 3", err=ERR_TYPE))
    out.append(build("block_type_3_second", [fixed(lits(b"abc")), reserved()], isize=3, reason="block type 3", err=ERR_TYPE))
    out.append(build("block_type_3_after_stored", [stored(b"abcdefg"), reserved()], isize=7, reason="block type 3", err=ERR_TYPE))
    out.append(build("stored_length_past_payload", [stored(b"abc", length=8)], isize=8, reason="a stored length past the payload"))
    out.append(build("stored_length_past_payload_far", [fixed(lits(b"ab")), stored(b"abc" * 30, length=60000)], isize=60002,
                     reason="a stored length past the payload"))
    out.append(build("stored_wrong_nlen", [stored(b"abcde", nlen=0x1234)], isize=5, reason="NLEN", err=ERR_STORED))
    out.append(build("stored_nlen_equals_len", [fixed(lits(b"a")), stored(b"abcde", nlen=5)], isize=6, reason="NLEN", err=ERR_STORED))
    out.append(build("stored_nlen_one_bit_off", [stored(b"abcde" * 20, nlen=(100 ^ 0xFFFF) ^ 0x8000)], isize=100, reason="NLEN", err=ERR_STORED))
    # one byte beyond ISIZE, by every way of writing a byte; one byte short of it
    long_lit = W.staircase_placing(266, STAIR_SYMS, {ord("a"): 15, 256: 9, 265: 12})
    stair_dist = W.staircase_placing(16, list(range(16)), {4: 9})
    for name, blocks in (("fast_literal", [fixed(lits(b"abcdefgh"))]),
                         ("slow_literal", [dynamic(lits(b"bcda"), long_lit, stair_dist)]),
                         ("fast_match", [fixed(lits(b"abcdefgh") + [match(8, 8)])]),
                         ("general_match", [fixed(lits(b"abcdefgh") + [match(100, 8)])]),
                         ("slow_match", [dynamic(lits(b"bcdefg") + [match(12, 6)], long_lit, stair_dist)]),
                         ("far_match", [stored(_rand(rng, 5000)), fixed([match(20, 4500)])]),
                         ("stored", [stored(b"abcdefgh")]),
                         ("stored_second", [fixed(lits(b"abc")), stored(b"abcdefgh" * 9)])):
        s = build("x", blocks)
        out.append(build("beyond_isize_" + name, blocks, isize=len(s.data) - 1, reason="output one byte beyond ISIZE"))
        out.append(build("short_of_isize_" + name, blocks, isize=len(s.data) + 1, reason="output one byte short of ISIZE"))
    # distances beyond the block's start
    for name, blocks in (("match_at_o0", [fixed([match(3, 1)])]),
                         ("match_at_o0_dynamic", [dynamic([match(3, 1)], SMALL_LIT, [1])]),
                         ("general_match_at_o0", [fixed([match(100, 1)])]),
                         ("dist_o_plus_1", [fixed(lits(b"abcde") + [match(3, 6)])]),
                         ("dist_o_plus_1_general", [fixed(lits(b"abcde") + [match(100, 6)])]),
                         ("dist_o_plus_1_slow", [dynamic(lits(b"bcde") + [match(12, 5)], long_lit, stair_dist)]),
                         ("dist_o_plus_1_at_100", [fixed(lits(b"abcde" * 20) + [match(30, 101)])]),
                         ("dist_o_plus_1_far", [stored(_rand(rng, 4999)), fixed([match(20, 5000)])]),
                         ("dist_32768_at_o_32767", [stored(_rand(rng, 32767)), fixed([match(3, 32768)])])):
        # (ISIZE: room for everything in front of the match and for the match, so that the distance is the one thing wrong)
        room = sum(len(b["data"]) if b["kind"] == "stored" else sum(t[1] if t[0] == "match" else 1 for t in b["tokens"]) for b in blocks)
        out.append(build(name, blocks, isize=room, reason="a distance beyond the block's start", err=ERR_DISTANCE))


# ---- truncation
def _truncation_bases(out, rng):
    text = b"the quick brown fox jumps over the lazy dog; "
    toks = lits(text) + [match(20, len(text)), match(4, 3)] + lits(b"the end") + [match(258, 1), match(30, 40)] + lits(_rand(rng, 60))
    out.append(build("trunc_fixed", [fixed(toks)]))
    lit_lens = W.staircase_placing(266, STAIR_SYMS, {256: 12, 265: 10})
    dist_lens = W.staircase_placing(16, list(range(16)), {4: 8})
    out.append(build("trunc_dynamic", [dynamic(STAIR_TOKENS * 3, lit_lens, dist_lens), dynamic(toks[:60], *full_codes())]))
    out.append(build("trunc_mixed", [fixed(toks[:50]), stored(b""), dynamic(STAIR_TOKENS, lit_lens, dist_lens), stored(_rand(rng, 10)),
                                     fixed([match(9, 5)] + lits(b"xyz")), stored(b""), stored(_rand(rng, 70))]))
    # long runs to the very end: the last bytes of input still have hundreds of bytes of output in front of them, and the stream's last
    # byte holds nothing but zero bits of the end-of-block code -- what follows a payload in memory may look just like it
    out.append(build("trunc_runs", [fixed(lits(b"ab") + [match(258, 2)] * 10 + lits(b"c"))]))
    assert out[-1].comp[-1] == 0
    for s in out[-4:]:
        assert len(s.comp) <= 300, (s.name, len(s.comp))


TRUNCATED = ("trunc_fixed", "trunc_dynamic", "trunc_mixed", "trunc_runs")


# ---- stored blocks entered at every bit
def _stored_entries(out, rng):
    for k in range(8):
        # k one-bit literals and a 15-bit end-of-block in front of every stored block (which ends on a byte boundary: the next
        # header starts at bit 0 again and the stored block behind it is entered at the same bit); every size class four times
        blocks = []
        for n in (0, 1, 64, 1024, 0, 63, 65, 1100, 0, 17, 100, 1024 + k, 0, 40, 200, 2000):
            blocks += [dynamic([lit(X)] * k, SLIDE_LIT, SLIDE_DIST), stored(_rand(rng, n))]
        out.append(build("stored_blocks_entered_after_%d_bits" % k, blocks))
    for n in (65535, 65534):
        out.append(build("stored_%d" % n, [stored(_rand(rng, n)), stored(_rand(rng, 65536 - n))]))


# ---- random valid streams
def _random_lengths(rng, n_syms, must, n_codes):
    """A random complete set of code lengths in which the symbols of `must` have codes."""
    lens = [1, 1]
    while len(lens) < n_codes:
        i = rng.choice([k for k, l in enumerate(lens) if l < 15])
        lens[i:i + 1] = [lens[i] + 1, lens[i] + 1]
    rng.shuffle(lens)
    syms = list(must) + rng.sample([s for s in range(n_syms) if s not in must], n_codes - len(must))
    out = [0] * n_syms
    for s, l in zip(syms, lens):
        out[s] = l
    return out


EDGE_LENS = (3, 4, 10, 11, 62, 63, 64, 65, 130, 131, 227, 257, 258)
EDGE_DISTS = (1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8192, 16384, 32767, 32768)


def _random_tokens(rng, o, room, lit_ok, len_ok, dist_ok):
    """Random tokens from position o for at most `room` bytes, out of the symbols that have codes; weight on the edges."""
    toks = []
    lits_ok = [s for s in range(256) if lit_ok[s]]
    while room > 0:
        r = rng.random()
        if r < 0.45 or o == 0:
            toks.append(lit(rng.choice(lits_ok)))
            o += 1
            room -= 1
            continue
        for _ in range(8):
            length = rng.choice(EDGE_LENS) if r < 0.75 else rng.randrange(3, 259)
            if r < 0.6:
                dist = rng.choice(EDGE_DISTS + (length - 1, length, length + 1, o, 4096 - 64 - length, 4096 - 63 - length))
            else:
                dist = rng.randrange(1, min(o, 32768) + 1) if r < 0.9 else rng.randrange(1, min(o, 64) + 1)
            if not (1 <= dist <= min(o, 32768)) or length > room:
                continue
            ls, ds = W.length_symbol(length)[0], W.dist_symbol(dist)[0]
            if len_ok[ls] and dist_ok[ds]:
                toks.append(match(length, dist))
                o += length
                room -= length
                break
        else:
            toks.append(lit(rng.choice(lits_ok)))
            o += 1
            room -= 1
    return toks, o


def random_stream(rng, name, max_out):
    blocks, o = [], 0
    target = rng.randrange(max_out // 4, max_out + 1)
    while o < target:
        room = min(target - o, rng.choice((50, 700, 5000, 40000)))
        kind = rng.random()
        if kind < 0.15:
            n = min(room, rng.choice((0, 1, 63, 64, 1000, 5000)))
            blocks.append(stored(_rand(rng, n)))
            o += n
        elif kind < 0.35:
            toks, o = _random_tokens(rng, o, room, [1] * 256, [1] * 286, [1] * 30)
            blocks.append(fixed(toks))
        else:
            n_lit = rng.choice((20, 60, 286))
            must = [256] + rng.sample(range(256), 4) + rng.sample(range(257, 286), 6)
            lit_lens = _random_lengths(rng, 286, must, n_lit)
            n_dist = rng.choice((2, 8, 30))
            dist_lens = _random_lengths(rng, 30, rng.sample(range(30), 2), n_dist)
            toks, o = _random_tokens(rng, o, room, lit_lens, lit_lens, dist_lens)
            blocks.append(dynamic(toks, lit_lens, dist_lens, runs=rng.random() < 0.8, span=rng.random() < 0.7))
    return build(name, blocks)


def _random(out, rng, count, max_out, prefix):
    for k in range(count):
        out.append(random_stream(rng, "%s_%d" % (prefix, k), max_out))


@functools.lru_cache(maxsize=None)
def catalogue():
    """Every stream, valid (reason None) and to be refused, under a name of its own."""
    out = []
    _staircases(out)
    _code_shapes(out)
    _matches(out, random.Random(11))
    _bit_positions(out, random.Random(12))
    _guard(out, random.Random(13))
    _many_blocks(out, random.Random(14))
    _refusals(out, random.Random(15))
    _truncation_bases(out, random.Random(16))
    _stored_entries(out, random.Random(17))
    _random(out, random.Random(18), N_RANDOM, 40 * 1024, "random")
    _random(out, random.Random(19), 150, 64, "random_small")
    names = [s.name for s in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(out)


def valid():
    return [s for s in catalogue() if s.reason is None]


def refused():
    return [s for s in catalogue() if s.reason is not None]


def small():
    """(valid, refused) streams of at most 64 bytes of output and 200 of input: what the many-block call of the GPU test cycles."""
    pick = [s for s in catalogue() if s.isize <= 64 and len(s.comp) <= 200]
    return [s for s in pick if s.reason is None], [s for s in pick if s.reason is not None]


@functools.lru_cache(maxsize=None)
def truncations():
    """Every byte prefix of four streams of at most 300 bytes: (name, prefix, isize of the whole stream)."""
    by_name = {s.name: s for s in catalogue()}
    return tuple(("%s[:%d]" % (n, k), by_name[n].comp[:k], by_name[n].isize) for n in TRUNCATED for k in range(len(by_name[n].comp)))
