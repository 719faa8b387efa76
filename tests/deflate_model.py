"""A plain Python inflate (RFC 1951) with a census of the paths the device kernel would take.

A third decoder beside csrc/inflate_kernel.hip and host/inflate.cpp: slow and obvious -- one bit at a time through the canonical
codes -- with zlib's acceptance rules (over-subscribed sets refused; incomplete ones too, unless a literal/length or distance set has
a single one-bit code or none at all).  Beside the output, or the reason for refusal, inflate() counts which path of the device
kernel every event of the stream takes, from the five constants below; tests/test_deflate_streams.py compares them with the text of
inflate_kernel.hip, so the census cannot go stale unnoticed, and demands a floor for every class, so the device test cannot pass
without having met the edge.
"""
import collections

# ---- what the census knows of csrc/inflate_kernel.hip
RING = 4096            # BVC_INFLATE_WINDOW: the LDS ring of a block's last output bytes
LIT_BITS = 9           # kLitBits: the first-level table of literal/length codes; longer codes take slow()
DIST_BITS = 7          # kDistBits: the same for distance codes
FAST_COPY = 63         # fast_symbols: a pair's pieces lie in lanes 0..63 of the batch; a fast copy is at most 63 bytes
READER_WINDOW = 1920   # the reader's window moves on at bp >= 1920 bits (60 words of the 64 a register holds; the next 4: 2048)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STRADDLE_BITS = (READER_WINDOW, READER_WINDOW + 128)

Result = collections.namedtuple("Result", "data error census")


class Refused(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.end = data, 0, 8 * len(data)

    def take(self, n):
        if self.pos + n > self.end:
            raise Refused("input")
        v = 0
        for i in range(n):
            p = self.pos + i
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << i
        self.pos += n
        return v


def _code(lens, may_be_short, what):
    """{(length, code): symbol} of a canonical code, or Refused: the sets zlib refuses."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise Refused("codes: over-subscribed " + what)
    longest = max([l for l in range(1, 16) if count[l]] + [0])
    if left > 0 and not (may_be_short and longest <= 1):
        raise Refused("codes: incomplete " + what)
    code, next_code = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        next_code[l] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, next_code[l])] = s
            next_code[l] += 1
    return table


def _symbol(b, table, what):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | b.take(1)
        s = table.get((l, code))
        if s is not None:
            return s, l
    raise Refused("symbol: no such " + what + " code")


def inflate(comp, isize=None):
    """Result(data, None, census) for a valid stream (isize given: that produces exactly so many bytes), Result(None, reason, census)
    for one that must be refused."""
    census = collections.Counter()
    out = bytearray()
    try:
        _inflate(comp, isize, out, census)
    except Refused as r:
        return Result(None, str(r), census)
    return Result(bytes(out), None, census)


def _straddles(census, kind, first, behind):
    """An object of the stream (bits first..behind-1) that lies across bit 1920 or 2048 of the payload's first word, at every
    alignment `lead` of the payload in its word."""
    for lead in range(4):
        for edge in STRADDLE_BITS:
            if first + 8 * lead < edge < behind + 8 * lead:
                census["%s across bit %d, lead %d" % (kind, edge, lead)] += 1


def _inflate(comp, isize, out, census):
    b = _Bits(comp)
    limit = isize if isize is not None else 1 << 62
    last = False
    n_block = 0
    prev_tables = None
    while not last:
        at = b.pos
        last = b.take(1) == 1
        kind = b.take(2)
        n_block += 1
        if kind == 0:
            entered = at & 7
            b.pos = (b.pos + 7) & ~7
            n = b.take(16)
            if b.take(16) != n ^ 0xFFFF:
                raise Refused("stored: NLEN")
            _straddles(census, "stored header", at, b.pos)
            if len(out) + n > limit:
                raise Refused("output")
            if b.pos + 8 * n > b.end:
                raise Refused("input: stored length past the payload")
            for cls, ok in (("0", n == 0), ("1..63", 1 <= n <= 63), ("64+", n >= 64), ("1024+", n >= 1024)):
                if ok:
                    census["stored block of %s bytes entered at bit %d" % (cls, entered)] += 1
            if len(out) // 1024 != (len(out) + n) // 1024:
                census["stored bytes across a multiple of 1024"] += 1
            out += comp[b.pos >> 3:(b.pos >> 3) + n]
            b.pos += 8 * n
            continue
        if kind == 3:
            raise Refused("type")
        if kind == 1:
            lit_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
            dist_lens = [5] * 32
        else:
            hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
            if hlit > 286 or hdist > 30:
                raise Refused("header: HLIT or HDIST")
            cl_lens = [0] * 19
            for i in range(hclen):
                cl_lens[CL_ORDER[i]] = b.take(3)
            cl = _code(cl_lens, False, "code-length set")
            lens = []
            while len(lens) < hlit + hdist:
                s, _ = _symbol(b, cl, "code-length")
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise Refused("header: repeat with nothing before it")
                    v, rep = lens[-1], 3 + b.take(2)
                elif s == 17:
                    v, rep = 0, 3 + b.take(3)
                else:
                    v, rep = 0, 11 + b.take(7)
                if len(lens) + rep > hlit + hdist:
                    raise Refused("header: repeat beyond HLIT + HDIST")
                census["header run: symbol %d, %d times" % (s, rep)] += 1
                if len(lens) < hlit < len(lens) + rep:
                    census["header run across the literal/distance boundary"] += 1
                lens += [v] * rep
            if lens[256] == 0:
                raise Refused("codes: no end-of-block code")
            lit_lens, dist_lens = lens[:hlit], lens[hlit:]
            _straddles(census, "dynamic header", at, b.pos)
            if max(cl_lens) == 7:
                census["dynamic header with 7-bit code-length codes"] += 1
        lit = _code(lit_lens, True, "literal/length set")
        dist = _code(dist_lens, True, "distance set")
        if prev_tables is not None and prev_tables != (lit_lens, dist_lens):
            census["later block with other tables than the block before"] += 1
        prev_tables = (lit_lens, dist_lens)
        _symbols(b, lit, dist, out, limit, census)
    if isize is not None and len(out) != isize:
        raise Refused("size")


def _symbols(b, lit, dist, out, limit, census):
    off = 0                      # the device's position in its batch of 64 lanes (a block's symbols start a batch)
    prev = None                  # the match before this symbol, if the symbol before was one: (destination, length, far)
    while True:
        if off > FAST_COPY:
            off = 0
        at = b.pos
        s, l = _symbol(b, lit, "literal/length")
        if s < 256:
            if len(out) >= limit:
                raise Refused("output")
            census["literal of the first level" if l <= LIT_BITS else "literal by slow()"] += 1
            if (len(out) + 1) % 1024 == 0:
                census["literal onto a multiple of 1024"] += 1
            out.append(s)
            off += l
            prev = None
            continue
        if s == 256:
            census["end-of-block of 1..9 bits" if l <= LIT_BITS else "end-of-block of 10..15 bits"] += 1
            _straddles(census, "end-of-block", at, b.pos)
            return
        if s > 285:
            raise Refused("symbol: literal/length 286 or 287")
        xb = LEN_EXTRA[s - 257]
        length = LEN_BASE[s - 257] + b.take(xb)
        d, dl = _symbol(b, dist, "distance")
        if d > 29:
            raise Refused("symbol: distance 30 or 31")
        dxb = DIST_EXTRA[d]
        distance = DIST_BASE[d] + b.take(dxb)
        _straddles(census, "pair", at, b.pos)
        if l > LIT_BITS:
            census["length symbol by slow()"] += 1
        if dl > DIST_BITS:
            census["distance symbol by slow()"] += 1
        if s == 284 and length == 258:
            census["length 258 as symbol 284"] += 1
        # the lane of the batch at which the pair's last piece (the distance's extra bits) is read: beyond 63 the batch is looked
        # up again from this symbol
        p = off + l + xb + dl
        if 62 <= p <= 65:
            census["pair whose last piece is at lane %d" % p] += 1
        if p > FAST_COPY:
            p = l + xb + dl
        off = p + dxb
        o = len(out)
        if distance > o:
            raise Refused("distance")
        if o + length > limit:
            raise Refused("output")
        first_level = l <= LIT_BITS and dl <= DIST_BITS
        if first_level and length <= FAST_COPY and distance >= length:
            far = distance + length > RING - 64
            census["fast far copy" if far else "fast near copy"] += 1
        elif distance + length + 64 <= RING:
            far = False
            if distance >= length:
                census["general near copy, dist >= len"] += 1
            elif distance & (distance - 1) == 0:
                census["general run, power-of-two dist"] += 1
            else:
                census["general run, other dist"] += 1
        else:
            far = True
            census["general far copy"] += 1
        if distance == o:
            census["match with dist == o"] += 1
        if distance + length in (RING - 65, RING - 64, RING - 63):
            census["match with dist + len == %d" % (distance + length)] += 1
        if prev is not None:
            if o - distance == prev[0]:
                census["match whose source is the previous match's destination"] += 1
            if prev[2] and not far and o - distance < prev[0] + prev[1] and o - distance + length > prev[0]:
                census["near match after a far match that reads its bytes"] += 1
        if o // 1024 != (o + length) // 1024:
            census["match across a multiple of 1024"] += 1
        if distance < length and o // RING != (o + length) // RING:
            census["run across a multiple of 4096"] += 1
        for _ in range(length):
            out.append(out[-distance])
        prev = (o, length, far)


# every class a catalogue must reach (tests/test_deflate_streams.py: at least 4 times each)
CENSUS_CLASSES = (
    ["literal of the first level", "literal by slow()", "end-of-block of 1..9 bits", "end-of-block of 10..15 bits",
     "length symbol by slow()", "distance symbol by slow()"] +
    ["pair whose last piece is at lane %d" % p for p in (62, 63, 64, 65)] +
    ["fast near copy", "fast far copy", "general near copy, dist >= len", "general run, power-of-two dist", "general run, other dist",
     "general far copy", "match with dist == o"] +
    ["match with dist + len == %d" % v for v in (RING - 65, RING - 64, RING - 63)] +
    ["match whose source is the previous match's destination", "near match after a far match that reads its bytes",
     "match across a multiple of 1024", "literal onto a multiple of 1024", "run across a multiple of 4096"] +
    ["stored block of %s bytes entered at bit %d" % (c, k) for c in ("0", "1..63", "64+", "1024+") for k in range(8)] +
    ["later block with other tables than the block before", "length 258 as symbol 284", "dynamic header with 7-bit code-length codes",
     "header run across the literal/distance boundary"] +
    ["header run: symbol %d, %d times" % sr for sr in ((16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138))])
# ... and these at every alignment of the payload
CENSUS_PER_LEAD = ["%s across bit %d, lead %%d" % (k, e) for k in ("dynamic header", "stored header", "pair", "end-of-block")
                   for e in STRADDLE_BITS]
