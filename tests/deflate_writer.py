"""A deflate encoder that does what it is told (test-side code, written from RFC 1951).

A compressor chooses a narrow slice of the format; the block decoders (csrc/inflate_kernel.hip, host/inflate.cpp) must take all of
it.  This writer emits a raw deflate stream from an explicit list of blocks -- stored(bytes), fixed(tokens),
dynamic(tokens, lit_lens, dist_lens, header options), reserved() -- with canonical codes built from caller-given code lengths, a
header encoder whose code-length code and 16/17/18 runs are inputs, and raw symbol escapes for streams that must be refused.
build() returns the bytes, the data they should inflate to (the tokens applied in plain Python) or the reason for refusal, and
the bit positions of every header, length/distance pair and end-of-block it wrote.
"""
import collections

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


class BitWriter:
    """Bits in the order deflate packs them: the first bit written is bit 0 of byte 0."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.nacc = 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.nacc

    def put(self, val, nbits):
        assert 0 <= val < (1 << nbits), (val, nbits)
        self.acc |= val << self.nacc
        self.nacc += nbits
        while self.nacc >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nacc -= 8

    def put_code(self, code, length):
        """A Huffman code: most significant bit first."""
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.nacc:
            self.put(0, 8 - self.nacc)

    def put_bytes(self, data):
        assert self.nacc == 0
        self.out += data

    def getvalue(self):
        w = BitWriter()
        w.out, w.acc, w.nacc = bytearray(self.out), self.acc, self.nacc
        w.align()
        return bytes(w.out)


def canonical_codes(lens):
    """RFC 1951 3.2.2: the code of every symbol with a non-zero length (None for the others)."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, next_code = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        next_code[b] = code
    codes = [None] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = next_code[l] & ((1 << l) - 1)               # (an over-subscribed set runs out of patterns: kept in range)
            next_code[l] += 1
    return codes


def kraft(lens, maxbits=15):
    """The Kraft sum of a set of code lengths in units of 2^-maxbits (complete: 1 << maxbits)."""
    return sum(1 << (maxbits - l) for l in lens if l)


def fill_lengths(n_codes, budget, maxbits):
    """n_codes lengths (ascending) whose Kraft sum is exactly `budget` units of 2^-maxbits: the set bits of the budget, the shortest
    code split in two until there are enough.  The budget's popcount <= n_codes <= budget must hold."""
    lens = [maxbits - b for b in range(maxbits, -1, -1) if (budget >> b) & 1]
    assert len(lens) <= n_codes <= budget, (n_codes, budget, maxbits)
    while len(lens) < n_codes:
        lens.sort()
        i = next(k for k, l in enumerate(lens) if l < maxbits)
        lens[i:i + 1] = [lens[i] + 1, lens[i] + 1]
    assert all(l >= 1 for l in lens), (n_codes, budget, maxbits)
    return sorted(lens)


def lengths_with(n_syms, forced, used, pool=(), maxbits=15):
    """A complete set of code lengths over n_syms symbols in which symbol s has length forced[s], every symbol of `used` has a code
    (the earlier in `used`, the shorter) and symbols of `pool` are given codes only where completeness needs more of them."""
    lens = [0] * n_syms
    for s, l in forced.items():
        lens[s] = l
    budget = (1 << maxbits) - kraft(lens, maxbits)
    rest = [s for s in used if s not in forced]
    extra = [s for s in pool if s not in forced and s not in rest]
    need = bin(budget).count("1") if budget else 0
    while len(rest) < need:
        rest.append(extra.pop(0))
    if budget == 0:
        assert not rest
        return lens
    for s, l in zip(rest, fill_lengths(len(rest), budget, maxbits)):
        lens[s] = l
    assert kraft(lens, maxbits) == 1 << maxbits
    return lens


def staircase(n_syms, order, maxbits=15):
    """Lengths 1, 2, ..., maxbits - 1, maxbits, maxbits (Kraft sum 1) for the maxbits + 1 symbols of `order`, in that order."""
    assert len(order) == maxbits + 1 and len(set(order)) == len(order)
    lens = [0] * n_syms
    for i, s in enumerate(order):
        lens[s] = min(i + 1, maxbits)
    return lens


def staircase_placing(n_syms, syms, placed, maxbits=15):
    """The staircase over `syms` (maxbits + 1 of them) permuted so that placed = {symbol: length} holds."""
    slots = list(range(1, maxbits + 1)) + [maxbits]
    lens = [0] * n_syms
    for s, l in placed.items():
        slots.remove(l)
        lens[s] = l
    for s in syms:
        if s not in placed:
            lens[s] = slots.pop(0)
    assert not slots
    return lens


def length_symbol(length, alt258=False):
    """(symbol, extra bits, extra value) of a match length; alt258: 258 as symbol 284 with extra value 31."""
    if length == 258:
        return (284, 5, 31) if alt258 else (285, 0, 0)
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i])
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    assert dist - DIST_BASE[i] < (1 << DIST_EXTRA[i])
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


# ---- tokens
def lit(b):
    return ("lit", b)


def match(length, dist, alt258=False):
    return ("match", length, dist, alt258)


def litsym(sym, ebits=0, evalue=0):
    """A raw literal/length symbol (with its extra bits): whatever the tables say, for streams that must be refused."""
    return ("litsym", sym, ebits, evalue)


def distsym(sym, ebits=0, evalue=0):
    return ("distsym", sym, ebits, evalue)


def rawbits(value, nbits):
    return ("rawbits", value, nbits)


def lits(data):
    return [("lit", b) for b in data]


def apply_tokens(tokens, out):
    """The tokens applied to `out` (bytearray) in plain Python.  False: a token no decoder may accept (the caller names the reason)."""
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            _, length, dist, _ = t
            if dist > len(out):
                return False
            for _ in range(length):
                out.append(out[-dist])
        elif t[0] == "litsym" and t[1] < 256:
            out.append(t[1])
        else:
            return False
    return True


# ---- blocks
def stored(data, length=None, nlen=None):
    """length / nlen: the header fields if they are to differ from len(data) / its complement."""
    return dict(kind="stored", data=bytes(data), length=length, nlen=nlen)


def fixed(tokens, eob=True):
    return dict(kind="fixed", tokens=list(tokens), eob=eob)


def dynamic(tokens, lit_lens, dist_lens, cl_lens=None, hclen=None, runs=True, span=True, cl_syms=None, cl_forced=None, eob=True,
            hlit_field=None, hdist_field=None):
    """lit_lens / dist_lens: HLIT / HDIST of them.  cl_lens: the code-length code (default: a complete one over the symbols used, with
    cl_forced = {symbol: length}); hclen: how many of its lengths are sent (4..19; default: as few as possible); runs: use symbols 16,
    17 and 18 (greedily); span: a run may cross from the literal/length lengths into the distance lengths; cl_syms: the header's
    code-length symbols [(symbol, extra value)] given outright; hlit_field / hdist_field: the raw 5-bit fields."""
    return dict(kind="dynamic", tokens=list(tokens), lit_lens=list(lit_lens), dist_lens=list(dist_lens), cl_lens=cl_lens, hclen=hclen,
                runs=runs, span=span, cl_syms=cl_syms, cl_forced=cl_forced, eob=eob, hlit_field=hlit_field, hdist_field=hdist_field)


def reserved():
    """Block type 3."""
    return dict(kind="reserved")


def run_length(seq, boundary=None):
    """The greedy 16/17/18 encoding of a sequence of code lengths; boundary: an index no run may cross."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v and (boundary is None or not (i < boundary <= i + r)):
            r += 1
        if v == 0 and r >= 3:
            k = min(r, 138)
            out.append((18, k - 11) if k >= 11 else (17, k - 3))
            i += k
            continue
        out.append((v, 0))
        i += 1
        r -= 1
        while v != 0 and r >= 3:
            k = min(r, 6)
            out.append((16, k - 3))
            i += k
            r -= k
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}

Stream = collections.namedtuple("Stream", "name comp data isize reason err marks")
# marks: [(kind, first bit, bit behind the last)] with kind in dynamic_header, stored_header, pair, eob


def _write_symbols(w, tokens, lit_lens, dist_lens, eob, marks):
    lit_codes, dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)

    def put_lit(sym, ebits, evalue):
        assert lit_lens[sym], ("no code for literal/length symbol", sym)
        w.put_code(lit_codes[sym], lit_lens[sym])
        w.put(evalue, ebits)

    def put_dist(sym, ebits, evalue):
        assert dist_lens[sym], ("no code for distance symbol", sym)
        w.put_code(dist_codes[sym], dist_lens[sym])
        w.put(evalue, ebits)

    for t in tokens:
        if t[0] == "lit":
            put_lit(t[1], 0, 0)
        elif t[0] == "match":
            at = w.bitpos
            put_lit(*length_symbol(t[1], t[3]))
            put_dist(*dist_symbol(t[2]))
            marks.append(("pair", at, w.bitpos))
        elif t[0] == "litsym":
            put_lit(t[1], t[2], t[3])
        elif t[0] == "distsym":
            put_dist(t[1], t[2], t[3])
        elif t[0] == "rawbits":
            w.put(t[1], t[2])
        else:
            raise ValueError(t)
    if eob:
        at = w.bitpos
        put_lit(256, 0, 0)
        marks.append(("eob", at, w.bitpos))


def write_block(w, blk, final, marks):
    if blk["kind"] == "stored":
        at = w.bitpos
        w.put(1 if final else 0, 1)
        w.put(0, 2)
        w.align()
        n = len(blk["data"]) if blk["length"] is None else blk["length"]
        w.put(n, 16)
        w.put((n ^ 0xFFFF) if blk["nlen"] is None else blk["nlen"], 16)
        marks.append(("stored_header", at, w.bitpos))
        w.put_bytes(blk["data"])
        return
    if blk["kind"] == "reserved":
        w.put(1 if final else 0, 1)
        w.put(3, 2)
        return
    if blk["kind"] == "fixed":
        w.put(1 if final else 0, 1)
        w.put(1, 2)
        _write_symbols(w, blk["tokens"], FIXED_LIT_LENS, FIXED_DIST_LENS, blk["eob"], marks)
        return
    at = w.bitpos
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    lit_lens, dist_lens = blk["lit_lens"], blk["dist_lens"]
    w.put(len(lit_lens) - 257 if blk["hlit_field"] is None else blk["hlit_field"], 5)
    w.put(len(dist_lens) - 1 if blk["hdist_field"] is None else blk["hdist_field"], 5)
    seq = lit_lens + dist_lens
    cl_syms = blk["cl_syms"]
    if cl_syms is None:
        cl_syms = run_length(seq, None if blk["span"] else len(lit_lens)) if blk["runs"] else [(v, 0) for v in seq]
    cl_lens = blk["cl_lens"]
    if cl_lens is None:
        freq = collections.Counter(s for s, _ in cl_syms)
        used = [s for s, _ in freq.most_common()]
        cl_lens = lengths_with(19, blk["cl_forced"] or {}, used, [s for s in (0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15, 16, 17, 18)],
                               maxbits=7)
        if sum(1 for l in cl_lens if l) == 1:                      # one code alone is an incomplete set: a second one nobody uses
            cl_lens = lengths_with(19, {}, used + [s for s in (0, 8, 7) if s not in used][:1], maxbits=7)
    hclen = blk["hclen"]
    if hclen is None:
        hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
    assert 4 <= hclen <= 19
    w.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.put(cl_lens[s], 3)
    cl_codes = canonical_codes(cl_lens)
    for s, extra in cl_syms:
        assert cl_lens[s], ("no code for code-length symbol", s)
        w.put_code(cl_codes[s], cl_lens[s])
        if s >= 16:
            w.put(extra, CL_EXTRA[s])
    marks.append(("dynamic_header", at, w.bitpos))
    full_lit = (lit_lens + [0] * 288)[:288]
    full_dist = (dist_lens + [0] * 32)[:32]
    _write_symbols(w, blk["tokens"], full_lit, full_dist, blk["eob"], marks)


def build(name, blocks, isize=None, reason=None, err=None, last_is_final=True):
    """The stream of `blocks` (the last one marked final).  reason None: a valid stream, whose data is what the tokens give; a string: why
    every decoder must refuse it (err: the device's status where the kernel has one unambiguous code for it).  isize: what the
    block's trailer would say (default: the size of the data)."""
    w = BitWriter()
    marks = []
    out = bytearray()
    ok = True
    for i, blk in enumerate(blocks):
        write_block(w, blk, last_is_final and i == len(blocks) - 1, marks)
        if not ok:
            continue
        if blk["kind"] == "stored":
            out += blk["data"]
            ok = blk["length"] is None and blk["nlen"] is None
        elif blk["kind"] == "reserved":
            ok = False
        else:
            ok = apply_tokens(blk["tokens"], out)
    if reason is None:
        assert ok, name + ": tokens that cannot be applied in a stream meant to be valid"
        data = bytes(out)
        return Stream(name, w.getvalue(), data, len(data) if isize is None else isize, None, None, marks)
    return Stream(name, w.getvalue(), bytes(out) if ok else None, len(out) if isize is None else isize, reason, err, marks)
