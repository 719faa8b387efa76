"""A plain Python model of the per-block dynamic Huffman code of the device deflate encoder (docs/BGZF_DYNAMIC.md holds the rule; the
device's copy is csrc/bgzf_codes_device.h).  encode() takes a block's symbols -- an int per literal, a (length, distance, ...) tuple per
match, as tests/bgzf_blocks.fixed_symbols returns them -- and gives the block's whole deflate data stored, in the fixed code and in the
dynamic code, and which of them the encoder writes.  read_blocks() reads deflate data back into code lengths, header symbols and
symbols.  Nothing here needs a device."""
from tests.bgzf_blocks import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}


# ---- (a), (d): code lengths from counts
def huffman_depths(counts):
    """Depths of the used symbols (two at least) in the tree of the rule, before any limit: {symbol: depth}."""
    leaves = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    assert len(leaves) >= 2
    weight, parent_of_leaf, parent_of_node = [], [0] * len(leaves), []
    li = ni = 0
    for _ in range(len(leaves) - 1):
        total = 0
        for _ in range(2):
            # the smaller weight; a leaf before an internal node of the same weight; internal nodes in the order they were made
            if li < len(leaves) and (ni >= len(weight) or leaves[li][0] <= weight[ni]):
                total += leaves[li][0]
                parent_of_leaf[li] = len(weight)
                li += 1
            else:
                total += weight[ni]
                parent_of_node[ni] = len(weight)
                ni += 1
        weight.append(total)
        parent_of_node.append(-1)
    depth = [0] * len(weight)
    for i in range(len(weight) - 2, -1, -1):
        depth[i] = depth[parent_of_node[i]] + 1
    return {leaves[i][1]: depth[parent_of_leaf[i]] + 1 for i in range(len(leaves))}


def code_lengths(counts, limit):
    """The rule's code lengths: a list as long as counts."""
    n = len(counts)
    assert 1 <= limit <= 15 and (1 << limit) >= max(n, 2)
    out = [0] * n
    used = [s for s in range(n) if counts[s] > 0]
    if len(used) < 2:
        # padding: the used symbol, if any, and the smallest unused symbols up to two in all take one bit each
        for s in used + [s for s in range(min(n, 2)) if counts[s] == 0][:2 - len(used)]:
            out[s] = 1
        return out
    depth = huffman_depths(counts)
    bl = [0] * (limit + 1)
    for d in depth.values():
        bl[min(d, limit)] += 1
    # leaves deeper than the limit now stand at the limit and the Kraft sum is above 1 by `excess` units of 2^-limit.  zlib's move takes
    # one unit away: the deepest leaf above the limit's level goes one level down, and a leaf of the limit's level becomes its sibling
    excess = sum(bl[b] << (limit - b) for b in range(1, limit + 1)) - (1 << limit)
    while excess > 0:
        bits = limit - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[limit] -= 1
        excess -= 1
    assert excess == 0 and min(bl) >= 0
    # the longest lengths to the smallest (count, symbol)
    order = sorted(used, key=lambda s: (counts[s], s))
    at = 0
    for length in range(limit, 0, -1):
        for _ in range(bl[length]):
            out[order[at]] = length
            at += 1
    assert at == len(order)
    return out


def canonical(lengths):
    """RFC 1951, 3.2.2: {symbol: (code, length)}, the code's first bit its most significant."""
    bl = [0] * 16
    for ln in lengths:
        bl[ln] += ln > 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


# ---- (b): the code-length sequence
def length_sequence(lengths):
    """[(symbol 0..18, extra value)] over HLIT + HDIST lengths as ONE row (a run crosses from the first alphabet into the second)."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, r = lengths[i], 1
        while i + r < n and lengths[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            k = min(r, 138)
            out.append((18, k - 11))
        elif v == 0 and r >= 3:
            k = r
            out.append((17, k - 3))
        elif v != 0 and i > 0 and lengths[i - 1] == v and r >= 3:
            k = min(r, 6)
            out.append((16, k - 3))
        else:
            k = 1
            out.append((v, 0))
        i += k
    return out


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):                                   # least significant bit first (extra bits, header fields)
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code_len):                                     # a Huffman code: most significant bit first
        c, ln = code_len
        self.put(int(format(c, "0%db" % ln)[::-1], 2), ln)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def length_symbol(length):
    for i in range(28, -1, -1):
        if length >= LEN_BASE[i]:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise ValueError(length)


def distance_symbol(dist):
    for i in range(29, -1, -1):
        if dist >= DIST_BASE[i]:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise ValueError(dist)


def plain_bytes(symbols):
    out = bytearray()
    for x in symbols:
        if isinstance(x, tuple):
            for _ in range(x[0]):
                out.append(out[-x[1]])
        else:
            out.append(x)
    return bytes(out)


def symbol_counts(symbols):
    ll, dl = [0] * 286, [0] * 30
    ll[256] = 1
    for x in symbols:
        if isinstance(x, tuple):
            ll[length_symbol(x[0])[0]] += 1
            dl[distance_symbol(x[1])[0]] += 1
        else:
            ll[x] += 1
    return ll, dl


FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def put_symbols(w, symbols, lit, dist):
    for x in symbols:
        if isinstance(x, tuple):
            s, eb, ev = length_symbol(x[0])
            w.code(lit[s])
            w.put(ev, eb)
            s, eb, ev = distance_symbol(x[1])
            w.code(dist[s])
            w.put(ev, eb)
        else:
            w.code(lit[x])
    w.code(lit[256])


def encode(symbols):
    """dict: stored, fixed, dynamic (the whole deflate data of the block in each form, BFINAL set), chosen ("stored" / "fixed" /
    "dynamic"), data (the chosen form), and the dynamic header: ll, dl (lengths), hlit, hdist, hclen, sequence."""
    plain = plain_bytes(symbols)
    n = len(plain)
    assert 0 < n <= 65535
    stored = bytes([1, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + plain
    w = BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    put_symbols(w, symbols, canonical(FIXED_LENGTHS), canonical([5] * 30))
    fixed = w.bytes()
    lc, dc = symbol_counts(symbols)
    ll, dl = code_lengths(lc, 15), code_lengths(dc, 15)
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = max(1, max(s for s in range(30) if dl[s]) + 1)
    seq = length_sequence(ll[:hlit] + dl[:hdist])
    cc = [0] * 19
    for s, _ in seq:
        cc[s] += 1
    cl = code_lengths(cc, 7)
    hclen = max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    w = BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl[CL_ORDER[i]], 3)
    clc = canonical(cl)
    for s, ev in seq:
        w.code(clc[s])
        w.put(ev, CL_EXTRA.get(s, 0))
    put_symbols(w, symbols, canonical(ll), canonical(dl))
    dynamic = w.bytes()
    # today's rule gives F; dynamic iff it is smaller
    f_form = "stored" if len(fixed) > n + 5 else "fixed"
    f_size = min(len(fixed), n + 5)
    chosen = "dynamic" if len(dynamic) < f_size else f_form
    forms = dict(stored=stored, fixed=fixed, dynamic=dynamic)
    return dict(forms, chosen=chosen, data=forms[chosen], ll=ll, dl=dl, hlit=hlit, hdist=hdist, hclen=hclen, sequence=seq, cl=cl)


# ---- the reader
class BitReader:
    def __init__(self, data, at=0):
        self.data, self.at, self.nbits = bytes(data), at, 8 * len(data)

    def bits(self, n):                                            # n <= 16
        assert self.at + n <= self.nbits, "read past the end of the data"
        i = self.at >> 3
        v = (int.from_bytes(self.data[i:i + 4], "little") >> (self.at & 7)) & ((1 << n) - 1)
        self.at += n
        return v

    def symbol(self, table):
        """table: {(length, code): symbol}"""
        i = self.at >> 3
        window = int.from_bytes(self.data[i:i + 4], "little") >> (self.at & 7)
        c = 0
        for ln in range(1, 16):
            c = (c << 1) | ((window >> (ln - 1)) & 1)
            if (ln, c) in table:
                assert self.at + ln <= self.nbits, "read past the end of the data"
                self.at += ln
                return table[(ln, c)]
        raise AssertionError("no such code")


def decode_table(lengths):
    return {(ln, c): s for s, (c, ln) in canonical(lengths).items()}


def read_blocks(data):
    """The deflate blocks of `data` up to and including the one with BFINAL: [dict(btype, final, symbols, and for btype 2: ll, dl, cl, hlit,
    hdist, hclen, header (the sequence's symbols 0..18))], and the bit position behind the last.  A stored block's symbols are its bytes."""
    r = BitReader(data)
    out = []
    while True:
        final, btype = r.bits(1), r.bits(2)
        blk = dict(final=final, btype=btype, symbols=[])
        assert btype != 3
        if btype == 0:
            r.at = (r.at + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n ^ nn == 0xFFFF
            blk["symbols"] = list(data[r.at // 8:r.at // 8 + n])
            assert len(blk["symbols"]) == n
            r.at += 8 * n
        else:
            if btype == 1:
                ll, dl = FIXED_LENGTHS + [8, 8], [5] * 30
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                assert hlit <= 286 and hdist <= 30
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = r.bits(3)
                ct, lens, header = decode_table(cl), [], []
                while len(lens) < hlit + hdist:
                    s = r.symbol(ct)
                    header.append(s)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        assert lens
                        lens += [lens[-1]] * (3 + r.bits(2))
                    else:
                        lens += [0] * (3 + r.bits(3) if s == 17 else 11 + r.bits(7))
                assert len(lens) == hlit + hdist, "a run goes past the last length"
                ll, dl = lens[:hlit], lens[hlit:]
                blk.update(ll=ll + [0] * (286 - hlit), dl=dl + [0] * (30 - hdist), cl=cl, hlit=hlit, hdist=hdist, hclen=hclen, header=header)
            lt, dt = decode_table(ll), decode_table(dl)
            while True:
                s = r.symbol(lt)
                if s < 256:
                    blk["symbols"].append(s)
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    length = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
                    ds = r.symbol(dt)
                    assert ds <= 29
                    blk["symbols"].append((length, DIST_BASE[ds] + r.bits(DIST_EXTRA[ds]), s, ds))
        out.append(blk)
        if final:
            return out, r.at


def kraft(lengths):
    """The Kraft sum as a fraction of 2^15."""
    return sum(1 << (15 - ln) for ln in lengths if ln)
