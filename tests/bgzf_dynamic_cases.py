"""The hand-built pieces that the dynamic Huffman code of the device deflate encoder is walked over, beside the catalogue of
tests/bgzf_deflate_cases.py (tests/test_gpu_bgzf_dynamic.py), and the families of symbol counts the code-length builder is held to
(tests/test_bgzf_dynamic_abi.py, bvc_bgzf_code_lengths on the device).  Every piece is the same on every call.  Nothing here needs a device."""
import math

import numpy as np

from tests import bgzf_blocks as bb
from tests import bgzf_deflate_cases as dc

B = dc.B


def perms(m, ks):
    """The values 0 .. m - 1 in the orders k * i mod m, one after the other: every value as often as any other, and -- the steps differ --
    no four bytes twice (has_no_match_of_four checks it), so the encoder writes literals only."""
    assert all(math.gcd(k, m) == 1 for k in ks)
    return b"".join(bytes((k * i) % m for i in range(m)) for k in ks)


def has_no_match_of_four(text):
    seen = set()
    for i in range(len(text) - 3):
        if text[i:i + 4] in seen:
            return False
        seen.add(text[i:i + 4])
    return True


KS_144 = (1, 5, 7, 11, 13, 17, 19, 23, 25, 29, 31, 35)
KS_256 = (3, 9, 15)                                              # (none of KS_144: a step below 144 walks the same values at first)


def every_symbol_piece():
    """One block in which a copy of every length symbol from 258 on (a match is used from 4 bytes on, so 257 is never written) and of every
    distance symbol lies where the encoder finds it, between random bytes below 144: the constructions of the "distance" and "match
    length" cases of tests/bgzf_deflate_cases.py, one after the other in one piece.  Distances up to 1025: the source of d bytes, then
    its first 40 bytes again.  Beyond: nine sources of 40 bytes 50 bytes apart, source i copied d_i bytes behind itself."""
    rng = np.random.default_rng(20261020)

    def rand8(n):
        return rng.integers(0, 144, n, dtype=np.uint8).tobytes()
    out = bytearray(rand8(255))
    # (a source whose first position has left the hash table is found one byte late: a length symbol with extra bits is aimed at one above
    # its base, one without is given three copies)
    for n, extra in zip(dc.LEN_BASE[1:], bb.LEN_EXTRA[1:]):
        for _ in range(1 if extra else 3):
            m = n + 1 if extra else n
            src = rand8(m + 1)
            out += src + src[:m] + bytes([src[m] ^ 1]) + b"!"
    near = [d for d in dc.DIST_BASE if d <= 1025]
    for d in near:
        r = rand8(d)
        out += r + (r * 40)[:40] + b"\x00\x8f"
    far = [d for d in dc.DIST_BASE if d > 1025]
    base = len(out)
    out += rand8(B - len(out))
    for i, d in enumerate(far):
        a = base + 50 * i
        out[a + d:a + d + 40] = out[a:a + 40]
    assert len(out) == B and base + 50 * len(far) + 40 < base + far[0]
    return bytes(out)


def catalogue():
    """[(name, bytes, the form its first block must take with "bgzf_codes" at 1: "stored", "fixed", "dynamic", or None where it is left
    to the comparison with the model)]."""
    rng = np.random.default_rng(20261021)
    out = []
    # 7.64 bits a byte in a code of 200 equal symbols; 8 bits (below 144) or 9 in the fixed code: 8.28 on average, more than stored
    out.append(("65280 random bytes over 200 values", rng.integers(0, 200, B, dtype=np.uint8).tobytes(), "dynamic"))
    # too short for a match of 4: no distance is used, and a header costs more than it saves
    out.append(("one distinct byte, 3 literals", b"aaa", "fixed"))
    out.append(("two distinct bytes, 5 literals", b"ababb", "fixed"))
    out.append(("three distinct bytes, 7 literals", b"abccbba", "fixed"))
    # literals only and every one as frequent as any other.  144 values: 7.17 bits each against 8, 1728 of them: 170 bytes saved by a header
    # of well under 100.  256 values: the first 144 are six times as frequent as the rest
    lo = perms(144, KS_144)
    both = perms(144, KS_144[:10]) + perms(256, KS_256)
    assert has_no_match_of_four(lo) and has_no_match_of_four(both)
    out.append(("literals 0..143 only", lo, "dynamic"))
    out.append(("literals 0..255 only", both, "dynamic"))
    # the same with one copy of 30 bytes 900 bytes behind its source: one match, one distance
    one = lo[:1000] + lo[100:130] + lo[1000:]
    assert lo[130] != lo[1000] and lo[99] != lo[999]
    out.append(("one match among literals", one, "dynamic"))
    out.append(("every length and distance symbol in one block", every_symbol_piece(), "dynamic"))
    # sixteen values, each half as frequent as the one before, in random order: two bits a byte; the rarest get the longest codes there are
    out.append(("30000 bytes of halving frequencies", np.minimum(rng.geometric(0.5, 30000) - 1, 15).astype(np.uint8).tobytes(), "dynamic"))
    return out


# ---- families of counts for the code-length builder: (name, counts, limit)
def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def count_families():
    out = [("fibonacci 20, limit 15", fibonacci(20), 15), ("fibonacci 10, limit 7", fibonacci(10), 7),
           ("powers of two, 15 symbols", [1 << k for k in range(15)], 15), ("powers of two, 20 symbols", [1 << k for k in range(20)], 15),
           ("powers of two, 7 symbols, limit 7", [1 << k for k in range(7)], 7)]
    for n in (2, 3, 19, 30, 286, 288):
        out.append((f"all equal, {n} symbols", [5] * n, 15))
    out.append(("all equal, 19 symbols, limit 7", [3] * 19, 7))
    out.append(("no used symbol, 30", [0] * 30, 15))
    out.append(("no used symbol, 1", [0], 15))
    for n, s in ((30, 0), (30, 1), (30, 17), (286, 256), (1, 0), (2, 1)):
        c = [0] * n
        c[s] = 9
        out.append((f"one used symbol {s} of {n}", c, 15))
    out.append(("two used symbols far apart", [0] * 100 + [7] + [0] * 150 + [1], 15))
    return out
