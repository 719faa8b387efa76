"""CPU tests of the hand-built pileup text (tests/pileup_lines.py): the catalogue is what it claims to be, and it leaves no path out.

The seeded random lines of tests/test_gpu_round5.py reach the edges of pileup_parse_kernel and the kernels around it only by
chance, and some never (a base token of 18..20 bytes, 512 tokens in a step, a line count that is no multiple of 4 ...).  Here:
(1) every regular case is regular by the plain statement of the format (tests/pileup_model.py), every irregular one is not, and
its twin is; (2) the restated parser's columns for the regular cases equal a strict split written below; (3) the census: the regular
cases reach every path class the model defines, and every case is needed for that, which is what keeps
tests/test_gpu_pileup_lines.py from passing without having met an edge; (4) host/pileup.cpp's text parser gives the same columns.
"""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pileup_lines as S
from tests import pileup_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return S.regular() + [S.large()]


@pytest.fixture(scope="module")
def censuses(cases):
    out = {}
    for c in cases:
        text, ls = S.layout(c.batch_lines, c.align)
        out[c.name] = M.census(text, ls, c.n_in_batch, c.carry_in)
    return out


def test_census_constants_are_the_kernels():
    """The sizes the census partitions a tile by, against the text of csrc/pileup_kernel.hip."""
    text = open(os.path.join(ROOT, "basevarc_amd", "csrc", "pileup_kernel.hip"), encoding="utf-8").read()
    assert "for (uint32_t off = s & ~15u; off < e; off += 16u * kWave)" in text and M.STEP == 16 * 64 and M.LANE == 16
    assert "for (int64_t base = 0; base < n_lines; base += %d)" % M.SCAN_STEP in text
    assert "for (int64_t t0 = 0; t0 < n_pos; t0 += %d)" % M.CALLED_STEP in text
    assert "constexpr int kSegBytes = %d;" % M.SEGMENT in text and "constexpr int kParseWaves = 4;" in text
    assert len(re.findall(r"blocks < 65536 \? blocks : 65536", text)) == 2 and M.TRIP_LINES == 65536 * 4
    assert "dim3((unsigned)((threads + 255) / 256)), dim3(%d)" % M.PATCH_BLOCK in text


def test_regular_cases_are_regular_and_irregular_ones_are_not(cases):
    for c in cases:
        text, ls = S.layout(c.batch_lines, c.align)
        assert c.regular and M.is_regular(text, ls, c.n_in_batch), c.name
    pairs = S.irregular()
    assert len(pairs) > 120 and len({bad.name for bad, _ in pairs}) == len(pairs)
    for bad, twin in pairs:
        assert not bad.regular and not M.is_regular(*S.layout(bad.batch_lines, bad.align), bad.n_in_batch), bad.name
        assert twin.regular and M.is_regular(*S.layout(twin.batch_lines, twin.align), twin.n_in_batch), twin.name
        assert bad.align == twin.align and bad.n_in_batch.tolist() == twin.n_in_batch.tolist()
    # a substituted byte is ONE byte, and it lies where its name says (bytes behind s & ~15)
    places = dict(S.PLACES)
    for bad, twin in pairs:
        a, b = bad.batch_lines[0][0], twin.batch_lines[0][0]
        place = next((p for p in places if bad.name.endswith("_" + p)), None)
        if place is None:
            continue
        at = S._first_difference(b, a)
        assert at + bad.align[0] == places[place], bad.name
        if bad.name.startswith("sub_"):
            assert len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1, bad.name
    for f in S.feeds():
        for b, lines in enumerate(f.batch_lines):
            assert all(M.line_is_regular(l.encode() + b"\n", int(f.n_in_batch[b])) for l in lines), (f.name, b)


def strict_columns(c):
    """The columns of a regular tile by a strict split: every line is its tokens, each with one space behind it; nothing is skipped,
    nothing is guessed.  [(entries, samples)] per position, an entry = (base, mapq, qual, rpr, strand, is_indel, indel text)."""
    ai = list(c.carry_in)
    sample0 = S.sample0_of(c.n_in_batch)
    cols = []
    for t in range(len(c.batch_lines[0])):
        ent, smp = [], []
        for b, lines in enumerate(c.batch_lines):
            line = lines[t]
            assert line == "" or line[-1] == " "
            toks = line[:-1].split(" ") if line else []
            assert len(toks) == c.n_in_batch[b], (c.name, b, t)
            for k, tok in enumerate(toks):
                if tok == ".":
                    continue
                if tok[0] in "+-N":
                    ent.append((ai[0], ai[1], ai[2], ai[3], ai[4], 1, tok))
                    smp.append(int(sample0[b]) + k)
                    continue
                f = tok.split(",")
                assert len(f) == 5 and all(1 <= len(x) <= 3 and x.isdigit() for x in f), tok
                v = [int(x) for x in f]
                ai = [v[0] & 7, v[1] & 255, v[2] & 255, v[3] & 255, v[4] & 1]
                if ai[0] != 4:
                    ent.append((ai[0], ai[1], ai[2], ai[3], ai[4], 0, ""))
                    smp.append(int(sample0[b]) + k)
        cols.append((ent, smp))
    return cols, ai


def parser_columns(c):
    p = S.parser_for(c)
    nb, T = len(c.batch_lines), len(c.batch_lines[0])
    cols = []
    for t in range(T):
        aiv, sample = p.parse([c.batch_lines[b][t] for b in range(nb)])
        cols.append(([(a["base"], a["mapq"], a["qual"], a["rpr"], a["strand"], a["is_indel"], a["indel"] if a["is_indel"] else "") for a in aiv], sample))
    return cols, [p.ai[k] for k in ("base", "mapq", "qual", "rpr", "strand")]


def test_restated_parser_equals_a_strict_split(cases, censuses):
    """oracle/emit_oracle.py's Parser -- the expectation of every GPU test of the text parser -- against the strict split, the carry the
    model predicts, and for the large case the vectorised expectation tests/test_gpu_pileup_lines.py compares with."""
    for c in cases:
        want, ai = strict_columns(c)
        got, ai2 = parser_columns(c)
        assert got == want and ai == ai2, c.name
        assert list(censuses[c.name][1]) == ai, c.name
    chain = {c.name: c for c in cases}
    assert list(censuses["chain_a"][1]) == chain["chain_b"].carry_in and list(censuses["chain_b"][1]) == chain["chain_c"].carry_in
    c = S.large()
    want, ai = strict_columns(c)
    x = S.large_expected()
    assert x["carry_out"] == ai
    rows = [e[:6] for ent, _ in want for e in ent]
    assert np.array_equal(np.array(rows), np.stack([x[k] for k in ("base", "mapq", "qual", "rpr", "strand", "is_indel")], axis=1))
    assert x["samples"].tolist() == [j for _, smp in want for j in smp]
    assert x["entry_off"].tolist() == np.concatenate([[0], np.cumsum([len(ent) for ent, _ in want])]).tolist()
    assert all(e[6] == "N" for ent, _ in want for e in ent if e[5])


def test_census_every_path_class_is_reached(censuses):
    """Every class of tests/pileup_model.py is reached by a regular case, a class left empty fails by name; and no case is there for
    nothing: without any one of them some class is empty.  A condition, not a measurement."""
    total = collections.Counter()
    for c, _ in censuses.values():
        total.update(c)
    empty = [k for k in M.CLASSES if total[k] == 0]
    assert not empty, empty
    idle = [name for name, (c, _) in censuses.items() if not [k for k in M.CLASSES if (total - c)[k] == 0]]
    assert not idle, "cases that reach no class of their own: %s" % idle
    print("\n".join("%8d  %s" % (total[k], k) for k in M.CLASSES))


def test_region_census_every_class_is_reached():
    """The same for the compressed tiles: the feeds of tests/pileup_lines.py reach every class of a region's 1 KiB segments."""
    total = collections.Counter()
    for f in S.feeds():
        c, Ts = M.region_census(S.feed_streams(f), f.skip, f.calls)
        assert sum(Ts) == len(f.batch_lines[0]), (f.name, Ts)
        total.update(c)
    empty = [k for k in M.REGION_CLASSES if total[k] == 0]
    assert not empty, empty
    print("\n".join("%8d  %s" % (total[k], k) for k in M.REGION_CLASSES))


@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    _, lib = b.build_host()
    L = C.CDLL(lib)
    L.bvchost_reset_parser.restype = None
    L.bvchost_site_parse.restype = C.c_void_p; L.bvchost_site_parse.argtypes = [C.c_char_p, C.c_int32]
    L.bvchost_site_free.restype = None; L.bvchost_site_free.argtypes = [C.c_void_p]
    L.bvchost_site_size.restype = C.c_int32; L.bvchost_site_size.argtypes = [C.c_void_p]
    L.bvchost_site_field.restype = C.c_int32; L.bvchost_site_field.argtypes = [C.c_void_p, C.c_int32, C.c_int]
    return L


def test_host_text_parser_on_the_catalogue(H, cases):
    """host/pileup.cpp's parse_pileup_line (what the host program parses a reported tile with) on every regular case: the fields and
    the sample of every entry.  Its long-lived state is set to a case's carry by parsing one base token with those fields.  The large
    case: its first 3000 positions."""
    for c in cases:
        want, _ = strict_columns(c._replace(batch_lines=[l[:3000] for l in c.batch_lines]))
        H.bvchost_reset_parser()
        s = H.bvchost_site_parse(("%d,%d,%d,%d,%d \n" % tuple(c.carry_in)).encode(), 0)
        assert H.bvchost_site_size(s) == (0 if c.carry_in[0] == 4 else 1)
        H.bvchost_site_free(s)
        for t, (ent, smp) in enumerate(want):
            # a batch of no samples has empty lines: the host takes a position's lines batch by batch and counts samples by tokens
            lines = b"".join(c.batch_lines[b][t].encode() + b"\n" for b in range(len(c.batch_lines)) if c.n_in_batch[b])
            s = H.bvchost_site_parse(lines, t)
            assert H.bvchost_site_size(s) == len(ent), (c.name, t)
            got = [[H.bvchost_site_field(s, k, f) for f in range(7)] for k in range(len(ent))]
            H.bvchost_site_free(s)
            assert got == [list(e[:6]) + [j] for e, j in zip(ent, smp)], (c.name, t)
