"""What a REGULAR tile of pileup text is, in plain Python, and a census of the device parser's paths over such a tile.

is_regular states the definition at the head of csrc/pileup_kernel.hip: a line is as many tokens as its batch has samples, each
followed by ONE space -- ".", "b,m,q,r,s" with one to three digits per field, or an indel token that starts with '+', '-' or 'N'
-- and the line's table entry ends behind its newline.  It does not look at the kernel's code.

census walks a regular tile the way the kernels partition it -- 16-byte lanes and 1 KiB steps from s & ~15 (pileup_parse_kernel),
4096 lines a scan step (pileup_scan_kernel), one patch thread per line in blocks of 256, 1024 positions a step of
called_scan_kernel, 65,536 workgroups of 4 lines a trip -- and names the class of every event.  region_census does the same for the
1 KiB segments of a compressed tile's regions (region_lines_kernel, region_scan_kernel).  The columns themselves come from
oracle/emit_oracle.py's Parser; this module only says which paths a tile takes, so that tests/test_pileup_lines.py can demand that
the catalogue (tests/pileup_lines.py) takes them all.
"""
import collections
import re

LANE, STEP, SCAN_STEP, PATCH_BLOCK, CALLED_STEP, TRIP_LINES, SEGMENT = 16, 1024, 4096, 256, 1024, 65536 * 4, 1024

TOKEN = rb"(?:\.|[0-9]{1,3}(?:,[0-9]{1,3}){4}|[+\-N][^ \n]*) "
_LINE = {}


def line_is_regular(line, n_tokens):
    """line: the bytes from the line's start to behind its newline."""
    rx = _LINE.get(n_tokens)
    if rx is None:
        rx = _LINE[n_tokens] = re.compile(rb"(?:" + TOKEN + rb"){%d}\n" % n_tokens)
    return rx.fullmatch(line) is not None


def is_regular(text, ls, n_in_batch):
    nb, T = ls.shape[0], ls.shape[1] - 1
    return all(int(ls[b, t + 1]) > int(ls[b, t]) and line_is_regular(text[int(ls[b, t]):int(ls[b, t + 1])], int(n_in_batch[b]))
               for b in range(nb) for t in range(T))


# ---------------------------------------------------------------------------------------------------------------- classes
BASE_LEN = ["base token of %d bytes at p %% 8 = %d" % (L, a) for L in range(10, 21) for a in range(8)]
FIELD_WIDTH = ["field %d of %d digits" % (f, w) for f in range(5) for w in (1, 2, 3)]
FIELD_WRAP = ["base value of 8 or more", "base value of 8 or more that is an N base", "N base token", "strand value of 2 or more",
              "token with 999 in four fields"] + \
             ["%s value of 256 or more" % k for k in ("mapq", "qual", "rpr")]
TOKEN_START = ["%s token starts at byte %d of a lane" % (k, i) for k in ("base", "dot", "indel") for i in range(16)]
STRADDLE = ["base token across a lane edge", "base token across a step edge", "base token last of its line",
            "base token last of its line and across a lane edge", "indel token across a step edge"]
STEP_EDGE = ["step edge on a separator", "step edge on a token's first byte", "step edge inside a base token", "step edge inside an indel token",
             "second step edge on a token's first byte", "second step edge inside a base token", "second step edge inside an indel token"]
DOT = ["dot: its space in the same lane", "dot at byte 15 of a lane (its space is the next lane's)", "dot at byte 15 of lane 63, the line going on",
       "dot at byte 15 whose space is the line's last byte", "dot at byte 15 of lane 63 whose space is the line's last byte", "dot last of its line"]
LINE_EDGE = ["line starts at %d mod 16" % i for i in range(16)] + ["line ends at %d mod 16" % i for i in range(16)] + \
            ["line of 0 bytes", "line of 2 bytes"] + ["line ends %d bytes behind s & ~15" % r for r in (1022, 1023, 1024, 1025, 1026, 2046, 2047, 2048, 2049, 2050)]
COUNTERS = ["step of 512 tokens, a step behind it", "step of 512 entries, a step behind it", "step of 103 base tokens, a step behind it"]
INDEL_LEN = ["indel token of 1 byte", "indel token of 15 bytes", "indel token of 16 bytes", "indel token of 17 bytes",
             "indel token over a whole step (a step without a token start)"] + ["indel token with '%s' inside" % c for c in "N+-"]
INDEL_SRC = ["indel entry from a base token of its lane (cur_last)", "indel entry from a base token of an earlier lane (left_last)",
             "indel entry from a base token of an earlier step (prev_tok)", "indel entry directly behind an N base token",
             "need: indel in a lane before the first base token's", "need: indel in the first base token's lane (ind_front)",
             "need: indel in a step before the first base token's", "need: line without a base token",
             "patch from an earlier batch's line of the same position", "patch from an earlier position", "patch from carry_in",
             "patch from a carry_in of zeros", "patch walks back 300 lines or more", "patch of 512 entries of one line"]
CARRY = ["carry_out is carry_in (no base token in the tile)", "a carry_in that is not zeros handed on by a tile without a base token",
         "a carry_in that is not zeros replaced by the tile's last base token", "a carry_in that is not zeros replaced by an N base token", "carry_out from the tile's last line", "carry_out from an earlier line"]
N_LINES = ["n_lines = %d of one-sample lines" % n for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097, 8191, 8193)] + ["n_lines_cap %% 4 = %d" % r for r in range(4)] + \
          ["n_lines + 1 = %d" % n for n in (256, 257, 513)] + ["scan: vector path", "scan: unaligned mode (scalar)", "scan: 2 steps", "scan: 3 steps",
                                                              "scan: a step's last thread group is partial", "parse: second trip of the line loop"]
N_POS = ["n_pos = %d" % n for n in (1023, 1024, 1025, 2049)] + ["called scan: %d steps" % n for n in (1, 2, 3)]
BATCHES = ["batches: %d" % n for n in (1, 3, 5, 7)]
CLASSES = BASE_LEN + FIELD_WIDTH + FIELD_WRAP + TOKEN_START + STRADDLE + STEP_EDGE + DOT + LINE_EDGE + COUNTERS + INDEL_LEN + INDEL_SRC + CARRY + \
    N_LINES + N_POS + BATCHES
assert len(set(CLASSES)) == len(CLASSES)


def _line_census(text, s, e, c):
    """One line [s, e) (text[e] is its newline).  Returns (indel entries in front of the first base token, last base token or None)."""
    off0 = s & ~(LANE - 1)
    c["line starts at %d mod 16" % (s % LANE)] += 1
    c["line ends at %d mod 16" % (e % LANE)] += 1
    if e - s in (0, 2):
        c["line of %d bytes" % (e - s)] += 1
    c["line ends %d bytes behind s & ~15" % (e - off0)] += 1
    toks, p = [], s
    while p < e:
        q = text.index(b" ", p)
        toks.append((p, q))
        p = q + 1
    starts = {p for p, _ in toks}
    per_step = collections.defaultdict(lambda: [0, 0, 0])            # tokens, entries, base tokens that start in the step
    last_base, first_base, need, prev_kind, last_tok = None, None, [], None, None
    for p, q in toks:
        step, lane, i = (p - off0) // STEP, (p - off0) % STEP // LANE, p % LANE
        ch = text[p:p + 1]
        n = per_step[step]
        n[0] += 1
        if ch == b".":
            c["dot token starts at byte %d of a lane" % i] += 1
            if q == e - 1:
                c["dot last of its line"] += 1
            if i < 15:
                c["dot: its space in the same lane"] += 1
            elif q == e - 1:
                c["dot at byte 15 of lane 63 whose space is the line's last byte" if lane == 63 else "dot at byte 15 whose space is the line's last byte"] += 1
            elif lane == 63:
                c["dot at byte 15 of lane 63, the line going on"] += 1
            else:
                c["dot at byte 15 of a lane (its space is the next lane's)"] += 1
            prev_kind = "dot"
        elif ch in b"+-N":
            n[1] += 1
            c["indel token starts at byte %d of a lane" % i] += 1
            ln = q - p
            if ln in (1, 15, 16, 17):
                c["indel token of %d byte%s" % (ln, "" if ln == 1 else "s")] += 1
            for x in "N+-":
                if x.encode() in text[p + 1:q]:
                    c["indel token with '%s' inside" % x] += 1
            if (q - off0) // STEP != step:
                c["indel token across a step edge"] += 1
            if (q - off0) // STEP > step + 1 and not any(off0 + (step + 1) * STEP <= x < off0 + (step + 2) * STEP for x in starts):
                c["indel token over a whole step (a step without a token start)"] += 1
            if prev_kind == "nbase":
                c["indel entry directly behind an N base token"] += 1
            if last_base is None:
                need.append(p)
            else:
                bstep, blane = (last_base - off0) // STEP, (last_base - off0) % STEP // LANE
                c["indel entry from a base token of its lane (cur_last)" if (bstep, blane) == (step, lane) else
                  "indel entry from a base token of an earlier lane (left_last)" if bstep == step else
                  "indel entry from a base token of an earlier step (prev_tok)"] += 1
            prev_kind = "indel"
        else:
            c["base token starts at byte %d of a lane" % i] += 1
            c["base token of %d bytes at p %% 8 = %d" % (q - p + 1, p % 8)] += 1
            f = text[p:q].split(b",")
            for k, v in enumerate(f):
                c["field %d of %d digits" % (k, len(v))] += 1
            v = [int(x) for x in f]
            if v[0] >= 8:
                c["base value of 8 or more"] += 1
                if v[0] & 7 == 4:
                    c["base value of 8 or more that is an N base"] += 1
            if v.count(999) == 4:
                c["token with 999 in four fields"] += 1
            if v[4] >= 2:
                c["strand value of 2 or more"] += 1
            for k, name in ((1, "mapq"), (2, "qual"), (3, "rpr")):
                if v[k] >= 256:
                    c["%s value of 256 or more" % name] += 1
            across_lane = p // LANE != q // LANE
            if across_lane:
                c["base token across a lane edge"] += 1
            if (q - off0) // STEP != step:
                c["base token across a step edge"] += 1
            if q == e - 1:
                c["base token last of its line"] += 1
                if across_lane:
                    c["base token last of its line and across a lane edge"] += 1
            n[2] += 1
            if v[0] & 7 == 4:
                c["N base token"] += 1
                prev_kind = "nbase"
            else:
                n[1] += 1
                prev_kind = "base"
            if first_base is None:
                first_base = p
            last_base = p
            last_tok = (v[0] & 7, v[1] & 255, v[2] & 255, v[3] & 255, v[4] & 1)
    for p in need:
        if first_base is None:
            c["need: line without a base token"] += 1
        elif (p - off0) // STEP != (first_base - off0) // STEP:
            c["need: indel in a step before the first base token's"] += 1
        elif (p - off0) // LANE != (first_base - off0) // LANE:
            c["need: indel in a lane before the first base token's"] += 1
        else:
            c["need: indel in the first base token's lane (ind_front)"] += 1
    for k in range(1, (e - 1 - off0) // STEP + 1 if e > s else 0):   # the step edges inside the line
        edge = off0 + k * STEP
        if edge <= s:
            continue
        which = "step edge" if k == 1 else "second step edge" if k == 2 else "later step edge"
        if text[edge:edge + 1] == b" ":
            c[which + " on a separator"] += 1
        elif edge in starts:
            c[which + " on a token's first byte"] += 1
        else:
            owner = max(x for x in starts if x < edge)
            c[which + (" inside an indel token" if text[owner:owner + 1] in b"+-N" else " inside a base token")] += 1
    last_step = max(per_step) if per_step else 0
    for step, (n_tok, n_ent, n_base) in per_step.items():
        if step < last_step:
            if n_tok == 512:
                c["step of 512 tokens, a step behind it"] += 1
            if n_ent == 512:
                c["step of 512 entries, a step behind it"] += 1
            if n_base == 103:
                c["step of 103 base tokens, a step behind it"] += 1
    return len(need), last_tok


def census(text, ls, n_in_batch, carry_in=(0, 0, 0, 0, 0)):
    """Counter of the classes a regular tile reaches; also returns the carry the tile leaves."""
    c = collections.Counter()
    nb, T = ls.shape[0], ls.shape[1] - 1
    n_lines = nb * T
    lasts = []                                                       # position-major: the order the reference parses in
    for t in range(T):
        for b in range(nb):
            need, last = _line_census(text, int(ls[b, t]), int(ls[b, t + 1]) - 1, c)
            if need:
                back = next((k for k in range(len(lasts) - 1, -1, -1) if lasts[k] is not None), None)
                if back is None:
                    c["patch from a carry_in of zeros" if tuple(carry_in) == (0, 0, 0, 0, 0) else "patch from carry_in"] += 1
                else:
                    c["patch from an earlier batch's line of the same position" if back // nb == t else "patch from an earlier position"] += 1
                    if len(lasts) - back >= 300:
                        c["patch walks back 300 lines or more"] += 1
                if need == 512:
                    c["patch of 512 entries of one line"] += 1
            lasts.append(last)
    back = next((k for k in range(n_lines - 1, -1, -1) if lasts[k] is not None), None)
    carry_out = tuple(carry_in) if back is None else lasts[back]
    if n_lines:
        c["carry_out is carry_in (no base token in the tile)" if back is None else
          "carry_out from the tile's last line" if back == n_lines - 1 else "carry_out from an earlier line"] += 1
    if n_lines and tuple(carry_in) != (0, 0, 0, 0, 0):
        c["a carry_in that is not zeros handed on by a tile without a base token" if back is None else
          "a carry_in that is not zeros replaced by an N base token" if carry_out[0] == 4 else
          "a carry_in that is not zeros replaced by the tile's last base token"] += 1
    c.update(counts_census(nb, T, n_lines, all(int(n) == 1 for n in n_in_batch)))
    return c, carry_out


def counts_census(nb, T, n_lines_cap, one_sample=False):
    """The classes of the kernels that walk lines and positions, not text: n_lines_cap is the room of the per-line arrays (nb x T for a
    text tile, nb x max_positions for a compressed one)."""
    c = collections.Counter()
    n_lines = nb * T
    if one_sample:
        c["n_lines = %d of one-sample lines" % n_lines] += 1
    c["n_lines + 1 = %d" % (n_lines + 1)] += 1
    c["batches: %d" % nb] += 1
    if n_lines:
        c["n_lines_cap %% 4 = %d" % (n_lines_cap % 4)] += 1
        vec = n_lines_cap % 4 == 0
        if vec and n_lines >= 4:
            c["scan: vector path"] += 1
        if not vec:
            c["scan: unaligned mode (scalar)"] += 1
        if n_lines % 4:
            c["scan: a step's last thread group is partial"] += 1
        steps = -(-n_lines // SCAN_STEP)
        if steps in (2, 3):
            c["scan: %d steps" % steps] += 1
        if n_lines > TRIP_LINES:
            c["parse: second trip of the line loop"] += 1
    if T:
        c["n_pos = %d" % T] += 1
        c["called scan: %d steps" % -(-T // CALLED_STEP)] += 1
    return c


# ------------------------------------------------------------------------------------------------- compressed tiles' regions
REGION_CLASSES = ["region starts at %d mod 16" % i for i in range(16)] + \
    ["newline at byte %d of a region" % i for i in (1023, 1024, 1025)] + \
    ["newline on a segment's first byte", "newline on a segment's last byte", "region of more than 64 segments", "region of no bytes",
     "batch without a new block", "partial line of more than 1 KiB left over", "block ends inside a token", "block ends on a newline",
     "max_pos = whole lines - 1", "max_pos = whole lines", "max_pos = whole lines + 1", "T cut by max_pos inside a segment that holds more lines",
     "scan: vector path with a partial last thread group"]


def region_census(streams, skip, calls):
    """What bvc_pileup_begin_bgzf's regions look like call by call: a batch's region = what the tile before left of it + its new
    blocks (minus the header line of the first), from a 16-byte boundary + the bytes skipped.  Returns (Counter, [T per call])."""
    c = collections.Counter()
    nb = len(streams)
    sent, left, first, Ts = [0] * nb, [b""] * nb, True, []
    for pieces, max_pos in calls:
        regions = []
        for b in range(nb):
            fresh = b""
            if not pieces[b]:
                c["batch without a new block"] += 1
            for n in pieces[b]:
                fresh += streams[b][sent[b]:sent[b] + n]
                sent[b] += n
                if sent[b] < len(streams[b]):
                    c["block ends on a newline" if streams[b][sent[b] - 1:sent[b]] == b"\n" else "block ends inside a token"] += 1
            k = skip[b] if first and not left[b] else 0
            regions.append((k % 16, left[b] + fresh[k:]))
        whole = [r.count(b"\n") for _, r in regions]
        T = min(min(whole), max_pos)
        for d, name in ((-1, "max_pos = whole lines - 1"), (0, "max_pos = whole lines"), (1, "max_pos = whole lines + 1")):
            if max_pos == min(whole) + d:
                c[name] += 1
        for b, (a, r) in enumerate(regions):
            c["region starts at %d mod 16" % a] += 1
            if not r:
                c["region of no bytes"] += 1
            if -(-len(r) // SEGMENT) > 64:
                c["region of more than 64 segments"] += 1
            nl = [i for i, x in enumerate(r) if x == 10]
            for i in nl:
                if i in (1023, 1024, 1025):
                    c["newline at byte %d of a region" % i] += 1
                if i % SEGMENT == 0:
                    c["newline on a segment's first byte"] += 1
                if i % SEGMENT == SEGMENT - 1:
                    c["newline on a segment's last byte"] += 1
            if T < len(nl) and T > 0 and nl[T - 1] // SEGMENT == nl[T] // SEGMENT:
                c["T cut by max_pos inside a segment that holds more lines"] += 1
            end = nl[T - 1] + 1 if T else 0
            left[b] = r[end:]
            if len(left[b]) - (left[b].rfind(b"\n") + 1) > 1024:
                c["partial line of more than 1 KiB left over"] += 1
        if (nb * max_pos) % 4 == 0 and (nb * T) % 4:
            c["scan: vector path with a partial last thread group"] += 1
        Ts.append(T)
        first = False
    return c, Ts
