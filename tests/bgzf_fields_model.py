"""A plain Python model of the field parse of the device deflate encoder (tuning key "bgzf_parse" = 1; docs/BGZF_FIELDS.md holds the rule,
the device's copy is csrc/bgzf_fields_device.h).  symbols() takes a block's bytes (at most 65280) and gives its symbols -- an int per
literal, a (length, distance) tuple per match -- in the form tests/bgzf_dynamic_model.encode takes; parse() also gives the cuts, the heads
and the match of every position, and candidates() the candidate set of every keyed head exactly as the kernel's tables hold it.
Nothing here needs a device."""
B = 65280
ROUND, WAYS, HASH_BITS = 256, 16, 11
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
MIN_KEYED, MAX_KEYED = 4, 32
DELIMITERS = (0x09, 0x3A)


def fields_of(x):
    """[(start, length)] of the fields of x: a cut at 0 and behind every tab and colon."""
    cuts = [0] + [p + 1 for p in range(len(x) - 1) if x[p] in DELIMITERS] if len(x) else []
    return [(c, (cuts[i + 1] if i + 1 < len(cuts) else len(x)) - c) for i, c in enumerate(cuts)]


def key_of(x, p, length):
    """The key of the field of `length` bytes at p: 11 bits of a hash of its length and bytes, four bytes at a time."""
    h = length
    for i in range(0, length, 4):
        w = int.from_bytes(x[p + i:p + min(i + 4, length)], "little")
        h = ((h ^ w) * 2654435761) & 0xFFFFFFFF
        h ^= h >> 15
    return h >> (32 - HASH_BITS)


def common_prefix(x, q, p, limit):
    """The number of bytes, up to limit, that x[q ..] and x[p ..] share."""
    a, b = x[q:q + limit], x[p:p + limit]
    if a == b:
        return limit
    lo, hi = 0, limit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def candidates(x, heads):
    """{p: sorted candidate positions} for every head p with 4 <= length <= 32 (heads: {start: length}).  The set the kernel's tables
    give: for each of the 16 ways w the LARGEST keyed head q with p's key whose round (q // 256) is below p's and = w (mod 16), and the
    FIRST keyed head with the key in p's own round, if it lies in front of p."""
    ways = [dict() for _ in range(WAYS)]                         # way -> {key: position}
    out, current, first, pending = {}, 0, {}, []
    for p in sorted(heads):
        length = heads[p]
        if not MIN_KEYED <= length <= MAX_KEYED:
            continue
        r = p // ROUND
        if r != current:                                           # the rounds before this one into their ways
            for q, k in pending:
                w = ways[(q // ROUND) % WAYS]
                w[k] = max(w.get(k, -1), q)
            current, first, pending = r, {}, []
        k = key_of(x, p, length)
        c = {w[k] for w in ways if k in w}
        if k in first:
            c.add(first[k])
        out[p] = sorted(c)
        first.setdefault(k, p)
        pending.append((p, k))
    return out


def parse(x):
    """dict: fields [(start, length)], heads {start: length}, match {position: (length, distance)}."""
    x = bytes(x)
    n = len(x)
    assert n <= B
    fields = fields_of(x)
    heads = {}
    for i, (p, length) in enumerate(fields):
        repeat = i > 0 and fields[i - 1][1] == length and x[p - length:p] == x[p:p + length]
        if not repeat:
            heads[p] = length
    is_cut = bytearray(n + 1)
    for p, _ in fields:
        is_cut[p] = 1
    if n:
        is_cut[n] = 1                                              # a match may end at the block's end
    cand = candidates(x, heads)
    match = {}
    # the start of the next head behind each field, or n
    next_head, e = {}, n
    for p, length in reversed(fields):
        next_head[p] = e
        if p in heads:
            e = p
    for p, length in fields:
        if p not in heads:
            m = min(next_head[p] - p, MAX_MATCH) // length * length
            if m >= MIN_MATCH:
                match[p] = (m, length)
            continue
        best = None
        for q in cand.get(p, ()):
            d = p - q
            if d > MAX_DIST:
                continue
            m = common_prefix(x, q, p, min(MAX_MATCH, n - p))
            if m < length:
                continue
            end = p + m
            while not is_cut[end]:
                end -= 1
            m = end - p
            if best is None or m > best[0] or (m == best[0] and d < best[1]):
                best = (m, d)
        if best is not None and best[0] >= MIN_MATCH:
            match[p] = best
    return dict(fields=fields, heads=heads, match=match, candidates=cand)


def symbols(x, parsed=None):
    """The greedy walk: the match of the position where it stands, else a literal."""
    x = bytes(x)
    match = (parsed or parse(x))["match"]
    out, p = [], 0
    while p < len(x):
        if p in match:
            out.append(match[p])
            p += match[p][0]
        else:
            out.append(x[p])
            p += 1
    return out


def blocks_of(piece):
    return [piece[at:at + B] for at in range(0, len(piece), B)]
