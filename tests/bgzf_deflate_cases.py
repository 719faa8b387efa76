"""The hand-built catalogue of byte ranges the device deflate encoder is walked over (tests/test_gpu_bgzf_deflate.py): the smallest inputs
at which an encoder can go wrong, and the three sample-column texts its output size is judged on.  Nothing here needs a device."""
import functools
import os
import re
import sys
import zlib

import numpy as np

from tests import vcf_samples_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 65280                                                          # input bytes of a block (include/bvc.h)
GRID = 256                                                         # workgroups of bgzf_block_kernel (csrc/bvc_internal.h, kBgzfDeflateGrid)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)


def periodic(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n]


def catalogue():
    """[(name, bytes)], the same on every call but for the two os.urandom cases."""
    rng = np.random.default_rng(20261019)

    def rand(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = [(f"length {n}", b"abcde"[:n]) for n in range(6)]
    # runs: the tail behind a longest match is too short to be a match
    for n in sorted(set(range(257, 263)) | {258 * k + j for k in (2, 3, 7) for j in range(4)}):
        out.append((f"run of one byte, {n}", b"\t" * n))
        out.append((f"run of ./.<tab>, {n}", periodic(b"./.\t", n)))
    # periodic across the cut between a piece's blocks: a second block must not reach into the first
    field = b"0/.:A:+:0.999369\t"
    for n in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
        out.append((f"period 4 across the cut, {n}", periodic(b"./.\t", n)))
        out.append((f"period 17 across the cut, {n}", periodic(field, n)))
    # A copy at a chosen distance and of a chosen length, where the encoder is bound to find it: the source starts at position 255, the
    # LAST of the first round of 256 positions, so it is the position its hash keeps in the table's first way until round 16 writes that way
    # again (copies up to 4096 bytes behind it; further back the source's 40 positions have to survive later rounds with their hash, and
    # it is enough that one does).  Bytes below 144 cost eight bits as literals, so that the copy decides coded against stored.
    def rand8(n):
        return rng.integers(0, 144, n, dtype=np.uint8).tobytes()
    # every distance on either side of each distance-code boundary: the source, then its first 40 bytes (its period repeated where it is shorter)
    for d in sorted({x for b in DIST_BASE[1:] for x in (b - 1, b)} | {32768, 32769}):
        r = rand8(d)
        out.append((f"distance {d}", rand8(255) + r + (r * 40)[:40] + b"\x00\x8f"))
    # every length on either side of each length-code boundary: the copy ended by a byte that differs
    for n in sorted({x for b in LEN_BASE for x in (b - 1, b)} | {259, 260, 2 * 258, 2 * 258 + 3} - {2}):
        src = rand8(n + 1)
        out.append((f"match length {n}", rand8(255) + src + src[:n] + bytes([src[n] ^ 1]) + b"!"))
    # (256 literals alone are smaller stored: a run behind them keeps the block coded, so that both literal code lengths are written)
    out.append(("all 256 byte values", bytes(range(256)) + b"\t" * 600))
    out.append(("all 256 byte values in three orders", bytes(range(256)) + bytes(range(255, -1, -1)) + bytes((37 * i) & 255 for i in range(256))
                + periodic(b"./.\t", 3000)))
    out.append(("65280 random bytes", os.urandom(B)))
    out.append(("65280 random letters of four", bytes(b"ACGT"[x & 3] for x in os.urandom(B))))
    return out


def stream_pieces():
    """More blocks in one call than the launch has workgroups twice over, many one-byte pieces among long ones."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(2 * GRID + 3):
        n = 1 if i % 3 else int(rng.integers(2, 400))
        out.append(periodic(b"./.\t0/.:C:-:0.9%d\t" % (i % 10), n) if i % 5 else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    out[7] = periodic(b"./.\t./.\t0/.:A:+:0.999000\t", 2 * B + 17)
    out[300] = b""
    out[301] = b""
    return out


def sample_text(n, coverage, seed):
    """The sample columns of one called site from tests/vcf_samples_cases.py's model: n samples, one alt at 5 %, qualities 10..40."""
    rng = np.random.default_rng(seed)
    s = np.flatnonzero(rng.random(n) < coverage).astype(np.int32)
    e = vc.make_entries(len(s), base=np.where(rng.random(len(s)) < 0.05, 1, 0), qual=rng.integers(10, 41, len(s)), strand=rng.integers(0, 2, len(s)))
    return vc.model_columns(n, s, e, 0, 1, (1, -1, -1))


SIZE_TEXTS = ((0.10, 101, 1.0), (0.01, 102, 1.0), (1.0, 103, 1.10))      # (coverage, seed, bound on device / zlib level 1)


def zlib_size(data, level):
    """zlib on the same bytes cut at the same 65280-byte marks, 26 bytes of block overhead added to each."""
    total = 0
    for at in range(0, len(data), B):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[at:at + B]) + c.flush()) + 26
    return total


# ---- the block kernel's sources as the CPU-side tests read them (tests/test_bgzf_*_abi.py, tests/test_bam_deflate_abi.py)
BLOCK_KERNELS = {(fields, dynamic): "bgzf_block_kernel<%s, %s>" % (str(fields).lower(), str(dynamic).lower())
                 for fields in (False, True) for dynamic in (False, True)}


@functools.lru_cache(maxsize=None)
def source_rows(source):
    """{kernel: its row of tools/isa_report.py} of one source of csrc, compiled once with the flags the library is built with."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    return {k["pretty"].split("::")[-1]: k for k in isa_report.kernels_of(isa_report.assembly(source))}


def assert_the_mode_is_built_in_one_place():
    """The three tuning keys of the encoder reach the launches as one BgzfMode, made from the context's LaunchState by one function: no
    other line of csrc reads a key, and every call hands the launch that function's result.  (tests/test_bgzf_fields_abi.py and tests/test_bam_deflate_abi.py ask it.)"""
    csrc = os.path.join(ROOT, "basevarc_amd", "csrc")
    texts = {f: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read()) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    made = re.search(r"BgzfMode bgzf_mode\(const LaunchState &ls\)\s*\{\s*return \{ls\.bgzf_parse == 1, ls\.bgzf_codes == 1, "
                     r"ls\.bgzf_cuts == 1 \? kBfDelimsSpaceNewline : kBfDelimsTabColon\};\s*\}", texts["bgzf_deflate_kernel.hip"])
    assert made, "bgzf_mode"
    for key in ("bgzf_parse", "bgzf_codes", "bgzf_cuts"):
        # its declaration in LaunchState, its row of the table of keys, and the one read
        reads = {f: len(re.findall(r"(?:\.|->|::)" + key + r"\b", text)) for f, text in texts.items()}
        assert {f: n for f, n in reads.items() if n} == {"bvc_context.hip": 1, "bgzf_deflate_kernel.hip": 1}, (key, reads)
    assert "kBfDelims" not in "".join(text for f, text in texts.items() if f not in ("bgzf_deflate_kernel.hip", "bgzf_fields_device.h"))
    assert re.search(r"launch_bgzf_deflate\([^;]*d_comp_off, bgzf_mode\(ctx->ls\)\)\);", texts["bvc_bgzf.hip"])
    assert sum(text.count("bgzf_mode(") for text in texts.values()) == 3          # declared, defined, called
    assert sum(len(re.findall(r"\blaunch_bgzf_deflate\(", text)) for text in texts.values()) == 3
