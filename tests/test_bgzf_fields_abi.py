"""The field parse of the device deflate encoder (tuning key "bgzf_parse") as far as a machine without a GPU can see it: the key is
declared in the header and in the library's table of knobs, the host program reads its knob, the new kernels are built from their own
source under the rules of every kernel and are in the library.  The plain Python model of the rule (tests/bgzf_fields_model.py,
docs/BGZF_FIELDS.md): its symbols reproduce every piece of tests/bgzf_fields_cases.py and of the catalogue of tests/bgzf_deflate_cases.py,
its matches are what the rule says on the hand-built pieces, zlib and the host program's inflater read what
tests/bgzf_dynamic_model.encode writes from them, and its size on the three sample-column texts is what
profiles/vcf_deflate_fields/README.txt records."""
import ctypes as C
import os
import re
import sys
import zlib

import pytest

from tests import bgzf_deflate_cases as dc
from tests import bgzf_dynamic_model as dm
from tests import bgzf_fields_cases as fc
from tests import bgzf_fields_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The committed model's output against zlib level 1 on the same bytes cut at the same marks (dc.zlib_size), N = 1e5: taken once on
# the CPU, {coverage: (fixed code or stored, the smallest of stored, fixed and dynamic)}.  The variant with the eight nearest heads of a
# key as candidates gave 0.915 / 1.049 / 0.926 and 0.744 / 0.776 / 0.635.
SIZE_AGAINST_LEVEL_1 = {0.10: (0.9015, 0.7424), 0.01: (1.0339, 0.7640), 1.0: (0.9124, 0.6458)}
MARGIN = 1.05


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_key_is_declared_and_the_host_program_reads_its_knob():
    from basevarc_amd import lib as bl
    header = read("include", "bvc.h")
    assert '"bgzf_parse"' in header and "BVC_BGZF_PARSE" in header
    # the key takes 0 and 1 and refuses 2: lo 0, hi 1, step 1, default 0 (bvc_set_tuning itself needs a device: tests/test_gpu_bgzf_fields.py)
    assert re.search(r'\{"bgzf_parse", "BVC_BGZF_PARSE", 0, 1, 1, 0, &LaunchState::bgzf_parse\}', read("basevarc_amd", "csrc", "bvc_context.hip"))
    dc.assert_the_mode_is_built_in_one_place()
    knobs = read("basevarc_amd", "host", "knobs.h")
    assert re.search(r'device_deflate_fields = num\("BVC_HOST_DEVICE_DEFLATE_FIELDS", 0\) != 0 && device_deflate;', knobs)
    assert re.search(r'knobs\.device_deflate_fields && bvc_set_tuning\(tr\.ctx, "bgzf_parse", 1\)', read("basevarc_amd", "host", "main.cpp"))
    # no new entry point: the key passes through bvc_set_tuning, which the binding hands any key
    assert "bvc_set_tuning" in bl.PROTOTYPES and not any("parse" in name or "fields" in name for name in bl.PROTOTYPES)
    assert "--parse" in read("tools", "bgzf_deflate_bench.py")


def test_the_kernels_are_in_the_library():
    from basevarc_amd import build as b
    from basevarc_amd import lib as bl
    b.build(force=b.needs_build())
    blob = open(bl.library_path(), "rb").read()
    # the four instantiations of the one block kernel, as their mangled names spell them, and none of the kernels they replaced
    for fields in (b"Lb0E", b"Lb1E"):
        for dynamic in (b"Lb0E", b"Lb1E"):
            assert b"17bgzf_block_kernelI" + fields + dynamic + b"E" in blob, (fields, dynamic)
    assert blob.count(b"_ZN3bvc17bgzf_block_kernelI") == blob.count(b"_ZN3bvc17bgzf_block_kernelILb") > 0      # (no other arguments)
    for kernel in (b"bgzf_deflate_fields_kernel", b"bgzf_deflate_fields_dynamic_kernel", b"bgzf_deflate_kernel", b"bgzf_deflate_dynamic_kernel"):
        assert b"%d%s" % (len(kernel), kernel) not in blob, kernel


def test_the_kernels_are_built_from_their_own_source_under_the_rules_of_every_kernel():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from basevarc_amd import build as b
    assert "bgzf_fields_kernel.hip" in b.SOURCES and "bgzf_fields_kernel.hip" in isa_report.DEVICE_SOURCES
    assert b.PER_SOURCE_FLAGS.get("bgzf_fields_kernel.hip") == ["-mllvm", "-disable-machine-licm"]
    assert {"bgzf_deflate_device.h", "bgzf_codes_device.h", "bgzf_dynamic_device.h", "bgzf_fields_device.h", "bgzf_block_kernel.h"} <= set(b.DEPS)
    rows = dc.source_rows("bgzf_fields_kernel.hip")
    assert set(rows) == {dc.BLOCK_KERNELS[True, False], dc.BLOCK_KERNELS[True, True]}, sorted(rows)
    fixed, dynamic = rows[dc.BLOCK_KERNELS[True, False]], rows[dc.BLOCK_KERNELS[True, True]]
    for k in (fixed, dynamic):
        assert k["private"] == 0 and k["scratch"] == 0 and k["flat"] == 0 and k["vgpr_spill"] == 0 and k["mfma"] == 0, k
        assert k["vgprs"] <= 128, k                                       # sixteen wavefronts a CU: 128 registers a lane at the most
    # the heads' bitmap and a round's best matches: 9 KiB beside what the general parse's kernels hold; one workgroup a CU either way
    assert 147600 + 8192 + 1024 == fixed["lds"] < dynamic["lds"] <= 160 * 1024
    # nothing is copied: the block's way through the passes is written once, in the template, and no source calls a pass itself
    template = read("basevarc_amd", "csrc", "bgzf_block_kernel.h")
    for header in ("bgzf_deflate_device.h", "bgzf_dynamic_device.h", "bgzf_fields_device.h"):
        assert f'#include "{header}"' in template
    csrc = os.path.join(ROOT, "basevarc_amd", "csrc")
    texts = {f: read("basevarc_amd", "csrc", f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    for call in ("bd_load(", "bd_path(", "BVC_POISON_LDS()", "bd_matches(", "bd_field_matches(", "bd_fixed_block(", "bd_dynamic_block("):
        assert template.count(call) == 1, call
    for call in ("bd_load(", "bd_path(", "bd_matches(", "bd_field_matches(", "bd_fixed_block(", "bd_dynamic_block("):
        # the template, and the device header that defines the pass
        assert len([f for f, text in texts.items() if call in text]) == 2, call
    assert "bd_field_matches(" in texts["bgzf_fields_device.h"]
    for source in ("bgzf_deflate_kernel.hip", "bgzf_dynamic_kernel.hip", "bgzf_fields_kernel.hip"):
        assert '#include "bgzf_block_kernel.h"' in texts[source]
        assert "atomicMax(" not in texts[source] and "hash_of(" not in texts[source] and "s_in" not in texts[source]


# ---- the model
@pytest.fixture(scope="module")
def parsed():
    """[(name, block, parse, symbols)] of every block of the new pieces, the existing catalogue and the stream pieces."""
    cases = fc.catalogue() + dc.catalogue() + [(f"piece {i}", p) for i, p in enumerate(dc.stream_pieces())]
    out = []
    for name, piece in cases:
        for data in fm.blocks_of(piece):
            ps = fm.parse(data)
            out.append((name, data, ps, fm.symbols(data, ps)))
    return out


def test_the_models_symbols_reproduce_the_input_and_keep_the_rule(parsed):
    assert len({name for name, _, _, _ in parsed}) > 800
    for name, data, ps, symbols in parsed:
        assert dm.plain_bytes(symbols) == data, name
        n = len(data)
        cuts, length_of = {p for p, _ in ps["fields"]} | {n}, dict(ps["fields"])
        assert sum(length for _, length in ps["fields"]) == n, name
        for p, (length, dist) in ps["match"].items():
            # matches begin and end at cuts (or at the block's end), inside the block, of deflate's lengths and distances
            assert p in cuts and p + length in cuts and 4 <= length <= 258 and 1 <= dist <= min(p, 32768), (name, p, length, dist)
            assert data[p:p + length] == (data[p - dist:p] * (length // dist + 1))[:length], (name, p)
            if p not in ps["heads"]:
                assert dist == length_of[p] and length % dist == 0, (name, p)
        for p, c in ps["candidates"].items():
            assert len(c) <= 17 and all(q < p and q in ps["heads"] for q in c), (name, p)
        p = 0
        for s in symbols:                                                  # the walk is at a cut or inside an unmatched field
            if isinstance(s, tuple):
                assert p in cuts, (name, p)
            p += s[0] if isinstance(s, tuple) else 1


def test_the_models_matches_on_the_hand_built_pieces():
    by = dict(fc.catalogue())

    def matches(name, block=0):
        return [s for s in fm.symbols(fm.blocks_of(by[name])[block]) if isinstance(s, tuple)]
    for n in range(1, 35):
        again, thrice = matches(f"fields: head of {n} bytes met again"), matches(f"fields: field of {n} bytes three times")
        assert again == ([(n, n + 3)] if 4 <= n <= 32 else []), (n, again)             # a key from 4 to 32 bytes
        assert thrice == ([(2 * n, n)] if 2 * n >= 4 else []), (n, thrice)             # a repeat at any length
    for n in (1, 3, 4, 17):
        whole = 258 // n * n
        for name in by:
            m = re.fullmatch(rf"fields: (\d+) repeats of {n} bytes( up to the end)?", name)
            if m:
                left, want = int(m.group(1)) * n, []
                while left >= 4 and min(left, 258) // n * n >= 4:
                    want.append((min(left, 258) // n * n, n))
                    left -= want[-1][0]
                assert matches(name) == want and (not want or want[0][0] <= whole), (name, matches(name), want)
    assert matches("fields: a run across a round's edge") == [(44, 4)]
    for at in (255, 256, 511, 512, 16 * 256, 16 * 256 + 255, 17 * 256):
        assert matches(f"fields: a head at position {at}") == [(5, at)]
    assert matches("fields: a head at the last position of each of three rounds") == [(5, 255), (5, 256), (5, 256)]
    assert matches("fields: the only candidate at distance 32768") == [(5, 32768)]
    assert matches("fields: the only candidate at distance 32769") == []
    assert matches("fields: the extension stops in the middle of a field") == [(5, 15)]
    assert matches("fields: the extension stops in the middle of the next field") == [(5, 12)]
    assert matches("fields: the extension stops at the head's own end") == [(5, 9)]
    assert matches("fields: the extension stops at a cut three fields on") == [(9, 13)]
    assert matches("fields: the extension reaches the block's end") == [(9, 12)]
    assert matches("fields: the extension reaches the block's end inside a field") == [(9, 14)]
    assert matches("fields: the extension reaches 258 bytes inside a field") == [(5, 308)]
    assert (258, 288) in matches("fields: the extension reaches 258 bytes at a cut")
    assert matches("fields: the farther candidate is the longer") == [(7, 256), (9, 512)]
    assert matches("fields: the nearer candidate is the longer") == [(7, 256), (9, 256)]
    assert matches("fields: the nearer of two equal candidates") == [(9, 256), (9, 256)]
    assert matches("fields: two heads with the key in the round itself") == [(7, 11), (7, 22)]   # (not (9, 11): the second head is no candidate)
    assert matches("fields: a head's twin in the block before", 1) == [(5, 5)]
    assert matches("fields: 65280 tabs") == [(258, 1)] * 253 + [(5, 1)]                 # 1 + 253 x 258 + 5
    assert matches("fields: no cut, 3000 letters") == []
    # a field astride the cut: the second block starts inside a field and takes that rest for its first field
    first, second = fm.blocks_of(by["fields: a field astride a piece's cut"])
    assert first[-1:] not in (b"\t", b":") and fm.parse(second)["fields"][0] == (0, min(second.index(b":"), second.index(b"\t")) + 1)


def test_zlib_and_the_host_programs_inflater_read_both_encodings(parsed):
    from basevarc_amd import build as b
    _, lib = b.build_host()
    H = C.CDLL(lib)
    H.bvchost_fast_inflate.restype = C.c_long
    H.bvchost_fast_inflate.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    forms = set()
    for name, data, _, symbols in parsed:
        if not data or name.startswith("piece ") and len(data) < 50:
            continue
        m = dm.encode(symbols)
        forms.add(m["chosen"])
        for f in ("fixed", "dynamic"):
            d = zlib.decompressobj(-15)
            assert d.decompress(m[f]) == data and d.eof and d.unused_data == b"", (name, f)
            buf = C.create_string_buffer(len(data) + 1)
            assert H.bvchost_fast_inflate(m[f], len(m[f]), buf, len(data)) == len(data) and buf.raw[:len(data)] == data, (name, f)
    assert forms == {"stored", "fixed", "dynamic"}


def test_size_on_the_sample_column_texts_against_zlib_level_1():
    for coverage, seed, _ in dc.SIZE_TEXTS:
        text = dc.sample_text(100000, coverage, seed)
        fixed = dynamic = heads = 0
        blocks = fm.blocks_of(text)
        for data in blocks:
            ps = fm.parse(data)
            heads += len(ps["heads"])
            m = dm.encode(fm.symbols(data, ps))
            fixed += min(len(m["fixed"]), len(data) + 5) + 26
            dynamic += len(m["data"]) + 26
        z1, z6 = dc.zlib_size(text, 1), dc.zlib_size(text, 6)
        print(f"coverage {coverage}: text {len(text)}, {heads / len(blocks):.0f} heads a block, fixed {fixed}, dynamic {dynamic}, zlib level 1 {z1}, "
              f"level 6 {z6}: fixed / level 1 {fixed / z1:.4f}, dynamic / level 1 {dynamic / z1:.4f}, / level 6 {fixed / z6:.3f}, {dynamic / z6:.3f}")
        want_fixed, want_dynamic = SIZE_AGAINST_LEVEL_1[coverage]
        assert fixed / z1 <= want_fixed * MARGIN and dynamic / z1 <= want_dynamic * MARGIN, (coverage, fixed / z1, dynamic / z1)
        assert fixed / z1 >= want_fixed / MARGIN and dynamic / z1 >= want_dynamic / MARGIN, (coverage, fixed / z1, dynamic / z1)
