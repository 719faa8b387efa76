"""The revisit rule of a run that piles phase 1 into class counts (host/pileup.h, counts_revisit; no device): which positions must be read
again entry by entry once the counts pass has made their class counts and tallies.

1. bvchost_counts_revisit against tests/bam_counts_model.revisit on seeded random tallies and on hand-made windows: one that starts with an
   indel position, one with two indel positions sharing a predecessor, one whose predecessor holds only class-4 tokens.
2. The rule is sufficient, on the CPU restatement of the pipeline (tests/hostref.Pipeline) over the 100 test BAMs: the CVG lines of the
   positions outside the set made from the model's tallies alone, plus the reference's parser run over the set alone per thread window,
   give Pipeline.outputs() -- VCF and CVG, for 1 and 4 threads.  Without the rule's third part they do not: the predecessor is needed.
3. The rule in a stand-alone program under the address sanitizer (tests/cpp/counts_revisit_main.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import bam_counts_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    from basevarc_amd import build as b
    _, lib = b.build_host()
    h = C.CDLL(lib)
    h.bvchost_counts_revisit.restype = None
    h.bvchost_counts_revisit.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    return h


def host_revisit(H, tally, called, thread):
    t = np.ascontiguousarray(tally)
    c = np.ascontiguousarray(called, dtype=np.uint8)
    flags = np.full(len(t) + 8, 0xEE, dtype=np.uint8)
    H.bvchost_counts_revisit(C.c_void_p(t.ctypes.data), C.c_void_p(c.ctypes.data), len(t), thread, C.c_void_p(flags.ctypes.data))
    assert (flags[len(t):] == 0xEE).all()
    return flags[:len(t)]


def tallies(spec):
    """spec: one string a position -- 'b' a base token of class 0..3, 'n' only class-4 tokens, 'i' indel entries, 'bi' both, '.' nothing."""
    t = np.zeros(len(spec), dtype=cm.TALLY)
    for k, s in enumerate(spec):
        if "b" in s:
            t["strand_base"][k, (3 * k) % 8] = 1 + k % 3
        if "n" in s:
            t["n_other"][k] = 2
        if "i" in s:
            t["n_indel"][k] = 1 + k % 2
    return t


def test_the_hand_made_windows(H):
    I, CY = cm.INDEL, cm.CARRY
    none = np.zeros(16, dtype=np.uint8)
    for spec, want in (
            (["i", "b", ".", "i"], [I, CY, 0, I]),                        # starts with an indel position: nothing in front to carry
            (["b", "b", ".", "i", ".", "i", "b"], [0, CY, 0, I, 0, I, 0]),  # two indel positions sharing a predecessor
            (["b", "n", ".", "i"], [0, CY, 0, I]),                        # the predecessor holds only class-4 tokens: still the last base token
            (["b", "bi", "i"], [CY, I | CY, I]),                          # an indel position with base tokens is the next one's predecessor
            ([".", ".", "i", "."], [0, 0, I, 0]),
            (["b", ".", "."], [0, 0, 0])):
        t = tallies(spec)
        got = host_revisit(H, t, none[:len(spec)], 1)
        assert got.tolist() == cm.revisit(t, none[:len(spec)], 1).tolist() == want, (spec, got.tolist())
    # the predecessor is looked for inside the thread's window alone: two threads over six positions cut them 3 + 3
    t = tallies(["b", ".", ".", "i", "b", "i"])
    assert cm.thread_window(6, 2, 0) == (0, 3) and cm.thread_window(6, 2, 1) == (3, 6)
    assert host_revisit(H, t, none[:6], 1).tolist() == [CY, 0, 0, I, CY, I]
    assert host_revisit(H, t, none[:6], 2).tolist() == cm.revisit(t, none[:6], 2).tolist() == [0, 0, 0, I, CY, I]
    # called positions are in the set whatever they hold
    called = np.array([0, 1, 0, 1, 0, 0], dtype=np.uint8)
    assert host_revisit(H, t, called, 1).tolist() == [CY, cm.CALLED, 0, I | cm.CALLED, CY, I]
    assert host_revisit(H, t[:0], called[:0], 3).tolist() == []


def test_seeded_random_tallies_against_the_model(H):
    rng = np.random.default_rng(20261020)
    seen = 0
    for P in (1, 2, 7, 64, 500, 3000):
        for density in (0.6, 0.1, 0.01):
            t = np.zeros(P, dtype=cm.TALLY)
            t["strand_base"] = rng.integers(1, 5, size=(P, 8)) * (rng.random((P, 8)) < density / 2)
            t["n_other"] = rng.random(P) < density / 3
            t["n_indel"] = (rng.random(P) < 0.08) * rng.integers(1, 3, size=P)
            called = (rng.random(P) < 0.03).astype(np.uint8)
            for thread in (1, 2, 4, 8, 13):
                got = host_revisit(H, t, called, thread)
                assert got.tolist() == cm.revisit(t, called, thread).tolist(), (P, density, thread)
                seen |= int(np.bitwise_or.reduce(got)) if P else 0
                # what the rule promises: every called and every indel position, and never a position without a base token for the carry
                assert ((got & cm.CALLED) != 0).tolist() == (called != 0).tolist() and ((got & cm.INDEL) != 0).tolist() == (t["n_indel"] > 0).tolist()
                bases = t["strand_base"].sum(axis=1) + t["n_other"]
                assert not ((got & cm.CARRY) != 0)[bases == 0].any()
    assert seen == cm.CALLED | cm.INDEL | cm.CARRY


# ---- the rule is sufficient, and its third part is needed ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline():
    """The CPU restatement's entries of the 100 test BAMs, the model's tallies of them, and the called positions (those of its VCF)."""
    from tests import hostref
    P = hostref.Pipeline(mapq=20)
    _, tally = cm.fold(P.maps, P.pv)
    first = P.outputs()
    vcf = first[0]
    called_at = {int(l.split("\t")[1]) for l in vcf.splitlines()}
    called = np.array([p in called_at for p in P.pv], dtype=np.uint8)
    assert called.sum() == len(called_at) == 76 and int((tally["n_indel"] > 0).sum()) == 45 and len(P.pv) == 66615
    return P, tally, called, first


def outputs_from_counts(P, tally, flags, thread):
    """(vcf, cvg) made as a run on counts makes them: per thread window the reference's parser (one long-lived AlleleInfo, fresh per window)
    sees the lines of the flagged positions alone; every other position's CVG line comes from its tally."""
    from oracle import emit_oracle as eo
    from oracle import orc
    vcf, cvg = [], []
    for i in range(thread):
        parser = eo.Parser()
        lo, hi = cm.thread_window(len(P.pv), thread, i)
        for t in range(lo, hi):
            p = P.pv[t]
            ref = "ACGT".index(P.refseq[p - P.rg_s])
            if flags[t]:
                aiv, sample = parser.parse(["".join(eo.format_token(m.get(p)) for m in P.maps) + "\n"])
                if not aiv:
                    continue
                cvg.append(eo.cvg_line(P.chr, p, ref, aiv))
                e = orc.basetype_lrt([a["base"] for a in aiv if not a["is_indel"]], [a["qual"] for a in aiv if not a["is_indel"]], ref, P.min_af)
                if e["called"]:
                    vcf.append(eo.vcf_line(e, P.chr, p, ref, aiv, sample, P.n, {}))
                continue
            sb = tally["strand_base"][t]
            if not sb.any():
                continue                                         # no entry the parser keeps: no line
            aiv = [dict(base=k & 3, strand=k >> 2, is_indel=0) for k in range(8) for _ in range(int(sb[k]))]
            cvg.append(eo.cvg_line(P.chr, p, ref, aiv))
    return "".join(vcf), "".join(cvg)


@pytest.mark.parametrize("thread", [1, 4])
def test_the_rule_is_sufficient_and_the_predecessor_is_needed(H, pipeline, thread):
    P, tally, called, first = pipeline
    P.thread = thread
    want = first if thread == 1 else P.outputs()
    flags = host_revisit(H, tally, called, thread)
    assert flags.tolist() == cm.revisit(tally, called, thread).tolist()
    n_carry = int(((flags & cm.CARRY) != 0).sum())
    assert 0 < n_carry <= 45 and 76 <= int((flags != 0).sum()) <= 76 + 45 + 45
    got = outputs_from_counts(P, tally, flags, thread)
    assert got[0] == want[0] and got[0].count("\n") == 76
    assert got[1] == want[1]
    # without the predecessors some indel position's strand counts come out wrong: the third part of the rule is not decoration
    short = cm.revisit(tally, called, thread, carry=False)
    assert int((short != 0).sum()) < int((flags != 0).sum())
    assert outputs_from_counts(P, tally, short, thread)[1] != want[1]


def test_the_rule_under_the_address_sanitizer(tmp_path):
    """host/pileup.h's counts_revisit in a stand-alone program (tests/cpp/counts_revisit_main.cpp) built with -fsanitize=address,undefined:
    every array a heap block of exactly its size."""
    host_dir = os.path.join(ROOT, "basevarc_amd", "host")
    exe = str(tmp_path / "counts_revisit")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-fno-omit-frame-pointer", "-pthread", "-I", host_dir, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "counts_revisit_main.cpp")] +
                          [os.path.join(host_dir, f) for f in ("pileup.cpp", "stats.cpp", "bgzf.cpp", "inflate.cpp")] + ["-lz", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-4000:]
    assert "105 cases, 0 wrong" in text
