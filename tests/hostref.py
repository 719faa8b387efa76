"""Python pipeline for the reference's `BaseVarC basetype` run on its own test data (test infrastructure):
BAM -> per-sample pileup -> temp-batch text -> parse -> BaseType (oracle) -> CVG/VCF text.  Used to check the
C++ host program (basevarc_amd/host) file by file.  Everything here restates reference source text
(see oracle/emit_oracle.py and tests/golden/make_testdata_pileup.py); parity is unpinned."""
import os

from oracle import emit_oracle as eo
from tests.golden import make_testdata_pileup as tp

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "testdata")
REGION = "chr17:41197700-41276155"
BUF = 1000                                  # the reference is fetched this far behind the region, and the reads this far around it


class Cohort:
    """What a run reads, for cohorts other than the 100 test BAMs (tests/cohort_cases.py writes them): the directory, the BAM paths in list
    order, the region as the command line takes it, the contig table [(name, length)] and the contigs' sequences {name: text}."""

    def __init__(self, directory, bams, region, contigs, sequences):
        self.dir, self.bams, self.region, self.contigs, self.sequences = str(directory), list(bams), region, list(contigs), dict(sequences)

    def split_region(self):
        """(contig, start, end) as splitrg reads the text, before its end - 1"""
        chrom, rest = self.region.split(":")
        s, e = rest.split("-")
        return chrom, int(s), int(e)

    def fetched(self):
        """the string fetch_reference gives for [start, end - 1 + BUF], clamped to the contig"""
        chrom, s, e = self.split_region()
        return self.sequences[chrom][s - 1:e - 1 + BUF]


def region_fixture(cohort=None):
    if cohort is not None:
        chrom, s, _ = cohort.split_region()
        return chrom, s, dict(cohort.contigs)[chrom], cohort.fetched()
    head, seq = open(os.path.join(DATA, "chr17_41197700_region.txt")).read().split("\n")[:2]
    contig, start, length = head.split()
    return contig, int(start), int(length), seq


def write_fasta(path, cohort=None):
    """A full-length single-contig FASTA (N outside the fixture region) + .fai, so that chr17 coordinates work.  A cohort's: every
    contig on one line."""
    if cohort is not None:
        from tests import bam_files
        return bam_files.write_reference(path, [(n, cohort.sequences[n]) for n, _ in cohort.contigs])
    contig, start, length, seq = region_fixture()
    with open(path, "w") as f:
        f.write(f">{contig}\n")
        f.write("N" * (start - 1))
        f.write(seq)
        f.write("N" * (length - (start - 1) - len(seq)))
        f.write("\n")
    with open(path + ".fai", "w") as f:
        f.write(f"{contig}\t{length}\t{len(contig) + 2}\t{length}\t{length + 1}\n")
    return path


def write_bam_list(path, cohort=None):
    with open(path, "w") as f:
        if cohort is not None:
            f.write("".join(b + "\n" for b in cohort.bams))
            return path
        for l in open(os.path.join(DATA, "bam.list")):
            if l.strip():
                f.write(os.path.join(DATA, l.strip().replace("data/", "", 1)) + "\n")
    return path


def thread_window(psize, thread, ithread):
    window = psize % thread + psize // thread
    lo = min(psize, ithread * window)
    hi = psize if ithread == thread - 1 else min(psize, (ithread + 1) * window)
    return lo, hi


class Pipeline:
    def __init__(self, mapq=20, batch=10, thread=1, maf=0.001, cohort=None):
        self.batch, self.thread, self.cohort = batch, thread, cohort
        contig, start, _, refseq = region_fixture(cohort)
        self.chr, self.refseq = contig, refseq
        chrom, s, e = tp.REGION if cohort is None else cohort.split_region()
        self.rg_s, self.rg_e = s, e - 1
        self.pv = [self.rg_s + i for i in range(len(refseq) - BUF) if refseq[i] in "ACGT"]
        if cohort is None:
            lst = os.path.join(DATA, "bam.list")
            names, rvs, _ = tp.load_samples(DATA, self._list_for_loader(lst), mapq=mapq)
        else:
            lst = write_bam_list(os.path.join(cohort.dir, "pipeline.list"), cohort)
            names, rvs, _ = tp.load_samples(cohort.dir, lst, region=(chrom, s, e), mapq=mapq)
        self.empty = [n for n, rv in zip(names, rvs) if not rv]     # the samples bt_r reports as empty, in list order
        self.names = names
        self.maps = [tp.find_snp_at_pos(rv, self.pv, refseq, self.rg_s) for rv in rvs]
        self.n = len(names)
        self.min_af = min(100.0 / self.n, 0.001, maf)

    @staticmethod
    def _list_for_loader(lst):
        import tempfile
        t = tempfile.NamedTemporaryFile("w", suffix=".list", delete=False)
        for l in open(lst):
            if l.strip():
                t.write(l.strip().replace("data/", "", 1) + "\n")
        t.close()
        return t.name

    def batch_files(self):
        """{(ithread, ibatch): text} as bt_r writes them."""
        nb = 1 + (self.n - 1) // self.batch
        out = {}
        psize = len(self.pv)
        for ib in range(nb):
            ms = self.maps[ib * self.batch:(ib + 1) * self.batch]
            names = "".join(n + "\t" for n in self.names[ib * self.batch:(ib + 1) * self.batch]) + "\n"
            for t in range(self.thread):
                lo, hi = thread_window(psize, self.thread, t)
                lines = [names]
                for p in self.pv[lo:hi]:
                    lines.append("".join(eo.format_token(m.get(p)) for m in ms) + "\n")
                out[(t, ib)] = "".join(lines)
        return out

    def outputs(self, group_of=None):
        """(vcf_text, cvg_text) bodies of the merged outputs.  group_of: {sample name: group name} or None."""
        import numpy as np
        from oracle import orc
        gnames, gidx = [], None
        if group_of:
            gnames = sorted(set(group_of[n] for n in self.names if n in group_of))
            gidx = np.array([gnames.index(group_of[n]) if n in group_of else 255 for n in self.names], dtype=np.uint8)
        files = self.batch_files()
        nb = 1 + (self.n - 1) // self.batch
        vcf, cvg = [], []
        for t in range(self.thread):
            P = eo.Parser()
            per_batch = [files[(t, ib)].split("\n")[1:] for ib in range(nb)]
            lo, hi = thread_window(len(self.pv), self.thread, t)
            for k, p in enumerate(self.pv[lo:hi]):
                aiv, sample = P.parse([pb[k] for pb in per_batch])
                if not aiv:
                    continue
                ref = "ACGT".index(self.refseq[p - self.rg_s])
                b = [a["base"] for a in aiv if not a["is_indel"]]
                q = [a["qual"] for a in aiv if not a["is_indel"]]
                e = orc.basetype_lrt(b, q, ref, self.min_af)
                gd, info = None, {}
                if gnames:
                    db = np.full(self.n, -1, dtype=np.int8)
                    dq = np.zeros(self.n, dtype=np.int8)
                    for a, j in zip(aiv, sample):
                        if not a["is_indel"]:
                            db[j], dq[j] = a["base"], a["qual"]
                    _, gdep, gaf, ran, pres = orc.dense_site_groups(db, dq, ref, self.min_af, gidx, len(gnames))
                    gd = gdep.tolist()
                    for g, name in enumerate(gnames):            # src/BaseVarC.cpp:646-659
                        if ran[g]:
                            info[name + "_AF"] = ",".join(eo.fx(gaf[g][i], 6) if pres[g] >> i & 1 else "0"
                                                          for i in range(e["n_alt"]))
                        else:
                            info[name + "_AF"] = "0"
                cvg.append(eo.cvg_line(self.chr, p, ref, aiv, gd))
                if e["called"]:
                    vcf.append(eo.vcf_line(e, self.chr, p, ref, aiv, sample, self.n, info))
        return "".join(vcf), "".join(cvg)


def headers(reference_path, names, group_names=(), cohort=None):
    contig, _, length, _ = region_fixture(cohort)
    contigs = [(contig, length)] if cohort is None else cohort.contigs
    # CVG_HEADER / VCF_HEADER, src/BaseVarC.cpp:65-88; assembled as bt_s does (:364-382)
    from tests.hostref_headers import CVG_HEADER, VCF_HEADER
    vh = VCF_HEADER
    for g in group_names:
        vh += (f"##INFO=<ID={g}_AF,Number=A,Type=Float,Description=\"Allele frequency in the {g} populations "
               "calculated based on LRT.[0,1]\">\n")
    vh += "".join(f"##contig=<ID={c},length={l}>\n" for c, l in contigs) + f"##reference=file://{reference_path}\n"
    vh += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n"
    return vh, CVG_HEADER + "".join("\t" + g for g in group_names) + "\n"


# ---- comparing a VCF with the pipeline's ---------------------------------------------------------------------------------------------
# The bars per key.  QUAL is printed {:.2f}: one unit of the last place and a tenth.  The keys printed {:.3f} likewise.  The allele
# frequencies are printed {:.6f} and computed by the device's EM: AF_ATOL of tests/test_gpu_lrt_sites.py (1e-6) plus one unit of the last
# printed place.  Everything else -- counts, depths, the sample columns -- is text and must be equal.
QUAL_BAR = 0.011
FIXED3_KEYS = ("QD", "MQRankSum", "ReadPosRankSum", "BaseQRankSum", "FS", "SOR")
FIXED3_BAR = 1.1e-3
AF_BAR = 2e-6


def info_bar(key):
    if key in ("CM_AF", "CM_CAF") or key.endswith("_AF"):
        return AF_BAR
    return FIXED3_BAR if key in FIXED3_KEYS else 0.0


def compare_vcf(got, want, say=True):
    """Line for line: equal text, apart from float fields within the bars above.  Returns {key: the worst difference seen} (and prints it,
    so that a run kept with its output shows how near the bars the fields came)."""
    worst = {}

    def near(key, x, y, bar):
        if x == y:
            return
        d = abs(float(x) - float(y))
        worst[key] = max(worst.get(key, 0.0), d)
        assert d <= bar, (key, x, y, bar)             # (a nan on one side only is no number <= bar: it fails here)
    gl, wl = got.split("\n"), want.split("\n")
    assert len(gl) == len(wl), (len(gl), len(wl))
    for g, w in zip(gl, wl):
        if g == w:
            continue
        gf, wf = g.split("\t"), w.split("\t")
        assert len(gf) == len(wf) > 8 and gf[:5] == wf[:5] and gf[6] == wf[6] and gf[8:] == wf[8:], (g[:300], w[:300])
        near("QUAL", gf[5], wf[5], QUAL_BAR)
        ga, wa = gf[7].split(";"), wf[7].split(";")
        assert len(ga) == len(wa), (gf[7], wf[7])
        for a, c in zip(ga, wa):
            (ka, va), (kc, vc) = a.split("="), c.split("=")
            assert ka == kc and va.count(",") == vc.count(","), (a, c)
            for x, y in zip(va.split(","), vc.split(",")):
                near(ka, x, y, info_bar(ka))
    if say and worst:
        print("vcf worst differences: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(worst.items())))
    return worst
