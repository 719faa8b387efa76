// popmatrix_main.cpp -- fetch_allele_type (host/bam.cpp) and the position-file reader (host/popmatrix.cpp) on hand-built records, as a
// stand-alone program: tests/test_popmatrix_abi.py builds it with -fsanitize=address,undefined and runs it.  Prints "<n> cases, <k> wrong".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "bam.h"
#include "popmatrix.h"

using namespace bvchost;

static int g_cases = 0, g_wrong = 0;

static BamRecord read(int32_t pos, std::vector<std::pair<char, int32_t>> cigar, const std::string &seq, uint16_t flag = 0)
{
    BamRecord r;
    r.ref_id = 0; r.pos = pos; r.mapq = 30; r.flag = flag; r.cigar = std::move(cigar); r.seq = seq; r.qual.assign(seq.size(), (char)30);
    return r;
}

static std::vector<PosInfo> lines(std::initializer_list<PosInfo> l) { return std::vector<PosInfo>(l); }
static PosInfo at(int32_t pos, char ref, char alt) { PosInfo p; p.chr = "c"; p.pos = pos; p.ref = ref; p.alt = alt; return p; }

static void expect(const char *name, const std::vector<BamRecord> &rv, const std::vector<PosInfo> &pv, const std::string &want, const std::string &refseq,
                   int32_t rg_s = 1000)
{
    ++g_cases;
    std::string got;
    try { got = fetch_allele_type(rv, rg_s, refseq, pv); } catch (const std::out_of_range &) { got = "!"; }
    if (got != want) { ++g_wrong; std::printf("WRONG %s: got %s, want %s\n", name, got.c_str(), want.c_str()); }
}

int main(int argc, char **argv)
{
    const std::string ref(200, 'A');
    // the empty read list: dots, never rv[0]
    expect("no read", {}, lines({at(1010, 'A', 'C'), at(1011, 'A', 'C')}), "..", ref);
    expect("no read, no line", {}, {}, "", ref);
    // one read 1010..1013 = A C G N: in front of it, its first and last base, behind it (the cursor sticks at the last read)
    const std::vector<BamRecord> one = {read(1009, {{'M', 4}}, "ACGN")};
    expect("one read", one, lines({at(1009, 'A', 'C'), at(1010, 'A', 'C'), at(1011, 'A', 'C'), at(1012, 'T', 'C'), at(1013, 'N', 'A'), at(1013, 'n', '='),
                                   at(1014, 'A', 'C')}), ".01.0..", ref);
    expect("one read, a list that descends", one, lines({at(1013, 'N', 'A'), at(1010, 'A', 'C'), at(1020, 'A', 'C'), at(1011, 'C', 'A')}), "00.0", ref);
    // two reads and a list that descends: the cursor stands on the second read, which starts behind 1012
    expect("two reads, descending", {read(1009, {{'M', 10}}, std::string(10, 'A')), read(1029, {{'M', 10}}, std::string(10, 'C'))},
           lines({at(1035, 'C', 'A'), at(1012, 'A', 'C')}), "0.", ref);
    // a CIGAR ending short of the position: a read's span is its CIGAR's, so the scan always finds an operation -- but clips and pads
    // move the rule's reference coordinate, so it stops early: 1010 is "in" the clip, and behind the pad the query offset is one short
    expect("soft clip and pad", {read(1009, {{'S', 2}, {'M', 3}, {'P', 1}, {'M', 3}}, "TTACGACG")}, lines({at(1010, 'T', 'A'), at(1012, 'G', 'A'), at(1015, 'G', 'A')}),
           "10.", ref);
    // the indel token: a dot, and the next position is a base again
    expect("insertion next", {read(1009, {{'M', 3}, {'I', 2}, {'M', 3}}, "ACGTTACG")}, lines({at(1011, 'C', 'A'), at(1012, 'G', 'A'), at(1013, 'A', 'C')}), "0.0", ref);
    expect("deletion, the next read covers it", {read(1009, {{'M', 3}, {'D', 3}, {'M', 3}}, "ACGACG"), read(1011, {{'M', 8}}, "GGGGGGGG")},
           lines({at(1012, 'G', 'A'), at(1013, 'G', 'A'), at(1015, 'G', 'A'), at(1016, 'A', 'C')}), ".000", ref);
    expect("deletion, nobody else", {read(1009, {{'M', 3}, {'D', 3}, {'M', 3}}, "ACGACG")}, lines({at(1013, 'G', 'A'), at(1016, 'A', 'C')}), ".0", ref);
    expect("reference skip, the next read starts behind", {read(1009, {{'M', 3}, {'N', 3}, {'M', 3}}, "ACGACG"), read(1019, {{'M', 3}}, "AAA")},
           lines({at(1014, 'G', 'A')}), ".", ref);
    // the out-of-range cases
    expect("query offset past the sequence", {read(1009, {{'M', 10}}, "ACGTA")}, lines({at(1012, 'G', 'A'), at(1016, 'A', 'C')}), "!", ref);
    expect("empty sequence", {read(1009, {{'M', 10}}, "")}, lines({at(1012, 'G', 'A')}), "!", ref);
    expect("insertion that starts past the sequence", {read(1009, {{'M', 5}, {'I', 3}, {'M', 5}}, "ACG")}, lines({at(1014, 'G', 'A')}), "!", ref);
    expect("deletion that starts past the reference", {read(1039, {{'M', 5}, {'D', 3}, {'M', 5}}, "ACGTACGTAC")}, lines({at(1044, 'A', 'C')}), "!", ref.substr(0, 30));
    expect("deletion that starts at the reference's end", {read(1024, {{'M', 5}, {'D', 3}, {'M', 5}}, "ACGTACGTAC")}, lines({at(1029, 'A', 'C')}), ".", ref.substr(0, 30));
    // (the text is built before the length is looked at: a zero-length insertion past the sequence throws, one inside it is no token)
    expect("zero-length insertion that starts past the sequence", {read(1009, {{'M', 5}, {'I', 0}, {'M', 5}}, "ACG")}, lines({at(1014, 'G', 'A')}), "!", ref);
    expect("zero-length insertion inside the sequence", {read(1009, {{'M', 5}, {'I', 0}, {'M', 5}}, "ACGTACGTAC")}, lines({at(1014, 'A', 'C')}), "0", ref);
    expect("deletion in front of the region's start", {read(1009, {{'M', 5}, {'D', 3}, {'M', 5}}, "ACGTACGTAC")}, lines({at(1014, 'A', 'C')}), "!", ref, 1100);

    // the position file: any white space between the fields, one character each for REF and ALT, the first bad line ends the list
    if (argc > 1) {
        const std::string path = std::string(argv[1]) + "/lines.pos";
        { std::ofstream f(path); f << "chr1 10 A C\n\n  chr1\t11\tAC\n chr2 12 G T trailing\nchr1 x A C\nchr1 13 A C\n"; }
        std::vector<PosInfo> pv;
        ++g_cases;
        // "AC" is REF 'A' and ALT 'C'; "trailing" is read as the next line's chr, whose pos then does not parse
        const bool ok = read_posfile(path, pv) && pv.size() == 3 && pv[0].chr == "chr1" && pv[0].pos == 10 && pv[0].ref == 'A' && pv[0].alt == 'C' &&
                        pv[1].pos == 11 && pv[1].ref == 'A' && pv[1].alt == 'C' && pv[2].chr == "chr2" && pv[2].pos == 12 && pv[2].alt == 'T' &&
                        posfile_region(pv) == "chr2:10-12" && positions_do_not_descend(pv);
        if (!ok) { ++g_wrong; std::printf("WRONG posfile: %zu lines\n", pv.size()); }
        ++g_cases;
        std::vector<PosInfo> none;
        if (read_posfile(path + ".missing", none) || !none.empty()) { ++g_wrong; std::printf("WRONG missing posfile\n"); }
        ++g_cases;
        if (positions_do_not_descend(lines({at(5, 'A', 'C'), at(5, 'A', 'G'), at(4, 'A', 'C')}))) { ++g_wrong; std::printf("WRONG descending\n"); }
    }
    std::printf("%d cases, %d wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
