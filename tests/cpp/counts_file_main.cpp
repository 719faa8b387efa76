// counts_file_main.cpp -- host/counts_file.cpp in a stand-alone program for the address and undefined-behaviour sanitizers: a counts file is
// written and read back piece for piece, and every prefix of its bytes -- the file cut at every length, section boundaries included -- is
// refused by the reader with one line, as is a byte changed in the magic, the version, the shape and the end mark.
// Usage: counts_file_main <scratch directory>.  Prints "<n> checks, <w> wrong".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "counts_file.h"

static int checks = 0, wrong = 0;
static void expect(bool ok, const std::string &what)
{
    ++checks;
    if (!ok) { ++wrong; std::cout << "WRONG: " << what << std::endl; }
}

// Reads the whole file: 0 sound, 1 refused (one line in err)
static int read_all(const std::string &path, CountsFileMeta &m, std::vector<CountsPiece> &pieces, std::string &err)
{
    CountsFileReader r;
    pieces.clear();
    if (!r.open(path, m, err)) return 1;
    CountsPiece p;
    int rc;
    while ((rc = r.next(p, err)) == 1) pieces.push_back(p);
    return rc < 0 ? 1 : 0;
}

static void write_bytes(const std::string &path, const std::string &bytes, size_t n)
{
    std::ofstream f(path.c_str(), std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), (std::streamsize)n);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::cerr << "usage: counts_file_main <scratch directory>" << std::endl; return 2; }
    const std::string dir = argv[1], path = dir + "/a.counts", cut = dir + "/cut.counts";
    CountsFileMeta m;
    m.chrom = "chr11"; m.rg_s = 5246595; m.rg_e = 5248428; m.n_positions = 9; m.mapq = 10; m.slots = 1; m.depth_groups = 2; m.n_quals = 40;
    const int32_t positions[9] = {1, 2, 3, 5, 8, 13, 21, 34, 55};
    m.pos_hash = counts_fnv1a64(positions, sizeof positions);
    m.groups = {"EAS", "EUR"};
    m.bam_paths = {"data/a.bam", "", "data/with space.bam"};
    m.bam_samples = {"S1", "S2", ""};
    expect(counts_fnv1a64("", 0) == 0xCBF29CE484222325ull && counts_fnv1a64("a", 1) == 0xAF63DC4C8601EC8Cull, "FNV-1a of the empty string and of 'a'");
    // three pieces: rows 0..3 with an empty row, rows 4..4 without an entry, rows 5..8 with the row's last cell
    std::vector<CountsPiece> want(3);
    want[0].t0 = 0; want[0].n = 4; want[0].row_start = {0, 2, 2, 3, 6}; want[0].cell = {0, 511, 7, 1, 512, 529}; want[0].count = {1, 0xFFFFFFFFu, 0x10000, 3, 0, 9};
    want[1].t0 = 4; want[1].n = 1; want[1].row_start = {0, 0};
    want[2].t0 = 5; want[2].n = 4; want[2].row_start = {0, 0, 0, 0, 1}; want[2].cell = {(uint16_t)(m.row_words() - 1)}; want[2].count = {77};
    std::string err;
    {
        CountsFileWriter w;
        bool ok = w.open(path, m, err);
        for (auto const &p : want) ok = ok && w.piece(p.t0, p.n, p.row_start.data(), p.cell.data(), p.count.data(), err);
        ok = ok && w.close(err);
        expect(ok && w.entries() == 7, "the writer: " + err);
    }
    CountsFileMeta got;
    std::vector<CountsPiece> pieces;
    expect(read_all(path, got, pieces, err) == 0, "the file reads back: " + err);
    expect(got.chrom == m.chrom && got.rg_s == m.rg_s && got.rg_e == m.rg_e && got.n_positions == m.n_positions && got.mapq == m.mapq && got.slots == m.slots &&
           got.depth_groups == m.depth_groups && got.n_quals == m.n_quals && got.pos_hash == m.pos_hash && got.groups == m.groups &&
           got.bam_paths == m.bam_paths && got.bam_samples == m.bam_samples, "the header round trip");
    expect(pieces.size() == want.size(), "the pieces' number");
    for (size_t i = 0; i < pieces.size() && i < want.size(); ++i)
        expect(pieces[i].t0 == want[i].t0 && pieces[i].n == want[i].n && pieces[i].row_start == want[i].row_start && pieces[i].cell == want[i].cell &&
               pieces[i].count == want[i].count, "piece " + std::to_string(i));
    std::ifstream in(path.c_str(), std::ios::binary);
    const std::string bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    // the file cut at every length: refused, with one line that names the file
    for (size_t n = 0; n < bytes.size(); ++n) {
        write_bytes(cut, bytes, n);
        err.clear();
        const int rc = read_all(cut, got, pieces, err);
        expect(rc == 1 && err.compare(0, cut.size() + 2, cut + ": ") == 0 && err.find('\n') == std::string::npos, "cut at " + std::to_string(n) + ": " + err);
    }
    // a byte more behind the end mark, and bytes changed where the reader must notice
    write_bytes(cut, bytes + "x", bytes.size() + 1);
    expect(read_all(cut, got, pieces, err) == 1, "a byte behind the end mark");
    const size_t end_mark = bytes.size() - 16;
    for (size_t at : {(size_t)0, (size_t)8, (size_t)12, (size_t)16, end_mark, end_mark + 4, end_mark + 8}) {
        std::string bad = bytes;
        bad[at] = (char)(bad[at] ^ 0x41);
        write_bytes(cut, bad, bad.size());
        err.clear();
        expect(read_all(cut, got, pieces, err) == 1 && !err.empty(), "byte " + std::to_string(at) + " changed");
    }
    // a missing file
    expect(read_all(dir + "/none.counts", got, pieces, err) == 1, "a file that does not exist");
    std::remove(path.c_str());
    std::remove(cut.c_str());
    std::cout << checks << " checks, " << wrong << " wrong" << std::endl;
    return wrong ? 1 : 0;
}
