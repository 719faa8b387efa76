// bam_blocks_main.cpp -- host/bam_blocks.cpp (the block gathering and the window cutting of phase 1's device path) over BAM files, for a
// build with -fsanitize=address,undefined (tests/test_bam_pileup_abi.py builds this program and runs it on the test BAMs and on damaged
// copies).  Per file: the block list with and without "to the file's end", every block inflated with zlib into a heap block of exactly
// ISIZE bytes and held to its CRC32, and the record chain walked from first_off -- it must start at a record and, for a list that runs
// to the file's end, end exactly with the bytes.  Usage: bam_blocks_main <contig> <beg0> <end0> <file>...   Files whose name ends in
// ".bad" must be refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <zlib.h>

#include "bam_blocks.h"

using namespace bvchost;

static bool inflate_list(const BamBlocks &l, std::vector<unsigned char> &out)
{
    out.clear();
    for (auto const &b : l.blocks) {
        std::unique_ptr<unsigned char[]> comp(new unsigned char[b.len ? b.len : 1]), plain(new unsigned char[b.isize ? b.isize : 1]);
        std::memcpy(comp.get(), b.payload, b.len);
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        zs.next_in = comp.get(); zs.avail_in = (uInt)b.len;
        zs.next_out = plain.get(); zs.avail_out = (uInt)b.isize;
        const int rc = inflate(&zs, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && zs.total_out == b.isize;
        inflateEnd(&zs);
        if (!ok || bgzf_crc32(plain.get(), b.isize) != b.crc32) return false;
        out.insert(out.end(), plain.get(), plain.get() + b.isize);
    }
    return true;
}

// records from `at` on: how many whole ones, and whether the chain ends exactly with the bytes
static long walk(const std::vector<unsigned char> &d, size_t at, bool &exact)
{
    long n = 0;
    exact = false;
    for (;;) {
        if (at == d.size()) { exact = true; return n; }
        if (d.size() - at < 4) return n;
        const uint32_t bs = le32u(d.data() + at);
        if (bs < 32 || bs > (1u << 28) || d.size() - at - 4 < bs) return n;
        at += 4 + (size_t)bs;
        ++n;
    }
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const std::string contig = argv[1];
    const int32_t beg0 = std::atoi(argv[2]), end0 = std::atoi(argv[3]);
    int wrong = 0, files = 0;
    for (int i = 4; i < argc; ++i, ++files) {
        const std::string path = argv[i];
        const bool must_fail = path.size() > 4 && path.substr(path.size() - 4) == ".bad";
        BamFile bam;
        MappedFile f(path);
        bool failed = !f.ok() || !bam.open(path);
        long n_short = -1, n_all = -1;
        if (!failed) {
            const int rid = bam.ref_index(contig);
            for (int to_eof = 0; to_eof < 2 && !failed; ++to_eof) {
                BamBlocks l;
                std::string err;
                std::vector<unsigned char> plain;
                if (!bam_region_blocks(f, path, bam.first_record(), rid, beg0, end0, to_eof != 0, l, err) || !inflate_list(l, plain)) { failed = true; break; }
                bool exact = false;
                if (l.first_off > plain.size()) { failed = true; break; }
                const long n = walk(plain, l.first_off, exact);
                if (l.to_eof && !exact) failed = true;
                if (to_eof && !l.to_eof) failed = true;
                (to_eof ? n_all : n_short) = n;
            }
            if (!failed && (n_short > n_all || n_all < 1)) failed = true;
        }
        if (failed != must_fail) {
            ++wrong;
            std::printf("%s: %s\n", path.c_str(), failed ? "refused" : "accepted");
        }
    }
    // the window cuts against bt_r's loop
    for (size_t psize = 0; psize < 40; ++psize)
        for (int thread = 1; thread < 9; ++thread) {
            const std::vector<size_t> cuts = window_cuts(psize, thread);
            const size_t window = psize % (size_t)thread + psize / (size_t)thread;
            for (size_t p = 0, j = 0; p < psize; ++p) {
                if (p == (j + 1) * window && j + 1 < (size_t)thread) ++j;
                size_t k = 0;
                while (p >= cuts[k]) ++k;
                if (k != j) { ++wrong; std::printf("cuts: psize %zu thread %d position %zu\n", psize, thread, p); break; }
            }
            if (cuts.back() != psize) ++wrong;
        }
    std::printf("%d files, %d wrong\n", files, wrong);
    return wrong ? 1 : 0;
}
