// host_tiles_main.cpp -- the host program's BGZF block walk (MappedBlocks, host/bgzf.cpp) and its tile packers (pack_ragged, pack_dense,
// host/pileup.h) for a build with -fsanitize=address,undefined (tests/test_host.py writes the inputs, builds this program and runs
// it as a child process, and compares what it prints with its own walk and its numpy model).
//
// usage: host_tiles tiles.bin [block file ...]
// Per block file one line: "walk <n>:" and per block " <payload offset>,<payload bytes>,<ISIZE>,<CRC32>,<sum of the payload's bytes>",
// or "walk refused: <what>".
// tiles.bin: u32 tiles, then per tile  u32 dense, u32 two_byte_only, u32 sites, per site (u32 entries, entries x 8 bytes as
// bvc_pileup_entry, entries x i32 sample), and for a dense tile  u32 samples, samples x u8 group of the sample, u32 stride.
// Per tile one line: "tile fits=<0|1> offsets=<,-separated> a=<hex> b=<hex>" (a: packed or bases, b: quals; a dense tile has no offsets).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "bgzf.h"
#include "pileup.h"

using namespace bvchost;

static uint32_t read_u32(FILE *f)
{
    uint32_t v = 0;
    if (std::fread(&v, 4, 1, f) != 1) { std::fprintf(stderr, "tiles.bin ends early\n"); std::exit(2); }
    return v;
}

template <class V>
static void print_hex(const char *name, const V &v, size_t n)
{
    std::printf(" %s=", name);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", (unsigned)(uint8_t)v[i]);
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s tiles.bin [block file ...]\n", argv[0]); return 2; }
    for (int i = 2; i < argc; ++i) {
        try {
            MappedBlocks m(std::vector<std::string>(1, argv[i]));
            std::string blocks;
            RawBlock rb;
            int n = 0;
            for (; m.pop(0, rb); ++n) {
                unsigned sum = 0;                                    // every byte of the payload is read
                for (size_t k = 0; k < rb.len; ++k) sum += rb.payload[k];
                char one[96];
                std::snprintf(one, sizeof one, " %ld,%zu,%u,%u,%u", (long)(rb.payload - m.data(0)), rb.len, rb.isize, rb.crc32, sum);
                blocks += one;
            }
            std::printf("walk %d:%s\n", n, blocks.c_str());
        } catch (const std::exception &e) {
            std::printf("walk refused: %s\n", e.what());
        }
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const uint32_t n_tiles = read_u32(f);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t dense = read_u32(f), two_byte_only = read_u32(f), n_sites = read_u32(f);
        std::vector<SiteColumn> sites(n_sites);
        for (auto &site : sites) {
            const uint32_t n = read_u32(f);
            std::vector<bvc_pileup_entry> e(n);
            std::vector<int32_t> sample(n);
            if (n && (std::fread(e.data(), sizeof e[0], n, f) != n || std::fread(sample.data(), 4, n, f) != n)) return 2;
            for (uint32_t k = 0; k < n; ++k) {
                AlleleInfo a;
                a.base = e[k].base; a.mapq = e[k].mapq; a.qual = e[k].qual; a.rpr = e[k].rpr; a.strand = e[k].strand; a.is_indel = e[k].is_indel;
                site.add(a, sample[k]);
            }
        }
        PackedTile p;
        bool fits;
        size_t n_obs;
        if (dense) {
            Groups g;
            g.of_sample.resize(read_u32(f));
            if (std::fread(g.of_sample.data(), 1, g.of_sample.size(), f) != g.of_sample.size()) return 2;
            g.order_columns();
            const uint32_t stride = read_u32(f);
            fits = pack_dense(sites.data(), sites.size(), stride, g.column_of.data(), two_byte_only != 0, p);
            n_obs = (size_t)n_sites * stride;
        } else {
            fits = pack_ragged(sites.data(), sites.size(), two_byte_only != 0, p);
            n_obs = (size_t)p.offsets.back();
        }
        std::printf("tile fits=%d offsets=", fits ? 1 : 0);
        for (size_t i = 0; i < p.offsets.size(); ++i) std::printf(i ? ",%ld" : "%ld", (long)p.offsets[i]);      // (none of a dense tile)
        if (fits) { print_hex("a", p.packed, n_obs); std::printf(" b="); }
        else { print_hex("a", p.bases, n_obs); print_hex("b", p.quals, n_obs); }
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
