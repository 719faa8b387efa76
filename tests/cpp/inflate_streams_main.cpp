// inflate_streams_main.cpp -- host/inflate.cpp over a file of deflate streams, for a build with -fsanitize=address,undefined
// (tests/test_deflate_streams.py writes the file, builds this program and runs it as a child process).
//
// The file: u32 n, then n records of  u32 comp_len, u32 cap, u32 valid, comp_len bytes, and (valid only) cap bytes of expected output.
// Every stream is copied into a heap block of exactly comp_len bytes and inflated into one of exactly cap bytes, so that a read or a
// write one byte outside either is the sanitizer's to report.  A valid stream must give exactly its data, any other anything but
// `cap` bytes.  Exit status 0: all as expected.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate.h"

static bool read_u32(FILE *f, uint32_t &v) { return std::fread(&v, 4, 1, f) == 1; }

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t n = 0;
    if (!read_u32(f, n)) return 2;
    long wrong = 0;
    std::vector<unsigned char> want;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t comp_len, cap, valid;
        if (!read_u32(f, comp_len) || !read_u32(f, cap) || !read_u32(f, valid)) return 2;
        unsigned char *comp = static_cast<unsigned char *>(std::malloc(comp_len));
        unsigned char *out = static_cast<unsigned char *>(std::malloc(cap));
        if (comp_len && std::fread(comp, 1, comp_len, f) != comp_len) return 2;
        want.resize(valid ? cap : 0);
        if (valid && cap && std::fread(want.data(), 1, cap, f) != cap) return 2;
        const long r = bvchost::fast_inflate(comp, comp_len, out, cap);
        const bool ok = valid ? (r == (long)cap && (cap == 0 || std::memcmp(out, want.data(), cap) == 0)) : r != (long)cap;
        if (!ok) {
            ++wrong;
            std::printf("stream %u: %s, returned %ld for %u bytes of room\n", i, valid ? "valid" : "to be refused", r, cap);
        }
        std::free(comp);
        std::free(out);
    }
    std::fclose(f);
    std::printf("%u streams, %ld wrong\n", n, wrong);
    return wrong ? 1 : 0;
}
