// counts_file.h -- the counts files of --tmp-format counts (BVC_HOST_COUNTS_SAVE / BVC_HOST_COUNTS_LOAD): an accumulator's rows as packed
// pieces (include/bvc_site_acc_pack.h) behind a header that records what the counts depend on.  The byte layout is docs/COUNTS_FILES.md's:
// little-endian, a magic and a version in front, an end mark with the totals behind, no compression.  No device code: the writer and the
// reader work on plain arrays (tests/cpp/counts_file_main.cpp, bvchost_counts_file_write / _read in capi.cpp).
#ifndef BVC_HOST_COUNTS_FILE_H
#define BVC_HOST_COUNTS_FILE_H

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct CountsFileMeta {
    std::string chrom;
    int32_t rg_s = 0, rg_e = 0, n_positions = 0;
    uint64_t pos_hash = 0;                          // counts_fnv1a64 of the positions as int32 words
    int32_t mapq = 0;                               // -q
    uint32_t slots = 1, depth_groups = 0;
    uint32_t n_quals = 128;                         // the writer's columns, for information only: the cells are logical
    std::vector<std::string> groups;                // the depth rows' group names (counts_group_map's sorted distinct names of the group file)
    std::vector<std::string> bam_paths, bam_samples;   // every BAM counted: its path as given in --input, its sample name
    uint32_t row_words() const { return slots * 512u + 10u + 4u * depth_groups; }
};

struct CountsPiece {
    int32_t t0 = 0, n = 0;
    std::vector<int64_t> row_start;                 // [n + 1]
    std::vector<uint16_t> cell;
    std::vector<uint32_t> count;
};

// 64-bit FNV-1a
uint64_t counts_fnv1a64(const void *data, size_t n);

// Every call returns false with one line in err ("<path>: ...") where it fails; nothing else may be called on the object then.
class CountsFileWriter {
public:
    CountsFileWriter() = default;
    CountsFileWriter(const CountsFileWriter &) = delete;
    CountsFileWriter &operator=(const CountsFileWriter &) = delete;
    ~CountsFileWriter();
    bool open(const std::string &path, const CountsFileMeta &meta, std::string &err);
    bool piece(int32_t t0, int32_t n, const int64_t *row_start, const uint16_t *cell, const uint32_t *count, std::string &err);
    bool close(std::string &err);                   // the end mark; the file is complete only after this
    int64_t bytes() const { return bytes_; }
    int64_t entries() const { return entries_; }
private:
    bool put(const void *p, size_t n, std::string &err);
    std::string path_;
    FILE *f_ = nullptr;
    int64_t bytes_ = 0, entries_ = 0;
    uint32_t pieces_ = 0;
};

class CountsFileReader {
public:
    CountsFileReader() = default;
    CountsFileReader(const CountsFileReader &) = delete;
    CountsFileReader &operator=(const CountsFileReader &) = delete;
    ~CountsFileReader();
    // the header: magic, version, the shape and what the counts depend on
    bool open(const std::string &path, CountsFileMeta &meta, std::string &err);
    // 1: a piece (checked: its rows inside the positions, row_start from 0 to its entries and never decreasing, every cell < W);
    // 0: the end mark, with the totals it must hold and nothing behind it; -1: truncated or damaged, one line in err
    int next(CountsPiece &piece, std::string &err);
    int64_t bytes() const { return size_; }
    int64_t entries() const { return entries_; }
private:
    bool get(void *p, size_t n, const char *field, std::string &err);
    bool get_string(std::string &s, const char *field, std::string &err);
    std::string path_;
    FILE *f_ = nullptr;
    int64_t size_ = 0, at_ = 0, entries_ = 0;
    uint32_t pieces_ = 0, row_words_ = 0;
    int32_t n_positions_ = 0;
};

#endif
