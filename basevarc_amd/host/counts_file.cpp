// counts_file.cpp -- the writer and the reader of the counts files (counts_file.h; docs/COUNTS_FILES.md).
#include "counts_file.h"

#include <cstring>

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "the counts file is little-endian and is written from memory as it lies"
#endif

namespace {

const char kMagic[8] = {'B', 'V', 'C', 'C', 'N', 'T', 'S', '\0'};
const uint32_t kVersion = 1, kTagPiece = 0x43454950u, kTagEnd = 0x21444E45u;      // "PIEC", "END!"
const uint32_t kMaxString = 1u << 20;

}  // namespace

uint64_t counts_fnv1a64(const void *data, size_t n)
{
    const unsigned char *p = static_cast<const unsigned char *>(data);
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

// ---- the writer ------------------------------------------------------------------------------------------------------------------------
CountsFileWriter::~CountsFileWriter() { if (f_) std::fclose(f_); }

bool CountsFileWriter::put(const void *p, size_t n, std::string &err)
{
    if (n && std::fwrite(p, 1, n, f_) != n) { err = path_ + ": fail to write the counts file"; return false; }
    bytes_ += (int64_t)n;
    return true;
}

bool CountsFileWriter::open(const std::string &path, const CountsFileMeta &m, std::string &err)
{
    path_ = path;
    f_ = std::fopen(path.c_str(), "wb");
    if (!f_) { err = path + ": can not open the counts file for writing"; return false; }
    auto str = [&](const std::string &s) { const uint32_t n = (uint32_t)s.size(); return put(&n, 4, err) && put(s.data(), s.size(), err); };
    const uint32_t head[4] = {kVersion, m.slots, m.depth_groups, m.n_quals};
    const int32_t ints[4] = {m.mapq, m.rg_s, m.rg_e, m.n_positions};
    if (!put(kMagic, 8, err) || !put(head, 16, err) || !put(ints, 16, err) || !put(&m.pos_hash, 8, err) || !str(m.chrom)) return false;
    uint32_t k = (uint32_t)m.groups.size();
    if (!put(&k, 4, err)) return false;
    for (auto const &g : m.groups) if (!str(g)) return false;
    k = (uint32_t)m.bam_paths.size();
    if (!put(&k, 4, err)) return false;
    for (size_t i = 0; i < m.bam_paths.size(); ++i) if (!str(m.bam_paths[i]) || !str(m.bam_samples[i])) return false;
    return true;
}

bool CountsFileWriter::piece(int32_t t0, int32_t n, const int64_t *row_start, const uint16_t *cell, const uint32_t *count, std::string &err)
{
    const int64_t ne = row_start[n];
    const int32_t rows[2] = {t0, n};
    if (!put(&kTagPiece, 4, err) || !put(rows, 8, err) || !put(&ne, 8, err) || !put(row_start, ((size_t)n + 1) * 8, err) ||
        !put(cell, (size_t)ne * 2, err) || !put(count, (size_t)ne * 4, err))
        return false;
    entries_ += ne;
    ++pieces_;
    return true;
}

bool CountsFileWriter::close(std::string &err)
{
    bool ok = put(&kTagEnd, 4, err) && put(&pieces_, 4, err) && put(&entries_, 8, err);
    if (std::fclose(f_) != 0 && ok) { err = path_ + ": fail to write the counts file"; ok = false; }
    f_ = nullptr;
    return ok;
}

// ---- the reader ------------------------------------------------------------------------------------------------------------------------
CountsFileReader::~CountsFileReader() { if (f_) std::fclose(f_); }

bool CountsFileReader::get(void *p, size_t n, const char *field, std::string &err)
{
    if ((int64_t)n > size_ - at_ || (n && std::fread(p, 1, n, f_) != n)) {
        err = path_ + ": the counts file is truncated (" + field + ")";
        return false;
    }
    at_ += (int64_t)n;
    return true;
}

bool CountsFileReader::get_string(std::string &s, const char *field, std::string &err)
{
    uint32_t n = 0;
    if (!get(&n, 4, field, err)) return false;
    if (n > kMaxString) { err = path_ + ": the counts file is damaged (" + field + ": a string of " + std::to_string(n) + " bytes)"; return false; }
    s.resize(n);
    return get(n ? &s[0] : nullptr, n, field, err);
}

bool CountsFileReader::open(const std::string &path, CountsFileMeta &m, std::string &err)
{
    path_ = path;
    f_ = std::fopen(path.c_str(), "rb");
    if (!f_) { err = path + ": can not open the counts file"; return false; }
    if (std::fseek(f_, 0, SEEK_END) != 0 || (size_ = (int64_t)std::ftell(f_)) < 0 || std::fseek(f_, 0, SEEK_SET) != 0) {
        err = path + ": can not read the counts file";
        return false;
    }
    char magic[8];
    uint32_t head[4];
    int32_t ints[4];
    if (!get(magic, 8, "magic", err)) return false;
    if (std::memcmp(magic, kMagic, 8) != 0) { err = path + ": not a counts file (magic)"; return false; }
    if (!get(head, 16, "version", err)) return false;
    if (head[0] != kVersion) { err = path + ": a counts file of version " + std::to_string(head[0]) + ", this program reads version 1"; return false; }
    if (!get(ints, 16, "region", err) || !get(&m.pos_hash, 8, "positions hash", err) || !get_string(m.chrom, "chromosome", err)) return false;
    m.slots = head[1]; m.depth_groups = head[2]; m.n_quals = head[3];
    m.mapq = ints[0]; m.rg_s = ints[1]; m.rg_e = ints[2]; m.n_positions = ints[3];
    if (m.slots < 1 || m.slots > 33 || m.depth_groups > 32 || m.n_positions < 0) { err = path + ": the counts file is damaged (slots, depth_groups or n_positions)"; return false; }
    uint32_t k = 0;
    if (!get(&k, 4, "group names", err)) return false;
    if (k > 32) { err = path + ": the counts file is damaged (group names)"; return false; }
    m.groups.resize(k);
    for (auto &g : m.groups) if (!get_string(g, "group names", err)) return false;
    if (!get(&k, 4, "BAM list", err)) return false;
    if ((int64_t)k * 8 > size_ - at_) { err = path + ": the counts file is truncated (BAM list)"; return false; }
    m.bam_paths.resize(k); m.bam_samples.resize(k);
    for (uint32_t i = 0; i < k; ++i) if (!get_string(m.bam_paths[i], "BAM list", err) || !get_string(m.bam_samples[i], "BAM list", err)) return false;
    row_words_ = m.row_words();
    n_positions_ = m.n_positions;
    return true;
}

int CountsFileReader::next(CountsPiece &p, std::string &err)
{
    uint32_t tag = 0;
    if (!get(&tag, 4, "piece or end mark", err)) return -1;
    if (tag == kTagEnd) {
        uint32_t pieces = 0;
        int64_t total = 0;
        if (!get(&pieces, 4, "end mark", err) || !get(&total, 8, "end mark", err)) return -1;
        if (pieces != pieces_ || total != entries_ || at_ != size_) { err = path_ + ": the counts file is damaged (end mark)"; return -1; }
        return 0;
    }
    if (tag != kTagPiece) { err = path_ + ": the counts file is damaged (piece tag)"; return -1; }
    int32_t rows[2];
    int64_t ne = 0;
    if (!get(rows, 8, "piece header", err) || !get(&ne, 8, "piece header", err)) return -1;
    p.t0 = rows[0]; p.n = rows[1];
    if (p.t0 < 0 || p.n < 0 || p.n > n_positions_ - p.t0 || ne < 0) { err = path_ + ": the counts file is damaged (piece header)"; return -1; }
    // (the sizes are held against the bytes the file still has before anything is allocated)
    if (((int64_t)p.n + 1) * 8 > size_ - at_ || ne > (size_ - at_) / 6) { err = path_ + ": the counts file is truncated (piece)"; return -1; }
    p.row_start.resize((size_t)p.n + 1); p.cell.resize((size_t)ne); p.count.resize((size_t)ne);
    if (!get(p.row_start.data(), p.row_start.size() * 8, "row_start", err) || !get(p.cell.data(), p.cell.size() * 2, "cell", err) ||
        !get(p.count.data(), p.count.size() * 4, "count", err))
        return -1;
    bool ok = p.row_start[0] == 0 && p.row_start[(size_t)p.n] == ne;
    for (int32_t t = 0; t < p.n && ok; ++t) ok = p.row_start[(size_t)t + 1] >= p.row_start[(size_t)t];
    for (size_t i = 0; i < p.cell.size() && ok; ++i) ok = p.cell[i] < row_words_;
    if (!ok) { err = path_ + ": the counts file is damaged (piece: row_start or a cell)"; return -1; }
    entries_ += ne;
    ++pieces_;
    return 1;
}
