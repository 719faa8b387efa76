#include "bam_blocks.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

namespace bvchost {

MappedFile::MappedFile(const std::string &path)
{
    fd_ = ::open(path.c_str(), O_RDONLY);
    if (fd_ < 0) return;
    struct stat st;
    if (::fstat(fd_, &st) != 0 || st.st_size <= 0) return;
    void *p = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd_, 0);
    if (p == MAP_FAILED) return;
    p_ = static_cast<const unsigned char *>(p);
    n_ = (size_t)st.st_size;
}

MappedFile::~MappedFile()
{
    if (p_) ::munmap(const_cast<unsigned char *>(p_), n_);
    if (fd_ >= 0) ::close(fd_);
}

namespace {

// The frame of the block at file offset `at`: false at the end of the file or on a damaged frame (bad set).
bool frame_at(const MappedFile &f, uint64_t at, size_t &bsize, RawBlock &blk, bool &bad)
{
    bad = false;
    if (at >= f.size()) return false;
    bad = true;
    if (f.size() - at < 18) return false;
    bsize = bgzf_block_size(f.data() + at);
    if (bsize == 0 || bsize < 26 || bsize > f.size() - at) return false;
    // (the extra field of a BGZF block is its one 'BC' subfield: the payload begins 18 bytes in)
    if (!bgzf_block_trailer(f.data() + at + bsize - 8, blk.crc32, blk.isize)) return false;
    blk.payload = f.data() + at + 18;
    blk.len = bsize - 26;
    bad = false;
    return true;
}

}  // namespace

bool bam_region_blocks(const MappedFile &f, const std::string &bam_path, uint64_t first_record, int rid, int32_t beg0, int32_t end0, bool to_eof,
                       BamBlocks &out, std::string &err)
{
    out = BamBlocks();
    out.to_eof = true;
    // where fetch seeks to: the index's offset when it names a block of this file and a place inside it, else the first record
    uint64_t start = first_record, voff = 0;
    size_t bsize = 0;
    RawBlock blk;
    bool bad = false;
    if (bai_linear_offset(bam_path, rid, beg0, voff) && frame_at(f, voff >> 16, bsize, blk, bad) && (voff & 0xffff) <= blk.isize) start = voff;
    // where to stop: the block of the first alignment that overlaps the window behind end0's, and one more
    uint64_t stop_at = UINT64_MAX;
    const int32_t w_end = (end0 < 0 ? 0 : end0) >> 14;
    if (!to_eof && w_end < (INT32_MAX >> 14) && bai_linear_offset(bam_path, rid, (w_end + 1) << 14, voff, false) && (voff >> 16) >= (start >> 16))
        stop_at = voff >> 16;
    out.first_off = (uint32_t)(start & 0xffff);
    int past_stop = 0;
    for (uint64_t at = start >> 16;;) {
        if (!frame_at(f, at, bsize, blk, bad)) {
            if (bad) { err = "ERROR: truncated or corrupt BAM record in " + bam_path; return false; }
            break;
        }
        if (at > stop_at && ++past_stop > 1) { out.to_eof = false; break; }
        if (blk.isize > 0 || out.blocks.empty()) {  // (the first block stays even when empty: first_off is an offset into it)
            out.blocks.push_back(blk);
            out.comp_bytes += blk.len;
            out.out_bytes += blk.isize;
        }
        at += bsize;
    }
    if (!out.blocks.empty() && out.first_off > out.blocks[0].isize) out.first_off = out.blocks[0].isize;
    return true;
}

std::vector<size_t> window_cuts(size_t psize, int thread)
{
    const size_t window = psize % (size_t)thread + psize / (size_t)thread;
    std::vector<size_t> cuts((size_t)thread, psize);
    for (int j = 0; j + 1 < thread; ++j) cuts[(size_t)j] = std::min(psize, (size_t)(j + 1) * window);
    return cuts;
}

}  // namespace bvchost
