// bam_blocks.h -- the BGZF blocks of a BAM file that hold a region's alignments, as they lie in the file: what phase 1 gathers for the
// device (BVC_HOST_DEVICE_PILEUP; bvc_bam_pileup_bgzf inflates them and piles the records up).  No GPU code here.
#ifndef BVC_HOST_BAM_BLOCKS_H
#define BVC_HOST_BAM_BLOCKS_H

#include <cstdint>
#include <string>
#include <vector>

#include "bam.h"
#include "bgzf.h"

namespace bvchost {

// A file mapped read-only for as long as the object lives.
class MappedFile {
 public:
    explicit MappedFile(const std::string &path);            // ok() is false when the file cannot be opened or mapped
    ~MappedFile();
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
    bool ok() const { return p_ != nullptr; }
    const unsigned char *data() const { return p_; }
    size_t size() const { return n_; }
 private:
    const unsigned char *p_ = nullptr;
    size_t n_ = 0;
    int fd_ = -1;
};

// The blocks of one sample for one region.
struct BamBlocks {
    std::vector<RawBlock> blocks;      // non-empty blocks in file order; the payloads point into the mapped file
    uint32_t first_off = 0;            // offset of the first record inside the first block's inflated bytes
    bool to_eof = false;               // the list runs to the file's end
    uint64_t comp_bytes = 0, out_bytes = 0;
};

// The blocks from the one BamFile::fetch would seek to -- the .bai linear index's offset for `beg0`, else the file's first record
// (first_record: its virtual offset) -- up to and including the block the linear index names for the window behind `end0` and one more
// (a record may straddle), when the index has such a window and to_eof is not asked for; else to the file's end.  A list that stops short
// may end before the region's last record: the device call then reports that the bytes ran out and the caller asks again with to_eof.
// False: a damaged BGZF frame (err says which).
bool bam_region_blocks(const MappedFile &f, const std::string &bam_path, uint64_t first_record, int rid, int32_t beg0, int32_t end0, bool to_eof,
                       BamBlocks &out, std::string &err);

// Where the threads' windows of positions begin: record i of psize goes to file j while i < cuts[j] (cuts[thread - 1] = psize), the
// rule of bt_r's loop (`i == (j + 1) * window`, window = psize % thread + psize / thread).
std::vector<size_t> window_cuts(size_t psize, int thread);

}  // namespace bvchost
#endif
