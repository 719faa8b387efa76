// bam.h -- BAM records, region fetch and the per-sample pileup rule (host side, f4).
// Counterparts in the reference: BamProcess::GetBRV / FindSnpAtPos / GetAllele / GetOffset
// (src/BamProcess.cpp:4-94, 214-304) and RefReader::GetTargetBase (src/RefReader.h:17-33), which sit on
// SeqLib + htslib there (both absent from the reference tree).  BAM/BAI/faidx are implemented from the
// SAM specification; the pileup rule follows the reference's source text.
#ifndef BVC_HOST_BAM_H
#define BVC_HOST_BAM_H

#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "pileup.h"

namespace bvchost {

struct BamRecord {
    int32_t ref_id = -1;
    int32_t pos = 0;                    // 0-based leftmost
    uint8_t mapq = 0;
    uint16_t flag = 0;
    std::vector<std::pair<char, int32_t>> cigar;
    std::string seq;
    std::string qual;                   // raw phred values (not +33)
    int32_t end_pos() const;            // 0-based exclusive = 1-based inclusive (bam_endpos)
    bool reverse() const { return flag & 0x10; }
    bool mate_reverse() const { return flag & 0x20; }
    bool duplicate() const { return flag & 0x400; }
};

class BamFile {
 public:
    bool open(const std::string &path);
    const std::string &header_text() const { return header_; }
    std::string sample_name() const;                         // first "SM:" of the header, src/BamProcess.cpp:273-287
    bool sorted() const { return header_.find("SO:coord") != std::string::npos; }
    int ref_index(const std::string &name) const;
    // Records overlapping [beg, end) of reference `rid` (0-based), duplicates and MAPQ < mapq dropped
    // (src/BamProcess.cpp:295-300).  Uses the .bai linear index when present, else scans the file.
    bool fetch(int rid, int32_t beg, int32_t end, int min_mapq, std::vector<BamRecord> &out);
    const std::string &path() const { return path_; }
    uint64_t first_record() const { return first_record_; }   // virtual offset of the first alignment record
 private:
    std::string path_, header_;
    std::vector<std::string> ref_names_;
    uint64_t first_record_ = 0;
};

// Smallest virtual offset of an alignment overlapping the 16 kbp window of `beg` (.bai linear index); false: no index, no such
// reference, an empty slot.  clamp: a window past the index takes the last one (fetch's start); else it is "not found"
bool bai_linear_offset(const std::string &bam_path, int rid, int32_t beg, uint64_t &voff, bool clamp = true);

typedef std::unordered_map<int32_t, AlleleInfo> PosAlleleMap;   // src/BamProcess.h:40
// BamProcess::FindSnpAtPos (src/BamProcess.cpp:4-94): first usable read per position.
void find_snp_at_pos(const std::vector<BamRecord> &rv, int32_t rg_s, const std::string &refseq,
                     const std::vector<int32_t> &pv, PosAlleleMap &allele_m);

// A line of a position file <CHR POS REF ALT> (src/BamProcess.h:8-27).
struct PosInfo {
    std::string chr;
    int32_t pos = 0;
    char ref = 0, alt = 0;
};
// BamProcess::FetchAlleleType + GetSnpCode (src/BamProcess.cpp:96-212) behind GetBRV: one character per line of pv -- '0' the first usable
// read's base is the line's REF, '1' its ALT, '.' anything else.  Follows the reference's text statement by statement, the read cursor
// kept across positions included, so a position file that is not sorted gets the reference's answer too.  Departure: no read at all is
// a row of '.' (the reference indexes an empty vector).  Throws std::out_of_range where the reference does.
std::string fetch_allele_type(const std::vector<BamRecord> &rv, int32_t rg_s, const std::string &refseq, const std::vector<PosInfo> &pv);

// RefReader::GetTargetBase: 1-based inclusive region of a faidx-indexed FASTA (plain or BGZF + .gzi),
// upper-cased.
bool fetch_reference(const std::string &fasta, const std::string &chr, int32_t start1, int32_t end1, std::string &seq,
                     std::string &err);

}  // namespace bvchost
#endif
