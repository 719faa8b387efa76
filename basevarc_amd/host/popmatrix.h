// popmatrix.h -- `BaseVarC popmatrix` and `BaseVarC concat` on the CPU (no GPU code): the position file, a BAM's row of the population
// matrix and the concatenation of matrix files.  Counterparts in the reference: runPopMatrix / runConcat (src/BaseVarC.cpp:671-795),
// PosInfo's operator>> and operator+ (src/BamProcess.h:8-27), BamProcess::GetBRV + FetchAlleleType (src/BamProcess.cpp:96-198, 264-304).
#ifndef BVC_HOST_POPMATRIX_H
#define BVC_HOST_POPMATRIX_H

#include <cstdint>
#include <string>
#include <vector>

#include "bam.h"

namespace bvchost {

// Every line the reference's `for (PosInfo p; ipos >> p;)` reads: whitespace-separated chr, int pos, one non-blank character each for
// REF and ALT; the first thing that does not parse ends the list.  False: the file does not open.
bool read_posfile(const std::string &path, std::vector<PosInfo> &pv);
// pv.front() + pv.back(): "chr:first-last" (the last line's chr).
std::string posfile_region(const std::vector<PosInfo> &pv);
// No position is smaller than the one before it (repeats allowed): what the device path needs.
bool positions_do_not_descend(const std::vector<PosInfo> &pv);

// One BAM's row (without the newline): GetBRV's checks in its order -- sorted, SM -- then the region's reads ([beg0, end0), mapq) and
// fetch_allele_type.  A contig that is not in the header prints "<sm>: region <rg> is empty." on stderr and gives a row of '.'.
std::string popmatrix_row(const std::string &bam, const std::string &chr, const std::string &rg, int32_t beg0, int32_t end0, int mapq, int32_t rg_s,
                          const std::string &refseq, const std::vector<PosInfo> &pv);

// runConcat's body: the header lines of the files listed in `list` (all N must agree), "N\t(sum of M)\n", then N times line i of every
// file in list order.  Written as BGZF to `out`, opened as given.  Throws the reference's errors.
void concat_matrices(const std::string &list, const std::string &out);

}  // namespace bvchost
#endif
