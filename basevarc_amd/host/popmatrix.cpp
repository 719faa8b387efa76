#include "popmatrix.h"

#include <deque>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "bgzf.h"

namespace bvchost {

bool read_posfile(const std::string &path, std::vector<PosInfo> &pv)
{
    std::ifstream ipos(path);
    if (!ipos.is_open()) return false;
    for (PosInfo p; ipos >> std::ws >> p.chr >> p.pos >> p.ref >> p.alt;) pv.push_back(p);   // src/BamProcess.h:23-26
    pv.shrink_to_fit();
    return true;
}

std::string posfile_region(const std::vector<PosInfo> &pv)
{
    return pv.back().chr + ":" + std::to_string(pv.front().pos) + "-" + std::to_string(pv.back().pos);
}

bool positions_do_not_descend(const std::vector<PosInfo> &pv)
{
    for (size_t i = 1; i < pv.size(); ++i)
        if (pv[i].pos < pv[i - 1].pos) return false;
    return true;
}

std::string popmatrix_row(const std::string &bam, const std::string &chr, const std::string &rg, int32_t beg0, int32_t end0, int mapq, int32_t rg_s,
                          const std::string &refseq, const std::vector<PosInfo> &pv)
{
    BamFile reader;
    if (!reader.open(bam)) throw std::runtime_error("ERROR: cannot open bam " + bam);
    if (!reader.sorted())
        throw std::runtime_error("ERROR: BAM file does not appear to be sorted (no SO:coordinate) found in header.\n       Sorted BAMs are required.");
    const std::string sm = reader.sample_name();
    const int rid = reader.ref_index(chr);
    if (rid < 0) {
        std::cerr << sm << ": region " << rg << " is empty." << std::endl;
        return std::string(pv.size(), '.');
    }
    std::vector<BamRecord> rv;
    reader.fetch(rid, beg0, end0, mapq, rv);
    return fetch_allele_type(rv, rg_s, refseq, pv);
}

void concat_matrices(const std::string &list, const std::string &out)
{
    std::vector<std::string> fm_v;
    { std::ifstream ifm(list); std::string l; while (std::getline(ifm, l)) fm_v.push_back(l); }
    BgzfWriter fpo(out);
    if (!fpo.ok()) throw std::runtime_error("ERROR: fail to write");
    long n = 0, mt = 0;
    std::deque<BgzfReader> fpv;                     // (a reader owns its file and does not move)
    std::string line;
    for (auto const &fm : fm_v) {
        fpv.emplace_back(fm);
        // (htslib would also read a plain gzip file; this reader takes BGZF, which is what popmatrix writes)
        if (!fpv.back().ok() || !fpv.back().is_bgzf()) throw std::runtime_error("ERROR: cannot open " + fm + " as a BGZF matrix file");
        if (fpv.back().getline(line)) {
            std::vector<std::string> tokens;
            std::istringstream ts(line);
            for (std::string token; std::getline(ts, token, '\t');) tokens.push_back(token);
            if (tokens.size() < 2) throw std::runtime_error("ERROR: no header line <N M> in " + fm);
            if (n > 0 && n != std::stol(tokens[0])) throw std::runtime_error("ERROR: the number of samples among the inputs are different!");
            n = std::stol(tokens[0]);
            mt += std::stol(tokens[1]);
        }
    }
    fpo.write(std::to_string(n) + "\t" + std::to_string(mt) + "\n");
    std::string ss;
    for (long i = 0; i < n; ++i) {
        if (i % 1000 == 0 && i != 0) std::cout << "reading the " << i << " samples" << std::endl;
        ss.clear();
        ss.reserve((size_t)mt + 1);
        for (size_t k = 0; k < fm_v.size(); ++k) {
            if (!fpv[k].getline(line)) throw std::runtime_error("ERROR: empty in the " + std::to_string(i) + " line of " + fm_v[k]);
            ss += line;
        }
        ss += "\n";
        fpo.write(ss);
    }
    if (!fpo.close()) std::cerr << "warning: fail to close file" << std::endl;
}

}  // namespace bvchost
