// batches.h -- a thread's temp-batch files as the compute phase reads them on the CPU: either form, position by position for the CPU
// parser or a tile's share at a time for the device parser.  Calls nothing of libbvc.
#ifndef BVC_HOST_BATCHES_H
#define BVC_HOST_BATCHES_H

#include <chrono>
#include <cstring>
#include <stdexcept>

#include "bgzf.h"
#include "pileup.h"

namespace bvchost {

// BVC_HOST_PROFILE=1: where a phase-2 thread spends its time (seconds), printed when the thread ends
struct StageClock {
    double read = 0, parse = 0, pack = 0, gpu = 0, cvg = 0, vcf = 0, write = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};

// (a temp batch holds one line or record per position of the thread's window)
static const char *const kTruncatedBatch = "ERROR: truncated temp batch (it ends before the thread's window does)";

// One temp-batch file of a thread, in either form (detected from its first bytes).
struct BatchInput {
    BgzfReader rd;
    bool bin = false;
    uint32_t n_in_batch = 0;                   // binary form: samples of this batch (the text form counts tokens)
    std::string names;                         // first line without its newline: tab-terminated sample names
    std::vector<unsigned char> rec;

    explicit BatchInput(const std::string &path) : rd(path)
    {
        unsigned char head[16];
        const size_t got = rd.read(head, 8);
        if (got == 8 && std::memcmp(head, kBinBatchMagic, 8) == 0) {
            bin = true;
            if (rd.read(head, 8) != 8) throw std::runtime_error("ERROR: truncated temp batch " + path);
            n_in_batch = le32u(head);
            const uint32_t l = le32u(head + 4);
            names.resize(l);
            if (l && rd.read(&names[0], l) != l) throw std::runtime_error("ERROR: truncated temp batch " + path);
            if (!names.empty() && names.back() == '\n') names.pop_back();
        } else {                                // text form: start over and take the names line
            rd.seek(0);
            rd.getline(names);
        }
    }

    // The next position's entries of this batch; returns the number of samples the batch spans (the `j` advance).
    int32_t next(int32_t j0, SiteColumn &site, std::string &line, StageClock &clk)
    {
        double t0 = StageClock::now();
        if (bin) {
            unsigned char b4[4];
            if (rd.read(b4, 4) != 4) throw std::runtime_error(kTruncatedBatch);
            const uint32_t n = le32u(b4);
            rec.resize(n);
            if (n && rd.read(rec.data(), n) != n) throw std::runtime_error("ERROR: truncated temp batch record");
            double t1 = StageClock::now();
            clk.read += t1 - t0;
            if (!parse_pileup_bin(rec.data(), n, j0, site)) throw std::runtime_error("ERROR: malformed temp batch record");
            clk.parse += StageClock::now() - t1;
            return (int32_t)n_in_batch;
        }
        const bool got = rd.getline(line);
        if (!got) throw std::runtime_error(kTruncatedBatch);
        double t1 = StageClock::now();
        clk.read += t1 - t0;
        const int32_t adv = parse_pileup_line(line.data(), line.size(), j0, site);
        clk.parse += StageClock::now() - t1;
        return adv;
    }
};

typedef std::deque<BatchInput> BatchInputs;     // a thread's temp-batch files, batch by batch (a deque: an input owns its file and does not move)

// One batch's share of a tile of TEXT: its next T lines, from a 16-byte boundary.
inline void stage_lines(BgzfReader &rd, size_t T, std::vector<char> &text, uint32_t *starts)
{
    text.resize((text.size() + 15) & ~(size_t)15, '\n');
    if (rd.read_lines(T, text, starts) != T) throw std::runtime_error(kTruncatedBatch);
    if (text.size() > (size_t)0xF0000000u) throw std::runtime_error("ERROR: more than 3.75 GiB of text in one tile: lower --tile");
}

// One batch's share of a tile of RECORDS: its next T records one after the other as they come out of its stream (inflated on the
// CPU, or copied: the raw form), from an 8-byte boundary.
inline void stage_records(BgzfReader &rd, size_t T, std::vector<char> &text, uint32_t *starts)
{
    text.resize((text.size() + 7) & ~(size_t)7, 0);
    for (size_t t = 0; t < T; ++t) {
        unsigned char b4[4];
        if (rd.read(b4, 4) != 4) throw std::runtime_error(kTruncatedBatch);
        const size_t n = le32u(b4);
        const size_t at = text.size();
        if (at + 4 + n > (size_t)0xF0000000u) throw std::runtime_error("ERROR: more than 3.75 GiB of records in one tile: lower --tile");
        starts[t] = (uint32_t)at;
        text.resize(at + 4 + n);
        std::memcpy(&text[at], b4, 4);
        if (n && rd.read(&text[at + 4], n) != n) throw std::runtime_error("ERROR: truncated temp batch record");
    }
    starts[T] = (uint32_t)text.size();
}

}  // namespace bvchost
#endif
