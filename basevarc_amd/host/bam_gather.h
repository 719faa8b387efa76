// bam_gather.h -- a batch of BAM files made ready for the device calls that take their BGZF blocks still compressed (bvc_bam_pileup_bgzf:
// phase 1 of basetype, BVC_HOST_DEVICE_PILEUP; bvc_bam_popmatrix_bgzf: popmatrix, BVC_HOST_DEVICE_POPMATRIX).  Headers, SM tags and the
// .bai index stay on the CPU; the region's blocks are copied once, as they lie in the mapped files, into a page-locked buffer.
#ifndef BVC_HOST_BAM_GATHER_H
#define BVC_HOST_BAM_GATHER_H

#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bvc.h"
#include "bam.h"
#include "bam_blocks.h"

namespace bvchost {

// a thread's context and page-locked buffer: made at its first batch, gone with the thread (or the command)
struct LoadDevice {
    bvc_ctx *ctx = nullptr;
    unsigned char *pin = nullptr;
    size_t pin_cap = 0;
    ~LoadDevice() { if (pin) bvc_host_free(pin); if (ctx) bvc_destroy(ctx); }
};

struct BamBatch {
    size_t ns = 0;
    std::vector<std::string> paths, sms;            // the files and their SM tags, in list order
    std::vector<int32_t> rid;                       // the region's reference in each header; -1: not there
    std::vector<uint64_t> first_record;
    std::deque<MappedFile> files;
    std::vector<BamBlocks> lists;
    std::vector<uint8_t> to_eof, eof;
    std::vector<int64_t> off, end;
    std::vector<bvc_bgzf_block> table;
    int64_t comp_bytes = 0, out_bytes = 0;          // of the gathered blocks: compressed in the page-locked buffer, inflated on the device

    // Opens bams[b0 .. b1): the reference's errors for a file that does not open, is not sorted or has no SM tag, in list order.
    void open(const std::vector<std::string> &bams, size_t b0, size_t b1, const std::string &chr)
    {
        ns = b1 - b0;
        rid.assign(ns, -1); first_record.assign(ns, 0);
        for (size_t b = b0; b < b1; ++b) {
            BamFile reader;
            if (!reader.open(bams[b])) throw std::runtime_error("ERROR: can not open file " + bams[b]);
            if (!reader.sorted())
                throw std::runtime_error("ERROR: BAM file does not appear to be sorted (no SO:coordinate) found in header.\n       Sorted BAMs are required.");
            paths.push_back(bams[b]);
            sms.push_back(reader.sample_name());
            rid[b - b0] = reader.ref_index(chr);
            first_record[b - b0] = reader.first_record();
            files.emplace_back(bams[b]);
            if (!files.back().ok()) throw std::runtime_error("ERROR: can not open file " + bams[b]);
        }
        lists.assign(ns, BamBlocks());
        to_eof.assign(ns, 0); eof.assign(ns, 0); off.assign(ns, 0); end.assign(ns, 0);
    }

    // The region's blocks of every sample into dev.pin, with the table and the samples' ranges the device calls take.  again: the
    // second gathering of a batch -- only the samples marked to_eof are listed anew, to their files' ends.
    void gather(int32_t beg0, int32_t end0, bool again, LoadDevice &dev)
    {
        std::string err;
        size_t need = 0;
        for (size_t s = 0; s < ns; ++s) {
            if (rid[s] < 0) { lists[s] = BamBlocks(); lists[s].to_eof = true; continue; }
            if (again && !to_eof[s]) continue;                        // (its list stands)
            if (!bam_region_blocks(files[s], paths[s], first_record[s], rid[s], beg0, end0, to_eof[s] != 0, lists[s], err)) throw std::runtime_error(err);
        }
        for (auto const &l : lists) need += l.comp_bytes;
        if (need + 16 > dev.pin_cap) {
            if (dev.pin) bvc_host_free(dev.pin);
            dev.pin_cap = need + need / 4 + 4096;
            dev.pin = static_cast<unsigned char *>(bvc_host_alloc(dev.pin_cap));
            if (!dev.pin) { dev.pin_cap = 0; throw std::runtime_error("ERROR: page-locked allocation failed"); }
        }
        table.clear();
        int64_t comp_at = 0, out_at = 0;
        for (size_t s = 0; s < ns; ++s) {
            off[s] = out_at + lists[s].first_off;
            for (auto const &blk : lists[s].blocks) {
                std::memcpy(dev.pin + comp_at, blk.payload, blk.len);
                table.push_back(bvc_bgzf_block{comp_at, out_at, (int32_t)blk.len, (int32_t)blk.isize, blk.crc32, 1u});
                comp_at += (int64_t)blk.len;
                out_at += (int64_t)blk.isize;
            }
            end[s] = out_at;
            if (off[s] > end[s]) off[s] = end[s];
            eof[s] = lists[s].to_eof ? 1 : 0;
        }
        comp_bytes = comp_at; out_bytes = out_at;
    }

    // After BVC_BAM_MORE: the samples whose list stopped short of their region's end go to their files' ends.
    void mark_short(const std::vector<uint32_t> &status)
    {
        for (size_t s = 0; s < ns; ++s) to_eof[s] = status[s] == 2u;
    }
};

}  // namespace bvchost
#endif
