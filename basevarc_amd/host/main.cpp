// main.cpp -- `BaseVarC basetype`, `popmatrix` and `concat` on MI355X: the reference's command line, temp-batch files and outputs, with
// the per-site BaseType work of a whole tile of positions handed to libbvc in one call.
//
// Counterparts in the reference (src/BaseVarC.cpp): main :151-174, runBaseType :176-314, bt_r :467-534,
// bt_s :316-465, bt_f :536-669, parseOptions :797-827.  Same options and defaults, same file names
// (<out>.vcf.gz, <out>.cvg.gz, <out>.tmp.thread.<t>/batch.<b>), same --load/--rerun/--keep_tmp behaviour.
// Additive: --gpus <n> (devices to spread the threads over; default all), --tile <sites per device call>.
#include <dlfcn.h>
#include <getopt.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <tuple>
#include <unordered_map>

#include "../../include/bvc_bam.h"
#include "../../include/bvc_bam_text.h"
#include "../../include/bvc_popmatrix.h"
#include "../../include/bvc_store.h"
#include "../../include/bvc_bam_deflate.h"
#include "../../include/bvc_site_acc_pack.h"
#include "bam.h"
#include "bam_blocks.h"
#include "bam_gather.h"
#include "counts_file.h"
#include "feeds.h"
#include "popmatrix.h"

using namespace bvchost;

static const char *BASEVARC_USAGE_MESSAGE =
    "Contact: Zilong Li [zimusen94@gmail.com]\n"
    "Usage  : BaseVarC <command> [options]\n\n"
    "Commands:\n"
    "         basetype       Variants Caller\n"
    "         popmatrix      Create population matrix\n"
    "         concat         Concat popmatrix\n";

static const char *BASETYPE_MESSAGE =
    "Commands: BaseVarC basetype\n"
    "Usage   : BaseVarC basetype [options]\n\n"
    "Options :\n"
    "  --input,      -i         BAM/CRAM file list, one file per row\n"
    "  --output,     -o         Output file prefix\n"
    "  --reference,  -r         Reference file\n"
    "  --region,     -s         Samtools-like region <chr:start-end>\n"
    "  --group,      -g         Population group information <SampleID Group>\n"
    "  --mapq,       -q <INT>   Mapping quality >= INT [10]\n"
    "  --thread,     -t <INT>   Number of threads\n"
    "  --batch,      -b <INT>   Number of samples each batch\n"
    "  --maf,        -a <FLOAT> Minimum allele count frequency [min(0.001, 100/N, maf)]\n"
    "  --load,                  Load data only\n"
    "  --rerun,                 Read previous loaded data and rerun\n"
    "  --keep_tmp,              Don't remove tmp files when basetype finished\n"
    "  --verbose,    -v         Set verbose output\n"
    "  --gpus           <INT>   MI355X devices to use [all]\n"
    "  --tile           <INT>   Positions per device call [4096]\n"
    "  --tmp-format     <STR>   Temp-batch files written by the load phase: text (as BaseVarC), bin (binary\n"
    "                           records, deflated) or raw (binary records, stored: fastest to read back) [text];\n"
    "                           mem: no files at all, the batches stay in the memory of one device (BVC_HOST_STORE_GB\n"
    "                           caps them; not with --load, --keep_tmp or --gpus above 1)\n"
    "                           (BVC_HOST_STORE_WINDOWS=K|auto: in K windows of positions, one at a time, as -t T*K cuts them)\n"
    "                           counts: no files either; every batch is added into per-position class counts on one device\n"
    "                           (2 KB a position whatever the samples' number), the positions are called from those, and only\n"
    "                           the called positions and those with indels are piled up a second time, as mem keeps them\n"
    "                           (BVC_HOST_STORE_GB caps the counts, then those batches; not with --group, --load, --keep_tmp\n"
    "                           or --gpus above 1; BVC_HOST_COUNTS_GROUPS=1 takes --group: 16 bytes a group and position more,\n"
    "                           32 distinct group names in the file at the most; BVC_HOST_COUNTS_QUALS=Q, a multiple of 4 in\n"
    "                           4..128 [128]: 16 x Q bytes a position, and a base quality of Q or more ends the run;\n"
    "                           BVC_HOST_COUNTS_SAVE=FILE: the class counts are written to FILE after the first pass and the run\n"
    "                           ends there; BVC_HOST_COUNTS_LOAD=FILE[:FILE...]: such files are added before the first pass,\n"
    "                           which skips the BAMs they record)\n";

static const char *POPMATRIX_MESSAGE =
    "Commands: BaseVarC popmatrix\n"
    "Usage   : BaseVarC popmatrix [options]\n\n"
    "Options :\n"
    "  --input,      -i        BAM/CRAM files list, one file per row.\n"
    "  --output,     -o        Output file path\n"
    "  --posfile,    -p        Position file without header <CHR POS REF ALT>\n"
    "  --reference,  -r        Reference file\n"
    "  --mapq,       -q <INT>  Mapping quality >= INT [10]\n";

static const char *CONCAT_MESSAGE =
    "Commands: BaseVarC concat\n"
    "Usage   : BaseVarC concat [options]\n\n"
    "Options :\n"
    "  --input,      -i       List of matrix files for concat, one file per row.\n"
    "  --output,     -o       Output filename prefix(.gz will be added auto)\n";

namespace opt {
static bool verbose = false, rerun = false, load = false, keep_tmp = false, batch_given = false;
static int mapq = 10, thread = 1, batch = 10, gpus = 0, tile = 4096;
static double maf = 0.001;
static std::string input, reference, posfile, group, region, output, tmp_format = "text";
}  // namespace opt

static const char *shortopts = "hva:i:r:p:s:o:q:t:b:g:";
static const struct option longopts[] = {
    {"help", no_argument, NULL, 'h'},        {"verbose", no_argument, NULL, 'v'},
    {"keep_tmp", no_argument, NULL, 6},      {"load", no_argument, NULL, 7},
    {"rerun", no_argument, NULL, 8},         {"maf", required_argument, NULL, 'a'},
    {"input", required_argument, NULL, 'i'}, {"reference", required_argument, NULL, 'r'},
    {"posfile", required_argument, NULL, 'p'}, {"group", required_argument, NULL, 'g'},
    {"region", required_argument, NULL, 's'}, {"output", required_argument, NULL, 'o'},
    {"batch", required_argument, NULL, 'b'}, {"thread", required_argument, NULL, 't'},
    {"mapq", required_argument, NULL, 'q'},  {"gpus", required_argument, NULL, 9},
    {"tile", required_argument, NULL, 10},   {"tmp-format", required_argument, NULL, 11},
    {NULL, 0, NULL, 0}};

static void parse_options(int argc, char **argv, const char *msg)          // src/BaseVarC.cpp:797-827
{
    bool die = false;
    for (int c; (c = getopt_long(argc, argv, shortopts, longopts, NULL)) != -1;) {
        std::istringstream arg(optarg != NULL ? optarg : "");
        switch (c) {
        case 'q': arg >> opt::mapq; break;
        case 'b': arg >> opt::batch; opt::batch_given = true; break;
        case 't': arg >> opt::thread; break;
        case 'i': arg >> opt::input; break;
        case 'r': arg >> opt::reference; break;
        case 'p': arg >> opt::posfile; break;
        case 's': arg >> opt::region; break;
        case 'g': arg >> opt::group; break;
        case 'o': arg >> opt::output; break;
        case 'a': arg >> opt::maf; break;
        case 8: opt::rerun = true; break;
        case 7: opt::load = true; break;
        case 6: opt::keep_tmp = true; break;
        case 9: arg >> opt::gpus; break;
        case 10: arg >> opt::tile; break;
        case 11: arg >> opt::tmp_format; break;
        case 'v': opt::verbose = true; break;
        default: die = true;
        }
    }
    if (opt::tmp_format != "text" && opt::tmp_format != "bin" && opt::tmp_format != "raw" && opt::tmp_format != "mem" && opt::tmp_format != "counts")
        die = true;
    if (die || opt::input.empty() || opt::output.empty()) {
        std::cerr << msg;
        std::exit(die ? EXIT_FAILURE : EXIT_SUCCESS);
    }
}

static std::tuple<std::string, int32_t, int32_t> splitrg(std::string rg)   // src/BaseVarUtils.h:49-75
{
    if (rg.find(":") == std::string::npos || rg.find("-") == std::string::npos)
        throw std::invalid_argument("region must be feed with samtools-like format, i.e. chr:start-end");
    size_t p = rg.find(":");
    std::string chr = rg.substr(0, p);
    rg.erase(0, p + 1);
    p = rg.find("-");
    const int32_t s = std::stoi(rg.substr(0, p));
    rg.erase(0, p + 1);
    const int32_t e = std::stoi(rg) - 1;                                 // the reference's end - 1
    return std::make_tuple(chr, s, e);
}

static bool file_exists(const std::string &f) { struct stat st; return ::stat(f.c_str(), &st) == 0; }

static std::string tmp_name(int ithread, int ibatch)
{
    return opt::output + ".tmp.thread." + std::to_string(ithread) + "/batch." + std::to_string(ibatch);
}


// ---- phase 1: BAM -> temp-batch pileup text (bt_r, src/BaseVarC.cpp:467-534) ------------------------------------
static void bt_r(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq,
                 const std::string &chr, int32_t rg_s, int32_t rg_e, int nb, int bc, int ib, int thread)
{
    const size_t b0 = (size_t)ib * bc, b1 = (ib == nb - 1) ? bams.size() : (size_t)(ib + 1) * bc;
    std::vector<PosAlleleMap> allele_mv;
    std::string names;
    for (size_t b = b0; b < b1; ++b) {
        BamFile reader;
        if (!reader.open(bams[b])) throw std::runtime_error("ERROR: can not open file " + bams[b]);
        if (!reader.sorted())
            throw std::runtime_error("ERROR: BAM file does not appear to be sorted (no SO:coordinate) found in header.\n       Sorted BAMs are required.");
        const std::string sm = reader.sample_name();
        PosAlleleMap m;
        std::vector<BamRecord> rv;
        const int rid = reader.ref_index(chr);
        // region padded by 1000 on both sides (gr.Pad(1000), src/BamProcess.cpp:290); [beg, end) 0-based
        if (rid < 0 || !reader.fetch(rid, std::max(0, rg_s - 1 - 1000), rg_e + 1000, opt::mapq, rv) || rv.empty())
            std::cerr << "warning: " << sm << " region " << opt::region << " is empty." << std::endl;
        else
            find_snp_at_pos(rv, rg_s, refseq, pv, m);
        allele_mv.push_back(std::move(m));
        names += sm + '\t';
    }
    names += "\n";
    const bool bin = opt::tmp_format != "text";
    // "raw": the same binary records in stored (deflate level 0) BGZF blocks -- still valid BGZF with the EOF block the
    // --rerun check looks for, but reading them back is a copy instead of an inflate (half of the compute phase's
    // host time once the tokenising is gone)
    const int level = opt::tmp_format == "raw" ? 0 : 6;
    std::deque<BgzfWriter> fpv;                 // (a deque: a writer owns its file and its threads and does not move)
    for (int i = 0; i < thread; ++i) {
        fpv.emplace_back(tmp_name(i, ib), level);
        BgzfWriter &fp = fpv.back();
        if (!fp.ok()) throw std::runtime_error("ERROR: fail to write " + tmp_name(i, ib));
        if (bin) { std::string h; bin_batch_header((uint32_t)(b1 - b0), names, h); fp.write(h); }
        else fp.write(names);
    }
    const size_t psize = pv.size();
    const size_t window = psize % thread + psize / thread;
    std::string out, payload;
    for (size_t i = 0, j = 0; i < psize; ++i) {
        const int32_t p = pv[i];
        out.clear();
        if (bin) {                              // one record per position: u32 payload bytes + the entries present
            payload.clear();
            for (size_t k = 0; k < allele_mv.size(); ++k) {
                auto it = allele_mv[k].find(p);
                if (it != allele_mv[k].end()) bin_batch_entry(it->second, (uint32_t)k, payload);
            }
            const uint32_t n = (uint32_t)payload.size();
            for (int t = 0; t < 4; ++t) out.push_back((char)((n >> (8 * t)) & 0xff));
            out += payload;
        } else {
            for (auto const &m : allele_mv) {
                auto it = m.find(p);
                format_pileup_token(it == m.end() ? nullptr : &it->second, out);
            }
            out += "\n";
        }
        if (i == (j + 1) * window && j + 1 < (size_t)thread) ++j;
        fpv[j].write(out);
    }
    for (auto &fp : fpv)
        if (!fp.close()) std::cerr << "warning: file cannot be closed" << std::endl;
}

// ---- phase 1 on the device (BVC_HOST_DEVICE_PILEUP, --tmp-format bin|raw): the batch's BAM blocks are gathered as they lie in the files,
// inflated and piled up by ONE library call, and the records that come back are cut at the threads' windows as bt_r cuts them.  Headers
// and the .bai index stay on the CPU.
// text (BVC_HOST_DEVICE_PILEUP_TEXT, --tmp-format text): the same gathering and the same retries around bvc_bam_pileup_text_bgzf, and the
// lines that come back are cut at the same windows behind the names line.  line_start is 32-bit: a batch whose lines cannot fit
// 0xFFFFFF00 bytes -- by their floor of 2 bytes a sample and a newline a position, or by what the call reports -- goes to bt_r, said once.
// With BVC_HOST_DEVICE_PILEUP_DEFLATE (bin and text, not raw) the calls are their _deflate twins (include/bvc_bam_deflate.h): the windows are the
// call's pieces, and a thread's file is its header through the writer, then its piece's finished blocks.
static std::atomic<long> g_device_batches(0);
static std::atomic<int> g_load_threads(0);
static std::atomic<bool> g_text_fallback_said(false);
// The gathering and the retries around one of phase 1's library calls, shared by its forms: the batch's blocks are gathered, `call` makes
// the library call and returns its code, and a sample whose list stopped short of its region's end is gathered to its file's end, once.
// Returns false when `call` gave the batch up (kBatchGivenUp); throws the CPU path's messages for the statuses 3 and 4.
static const int kBatchGivenUp = -1000;
static std::string store_overflow_line(bvc_ctx *ctx)
{
    return std::string("ERROR: the batches do not fit the device's store (") + bvc_last_error(ctx) + "); --tmp-format bin keeps them in files";
}
template <class Call>
static bool device_batch_loop(BamBatch &batch, LoadDevice &dev, const std::vector<std::string> &bams, size_t b0, int32_t beg0, int32_t end0,
                              std::vector<uint32_t> &status, Call call)
{
    for (int attempt = 0;; ++attempt) {
        batch.gather(beg0, end0, attempt > 0, dev);
        const int rc = call();
        if (rc == BVC_OK) return true;
        if (rc == kBatchGivenUp) return false;
        if (rc == BVC_BAM_MORE && attempt == 0) {                     // a list that stopped short of its region's end: that sample to the file's end, once
            batch.mark_short(status);
            continue;
        }
        if (rc == BVC_ERR_DATA)
            for (size_t s = 0; s < status.size(); ++s) {
                // the messages of the CPU path: fetch's, and find_snp_at_pos's std::out_of_range
                if (status[s] == 3u) throw std::runtime_error("ERROR: truncated or corrupt BAM record in " + bams[b0 + s]);
                if (status[s] == 4u) throw std::out_of_range("index offset is out of range of the sequence");
            }
        if (rc == BVC_ERR_ALLOC) throw std::runtime_error(store_overflow_line(dev.ctx));
        throw std::runtime_error(std::string("ERROR: device pileup failed: ") + bvc_last_error(dev.ctx));
    }
}

static void bt_r_device(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq,
                        const std::string &chr, int32_t rg_s, int32_t rg_e, int nb, int bc, int ib, int thread, int gpus, bool text, const Knobs &knobs)
{
    const int64_t kTextMax = (int64_t)0xFFFFFF00u;
    auto on_the_cpu = [&]() {
        if (!g_text_fallback_said.exchange(true))
            std::cerr << "basetype: a batch's lines exceed 0xFFFFFF00 bytes, such batches are extracted on the CPU" << std::endl;
        bt_r(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, ib, thread);
    };
    {
        const int64_t n = (int64_t)((ib == nb - 1) ? bams.size() : (size_t)(ib + 1) * bc) - (int64_t)ib * bc;
        if (text && (2 * n + 1) * (int64_t)pv.size() > kTextMax) return on_the_cpu();
    }
    // a pool thread's context and page-locked buffer: made at its first batch, on the device device_of_thread gives, gone with the thread
    static thread_local LoadDevice dev;
    // deflate (BVC_HOST_DEVICE_PILEUP_DEFLATE, not with raw): the batch comes back as finished BGZF blocks, a piece a thread's window
    const bool deflate = knobs.device_pileup_deflate && opt::tmp_format != "raw";
    if (!dev.ctx) {
        if (bvc_create(&dev.ctx, device_of_thread(g_load_threads++, gpus, opt::gpus)) != BVC_OK)
            throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
        const bool tokens = deflate && text && knobs.device_pileup_deflate_tokens;
        if ((deflate && knobs.device_pileup_deflate_codes && bvc_set_tuning(dev.ctx, "bgzf_codes", 1) != BVC_OK) ||
            (tokens && (bvc_set_tuning(dev.ctx, "bgzf_parse", 1) != BVC_OK || bvc_set_tuning(dev.ctx, "bgzf_cuts", 1) != BVC_OK)))
            throw std::runtime_error(std::string("ERROR: libbvc: ") + bvc_last_error(dev.ctx));
    }
    const size_t b0 = (size_t)ib * bc, b1 = (ib == nb - 1) ? bams.size() : (size_t)(ib + 1) * bc, ns = b1 - b0;
    const int32_t beg0 = std::max(0, rg_s - 1 - 1000), end0 = rg_e + 1000;
    BamBatch batch;                                 // (headers, the mapped files, the blocks' gathering: bam_gather.h)
    batch.open(bams, b0, b1, chr);
    const std::vector<std::string> &sms = batch.sms;
    const std::vector<int32_t> &rid = batch.rid;
    std::string names;
    for (auto const &sm : sms) names += sm + '\t';
    names += "\n";
    std::vector<uint32_t> status(ns), rec_start(pv.size() + 1);
    std::vector<uint8_t> records;
    const std::vector<size_t> cuts = window_cuts(pv.size(), thread);
    std::vector<int32_t> piece_pos(1, 0);
    for (size_t c : cuts) piece_pos.push_back((int32_t)c);
    std::vector<int64_t> out_off((size_t)thread + 1, 0), piece_bytes((size_t)thread, 0);
    static thread_local std::vector<uint8_t> blocks; // (kept from batch to batch: a batch of the same size needs no second step)
    const bool done = device_batch_loop(batch, dev, bams, b0, beg0, end0, status, [&]() {
        int64_t need = 0;
        int rc;
        if (deflate) {
            rc = (text ? bvc_bam_pileup_text_bgzf_deflate : bvc_bam_pileup_bgzf_deflate)(
                dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(), batch.out_bytes, batch.off.data(),
                batch.end.data(), batch.eof.data(), rid.data(), beg0, end0, opt::mapq, (int32_t)pv.size(), pv.data(), rg_s, refseq.data(),
                (int64_t)refseq.size(), (int32_t)thread, piece_pos.data(), blocks.data(), (int64_t)blocks.size(), &need, out_off.data(),
                piece_bytes.data(), status.data());
            if (text && rc == BVC_ERR_ARG && need > kTextMax) return kBatchGivenUp;
            if (rc == BVC_BAM_MORE && need > (int64_t)blocks.size()) {  // the blocks are finished and kept: room for them, and a fetch
                blocks.resize((size_t)need + (size_t)need / 8);
                rc = bvc_bam_pileup_deflate_fetch(dev.ctx, blocks.data(), (int64_t)blocks.size());
            }
            return rc;
        }
        for (;;) {
            // (the two calls take the same arguments: records and rec_start hold the lines and line_start with text)
            rc = (text ? bvc_bam_pileup_text_bgzf : bvc_bam_pileup_bgzf)(
                dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(), batch.out_bytes, batch.off.data(),
                batch.end.data(), batch.eof.data(), rid.data(), beg0, end0, opt::mapq, (int32_t)pv.size(), pv.data(), rg_s, refseq.data(),
                (int64_t)refseq.size(), records.data(), (int64_t)records.size(), &need, rec_start.data(), status.data());
            if (text && rc == BVC_ERR_ARG && need > kTextMax) return kBatchGivenUp;
            if (rc != BVC_BAM_MORE || need <= (int64_t)records.size()) break;
            records.resize((size_t)need);
        }
        if (rc == BVC_OK) records.resize((size_t)need);
        return rc;
    });
    if (!done) return on_the_cpu();
    for (size_t s = 0; s < ns; ++s)
        if (rid[s] < 0 || status[s] == 1u) std::cerr << "warning: " << sms[s] << " region " << opt::region << " is empty." << std::endl;
    const int level = opt::tmp_format == "raw" ? 0 : 6;
    size_t lo = 0;
    for (int i = 0; i < thread; ++i) {
        BgzfWriter fp(tmp_name(i, ib), level);
        if (!fp.ok()) throw std::runtime_error("ERROR: fail to write " + tmp_name(i, ib));
        if (text) fp.write(names);
        else {
            std::string h;
            bin_batch_header((uint32_t)ns, names, h);
            fp.write(h);
        }
        const size_t hi = cuts[(size_t)i];
        if (deflate) fp.write_blocks(blocks.data() + out_off[(size_t)i], (size_t)(out_off[(size_t)i + 1] - out_off[(size_t)i]));
        else fp.write(reinterpret_cast<const char *>(records.data()) + rec_start[lo], (size_t)(rec_start[hi] - rec_start[lo]));
        lo = hi;
        if (!fp.close()) std::cerr << "warning: file cannot be closed" << std::endl;
    }
    ++g_device_batches;
}

// ---- phase 1 into the device's memory (--tmp-format mem): the same gathering and the same retries around bvc_bam_pileup_bgzf_store; the
// batch's records stay on device 0 as batch `ib` of the process's one store, and nothing is written.  The batch's sample names are kept
// here for the VCF header.
// With BVC_HOST_STORE_WINDOWS=K the region's positions are cut into K windows (store_windows, pileup.h) and a MemBatches is ONE window's
// store: positions pv[a .. b) piled up from the blocks gathered for [beg0, end0) (store_window_ranges), filled, computed from and dropped
// before the next one's (beside it with BVC_HOST_STORE_OVERLAP).  The reads of those blocks are filtered by the REGION's start, not the
// window's (keep_from): a read that ended in front of the window's cut stays in the list, because the rule steps from a first covering read
// whose position is deleted or skipped to the NEXT read of the list, covering or not -- without it the step would land on another read
// than the whole-region fetch's.  What outlives a window -- the sample names, which window 0 keeps, and the
// samples that had reads in some window -- is the run's (MemRun).
struct MemRun {
    std::vector<std::vector<std::string>> names;    // per batch, filled by the thread that extracts it (window 0)
    std::vector<std::string> sms;                   // per sample of the list: its name as the warning prints it (window 0)
    std::vector<char> has_reads;                    // per sample of the list: not empty (status 1 or no such reference) in some window
    int windows = 1;
    // the line that ends a run whose batches pass the budget also proposes a K: with K > 1, and with the knob unset
    bool propose_windows = false;
    // --tmp-format counts, its second pile-up: the names are kept and the warnings printed already
    bool quiet = false;
};
struct MemBatches {
    bvc_store *store = nullptr;                     // (none for a window without positions)
    size_t a = 0, b = 0;                            // the window's positions: pv[a .. b); the store's position 0 is pv[a]
    int32_t beg0 = 0, end0 = 0;                     // the range its blocks are gathered for
    int32_t keep_from = 0;                          // the region's padded start: reads that end behind it are kept, as the whole-region fetch keeps them
    std::atomic<int> kept{0};                       // batches put so far
    double load_s = 0;
    MemRun *run = nullptr;
    MemBatches() = default;
    MemBatches(const MemBatches &) = delete;
    MemBatches &operator=(const MemBatches &) = delete;
    ~MemBatches() { bvc_store_destroy(store); }
    void drop() { bvc_store_destroy(store); store = nullptr; }
};
static void bt_r_mem(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq, const std::string &chr,
                     int32_t rg_s, int nb, int bc, int ib, MemBatches &mem, int iwindow)
{
    static thread_local LoadDevice dev;
    if (!dev.ctx && bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
    const size_t b0 = (size_t)ib * bc, b1 = (ib == nb - 1) ? bams.size() : (size_t)(ib + 1) * bc, ns = b1 - b0;
    const int32_t beg0 = mem.beg0, end0 = mem.end0;
    MemRun &run = *mem.run;
    BamBatch batch;
    batch.open(bams, b0, b1, chr);
    std::vector<uint32_t> status(ns);
    device_batch_loop(batch, dev, bams, b0, beg0, end0, status, [&]() {
        int64_t bytes = 0;
        // (rg_s and refseq stay the region's: deletion text is cut from them)
        const int rc = bvc_bam_pileup_bgzf_store(dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(),
                                                 batch.out_bytes, batch.off.data(), batch.end.data(), batch.eof.data(), batch.rid.data(), mem.keep_from, end0,
                                                 opt::mapq, (int32_t)(mem.b - mem.a), pv.data() + mem.a, rg_s, refseq.data(), (int64_t)refseq.size(), mem.store, ib,
                                                 &bytes, status.data());
        if (rc == BVC_ERR_ALLOC && run.propose_windows) {
            // the windows that would fit, going by the share of the batches that did: K x (batches in all / batches kept), rounded up
            // (a run that kept none: as if it had kept half a batch)
            const int kept = mem.kept.load();
            const int64_t k = ((int64_t)run.windows * nb * 2 + std::max(1, 2 * kept) - 1) / std::max(1, 2 * kept);
            throw std::runtime_error(store_overflow_line(dev.ctx) + "; BVC_HOST_STORE_WINDOWS=" + std::to_string(std::max<int64_t>(k, run.windows + 1)) +
                                     " (or auto) cuts the region into windows of positions that fit one after the other");
        }
        return rc;
    });
    if (run.quiet) {
    } else if (run.windows == 1) {
        for (size_t s = 0; s < ns; ++s)
            if (batch.rid[s] < 0 || status[s] == 1u) std::cerr << "warning: " << batch.sms[s] << " region " << opt::region << " is empty." << std::endl;
    } else {
        // (a sample is empty in the region exactly when it is in every window: the warnings are printed after the last one)
        for (size_t s = 0; s < ns; ++s)
            if (!(batch.rid[s] < 0 || status[s] == 1u)) run.has_reads[b0 + s] = 1;
    }
    if (iwindow == 0 && !run.quiet) {
        run.names[(size_t)ib] = batch.sms;
        for (size_t s = 0; s < ns; ++s) run.sms[b0 + s] = batch.sms[s];
    }
    ++mem.kept;
    ++g_device_batches;
}

// ---- phase 1 into class counts (--tmp-format counts): the same gathering and the same retries around bvc_bam_counts_bgzf_acc; the batch
// is ADDED into the run's one accumulator on device 0 (only a call that succeeds adds anything, so the retry adds once) and nothing is
// kept of it but the names and the warnings, as --tmp-format mem prints them.
// What the counts pass leaves for the compute threads: the tallies of every position, which positions are revisited (counts_revisit,
// pileup.h), those positions as one ascending list -- what the second pile-up's store holds -- and each thread's share of that list.
struct CountsPass {
    const std::vector<int32_t> *pv = nullptr;       // the region's positions
    std::vector<bvc_bam_site_tally> tally;          // [pv->size()]
    std::vector<uint8_t> flags;                     // [pv->size()]: kRevisit* bits; 0 = the CVG line comes from the tally
    std::vector<int32_t> pvS;                       // the revisited positions
    std::vector<size_t> lo, hi;                     // per thread: its window of pv, cut with the set, as indices into pvS
    // BVC_HOST_COUNTS_GROUPS with --group: the groups' depths of every position, one row a distinct group name of the file (counts_group_map,
    // pileup.h), and per group that has a sample -- Groups' order -- its row
    int n_file_groups = 0;                          // 0: no --group
    std::vector<uint32_t> depth;                    // [pv->size()][n_file_groups][4]
    std::vector<int32_t> column_file_index;
};
// The group file as the counts pass reads it, once, before anything is piled up
struct GroupFile {
    std::vector<std::string> ids, groups, names;    // the lines in order; the distinct group names, sorted
};
// What the counts files of BVC_HOST_COUNTS_LOAD say of the run's BAMs, per BAM of --input: the file that records it as counted (-1: none,
// pass 1 piles it up) and its sample name as that file has it
struct LoadedCounts {
    std::vector<std::string> files;
    std::vector<int> file_of;
    std::vector<std::string> sample;
    std::atomic<int> piled{0};                      // batches pass 1 opened
    int64_t skipped = 0, entries = 0, bytes = 0;
};
static void bt_r_counts(const std::vector<std::string> &all_bams, const std::vector<int32_t> &pv, const std::string &refseq, const std::string &chr,
                        int32_t rg_s, int32_t rg_e, int nb, int bc, int ib, bvc_site_acc *acc, MemRun &run, const GroupFile *gf, int quals,
                        LoadedCounts &loaded)
{
    const size_t a0 = (size_t)ib * bc, a1 = (ib == nb - 1) ? all_bams.size() : (size_t)(ib + 1) * bc;
    // the batch's BAMs that no loaded file records: a batch without one is not opened, its names come from the files
    std::vector<std::string> bams;
    for (size_t b = a0; b < a1; ++b)
        if (loaded.file_of[b] < 0) bams.push_back(all_bams[b]);
    std::vector<std::string> &names_out = run.names[(size_t)ib];
    names_out.clear();
    if (bams.empty()) {
        for (size_t b = a0; b < a1; ++b) names_out.push_back(loaded.sample[b]);
        return;
    }
    ++loaded.piled;
    static thread_local LoadDevice dev;
    if (!dev.ctx && bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
    const size_t b0 = 0, b1 = bams.size(), ns = b1 - b0;
    const int32_t beg0 = std::max(0, rg_s - 1 - 1000), end0 = rg_e + 1000;
    BamBatch batch;
    batch.open(bams, b0, b1, chr);
    std::vector<uint32_t> status(ns);
    // (the labels of the groups' depths go by the group file alone: the other batches' names are not known yet)
    std::vector<uint8_t> label;
    if (gf) {
        std::vector<std::string> names;
        std::vector<int32_t> columns;
        counts_group_map(gf->ids, gf->groups, batch.sms, names, label, columns);
    }
    device_batch_loop(batch, dev, bams, b0, beg0, end0, status, [&]() {
        const int rc = bvc_bam_counts_bgzf_acc(dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(),
                                               batch.out_bytes, batch.off.data(), batch.end.data(), batch.eof.data(), batch.rid.data(), beg0, end0, opt::mapq,
                                               (int32_t)pv.size(), pv.data(), rg_s, (int64_t)refseq.size(), gf ? label.data() : nullptr, acc, status.data());
        // narrow rows (BVC_HOST_COUNTS_QUALS): a batch refused for a quality the rows have no column for ends the run (statuses 3 and 4 of
        // the same batch go first, with the loop's own messages)
        if (rc == BVC_ERR_DATA && std::none_of(status.begin(), status.end(), [](uint32_t s) { return s == 3u || s == 4u; }))
            for (size_t s = 0; s < ns; ++s)
                if (status[s] == 5u)
                    throw std::runtime_error("ERROR: a base quality of " + std::to_string(quals) + " or more in " + bams[b0 + s] + ": the counts keep " +
                                             std::to_string(quals) + " quality columns, run with BVC_HOST_COUNTS_QUALS=128");
        return rc;
    });
    for (size_t s = 0; s < ns; ++s)
        if (batch.rid[s] < 0 || status[s] == 1u) std::cerr << "warning: " << batch.sms[s] << " region " << opt::region << " is empty." << std::endl;
    // (a batch with some BAMs recorded: the names are spliced in input order)
    for (size_t b = a0, s = 0; b < a1; ++b) names_out.push_back(loaded.file_of[b] < 0 ? batch.sms[s++] : loaded.sample[b]);
    ++g_device_batches;
}

// The counts files of BVC_HOST_COUNTS_LOAD, opened and held against the run before anything is piled up: every refusal that a header can
// decide is one line naming the file and the field.  The readers stay open for counts_files_add.
struct CountsFileRun {
    CountsFileMeta meta;                            // what a file of THIS run records (the BAM lists are filled when it is saved)
    std::deque<CountsFileReader> readers;
};
static void counts_files_open(const std::vector<std::string> &files, const std::vector<std::string> &bams, CountsFileRun &cr, LoadedCounts &loaded)
{
    loaded.files = files;
    loaded.file_of.assign(bams.size(), -1);
    loaded.sample.assign(bams.size(), std::string());
    std::unordered_map<std::string, size_t> index_of;
    // (recorded BAMs are matched to --input by their path strings: with files to load, a path listed twice has no one line to match)
    for (size_t b = 0; b < bams.size() && !files.empty(); ++b)
        if (!index_of.insert({bams[b], b}).second)
            throw std::runtime_error("ERROR: --input lists " + bams[b] + " twice, and BVC_HOST_COUNTS_LOAD matches the counts files' BAM lists to it by path");
    const CountsFileMeta &want = cr.meta;
    for (size_t f = 0; f < files.size(); ++f) {
        cr.readers.emplace_back();
        CountsFileMeta m;
        std::string err;
        if (!cr.readers.back().open(files[f], m, err)) throw std::runtime_error("ERROR: " + err);
        auto refuse = [&](const std::string &field, const std::string &has, const std::string &run_has) {
            throw std::runtime_error("ERROR: " + files[f] + ": the counts file's " + field + " is " + has + ", the run's is " + run_has);
        };
        auto join = [](const std::vector<std::string> &v) { std::string t; for (auto const &x : v) t += (t.empty() ? "" : ",") + x; return "[" + t + "]"; };
        if (m.chrom != want.chrom) refuse("chromosome", m.chrom, want.chrom);
        if (m.rg_s != want.rg_s || m.rg_e != want.rg_e)
            refuse("range", std::to_string(m.rg_s) + "-" + std::to_string(m.rg_e), std::to_string(want.rg_s) + "-" + std::to_string(want.rg_e));
        if (m.n_positions != want.n_positions) refuse("n_positions", std::to_string(m.n_positions), std::to_string(want.n_positions));
        if (m.pos_hash != want.pos_hash) refuse("positions hash", std::to_string(m.pos_hash), std::to_string(want.pos_hash));
        if (m.mapq != want.mapq) refuse("-q", std::to_string(m.mapq), std::to_string(want.mapq));
        if (m.slots != want.slots) refuse("slots", std::to_string(m.slots), std::to_string(want.slots));
        if (m.depth_groups != want.depth_groups) refuse("depth_groups", std::to_string(m.depth_groups), std::to_string(want.depth_groups));
        if (m.groups != want.groups) refuse("group names", join(m.groups), join(want.groups));
        for (size_t i = 0; i < m.bam_paths.size(); ++i) {
            auto it = index_of.find(m.bam_paths[i]);
            if (it == index_of.end()) throw std::runtime_error("ERROR: " + files[f] + ": the counts file's BAM list records " + m.bam_paths[i] + ", which is not in --input");
            const size_t b = it->second;
            if (loaded.file_of[b] >= 0)
                throw std::runtime_error("ERROR: " + files[f] + ": the counts file's BAM list records " + m.bam_paths[i] + ", which " +
                                         files[(size_t)loaded.file_of[b]] + " records too");
            loaded.file_of[b] = (int)f;
            loaded.sample[b] = m.bam_samples[i];
            ++loaded.skipped;
        }
    }
}
// Every loaded file's pieces added into the new accumulator (bvc_site_acc_add_packed), in front of pass 1
static void counts_files_add(bvc_ctx *ctx, bvc_site_acc *acc, int quals, CountsFileRun &cr, LoadedCounts &loaded)
{
    CountsPiece p;
    std::string err;
    for (size_t f = 0; f < cr.readers.size(); ++f) {
        CountsFileReader &r = cr.readers[f];
        int rc;
        while ((rc = r.next(p, err)) == 1) {
            // narrow rows (BVC_HOST_COUNTS_QUALS): a count the rows have no column for ends the run (one slot: cells 0..511 are counts)
            for (size_t i = 0; i < p.cell.size() && quals < 128; ++i)
                if (p.cell[i] < 512u && (int)(p.cell[i] & 127u) >= quals)
                    throw std::runtime_error("ERROR: " + loaded.files[f] + ": the counts file holds a count of base quality " + std::to_string(p.cell[i] & 127u) +
                                             " and the counts keep " + std::to_string(quals) + " quality columns, run with BVC_HOST_COUNTS_QUALS=128");
            if (bvc_site_acc_add_packed(ctx, acc, p.t0, p.n, p.row_start.data(), p.cell.data(), p.count.data(), (int64_t)p.cell.size(), BVC_PTR_HOST) != BVC_OK)
                throw std::runtime_error("ERROR: " + loaded.files[f] + ": the counts file's piece at row " + std::to_string(p.t0) + " is refused: " + bvc_last_error(ctx));
        }
        if (rc < 0) throw std::runtime_error("ERROR: " + err);
        loaded.entries += r.entries();
        loaded.bytes += r.bytes();
    }
    cr.readers.clear();
}
// The accumulator packed in pieces of rows (bvc_site_acc_pack: host memory stays bounded) and written to `path`
static void counts_file_save(bvc_ctx *ctx, const bvc_site_acc *acc, size_t P, const std::string &path, const CountsFileMeta &meta, int64_t &entries, int64_t &bytes)
{
    const size_t rows = 65536;
    CountsFileWriter w;
    std::string err;
    if (!w.open(path, meta, err)) throw std::runtime_error("ERROR: " + err);
    std::vector<int64_t> row_start(rows + 1);
    std::vector<uint16_t> cell;
    std::vector<uint32_t> count;
    for (size_t t0 = 0; t0 < P; t0 += rows) {
        const size_t n = std::min(rows, P - t0);
        int64_t need = 0;
        int rc = bvc_site_acc_pack(ctx, acc, (int32_t)t0, (int32_t)n, row_start.data(), cell.data(), count.data(), (int64_t)cell.size(), &need, BVC_PTR_HOST);
        if (rc == BVC_ACC_MORE) {
            cell.resize((size_t)need); count.resize((size_t)need);
            rc = bvc_site_acc_pack(ctx, acc, (int32_t)t0, (int32_t)n, row_start.data(), cell.data(), count.data(), (int64_t)cell.size(), &need, BVC_PTR_HOST);
        }
        bvc_check(ctx, rc);
        if (!w.piece((int32_t)t0, (int32_t)n, row_start.data(), cell.data(), count.data(), err)) throw std::runtime_error("ERROR: " + err);
    }
    if (!w.close(err)) throw std::runtime_error("ERROR: " + err);
    entries = w.entries();
    bytes = w.bytes();
}

// ---- phase 2: temp batches -> tiles -> libbvc -> CVG/VCF (successor of bt_s + bt_f; the tiles' three stages: tile_runner.h, what
// fills them: feeds.h, the knobs: knobs.h) -------------------------------------------------------------------------------------
// population groups (src/BaseVarC.cpp:335-369): name-sorted, a sample not listed belongs to no group
static Groups read_groups(const std::vector<std::string> &names, int32_t N)
{
    Groups groups;
    if (opt::group.empty()) return groups;
    std::ifstream ifg(opt::group);
    std::unordered_map<std::string, std::string> popg_m;
    std::string id, grp;
    while (ifg >> id >> grp) popg_m.insert({id, grp});
    std::map<std::string, std::vector<int>> popg_idx;
    for (size_t i = 0; i < names.size(); ++i) {
        auto it = popg_m.find(names[i]);
        if (it != popg_m.end()) popg_idx[it->second].push_back((int)i);
    }
    if (popg_idx.size() > BVC_MAX_GROUPS) throw std::runtime_error("ERROR: more than 32 population groups");
    groups.of_sample.assign((size_t)N, 255);
    for (auto const &kv : popg_idx) {
        for (int i : kv.second) groups.of_sample[(size_t)i] = (uint8_t)groups.names.size();
        groups.names.push_back(kv.first);
    }
    groups.order_columns();
    return groups;
}

static void bt_s(const std::vector<std::string> &ftmp_v, const std::vector<int32_t> &pv, const std::string &refseq,
                 const std::string &chr, int32_t rg_s, int32_t N, int thread, int ithread, int device, const Knobs &knobs, DeviceSlots &slots,
                 const MemBatches *mem, const CountsPass *cp = nullptr)
{
    const double t_start = StageClock::now();
    // the outputs are deflated by threads of their writers' own (a VCF line carries a field per SAMPLE, a megabyte at 1e5 samples: up
    // to three threads deflate the VCF text)
    BgzfWriter fpv(opt::output + "." + std::to_string(ithread) + ".vcf.gz", 6, true, knobs.vcf_deflaters);
    BgzfWriter fpc(opt::output + "." + std::to_string(ithread) + ".cvg.gz", 6, true);
    std::deque<InflatePool> inflate_pool;                               // (none with BVC_HOST_INFLATE_THREADS=0; outlives the inputs)
    const int n_inflate = knobs.inflate_threads;
    if (n_inflate > 0) inflate_pool.emplace_back(n_inflate);
    BatchInputs in;
    for (auto const &f : ftmp_v) in.emplace_back(f);
    if (!inflate_pool.empty()) for (auto &fp : in) fp.rd.attach(&inflate_pool.front());
    // (BVC_HOST_PROFILE: on a GPU box the first ~0.5 s of every worker thread go to process-wide stalls while the HIP
    // runtime, started by bvc_device_count in main, finishes coming up -- whatever the thread does first pays them.)
    const double t_opened = StageClock::now();
    std::string sams;
    for (auto const &fp : in) sams += fp.names;
    if (!sams.empty()) sams.pop_back();                                 // names are tab-terminated
    std::vector<std::string> names;
    { std::istringstream iss(sams); std::string id; while (std::getline(iss, id, '\t')) names.push_back(id); }
    if (mem)                                                            // (no batch files: the names phase 1 kept, in batch order)
        for (auto const &of_batch : mem->run->names) names.insert(names.end(), of_batch.begin(), of_batch.end());
    const Groups groups = read_groups(names, N);
    if (ithread == 0) {
        fpc.write(cvg_header(groups));
        fpv.write(vcf_header(groups, opt::reference, names));
    }
    std::cerr << "begin to load data and run basetype" << std::endl;
    const double t_header = StageClock::now();
    TileRunner tr(knobs);
    const double t_create = StageClock::now();
    if (bvc_create(&tr.ctx, device) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
    if (knobs.device_deflate_codes && bvc_set_tuning(tr.ctx, "bgzf_codes", 1) != BVC_OK)
        throw std::runtime_error(std::string("ERROR: libbvc: ") + bvc_last_error(tr.ctx));
    if (knobs.device_deflate_fields && bvc_set_tuning(tr.ctx, "bgzf_parse", 1) != BVC_OK)
        throw std::runtime_error(std::string("ERROR: libbvc: ") + bvc_last_error(tr.ctx));
    const double create_s = StageClock::now() - t_create;
    tr.groups = groups.empty() ? nullptr : &groups;
    tr.chr = chr;
    tr.n_samples = N;
    tr.ithread = ithread;
    double min_af = 100.0 / N;                                          // src/BaseVarC.cpp:541-543
    if (min_af > 0.001) min_af = 0.001;
    if (opt::maf < min_af) min_af = opt::maf;
    tr.min_af = min_af;
    tr.fvcf = &fpv;
    tr.fcvg = &fpc;
    // --tmp-format counts: pv is the revisited positions; the CVG lines of the thread's other positions are written from their tallies, in
    // front of each revisited position's lines and at the window's end (a position without an entry the parser keeps gets no line)
    size_t fill_at = 0, fill_hi = 0;
    // (with groups: one record a group that has a sample, its depth from the counts pass's row of that group)
    std::vector<bvc_group_result> fill_grp;
    if (cp) {
        thread_window(cp->pv->size(), thread, ithread, fill_at, fill_hi);
        if (cp->n_file_groups > 0) {
            if (cp->column_file_index.size() != groups.names.size()) throw std::runtime_error("ERROR: the counts pass's groups are not the group file's");
            fill_grp.assign(groups.names.size(), bvc_group_result());
        }
        tr.before_pos = [&, cp](int32_t pos) {
            for (; fill_at < fill_hi && (*cp->pv)[fill_at] < pos; ++fill_at) {
                if (cp->flags[fill_at]) continue;
                const bvc_bam_site_tally &y = cp->tally[fill_at];
                int32_t cnt[4], fwd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int b = 0; b < 4; ++b) { rev[b] = (int32_t)y.strand_base[b]; fwd[b] = (int32_t)y.strand_base[4 + b]; cnt[b] = rev[b] + fwd[b]; }
                if (cnt[0] + cnt[1] + cnt[2] + cnt[3] == 0) continue;
                SiteView v;
                v.pos = (*cp->pv)[fill_at]; v.cnt = cnt; v.fwd = fwd; v.rev = rev;
                const uint32_t *row = fill_grp.empty() ? nullptr : cp->depth.data() + fill_at * (size_t)cp->n_file_groups * 4;
                for (size_t c = 0; c < fill_grp.size(); ++c)
                    for (int b = 0; b < 4; ++b) fill_grp[c].depth[b] = (int32_t)row[(size_t)cp->column_file_index[c] * 4 + (size_t)b];
                fpc.write(cvg_line(chr, ref_code(refseq[(size_t)(v.pos - rg_s)]), v, fill_grp.empty() ? nullptr : fill_grp.data(), (int)fill_grp.size()));
            }
        };
    }
    tr.start();
    Window w = {pv, refseq, rg_s, 0, 0, opt::tile > 0 ? opt::tile : 4096};
    if (!groups.empty()) w.tile = std::max<int64_t>(1, std::min<int64_t>(w.tile, ((int64_t)256 << 20) / std::max(1, N)));
    thread_window(pv.size(), thread, ithread, w.lo, w.hi);
    if (cp) { w.lo = cp->lo[(size_t)ithread]; w.hi = cp->hi[(size_t)ithread]; }
    reset_parser_carry();
    // The feed.  Tiles of TEXT, or of binary RECORDS when every batch file is binary, for the device parser (the default);
    // BVC_HOST_DEVICE_PARSE=0 keeps the CPU parser (A/B runs, and what the quality-shift test hook and a mix of text and binary files
    // use) ...
    const int qual_shift = knobs.qual_shift;
    bool dev_parse = (!qual_shift && knobs.device_parse) || mem;
    size_t n_bin_files = 0;
    for (auto const &fp : in) if (fp.bin) ++n_bin_files;
    if (n_bin_files != 0 && n_bin_files != in.size()) dev_parse = false;
    const bool dev_bin = dev_parse && n_bin_files != 0;
    const double t_loop = StageClock::now();
    // ... and with the blocks of the text batches inflated on the device too (the default): BVC_HOST_DEVICE_INFLATE=0 inflates on the CPU
    const bool dev_inflate = dev_parse && !dev_bin && knobs.device_inflate;
    if (dev_parse) {
        // per batch: its first sample and its samples, from the binary header or the names line (tab-terminated names,
        // src/BaseVarC.cpp:495, 503)
        int32_t j0 = 0;
        for (auto const &fp : in) {
            const int32_t n_in = fp.bin ? (int32_t)fp.n_in_batch : (int32_t)std::count(fp.names.begin(), fp.names.end(), '\t');
            tr.sample0.push_back(j0); tr.n_in_batch.push_back(n_in);
            j0 += n_in;
        }
        get_parser_carry(tr.carry);                                     // (zeros: reset_parser_carry above)
    }
    if (mem) feed_store_tiles(tr, w, mem->store, mem->a, slots, device);       // (a window without positions has no store and no tile)
    else if (dev_inflate) {
        std::vector<int32_t> skip;
        for (auto const &fp : in) skip.push_back((int32_t)fp.names.size() + 1);      // the names line and its newline
        in.clear();                                                     // closed before the feed maps the same files
        BgzfFeed(tr, w, ftmp_v, skip, slots, device).run();
    } else if (dev_bin) feed_staged_tiles(tr, w, in, TileForm::Records);
    else if (dev_parse) feed_staged_tiles(tr, w, in, TileForm::Text);
    else feed_cpu_parser(tr, w, in, qual_shift);
    tr.finish();
    if (cp) tr.before_pos(0x7FFFFFFF);                                  // (the stages are joined: the lines behind the last revisited position)
    const double loop_s = StageClock::now() - t_loop, setup_s = t_loop - t_start;
    if (knobs.profile) {
        // (each line composed first and written at once: the threads end side by side, and a line written piece by piece ends up inside
        // another thread's)
        std::ostringstream os;
        os << "[profile] thread " << ithread << ": library calls on one-byte tiles " << tr.tiles_one_byte << ", on two-byte tiles "
           << tr.tiles_two_byte << "; tiles of text or records parsed on the device " << tr.tiles_dev_parsed << ", handed back to the CPU parser "
           << tr.tiles_cpu_parsed << "; with the called positions' statistics from the device " << tr.tiles_dev_stats
           << ", with their sample columns from the device " << tr.tiles_dev_samples << ", with those columns deflated on the device "
           << tr.tiles_dev_deflate << "\n";
        const StageClock &c = tr.clk, &d = tr.clk_dev, &o = tr.clk_out;
        os << "[profile] thread " << ithread << ": stage 1 read+inflate " << c.read << " s, parse " << c.parse << " s | stage 2 pack "
           << d.pack << " s, libbvc " << d.gpu << " s | stage 3 cvg lines " << o.cvg << " s, vcf lines " << o.vcf
           << " s, compress+write " << o.write << " s; setup (open batches " << t_opened - t_start << " s, names + header "
           << t_header - t_opened << " s, bvc_create " << create_s << " s) " << setup_s << " s, position loop " << loop_s << " s, thread total "
           << StageClock::now() - t_start << " s\n";
        std::cerr << os.str() << std::flush;
    }
    bvc_destroy(tr.ctx);
    if (!fpv.close()) std::cerr << "warning: file cannot be closed" << std::endl;
    if (!fpc.close()) std::cerr << "warning: file cannot be closed" << std::endl;
    in.clear();
    if (!opt::keep_tmp)
        for (auto const &f : ftmp_v) std::remove(f.c_str());
}

template <class F>
static void run_pool(int n_tasks, int n_threads, F fn)
{
    std::atomic<int> next(0);
    std::mutex mu;
    std::string err;
    std::vector<std::thread> ws;
    for (int t = 0; t < std::max(1, std::min(n_threads, n_tasks)); ++t)
        ws.emplace_back([&]() {
            for (int i; (i = next++) < n_tasks;) {
                try { fn(i); } catch (const std::exception &e) { std::lock_guard<std::mutex> g(mu); if (err.empty()) err = e.what(); }
            }
        });
    for (auto &w : ws) w.join();
    if (!err.empty()) throw std::runtime_error(err);
}

// ---- --tmp-format mem: both phases, window by window (BVC_HOST_STORE_WINDOWS; one window = the whole region without it) -----------------
// The free memory of the device, as the HIP runtime that libbvc brought into the process reports it (the library has no call for it and
// the host program does not link the runtime itself); 0 where the runtime's symbol is not to be had.
static double device_free_bytes()
{
    typedef int (*mem_info_fn)(size_t *, size_t *);
    mem_info_fn fn = reinterpret_cast<mem_info_fn>(dlsym(RTLD_DEFAULT, "hipMemGetInfo"));
    size_t free_b = 0, total_b = 0;
    return fn && fn(&free_b, &total_b) == 0 ? (double)free_b : 0.0;
}

// BVC_HOST_STORE_WINDOWS=auto: batch 0 piled up once for the whole region (bvc_bam_pileup_bgzf, its records on the host); its rec_start
// scaled to the cohort is the estimate auto_store_windows (knobs.h) sizes the windows by.  budget <= 0: the device's free memory.
static int choose_store_windows(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq, const std::string &chr,
                                int32_t rg_s, int32_t rg_e, int nb, int bc, int thread, double budget)
{
    LoadDevice dev;
    if (bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
    const size_t ns = nb == 1 ? bams.size() : (size_t)bc;
    const int32_t beg0 = std::max(0, rg_s - 1 - 1000), end0 = rg_e + 1000;
    BamBatch batch;
    batch.open(bams, 0, ns, chr);
    std::vector<uint32_t> status(ns), rec_start(pv.size() + 1);
    std::vector<uint8_t> records;
    device_batch_loop(batch, dev, bams, 0, beg0, end0, status, [&]() {
        int64_t need = 0;
        int rc;
        for (;;) {
            rc = bvc_bam_pileup_bgzf(dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(), batch.out_bytes,
                                     batch.off.data(), batch.end.data(), batch.eof.data(), batch.rid.data(), beg0, end0, opt::mapq, (int32_t)pv.size(), pv.data(),
                                     rg_s, refseq.data(), (int64_t)refseq.size(), records.data(), (int64_t)records.size(), &need, rec_start.data(), status.data());
            if (rc != BVC_BAM_MORE || need <= (int64_t)records.size()) break;
            records.resize((size_t)need);
        }
        return rc;
    });
    if (budget <= 0) budget = device_free_bytes();
    if (budget <= 0) throw std::runtime_error("ERROR: BVC_HOST_STORE_WINDOWS=auto cannot learn the device's free memory; give BVC_HOST_STORE_GB");
    return auto_store_windows(rec_start.data(), pv.size(), thread, kStoreWindowsMaxThreads / thread, (double)bams.size() / (double)ns, nb, budget);
}

template <class Compute>
static void basetype_in_memory(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq, const std::string &chr,
                               int32_t rg_s, int32_t rg_e, int nb, int bc, int thread, const Knobs &knobs, int &n_sub, std::string &werr, std::mutex &mu,
                               double &t_loaded, Compute compute)
{
    if (bvc_device_count() <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
    const int64_t budget = (int64_t)(knobs.store_gb * 1073741824.0);
    int K = knobs.store_windows;
    // (with BVC_HOST_STORE_OVERLAP two stores are alive at a time: each gets half of the budget)
    const bool may_overlap = knobs.store_overlap && K != 1;
    if (K == 0) {
        K = choose_store_windows(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, thread, (double)budget / (may_overlap ? 2.0 : 1.0));
        if (knobs.profile) std::cerr << "[profile] main: BVC_HOST_STORE_WINDOWS=auto chose " << K << " windows" << std::endl;
    }
    const bool overlap = may_overlap && K > 1;
    const int64_t window_budget = overlap ? std::max<int64_t>(budget / 2, budget > 0 ? 1 : 0) : budget;
    n_sub = thread * K;
    MemRun run;
    run.windows = K;
    run.propose_windows = K > 1 || knobs.store_windows != 1 || !Knobs::set("BVC_HOST_STORE_WINDOWS");
    run.names.resize((size_t)nb);
    run.sms.resize(bams.size());
    run.has_reads.assign(bams.size(), 0);
    std::vector<size_t> wa((size_t)K), wb((size_t)K);
    std::vector<int32_t> wbeg((size_t)K), wend((size_t)K);
    store_windows(pv.size(), thread, K, wa.data(), wb.data());
    store_window_ranges(pv.data(), K, wa.data(), wb.data(), std::max(0, rg_s - 1 - 1000), rg_e + 1000, wbeg.data(), wend.data());
    std::deque<MemBatches> wins;                    // (a deque: a window's store does not move)
    for (int w = 0; w < K; ++w) {
        wins.emplace_back();
        MemBatches &m = wins.back();
        m.a = wa[(size_t)w]; m.b = wb[(size_t)w]; m.beg0 = wbeg[(size_t)w]; m.end0 = wend[(size_t)w]; m.keep_from = wbeg[0]; m.run = &run;
    }
    auto failed = [&]() { std::lock_guard<std::mutex> g(mu); return !werr.empty(); };
    // a window's load: its store made, every batch piled up into it, the store sealed.  An error is kept as the compute threads' are
    auto load = [&](int w) {
        MemBatches &m = wins[(size_t)w];
        if (m.a == m.b && w > 0) return;                                // (no positions: no store; window 0 keeps the names even so)
        const double t0 = StageClock::now();
        try {
            if (bvc_store_create(&m.store, 0, (int32_t)(m.b - m.a), nb, window_budget) != BVC_OK)
                throw std::runtime_error("ERROR: no usable gfx950 device for the store of the batches");
            run_pool(nb, thread, [&](int t) { bt_r_mem(bams, pv, refseq, chr, rg_s, nb, bc, t, m, w); });
            LoadDevice dev;                                             // (sealing takes a context; any of the store's device)
            if (bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
            bvc_check(dev.ctx, bvc_store_seal(dev.ctx, m.store));
        } catch (const std::exception &e) { std::lock_guard<std::mutex> g(mu); if (werr.empty()) werr = e.what(); }
        m.load_s = StageClock::now() - t0;
    };
    auto used_bytes = [&](int w) { int64_t used = 0; if (wins[(size_t)w].store) bvc_store_bytes(wins[(size_t)w].store, &used, nullptr); return used; };
    // once the last window is loaded: the samples that were empty in every window, in list order, and the line that ends the load phase
    auto all_loaded = [&]() {
        if (K > 1) {
            std::ostringstream os;
            for (size_t s = 0; s < bams.size(); ++s)
                if (!run.has_reads[s]) os << "warning: " << run.sms[s] << " region " << opt::region << " is empty.\n";
            std::cerr << os.str() << std::flush;
        } else if (knobs.profile) {
            std::cerr << "[profile] main: load phase on the device, " << g_device_batches.load() << " batches kept there (bvc_bam_pileup_bgzf_store), "
                      << used_bytes(0) << " bytes" << std::endl;
        }
        time_t tim1 = time(0);
        std::cout << "basetype loading done -- " << ctime(&tim1);
    };
    double compute_total = 0;
    int64_t largest = 0;
    int largest_w = 0;
    load(0);
    if (K == 1 && !failed()) all_loaded();
    for (int w = 0; w < K && !failed(); ++w) {
        // BVC_HOST_STORE_OVERLAP: the next window is loaded beside this one's compute threads, and both are joined before anything else
        std::thread loader;
        if (overlap && w + 1 < K) loader = std::thread([&, w]() { load(w + 1); });
        const double t0 = StageClock::now();
        compute(w * thread, &wins[(size_t)w], 0, nullptr);
        const double compute_s = StageClock::now() - t0;
        if (loader.joinable()) loader.join();
        compute_total += compute_s;
        const int64_t used = used_bytes(w);
        if (used > largest) { largest = used; largest_w = w; }
        if (knobs.profile && K > 1) {
            std::ostringstream os;
            os << "[profile] main: window " << w << " of " << K << ": positions [" << wins[(size_t)w].a << ", " << wins[(size_t)w].b << "), fetch range ["
               << wins[(size_t)w].beg0 << ", " << wins[(size_t)w].end0 << "), " << wins[(size_t)w].kept.load() << " batches kept, " << used << " bytes, load "
               << wins[(size_t)w].load_s << " s, compute " << compute_s << " s\n";
            if (overlap && w + 1 < K)
                os << "[profile] main: windows " << w << " and " << w + 1 << " alive together: " << used << " + " << used_bytes(w + 1) << " = "
                   << used + used_bytes(w + 1) << " bytes (budget " << budget << ")\n";
            std::cerr << os.str() << std::flush;
        }
        wins[(size_t)w].drop();
        if (!overlap && w + 1 < K && !failed()) load(w + 1);
        if (K > 1 && w + 2 == K && !failed()) all_loaded();             // (the last window's load has just ended, either way)
    }
    if (knobs.profile && K > 1 && !failed())
        std::cerr << "[profile] main: " << K << " windows, the largest store held " << largest << " bytes (window " << largest_w << ")" << std::endl;
    t_loaded = StageClock::now() - compute_total;
}

// ---- --tmp-format counts: pass 1 adds every batch into one accumulator of class counts and tallies (bvc_bam_counts.h) and calls the
// positions from it; pass 2 piles the revisited positions -- the called ones, those with indel entries and their predecessors, a fraction of
// a per cent -- up a second time into a store, as --tmp-format mem does for all of them, and the compute threads run on that store.  The
// BAMs are gathered exactly twice whatever the cohort's size and the region's length; the accumulator and the store are never alive together.
// With BVC_HOST_COUNTS_LOAD the accumulator starts from the loaded files' sum and pass 1 skips the BAMs they record; with
// BVC_HOST_COUNTS_SAVE the run ends behind pass 1, the accumulator written to a counts file (returns true: nothing was computed).
template <class Compute>
static bool basetype_counts(const std::vector<std::string> &bams, const std::vector<int32_t> &pv, const std::string &refseq, const std::string &chr,
                            int32_t rg_s, int32_t rg_e, int nb, int bc, int thread, const Knobs &knobs, const GroupFile *gf, double &t_loaded,
                            Compute compute)
{
    if (bvc_device_count() <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
    const int64_t budget = (int64_t)(knobs.store_gb * 1073741824.0);
    const size_t P = pv.size();
    const size_t G = gf ? gf->names.size() : 0;                         // (depth rows: 16 bytes a group and position)
    const int Q = knobs.counts_quals;                                   // (BVC_HOST_COUNTS_QUALS: 128 unless set; checked in run_basetype)
    const int64_t need = (int64_t)P * (int64_t)(16 * (size_t)Q + sizeof(bvc_bam_site_tally) + 16 * G);
    const std::string what = "the class counts" + std::string(G ? " and the groups' depths" : "") + " of " + std::to_string(P) + " positions take " +
                             std::to_string(need) + " bytes";
    if (budget > 0 && need > budget)
        throw std::runtime_error("ERROR: " + what + " and BVC_HOST_STORE_GB allows " + std::to_string(budget) + "; --tmp-format bin keeps the batches in files");
    MemRun run;
    run.names.resize((size_t)nb);
    run.sms.resize(bams.size());
    // the counts files: what a file of this run records, and the loaded files held against it before anything is piled up
    CountsFileRun cr;
    LoadedCounts loaded;
    cr.meta.chrom = chr; cr.meta.rg_s = rg_s; cr.meta.rg_e = rg_e; cr.meta.n_positions = (int32_t)P; cr.meta.mapq = opt::mapq;
    cr.meta.pos_hash = counts_fnv1a64(pv.data(), P * sizeof(int32_t));
    cr.meta.slots = 1; cr.meta.depth_groups = (uint32_t)G; cr.meta.n_quals = (uint32_t)Q;
    if (gf) cr.meta.groups = gf->names;
    counts_files_open(knobs.counts_load, bams, cr, loaded);
    const bool files = !knobs.counts_load.empty() || !knobs.counts_save.empty();
    int64_t saved_entries = 0, saved_bytes = 0;
    CountsPass cp;
    cp.pv = &pv;
    cp.tally.resize(P);
    cp.flags.assign(P, 0);
    cp.n_file_groups = (int)G;
    cp.depth.resize(P * G * 4);
    std::vector<uint8_t> called(P, 0);
    double min_af = 100.0 / (double)bams.size();                        // src/BaseVarC.cpp:541-543, as bt_s has it
    if (min_af > 0.001) min_af = 0.001;
    if (opt::maf < min_af) min_af = opt::maf;
    int64_t acc_bytes = 0;
    {
        struct Acc { bvc_site_acc *p = nullptr; ~Acc() { bvc_site_acc_destroy(p); } } acc;
        if ((Q < 128 ? bvc_site_acc_create_quals(&acc.p, 0, (int32_t)P, (int32_t)G, Q, budget)
             : G     ? bvc_site_acc_create_depth(&acc.p, 0, (int32_t)P, (int32_t)G, budget)
                     : bvc_site_acc_create(&acc.p, 0, (int32_t)P, 0, budget)) != BVC_OK)
            throw std::runtime_error("ERROR: the device has no room: " + what + "; --tmp-format bin keeps the batches in files");
        LoadDevice dev;
        if (bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
        counts_files_add(dev.ctx, acc.p, Q, cr, loaded);
        run_pool(nb, thread, [&](int t) { bt_r_counts(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, t, acc.p, run, gf, Q, loaded); });
        bvc_site_acc_bytes(acc.p, &acc_bytes, nullptr);
        if (!knobs.counts_save.empty()) {
            // every BAM of --input is counted now, by a loaded file or by pass 1: the saved file holds the sum and the union of the lists
            cr.meta.bam_paths = bams;
            for (auto const &of_batch : run.names) cr.meta.bam_samples.insert(cr.meta.bam_samples.end(), of_batch.begin(), of_batch.end());
            counts_file_save(dev.ctx, acc.p, P, knobs.counts_save, cr.meta, saved_entries, saved_bytes);
        }
        if (knobs.profile && files)
            std::cerr << "[profile] main: counts files: " << knobs.counts_load.size() << " loaded (" << loaded.entries << " entries added, " << loaded.bytes
                      << " bytes), " << loaded.skipped << " BAMs skipped, " << loaded.piled.load() << " of " << nb << " batches piled up in pass 1, "
                      << (knobs.counts_save.empty() ? 0 : 1) << " saved (" << saved_entries << " entries written, " << saved_bytes
                      << " bytes), accumulator " << acc_bytes << " bytes" << std::endl;
        if (!knobs.counts_save.empty()) {
            std::cout << "basetype counts saved -- " << knobs.counts_save << ": " << bams.size() << " BAMs, " << saved_entries << " entries, " << saved_bytes
                      << " bytes" << std::endl;
            return true;
        }
        const size_t chunk = 8192;
        std::vector<int8_t> refs(chunk);
        std::vector<bvc_site_result> res(chunk);
        for (size_t t0 = 0; t0 < P; t0 += chunk) {
            const size_t n = std::min(chunk, P - t0);
            for (size_t k = 0; k < n; ++k) refs[k] = ref_code(refseq[(size_t)(pv[t0 + k] - rg_s)]);
            bvc_check(dev.ctx, bvc_site_acc_lrt(dev.ctx, acc.p, (int32_t)t0, (int32_t)n, refs.data(), min_af, res.data(), nullptr));
            bvc_check(dev.ctx, bvc_site_acc_get(dev.ctx, acc.p, (int32_t)t0, (int32_t)n, nullptr, &cp.tally[t0]));
            if (G) bvc_check(dev.ctx, bvc_site_acc_get_depth(dev.ctx, acc.p, (int32_t)t0, (int32_t)n, &cp.depth[t0 * G * 4]));
            for (size_t k = 0; k < n; ++k) called[t0 + k] = res[k].called != 0;
        }
    }
    if (gf) {
        // the names are known now: the groups that have a sample (read_groups' set, in its order) and each one's depth row
        std::vector<std::string> all, names;
        std::vector<uint8_t> label;
        for (auto const &of_batch : run.names) all.insert(all.end(), of_batch.begin(), of_batch.end());
        counts_group_map(gf->ids, gf->groups, all, names, label, cp.column_file_index);
    }
    counts_revisit(cp.tally.data(), called.data(), P, thread, cp.flags.data());
    size_t n_called = 0, n_indel = 0, n_carry = 0;
    cp.lo.assign((size_t)thread, 0); cp.hi.assign((size_t)thread, 0);
    for (int i = 0; i < thread; ++i) {
        size_t lo, hi;
        thread_window(P, thread, i, lo, hi);
        cp.lo[(size_t)i] = cp.pvS.size();
        for (size_t t = lo; t < hi; ++t) {
            const uint8_t f = cp.flags[t];
            if (!f) continue;
            cp.pvS.push_back(pv[t]);
            if (f & kRevisitCalled) ++n_called;
            if (f & kRevisitIndel) ++n_indel;
            if (f == kRevisitCarry) ++n_carry;
        }
        cp.hi[(size_t)i] = cp.pvS.size();
    }
    MemBatches m;
    m.run = &run; m.a = 0; m.b = cp.pvS.size(); m.beg0 = m.keep_from = std::max(0, rg_s - 1 - 1000); m.end0 = rg_e + 1000;
    int64_t store_bytes = 0;
    if (!cp.pvS.empty()) {
        run.quiet = true;
        if (bvc_store_create(&m.store, 0, (int32_t)cp.pvS.size(), nb, budget) != BVC_OK)
            throw std::runtime_error("ERROR: no usable gfx950 device for the store of the batches");
        run_pool(nb, thread, [&](int t) { bt_r_mem(bams, cp.pvS, refseq, chr, rg_s, nb, bc, t, m, 0); });
        LoadDevice dev;
        if (bvc_create(&dev.ctx, 0) != BVC_OK) throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
        bvc_check(dev.ctx, bvc_store_seal(dev.ctx, m.store));
        bvc_store_bytes(m.store, &store_bytes, nullptr);
    }
    if (knobs.profile)
        std::cerr << "[profile] main: counts pass: " << P << " positions, " << cp.pvS.size() << " revisited (" << n_called << " called, " << n_indel
                  << " with indel entries, " << n_carry << " for the carry), accumulator " << acc_bytes << " bytes, store " << store_bytes << " bytes" << std::endl;
    time_t tim1 = time(0);
    std::cout << "basetype loading done -- " << ctime(&tim1);
    t_loaded = StageClock::now();
    compute(0, &m, 0, &cp);
    return false;
}

static void run_basetype(int argc, char **argv)                          // src/BaseVarC.cpp:176-314
{
    parse_options(argc, argv, BASETYPE_MESSAGE);
    const bool counts = opt::tmp_format == "counts";                    // (no temp files either: everything `mem` refuses, and --group without its knob)
    const bool in_memory = opt::tmp_format == "mem" || counts;
    const std::string fmt = "--tmp-format " + opt::tmp_format;
    if (in_memory && opt::load) throw std::invalid_argument("ERROR: " + fmt + " with --load: nothing would be left to compute from");
    if (in_memory && opt::keep_tmp) throw std::invalid_argument("ERROR: " + fmt + " with --keep_tmp: there are no temp files to keep");
    if (in_memory && opt::gpus > 1) throw std::invalid_argument("ERROR: " + fmt + " with --gpus above 1: the batches stay in the memory of one device");
    // (BVC_HOST_COUNTS_GROUPS=1 takes --group with counts; read here, where the refusal stands, in front of everything else the run reads)
    const bool counts_groups = counts && !opt::group.empty() && Knobs::counts_groups_on();
    if (counts && !opt::group.empty() && !counts_groups)
        throw std::invalid_argument("ERROR: --tmp-format counts with --group: the program calls the groups from kept batches only, use --tmp-format mem "
                                    "(or set BVC_HOST_COUNTS_GROUPS=1)");
    // (BVC_HOST_COUNTS_QUALS acts with counts only; a value that is no multiple of 4 in 4..128 is refused here, before anything is opened)
    if (counts && parse_counts_quals(getenv("BVC_HOST_COUNTS_QUALS")) < 0)
        throw std::invalid_argument("ERROR: BVC_HOST_COUNTS_QUALS must be a multiple of 4 in 4..128");
    // (BVC_HOST_COUNTS_LOAD and BVC_HOST_COUNTS_SAVE act with counts only; an empty name is refused here)
    {
        std::vector<std::string> files;
        if (counts && !parse_counts_load(getenv("BVC_HOST_COUNTS_LOAD"), files))
            throw std::invalid_argument("ERROR: BVC_HOST_COUNTS_LOAD must be FILE[:FILE...] without an empty name");
        if (counts && parse_counts_save(getenv("BVC_HOST_COUNTS_SAVE")) < 0) throw std::invalid_argument("ERROR: BVC_HOST_COUNTS_SAVE must name a file");
    }
    GroupFile group_file;
    if (counts_groups) {
        std::ifstream ifg(opt::group);
        std::string id, grp;
        while (ifg >> id >> grp) { group_file.ids.push_back(id); group_file.groups.push_back(grp); }
        std::vector<uint8_t> label;
        std::vector<int32_t> columns;
        counts_group_map(group_file.ids, group_file.groups, std::vector<std::string>(), group_file.names, label, columns);
        if (group_file.names.size() > BVC_MAX_GROUPS)
            throw std::invalid_argument("ERROR: --tmp-format counts with --group: " + std::to_string(group_file.names.size()) + " group names in " + opt::group +
                                        ", the counts pass keeps the depths of 32 at the most, use --tmp-format mem");
    }
    if (in_memory && opt::rerun) {
        std::cerr << "basetype: --rerun has nothing to reuse with " << fmt << ", it is ignored" << std::endl;
        opt::rerun = false;
    }
    const Knobs knobs(opt::thread);                                      // the environment, read once before any thread starts
    // (BVC_HOST_STORE_WINDOWS acts with --tmp-format mem only; refused before anything is read, made or written)
    if (in_memory && !counts && (knobs.store_windows < 0 || (knobs.store_windows > 0 && store_windows_refused(knobs.store_windows, std::max(1, opt::thread)))))
        throw std::invalid_argument("ERROR: BVC_HOST_STORE_WINDOWS must be auto or an integer K >= 1 with K x threads <= " +
                                    std::to_string(kStoreWindowsMaxThreads));
    if (opt::reference.empty()) throw std::invalid_argument("reference must be feed");
    time_t tim = time(0);
    const clock_t ctb = clock();
    std::cout << "basetype start -- " << ctime(&tim);
    std::vector<std::string> bams;
    { std::ifstream ibam(opt::input); std::string l; while (std::getline(ibam, l)) bams.push_back(l); }
    const int32_t N = (int32_t)bams.size();
    if (N == 0) throw std::invalid_argument("empty input list");
    std::string chr;
    int32_t rg_s, rg_e;
    const int32_t buf = 1000;
    std::tie(chr, rg_s, rg_e) = splitrg(opt::region);
    std::string refseq, err;
    if (!fetch_reference(opt::reference, chr, rg_s, rg_e + buf, refseq, err)) throw std::runtime_error(err);
    std::vector<int32_t> pv;
    for (size_t i = 0; i + buf < refseq.length(); ++i) {
        const char c = refseq[i];
        if (c == 'A' || c == 'C' || c == 'G' || c == 'T') pv.push_back((int32_t)i + rg_s);
    }
    const int thread = std::max(1, opt::thread);
    for (int i = 0; i < thread && !in_memory; ++i) {
        const std::string d = opt::output + ".tmp.thread." + std::to_string(i);
        if (::mkdir(d.c_str(), 0777) != 0 && !file_exists(d)) throw std::runtime_error("ERROR: fail to run mkdir");
    }
    const int bc = std::max(1, opt::batch);
    const int nb = 1 + (N - 1) / bc;
    std::vector<std::vector<std::string>> ftmp_vv((size_t)thread);
    int ngz = 0, bk = nb - 1;
    for (int j = 0; j < nb && !in_memory; ++j) {
        int k = 0;
        for (int i = 0; i < thread; ++i) {
            const std::string f = tmp_name(i, j);
            ftmp_vv[(size_t)i].push_back(f);
            if (file_exists(f)) {
                if (BgzfReader(f).is_bgzf()) { if (BgzfReader::has_eof_marker(f)) { k += 1; ngz += 1; } }
                else std::cerr << "warning: " << f << " is not bgziped" << std::endl;
            }
        }
        if (k != thread) bk = bk > j ? j : bk;
    }
    int first_batch = 0;
    bool extract = true;
    if (opt::rerun && ngz > 0) { extract = ngz != thread * nb; first_batch = bk; }
    int n_sub = thread;                                                  // the sub-files: one per compute thread (of every window)
    DeviceSlots slots(knobs.device_slots);
    std::mutex mu;
    std::string werr;                                                    // the first error of a compute thread (or of a window's loader)
    // The compute threads of the region, or of one position window: thread i works as thread sub0 + i of n_sub.  Every worker is joined
    // BEFORE anything can throw: unwinding past a joinable std::thread is std::terminate, which would lose the error text and leave the
    // other threads in the middle of their device calls.
    auto compute = [&](int sub0, const MemBatches *mem, int gpus, const CountsPass *cp) {
        std::vector<std::thread> workers;
        for (int i = 0; i < thread; ++i)
            workers.emplace_back([&, i]() {
                try { bt_s(mem ? std::vector<std::string>() : ftmp_vv[(size_t)i], cp ? cp->pvS : pv, refseq, chr, rg_s, N, n_sub, sub0 + i,
                           mem ? 0 : device_of_thread(i, gpus, opt::gpus), knobs, slots, mem, cp); }
                catch (const std::exception &e) { std::lock_guard<std::mutex> g(mu); if (werr.empty()) werr = e.what(); }
            });
        for (auto &w : workers) w.join();
    };
    double t_loaded = 0, t_joined = 0;
    if (counts) {
        std::cerr << "begin to extract reads from bam" << std::endl;
        if (basetype_counts(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, thread, knobs, counts_groups && !group_file.names.empty() ? &group_file : nullptr,
                            t_loaded, compute))
            return;                                                      // (BVC_HOST_COUNTS_SAVE: the counts analogue of --load -- nothing to compute or merge)
        t_joined = StageClock::now();
    } else if (in_memory) {
        std::cerr << "begin to extract reads from bam" << std::endl;
        basetype_in_memory(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, thread, knobs, n_sub, werr, mu, t_loaded, compute);
        t_joined = StageClock::now();
    } else if (extract) {
        std::cerr << "begin to extract reads from bam" << std::endl;
        if (knobs.device_pileup && opt::tmp_format != "text") {
            const int load_gpus = bvc_device_count();
            if (load_gpus <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
            run_pool(nb - first_batch, thread, [&](int t) { bt_r_device(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, first_batch + t, thread, load_gpus, false, knobs); });
            if (knobs.profile) std::cerr << "[profile] main: load phase on the device, " << g_device_batches.load() << " batches ("
                                         << (knobs.device_pileup_deflate && opt::tmp_format != "raw" ? "bvc_bam_pileup_bgzf_deflate" : "bvc_bam_pileup_bgzf") << ")" << std::endl;
        } else if (knobs.device_pileup_text && opt::tmp_format == "text") {
            const int load_gpus = bvc_device_count();
            if (load_gpus <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
            run_pool(nb - first_batch, thread, [&](int t) { bt_r_device(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, first_batch + t, thread, load_gpus, true, knobs); });
            if (knobs.profile) std::cerr << "[profile] main: load phase on the device, " << g_device_batches.load() << " batches ("
                                         << (knobs.device_pileup_deflate ? "bvc_bam_pileup_text_bgzf_deflate" : "bvc_bam_pileup_text_bgzf") << ")" << std::endl;
        } else
            run_pool(nb - first_batch, thread, [&](int t) { bt_r(bams, pv, refseq, chr, rg_s, rg_e, nb, bc, first_batch + t, thread); });
    }
    if (!in_memory) {
        time_t tim1 = time(0);
        t_loaded = StageClock::now();
        std::cout << "basetype loading done -- " << ctime(&tim1);
        if (opt::load) std::exit(EXIT_SUCCESS);
        const int gpus = bvc_device_count();
        if (gpus <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
        compute(0, nullptr, gpus, nullptr);
        t_joined = StageClock::now();
    }
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!werr.empty()) {
                for (int i = 0; i < n_sub; ++i) {                        // partial sub-files are of no use; the temp
                    std::remove((opt::output + "." + std::to_string(i) + ".vcf.gz").c_str());   // batches stay for --rerun
                    std::remove((opt::output + "." + std::to_string(i) + ".cvg.gz").c_str());
                }
                throw std::runtime_error(werr);
            }
        }
        // merge the per-thread sub-files in thread (= position) order (src/BaseVarC.cpp:268-296)
        BgzfWriter fov(opt::output + ".vcf.gz"), foc(opt::output + ".cvg.gz");
        if (!merge_subfiles(opt::output, ".vcf.gz", n_sub, fov) || !merge_subfiles(opt::output, ".cvg.gz", n_sub, foc))
            throw std::runtime_error("ERROR: fail to write");
        std::cout << "merge subfiles done" << std::endl;
        if (!fov.close()) std::cerr << "warning: file cannot be closed" << std::endl;
        if (!foc.close()) std::cerr << "warning: file cannot be closed" << std::endl;
        if (knobs.profile) {
            // CPU time the whole process has consumed so far (all threads, the HIP runtime's included): on a box that grants a quota of
            // CPUs this, not the thread count, is what the feed is bounded by
            struct rusage ru;
            getrusage(RUSAGE_SELF, &ru);
            const double cpu = (double)ru.ru_utime.tv_sec + 1e-6 * (double)ru.ru_utime.tv_usec + (double)ru.ru_stime.tv_sec + 1e-6 * (double)ru.ru_stime.tv_usec;
            std::cerr << "[profile] main: compute phase (threads) " << t_joined - t_loaded << " s, merge of sub-files "
                      << StageClock::now() - t_joined << " s; process CPU time " << cpu << " s (user "
                      << (double)ru.ru_utime.tv_sec + 1e-6 * (double)ru.ru_utime.tv_usec << ")" << std::endl;
        }
    }
    for (int i = 0; i < thread && !in_memory; ++i) ::rmdir((opt::output + ".tmp.thread." + std::to_string(i)).c_str());
    time_t tim2 = time(0);
    std::cout << "basetype computing done -- " << ctime(&tim2);
    std::cout << "basetype elapsed cpu secs : " << double(clock() - ctb) / CLOCKS_PER_SEC << std::endl;
    std::cout << "basetype done" << std::endl;
}

// ---- popmatrix (runPopMatrix, src/BaseVarC.cpp:671-729) -----------------------------------------------------------------------
// The rows of the BAMs in list order from the device (BVC_HOST_DEVICE_POPMATRIX): batches of `bc` samples, per batch the region's BGZF
// blocks gathered as phase 1 of basetype gathers them (bam_gather.h) and ONE library call; one context, one thread.  Returns the batches.
static long popmatrix_device(const std::vector<std::string> &bams, const std::vector<PosInfo> &pv, const std::string &chr, const std::string &rg,
                             int32_t rg_s, int32_t beg0, int32_t end0, int64_t refseq_len, int bc, BgzfWriter &fp)
{
    if (bvc_device_count() <= 0) throw std::runtime_error("ERROR: no gfx950 device (libbvc has no CPU fallback)");
    LoadDevice dev;
    if (bvc_create(&dev.ctx, device_of_thread(0, bvc_device_count(), opt::gpus)) != BVC_OK)
        throw std::runtime_error("ERROR: no usable gfx950 device for libbvc");
    const size_t M = pv.size();
    std::vector<int32_t> positions(M);
    std::vector<uint8_t> ref(M), alt(M), matrix;
    for (size_t t = 0; t < M; ++t) { positions[t] = pv[t].pos; ref[t] = (uint8_t)pv[t].ref; alt[t] = (uint8_t)pv[t].alt; }
    long batches = 0;
    std::string row;
    for (size_t b0 = 0, count = 0; b0 < bams.size(); b0 += (size_t)bc, ++batches) {
        const size_t b1 = std::min(bams.size(), b0 + (size_t)bc), ns = b1 - b0;
        BamBatch batch;
        batch.open(bams, b0, b1, chr);
        std::vector<uint32_t> status(ns);
        matrix.resize(ns * M);
        for (int attempt = 0;; ++attempt) {
            batch.gather(beg0, end0, attempt > 0, dev);
            const int rc = bvc_bam_popmatrix_bgzf(dev.ctx, (int32_t)ns, dev.pin, batch.comp_bytes, batch.table.data(), (int64_t)batch.table.size(),
                                                  batch.out_bytes, batch.off.data(), batch.end.data(), batch.eof.data(), batch.rid.data(), beg0, end0,
                                                  opt::mapq, (int32_t)M, positions.data(), ref.data(), alt.data(), rg_s, refseq_len, matrix.data(),
                                                  (int64_t)M, status.data());
            if (rc == BVC_OK) break;
            if (rc == BVC_BAM_MORE && attempt == 0) {                 // a list that stopped short of its region's end: that sample to the file's end, once
                batch.mark_short(status);
                continue;
            }
            if (rc == BVC_ERR_DATA)
                for (size_t s = 0; s < ns; ++s) {
                    // the messages of the CPU path: fetch's, and fetch_allele_type's std::out_of_range
                    if (status[s] == 3u) throw std::runtime_error("ERROR: truncated or corrupt BAM record in " + bams[b0 + s]);
                    if (status[s] == 4u) throw std::out_of_range("index offset is out of range of the sequence");
                }
            throw std::runtime_error(std::string("ERROR: device popmatrix failed: ") + bvc_last_error(dev.ctx));
        }
        for (size_t s = 0; s < ns; ++s) {
            if (!(++count % 1000)) std::cerr << "Processing the number " << count / 1000 << "k bam" << std::endl;
            if (batch.rid[s] < 0) std::cerr << batch.sms[s] << ": region " << rg << " is empty." << std::endl;
            row.assign(reinterpret_cast<const char *>(matrix.data()) + s * M, M);
            row += "\n";
            fp.write(row);
        }
    }
    return batches;
}

static void run_popmatrix(int argc, char **argv)
{
    parse_options(argc, argv, POPMATRIX_MESSAGE);
    if (opt::reference.empty() || opt::posfile.empty()) throw std::invalid_argument(POPMATRIX_MESSAGE);
    std::cerr << "popmatrix start" << std::endl;
    const clock_t ctb = clock();
    std::ifstream ibam(opt::input);
    std::vector<PosInfo> pv;
    if (!ibam.is_open() || !read_posfile(opt::posfile, pv)) throw std::runtime_error("ERROR: bamlist or posifle fail to be opend");
    std::vector<std::string> bams;
    for (std::string l; std::getline(ibam, l);) bams.push_back(l);
    if (pv.empty()) throw std::invalid_argument("ERROR: no position in " + opt::posfile);   // (the reference takes front() of an empty vector)
    const size_t N = bams.size(), M = pv.size();
    BgzfWriter fp(opt::output);
    if (!fp.ok()) throw std::runtime_error("ERROR: fail to write");
    fp.write(std::to_string(N) + "\t" + std::to_string(M) + "\n");
    const std::string rg = posfile_region(pv);
    std::string chr;
    int32_t rg_s, rg_e;
    std::tie(chr, rg_s, rg_e) = splitrg(rg);
    std::string refseq, err;
    // (only its length reaches the rule, but the reference fetches it and fails where it cannot)
    if (!fetch_reference(opt::reference, chr, rg_s, rg_e + 1000, refseq, err)) throw std::runtime_error(err);
    // the region padded by 1000 on both sides (gr.Pad(1000), src/BamProcess.cpp:290), as bt_r has it; [beg, end) 0-based
    const int32_t beg0 = std::max(0, rg_s - 1 - 1000), end0 = rg_e + 1000;
    const Knobs knobs(1);
    bool device = knobs.device_popmatrix;
    if (device && !positions_do_not_descend(pv)) {
        std::cerr << "popmatrix: the position file is not sorted, the rows are made on the CPU" << std::endl;
        device = false;
    }
    long batches = 0;
    if (device)
        batches = popmatrix_device(bams, pv, chr, rg, rg_s, beg0, end0, (int64_t)refseq.size(), opt::batch_given ? std::max(1, opt::batch) : 100, fp);
    else
        for (size_t i = 0, count = 0; i < N; ++i) {
            if (!(++count % 1000)) std::cerr << "Processing the number " << count / 1000 << "k bam" << std::endl;
            fp.write(popmatrix_row(bams[i], chr, rg, beg0, end0, opt::mapq, rg_s, refseq, pv) + "\n");
        }
    if (knobs.profile) std::cerr << "[profile] main: popmatrix on the device, " << batches << " batches (bvc_bam_popmatrix_bgzf)" << std::endl;
    if (!fp.close()) std::cerr << "warning: fail to close file" << std::endl;
    std::cout << "elapsed secs : " << double(clock() - ctb) / CLOCKS_PER_SEC << std::endl;
    std::cerr << "popmatrix done" << std::endl;
}

static void run_concat(int argc, char **argv)                            // runConcat, src/BaseVarC.cpp:731-795
{
    parse_options(argc, argv, CONCAT_MESSAGE);
    const clock_t ctb = clock();
    concat_matrices(opt::input, opt::output);                           // (-o is opened as given: the reference adds no ".gz" either)
    std::cout << "elapsed secs : " << double(clock() - ctb) / CLOCKS_PER_SEC << std::endl;
    std::cout << "concat done" << std::endl;
}

int main(int argc, char **argv)
{
    if (argc <= 1) { std::cerr << BASEVARC_USAGE_MESSAGE; return 0; }
    // every thread drives the device through a stream of its own: as many hardware queues as threads that may be inside the device's
    // part of a tile at a time (the runtime's default is four, two streams then share a queue; profiles/r05_host/README.txt)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    const std::string command(argv[1]);
    try {
        if (command == "basetype") run_basetype(argc - 1, argv + 1);
        else if (command == "popmatrix") run_popmatrix(argc - 1, argv + 1);
        else if (command == "concat") run_concat(argc - 1, argv + 1);
        else { std::cerr << BASEVARC_USAGE_MESSAGE; return 0; }
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}
