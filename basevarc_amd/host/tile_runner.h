// tile_runner.h -- a phase-2 thread's tiles of positions and the three stages they pass through: parsed or staged (stage 1), handed to
// libbvc (stage 2), written out as CVG and VCF lines (stage 3).  Included by main.cpp alone: what is here calls libbvc.
#ifndef BVC_HOST_TILE_RUNNER_H
#define BVC_HOST_TILE_RUNNER_H

#include <atomic>
#include <functional>
#include <future>
#include <iostream>
#include <map>
#include <thread>

#include "batches.h"
#include "knobs.h"
#include "tile.h"

namespace bvchost {

struct TileRunner {
    const Knobs &knobs;
    explicit TileRunner(const Knobs &k) : knobs(k) {}
    StageClock clk;                      // stage 1 (the caller's thread): read, parse
    StageClock clk_dev, clk_out;         // stage 2: pack, gpu; stage 3: cvg, vcf, write
    bvc_ctx *ctx = nullptr;
    const Groups *groups = nullptr;
    std::string chr;
    int32_t n_samples = 0, ithread = 0;
    double min_af = 0;
    BgzfWriter *fvcf = nullptr, *fcvg = nullptr;

    static const int kTiles = 3;
    Tile tiles[kTiles];
    Tile *cur = nullptr;                 // the tile stage 1 is filling
    TileQueue free_q, dev_q, out_q;
    std::thread dev_thread, out_thread;
    std::mutex err_mu;
    std::string err;                     // first failure of stage 2 or 3
    bool started = false;
    int64_t tiles_one_byte = 0, tiles_two_byte = 0;   // library calls by tile form (stage 2's thread; read after finish())
    int64_t tiles_dev_stats = 0;                      // of the tiles parsed on the device: those whose called positions' statistics the device computed
    int64_t tiles_dev_samples = 0;                    // ... and whose called positions' sample columns the device formatted
    int64_t tiles_dev_deflate = 0;                    // ... and deflated
    int64_t tiles_dev_parsed = 0, tiles_cpu_parsed = 0;   // tiles of text or records: parsed on the device / handed back (a line was not regular)
    std::vector<int32_t> sample0, n_in_batch;         // per temp batch: its first sample and its samples (device-parsed tiles)
    uint8_t carry[5] = {0, 0, 0, 0, 0};               // the parser's long-lived AlleleInfo between tiles (stage 2's thread)
    std::atomic<int64_t> sites_done{0};
    // --tmp-format counts: the tiles hold the revisited positions alone; called with a position before its lines are written (and by the
    // caller with the window's end once the tiles are through), it writes the CVG lines of the positions in between from their tallies
    std::function<void(int32_t)> before_pos;

    void fail(const std::string &what)
    {
        { std::lock_guard<std::mutex> g(err_mu); if (err.empty()) err = what; }
        // let every stage run dry: tiles still flow back to the parser, which sees the error at its next flush
    }
    bool failed() { std::lock_guard<std::mutex> g(err_mu); return !err.empty(); }
    // stage 1 throws the first failure of a later stage
    void rethrow_if_failed()
    {
        std::lock_guard<std::mutex> g(err_mu);
        if (!err.empty()) throw std::runtime_error(err);
    }

    void start()
    {
        for (int i = 0; i < kTiles; ++i) free_q.push(&tiles[i]);
        cur = free_q.pop();
        dev_thread = std::thread([this] {
            for (Tile *t; (t = dev_q.pop()) != nullptr;) {
                if (!failed()) { try { if (t->form == TileForm::Sites) run_device(*t); else run_device_parsed(*t); } catch (const std::exception &e) { fail(e.what()); } }
                out_q.push(t);
            }
            out_q.close();
        });
        out_thread = std::thread([this] {
            for (Tile *t; (t = out_q.pop()) != nullptr;) {
                if (!failed()) { try { write_out(*t); } catch (const std::exception &e) { fail(e.what()); } }
                t->reset();
                free_q.push(t);
            }
        });
        started = true;
    }

    SiteColumn &slot() { return cur->slot(); }

    // stage 1 hands its tile on and takes a free one (waits when both later stages are still busy)
    void flush()
    {
        if (cur->empty()) return;
        dev_q.push(cur);
        cur = free_q.pop();
        rethrow_if_failed();
    }

    // end of the window: drain the pipeline; rethrows the first failure of a later stage
    void finish()
    {
        if (!started) return;
        if (cur && !cur->empty()) dev_q.push(cur);
        dev_q.close();
        dev_thread.join();
        out_thread.join();
        started = false;
        rethrow_if_failed();
    }
    ~TileRunner()
    {
        if (started) { dev_q.close(); dev_thread.join(); out_thread.join(); }
    }

    // A tile whose lines are in T.text / T.line_start through the reference's own rules (strtok_r, atoi) on the CPU, position by position,
    // batch by batch; then the ragged call.  (A line of the tile is not what the reference's writer produces.)
    void cpu_parse_tile(Tile &T)
    {
        const double t0 = StageClock::now();
        tiles_cpu_parsed += 1;
        T.handed_back = true;
        T.called_from = CalledFrom::HostEntries;
        set_parser_carry(carry);
        const size_t nb = sample0.size();
        for (size_t t = 0; t < T.n_pos; ++t) {
            SiteColumn &site = T.slot();
            site.clear();
            site.pos = T.pos[t];
            int32_t j = 0;
            for (size_t b = 0; b < nb; ++b) {
                const uint32_t s0 = T.line_start[b * (T.n_pos + 1) + t], s1 = T.line_start[b * (T.n_pos + 1) + t + 1];
                j += parse_pileup_line(T.text.data() + s0, (size_t)(s1 - s0 - 1), j, site);
            }
            if (!site.aiv.empty()) { T.refs[T.n_used] = T.refs[t]; ++T.n_used; }
        }
        T.refs.resize(T.n_used);
        get_parser_carry(carry);
        clk_dev.pack += StageClock::now() - t0;
        if (T.n_used) run_device(T);
    }

    // One of the bvc_pileup_finish* calls: the arguments they all begin with, then `tail`, the call's own.
    template <class Fn, class... Tail>
    int finish_call(Fn fn, Tile &T, uint8_t carry_out[5], Tail... tail)
    {
        const int ng = groups ? (int)groups->names.size() : 0;
        return fn(ctx, T.refs.data(), min_af, carry, carry_out, ng ? groups->of_sample.data() : nullptr,
                  ng ? (int64_t)groups->of_sample.size() : 0, ng, T.entry_off.data(), T.tally.data(), tail...);
    }

    // bvc_pileup_finish into the tile's arrays (after a begin that returned BVC_OK).  text_on_device: the indel tokens' text comes back
    // in T.text (the tile's own text never was on the host).
    void finish_tile(Tile &T, int64_t n_ent, int64_t n_ind, int64_t ind_bytes, bool text_on_device)
    {
        const int ng = groups ? (int)groups->names.size() : 0;
        T.entry_off.resize(T.n_pos + 1);
        T.tally.resize(T.n_pos * 32);
        T.ent.resize((size_t)n_ent + 1);
        T.samples.resize((size_t)n_ent + 1);
        T.indels.resize((size_t)n_ind + 1);
        T.res.resize(T.n_pos);
        T.gres.resize(T.n_pos * (size_t)ng);
        if (text_on_device) T.text.resize((size_t)ind_bytes + 1);
        char *const ind_text = text_on_device ? T.text.data() : nullptr;
        bvc_group_result *const gres = ng ? T.gres.data() : nullptr;
        uint8_t carry_out[5];
        int rc;
        T.stats.clear();
        T.called_from = !knobs.called_only ? CalledFrom::HostEntries : !knobs.device_samples ? CalledFrom::HostCalledEntries
                        : knobs.device_deflate ? CalledFrom::DeviceBlocks : CalledFrom::DeviceText;
        if (T.called_from == CalledFrom::DeviceText || T.called_from == CalledFrom::DeviceBlocks) {
            // no entry comes back: the statistics with the records, then the called positions' sample columns as text or as blocks
            T.stats.resize(T.n_pos);
            rc = finish_call(bvc_pileup_finish_called_text, T, carry_out, T.indels.data(), ind_text, T.res.data(), gres, T.stats.data());
            bvc_check(ctx, rc);
            const bool deflate = T.called_from == CalledFrom::DeviceBlocks;
            int64_t need = 0;
            for (size_t t = 0; t < T.n_pos; ++t)
                if (T.res[t].called) {
                    const int64_t slot = bvc_vcf_samples_slot(n_samples, T.entry_off[t + 1] - T.entry_off[t]);
                    need += deflate ? bvc_bgzf_bound(slot) : slot;
                }
            T.vout.reserve((size_t)need);                                // the text, or its blocks
            T.vtext_len.resize(T.n_pos + 1);                             // (sized as the offsets are; the calls fill n_pos of it)
            if (deflate) {
                T.vcomp_off.resize(T.n_pos + 1);
                rc = bvc_pileup_sample_bgzf(ctx, n_samples, T.vout.data(), (int64_t)T.vout.cap, T.vcomp_off.data(), T.vtext_len.data());
                tiles_dev_deflate += 1;
            } else {
                T.vtext_off.resize(T.n_pos + 1);
                rc = bvc_pileup_sample_text(ctx, n_samples, reinterpret_cast<char *>(T.vout.data()), (int64_t)T.vout.cap, T.vtext_off.data(),
                                            T.vtext_len.data());
            }
            tiles_dev_samples += 1;
        } else if (T.called_from == CalledFrom::HostCalledEntries) {
            T.called_off.resize(T.n_pos + 1);
            if (knobs.device_stats) T.stats.resize(T.n_pos);
            rc = finish_call(bvc_pileup_finish_called_stats, T, carry_out, T.called_off.data(), n_ent, T.ent.data(), T.samples.data(),
                             T.indels.data(), ind_text, T.res.data(), gres, T.stats.empty() ? nullptr : T.stats.data());
        } else {
            rc = finish_call(bvc_pileup_finish, T, carry_out, T.ent.data(), T.samples.data(), T.indels.data(), ind_text, T.res.data(), gres);
        }
        bvc_check(ctx, rc);
        std::memcpy(carry, carry_out, 5);
        T.indels.resize((size_t)n_ind);
        std::sort(T.indels.begin(), T.indels.end(), [](const bvc_pileup_indel &a, const bvc_pileup_indel &b) { return a.entry < b.entry; });
        tiles_dev_parsed += 1;
        if (!T.stats.empty()) tiles_dev_stats += 1;
    }

    // stage 2 of a tile of TEXT or of binary RECORDS: parse and LRT on the device.  Text goes to the CPU parser when a line is not what
    // the writer produces; a record that does not add up is an error (the CPU parser would refuse it too: binary records have no
    // second meaning)
    void run_device_parsed(Tile &T)
    {
        const double t0 = StageClock::now();
        const bool records = T.form == TileForm::Records;
        int64_t n_ent = 0, n_ind = 0;
        const int rc = records ? bvc_pileup_begin_bin(ctx, reinterpret_cast<const uint8_t *>(T.text.data()), (int64_t)T.text.size(), T.line_start.data(),
                                                      sample0.data(), n_in_batch.data(), (int32_t)sample0.size(), (int32_t)T.n_pos, &n_ent, &n_ind)
                               : bvc_pileup_begin(ctx, T.text.data(), (int64_t)T.text.size(), T.line_start.data(), sample0.data(), n_in_batch.data(),
                                                  (int32_t)sample0.size(), (int32_t)T.n_pos, &n_ent, &n_ind);
        if (!records && rc == BVC_PILEUP_IRREGULAR) { cpu_parse_tile(T); return; }
        if (records && rc == BVC_ERR_DATA) throw std::runtime_error(std::string("ERROR: malformed temp batch record (") + bvc_last_error(ctx) + ")");
        bvc_check(ctx, rc);
        finish_tile(T, n_ent, n_ind, 0, false);
        clk_dev.gpu += StageClock::now() - t0;
    }

    // stage 2: the tile in the form libbvc takes (pack_ragged; with groups pack_dense: columns are the samples ordered by group, the
    // group of each column is shared by all sites), and the call.  BVC_HOST_TWO_BYTE_TILES=1 forces the two-byte form.
    void run_device(Tile &T)
    {
        const int64_t ns = (int64_t)T.n_used;
        T.res.resize((size_t)ns);
        const int ng = groups ? (int)groups->names.size() : 0;
        const int64_t stride = ((int64_t)n_samples + 127) / 128 * 128;
        static const int8_t none = 0;                                    // (what an empty ragged tile points at)
        PackedTile &in = T.in;
        int rc;
        double t0 = StageClock::now();
        const bool fits = ng == 0 ? pack_ragged(T.sites.data(), T.n_used, knobs.two_byte_tiles, in)
                                  : pack_dense(T.sites.data(), T.n_used, stride, groups->column_of.data(), knobs.two_byte_tiles, in);
        if (ng) T.gres.resize((size_t)(ns * ng));
        (fits ? tiles_one_byte : tiles_two_byte) += 1;
        const double t1 = StageClock::now();
        clk_dev.pack += t1 - t0; t0 = t1;
        if (ng == 0 && fits)
            rc = bvc_lrt_csr_packed(ctx, ns, in.offsets.data(), in.packed.empty() ? reinterpret_cast<const uint8_t *>(&none) : in.packed.data(),
                                    T.refs.data(), min_af, T.res.data(), BVC_PTR_HOST);
        else if (ng == 0)
            rc = bvc_lrt_csr(ctx, ns, in.offsets.data(), in.bases.empty() ? &none : in.bases.data(), in.quals.empty() ? &none : in.quals.data(),
                             T.refs.data(), min_af, T.res.data(), BVC_PTR_HOST);
        else if (fits)
            rc = bvc_lrt_dense_groups_packed(ctx, ns, n_samples, stride, in.packed.data(), T.refs.data(), min_af, groups->of_column.data(), ng,
                                             T.res.data(), T.gres.data(), BVC_PTR_HOST);
        else
            rc = bvc_lrt_dense_groups(ctx, ns, n_samples, stride, in.bases.data(), in.quals.data(), T.refs.data(), min_af,
                                      groups->of_column.data(), ng, T.res.data(), T.gres.data(), BVC_PTR_HOST);
        bvc_check(ctx, rc);
        clk_dev.gpu += StageClock::now() - t0;
    }

    // stage 3: the CVG line of every position, the VCF line of every called one (bt_f, src/BaseVarC.cpp:548-666)
    void write_out(Tile &T) { if (T.device_parsed()) write_device_parsed(T); else write_sites(T); }

    // What both writers end a position with: its CVG line (formatted since t0) written; where it is called its VCF line -- vcf_line()
    // formats it or has it ready -- written, with the finished BGZF blocks of its sample columns and the newline where they are apart.
    template <class VcfLine>
    void write_lines(double &t0, const std::string &cl, bool called, VcfLine vcf_line, const unsigned char *blocks = nullptr, size_t n_blocks = 0)
    {
        StageClock &c = clk_out;
        double t1 = StageClock::now(); c.cvg += t1 - t0; t0 = t1;
        fcvg->write(cl);
        t1 = StageClock::now(); c.write += t1 - t0; t0 = t1;
        if (!called) return;
        const std::string vl = vcf_line();
        t1 = StageClock::now(); c.vcf += t1 - t0; t0 = t1;
        fvcf->write(vl);
        if (blocks) { fvcf->write_blocks(blocks, n_blocks); fvcf->write("\n", 1); }
        t1 = StageClock::now(); c.write += t1 - t0; t0 = t1;
    }

    // a tile the device parsed: the position's slice of the arrays it returned; its tallies (src/BaseVarC.cpp:560-590) from the 32 counters
    void write_device_parsed(Tile &T)
    {
        const int ng = groups ? (int)groups->names.size() : 0;
        double t0 = StageClock::now();
        size_t ii = 0;                                   // next indel record (sorted by entry)
        std::vector<std::string> ind_text;
        // the VCF lines of the tile's called positions -- one field per SAMPLE each, ~1 ms to format at 1e5 samples -- ahead of the
        // loop, on this thread and two more where the CPUs allow (vcf_line reads the position's entries and its record only)
        std::vector<size_t> called_t;
        for (size_t t = 0; t < T.n_pos; ++t) if (T.res[t].called && T.entry_off[t + 1] > T.entry_off[t]) called_t.push_back(t);
        std::vector<std::string> vcf_pre(called_t.size());
        auto format_share = [&](size_t k0, size_t k1) {
            for (size_t k = k0; k < k1; ++k) {
                const size_t t = called_t[k];
                std::map<std::string, std::string> info;
                if (ng) group_af_info(T.res[t], &T.gres[t * (size_t)ng], *groups, info);
                if (T.called_from == CalledFrom::DeviceBlocks) {
                    // the line around columns that are not here: everything in front of them; their blocks and the newline follow below
                    vcf_pre[k] = vcf_line(T.res[t], chr, T.pos[t], T.refs[t], T.stats[t], info, "", 0);
                    vcf_pre[k].pop_back();
                } else if (T.called_from == CalledFrom::DeviceText)
                    vcf_pre[k] = vcf_line(T.res[t], chr, T.pos[t], T.refs[t], T.stats[t], info, reinterpret_cast<const char *>(T.vout.data()) + T.vtext_off[t], (size_t)T.vtext_len[t]);
                else
                    vcf_pre[k] = vcf_line(T.res[t], chr, T.refs[t], T.view(t), info, n_samples);
            }
        };
        {
            const size_t nc = called_t.size();
            const size_t shares = (nc >= 3 && knobs.cpus_per_loop >= 4) ? 3 : 1;
            std::vector<std::future<void>> helpers;
            for (size_t h = 1; h < shares; ++h)
                helpers.push_back(std::async(std::launch::async, format_share, nc * h / shares, nc * (h + 1) / shares));
            format_share(0, nc / shares);
            for (auto &f : helpers) f.get();
            const double t1 = StageClock::now(); clk_out.vcf += t1 - t0; t0 = t1;
        }
        size_t next_called = 0;
        for (size_t t = 0; t < T.n_pos; ++t) {
            const int64_t e0 = T.entry_off[t], e1 = T.entry_off[t + 1];
            if (before_pos) before_pos(T.pos[t]);
            if (e1 == e0) continue;                      // no entry: the reference skips the position (:443)
            const int32_t *ta = &T.tally[t * 32];
            int32_t cnt[4], fwd[8], rev[8];
            for (int b = 0; b < 8; ++b) { rev[b] = ta[b] + ta[16 + b]; fwd[b] = ta[8 + b] + ta[24 + b]; }
            for (int b = 0; b < 4; ++b) cnt[b] = ta[b] + ta[8 + b];
            ind_text.clear();
            for (; ii < T.indels.size() && T.indels[ii].entry < e1; ++ii)
                ind_text.emplace_back(T.text.data() + T.indels[ii].text_off, (size_t)T.indels[ii].len);
            SiteView v = T.view(t);             // (a position that is not called: the CVG line reads the tallies and the indel strings only)
            v.cnt = cnt; v.fwd = fwd; v.rev = rev;
            v.indels = ind_text.data(); v.n_indels = ind_text.size();
            const bool called = T.res[t].called != 0, blocks = called && T.called_from == CalledFrom::DeviceBlocks;
            write_lines(t0, cvg_line(chr, T.refs[t], v, ng ? &T.gres[t * (size_t)ng] : nullptr, ng), called,
                        [&] { return std::move(vcf_pre[next_called++]); }, blocks ? T.vout.data() + T.vcomp_off[t] : nullptr,
                        blocks ? (size_t)(T.vcomp_off[t + 1] - T.vcomp_off[t]) : 0);
            const int64_t done = ++sites_done;
            if (!(done % 1000)) std::cerr << "basetype completed " << done << " sites -- thread" << ithread << std::endl;
        }
    }

    // a tile of the CPU parser's columns
    void write_sites(Tile &T)
    {
        const int ng = groups ? (int)groups->names.size() : 0;
        double t0 = StageClock::now();
        for (size_t s = 0; s < T.n_used; ++s) {
            const bvc_group_result *g = ng ? &T.gres[s * (size_t)ng] : nullptr;
            write_lines(t0, cvg_line(chr, T.sites[s].pos, T.refs[s], T.sites[s], g, ng), T.res[s].called != 0, [&] {
                std::map<std::string, std::string> info;
                if (ng) group_af_info(T.res[s], g, *groups, info);
                return vcf_line(T.res[s], chr, T.sites[s].pos, T.refs[s], T.sites[s], info, n_samples);
            });
        }
    }
};

}  // namespace bvchost
#endif
