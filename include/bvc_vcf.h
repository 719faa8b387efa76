/*
 * bvc_vcf.h -- C ABI of libbvc, second header: the sample columns of the called positions' VCF lines formatted on the device.
 * Everything of bvc.h (conventions, records, contexts, flags) holds here; the entry points below are exported by the same library.
 * They have a header of their own because bvc.h's list of entry points is closed: its bindings are generated from, and checked
 * against, that list.
 */
#ifndef BVC_VCF_H
#define BVC_VCF_H

#include "bvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Additive: the SAMPLE COLUMNS of a called position's VCF line (WriteVcf, src/BaseType.cpp:187-212: one GT:AB:SO:BP field per sample,
 * 400 KB per position at 1e5 samples) formatted on the device from the position's entries and the sample each belongs to.  The text is,
 * byte for byte, what the host program's vcf_line puts behind "GT:AB:SO:BP\t" (host/pileup.cpp):
 *   - the entries count up to the first k with samples[k] < (one past the previous entry's sample, 0 at the start) or samples[k] outside
 *     0 .. n_samples - 1; that entry and all behind it are ignored.  Indel entries and N bases are formatted like any other entry
 *   - a sample without an entry is "./."; a sample with one is "g:B:S:d.dddddd": g = "0/." where base == ref_base[s] (as ints: a
 *     negative ref_base matches nothing), else "./i" with i - 1 the LAST index below n_alt (n_alt > 3 is read as 3) whose
 *     alt_base & 7 equals the base, else "./."; B = "ACGTNN"[min(base, 5)]; S = "-+"[strand & 1]; d.dddddd = 1 - 10^(-qual / 10) as %.6f
 *     (the 256 strings of bvc_vcf_bp_lut).  The base is read & 7
 *   - fields are separated by tabs: n_samples fields, text_len = max(0, 4 * n_samples + 13 * (entries that count) - 1) bytes
 * Layout: site s has a slot iff results[s].called != 0, of bvc_vcf_samples_slot(n_samples, offsets[s + 1] - offsets[s]) bytes, the slots
 * one after the other in site order from byte 0 of `text`: text_off [n_sites + 1] are their starts (text_off[n_sites] = their sum, which
 * text_cap must reach), text_len [n_sites] the bytes of text in each (0 for a site that is not called).  The bytes of a slot behind its
 * text are unspecified; nothing outside the slots is written.
 * Host or device pointers (flags), as bvc_site_stats_csr: of `results` called, n_alt and alt_base are read and must be complete (overlap
 * mode: bvc_join first).  Device `entries` / `samples` may start at any element, device `text` must start on a 16-byte boundary (the text
 * is written with 16-byte stores); the device form waits once, for the sum of the slots, before it formats (asynchronously).  With host
 * pointers the small arrays are staged through the context's page-locked buffer, the entries and samples go up from the caller's memory
 * as it is and the text comes down straight into it (a DMA where that is bvc_host_alloc memory).  BVC_ERR_ARG: null pointers with work
 * present, a negative n_sites, n_samples or text_cap, host offsets that do not start at 0 or that decrease, a text_cap smaller than the sum
 * of the slots (bvc_last_error names the need; with host pointers nothing has been launched, with either the context stays usable).
 */
/* Bytes of a called site's slot, for callers to size `text`: 4 * n_samples + 13 * n_entries rounded up to 16. */
static inline int64_t bvc_vcf_samples_slot(int64_t n_samples, int64_t n_entries)
{
    return (4 * n_samples + 13 * n_entries + 15) / 16 * 16;
}
/* The eight characters d.dddddd for quality q at out[8 * q], q = 0..255.  Needs no context and no device. */
void bvc_vcf_bp_lut(char out[2048]);
int bvc_vcf_samples_csr(bvc_ctx *ctx, int64_t n_sites, const int64_t *offsets, const bvc_pileup_entry *entries,
                        const int32_t *samples, const int8_t *ref_base, const bvc_site_result *results, int64_t n_samples,
                        char *text, int64_t text_cap, int64_t *text_off, int64_t *text_len, uint32_t flags);
/*
 * The same behind the producer calls.  bvc_pileup_finish_called_text is bvc_pileup_finish_called_stats without the gather and the
 * download of the called positions' entries and samples (stats is required): one wait.  It leaves the tile's columns and records on
 * the device, and until the next bvc_pileup_begin* on the context bvc_pileup_sample_text formats the called positions' sample columns
 * from them: text / text_off / text_len as above (host pointers), n_positions sites.  The caller sizes `text` from entry_off, results
 * and bvc_vcf_samples_slot; a text_cap that is too small is BVC_ERR_ARG (bvc_last_error names the need) and consumes nothing: the call
 * may be repeated with a larger buffer -- as it may be repeated anyway.  bvc_pileup_sample_text without a preceding
 * bvc_pileup_finish_called_text, or after the next begin: BVC_ERR_ARG.  One wait; the text comes straight into the caller's memory.
 */
int bvc_pileup_finish_called_text(bvc_ctx *ctx, const int8_t *ref_base, double min_af, const uint8_t carry_in[5], uint8_t carry_out[5],
                                  const uint8_t *group_of_sample, int64_t n_samples, int32_t n_groups,
                                  int64_t *entry_off, int32_t *tally, bvc_pileup_indel *indels, char *indel_text,
                                  bvc_site_result *results, bvc_group_result *grp_results, bvc_site_stats *stats);
int bvc_pileup_sample_text(bvc_ctx *ctx, int64_t n_samples, char *text, int64_t text_cap, int64_t *text_off, int64_t *text_len);

#ifdef __cplusplus
}
#endif
#endif /* BVC_VCF_H */
