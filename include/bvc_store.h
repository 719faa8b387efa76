/*
 * bvc_store.h -- C ABI of libbvc, sixth header: temp batches that never leave the device.  Phase 1 of `BaseVarC basetype` leaves a batch's
 * binary records in device memory (a store), phase 2 makes its tiles of positions out of all kept batches there.  Everything of bvc.h
 * (conventions, contexts, return codes) holds here; the entry points below are exported by the same library.  A header of its own because
 * bvc.h's list of entry points is closed (bvc_bam.h's opening comment).
 */
#ifndef BVC_STORE_H
#define BVC_STORE_H

#include "bvc_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A store: n_batches batches of the binary temp-batch records of bvc_pileup_begin_bin (bvc_bam.h has the record's form), each of the same
 * n_positions positions, on ONE device.  A batch is its n_positions + 1 words of rec_start and its records, in a device allocation of
 * its own of exactly that size.  A store belongs to no context: phase 1 fills it through several threads' contexts, phase 2 reads it through
 * others; all of them must be contexts of the store's device (else BVC_ERR_ARG).  The store's bookkeeping is under a mutex: puts of
 * DIFFERENT batches may run at the same time from different contexts and threads, and so may bvc_pileup_begin_store calls once the store
 * is sealed.  A store must outlive every call that names it.
 *
 * Life: create -> every batch put once (bvc_store_put / bvc_bam_pileup_bgzf_store, any order) -> bvc_store_seal -> bvc_store_tile +
 * bvc_pileup_begin_store, any number of times -> destroy.
 */
typedef struct bvc_store bvc_store;

/* bytes of a batch's slice that one work item of the gather kernel copies (store_kernel.hip); the tests straddle it */
#define BVC_STORE_CHUNK 16384

/*
 * byte_budget: the most device memory the batches may take together (what bvc_store_bytes reports as used); <= 0: no cap but the
 * device's.  BVC_ERR_ARG: null out, negative sizes.  BVC_ERR_DEVICE / BVC_ERR_ALLOC: the device cannot be used.
 */
int bvc_store_create(bvc_store **out, int device, int32_t n_positions, int32_t n_batches, int64_t byte_budget);
/* frees the batches; null is ignored.  No call that names the store may be running */
void bvc_store_destroy(bvc_store *st);

/*
 * Puts batch `batch` from host memory: records_bytes bytes of records of n_in_batch samples and rec_start [n_positions + 1] (record t
 * begins -- at its length word -- at rec_start[t]; bytes in front of rec_start[0] and between nothing are allowed, they are kept and never
 * read).  The row is checked as bvc_pileup_begin_bin checks one: records ascend, each holds its length word and is as long as that
 * word says, all lie inside records_bytes (BVC_ERR_ARG).  BVC_ERR_ARG too: a batch index outside the store, a batch that has been put
 * (or is being put), a put after bvc_store_seal, n_in_batch < 0, records_bytes > 0xFFFFFF00, a context of another device.
 * BVC_ERR_ALLOC: the batch would pass byte_budget (bvc_last_error names both numbers) or the device has no room; the store stays usable
 * and the batch may be put again.  The batch is complete on the device when the call returns (it waits for the context's stream).
 */
int bvc_store_put(bvc_ctx *ctx, bvc_store *st, int32_t batch, int32_t n_in_batch, const uint8_t *records, int64_t records_bytes,
                  const uint32_t *rec_start);

/*
 * bvc_bam_pileup_bgzf (bvc_bam.h), but the records and rec_start stay on the device as batch `batch` of the store (n_samples is its
 * n_in_batch; n_positions must be the store's).  The arguments up to refseq_len, sample_status, *records_needed (named records_bytes
 * here), the statuses, BVC_BAM_MORE for a sample of status 2 and BVC_ERR_DATA are that call's; there is no records_cap, so BVC_BAM_MORE
 * never asks for room.  Only BVC_OK puts anything: after every other return the store is as it was.  The refusals of bvc_store_put hold
 * (the budget is checked once the size is known: between the call's two passes).  Complete on the device when it returns.
 */
int bvc_bam_pileup_bgzf_store(bvc_ctx *ctx, int32_t n_samples, const uint8_t *comp, int64_t comp_bytes, const bvc_bgzf_block *blocks,
                              int64_t n_blocks, int64_t bam_bytes, const int64_t *sample_off, const int64_t *sample_end,
                              const uint8_t *sample_eof, const int32_t *rid, int32_t beg0, int32_t end0, int32_t min_mapq,
                              int32_t n_positions, const int32_t *positions, int32_t rg_s, const char *refseq, int64_t refseq_len,
                              bvc_store *st, int32_t batch, int64_t *records_bytes, uint32_t *sample_status);

/*
 * A kept batch back on the host, in two steps like bvc_pileup_text: *records_needed is always set; with records == NULL and rec_start == NULL
 * nothing else happens; else records_cap >= *records_needed and rec_start [n_positions + 1] are required (BVC_ERR_ARG).  A batch that has not been put
 * is BVC_ERR_ARG.  Waits for the context's stream.
 */
int bvc_store_get(bvc_ctx *ctx, const bvc_store *st, int32_t batch, uint8_t *records, int64_t records_cap, int64_t *records_needed,
                  uint32_t *rec_start);

/*
 * Ends the filling: every batch must have been put (else BVC_ERR_ARG; bvc_last_error names the first that is missing, and the store
 * stays open).  Brings down the cumulative sizes -- cum[t] = the sum over the batches of rec_start[t], which every put added on the
 * device -- and lays down the batches' table for bvc_pileup_begin_store.  Sealing twice is harmless.
 */
int bvc_store_seal(bvc_ctx *ctx, bvc_store *st);

/*
 * Host arithmetic only (a sealed store; else BVC_ERR_ARG, as for t0 outside [0, n_positions), max_positions < 1 or null outputs):
 * *n_positions = the largest T <= min(max_positions, n_positions - t0) with cum[t0 + T] - cum[t0] + 16 * n_batches <= max_bytes, at least 1;
 * *bytes = cum[t0 + T] - cum[t0] + 16 * n_batches for that T: an upper bound of the tile buffer bvc_pileup_begin_store fills.
 */
int bvc_store_tile(const bvc_store *st, int32_t t0, int32_t max_positions, int64_t max_bytes, int32_t *n_positions, int64_t *bytes);
/* bvc_store_tile's arithmetic on cumulative sizes of the caller's (cum [n_positions + 1], ascending; 0 <= t0 < n_positions, max_positions
 * >= 1): returns T and sets *bytes.  Needs no store and no device. */
static inline int32_t bvc_store_tile_fit(const int64_t *cum, int32_t n_positions, int32_t n_batches, int32_t t0, int32_t max_positions,
                                         int64_t max_bytes, int64_t *bytes)
{
    const int64_t *c = cum + t0, pad = (int64_t)16 * n_batches;
    int32_t lo = 1, hi = n_positions - t0 < max_positions ? n_positions - t0 : max_positions;
    while (lo < hi) {                      /* cum ascends: the largest T that fits, by bisection; one position where none does */
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (c[mid] - c[0] + pad <= max_bytes) lo = mid; else hi = mid - 1;
    }
    *bytes = c[lo] - c[0] + pad;
    return lo;
}
/* *used: device bytes of the batches put so far (rec_start rows and records); *budget: byte_budget as given.  Either may be null */
int bvc_store_bytes(const bvc_store *st, int64_t *used, int64_t *budget);

/*
 * The tile = positions [t0, t0 + n_positions) of EVERY batch, gathered on the device into the context's tile buffer; then
 * bvc_pileup_finish* exactly as after bvc_pileup_begin_bin -- batch b's samples are sample0[b] .. + n_in_batch[b], sample0 the prefix
 * sum of the n_in_batch values put.  The tile's records never were on the host, so its indel records' text_off mean nothing there: a
 * finish call must be given indel_text (room for *indel_text_bytes bytes), as after bvc_pileup_begin_bgzf; without it a tile that has
 * indels is BVC_ERR_ARG.  bvc_pileup_text delivers the gathered bytes and the tile's table (tests).
 * BVC_ERR_ARG: an unsealed store, a store on another device, positions outside the store, a tile whose slices (with 16 bytes a batch)
 * exceed 0xFFFFFF00 bytes -- use fewer positions; decided from the cumulative sizes before anything is launched.  BVC_ERR_DATA: a
 * malformed record, as bvc_pileup_begin_bin.  One wait; a second call of the same shape allocates nothing.
 */
int bvc_pileup_begin_store(bvc_ctx *ctx, const bvc_store *st, int32_t t0, int32_t n_positions, int64_t *n_entries, int64_t *n_indels,
                           int64_t *indel_text_bytes);

#ifdef __cplusplus
}
#endif
#endif /* BVC_STORE_H */
