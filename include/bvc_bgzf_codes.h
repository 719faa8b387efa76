/*
 * bvc_bgzf_codes.h -- C ABI of libbvc, second header: the code-length builder of the device deflate encoder's dynamic blocks on its own.
 * Everything of bvc.h (conventions, contexts, return codes) holds here; the entry point below is exported by the same library.  It has
 * a header of its own because bvc.h's list of entry points is closed: the binding's first table is checked against that list, name by
 * name and by their number (tests/test_binding_abi.py).
 */
#ifndef BVC_BGZF_CODES_H
#define BVC_BGZF_CODES_H

#include "bvc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Rule (a) of "bgzf_codes" on its own, by the device code the block kernel uses (one wavefront a set): lengths[i][s] = the code length of
 * symbol s from counts[i][0 .. n_symbols), none above `limit`; 0 for an unused symbol but for the padding.  (n_symbols = 1: the one
 * symbol gets length 1.)  Host pointers, one wait.  It is there so that the builder can be driven with counts no small text produces.
 * BVC_ERR_ARG, before anything is launched and with the context left usable: null pointers with work present, a negative n_sets (or one
 * above 2^22), n_symbols outside 1..288, limit outside 1..15 or 2^limit < max(n_symbols, 2), a set whose counts sum to 2^24 or more.
 */
int bvc_bgzf_code_lengths(bvc_ctx *ctx, int64_t n_sets, const uint32_t *counts, int32_t n_symbols, int32_t limit, uint8_t *lengths);

#ifdef __cplusplus
}
#endif
#endif /* BVC_BGZF_CODES_H */
