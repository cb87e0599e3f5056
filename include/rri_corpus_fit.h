/* rri_corpus_fit.h -- the recommender side of the resident-corpus chain (rri_hip.h, "a CSR corpus that lives on the device";
 * rri_corpus_ops.h, rri_corpus_build.h): the observation pattern and ratings of a pattern-only handle from a corpus, the clipped
 * prediction error of W T at the stored entries of a corpus, and the range of a corpus's values.  Additions to ABI 1.
 *
 * rri_upload_observed_corpus: what rri_upload_observed_csr does for host arrays, for a corpus of the handle's shape and device.
 * The canonical arrays are copied device to device and the store -- the canonical CSR in the storage type and both blocked
 * copies with segment pointers, offsets, permutations and work items -- is built on the device: byte for byte the store that
 * rri_upload_observed_csr leaves for the same canonical matrix.  The stored entries are the observed ones; a canonical corpus
 * holds no zeros, and values of either sign are taken.  The handle owns every buffer: the corpus is not kept and may be destroyed
 * right after the call.  Before anything of the handle is touched: RRI_ERR_INVALID for a NULL handle (without a device call), a
 * handle that is not RRI_WEIGHTED_SPARSE, a NULL or destroyed corpus, a corpus on another device and a shape that is not the
 * handle's (n, d); RRI_ERR_UNSUPPORTED for 2^31 - 1 stored entries or more.  A refusal leaves the handle's store, its cached state
 * and both memory counters as they were.
 *
 * rri_corpus_entries_error: request q (0 <= q < the corpus's rows) is row q of the corpus scored against row rows[q] of W; rows
 * NULL: row q, and then the corpus has at most n rows.  Duplicates and any order are allowed.  For an entry with column j and
 * value v: p = sum_t W[i,t] T[t,j] in float64, c = min(max(p, clip_lo), clip_hi), r = c - v; clip_lo = -inf and clip_hi = +inf
 * clip nothing.  Outputs, any of which may be NULL: sq_out[q] = sum r^2 and abs_out[q] = sum |r| over the request's entries
 * (n_rows doubles each), pred_out[e] = c per canonical entry in corpus order (nnz doubles), totals = {sum_q sq, sum_q abs, the
 * number of entries}, added on the host in ascending q, and kernel_ms, the HIP-event time of the call's kernels.  Every sum
 * depends on k and on the request's own segment only: a request scored alone and among others, two calls, and two handles of
 * different flavour that hold the same W and T return the same bits.  The call reads the handle's current W and T -- any
 * flavour, a factors-only handle included --, writes nothing a later sweep reads and keeps no buffer (rri_device_memory reports
 * what it reported before); it blocks, and on a row-sharded handle it is rank-local and not collective.  RRI_ERR_INVALID for a
 * NULL handle or corpus, a corpus on another device, a corpus whose columns are not d, a row outside [0, n), clip_lo > clip_hi, a
 * NaN bound and -- with entries to score -- W or T not set; RRI_ERR_UNSUPPORTED for 12 d > 64 MiB, as rri_entries_loglik.  An
 * empty corpus returns RRI_OK with zeroed outputs and launches nothing.  Negative values are accepted (rri_corpus_entries_loglik
 * refuses them).
 *
 * rri_corpus_value_range: out = {min, max} of the canonical values, reduced on the device in two stages of plain stores.
 * RRI_ERR_INVALID for a NULL argument, a corpus on another device and an empty corpus. */
#ifndef RRI_CORPUS_FIT_H
#define RRI_CORPUS_FIT_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_upload_observed_corpus(rri_ctx* ctx, const rri_corpus* corpus);
rri_status rri_corpus_entries_error(rri_ctx* ctx, const rri_corpus* corpus, const int64_t* rows, double clip_lo,
                                    double clip_hi, double* sq_out, double* abs_out, double* pred_out, double totals[3],
                                    double* kernel_ms);
rri_status rri_corpus_value_range(rri_ctx* ctx, const rri_corpus* corpus, double out[2]);

#ifdef __cplusplus
}
#endif
#endif /* RRI_CORPUS_FIT_H */
