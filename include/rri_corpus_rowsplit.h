/* rri_corpus_rowsplit.h -- a split of a resident corpus (rri_hip.h, "a CSR corpus that lives on the device"; rri_corpus_build.h) that
 * holds out an exact number of entries of every row: leave-k-out, and the per-user split of users a fit never saw.  An addition to
 * ABI 1.
 *
 * As in rri_corpus_split_entries the handle lends its device, its stream and its error text and nothing else: none of its cached
 * state is read or touched.  The call blocks.  The outputs are ordinary corpora: rri_corpus_memory counts them and
 * rri_device_memory does not, rri_corpus_destroy destroys them, every call that takes a corpus takes them, and rri_corpus_info
 * reports the HIP-event time of the call's kernels as ingest_ms.  RRI_ERR_INVALID for a NULL handle (without a device call), a
 * NULL output pointer, a NULL or destroyed corpus and a corpus on another device than the handle.  On any refusal or HIP error both
 * outputs are NULL and both memory counters are what they were; the temporaries of the call are freed on every return path.
 *
 * rri_corpus_split_rows: entry (i, j) of the source has the 64-bit key K = (word0 << 32) | (uint32_t)j, word0 being word 0 of
 * Philox4x32-10 with the key (seed low word, seed high word) and the counter (column, row low word, row high word, 0) -- the
 * generator, key and counter of rri_corpus_split_entries.  The columns of a row are distinct, so its keys are; every comparison is on
 * the whole key.  Row i with L stored entries gives up
 *     h = min(want, max(L - min_observed, 0)),   want = n_held                        in count mode    (n_held >= 1, fraction == 0)
 *                                                want = floor(fraction * L + 0.5)     in fraction mode (n_held == -1, 0 < fraction <= 1)
 * entries (want in double; h from the corpus's host copy of indptr): the h entries of the row with the smallest keys go to *held,
 * the others to *observed, each in source order.  Values are copied bit for bit and may be negative or fractional; there is no value
 * check.  Both outputs have the source's shape and are canonical; their patterns are disjoint and their union is the source's; row i
 * of *held has exactly h entries.  The split depends on (row, column, seed) and the quota alone, and two calls give the same bytes.
 * Under one seed the held set of a row for h is inside its held set for h + 1, and where rri_corpus_split_entries with some
 * threshold holds m entries of a row, a quota of m holds the same m entries.
 * RRI_ERR_INVALID also for n_held == 0, n_held below -1, a count together with a fraction that is not 0, a fraction outside (0, 1]
 * in fraction mode (NaN included in both), and a negative min_observed. */
#ifndef RRI_CORPUS_ROWSPLIT_H
#define RRI_CORPUS_ROWSPLIT_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_corpus_split_rows(rri_ctx* ctx, const rri_corpus* src, int64_t n_held, double fraction, int64_t min_observed,
                                 uint64_t seed, rri_corpus** observed, rri_corpus** held);

#ifdef __cplusplus
}
#endif
#endif /* RRI_CORPUS_ROWSPLIT_H */
