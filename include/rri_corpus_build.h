/* rri_corpus_build.h -- the two ends of the resident-corpus chain (rri_hip.h, "a CSR corpus that lives on the device";
 * rri_corpus_ops.h): a corpus from a list of (row, column, value) pairs, and a split of a corpus by whole entries.  Additions to
 * ABI 1.
 *
 * As in rri_corpus_create and rri_corpus_ops.h the handle lends its device, its stream and its error text and nothing else: none
 * of its cached state is read or touched.  Both calls block.  The outputs are ordinary corpora: rri_corpus_memory counts them and
 * rri_device_memory does not, rri_corpus_destroy destroys them, every call that takes a corpus takes them, and rri_corpus_info
 * reports the HIP-event time of the call's kernels as ingest_ms.  RRI_ERR_INVALID for a NULL handle (without a device call), a
 * NULL output pointer and, for the split, a NULL or destroyed corpus and a corpus on another device than the handle.  On any
 * refusal or HIP error the outputs are NULL and both memory counters are what they were; the temporaries of a call are freed on
 * every return path.
 *
 * rri_corpus_from_pairs: pair p (0 <= p < n_pairs) is (rows[p * index_stride], cols[p * index_stride], values[p]).  index_dtype is
 * RRI_I32 or RRI_I64 and applies to both index arrays; index_stride >= 1 is in elements: 1 for two separate arrays, 2 with
 * cols == rows + 1 for an interleaved (m, 2) array, read where it lies.  values is RRI_F32, RRI_F64 or NULL: every pair counts 1,
 * so tokens become term counts.  on_device as in rri_corpus_create: the arrays are read during the call and never kept.  The
 * result is, byte for byte, the corpus rri_corpus_create makes of the raw CSR matrix whose row i holds the pairs of row i in the
 * order they were given (a stable sort of the pairs by row): the values of one (i, j) are added in float64 in the order given,
 * starting from the first; a sum that is exactly 0 is dropped; float32 widens exactly.  The ten fields of rri_corpus_info are
 * those of that call -- stored = n_pairs; rows rewritten = rows whose pairs, as given, do not ascend strictly by column or hold a
 * zero value; duplicates, zeros, negatives, long rows -- but for the device bytes.  Two ingests of one list give the same bytes.
 * Before any array is read: RRI_ERR_INVALID for a negative size, an unknown dtype code, index_stride < 1 and a NULL rows or cols
 * with n_pairs > 0; RRI_ERR_UNSUPPORTED for n_cols >= 2^31 and n_pairs > 2^31 - 1.  Then RRI_ERR_INVALID for, each over all pair
 * positions before the next, a row outside [0, n_rows), a column outside [0, n_cols), a NaN or infinite value: the smallest
 * offending pair position of the first broken rule is named.  The check reads by position only and nothing else runs before it
 * has passed.  RRI_ERR_UNSUPPORTED also for a row of more than 2^30 pairs.
 *
 * rri_corpus_split_entries: entry (i, j) of the source goes to *held when word 0 of Philox4x32-10 with the key (seed low word,
 * seed high word) and the counter (column, row low word, row high word, 0) is below threshold, and to *observed otherwise -- the
 * generator, key and counter of rri_corpus_split, so an entry whose count is 1 goes the same way in both under one seed and
 * threshold.  The split depends on (row, column, seed) alone.  Values are copied bit for bit and may be negative or fractional;
 * there is no value check.  Both outputs have the source's shape and are canonical; their patterns are disjoint and their union
 * is the source's.  RRI_ERR_INVALID also for a threshold of 0. */
#ifndef RRI_CORPUS_BUILD_H
#define RRI_CORPUS_BUILD_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_corpus_from_pairs(rri_ctx* ctx, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t n_pairs,
                                 const void* rows, const void* cols, int32_t index_dtype, int64_t index_stride,
                                 const void* values, int32_t values_dtype, int32_t on_device);
rri_status rri_corpus_split_entries(rri_ctx* ctx, const rri_corpus* src, uint32_t threshold, uint64_t seed,
                                    rri_corpus** observed, rri_corpus** held);

#ifdef __cplusplus
}
#endif
#endif /* RRI_CORPUS_BUILD_H */
