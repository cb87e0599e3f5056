/* rri_corpus_ops.h -- corpora derived from a resident corpus (rri_hip.h, "a CSR corpus that lives on the device"), on the device:
 * a selection of rows and columns, the document frequencies, and a binomial split of the counts.  Additions to ABI 1.
 *
 * The source is a live canonical rri_corpus and is never modified.  The handle lends its device, its stream and its error text
 * and nothing else, as in rri_corpus_create: none of its cached state is read or touched.  Every call blocks.  The outputs are
 * ordinary corpora: rri_corpus_memory counts them and rri_device_memory does not, rri_corpus_destroy destroys them, every call
 * that takes a corpus takes them.  rri_corpus_info reports for one of them stored == canonical entries, no rows rewritten, no
 * duplicates merged, no zeros dropped, no long rows, its own negatives and device bytes, and the HIP-event time of the
 * derivation's kernels as ingest_ms.  The outputs equal the plain loops of rri_derive.hpp byte for byte and are the same on every
 * run.  RRI_ERR_INVALID for a NULL handle (without a device call), a NULL output pointer, a NULL or destroyed corpus and a corpus
 * on another device than the handle.  On any refusal or HIP error the outputs are NULL and both memory counters are what they
 * were; the temporaries of a call are freed on every return path.
 *
 * rri_corpus_select: rows is NULL with n_rows_out = 0 (all rows, in order) or n_rows_out >= 0 row numbers in [0, n_rows), in any
 * order, repeats allowed; keep is NULL with n_cols_out = 0 (all columns) or n_cols_out >= 0 source columns, strictly ascending,
 * each in [0, n_cols).  Both are host arrays, checked on the host before any device call.  Row q of *out holds the entries of
 * source row rows[q] whose column is in keep, each column renumbered to its place in keep, the values copied bit for bit: the
 * canonical form of A[rows][:, keep].  RRI_ERR_INVALID also for an entry out of range, a keep that does not ascend strictly, a
 * negative count and a NULL list with a non-zero count.
 *
 * rri_corpus_column_counts: df_out[j], j < n_cols, is the number of rows with a canonical entry in column j.
 *
 * rri_corpus_split: every token of every count goes to *held with probability threshold / 2^32 and to *observed otherwise,
 * independently: Philox4x32-10 with the key (seed low word, seed high word) and the counter (column, row low word, row high
 * word, block b); token t of an entry uses word t % 4 of block t / 4 and is held when that word is below threshold.  The split
 * depends on (row, column, count, seed) alone.  Both outputs have the source's shape, hold the entries whose part is above 0,
 * and observed + held == source exactly.  The values must be counts: RRI_ERR_INVALID for a negative value, then for one that is
 * not whole, then RRI_ERR_UNSUPPORTED for one above 2^20 -- the smallest offending canonical position of the first broken rule
 * is named, and nothing of the outputs is allocated before that verdict.  RRI_ERR_INVALID also for a threshold of 0. */
#ifndef RRI_CORPUS_OPS_H
#define RRI_CORPUS_OPS_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_corpus_select(rri_ctx* ctx, const rri_corpus* src, const int64_t* rows, int64_t n_rows_out, const int32_t* keep,
                             int64_t n_cols_out, rri_corpus** out);
rri_status rri_corpus_column_counts(rri_ctx* ctx, const rri_corpus* src, int64_t* df_out);
rri_status rri_corpus_split(rri_ctx* ctx, const rri_corpus* src, uint32_t threshold, uint64_t seed, rri_corpus** observed,
                            rri_corpus** held);

#ifdef __cplusplus
}
#endif
#endif /* RRI_CORPUS_OPS_H */
