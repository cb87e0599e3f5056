/* rri_corpus_rank.h -- the last step of the resident-corpus chain of a recommender (rri_corpus_build.h, rri_corpus_fit.h): top-N
 * lists, ranks and ranking metrics of W T against corpora that stay where they lie.  Additions to ABI 1.
 *
 * Order, eligibility, rank, value and clip are those of rri_topn_rows and rri_rank_entries; an open clip side is -inf or +inf.
 *
 * The EXCLUSION (NULL: none) is a corpus of the handle's shape (n, d) on the handle's device.  Request q, scoring row i = rows[q]
 * of W (rows NULL: i = q), excludes the stored columns of row i of that corpus: it is indexed by the row of W, not by the request,
 * so the whole training corpus is passed as it is for any list of rows, in any order, with repeats.  Nothing of it is copied or
 * checked again: canonical form is the check.
 *
 * rri_corpus_topn_rows: rri_topn_rows with such an exclusion.  idx_out and val_out have count x topn slots.
 *
 * rri_corpus_rank_entries: request q is row q of `targets` (d columns), scored against row rows[q] of W; rows NULL: row q, and then
 * the corpus has at most n rows.  Every stored entry is a target.  rank_out / val_out have one slot per canonical entry in corpus
 * order; either may be NULL.  eligible_out has one slot per corpus row and may be NULL; a row without stored entries is not scored
 * and gets -1.  The pieces of the scoring launch are cut on the device; the one int64 read back is their number.
 *
 * rri_corpus_ranking_metrics: the ranks of rri_corpus_rank_entries reduced on the device.  Over the targets whose stored value is
 * >= relevant_from (NaN: every entry), with N = n_items (any positive integer), out = {users, targets, targets_not_eligible,
 * sum [hits > 0], sum hits / N, sum hits / P, sum dcg / ideal, sum 1 / (1 + r0), sum auc term, users with L > P, sum S / (L - 1),
 * targets with L > 1, 0, 0, 0, 0}: per row P eligible targets, hits of them with rank < N, r0 the smallest and S the sum of their
 * ranks, L the row's eligible count, dcg = sum over hits of 1 / log2(rank + 2), ideal = sum_{p < min(N, P)} 1 / log2(p + 2), auc
 * term = 1 - (S - P (P - 1) / 2) / (P (L - P)) over rows with L > P; a row with P >= 1 is a user.  The caller divides.  Counts are
 * exact as doubles.  A row's terms depend on k and on the row's own segment only, and the 12 sums are added in ascending row order
 * by a fixed tree: the same request alone, among others, in a second call and on a handle of another flavour holding the same W
 * and T returns the same bits.
 *
 * All three read the handle's current W and T -- any flavour, a factors-only handle included --, write nothing a later sweep reads
 * and keep no buffer (rri_device_memory reports what it reported before); they block, and on a row-sharded handle they are
 * rank-local and not collective.  kernel_ms (may be NULL) takes the HIP-event time of the call's kernels.  Refusals come before any
 * device work and leave the handle's cached state and both memory counters as they were: RRI_ERR_INVALID for a NULL handle (without
 * a text) or targets, a destroyed corpus, a corpus on another device, an exclusion whose shape is not (n, d), targets whose columns
 * are not d, a row outside [0, n), n_items < 1, clip_lo > clip_hi, a NaN bound, a NULL output that is required and -- with
 * something to score -- W or T not set; RRI_ERR_UNSUPPORTED for topn outside 1 .. RRI_MAX_TOPN.  An empty targets corpus or
 * count == 0 returns RRI_OK with zeroed outputs (eligible -1) and launches nothing. */
#ifndef RRI_CORPUS_RANK_H
#define RRI_CORPUS_RANK_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_corpus_topn_rows(rri_ctx* ctx, const int64_t* rows, int64_t count, int32_t topn, const rri_corpus* exclude,
                                double clip_lo, double clip_hi, int32_t* idx_out, double* val_out, double* kernel_ms);
rri_status rri_corpus_rank_entries(rri_ctx* ctx, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude,
                                   double clip_lo, double clip_hi, int32_t* rank_out, double* val_out, int32_t* eligible_out,
                                   double* kernel_ms);
rri_status rri_corpus_ranking_metrics(rri_ctx* ctx, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude,
                                      int64_t n_items, double relevant_from, double out[16], double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* RRI_CORPUS_RANK_H */
