/* rri_fold.h -- fold new rows in against a fixed T on a pattern-only handle, one launch per sweep (rri_hip.h, "RRI_WEIGHTED_SPARSE
 * handles"; rri_corpus_fit.h).  Additions to ABI 1.
 *
 * The schedule.  With fix_T set and fix_W clear, row i of W depends on row i's own observed entries alone.  A handle that asked
 * takes, per sweep, ONE launch for the W half of all topics: per row q = sum_j x_ij T[:,j] and G = sum_j T[:,j] T[:,j]^T over the
 * row's stored entries j, then for t = t0 .. k-1 in order
 *     numer = q_t - sum_{l != t} G_tl W[i,l] - reg_w_l1 ,  c = G_tt + reg_w_l2
 *     W[i,t] = (c > 0) ? max(numer, 0) / (c + eps_div) : 0 ;  has_w_row_sum: W[i,t] = min(W[i,t], w_row_sum)
 * -- the update of the launch-per-topic schedule restated, all of it in float64 on the stored values, so an RRI_F32 handle is
 * computed exactly on what it stores.  Every sum has a fixed order that depends on the row's own entries, k and t0 only: two runs,
 * a row among others or alone, and the rows in another order give the same bits per row.  After the launch the column verdicts are
 * taken in topic order: the first topic whose column sums to 1e-10 or less (a reset event while resets are left, else
 * RRI_ERR_W_COL_ZERO) or that met a negative denominator without w_row_sum (RRI_ERR_UNBOUNDED) halts the run at the position the
 * launch-per-topic schedule reports, and a reset event leaves the columns after that topic as they were before the sweep: the
 * state in which the launch-per-topic schedule halts.  rri_pending_event, the reset calls and rri_resume work as they do there; the
 * resumed sweep enters the launch at the topic after the reset one.  The stored residual is stale after the launch: the next
 * objective or free sweep rebuilds it.
 *
 * Limits.  The handle is RRI_WEIGHTED_SPARSE on one device (not row-sharded), fix_T is set and fix_W clear, 1 <= k <= 64.  A handle
 * that asked and is outside them runs launch by launch, with the same results as one that never asked, and rri_fold_info says so.
 * The first one-launch sweep allocates k ldw + 2 k ceil(n / 16) doubles (the copy of W a halt restores from, the per-workgroup
 * column sums and negative-denominator counts); rri_device_memory of a handle that never takes such a sweep is unchanged.
 *
 * rri_set_fold_schedule: on != 0 asks for the schedule, 0 takes the request back; remembered for the handle's life, whatever
 * parameters, factors and observations are set later.  It touches no cached state and launches nothing.  RRI_ERR_INVALID for a NULL
 * handle (without a device call) and for a handle that is not RRI_WEIGHTED_SPARSE.
 *
 * rri_fold_info: out = {asked (0 / 1), eligible under the current parameters (0 / 1; 0 before rri_set_params), sweeps taken as one
 * launch (a sweep resumed after an event counts again; the launches queued behind a halt, which return at once, do not), sweeps
 * that took the launch-per-topic schedule while asked, halts found inside a launch, rows per workgroup}.  Reads host state only.
 * RRI_ERR_INVALID for a NULL handle or out (without a device call) and for a handle that is not RRI_WEIGHTED_SPARSE. */
#ifndef RRI_FOLD_H
#define RRI_FOLD_H

#include "rri_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

rri_status rri_set_fold_schedule(rri_ctx* ctx, int on);
rri_status rri_fold_info(const rri_ctx* ctx, int64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* RRI_FOLD_H */
