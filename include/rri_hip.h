/*
 * rri_hip.h -- C ABI of librri_hip.so: the MI355X (gfx950) implementation of the
 * rank-one residue iteration (RRI) inner loop of maksimt/rri_nmf.
 *
 * The reference has no FFI: its seams are the Python callable
 *     nmf(X, k, ...) -> dict                       src/rri_nmf/nmf.py:98-108, :551-560
 * and the per-topic helpers it calls through **locals():
 *     _compute_update_T                            nmf.py:633-715
 *     _compute_update_W                            nmf.py:718-747
 *     qf_min                                       optimization.py:12-88
 *     euclidean_proj_simplex / proj_mat_to_simplex matrixops.py:5-100
 *     _project_and_check_reset_t / _check_reset_W  nmf.py:751-816
 *     TrueObjComputer.true_objective               nmf.py:71-94
 * A maintainer of the reference would bind exactly the entry points below with
 * ctypes (INTEGRATION.md shows the stub) and call them from nmf()'s sweep loop.
 *
 * Conventions
 *   - plain C, no torch / C++ types; every function returns an rri_status (0 = ok),
 *     never throws; rri_last_error() gives the text of the last failure on a handle.
 *   - host matrices are row-major, caller-owned and never written unless the
 *     argument is an explicit output; `ld` arguments are row strides in ELEMENTS.
 *   - one opaque handle per nmf() call; calls on one handle are serialised by the
 *     caller; all device work of a handle runs on ONE HIP stream (its own, or the
 *     caller's when `stream` is non-NULL, e.g. torch's current stream).
 *   - notation follows the reference: X n*d, W n*k ("documents x topics"),
 *     T k*d ("topics x features"; north_star's H).  W[:,t] is Ho's u_t, T[t,:] is v_t^T.
 */
#ifndef RRI_HIP_H
#define RRI_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRI_ABI_VERSION 1
/* the Gram part of the reduce buffer travels as this many slice sums (see rri_topic_reduce_local) */
#define RRI_GRAM_SLICES 8
/* largest rank k a handle takes */
#define RRI_MAX_K 1024
/* longest list rri_topn_rows returns per row */
#define RRI_MAX_TOPN 64
/* most words per group rri_cooccurrence_counts takes: one bit per slot of a 32-bit word */
#define RRI_MAX_COOC_WORDS 32

typedef struct rri_ctx rri_ctx;   /* opaque: one nmf() call (or one row shard of it) on one GPU */
typedef struct rri_comm rri_comm; /* opaque: the communicator of a row-sharded run, one per process */
#define RRI_COMM_ID_BYTES 128     /* sizeof(ncclUniqueId) */

typedef int32_t rri_status;
enum {
    RRI_OK = 0,
    RRI_PAUSED = 1,             /* a sweep stopped at a rare branch; see rri_pending_event */
    RRI_ERR_INVALID = -1,       /* bad argument / shape / state                              */
    RRI_ERR_HIP = -2,           /* a HIP runtime call failed                                */
    RRI_ERR_UNSUPPORTED = -3,   /* option not available on the device path                  */
    RRI_ERR_UNBOUNDED = -4,     /* qf_min: minimum objective is unbounded (optimization.py:66-67,76-77) */
    RRI_ERR_W_COL_ZERO = -5,    /* assert sum(W[:,t]) > 0 failed (nmf.py:476)               */
    RRI_ERR_NOT_IMPLEMENTED = -6, /* qf_min: c<=0 with s not in {None,1.0} (optimization.py:72-73) */
    RRI_ERR_COMM = -7            /* a collective (RCCL, or the caller's transport) failed                   */
};

enum { RRI_F32 = 0, RRI_F64 = 1,     /* storage type of X, mask, residual in HBM (arithmetic is float64) */
       /* float16 (IEEE binary16): for the dense X of an RRI_UNWEIGHTED handle only -- the one flavour in which the stored matrix is
        * never rewritten, so the storage type costs exactly one rounding, at upload (to nearest even, one step from the host
        * type), and a float16 value converts to float64 exactly: the handle solves the float64 problem on the ROUNDED X.  Half the
        * bytes of fp32 per pass and per matrix.  Suits magnitudes below 65520 and data of 11 significant bits: integers up to 2048
        * (term counts, ratings, pixels, 0/1) are stored exactly; otherwise the relative rounding is 2^-11 above 6.1e-5 and the
        * absolute one 3e-8 below it (rri_storage_error reports what it came to).  rri_create refuses it (RRI_ERR_UNSUPPORTED) for
        * the four other flavours; the handle refuses everything that would rewrite X or needs a mask, a residual or a CSR store
        * (rri_scale_X, rri_column_positive_counts, rri_upload_mask*, rri_bind_mask_device, rri_upload_X_csr, rri_upload_observed_csr,
        * rri_residual_*, rri_get_residual, rri_bench_*) and rri_attach_comm, and never takes the persistent on-chip path. */
       RRI_F16 = 2,
       /* counts (unsigned bytes, 0..255) with a float64 scale per row and per column kept on the handle: the second store of a
        * dense X that is only read.  The X every kernel sees is (C[i,j] * cscale[j]) * rscale[i], formed in float64 where it is
        * read -- byte -> float -> double is exact -- so the store costs no rounding at all, a quarter of the fp32 bytes per pass,
        * and tf-idf and row normalisation are two vector updates (rri_scale_X writes no matrix on such a handle).  Refused and
        * allowed exactly as RRI_F16 is, but for the two preprocessing calls, which it takes; both scale vectors are ones after
        * rri_create and after every rri_upload_X / rri_bind_X_device (rri_set_X_scales, rri_get_X_scales).  A scale may be zero or
        * negative (the idf of a term that occurs in every document is a tiny negative number). */
       /* (code 3 stays unassigned: rri_create has always refused it with RRI_ERR_INVALID) */
       RRI_U8 = 4 };
/* rri_create's `weighted`: the flavour of the handle */
enum { RRI_UNWEIGHTED = 0, RRI_WEIGHTED_DENSE = 1, RRI_WEIGHTED_SPARSE = 2, RRI_UNWEIGHTED_RESIDUAL = 3,
       RRI_UNWEIGHTED_SPARSE = 4 };
enum { RRI_RESET_NONE = 0, RRI_RESET_MAX_RESID_DOCUMENT = 1, RRI_RESET_RANDOM = 2 };
enum { RRI_EVENT_NONE = 0, RRI_EVENT_RESET_T = 1, RRI_EVENT_RESET_W = 2 };

/* The options of nmf() that reach the inner loop (nmf.py:98-108).  "has_*" = the
 * Python value is not None. */
typedef struct rri_params {
    int32_t fix_W;                 /* nmf.py:460 */
    int32_t fix_T;                 /* nmf.py:417 */
    int32_t project_T_each_iter;   /* s = t_row_sum in the T-row qf_min, nmf.py:442-447 */
    int32_t has_t_row_sum;
    int32_t has_w_row_sum;         /* scalar w_row_sum: the `ub` of the W-column qf_min, nmf.py:469 */
    int32_t reset_method;          /* RRI_RESET_*; nmf.py:104 */
    int32_t resets_left;           /* nmf.py:105,192-193: budget still available */
    int32_t reserved0;
    double t_row_sum;
    double w_row_sum;
    double reg_w_l1, reg_w_l2, reg_t_l1, reg_t_l2; /* nmf.py:106 */
    double eps_div;                /* np.spacing(10), nmf.py:52 */
} rri_params;

typedef struct rri_event {
    int32_t kind;          /* RRI_EVENT_* */
    int32_t topic;         /* t: the row of T / column of W to reset */
    int32_t sweep;         /* sweep index (inside the interrupted call) of the step that detected it */
    int32_t resume_topic;  /* topic of that step: a RESET_T resumes at the W half of `topic`, a RESET_W at
                              the T half of `resume_topic` */
} rri_event;

/* ---- lifetime ------------------------------------------------------------------ */
uint32_t   rri_abi_version(void);
/* dtype: RRI_F32 / RRI_F64, or RRI_F16 / RRI_U8 with RRI_UNWEIGHTED (see the enum).  weighted: RRI_UNWEIGHTED; RRI_WEIGHTED_DENSE reserves the mask and masked-residual
 * buffers of the elementwise-weighted flavour (WRRI, nmf.py:687-701,735-746) as dense n x d arrays;
 * RRI_WEIGHTED_SPARSE keeps that flavour on a 0/1 observation pattern only (rri_upload_observed_csr).
 * RRI_UNWEIGHTED_RESIDUAL is the unweighted flavour on the EXPLICIT residual R = X - W T (kept in HBM beside X): every
 * topic step is one rank-one residual update pass R <- R -+ v u^T fused with the residual products R t / R^T w of
 * nmf.py:670-676,728-734 (SURVEY 8a "explicit-residual variant"; k >= 2, both halves free), 2 n d bytes per step
 * where the default Gram-form schedule (RRI_UNWEIGHTED) reads X once.  Same results to rounding.
 * RRI_UNWEIGHTED_SPARSE is the unweighted flavour (the Gram form of RRI_UNWEIGHTED) with X kept as CSR: the topic-model case of
 * term counts at a few per cent density or less (nmf.py:670-676, 728-734 on a sparse X).  rri_upload_X_csr then keeps the
 * canonical CSR (8 B of index and value per stored fp32 entry, 12 B fp64) and two blocked copies of it, rows and columns as
 * segments (6 B per entry each fp32, 10 B fp64, plus a 4-byte position), and no dense n x d array at all; every topic step reads
 * both copies once (12 nnz bytes fp32) in one launch.  It refuses (RRI_ERR_UNSUPPORTED) rri_upload_X, rri_bind_X_device, every
 * mask, rri_attach_comm and rri_range_finder (its range finder is rri_sparse_range_finder), and answers RRI_ERR_INVALID to the dense preprocessing calls
 * (rri_column_positive_counts, rri_scale_X): tf-idf / normalisation of a CSR X have their own pair,
 * rri_csr_column_positive_counts and rri_csr_scale_X.  Never takes the persistent on-chip path; at most 2^31 - 2 entries.
 * device: HIP device ordinal.  stream: hipStream_t to run on, or NULL for an own stream. */
rri_status rri_create(rri_ctx** out, int64_t n, int64_t d, int32_t k, int32_t dtype,
                      int32_t weighted, int32_t device, void* stream);
rri_status rri_destroy(rri_ctx* ctx);
const char* rri_last_error(const rri_ctx* ctx);   /* NULL ctx: error of the last failed rri_create */

/* ---- data: replaces the numpy arrays nmf() holds (nmf.py:272,351,867-868) --------- */
/* host_dtype: RRI_F32 / RRI_F64 of the HOST buffer; converted to the handle's dtype.  rri_upload_X on an RRI_F16 handle also
 * takes a host buffer of halves (RRI_F16); whatever the host type, a value that is not finite as a float16 (|x| >= 65520, inf,
 * NaN) fails the call with RRI_ERR_INVALID and leaves the handle without an X.  On an RRI_U8 handle the host buffer is RRI_F32,
 * RRI_F64 or RRI_U8 (bytes, taken as they are); a value that is not an integer in 0..255 (fractions, negatives, inf, NaN) fails
 * the call the same way, and a successful upload sets both scale vectors to ones. */
rri_status rri_upload_X(rri_ctx* ctx, const void* host, int64_t ld, int32_t host_dtype);
rri_status rri_upload_mask(rri_ctx* ctx, const void* host, int64_t ld, int32_t host_dtype); /* W_mat */
/* Zero-copy alternative: X (and mask) already in device memory in the handle's dtype,
 * row-major with row stride ld (a multiple of 16 bytes, base 16-byte aligned).  The calls synchronise the device
 * once, so memory just produced on another stream is complete (rri_bind_mask_device reads the mask at once to
 * bit-pack it); later changes to the memory are the caller's to order against the handle's stream. */
/* (an RRI_F16 handle binds an array of halves, e.g. a torch.float16 tensor: ld a multiple of 8 elements; an RRI_U8 handle an
 * array of bytes, e.g. a torch.uint8 tensor: base 8-byte aligned, ld and d multiples of 8 elements; both scale vectors are ones
 * afterwards) */
rri_status rri_bind_X_device(rri_ctx* ctx, const void* dev, int64_t ld);
/* What storing X cost: out[0] = sum (x - stored(x))^2, out[1] = sum x^2 over the matrix given to the last rri_upload_X of an
 * RRI_F16 handle (float64 sums in a fixed order; sqrt(out[0] / out[1]) is the relative Frobenius distance between the caller's
 * X and the X the handle factorises -- the rounding nmf() adds to a float64 run, nmf.py:272).  Zeros on float32 / float64 / uint8
 * handles (what RRI_U8 accepts it stores exactly) and for bound arrays, which are taken as they are. */
rri_status rri_storage_error(rri_ctx* ctx, double out[2]);
rri_status rri_bind_mask_device(rri_ctx* ctx, const void* dev, int64_t ld);
/* Ingestion without host densification (the reference densifies with .toarray(), sklearn_interface.py:78-102):
 * X from host CSR arrays (indptr n+1 int64, indices int32 column ids, data of data_dtype) scattered into the
 * zero-filled dense device X; and the observation mask W_mat = [X != 0] of such a matrix, built bit-packed. */
/* On an RRI_UNWEIGHTED_SPARSE handle rri_upload_X_csr keeps X as CSR instead (column indices are sorted per row on the host,
 * duplicates refused, explicit zeros kept): see rri_create. */
rri_status rri_upload_X_csr(rri_ctx* ctx, const int64_t* indptr, const int32_t* indices, const void* data,
                            int64_t nnz, int32_t data_dtype);
rri_status rri_upload_mask_csr_pattern(rri_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                                       const void* data, int64_t nnz, int32_t data_dtype);
/* RRI_WEIGHTED_SPARSE handles: W_mat is the 0/1 pattern of a CSR matrix and X is given on that pattern only
 * (values[p] = X[r, indices[p]], explicit zeros allowed; X is taken as 0 elsewhere, where W_mat = 0 hides it from
 * every sum of nmf.py:687-746 and the reset search of nmf.py:770-773 sees max(0 - WT, 0) = 0).  The recommender
 * case of sklearn_interface.py:78-102 without any dense n x d array: the residual is kept on the pattern, as a
 * CSR and a CSC copy.  Replaces rri_upload_X + rri_upload_mask for such a handle. */
rri_status rri_upload_observed_csr(rri_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                                   const void* values, int64_t nnz, int32_t data_dtype);
rri_status rri_set_W(rri_ctx* ctx, const void* host, int64_t ld, int32_t host_dtype);  /* n*k */
rri_status rri_set_T(rri_ctx* ctx, const void* host, int64_t ld, int32_t host_dtype);  /* k*d */
rri_status rri_get_W(rri_ctx* ctx, void* host, int64_t ld, int32_t host_dtype);
rri_status rri_get_T(rri_ctx* ctx, void* host, int64_t ld, int32_t host_dtype);
rri_status rri_set_params(rri_ctx* ctx, const rri_params* p);

/* ---- the hot path: the topic loop of nmf.py:415-476 ----------------------------- */
/* Runs n_sweeps Gauss-Seidel sweeps (each = k topic steps: T-row update, then W-column
 * update).  Returns RRI_OK, RRI_PAUSED (a reset condition of nmf.py:762-783 / :796-816
 * was met: query rri_pending_event, resolve it with rri_apply_reset_* and call
 * rri_resume), or a negative error mirroring the reference's exceptions.
 * sweeps_done (may be NULL) receives the number of COMPLETED sweeps of this call.
 * Schedules chosen by the library, same results to summation order and the same events, statuses and resume positions:
 * launch-bound sizes run as one persistent launch (rri_onchip_info); with fix_T set (the fold-in of nmf.py:417 / 460-476,
 * sklearn_interface.py:327-333) an unweighted handle takes X T^T and T T^T once per T and runs the W half of all k topics of
 * a sweep as ONE launch over the rows of W, the column checks of nmf.py:471-476 in topic order after it (k n + k^2 doubles
 * of device memory more, allocated at the first such sweep; RRI_WSWEEP=0 in the environment of rri_create: topic by topic);
 * dense weighted handles whose W_mat is 0 / 1 and below 12 % set keep a second bit-packed copy of it (n d / 8 bytes);
 * handles of 10^8 elements or more time their pass once, before the first sweep, under the two ways of dealing its tiles to
 * the XCDs and keep the faster (the read-only pass over X: ~5 ms; the read-modify-write pass over a stored residual --
 * RRI_UNWEIGHTED_RESIDUAL, dense weighted --: ~12 ms, the residual rewritten with its own values meanwhile; RRI_ROT_CAL=0: not). */
rri_status rri_sweep(rri_ctx* ctx, int32_t n_sweeps, int32_t* sweeps_done);
rri_status rri_resume(rri_ctx* ctx, int32_t* sweeps_done);
rri_status rri_pending_event(rri_ctx* ctx, rri_event* ev);
/* 'max_resid_document' (nmf.py:770-776, :804-810), entirely on the device. */
rri_status rri_apply_reset_max_resid(rri_ctx* ctx, int32_t t, int64_t* row_chosen);
/* 'random' (nmf.py:778-783, :811-816): the caller draws the vectors with numpy's
 * global RNG (as the reference does) and hands them over. */
rri_status rri_apply_reset_vectors(rri_ctx* ctx, int32_t t, const double* T_row, const double* W_col);
/* skip the pending reset (budget exhausted, nmf.py:765-768 / :797-800) */
rri_status rri_skip_reset(rri_ctx* ctx);

/* Finer-grained steps (tests, host drivers): one half of one topic step. */
rri_status rri_update_T_row(rri_ctx* ctx, int32_t t);   /* nmf.py:417-458 */
rri_status rri_update_W_col(rri_ctx* ctx, int32_t t);   /* nmf.py:460-476 */

/* ---- the explicit residual (RRI_UNWEIGHTED_RESIDUAL handles) ---------------------- */
/* R = X - W T for the handle's current factors (the products of nmf.py:670-676 / 728-734 are taken on it). */
rri_status rri_residual_rebuild(rri_ctx* ctx);
/* The outer-product residual update as an operation of its own:
 *     R <- R - a b^T [- a2 b2^T]      (a, a2: n doubles; b, b2: d doubles; a2 = b2 = NULL for one term)
 * fused with y = R_new trow (n, nmf.py:729) and z = R_new^T wcol (d, nmf.py:672) of the updated residual, all host
 * vectors, float64 arithmetic, R rounded to the handle's storage type when stored.  y_out / z_out may be NULL.
 * The stored R then no longer belongs to the handle's (W, T): the next sweep rebuilds it. */
rri_status rri_residual_update(rri_ctx* ctx, const double* a, const double* b, const double* a2, const double* b2,
                               const double* trow, const double* wcol, double* y_out, double* z_out);
rri_status rri_get_residual(rri_ctx* ctx, void* host, int64_t ld, int32_t host_dtype);   /* n*d, as stored */

/* ---- around the loop ------------------------------------------------------------ */
/* Row-wise simplex projection of W (proj_mat_to_simplex, matrixops.py:72-100; final
 * projection nmf.py:519-529).  s_vec == NULL: every row to the scalar s; else n doubles. */
rri_status rri_project_W_rows(rri_ctx* ctx, double s, const double* s_vec);
/* true_objective (nmf.py:71-94) with the handle's regularisers and mask; float64 accumulation.  Right after rri_sweep on an
 * unweighted handle no pass over X is made (1/2 ||X||^2 - sum_t <w_t, X t_t> + 1/2 <W^T W, T T^T>, the cross terms left by the
 * sweep); after a sweep of the register-resident kernel nothing is launched at all -- the kernel left the value with the state
 * the host reads anyway (RRI_ONCHIP_OBJ=0: the Gram kernels instead). */
rri_status rri_objective(rri_ctx* ctx, double* out);
/* argmax over topics of every row of W (harden_distributions, matrixops.py:203-209). */
rri_status rri_argmax_rows(rri_ctx* ctx, int32_t* out_host);
/* X*T^T clipped reconstruction error on listed entries: RMSE of NMF_RS_Estimator.score /
 * RMSE_val (sklearn_interface.py:85-91,172-182).  idx = (i,j) pairs, vals = ratings.
 * On a handle with a communicator attached the call is collective: (i, j) are this rank's LOCAL rows (count may be 0),
 * the result is sqrt(sum of squared errors over all ranks / number of entries over all ranks), equal on every rank -- the
 * early-stop decision of nmf.py:381-407 is then the same everywhere.  A rank whose own arguments are bad (an index out of range,
 * a NULL list) still takes part in the collective and raises a flag in it: EVERY rank returns RRI_ERR_INVALID (the failing one
 * names its entry, the others say "on another rank"), nobody is left waiting, and the ranks stay in step for the next call. */
rri_status rri_masked_rmse(rri_ctx* ctx, const int64_t* ij, const double* vals, int64_t count,
                           double clip_lo, double clip_hi, double* out);
/* The topn best columns of W T for each of `count` rows: what a recommender shows a user.  For a requested row i the score of
 * column j is s_ij = sum_t W[i,t] T[t,j] in float64; eligible are the columns 0 .. d-1 that the row does not exclude and whose
 * score is not NaN; the order is larger score first and, among equal scores, smaller column first (a total order: the answer
 * does not depend on how the work is split).  idx_out[r * topn ..] takes the first min(topn, eligible) columns of that order,
 * val_out their scores clipped to [clip_lo, clip_hi] -- the ranking uses the UNCLIPPED score; a NaN bound leaves that side open
 * -- and the slots after them the index -1 and the value NaN.  Nothing of size n x d exists anywhere: the scores are formed tile
 * by tile on the matrix cores and only the lists leave the chip.
 *   rows          count row indices in [0, n), any order, duplicates allowed; NULL: rows 0 .. count-1
 *   excl_indptr   NULL: nothing excluded.  Else a CSR pattern with one row per REQUEST (count + 1 entries, starting at 0,
 *                 monotone); excl_indices: per request strictly ascending columns in [0, d)
 * Blocking; reads the handle's current W and T (both must have been set: a handle with factors and no X will do, rri_create
 * allocates nothing of size n x d) and works on every flavour and storage type.  Writes nothing a later sweep reads and keeps no
 * buffer: rri_device_memory is what it was.  On a row-sharded handle the rows are local ones and the call is not collective.
 * RRI_ERR_INVALID: a NULL handle or output, count < 0, a row out of range, factors not set, a malformed exclusion;
 * RRI_ERR_UNSUPPORTED: topn outside 1 .. RRI_MAX_TOPN; count == 0: RRI_OK, nothing launched (outputs may be NULL). */
rri_status rri_topn_rows(rri_ctx* ctx, const int64_t* rows, int64_t count, int32_t topn, const int64_t* excl_indptr,
                         const int32_t* excl_indices, double clip_lo, double clip_hi, int32_t* idx_out, double* val_out);
/* The rank of listed columns in the total order of their rows: what hit rate, recall@N, NDCG@N, MRR, AUC and mean percentile
 * rank of held-out pairs are computed from.  Request q has the row rows[q] (NULL: row q), the exclusion segment of rri_topn_rows
 * (excl_indptr NULL: none) and the TARGET segment tgt_indices[tgt_indptr[q] .. tgt_indptr[q + 1]): columns strictly ascending
 * inside [0, d); tgt_indptr is required.  Scores, eligibility and order are those of rri_topn_rows.  For target column j of
 * request q, at its place in tgt_indices:
 *   rank_out  the number of eligible columns j' != j that stand before j in the order -- the 0-based place j would have in an
 *             unbounded rri_topn_rows list; the request's other targets count as competitors --, or -1 when j is itself not
 *             eligible (excluded, or its score is NaN);
 *   val_out   the score of j clipped to [clip_lo, clip_hi] (a NaN bound leaves that side open), NaN when j is not eligible: the
 *             bits rri_topn_rows returns for that column;
 * and eligible_out[q] (may be NULL) takes the number of eligible columns of request q.  There is no cap on the targets of a
 * request.  The counts are integers formed without atomics: the answer does not depend on how the work is split.
 * Like rri_topn_rows the call needs W and T set and nothing else, works on every flavour and storage type, writes nothing a
 * later sweep reads and keeps no buffer; on a row-sharded handle the rows are local ones and the call is not collective.
 * RRI_ERR_INVALID: a NULL handle or output, count < 0, a row out of range, factors not set, tgt_indptr NULL, malformed targets or
 * exclusion; count == 0 or no target at all: RRI_OK, nothing launched and no output written (the outputs may be NULL). */
rri_status rri_rank_entries(rri_ctx* ctx, const int64_t* rows, int64_t count,
                            const int64_t* tgt_indptr, const int32_t* tgt_indices,
                            const int64_t* excl_indptr, const int32_t* excl_indices,
                            double clip_lo, double clip_hi,
                            int32_t* rank_out, double* val_out, int32_t* eligible_out);
/* Document and co-document frequencies of groups of words: the two integer tables that topic coherence (UMass, PMI, NPMI over
 * document co-occurrence) is computed from.  The corpus is a CSR PATTERN of n_rows x n_cols: indptr (n_rows + 1 entries, from 0,
 * monotone) and indices (strictly ascending inside every row, inside [0, n_cols)); a stored entry means "the word occurs in the
 * document", there are no values (drop explicit zeros first).  n_rows and n_cols belong to the request, not to the handle: a
 * reference corpus need not be the training matrix.  words is n_groups x group_size, row-major: a column in [0, n_cols) or -1 for
 * an empty slot, empty slots anywhere, a column at most once inside one group and in any number of groups.
 *   df_out    n_groups x group_size: the number of rows that contain words[g, a];
 *   codf_out  n_groups x group_size x group_size: the number of rows that contain both words[g, a] and words[g, b]; symmetric,
 *             codf[g, a, a] = df[g, a];
 * a -1 slot has 0 in its row and its column.  The counts are integers summed exactly: the answer does not depend on how the work
 * is split, and two calls return the same bits.
 * Blocking.  The handle supplies the device, the stream and the error text and nothing else: no X, W or T is needed, every flavour
 * and storage type will do, nothing a later sweep reads is written, no buffer is kept (rri_device_memory is what it was), and on
 * a handle with a communicator the call is not collective -- counts of row blocks add, so a caller sums them.  The request is
 * checked before any HIP call.
 * RRI_ERR_INVALID: a NULL handle, array or output, a negative size, a malformed CSR pattern, a word out of range or twice in one
 * group; RRI_ERR_UNSUPPORTED: group_size outside 1 .. RRI_MAX_COOC_WORDS or n_groups outside 1 .. RRI_MAX_K; n_rows == 0 or no
 * stored entry: RRI_OK, the outputs zeroed, nothing launched. */
rri_status rri_cooccurrence_counts(rri_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                                   int64_t n_rows, int64_t n_cols,
                                   const int32_t* words, int32_t n_groups, int32_t group_size,
                                   int64_t* df_out, int64_t* codf_out);
/* The log-likelihood of stored counts under the rows of W T: what the held-out perplexity of a topic model is computed from.
 * A call has `count` requests.  Request q has a row i = rows[q] of W (rows NULL: i = q, so count <= n; duplicates allowed, any
 * order) and a segment of a CSR matrix WITH values: indices[indptr[q] .. indptr[q + 1]) and values[...], the columns strictly
 * ascending inside [0, d), the values finite and >= 0; indptr has count + 1 entries, from 0, monotone.  For entry e of the segment,
 * with column j and value v:  p_e = sum_t W[i,t] T[t,j] in float64;  term_e = 0 exactly when v == 0, else
 * v * log(p_e < floor ? floor : p_e) -- a NaN p_e stays NaN, and with floor == 0 and p_e == 0 the term is -inf.
 *   ll_out[q]       sum_e term_e
 *   mass_out[q]     sum_e v
 *   floored_out[q]  the number of entries with v > 0 and p_e < floor
 * Every sum is taken in an order that depends on k and on the request's own segment only: a request scored alone and among
 * others returns the same bits, and so do two calls.  Nothing is scaled: when every row of W T is a distribution, ll is a
 * log-likelihood.
 * Blocking.  Reads the handle's current W and T (both must be set; a factors-only handle will do, every flavour and storage
 * type), writes nothing a later sweep reads and keeps no buffer (rri_device_memory is what it was); on a row-sharded handle the
 * rows are local and the call is not collective.  The entries travel in chunks of whole requests of at most 64 MiB at 12 bytes
 * per entry.  The request is checked before any HIP call.
 * RRI_ERR_INVALID: a NULL handle, indptr or output, NULL indices or values with entries present, indptr not from 0 or not
 * monotone, a column out of range or not strictly ascending, a negative, NaN or infinite value, a row out of range, count < 0,
 * a negative, NaN or infinite floor, W or T not set; RRI_ERR_UNSUPPORTED: 12 d > 64 MiB (a full row would not fit a chunk);
 * count == 0 or no entry at all: RRI_OK, the outputs zeroed, nothing launched. */
rri_status rri_entries_loglik(rri_ctx* ctx, const int64_t* rows, int64_t count,
                              const int64_t* indptr, const int32_t* indices, const double* values,
                              double floor, double* ll_out, double* mass_out, int64_t* floored_out);
/* ---- a CSR corpus that lives on the device ------------------------------------------------------------------------------------
 * The evaluation calls above take a sparse corpus from the host on every call; a loop that scores the same corpus after every
 * batch or sweep pays for the host's canonical copy and the upload each time, and counts that are already in device memory have
 * to travel to the host and back.  An rri_corpus is that matrix, checked and made canonical ON the device, once.
 * The raw matrix is n_rows x n_cols with nnz_stored entries: indptr (n_rows + 1 entries) and indices as RRI_I32 or RRI_I64, values
 * as RRI_F32 or RRI_F64, or NULL for a pattern (every stored entry has the value 1; values_dtype is then not read).  Its rows may
 * be unsorted, hold a column several times and hold explicit zeros.  It is refused, with the smallest offending position of the
 * first broken rule in rri_last_error, for: indptr[0] != 0, a decreasing indptr, indptr[n_rows] != nnz_stored, a column outside
 * [0, n_cols), a NaN or infinite value (all RRI_ERR_INVALID), n_cols >= 2^31 (RRI_ERR_UNSUPPORTED).  The check reads the arrays
 * by position only and nothing else runs before it has passed: a malformed matrix never becomes an address.
 * The canonical form: per row the columns ascend strictly, the stored entries of one column are added in float64 in their stored
 * order, an entry whose sum is exactly 0 is dropped, a float32 value widens exactly; int32 indices, float64 values, int64 indptr.
 * Two ingests of one matrix give the same bytes.
 * rri_corpus_create: the handle supplies the device, the stream and the error text and nothing else; the corpus outlives it and
 * serves every handle on the same device (one on another device: RRI_ERR_INVALID).  on_device = 0: the three arrays are host
 * memory; they are uploaded as they are and checked and made canonical by the same kernels.  on_device = 1: they are device
 * pointers on that device, whatever produced them has been synchronised by the caller, they are read during the call and never
 * kept: the corpus owns its own copy.  Blocking.  RRI_ERR_INVALID also for a NULL handle or output pointer, a negative size, a
 * NULL indptr, NULL indices with entries present, or an unknown dtype code; RRI_ERR_UNSUPPORTED also for a row of more than 2^30
 * stored entries that is not canonical already.  On any failure *out is NULL and nothing is kept.
 * The corpus's buffers are not handle-owned: rri_device_memory does not count them.  rri_corpus_memory is their own counter (the
 * corpora alive in the process and their device bytes; either pointer may be NULL); the temporaries of an ingest are freed on
 * every return path. */
enum { RRI_I32 = 8, RRI_I64 = 9 };     /* dtype codes of the index arrays of rri_corpus_create */
#define RRI_CORPUS_INFO_FIELDS 10
typedef struct rri_corpus rri_corpus;  /* opaque */
rri_status rri_corpus_create(rri_ctx* ctx, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t nnz_stored,
                             const void* indptr, int32_t indptr_dtype, const void* indices, int32_t indices_dtype,
                             const void* values, int32_t values_dtype, int32_t on_device);
rri_status rri_corpus_destroy(rri_corpus* corpus);
/* out[0 .. n): rows, columns, stored entries, canonical entries, rows rewritten (rows that were not strictly ascending without a
 * stored zero), duplicates merged (stored entries minus distinct columns, per row), zeros dropped (distinct columns whose sum is
 * 0), negative canonical values, device bytes, long rows (rewritten rows too long for LDS) -- RRI_CORPUS_INFO_FIELDS of them, a
 * longer out is zero-filled; *ingest_ms (may be NULL): the HIP-event time of the ingest's kernels. */
rri_status rri_corpus_info(const rri_corpus* corpus, int64_t* out, int32_t n, double* ingest_ms);
/* the canonical arrays on the host: indptr_out n_rows + 1, indices_out and values_out canonical entries each; any may be NULL */
rri_status rri_corpus_get(rri_ctx* ctx, const rri_corpus* corpus, int64_t* indptr_out, int32_t* indices_out, double* values_out);
rri_status rri_corpus_memory(int64_t* corpora, int64_t* bytes);
/* rri_cooccurrence_counts over the pattern of a resident corpus: the same kernels read the resident arrays, nothing of the
 * corpus's size is copied, the same counts. */
rri_status rri_corpus_cooccurrence_counts(rri_ctx* ctx, const rri_corpus* corpus, const int32_t* words, int32_t n_groups,
                                          int32_t group_size, int64_t* df_out, int64_t* codf_out);
/* rri_entries_loglik over the whole of a resident corpus: request q is corpus row q, rows is NULL (row q of W) or n_rows rows of
 * W; the outputs have n_rows entries.  The same bits as rri_entries_loglik on the canonical arrays.  RRI_ERR_INVALID also for a
 * corpus with negative values or with n_cols != d; RRI_ERR_UNSUPPORTED for 12 d > 64 MiB as there. */
rri_status rri_corpus_entries_loglik(rri_ctx* ctx, const rri_corpus* corpus, const int64_t* rows, double floor,
                                     double* ll_out, double* mass_out, int64_t* floored_out);
/* ---- the fit from a resident corpus ----------------------------------------------------------------------------------------------
 * rri_upload_X_corpus: X of an RRI_UNWEIGHTED_SPARSE handle from a corpus, without the host.  The corpus's canonical arrays are
 * copied device to device (12 bytes per entry, once) and the handle's blocked store -- the canonical CSR in the storage type and
 * the two blocked copies with their segment pointers, 16-bit offsets, permutations, values and work items -- is built on the
 * device by count, padded scan, claim and a sort of every claimed segment by canonical position: the same bytes as
 * rri_upload_X_csr leaves for the same matrix on the same device, whatever the scheduling.  Only the segment pointers (8 nblk
 * (nseg + 1) bytes per copy) cross to the host, where the work items are cut by the cutter of rri_upload_X_csr.  The handle owns
 * all its buffers: the corpus is not modified, not kept, and may be destroyed right after the call.  Uniform rows are cleared
 * as by rri_upload_X_csr.  Blocking.  RRI_ERR_INVALID for a NULL or destroyed corpus, one on another device, one whose shape is
 * not (n, d), and for a handle that is not RRI_UNWEIGHTED_SPARSE; RRI_ERR_UNSUPPORTED for 2^31-1 canonical entries or more and
 * for an RRI_F16 / RRI_U8 handle.  A refusal leaves the handle's store and every counter as they were.  Negative values are
 * accepted, as by rri_upload_X_csr.
 * rri_sparse_store_get: blocked copy `which` (0: rows as segments, 1: columns as segments) of any handle that has a blocked
 * store, whichever route built it -- for tests and probes.  info[0 .. n_info): nblk, bw, nseg, gdim, count (entries incl. the
 * padding of every segment to a multiple of 4), nwork, lps, nnz, longest row, and the HIP-event time in microseconds of the
 * kernels of a device build (0: the host built the store) -- RRI_SPARSE_STORE_INFO_FIELDS of them, a longer info is zero-filled.
 * segptr: nblk (nseg + 1) entries; idx, perm, val: max(count, 4) entries, val in the handle's storage type; work: 4 ints per
 * item (block, first segment, end segment, copy).  Any array pointer may be NULL.  RRI_ERR_INVALID without a blocked store. */
#define RRI_SPARSE_STORE_INFO_FIELDS 10
rri_status rri_upload_X_corpus(rri_ctx* ctx, const rri_corpus* corpus);
rri_status rri_sparse_store_get(rri_ctx* ctx, int32_t which, int64_t* info, int32_t n_info, int64_t* segptr, uint16_t* idx,
                                int32_t* perm, void* val, int32_t* work);
/* device-side copy of (W,T) for the early-stop rollback of nmf.py:360-363,393-407 */
rri_status rri_snapshot(rri_ctx* ctx);
rri_status rri_rollback(rri_ctx* ctx);

/* Products with the resident X for the initialisation (randomized SVD behind NNDSVD, initialization.py:105;
 * SURVEY 8f rank 2): out = X B (B: d x m host row-major, out: n x m) and out = X^T Q (Q: n x m, out: d x m),
 * float64 arithmetic on the stored X.  Blocking; not part of the sweep path.  On a pattern-only handle X is the
 * matrix of the observed values (= W_mat .* X, what initialization.py:104 factorises for the weighted flavour)
 * and m <= 64 per call. */
rri_status rri_X_times(rri_ctx* ctx, const double* B, int32_t m, double* out);
rri_status rri_Xt_times(rri_ctx* ctx, const double* Q, int32_t m, double* out);
/* The whole range finder of that randomized SVD in one call, its panels resident on the device (sklearn.utils.extmath.
 * randomized_svd behind initialization.py:105: n_iter rounds of Q <- normalise(A Q), Q <- normalise(A^T Q); Q <- orth(A Q);
 * B = Q^T A), with A = X (transpose = 0; Q0: d x m) or A = X^T (transpose = 1, scikit-learn's choice when n < d; Q0: n x m).
 * Every normalisation is (shifted) Cholesky-QR, three passes, instead of the host's LU / QR: another basis of the same range, so the SVD built
 * on Q and B (the small SVD of B stays with the caller) is scikit-learn's up to rounding.  Q0, Q_out (rows of A x m) and
 * B_out (m x columns of A) are host arrays, row-major; 1 <= m <= 64.  Dense handles only. */
rri_status rri_range_finder(rri_ctx* ctx, const double* Q0, int32_t m, int32_t n_iter, int32_t transpose, double* Q_out,
                            double* B_out);
/* The same call for the handles that keep X sparse -- RRI_UNWEIGHTED_SPARSE (the CSR X) and RRI_WEIGHTED_SPARSE (X = the matrix
 * of the observed values, as rri_X_times takes it) --, which rri_range_finder refuses: same contract, same arguments, same
 * shifted Cholesky-QR in three passes (1e-9 trace shift in the first, pivots held at 1e-14 of their diagonal entry), float64
 * arithmetic on the stored values.  Both panels stay on the device as tall row-major matrices, the layout the sparse products
 * read and write; all sums are taken in a fixed order, so a rerun gives the same bits.  RRI_ERR_INVALID on a dense handle, before
 * an upload, for m outside 1..64, n_iter < 0 and NULL arrays.  Rank-local (a handle with a communicator works on its own rows);
 * borrows no buffer of the handle: a factorisation in progress goes on as if the call had not been made. */
rri_status rri_sparse_range_finder(rri_ctx* ctx, const double* Q0, int32_t m, int32_t n_iter, int32_t transpose, double* Q_out,
                                   double* B_out);

/* Preprocessing of the resident dense X in place (unweighted handles):
 *   rri_column_positive_counts  df[j] = #{i : X[i,j] > 0}, the document frequencies of tfidf (matrixops.py:169)
 *   rri_scale_X                 X[i,j] <- (X[i,j] * col_scale[j]) / (sum_j X[i,j] * col_scale[j] + spacing(1)) when
 *                               normalize_rows != 0 (rows summing to < 1e-10 become 1/d: normalize, matrixops.py:139-147),
 *                               else X[i,j] * col_scale[j] (X * idf, matrixops.py:172); col_scale == NULL: all ones.
 * float64 arithmetic, rounded to the handle's storage type when stored.
 * On an RRI_U8 handle no matrix is written: df counts the stored counts > 0 whatever the scales are, and rri_scale_X does
 *   cscale[j] *= col_scale[j];  normalize_rows: rscale[i] *= 1 / (sum_j C[i,j] * cscale[j] * rscale[i] + spacing(1)).
 * Counts cannot hold the dense row 1/d: when rows would sum to < 1e-10 the call changes nothing and fails with RRI_ERR_INVALID,
 * its message (rri_last_error) starting with their number: "<count> row(s) ...". */
rri_status rri_column_positive_counts(rri_ctx* ctx, double* df_out);
rri_status rri_scale_X(rri_ctx* ctx, const double* col_scale, int32_t normalize_rows);
/* The two scale vectors of an RRI_U8 handle (RRI_ERR_INVALID on every other): row_scale has n entries, col_scale d, float64 on the
 * host.  set: NULL leaves that vector as it is; a change of a scale is a change of X.  get: NULL skips that vector. */
rri_status rri_set_X_scales(rri_ctx* ctx, const double* row_scale, const double* col_scale);
rri_status rri_get_X_scales(rri_ctx* ctx, double* row_out, double* col_out);
/* The same two steps (matrixops.py:124-179) on the X of an RRI_UNWEIGHTED_SPARSE handle; RRI_ERR_INVALID on every other handle
 * and before rri_upload_X_csr.  The stored values are rewritten and both blocked copies gathered from them again.
 *   rri_csr_column_positive_counts  df[j] = number of STORED entries of column j that are > 0 (explicit zeros do not count):
 *                               exact integers, the same bits on every run.
 *   rri_csr_scale_X             x <- (1 / tot[i]) * (x * col_scale[j]) with tot[i] = sum_j x * col_scale[j] + spacing(1) when
 *                               normalize_rows != 0 (matrixops.py:139-142), else x * col_scale[j] (:172); col_scale == NULL: ones.
 *                               float64 arithmetic, one rounding to the storage type.  A row with tot[i] < 1e-10 -- an empty one,
 *                               or a document made only of terms whose idf is 0 -- would become the DENSE row 1/d (:143-147),
 *                               which the pattern cannot take: the totals are therefore taken before anything is written, and
 *                               when there are such rows X is left bit for bit as it was, *zero_rows_out is their number (> 0)
 *                               and the call returns RRI_OK; the caller preprocesses that matrix on the host.  Otherwise
 *                               *zero_rows_out = 0.  zero_rows_out may be NULL only when normalize_rows == 0. */
rri_status rri_csr_column_positive_counts(rri_ctx* ctx, double* df_out);
rri_status rri_csr_scale_X(rri_ctx* ctx, const double* col_scale, int32_t normalize_rows, int64_t* zero_rows_out);
/* Uniform rows of an RRI_UNWEIGHTED_SPARSE handle: the dense rows that normalisation makes of zero-total rows, kept BESIDE the
 * pattern.  With U a sorted list of rows and c a value, the X every entry point of the handle sees is X = S + c e_U 1^T: S is
 * the stored CSR with zeros in the rows of U, and row i in U is the dense row c for every column j < d.  Sweeps (both halves
 * free or fixed), the objective in both forms, the max-residual reset (a uniform row can win it: T[t,:] becomes the dense
 * max(c - (W T)_i, 0)), rri_X_times / rri_Xt_times and rri_sparse_range_finder all work on that X; each adds the rows' share
 * in a fixed order, float64, no atomics, so a rerun is bit-identical.  With U empty (the default) nothing is launched for it.
 * RRI_ERR_INVALID on every other handle and before rri_upload_X_csr; rri_upload_X_csr empties U.
 *   rri_set_uniform_rows      declares rows[0 .. count) of the resident X as the dense row `value`: their stored values become 0
 *                             (the pattern is unchanged) and both blocked copies are gathered again.  rows may be unsorted; they
 *                             are kept sorted.  count == 0 clears the list.  A list the handle already has is REPLACED (its rows
 *                             stay rows of zeros unless listed again).  RRI_ERR_INVALID, with nothing changed, for a duplicate, a
 *                             row outside [0, n), a non-finite value.  Everything the handle has cached of X is dropped.
 *                             The list is replaced after the store has been rewritten: a call that fails on the device keeps
 *                             the list the handle had.
 *   rri_get_uniform_rows      *count_out = |U|, *value_out = c (0 while U is empty), rows_out[0 .. |U|) = U when capacity >= |U|.
 *                             rows_out == NULL asks for the count alone; a capacity that is too small is RRI_ERR_INVALID.
 *   rri_csr_scale_X_uniform   rri_csr_scale_X, except that rows with tot[i] < 1e-10 do not stop it: they take zeros, every other
 *                             row the normalised values, and the handle keeps them as its uniform rows with the value 1.0 / d
 *                             (float64, as matrixops.py:146 writes it).  *uniform_rows_out = |U| (may be NULL).  Without
 *                             normalize_rows there are no totals and no uniform rows.
 * On a handle that HAS uniform rows rri_csr_scale_X, rri_csr_scale_X_uniform and rri_csr_column_positive_counts answer
 * RRI_ERR_INVALID and leave X alone: a second preprocessing of such an X is not built.  While frozen statistics are set (below)
 * rri_set_uniform_rows with count > 0, and rri_csr_scale_X_uniform where rows would be collected, answer RRI_ERR_UNSUPPORTED
 * and change nothing: a handle never has both. */
rri_status rri_set_uniform_rows(rri_ctx* ctx, const int32_t* rows, int64_t count, double value);
rri_status rri_get_uniform_rows(rri_ctx* ctx, int32_t* rows_out, int64_t capacity, int64_t* count_out, double* value_out);
rri_status rri_csr_scale_X_uniform(rri_ctx* ctx, const double* col_scale, int32_t normalize_rows, int64_t* uniform_rows_out);

/* ---- row-sharded multi-GPU inside the library (one process per GPU; SURVEY 8b "sharded by row block internally",
 *      8e).  The reference has one call for the whole X (nmf.py:98-108); here every rank creates a handle for its row
 *      block [row_offset, row_offset + n) of the n_global-row problem (W rows alike, T replicated), attaches the
 *      process's communicator, and then calls the SAME entry points -- rri_sweep, rri_resume, rri_update_*,
 *      rri_objective, rri_apply_reset_* -- collectively, with the same arguments on every rank.  The one cross-row
 *      reduction of a topic step ([w_t^T X | w_t^T W | ||w_t||^2 | sum W[:,t-1]], or [numerator | denominator] of the
 *      weighted flavour) is all-reduced by RCCL over xGMI on the handle's stream between two kernels: a sweep is ONE
 *      call with no host work per topic.  Every decision (reset events, the assert of nmf.py:476, unbounded cases)
 *      is taken from all-reduced or replicated values, so all ranks return the same status.
 *      All flavours and flags of rri_sweep: fixed halves, k = 1, weighted dense and pattern-only, and the explicit-residual
 *      schedule (RRI_UNWEIGHTED_RESIDUAL: every rank keeps its rows of R; the sums it sends are the same message). */
/* rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks by any channel the host program has */
rri_status rri_comm_unique_id(uint8_t* id_out /* RRI_COMM_ID_BYTES */);
/* RCCL communicator of `world` ranks; this process is `rank` and drives HIP device `device`.  Collective. */
rri_status rri_comm_create(rri_comm** out, const uint8_t* id, int32_t rank, int32_t world, int32_t device);
/* The same protocol over the CALLER's transport (tests with several ranks on one GPU; hosts without RCCL): the
 * library drains the stream, hands `count` doubles in host memory to the function and copies the result back.
 * Each function returns 0 on success.  allreduce: sum in place over the ranks; allgather: recv = world x count;
 * broadcast: from `root` in place. */
typedef int32_t (*rri_allreduce_fn)(void* user, double* buf, int64_t count);
typedef int32_t (*rri_allgather_fn)(void* user, const double* send, int64_t count, double* recv);
typedef int32_t (*rri_broadcast_fn)(void* user, double* buf, int64_t count, int32_t root);
rri_status rri_comm_create_host(rri_comm** out, int32_t rank, int32_t world, rri_allreduce_fn allreduce,
                                rri_allgather_fn allgather, rri_broadcast_fn broadcast, void* user);
rri_status rri_comm_destroy(rri_comm* comm);     /* after every handle it was attached to is destroyed */
/* comm == NULL detaches.  row_offset: global index of the handle's first row. */
rri_status rri_attach_comm(rri_ctx* ctx, rri_comm* comm, int64_t row_offset, int64_t n_global);
/* small host-side collectives for the host driver (the vectors of a 'random' reset drawn on rank 0, nmf.py:778-783;
 * stop decisions; the d x m panels of a row-sharded randomized SVD): no-ops on a handle without a communicator. */
rri_status rri_comm_broadcast(rri_ctx* ctx, double* host, int64_t count, int32_t root);
rri_status rri_comm_allreduce_sum(rri_ctx* ctx, double* host, int64_t count);
rri_status rri_comm_stats(rri_ctx* ctx, int32_t* rank, int32_t* world, int64_t* allreduce_calls);

/* ---- row-sharded stepping with the collective in the CALLER's hands (the protocol the calls above run inside
 *      rri_sweep; kept for hosts that own their collectives and for the Gaussian mechanism, whose noise enters at the
 *      same point) ---- */
/* A topic step splits at the one cross-row reduction it needs.  rri_topic_reduce_local
 * leaves this rank's partial sums [w_t^T X (LD) | RRI_GRAM_SLICES x (w_t^T W (k), ||w_t||^2, sum W[:,t-1])]
 * (LD = d rounded up to the 16-byte row stride; a Gram entry is the sum of its slices)
 * in the reduce buffer; the caller all-reduces (sum) that buffer over the ranks (RCCL over
 * xGMI via torch.distributed) and calls rri_topic_finish, which is rank-local.
 * Weighted handles (WRRI, nmf.py:687-701): the buffer is [numerator w_t^T Rt (LD) | denominator
 * (w_t^2)^T M (LD) | sum of W[:,t-1], its negative-denominator flag], LD = d rounded up to the
 * 16-byte row stride; same protocol (one all-reduce of [numerator | denominator] per topic). */
rri_status rri_reduce_buffer(rri_ctx* ctx, void** dev_ptr, int64_t* n_elems); /* dtype = handle's */
rri_status rri_bind_reduce_buffer(rri_ctx* ctx, void* dev_ptr, int64_t n_elems);
/* (T must be free; W may be fixed -- the step is then the T row alone, the kept column taking its scale, nmf.py:450-452 -- and
 * k may be 1: the reference's loop, nmf.py:417-456, has no limit there.) */
rri_status rri_topic_reduce_local(rri_ctx* ctx, int32_t t);
/* Host access to the first `count` doubles of the reduce buffer between rri_topic_reduce_local and
 * rri_topic_finish: what a caller needs to perturb the T-row sums -- the Gaussian mechanism of nmf.py:422-435
 * adds its noise to wR and nw there.  Blocking. */
rri_status rri_reduce_read(rri_ctx* ctx, double* out, int64_t count);
rri_status rri_reduce_write(rri_ctx* ctx, const double* in, int64_t count);
rri_status rri_topic_finish(rri_ctx* ctx, int32_t t);
/* only the W-column half of topic t (a sharded run resuming after a T-row reset) */
rri_status rri_topic_finish_w(rri_ctx* ctx, int32_t t);
/* Pieces of the 'max_resid_document' reset for a sharded run (nmf.py:771-776): the largest
 * sum_j max(X - W T, 0)_ij^2 over THIS rank's rows and its local row index; and the reset row
 * max(X[i,:] - W[i,:] T, 0) of a local row (d doubles to the host).  The caller picks the global winner. */
rri_status rri_resid_row_argmax(rri_ctx* ctx, double* value, int64_t* local_row);
rri_status rri_reset_row(rri_ctx* ctx, int64_t local_row, double* row_out_host);
/* status word of the interrupted / failed step after a stream sync (same codes as rri_sweep) */
rri_status rri_poll(rri_ctx* ctx);
/* rank-local pieces of the objective: out[0] = 0.5*sum (Wm.)(X-WT)^2 over local rows,
 * out[1] = sum W^2, out[2] = sum |W| (local rows); T terms are replicated. */
rri_status rri_objective_parts(rri_ctx* ctx, double out[3]);

/* ---- rows that left the device, kept as frozen statistics (online fits; rri_frozen.hpp) ---- */
/* A T-row step sees the rows of X and W only through the sums a row-sharded run all-reduces.  Rows O whose W no longer changes
 * are therefore replaced by B = W_O^T X_O (k x d, row-major), A = W_O^T W_O (k x k), s = 1^T W_O (k) and c = ||X_O||^2, all
 * float64: one more rank that never moves.  While statistics are set, every T-row step and every column check of rri_sweep,
 * rri_resume, rri_update_T_row and rri_topic_reduce_local / rri_topic_finish is that of the stacked problem [X_O; X] in which
 * the rows W_O are never updated: the statistics are added on the device into the reduce buffer, after the handle's own sums
 * (the Gram terms into slice 0).  The fused T-row launch of small sizes and the persistent sweep do not have that buffer and
 * are not taken (rri_onchip_info: eligible = 0; rri_sweep_until: RRI_ERR_UNSUPPORTED); sweeps with T fixed ignore the
 * statistics; rri_objective and rri_objective_parts[0] add the frozen rows' share 1/2 (c - 2 <B, T> + <A, T T^T>).  A reset
 * of topic t (rri_apply_reset_max_resid, rri_apply_reset_vectors) zeroes row t of B, row and column t of A and s[t]: W[:,t] = 0
 * of nmf.py:775 on the frozen rows; only the handle's own rows are reset candidates.
 * Handles: RRI_UNWEIGHTED with RRI_F32 or RRI_F64 storage, and RRI_UNWEIGHTED_SPARSE without uniform rows.
 * RRI_ERR_UNSUPPORTED, with nothing changed: weighted handles, RRI_UNWEIGHTED_RESIDUAL, RRI_F16 and RRI_U8, uniform rows (and,
 * while statistics are set, rri_set_uniform_rows with count > 0 and an rri_csr_scale_X_uniform that would collect rows), an
 * attached communicator (and rri_attach_comm while statistics are set); rri_sweep, rri_update_T_row, rri_topic_reduce_local
 * and rri_topic_finish with fix_W while statistics are set (the W[:,t] *= nt1 of nmf.py:450-452 would have to reach the frozen
 * rows).  Arguments are checked before any HIP call. */
/* Sets the statistics: all values finite, B, A, s >= 0, A symmetric, c >= 0; the count of absorbed rows starts from 0.
 * B == NULL clears them (on any handle) and frees their device memory. */
rri_status rri_frozen_set(rri_ctx* ctx, const double* B, const double* A, const double* s, double c);
/* Reads them back; any pointer may be NULL.  RRI_ERR_INVALID when none are set. */
rri_status rri_frozen_get(rri_ctx* ctx, double* B_out, double* A_out, double* s_out, double* c_out, int64_t* rows_out);
/* F <- decay F + (W^T X, W^T W, 1^T W, ||X||^2) of the handle's own rows and current W, decay in (0, 1]; from zeros when
 * nothing is set; the row count grows by n.  W^T X of a dense handle is one pass over X on the float64 matrix cores (k <= 128;
 * one pass per 128 topics above), of a CSR handle the blocked product behind rri_Xt_times (cost ~ nnz).  No atomics: the same
 * call on the same state leaves the same bits.  W, T and everything the handle keeps between steps are left as they were. */
rri_status rri_frozen_absorb(rri_ctx* ctx, double decay);

/* ---- measurement --------------------------------------------------------------- */
/* HIP-event timing of the streaming kernels on the handle's stream.  kernel_id:
 * 0 = fused X pass (row dots + column sums), 1 = W-column update, 2 = T-row update chain,
 * 3 = rank-one residual update (explicit-residual / WRRI flavour); on an RRI_UNWEIGHTED_SPARSE handle with uniform rows: the
 *     launch that adds their share after every X pass (also inside the bracket of id 0),
 * 4 = the launch of rri_topn_rows, 5 = the launch of rri_rank_entries,
 * 6 = the launches of rri_cooccurrence_counts: two per row chunk (masks, then counts), each in a bracket of its own,
 * 7 = the launches of rri_entries_loglik: the transposed copy of T once per call, then two per chunk of requests (entries, then
 *     the sum over a request's pieces), each in a bracket of its own,
 * 8 = the launches of rri_frozen_absorb: per chunk of topics the panel W^T X and the sum of its row-block partials (CSR: the
 *     transposed copy of the chunk's columns of W, the blocked product and its accumulation) in one bracket, then W^T W with
 *     1^T W in a bracket of its own.  (The addend of a handle with frozen statistics sits inside the bracket of id 2.) */
/* on = 0: off; on = N > 0: bracket every N-th launch of each kernel id with an event pair (N = 1: all).
 * An event record costs a bubble of a few microseconds on the stream, so sample when the timed region is
 * also the throughput measurement. */
rri_status rri_timing_enable(rri_ctx* ctx, int32_t on);
rri_status rri_timing_read(rri_ctx* ctx, int32_t kernel_id, int64_t* launches, double* total_ms);
rri_status rri_synchronize(rri_ctx* ctx);
/* Launch-bound sizes: when X fits the registers of the chip -- 40 MB: about 10000 x 1024 or 5000 x 2048 in fp32, half the rows in
 * float64 -- and the configuration is the unweighted one with both halves free (plain with d <= 2048, or the topic-model flags
 * with T rows projected at every step and d <= 1024), k in 2..64, one device, rri_sweep / rri_resume run as ONE persistent
 * launch with X resident on chip and two (topic model: three) exchanges between workgroups per topic step
 * (rri_onchip_kernels.hpp) instead of three or four launches per topic step; the whole launch is then timed as kernel_id 0.  *eligible: would the next
 * rri_sweep take that path; *launches: how many it has taken on this handle.  RRI_ONCHIP=0 (environment, read by
 * rri_create) switches it off.  Either pointer may be NULL. */
rri_status rri_onchip_info(rri_ctx* ctx, int32_t* eligible, int64_t* launches);
/* What the handle decided about its layout and routes, for tests and diagnostics; changes nothing.  Fills out[0 .. min(n,
 * RRI_LAYOUT_FIELDS)):
 *   0..3   the row copy of a blocked CSR store (pattern-only weighted and CSR-X handles, after the upload; 0 on dense handles):
 *          column blocks, block width (factors per LDS table), lanes per segment, work items;   4..7  the same of the column copy
 *   8..10  rows per row block, row blocks and column panels of the streaming pass (blocked store: 10 = column blocks of the row
 *          copy, 9 = row blocks of the column copy)
 *   11     a bit-packed 0/1 mask exists;   12  its column-major copy exists;   13  the measured mask density in 1e-9, -1 before
 *          it has been measured (the column-major copy is made, or given up, by the first topic step that wants it)
 *   14     dense weighted: rri_sweep takes the fused T-row launch (few row blocks, one device)
 *   15     dense weighted: the last T-row step took nw = (w^2)^T M from the mask-only kernel, not from the pass
 *   16     dense handles: read-only passes deal their row blocks interleaved (few workgroups)
 *   17     row blocks of the last mask-only correction launch (0 before the first);   18  compute units of the device (the cap
 *          of a blocked copy's work items)
 *   19     the read-only pass streams the packed 28-bit copy of an fp32 X (RRI_X_PACK; decided by the first sweep after X was set);
 *          20  the first top byte of its window;   21  tiles (8 rows x 1024 columns) with an element outside the window, read as
 *          fp32 (with more than 1/8 of them flagged there is no copy: 19 is 0, 21 and 22 say why);   22  tiles in all
 *   23     bits per element of the copy the pass streams: 28, 26 (the book-coded copy, rri_xnarrow.hpp; RRI_X_PACK=2, or unset and
 *          few exceptions) or 0;   24  the book of the 26-bit copy, its seven exponent bytes in bytes 0..6, else 0;   25  elements
 *          of X inside the window and outside the book (the exception entries of a 26-bit copy) as the last build counted them,
 *          -1 where none was counted
 *   26     the handle, with the parameters it has now, takes the early-sums schedule (RRI_EARLY_SUMS: the W-sized sums of a topic
 *          step ride in the grid of its pass) wherever a step's early partials are valid;   27  W-column steps that took it so far
 *   28     the workgroups of that job are dealt through the pass's grid behind its first round (RRI_EARLY_DEAL=1), not placed
 *          there in one run (unset or 0);   29  the pass's own workgroups between two of the job (0: one run -- the switch is off,
 *          or the pass has fewer workgroups behind its first round than the job) */
#define RRI_LAYOUT_FIELDS 30
rri_status rri_layout_info(rri_ctx* ctx, int64_t* out, int32_t n);
/* The exchanges of that launch poll a bounded number of times.  When its workgroups cannot all run at once (a device shared
 * with another process, CUs masked away) the launch gives up, and the call does what the reference's sweep does under any
 * scheduling (nmf.py:415-476): it completes -- W and T are put back to what they were before the launch and the same steps
 * run on the launch-per-phase schedule, which the handle then keeps for a while: 2 s after its first fallback, twice as long after
 * every further one up to 64 s (and every handle of the process stays off the path for RRI_ONCHIP_BACKOFF_MS, default 2000).
 * *eligible of rri_onchip_info and RRI_ERR_UNSUPPORTED of rri_sweep_until therefore depend on the clock after a fallback.
 * *fallbacks: how often that happened on this handle. */
rri_status rri_onchip_fallbacks(rri_ctx* ctx, int64_t* fallbacks);
/* The device buffers that handles of this process own at this moment, and their bytes: what rri_create, the uploads and the
 * buffers made on first use allocated and rri_destroy (or a replacement) has not yet freed.  Bound caller memory (rri_bind_*)
 * and the temporaries of a call are not counted.  Takes no handle, so it can be read after rri_destroy: both values are then
 * back where they were before rri_create.  Either pointer may be NULL. */
rri_status rri_device_memory(int64_t* buffers, int64_t* bytes);
/* diagnostics: the XCD (XCC_ID) each of `count` workgroups of a launch on the handle's stream lands on */
rri_status rri_debug_xcc(rri_ctx* ctx, int32_t* out, int32_t count);
/* The sweep / objective / stop-rule loop of nmf.py:377-516 for launch-bound sizes, in one call: up to n_sweeps sweeps of the
 * register-resident kernel with the objective of every sweep kept (true_objective, nmf.py:71-94, 488-490) and the rule of
 * nmf.py:510 / optimization.py:284-291 applied ON THE DEVICE after every sweep: the run ends after the first sweep s with
 * |o_s - o_(s-1)| <= stop_scale, where o_(-1) = obj_prev and the caller passes stop_scale = eps_stop |o_0 - o_1| of its run
 * (a negative stop_scale never stops).  *sweeps_done sweeps have run; obj_hist (room for n_sweeps doubles) holds their
 * objectives, NaN where the kernel left none -- the sweep an event interrupted (the call ends with that sweep once the event
 * is resolved and rri_resume has finished it) or a sweep run on the launch-per-phase schedule after a fallback (the call then
 * ends after one sweep): take rri_objective there.  RRI_ERR_UNSUPPORTED when the handle does not take the persistent
 * path (rri_onchip_info) or n_sweeps > 512: call rri_sweep / rri_objective sweep by sweep. */
rri_status rri_sweep_until(rri_ctx* ctx, int32_t n_sweeps, double obj_prev, double stop_scale, double* obj_hist,
                           int32_t* sweeps_done);
/* Stand-alone kernels for roofline measurement (bench.py): R <- R - a b^T fused with the
 * next residual products, on a scratch copy of X, with the handle's own W[:,0], T[0,:] as factors. */
rri_status rri_bench_rank1_update(rri_ctx* ctx, int32_t reps, double* avg_ms);
rri_status rri_bench_stream_copy(rri_ctx* ctx, int32_t reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* RRI_HIP_H */
