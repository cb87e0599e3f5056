// rri_halt.hpp -- the rules by which a sweep stops early, written once (DESIGN "Halting rules").
//
// A queue of topic steps runs without the host; what the reference decides between two steps -- reset a dead topic, fail an
// assertion, take another branch of qf_min -- is decided here by whichever kernel holds the sum in question.  It writes the
// halt record of DevState, every later kernel of the queue returns at once, and the host resolves the event (status_from_halt).
// The rules are the reference's and nothing else:
//     a W column that sums to zero      reset, or the assertion                  nmf.py:471-476, 787-816
//     a T row that sums to zero         reset                                    nmf.py:751-769
//     a scalar denominator c <= 0       bounds, one-hot, unbounded, "not implemented"     optimization.py:60-73
// (rri_sweep_until adds its stop rule, HALT_EVENT_STOP, in the persistent sweep.)  Every kernel that can meet one of them calls
// the functions below; a store to DevState::halt stands in this file alone, and so does the threshold 1e-10 beside
// reset_method -- but for the REMAINING COPIES: four sites inside the step loop of k_onchip_sweeps (rri_onchip_kernels.hpp)
// keep their own text of wcol_code, trow_denominator_mode, trow_resets and wcol_denominator_mode, because every wording
// through this header that was tried moves the register allocation of that loop, and the persistent sweep at 10000 x 1000,
// k = 20 then ran 6 % slower (profiles/r10_halt_bench_ab.log).  Outside its loop that kernel calls this header too.
//
// Plain inline functions, host and device: the host schedules with next_step, and the stand-alone CPU test compiles this
// header with the host compiler and checks every rule over the cross product of its inputs.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RRI_HALT_FN __host__ __device__ inline
#else
#define RRI_HALT_FN inline
#endif

namespace rri {

enum { HALT_EVENT_RESET_T = 1, HALT_EVENT_RESET_W = 2,
       HALT_EVENT_STOP = 3,    // the persistent sweep: the stop rule of nmf.py:510 held at the end of sweep halt_sweep - 1
       HALT_ERR_UNBOUNDED = -4, HALT_ERR_W_COL_ZERO = -5, HALT_ERR_NOT_IMPLEMENTED = -6 };
enum { RESET_NONE = 0, RESET_MAX_RESID = 1, RESET_RANDOM = 2 };

struct DevState {
    int halt;        // 0 = running, >0 event, <0 error
    int halt_topic;  // topic the event refers to
    int halt_sweep;  // position of the DETECTING step
    int halt_pos;
    int tmode;       // qf_min branch of the current T row: 0 c>0, 1 c<=0 bounds, 2 c<=0 one-hot
    int proj_iters;  // Michelot iterations of the last projection (diagnostic)
    int pad0;        // k_wsweep_verdict: first column k_wsweep_repair restores after a reset event (0: none); cleared with halt
    int pad1;        // k_wfold_verdict: 1 when the halt was found inside a one-launch fold sweep (rri_fold_info counts them); cleared with halt
    double nt1;      // 1-norm of the unprojected T-row solution (qf_min's nx, nmf.py:447)
    double nt;       // ||T[t,:]||^2
    double sumT;
    double theta;
    double obj_track;   // the persistent sweep: objective of the launch's last sweep minus 1/2 ||X||^2 (OnchipArgs.track)
};

struct KParams {
    int fix_W, fix_T, project_T, has_trs, has_wrs, reset_method, resets_left, pad;
    double t_row_sum, w_row_sum, reg_w_l1, reg_w_l2, reg_t_l1, reg_t_l2, eps;
};

// The halt record: what stopped the queue (code), the topic it refers to, and the position (sweep, pos) the host hands back.
// Which thread writes it -- one thread of one workgroup -- is the caller's business.
RRI_HALT_FN void halt_set(DevState* st, int code, int topic, int sweep, int pos) {
    st->halt = code; st->halt_topic = topic; st->halt_sweep = sweep; st->halt_pos = pos;
}

// _check_reset_W and the assertion after it (nmf.py:471-476, 793-816) on sum = sum(W[:,t]): 0 (the run goes on),
// HALT_EVENT_RESET_W (nw1 <= 1e-10, a reset method and resets left: nmf.py:794-801) or HALT_ERR_W_COL_ZERO (no reset, and
// `assert np.sum(W[:, t]) > 0` fails: nmf.py:476).
// One known difference from the reference: a NaN sum with resets left is HALT_ERR_W_COL_ZERO here (NaN <= 1e-10 is false),
// where the reference resets (`nw1 > 1e-10` is false too, nmf.py:794).  Kept as it is; the CPU test asserts it.
RRI_HALT_FN int wcol_code(double sum, const KParams& p) {
    if ((sum <= 1e-10) && p.reset_method != RESET_NONE && p.resets_left > 0) return HALT_EVENT_RESET_W;
    return !(sum > 0.0) ? (int)HALT_ERR_W_COL_ZERO : 0;
}

// The weighted flavour (vector c, optimization.py:75-77 with s = None, ub = w_row_sum): a negative denominator somewhere in
// the column (negflag > 0) and no upper bound is "unbounded"; then the column checks above.
RRI_HALT_FN int wwcol_code(double sum, double negflag, const KParams& p) {
    if (negflag > 0.0 && !p.has_wrs) return HALT_ERR_UNBOUNDED;
    return wcol_code(sum, p);
}

// _project_and_check_reset_t (nmf.py:757-769; oracle/rri_oracle.py:310-319) on sumT = sum(T[t,:]): the row is kept (and
// projected again where nmf.py:759-761 says so) ...
RRI_HALT_FN bool trow_kept(double sumT, const KParams& p) { return sumT > 1e-10 || p.reset_method == RESET_NONE; }
// ... or reset, while resets are left (nmf.py:765-769): HALT_EVENT_RESET_T.  With none left the row stays as it is.
RRI_HALT_FN bool trow_resets(double sumT, const KParams& p) { return !trow_kept(sumT, p) && p.resets_left > 0; }

// qf_min with the scalar denominator c = nw + reg_t_l2 of a T row (nmf.py:438-447; optimization.py:53-73), s = t_row_sum when
// the row is projected and None otherwise, ub = t_row_sum:
//     0  c > 0, the closed form                                   1  c <= 0, s None: entries jump to ub (:62-65)
//     2  c <= 0, s == 1: one-hot at the arg-max (:68-70)          HALT_ERR_UNBOUNDED (:67), HALT_ERR_NOT_IMPLEMENTED (:71-73)
// A NaN c takes the c <= 0 side.
RRI_HALT_FN int trow_denominator_mode(double c, const KParams& p) {
    if (c > 0.0) return 0;
    if (p.project_T && p.has_trs) return p.t_row_sum == 1.0 ? 2 : (int)HALT_ERR_NOT_IMPLEMENTED;
    return (p.has_trs && p.t_row_sum != 0.0) ? 1 : (int)HALT_ERR_UNBOUNDED;
}

// The same for the denominator cden = nt + reg_w_l2 of a W column (nmf.py:465-469: s = None, ub = w_row_sum): 0, 1 or
// HALT_ERR_UNBOUNDED (optimization.py:60-67).
RRI_HALT_FN int wcol_denominator_mode(double cden, const KParams& p) {
    if (cden > 0.0) return 0;
    return (p.has_wrs && p.w_row_sum != 0.0) ? 1 : (int)HALT_ERR_UNBOUNDED;
}

// The step after topic t of `sweep`: where a resumed run continues when the column verdict of step t halts the queue.
struct StepPos { int sweep, pos; };
RRI_HALT_FN StepPos next_step(int sweep, int t, int k) {
    return t + 1 == k ? StepPos{sweep + 1, 0} : StepPos{sweep, t + 1};
}

}  // namespace rri
