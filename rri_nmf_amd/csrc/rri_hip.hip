// rri_hip.hip -- librri_hip.so: host side of the C ABI declared in include/rri_hip.h.
//
// Build (see __graft_entry__.build / rri_nmf_amd/build.py):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC -Iinclude rri_nmf_amd/csrc/rri_hip.hip
//
// Data layout in HBM (one handle = one nmf() call = one row shard of one GPU).  X (and the mask /
// masked residual) are stored in the handle's dtype (fp32 or fp64; float16 for the read-only dense X of an RRI_UNWEIGHTED
// handle, DISPATCH_RO); everything else is float64:
//   X     n x LD   row-major, LD = d rounded up to a 16-byte multiple of X's type, pad columns zero
//   Wt    k x n    k-major (W transposed): column t of W is the contiguous row Wt[t,:], so the
//                  streaming pass stages the active column into LDS with coalesced loads
//   T     k x LD   row-major, pad columns zero
//   Ypart npanels x n      per-column-panel partial row dots of the pass
//   Zpart nrb x LD         per-row-block partial column sums of the pass
//   Gpart nwb x (k+2)      per-block partial Gram row / norm / column sum (float64)
//   red   LD + 8 (k+2)     reduced [w^T X | 8 slice sums of (w^T W, ||w||^2, sum W[:,t-1])]  (all-reduce payload)
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: the symbols are resolved at run time (rccl_api below), so the
                         // library has no link-time dependency on RCCL and loads on a box without it

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <set>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rri_hip.h"
#include "rri_layout.hpp"
#include "rri_pick.hpp"
#include "rri_kernels.hpp"
#include "rri_wrri_kernels.hpp"
#include "rri_sparse_kernels.hpp"
#include "rri_onchip_kernels.hpp"
#include "rri_topn_kernels.hpp"
#include "rri_rank_kernels.hpp"
#include "rri_cooc_kernels.hpp"
#include "rri_loglik_kernels.hpp"
#include "rri_frozen_kernels.hpp"
#include "rri_corpus_kernels.hpp"
#include "rri_spbuild_kernels.hpp"
#include "rri_corpus_ops.h"
#include "rri_derive_kernels.hpp"
#include "rri_corpus_build.h"
#include "rri_corpus_build_kernels.hpp"
#include "rri_corpus_fit.h"
#include "rri_fiterr_kernels.hpp"
#include "rri_corpus_rank.h"
#include "rri_corpus_rank_kernels.hpp"
#include "rri_fold.h"
#include "rri_fold_kernels.hpp"
#include "rri_corpus_rowsplit.h"
#include "rri_rowsplit_kernels.hpp"

using namespace rri;

namespace {

thread_local std::string g_create_error;   // text of the last failed rri_create of this thread

struct Cursor {
    int sweep, topic, phase;  // phase 0 = T-row half, 1 = W-column half
};

struct TimedLaunch {
    hipEvent_t a, b;
};

}  // namespace

// ---- communicator of a row-sharded run (one process per GPU) ---------------------------------------------------
// RCCL entry points, looked up in the process (a host program that already carries an RCCL -- PyTorch-ROCm ships its
// own, bound to its own HIP runtime -- must be the one used: two HIP runtimes in one process do not share streams) and
// only then in librccl.so.1.  RRI_RCCL_LIB names another file.
namespace {
struct RcclApi {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;     // optional: what a rank that fails between two matched collectives calls
    bool ok = false;
    std::string err;
};
RcclApi load_rccl() {
    RcclApi a;
    void* h = nullptr;
    auto resolve = [&](void* from) {
        a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(from, "ncclGetUniqueId");
        a.CommInitRank = (decltype(a.CommInitRank))dlsym(from, "ncclCommInitRank");
        a.CommDestroy = (decltype(a.CommDestroy))dlsym(from, "ncclCommDestroy");
        a.AllReduce = (decltype(a.AllReduce))dlsym(from, "ncclAllReduce");
        a.AllGather = (decltype(a.AllGather))dlsym(from, "ncclAllGather");
        a.Broadcast = (decltype(a.Broadcast))dlsym(from, "ncclBroadcast");
        a.GetErrorString = (decltype(a.GetErrorString))dlsym(from, "ncclGetErrorString");
        a.CommAbort = (decltype(a.CommAbort))dlsym(from, "ncclCommAbort");
        return a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce && a.AllGather && a.Broadcast &&
               a.GetErrorString;
    };
    if (const char* e = getenv("RRI_RCCL_LIB")) {
        h = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
        if (h && resolve(h)) { a.ok = true; return a; }
        a.err = std::string("RRI_RCCL_LIB=") + e + " could not be used";
        return a;
    }
    if (resolve(RTLD_DEFAULT)) { a.ok = true; return a; }
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h && resolve(h)) { a.ok = true; return a; }
    }
    a.err = "RCCL not found (no ncclAllReduce in the process, no librccl.so.1)";
    return a;
}
RcclApi& rccl_api() {
    static RcclApi api = load_rccl();
    return api;
}
}  // namespace

struct rri_comm {
    int rank = 0, world = 1, device = 0;
    ncclComm_t nccl = nullptr;                 // RCCL transport (xGMI), or
    rri_allreduce_fn h_allreduce = nullptr;    // host-callback transport (tests: several ranks on one GPU)
    rri_allgather_fn h_allgather = nullptr;
    rri_broadcast_fn h_broadcast = nullptr;
    void* user = nullptr;
    std::vector<double> hbuf, hbuf2;           // host staging of the callback transport
    long n_allreduce = 0;
    bool aborted = false;                      // a rank left a collective sequence half way: the communicator is unusable
};

// (the environment switches a handle keeps, rri_switches, and every rule of its geometry: rri_layout.hpp)
struct rri_ctx {
    i64 n = 0, d = 0, LD = 0;
    int k = 0, dtype = RRI_F32, weighted = 0, device = 0;
    size_t es = 4;  // element size of X / mask / residual; all other buffers are float64
    double store_err[2] = {0.0, 0.0};   // rri_storage_error: sum (x - stored(x))^2 and sum x^2 of the last rri_upload_X
    int VN = 4, PW = 1024;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    rri_switches sw;
    DensePlan plan;   // what dense_plan (rri_layout.hpp) decided at rri_create; the geometry members below are copies of its fields

    void *X = nullptr, *M = nullptr, *E = nullptr;
    i64 ldx = 0, ldm = 0;
    // what the handle allocated (dev_alloc, dev_adopt) and rri_destroy frees: the field that holds it, the pointer, its size.  X, M
    // and red may hold bound caller memory instead, which is not listed here and therefore never freed
    struct Owned { const void* field; void* p; size_t bytes; };
    std::vector<Owned> owned;
    double *W = nullptr, *T = nullptr, *Wprev = nullptr, *Tprev = nullptr;
    double *Ypart = nullptr, *Zpart = nullptr, *red = nullptr, *xraw = nullptr, *Ttpart = nullptr;
    unsigned* Mbits = nullptr;   // bit-packed 0/1 mask (weighted flavour), ldb words per row; NULL = fp mask in M
    i64 ldb = 0;
    double* Qt = nullptr;     // X T^T (k x n), valid while T is fixed
    bool q_valid = false;
    // tile -> XCD rotation of the passes over X (read only) and over the stored residual (read-modify-write): 0 or 1, the faster
    // of the two for THIS handle's buffers (calibrate_rot); RRI_PASS_ROT forces one for all
    int rot_x = 0, rot_r = 0;
    bool rot_done = false;
    int ro_il = -1;    // read-only pass: interleaved (1) or contiguous (0) row chunks forced by RRI_PASS_PK_GEOM; -1: by the workgroup count
    int keep_q = -1;   // read-only pass over X: row blocks loaded with default policy, the others non-temporally; -1: all of X plain (pass_keep)
    // the packed copy of an fp32 X that the read-only pass streams instead of X (rri_xpack.hpp; xpack_ensure): 3.5 bytes per element
    unsigned char *xp = nullptr, *xp_flags = nullptr;   // the records; one flag byte per 8-row chunk and column group (tile)
    unsigned* xp_hmax = nullptr;                        // device: the largest top byte of X inside [1, 0x7e]
    // ... or its 26-bit copy (rri_xnarrow.hpp; xnarrow_build): the fixed parts of the records, the directory of their exception
    // entries, the entries.  xn_valid (with xp_valid): the passes read this one; flags, window and base are the 28-bit format's
    unsigned char* xn = nullptr;
    unsigned* xn_dir = nullptr;
    unsigned short* xn_exc = nullptr;
    bool xn_valid = false;
    xnarrow::Books xn_books = {};
    i64 xn_exceptions = -1;     // elements of X inside the window and outside the 7-entry book, as the histogram counts them; -1: not counted
    // RRI_U8: the X every kernel sees is (C[i][j] * cscale[j]) * rscale[i]; rscale[n], cscale[LD] (pad columns: 1), ones until set
    double *rscale = nullptr, *cscale = nullptr;
    bool xp_valid = false;      // the passes read xp: it was built from the X the handle holds and few enough tiles are flagged
    bool xp_done = false;       // ... or the question is settled for this X (not wanted, no memory, too many flagged tiles)
    int xp_base = 0;            // the window of top bytes: xp_base .. xp_base + 14
    i64 xp_flagged = 0, xp_tiles = 0;
    bool gfull_valid = false;   // Gfull = T T^T of the current T (k_wsweep_rows)
    double *Gfull = nullptr, *Wsweep0 = nullptr, *wsum_part = nullptr, *wsums = nullptr;   // whole-sweep W half with T fixed: lazily allocated
    // ... and its form for a pattern-only handle (rri_fold.h; k_wfold_rows): asked for with rri_set_fold_schedule, for the handle's
    // life.  fold_part: per topic and workgroup the column sum, then the count of negative denominators (2 k fold_nwg doubles,
    // allocated by the first such sweep, like Wsweep0).  tt_valid: sp_Tt holds the transpose of the handle's current T
    bool fold_asked = false, tt_valid = false;
    double* fold_part = nullptr;
    long fold_launches = 0, fold_stepped = 0, fold_halts = 0;   // sweeps as one launch; sweeps launch by launch while asked; halts in a launch
    double *Y2part = nullptr, *Z2part = nullptr, *dtv = nullptr, *dwv = nullptr, *wold = nullptr, *zeros = nullptr;  // weighted
    i64 ldw = 0;     // row stride of the k-major W (>= n)
    int nsplit = 4;  // column slices of k_tgram
    i64 red_elems = 0;
    // weighted flavour on a CSR observation pattern (rri_upload_observed_csr): no dense n x d array at all
    bool sparse = false;
    i64 nnz = 0;
    int sp_max_row = 0, kp = 8;
    i64* sp_rowptr = nullptr;   // canonical CSR of the pattern with X on it: residual rebuild, objective, resets
    int* sp_col = nullptr;
    void *sp_x = nullptr, *sp_e = nullptr;
    double* sp_Tt = nullptr;    // T transposed, d x kp
    // the two blocked copies of the residual (rri_sparse_kernels.hpp): [0] rows as segments, cut into column
    // blocks; [1] columns as segments, cut into row blocks
    struct SpCopy {
        int nblk = 1, bw = 1, lps = 64, nwork = 0;
        i64 nseg = 0, gdim = 0, count = 0;   // count: entries incl. the padding of every segment to a multiple of 4
        i64* segptr = nullptr;          // [nblk][nseg + 1]
        unsigned short* idx = nullptr;  // offset inside the block
        void* val = nullptr;
        int* perm = nullptr;            // position in the canonical CSR
        SpWork* work = nullptr;
    } sp[2];
    // unweighted flavour with X kept as CSR (RRI_UNWEIGHTED_SPARSE; `sparse` is set too, `weighted` is not): the copies hold X
    // itself, read by k_spx_pass; spx_work = the items of copy 0 followed by those of copy 1 (SpWork.pad = copy)
    bool sparse_x = false;
    SpWork* spx_work = nullptr;
    double spb_ms = 0.0;        // HIP-event time of the kernels that built the blocked store on the device (rri_upload_X_corpus); 0: the host built it
    double* rowhat = nullptr;   // per-row sum of (W T)_ij^2 over the pattern (the objective's fallback)
    // uniform rows of that handle (rri_set_uniform_rows, rri_csr_scale_X_uniform): X = S + uni_value e_U 1^T, S the stored CSR
    // with zeros in the rows of U = uni_rows (sorted, device).  uni_n == 0: nothing of this is launched anywhere
    int* uni_rows = nullptr;
    i64 uni_n = 0;
    double uni_value = 0.0;
    double* uni_part = nullptr;   // [64][64] column sums of an operand panel by row chunks (k_spu_panel_part)
    // what the next rri_csr_scale_X is asked for besides scaling (consumed there, the one place that rewrites this X):
    enum { UNI_REQ_NONE = 0, UNI_REQ_COLLECT = 1, UNI_REQ_ZERO = 2 };
    int uni_req = UNI_REQ_NONE;
    const int* uni_req_rows = nullptr;   // UNI_REQ_ZERO: the rows that take zeros (device, the caller's), and how many
    i64 uni_req_n = 0;
    // what the next rri_upload_observed_csr takes in place of host arrays (consumed there, the one place that replaces this store):
    // the canonical arrays of a corpus on this device (rri_upload_observed_corpus, which has checked them and clears the request
    // on every return path)
    struct ObsReq {
        const i64* indptr;
        const int* indices;
        const double* values;
        i64 nnz;
    };
    const ObsReq* obs_req = nullptr;
    // dense weighted, one read-modify-write pass per topic step: the column sums a pass leaves for the next T row lack the
    // rank-one term of the W update that follows it; k_wmcorr takes that term from the mask alone (Cpart: its partials)
    double* Cpart = nullptr;
    double* N2part = nullptr;   // [cpart_rows x LD] nw = (w^2)^T M as row-block partials, where k_wmcorr_cols takes it (nw_from_mask)
    unsigned* Mcols = nullptr;  // the packed 0/1 mask once more with the rows in the bits (k_wmcorr_cols), built on first use
    bool nw_mask = false;       // this T-row step's nw was taken by k_wmcorr_cols (N2part), not by the pass (Z2part)
    bool mcols_tried = false;   // ... or found not worth it (dense mask, no memory)
    double mask_density = 1.0;
    int cpart_rows = 0;         // rows allocated in Cpart
    bool wcorr = false;         // the T-row step being enqueued subtracts T[wcorr_topic,:] .* sum_b Cpart[b]
    int wcorr_topic = 0, wcorr_nrb = 0;
    bool resid_fresh = false;   // weighted: E was rebuilt and no half step has run since
    bool dt_pending = false;    // weighted: dtv holds a T-row change that E does not contain yet
    // explicit-residual schedule of the unweighted flavour (RRI_UNWEIGHTED_RESIDUAL): R = X - W T lives in E and takes
    // the two rank-one terms of a topic step inside the pass of the next one
    bool explicit_resid = false;
    bool dw_pending = false;    // dwv holds a W-column change (of topic dw_topic) that R does not contain yet
    int dw_topic = 0;
    double* told = nullptr;     // T[t,:] before its last update (dt = T[t,:] - told while dt_pending)
    double *Gpart = nullptr, *tpart = nullptr, *rowobj = nullptr, *rowpos = nullptr, *normpart = nullptr;
    double *dtmp = nullptr;  // small double scratch (device): [0] sum, ...
    double* objbuf = nullptr;   // W^T W | T T^T | cross terms of the objective assembled after a sweep
    i64* itmp = nullptr;     // small i64 scratch (device)
    i64* tpart_idx = nullptr;
    double *resetT = nullptr, *resetW = nullptr;  // staging for 'random' reset vectors
    DevState* st = nullptr;

    int npanels = 1, rpb = 1, nrb = 1, nwb = 1, ntb = 1;
    int gpart_n = 1;   // rows of Gpart its last writer left (k_wcol: nwb, k_wcol_resid: nwb256, fused pass: nrb)
    int ttpart_n = 0;  // partial vectors T T[t]^T in Ttpart (k_tgram: nsplit)
    int xy_rows = 0;   // blocks per topic in XYpart (stride xy_stride)
    int xy_stride = 1;
    int ntb32 = 1;     // 32-column blocks of k_trow_small
    int tpart_n = 1;   // entries the last T-row step left in tpart (128- or 32-column blocks)

    rri_params prm{};
    bool have_params = false, have_X = false, have_W = false, have_T = false, have_M = false;


    bool carry_valid = false;
    int carry_topic = -1;
    // The early-sums schedule (RRI_EARLY_SUMS; early_ok): Tearly holds the partials of T T[t,:]^T of topic early_topic, left by
    // k_trow_early, while early_valid -- the one thing the early job in the pass of that topic's W half needs before the pass is
    // launched.  carry_wfin qualifies carry_valid: the carry was left by k_wfin (after step wfin_topic), so red is reduced
    // already, its Gram entries wfin_topic and k + 1 are per-tile partials in wfp, and only k_trow_early can take it up.
    // edot: the early job's row dots; Gearly: its Gram partials; ent: ||T[t,:]||^2; wfp: k_wfin's two vectors of tile partials.
    double *Tearly = nullptr, *edot = nullptr, *Gearly = nullptr, *ent = nullptr, *wfp = nullptr;
    bool early_valid = false, carry_wfin = false;
    int early_topic = -1, wfin_topic = -1;
    long early_steps = 0;      // W halves that took k_wfin (rri_layout_info)
    // <w_t, X t_t> of every topic's W half (per k_wcol block): with ||X||^2 and the two Gram matrices it gives the
    // objective without another pass over X.  xy_run = topics 0 .. xy_run-1 of the current sweep have run their
    // W half in order since the last change from outside; xy_valid: all k have, and no T row changed since.
    double* XYpart = nullptr;
    int xy_run = -1;
    bool xy_valid = false, x_sq_valid = false;
    // the persistent sweep left the objective of the sweep that has just ended (minus 1/2 ||X||^2) in DevState.obj_track: pending
    // while the launch is in flight, valid exactly as long as xy_valid is
    bool obj_track_pending = false, obj_track_valid = false;
    double obj_track_value = 0.0;
    // rri_sweep_until: sweeps with the objective history kept and the stop rule applied on the device (persistent sweep only)
    struct { bool active = false; double prev = 0.0, scale = 0.0; int n = 0; double* out = nullptr; } until;
    double *objhist = nullptr, *objdec = nullptr;
    double x_sq = 0.0;
    bool pending_wcheck = false;
    int pending_wcheck_topic = -1;

    // interrupted run
    bool paused = false;
    int run_total = 0;
    Cursor resume_at{0, 0, 0};
    bool resume_done = false;
    rri_event pending{RRI_EVENT_NONE, -1, 0, 0};

    bool resid_valid = false;  // masked residual E is in sync with (W,T) (weighted flavour)
    bool skip_row_finish = false;  // the resumed W half must not re-run the T-row checks (stale partial sums)
    int nwb256 = 1;

    // row-sharded run: this handle holds rows [row_offset, row_offset + n) of an n_global-row problem and every
    // cross-row sum of the schedule is all-reduced over `comm` on the handle's stream (rri_attach_comm)
    rri_comm* comm = nullptr;
    i64 row_offset = 0, n_global = 0;
    double* ctail = nullptr;   // 8 doubles (device): small collectives (column verdicts, objective parts)
    double* cand = nullptr;    // 2 * world doubles (device): candidates of the max-residual reset
    // rows that left the device, as frozen statistics (rri_frozen.hpp; rri_frozen_set / rri_frozen_absorb): B (k x LD, pad columns
    // zero), A (k x k), s (k) and two doubles for a column check taken alone, all four allocated together and NULL together.
    // They are inputs read at the point of use -- added into red after k_reduce, into fztail after k_colsum_tail -- and no cache:
    // nothing the handle keeps between calls was computed from them
    double *fzB = nullptr, *fzA = nullptr, *fzs = nullptr, *fztail = nullptr;
    double fz_c = 0.0;         // ||X_O||^2
    i64 fz_rows = 0;           // rows absorbed so far (rri_frozen_absorb counts them; rri_frozen_set starts from 0)
    rri_status comm_status = RRI_OK;   // first failure of a collective inside an enqueued sequence (or of a dispatch: f16_unreachable)

    // register-resident sweeps (rri_onchip_kernels.hpp): per-workgroup partial arrays and the grid barrier's counter
    int n_cu = 0;
    double *mkZ = nullptr, *mkG = nullptr, *mkP = nullptr, *mkX = nullptr, *mkT = nullptr, *objE = nullptr;
    unsigned* mkbar = nullptr;
    long onchip_launches = 0;
    // a persistent launch whose workgroups could not synchronise (HALT_ERR_GRID_SYNC: the device was shared, not every
    // workgroup resident in time) is undone and its range of steps run on the launch-per-phase schedule instead:
    // W, T as they were before the launch, the host flags the launch-per-phase schedule would have started from
    double *Wsafe = nullptr, *Tsafe = nullptr;
    bool onchip_in_flight = false;      // the sequence just enqueued was a persistent launch (run_and_collect reads it)
    bool onchip_off = false;            // after a fallback the handle stays on the launch-per-phase schedule ...
    long long onchip_off_until = 0;     // ... until this time (steady clock, ns): 2 s after the first fallback, doubling up to 64 s
    bool onchip_saved_skip = false;
    long onchip_fallbacks = 0;

    int timing = 0;            // 0 off, N > 0: time every N-th launch of each kernel id
    long timing_seq[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // kernel ids of rri_timing_read
    std::vector<TimedLaunch> timed[9];
    std::vector<hipEvent_t> event_pool;

    std::string err;
};
static inline bool ro_pass_interleaved(const rri_ctx* c) { return rri::ro_pass_interleaved(c->ro_il, c->npanels, c->nrb); }

// ---- what a handle keeps between steps and calls, and what each piece was computed from ------------------------------------
//                                              X   M   W   T   scratch  penalties
//   carry_valid / carry_topic                  x   x   x   x      x                 one topic's partial sums in Zpart / Gpart (Z2part)
//   resid_valid                               x   x   x   x                        E (pattern-only: sp_e and its copies) = [M .*] (X - W T)
//   xy_run / xy_valid                          x       x   x                        XYpart: <w_t, X t_t> of the topics of one sweep, in order
//   obj_track_valid                            x       x   x                x       DevState.obj_track of the last persistent launch
//   q_valid                                    x           x                        Qt = X T^T
//   gfull_valid                                            x                        Gfull = T T^T
//   x_sq_valid                                 x                                    x_sq = ||X||^2
// (X of an RRI_U8 handle: the counts AND its two scale vectors -- a changed scale is CH_X.)
// (X of an RRI_UNWEIGHTED_SPARSE handle: the stored CSR AND its uniform rows -- a changed list or value is CH_X; the list itself
// is no cache: only rri_set_uniform_rows, rri_csr_scale_X_uniform and a new X, rri_upload_X_csr, which empties it, write it.)
// (The early-sums schedule adds no row: carry_wfin qualifies carry_valid -- the carry is k_wfin's: red reduced already, two Gram
// entries as tile sums in wfp -- and goes wherever carry_valid goes; early_valid, the partials of T T[t,:]^T in Tearly, lives from
// the T half that leaves them to the W half of the same topic and is dropped by ANY change, that W half's own included.)
// (scratch: Zpart / Gpart / red, which other entry points borrow.)  resid_fresh, dt_pending and dw_pending qualify E and are
// read only while resid_valid holds; every rebuild resets them (resid_rebuilt).  pending_wcheck is no cache but a verdict still
// owed on the column sums in Gpart: it is taken before Gpart is overwritten (flush_wcheck) and dropped only with the run it
// belongs to (CH_ENDED).  A step that PRODUCES one of these sets it itself, next to its launch; what makes one stale is said
// here, by what changed, and nowhere else.  xp_valid / xp_done qualify the packed copy of X (xpack_ensure) and go exactly where
// x_sq_valid goes: the copy is of the X the handle held, the passes read the fp32 X again from that moment and the next sweep
// builds the copy anew.  keep_q is NOT recomputed at that moment (it is set where the copy is decided, xpack_ensure): single topic
// steps between a new X and the next sweep read the fp32 X with the kept row-block count of the 3.5-byte blocks, about 14 % more
// kept bytes than the budget of pass_keep -- a cache policy, no bit of any result -- until that sweep recomputes it.
// (tt_valid -- sp_Tt holds the transpose of the current T, for the one-launch fold sweep of a pattern-only handle -- was computed
// from T alone and goes wherever gfull_valid goes; the borrowers of sp_Tt that write another matrix into it drop it themselves.)
// Coarser than the table on purpose: any change from outside the schedule drops the first four rows together, and a new X drops
// Gfull as well.  A narrower rule would move where an fp32 residual is rebuilt, and with it the low bits of a run.
enum : unsigned {
    CH_X = 1u << 0,         // X replaced or rewritten in place
    CH_M = 1u << 1,         // the mask or the observed pattern replaced
    CH_W = 1u << 2,         // W written from outside the schedule
    CH_T = 1u << 3,         // T written from outside the schedule (the row of a reset included)
    CH_SCRATCH = 1u << 4,   // the scratch arrays were borrowed or rebound, or their sums belong to another form or communicator
    CH_PENALTY = 1u << 5,   // reg_w_* / reg_t_* changed
    CH_ENDED = 1u << 6,     // the run in progress is over (halt, failed collective, factors replaced, last check taken on the device):
                            // its sums are those of an unknown step and no column verdict is owed
    CH_T_ROW = 1u << 7,     // a step of the schedule rewrote one T row (xy_run stays: the W half of the same topic continues it)
    CH_W_COL = 1u << 8,     // ... one or all W columns (the step leaves its own carry, cross terms and column verdict)
    CH_E_FOLLOWS = 1u << 9  // with the two above: the step keeps E in step through dt_pending / dw_pending
};
static void changed(rri_ctx* c, unsigned what) {
    // the early partials of T T[t,:]^T live from the T half that leaves them to the W half of the same topic and no longer: that T
    // half sets the bit after its own CH_T_ROW, and every change -- the W half's own CH_W_COL included -- drops it
    if (what) c->early_valid = false;
    if (what & (CH_X | CH_M | CH_W | CH_T | CH_SCRATCH | CH_ENDED | CH_T_ROW)) c->carry_wfin = false;   // wherever carry_valid goes
    if (what & (CH_X | CH_M | CH_W | CH_T | CH_SCRATCH | CH_ENDED)) {
        c->carry_valid = false;
        c->carry_topic = -1;
        c->resid_valid = false;
        c->xy_run = -1;
        c->xy_valid = false;
        c->obj_track_valid = false;
    }
    if (what & CH_T_ROW) { c->carry_valid = false; c->xy_valid = false; }
    if ((what & (CH_T_ROW | CH_W_COL)) && !(what & CH_E_FOLLOWS)) c->resid_valid = false;
    if (what & (CH_T_ROW | CH_W_COL | CH_PENALTY)) c->obj_track_valid = false;
    if (what & (CH_X | CH_T | CH_T_ROW)) { c->q_valid = false; c->gfull_valid = false; c->tt_valid = false; }
    if (what & CH_X) { c->x_sq_valid = false; c->xp_valid = false; c->xn_valid = false; c->xp_done = false; }
    if (what & CH_ENDED) c->pending_wcheck = false;
}
// E has just been rebuilt from the current W and T: nothing is pending on it
static void resid_rebuilt(rri_ctx* c) {
    c->resid_valid = true;
    c->resid_fresh = true;
    c->dt_pending = false;
    c->dw_pending = false;
}


namespace {

rri_status fail(rri_ctx* c, rri_status code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), RRI_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

#define CHECK_CTX(c) \
    if (!(c)) return RRI_ERR_INVALID


// ---- who owns device memory ("Who owns device memory") ------------------------------------------------------------
// temporary device buffer that is released on every return path
struct DevTmp {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevTmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t b) { bytes = b; return hipMalloc(&p, b); }
};
// the two events of one measurement, destroyed on every return path
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t create() { const hipError_t e = hipEventCreate(&a); return e == hipSuccess ? hipEventCreate(&b) : e; }
};
// handle-owned allocations alive in the process (rri_device_memory)
std::atomic<long long> g_dev_buffers{0}, g_dev_bytes{0};
void dev_count(long long buffers, size_t bytes) { g_dev_buffers += buffers; g_dev_bytes += buffers * (long long)bytes; }
rri_ctx::Owned* dev_owned(rri_ctx* c, const void* field) {
    for (auto& o : c->owned)
        if (o.field == field) return &o;
    return nullptr;
}
// frees what the field holds if the handle allocated it; a bound (borrowed) pointer is only forgotten
template <typename P>
void dev_release(rri_ctx* c, P*& p) {
    if (rri_ctx::Owned* o = dev_owned(c, &p)) {
        (void)hipFree(o->p);
        dev_count(-1, o->bytes);
        c->owned.erase(c->owned.begin() + (o - c->owned.data()));
    }
    p = nullptr;
}
// a temporary becomes the handle's buffer p; what the field held before goes first, so a field never has two entries
template <typename P>
void dev_adopt(rri_ctx* c, P*& p, DevTmp& t) {
    dev_release(c, p);
    p = (P*)t.p;
    c->owned.push_back({&p, t.p, t.bytes});
    dev_count(1, t.bytes);
    t.p = nullptr;
}
// the one way a handle gets device memory; zero: cleared on the handle's stream.  A failure leaves p NULL and no sticky error
template <typename P>
hipError_t dev_alloc(rri_ctx* c, P*& p, size_t bytes, bool zero = false) {
    DevTmp t;
    hipError_t e = t.alloc(bytes);
    if (e == hipSuccess && zero) e = hipMemsetAsync(t.p, 0, bytes, c->stream);
    if (e == hipSuccess) dev_adopt(c, p, t);
    else { p = nullptr; (void)hipGetLastError(); }
    return e;
}
// ... and the one idiom of a buffer that is allocated on first use
template <typename P>
hipError_t dev_ensure(rri_ctx* c, P*& p, size_t bytes, bool zero = false) {
    return p ? hipSuccess : dev_alloc(c, p, bytes, zero);
}
// opts kernel K in to more than 64 KiB of dynamic LDS, once per instantiation and device (the attribute belongs to the device's
// code object)
template <auto K>
hipError_t allow_lds(const rri_ctx* c, int bytes) {
    static bool done[64] = {};
    bool& d = done[c->device & 63];
    if (d) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) d = true;
    else (void)hipGetLastError();
    return e;
}

// ---- collectives of a row-sharded handle: all on the handle's stream --------------------------------------------
// RCCL: enqueued like a kernel (no host synchronisation).  Host-callback transport: the stream is drained, the
// buffer goes through host memory and the caller's function (tests with several ranks on one GPU).
void comm_fail(rri_ctx* c, rri_status code, const char* what, const char* detail) {
    if (c->comm_status == RRI_OK) {
        c->comm_status = code;
        c->err = std::string("collective failed: ") + what + ": " + (detail ? detail : "?");
    }
}
// A rank that cannot go on BETWEEN two collectives its peers will still enter (a device error after the all-gather of a
// reset and before its broadcast) must not simply return: the peers would block inside RCCL with nothing to interrupt them.
// It aborts the communicator (ncclCommAbort: pending and later collectives of every rank end with an error) and reports.
// The host-callback transport has no such call; its collectives are host functions of the caller, who owns their time-outs.
rri_status comm_abort(rri_ctx* c, const char* what, hipError_t e) {
    rri_comm* m = c->comm;
    if (m && m->nccl && !m->aborted && rccl_api().CommAbort) {
        (void)rccl_api().CommAbort(m->nccl);
        m->nccl = nullptr;
    }
    if (m) m->aborted = true;
    c->comm_status = RRI_OK;
    return fail(c, RRI_ERR_COMM, "%s failed between two collectives (%s): the communicator was aborted so that the other ranks do not wait", what, hipGetErrorString(e));
}
void comm_allreduce(rri_ctx* c, double* dev, i64 count) {
    rri_comm* m = c->comm;
    if (m && m->aborted) { comm_fail(c, RRI_ERR_COMM, "all-reduce", "the communicator was aborted"); return; }
    if (!m || c->comm_status != RRI_OK) return;
    m->n_allreduce += 1;
    if (m->nccl) {
        ncclResult_t r = rccl_api().AllReduce(dev, dev, (size_t)count, ncclDouble, ncclSum, m->nccl, c->stream);
        if (r != ncclSuccess) comm_fail(c, RRI_ERR_COMM, "ncclAllReduce", rccl_api().GetErrorString(r));
        return;
    }
    m->hbuf.resize((size_t)count);
    hipError_t e = hipMemcpyAsync(m->hbuf.data(), dev, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e)); return; }
    if (m->h_allreduce(m->user, m->hbuf.data(), count) != 0) { comm_fail(c, RRI_ERR_COMM, "all-reduce callback", "non-zero return"); return; }
    e = hipMemcpyAsync(dev, m->hbuf.data(), (size_t)count * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // hbuf is reused by the next collective
    if (e != hipSuccess) comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e));
}
void comm_allgather(rri_ctx* c, const double* dev_send, i64 count, double* dev_recv) {
    rri_comm* m = c->comm;
    if (m && m->aborted) { comm_fail(c, RRI_ERR_COMM, "all-gather", "the communicator was aborted"); return; }
    if (!m || c->comm_status != RRI_OK) return;
    if (m->nccl) {
        ncclResult_t r = rccl_api().AllGather(dev_send, dev_recv, (size_t)count, ncclDouble, m->nccl, c->stream);
        if (r != ncclSuccess) comm_fail(c, RRI_ERR_COMM, "ncclAllGather", rccl_api().GetErrorString(r));
        return;
    }
    m->hbuf.resize((size_t)count);
    m->hbuf2.resize((size_t)count * m->world);
    hipError_t e = hipMemcpyAsync(m->hbuf.data(), dev_send, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e)); return; }
    if (m->h_allgather(m->user, m->hbuf.data(), count, m->hbuf2.data()) != 0) { comm_fail(c, RRI_ERR_COMM, "all-gather callback", "non-zero return"); return; }
    e = hipMemcpyAsync(dev_recv, m->hbuf2.data(), (size_t)count * m->world * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e));
}
void comm_broadcast(rri_ctx* c, double* dev, i64 count, int root) {
    rri_comm* m = c->comm;
    if (m && m->aborted) { comm_fail(c, RRI_ERR_COMM, "broadcast", "the communicator was aborted"); return; }
    if (!m || c->comm_status != RRI_OK) return;
    if (m->nccl) {
        ncclResult_t r = rccl_api().Broadcast(dev, dev, (size_t)count, ncclDouble, root, m->nccl, c->stream);
        if (r != ncclSuccess) comm_fail(c, RRI_ERR_COMM, "ncclBroadcast", rccl_api().GetErrorString(r));
        return;
    }
    m->hbuf.resize((size_t)count);
    hipError_t e = hipMemcpyAsync(m->hbuf.data(), dev, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e)); return; }
    if (m->h_broadcast(m->user, m->hbuf.data(), count, root) != 0) { comm_fail(c, RRI_ERR_COMM, "broadcast callback", "non-zero return"); return; }
    e = hipMemcpyAsync(dev, m->hbuf.data(), (size_t)count * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) comm_fail(c, RRI_ERR_HIP, "staging", hipGetErrorString(e));
}
// `count` host doubles summed over the ranks in place (objective parts, decisions of the host driver)
rri_status comm_allreduce_host(rri_ctx* c, double* host, i64 count) {
    if (!c->comm) return RRI_OK;
    if (count > 8) return fail(c, RRI_ERR_INVALID, "host all-reduce takes at most 8 values");
    HIPCHK(c, hipMemcpyAsync(c->ctail, host, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
    comm_allreduce(c, c->ctail, count);
    HIPCHK(c, hipMemcpyAsync(host, c->ctail, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_status != RRI_OK) { rri_status r = c->comm_status; c->comm_status = RRI_OK; return r; }
    return RRI_OK;
}

KParams kparams(const rri_ctx* c) {
    KParams p{};
    const rri_params& q = c->prm;
    p.fix_W = q.fix_W; p.fix_T = q.fix_T; p.project_T = q.project_T_each_iter;
    p.has_trs = q.has_t_row_sum; p.has_wrs = q.has_w_row_sum;
    p.reset_method = q.reset_method; p.resets_left = q.resets_left;
    p.t_row_sum = q.t_row_sum; p.w_row_sum = q.w_row_sum;
    p.reg_w_l1 = q.reg_w_l1; p.reg_w_l2 = q.reg_w_l2; p.reg_t_l1 = q.reg_t_l1; p.reg_t_l2 = q.reg_t_l2;
    p.eps = q.eps_div;
    return p;
}

// Does this handle step through its explicit residual?  Only with both halves free: with T (or W) fixed one half of every
// step is missing, and the Gram form is then the cheaper schedule by far (T fixed: X T^T once, no pass over the matrix per
// topic at all; W fixed: one read pass per topic instead of a read-modify-write), so a handle of the explicit-residual
// schedule takes it for such calls -- fold-in (sklearn_interface.py:327-333, nmf.py:417,460) works on either kind of handle.
// The stored residual is stale afterwards and rebuilt when next needed.
bool resid_sched(const rri_ctx* c) { return c->explicit_resid && !c->prm.fix_T && !c->prm.fix_W && c->k >= 2; }

bool no_regs(const rri_ctx* c) {
    const rri_params& q = c->prm;
    return std::abs(q.reg_w_l1) + std::abs(q.reg_w_l2) + std::abs(q.reg_t_l1) + std::abs(q.reg_t_l2) == 0.0;
}

// ---- timing ------------------------------------------------------------------------------
hipEvent_t get_event(rri_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
struct TimedScope {
    rri_ctx* c;
    int id;
    TimedLaunch tl{nullptr, nullptr};
    bool on;
    TimedScope(rri_ctx* c_, int id_)
        : c(c_), id(id_),
          on(c_->timing > 0 && (c_->timing_seq[id_]++ % c_->timing) == 0 && c_->timed[id_].size() < 400000) {
        if (on) {
            tl.a = get_event(c);
            tl.b = get_event(c);
            (void)hipEventRecord(tl.a, c->stream);
        }
    }
    ~TimedScope() {
        if (on) {
            (void)hipEventRecord(tl.b, c->stream);
            c->timed[id].push_back(tl);
        }
    }
};

// element sizes of the storage types (0: not a storage type)
// the loads the kernels are written for are the loads the plan counts columns in
static_assert(load_elems(RRI_F32) == XVec<float>::N, "fp32: elements per load");
static_assert(load_elems(RRI_F64) == XVec<double>::N, "float64: elements per load");
static_assert(load_elems(RRI_F16) == XVec<_Float16>::N, "float16: elements per load");
static_assert(load_elems(RRI_U8) == XVec<unsigned char>::N, "uint8: elements per load");
// the two stores of a dense X that is only ever read (RRI_UNWEIGHTED, Gram form): float16, and uint8 counts with scales
bool ro_store(int dt) { return dt == RRI_F16 || dt == RRI_U8; }
const char* dtype_name(int dt) { return dt == RRI_F32 ? "RRI_F32" : dt == RRI_F64 ? "RRI_F64" : dt == RRI_F16 ? "RRI_F16" : dt == RRI_U8 ? "RRI_U8" : "?"; }

// a read-only store (float16, uint8) reached a kernel family that does not exist for it: reported like a failed step of an enqueued sequence
void f16_unreachable(rri_ctx* c) {
    if (c->comm_status == RRI_OK) {
        c->comm_status = RRI_ERR_UNSUPPORTED;
        c->err = "this operation rewrites X or needs a mask, a residual or a CSR store: not available on an RRI_F16 or RRI_U8 handle";
    }
}

// ---- typed launch helpers ------------------------------------------------------------------
// kernels that touch X / mask / residual depend on the storage type SX; the rest is float64
template <typename SX>
struct LaunchX {
    typedef SX Elem;
    // float16 storage is read-only (RRI_F16: dense X, Gram form): only the members DISPATCH_RO reaches are ever instantiated for
    // it, and inside those the branches to the CSR, masked and residual-writing kernels are compiled out
    // uint8 storage (RRI_U8) is the same handle with counts and two scale vectors (xscale)
    static constexpr bool RO = std::is_same<SX, _Float16>::value || std::is_same<SX, unsigned char>::value;
    static XScale xscale(const rri_ctx* c) { return XScale{c->rscale, c->cscale}; }
    // row-dot slots of the 4 waves, the active W column, (UPD: one or two arrays of rank-one row factors,) the row-sum tiles
    static size_t pass_shmem(const rri_ctx* c, int upd) {
        return ((5 + upd) * (size_t)c->rpb + 4 * 8 * 72) * sizeof(double);
    }
    // the rank-one terms a pass folds into the residual before it takes its products (UPD = 1: a, b; UPD = 2: also a2 and
    // b2 - b2sub)
    struct Upd {
        const double *a = nullptr, *b = nullptr, *a2 = nullptr, *b2 = nullptr, *b2sub = nullptr;
    };
    // Non-temporal loads keep a streamed matrix from washing W, T and the partial sums out of the caches -- where it cannot
    // stay there anyway.  A matrix that fits the 256 MB Infinity Cache is re-read from it by every pass: plain loads are
    // 4 % faster at 10000 x 1000 (2020 against 1937 sweeps/s, profiles/r02_c2_variants.log).
    // The passes over a stored residual and the one pass of the preprocessing: all or nothing (their stores leave L2 on every
    // pass; the read-only pass of the sweeps keeps a part of X instead, pass_keep).  The `keep` of pass_cfg: -1 plain, 0 streamed.
    static int stream_whole(const rri_ctx* c) {
        return (double)c->n * (double)c->LD * (double)c->es > 192.0e6 ? 0 : -1;
    }
    template <bool DO_Y, bool DO_Z, int UPD, int U, bool NT, bool RS, int PK, bool EJ>
    static void pass_k(rri_ctx* c, void* Xp, i64 ldp, const double* trow, const double* wc, const Upd& u, const TgramJob& job,
                       int keep, const EarlyJob& ej) {
        const int ncols = (int)std::min<i64>(ldp, c->LD);
        typedef typename std::conditional<(UPD > 0), SX, const SX>::type XT;
        hipLaunchKernelGGL((k_pass<SX, DO_Y, DO_Z, UPD, U, NT, RS, PK, EJ>), dim3(c->npanels * c->nrb + job.nblocks + (EJ ? ej.nblocks : 0)), dim3(256),
                           pass_shmem(c, UPD), c->stream, (XT*)Xp, ldp, (int)c->n, ncols, trow, wc, c->Ypart,
                           c->Zpart, c->LD, c->rpb, c->npanels, u.a, u.b, u.a2, u.b2, u.b2sub, (const DevState*)c->st, job,
                           // interleaved row chunks: the workgroups running at one time walk ONE window of the matrix, as a
                           // linear stream does.  Read-only pass: +2 % up to 1024 workgroups (20000 x 5000), -1 % at C3, where
                           // it stays off.  Read-modify-write (UPD): +4-9 % at C3 (profiles/r02_residual_schedule_geometry.log)
                           // -- reads and writes of a window stay in the DRAM pages that are open
                           ((ro_pass_interleaved(c) || UPD > 0) ? c->nrb : 0) |
                               ((c->sw.pass_rot >= 0 ? c->sw.pass_rot : (UPD > 0 ? c->rot_r : c->rot_x)) << 27),
                           keep, PK == 2 ? (const unsigned char*)c->xn : PK ? (const unsigned char*)c->xp : nullptr, PK ? (const unsigned char*)c->xp_flags : nullptr,
                           PK ? c->xp_base : 0, (const double*)c->rscale, (const double*)c->cscale,
                           PK == 2 ? (const unsigned*)c->xn_dir : nullptr, PK == 2 ? (const unsigned short*)c->xn_exc : nullptr,
                           PK == 2 ? c->xn_books : xnarrow::Books{}, ej);
    }
    // The read-only pass: 8 rows in flight per wave, the row dots (DO_Y) through LDS row sums.  The read-modify-write variants:
    // 16 rows in flight per wave, row dots by DPP wave sums -- 0.665 against 0.639 of 8 TB/s for the 8-row LDS row-sum variant
    // at C3 (profiles/r02_residual_schedule_geometry.log).  (The LDS-DMA ring k_pass_dma measured between +3 % and -9 % against
    // this pass, profiles/r04_pass_dma_ab.log, and was removed.)
    // keep: -1 = default-policy loads (and stores) throughout; >= 0: non-temporal, but for `keep` row blocks of a read-only pass
    // PK: the read-only pass of an fp32 handle over the packed copy of X (1: c->xp, 2: the 26-bit c->xn; flagged tiles from Xp itself)
    template <bool DO_Y, bool DO_Z, int UPD, int PK = 0>
    static void pass_cfg(rri_ctx* c, void* Xp, i64 ldp, const double* trow, const double* wc, int keep, const Upd& u = Upd{},
                         const TgramJob& job = TgramJob{}, const EarlyJob& ej = EarlyJob{}) {
        constexpr int U = UPD > 0 ? 16 : 8;
        constexpr bool RS = UPD == 0 && DO_Y;
        // the build with the early-sums job only where a job rides (the fused read-only pass of an early W half)
        constexpr bool CAN_EJ = DO_Y && DO_Z && UPD == 0;
        pick_bool(keep >= 0, [&](auto nt) {
            pick_bool(CAN_EJ && ej.nblocks > 0, [&](auto with_job) {
                if constexpr (CAN_EJ || !with_job) pass_k<DO_Y, DO_Z, UPD, U, nt, RS, PK, with_job>(c, Xp, ldp, trow, wc, u, job, nt ? keep : 0, ej);
            });
        });
    }
    // row dots against T[t,:] (DO_Y) and column sums against W[:,tz] (DO_Z); `job`: the Gram row of T[t,:] rides along; `ej`: and
    // the W-sized sums of the step (the early-sums schedule; the fused pass of a dense X only)
    template <bool DO_Y, bool DO_Z>
    static void pass(rri_ctx* c, int t, int tz, const TgramJob& job = TgramJob{}, const EarlyJob& ej = EarlyJob{}) {
        TimedScope ts(c, 0);
        if constexpr (!RO) {
            if (c->sparse_x) {    // X on CSR: the read-only pass over its two blocked copies (no side job: the caller runs k_tgram)
                spx_pass<DO_Y, DO_Z>(c, c->T + (i64)t * c->LD, c->W + (i64)tz * c->ldw);
                return;
            }
        }
        // the packed copy of X exists for an fp32 handle only: no PK pass is built for another storage type
        constexpr bool F32 = std::is_same<SX, float>::value;
        pick_int<2, 1, 0>(F32 && c->xp_valid ? (c->xn_valid ? 2 : 1) : 0, [&](auto PK) {
            if constexpr (F32 || !PK) pass_cfg<DO_Y, DO_Z, 0, PK>(c, c->X, c->ldx, c->T + (i64)t * c->LD, c->W + (i64)tz * c->ldw, c->keep_q, Upd{}, job, ej);
        });
    }
    // explicit-residual schedule: the same products over the stored residual R (c->E, stride LD)
    static void rpass_colsums(rri_ctx* c, int tz) {
        TimedScope ts(c, 0);
        pass_cfg<false, true, 0>(c, c->E, c->LD, nullptr, c->W + (i64)tz * c->ldw, stream_whole(c));
    }
    // R <- R - a b^T [- a2 (b2 - b2sub)^T] fused with the row dots (against trow) and column sums (against wc) of
    // the new R: the rank-one residual update north_star names
    static void rank_update(rri_ctx* c, void* R, i64 ldr, const Upd& u, const double* trow, const double* wc,
                            const TgramJob& job = TgramJob{}) {
        TimedScope ts(c, 3);
        pick_int<2, 1>(u.a2 ? 2 : 1, [&](auto upd) { pass_cfg<true, true, upd>(c, R, ldr, trow, wc, stream_whole(c), u, job); });
    }
    template <bool DO_Y, bool DO_Z, bool UPD2, bool WRITE, bool MBITS, int U, bool RS, bool DO_Z2>
    static void wpass_k(rri_ctx* c, const double* trow, const double* wc, const double* a1, const double* b1,
                        const double* a2, const double* b2) {
        const int ncols = (int)std::min<i64>(c->ldx, c->LD);
        const int rot = (c->sw.pass_rot >= 0 ? c->sw.pass_rot : c->rot_r) << 27;
        auto launch = [&](auto kernel, int grid_flags) {
            hipLaunchKernelGGL(kernel, dim3(c->npanels * c->nrb), dim3(256), (11 * (size_t)c->rpb + 4 * 8 * 72) * sizeof(double),
                               c->stream, (SX*)c->E, (const SX*)c->M, c->LD, c->ldm, (const unsigned*)c->Mbits, c->ldb, (int)c->n,
                               ncols, trow, wc, a1, b1, a2, b2, c->Ypart, c->Y2part, c->Zpart, c->Z2part, c->LD, c->rpb, c->npanels,
                               (const DevState*)c->st, grid_flags);
        };
        if constexpr (DO_Y && WRITE && U == 4 && (DO_Z2 || !DO_Z)) {
            // the one-pass step, 4 rows in flight: the build for four waves per SIMD (the compiler's own register count, 130,
            // gives 3); the step whose nw comes from the mask (DO_Z && !DO_Z2) takes k_wpass below
            launch(k_wpass_occ4<SX, DO_Y, DO_Z, UPD2, WRITE, U, true, MBITS, RS, DO_Z2>, c->nrb | rot);
        } else {
            // interleaved row chunks for the passes that write E back (read-modify-write), as for k_pass<UPD>
            launch(k_wpass<SX, DO_Y, DO_Z, UPD2, WRITE, U, true, MBITS, RS, DO_Z2>,
                   ((WRITE || ro_pass_interleaved(c)) ? c->nrb : 0) | rot);
        }
    }
    // Rows in flight.  The one-pass step (row products and a write): 4, DPP row sums -- 1.458 ms at BASELINE config 5 against
    // 1.553 ms for 8 with LDS row sums (240 VGPRs, 2 waves per SIMD) and 1.618 ms for 8 with DPP row sums, engines made
    // alternately in one process (profiles/r04_wpass_one_variants.log).  The other passes that take row products: 8, LDS row
    // sums.  Column sums alone: 8 with a bit-packed mask (one mask word per chunk; +1.3 % at C5 over 4, 16 falls to one wave
    // per SIMD: profiles/r02_weighted_pass_variants.log), 4 with an fp mask array.
    template <bool DO_Y, bool DO_Z, bool UPD2, bool WRITE>
    static void wpass(rri_ctx* c, const double* trow, const double* wc, const double* a1, const double* b1,
                      const double* a2, const double* b2) {
        TimedScope ts(c, 3);
        if (c->sparse) { sp_wpass<DO_Y, DO_Z, UPD2, WRITE>(c, trow, wc, a1, b1, a2, b2); return; }
        pick_bool(c->Mbits != nullptr, [&](auto mbits) {
            constexpr bool MBITS = mbits;
            constexpr bool ONE = DO_Y && WRITE;
            constexpr int U = ONE ? 4 : (MBITS || DO_Y) ? 8 : 4;
            constexpr bool RS = !ONE && DO_Y;
            // the second column sum rides with the first, but for a sparse 0/1 mask: there nw comes from k_wmcorr_cols and the
            // pass leaves Z2part alone
            bool z2 = DO_Z;
            if constexpr (DO_Z && MBITS) z2 = !nw_from_mask(c);
            pick_bool(z2, [&](auto do_z2) {
                // DO_Z2 differs from DO_Z in that one case only: nothing else is ever launched, so nothing else is built
                if constexpr (do_z2 == DO_Z || (DO_Z && MBITS)) wpass_k<DO_Y, DO_Z, UPD2, WRITE, MBITS, U, RS, do_z2>(c, trow, wc, a1, b1, a2, b2);
            });
        });
    }
    // c = M^T (wn .* dw) as row-block partials in Cpart (k_wmcorr): the correction of the column sums a one-pass topic step
    // leaves behind.  Geometry: wmcorr_grid / wmcorr_cols_grid (rri_layout.hpp).
    // the column-major copy of the packed mask, on first use (one-off: a kernel, a count, one synchronisation)
    static bool mask_cols(rri_ctx* c) {
        if (!c->Mbits || !c->sw.wmcorr_cols) return false;
        if (!c->mcols_tried) {
            c->mcols_tried = true;
            const i64 ng = (c->n + 31) / 32;
            DevTmp cnt;
            if (dev_alloc(c, c->Mcols, (size_t)ng * c->LD * sizeof(unsigned)) != hipSuccess) return false;
            if (cnt.alloc(sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); dev_release(c, c->Mcols); return false; }
            (void)hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), c->stream);
            hipLaunchKernelGGL(k_mask_cols_from_bits, dim3(4096), dim3(256), 0, c->stream, (const unsigned*)c->Mbits, c->ldb, c->n, c->Mcols,
                               c->LD, (unsigned long long*)cnt.p);
            unsigned long long h = 0;
            hipError_t e = hipMemcpyAsync(&h, cnt.p, sizeof h, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { dev_release(c, c->Mcols); return false; }
            c->mask_density = (double)h / ((double)c->n * (double)c->d);
            if (c->mask_density > 0.12) dev_release(c, c->Mcols);     // the dense-bit kernel is the cheaper one there
        }
        return c->Mcols != nullptr;
    }
    // the second column sum of a T-row step, nw = (w^2)^T M, from the mask-only kernel instead of the pass: dense handles on the
    // one-pass schedule whose mask is 0/1 and sparse enough for the column-major copy
    static bool nw_from_mask(rri_ctx* c) { return !c->sparse && c->sw.wnw_mask && mask_cols(c); }
    // dw == NULL: nothing pending, nw alone (nw_from_mask handles)
    static void wmcorr(rri_ctx* c, const double* wn, const double* dw) {
        TimedScope ts(c, 2);
        if (mask_cols(c)) {     // a sparse 0/1 mask: the set bits only
            const bool nw = nw_from_mask(c);
            const WmcorrGrid g = wmcorr_cols_grid(c->n, c->LD, c->n_cu);
            const int npg = g.npg;
            const i64 rpb = g.rpb;
            c->wcorr_nrb = g.wcorr_nrb;
            const dim3 grid((unsigned)(npg * g.nrb));
            const size_t sh = (size_t)rpb * sizeof(double) * ((dw && nw) ? 2 : 1);
            pick_bool(dw != nullptr, [&](auto has_dw) {
                pick_bool(nw, [&](auto has_nw) {
                    // nothing pending and no nw wanted: nothing is launched, and no such kernel is built
                    if constexpr (has_dw || has_nw)
                        hipLaunchKernelGGL((k_wmcorr_cols<has_dw, has_nw>), grid, dim3(256), sh, c->stream, (const unsigned*)c->Mcols, c->LD,
                                           (int)c->n, (int)c->LD, wn, dw, c->Cpart, c->N2part, c->LD, (int)rpb, npg, (const DevState*)c->st);
                });
            });
            return;
        }
        if (!dw) return;
        const bool bits = c->Mbits != nullptr;
        const WmcorrGrid g = wmcorr_grid(c->n, bits, c->ldb, c->npanels, c->n_cu, c->cpart_rows);
        const int npg = g.npg;
        const i64 nrb = g.nrb, rpb = g.rpb;
        c->wcorr_nrb = g.wcorr_nrb;
        const int ncols = (int)std::min<i64>(bits ? c->ldb * 4 : c->ldm, c->LD);
        if (bits)      // (a packed mask: rows whose factor is zero are skipped)
            hipLaunchKernelGGL((k_wmcorr<SX, true, true>), dim3((unsigned)(npg * nrb)), dim3(256), (size_t)rpb * sizeof(double), c->stream,
                               (const SX*)nullptr, (i64)0, (const unsigned*)c->Mbits, c->ldb, (int)c->n, (int)(c->ldb * 4), wn, dw,
                               c->Cpart, c->LD, (int)rpb, npg, (const DevState*)c->st);
        else
            hipLaunchKernelGGL((k_wmcorr<SX, false, false>), dim3((unsigned)(npg * nrb)), dim3(256), (size_t)rpb * sizeof(double), c->stream,
                               (const SX*)c->M, c->ldm, (const unsigned*)nullptr, (i64)0, (int)c->n, ncols, wn, dw, c->Cpart,
                               c->LD, (int)rpb, npg, (const DevState*)c->st);
    }
    // ---- sparse pattern (rri_sparse_kernels.hpp) ----------------------------------------------------
    template <bool DO_S, bool UPD2, bool WRITE, int LPS>
    static void sp_blk_k(rri_ctx* c, const rri_ctx::SpCopy& cp, const double* B1, const double* B2, const double* V,
                         const double* A1, const double* A2, double* S1, double* S2, i64 lds) {
        const size_t sh = sp_lds_bytes<SX>(cp.bw);
        (void)allow_lds<k_sp_blk<SX, DO_S, UPD2, WRITE, LPS>>(c, SP_BLOCK_BYTES + 64);
        if (cp.nwork < 1) return;
        hipLaunchKernelGGL((k_sp_blk<SX, DO_S, UPD2, WRITE, LPS>), dim3(cp.nwork), dim3(1024), sh, c->stream,
                           (const SpWork*)cp.work, (const i64*)cp.segptr, cp.nseg, (const unsigned short*)cp.idx,
                           (SX*)cp.val, cp.bw, cp.gdim, B1, B2, V, A1, A2, S1, S2, lds, (const DevState*)c->st);
    }
    template <bool DO_S, bool UPD2, bool WRITE>
    static void sp_blk(rri_ctx* c, int which, const double* B1, const double* B2, const double* V, const double* A1,
                       const double* A2, double* S1, double* S2, i64 lds) {
        const rri_ctx::SpCopy& cp = c->sp[which];
        pick_int<8, 16, 32, 64>(cp.lps, [&](auto lps) { sp_blk_k<DO_S, UPD2, WRITE, lps>(c, cp, B1, B2, V, A1, A2, S1, S2, lds); });
    }
    // the same operation as wpass on the two copies of the pattern residual: row products from the row copy
    // (one Ypart "panel" per column block), column sums from the column copy (one Zpart row per row block)
    template <bool DO_Y, bool DO_Z, bool UPD2, bool WRITE>
    static void sp_wpass(rri_ctx* c, const double* trow, const double* wc, const double* a1, const double* b1,
                         const double* a2, const double* b2) {
        if (DO_Y || WRITE)   // segments = rows (factors a1, a2), gathered = columns (b1, b2, trow)
            sp_blk<DO_Y, UPD2, WRITE>(c, 0, b1, b2, trow, a1, a2, c->Ypart, c->Y2part, c->n);
        if (DO_Z || WRITE)   // segments = columns (b1, b2), gathered = rows (a1, a2, wc)
            sp_blk<DO_Z, UPD2, WRITE>(c, 1, a1, a2, wc, b1, b2, c->Zpart, c->Z2part, c->LD);
    }
    // out (nseg x m, row-major, device) = the X on the pattern (which = 0) or its transpose (1) times B (gdim x m)
    // RRI_UNWEIGHTED_SPARSE: row dots against trow (DO_Y, the row copy, into Ypart) and column sums against wc (DO_Z, the
    // column copy, into Zpart) in ONE launch over the items of both copies (k_spx_pass)
    template <bool DO_Y, bool DO_Z>
    static void spx_pass(rri_ctx* c, const double* trow, const double* wc) {
        SpxArgs<SX> a{};
        a.work = c->spx_work;
        a.first = DO_Y ? 0 : c->sp[0].nwork;
        for (int w = 0; w < 2; ++w) {
            const rri_ctx::SpCopy& cp = c->sp[w];
            a.segptr[w] = cp.segptr; a.idx[w] = cp.idx; a.val[w] = (const SX*)cp.val;
            a.nseg[w] = cp.nseg; a.gdim[w] = cp.gdim; a.bw[w] = cp.bw; a.lps[w] = cp.lps;
        }
        a.F[0] = trow; a.S[0] = c->Ypart; a.lds[0] = c->n;
        a.F[1] = wc; a.S[1] = c->Zpart; a.lds[1] = c->LD;
        const int items = (DO_Y ? c->sp[0].nwork : 0) + (DO_Z ? c->sp[1].nwork : 0);
        // (upload_X_csr_kept refuses a copy without a work item: every pass writes its partials, to which the uniform rows' share
        // below is added)
        if (items < 1) return;
        const int bwmax = std::max(DO_Y ? c->sp[0].bw : 0, DO_Z ? c->sp[1].bw : 0);
        hipLaunchKernelGGL((k_spx_pass<SX>), dim3(items), dim3(1024), spx_lds_bytes(bwmax), c->stream, a,
                           (const DevState*)c->st);
        if (c->uni_n > 0) {   // the uniform rows' share, into block 0 of the partials the pass has just written
            TimedScope tu(c, 3);   // (timing id 3 has no other user on this handle; id 0's bracket, in pass(), holds both launches)
            const int nzb = DO_Z ? (int)((c->d + 1023) / 1024) : 0;
            hipLaunchKernelGGL((k_spu_pass<DO_Y, DO_Z>), dim3(nzb + (DO_Y ? 1 : 0)), dim3(1024), 0, c->stream,
                               (const int*)c->uni_rows, (int)c->uni_n, c->uni_value, trow, c->d, wc, c->Ypart, c->Zpart, nzb,
                               (const DevState*)c->st);
        }
    }
    // k_spx_rowtot (totals) or k_spx_scale on the canonical CSR, a group of spx_scale_lps lanes per row
    static void spx_scale(rri_ctx* c, const double* sdev, double* tot, unsigned long long* nzero, bool totals, bool uni = false) {
        pick_int<64, 8>(spx_scale_lps(c->nnz, c->n), [&](auto LPS) {
            const unsigned nb = (unsigned)((c->n + 256 / LPS - 1) / (256 / LPS));
            if (totals)
                hipLaunchKernelGGL((k_spx_rowtot<SX, LPS>), dim3(nb), dim3(256), 0, c->stream, (const i64*)c->sp_rowptr,
                                   (const int*)c->sp_col, (const SX*)c->sp_x, c->n, sdev, tot, nzero);
            else if (uni)     // rows with a total below 1e-10 take zeros (rri_csr_scale_X_uniform)
                hipLaunchKernelGGL((k_spx_scale<SX, LPS, true>), dim3(nb), dim3(256), 0, c->stream, (const i64*)c->sp_rowptr,
                                   (const int*)c->sp_col, (SX*)c->sp_x, c->n, sdev, (const double*)tot);
            else
                hipLaunchKernelGGL((k_spx_scale<SX, LPS>), dim3(nb), dim3(256), 0, c->stream, (const i64*)c->sp_rowptr,
                                   (const int*)c->sp_col, (SX*)c->sp_x, c->n, sdev, (const double*)tot);
        });
    }
    static void spx_xtt(rri_ctx* c, const double* Tm, int m, double* out) {   // out (m x n) = (X Tm^T)^T on the CSR
        const i64 total = (i64)m * c->d;
        c->tt_valid = false;      // sp_Tt is borrowed for the transpose of Tm
        hipLaunchKernelGGL((k_convert2d<double, double, true>), dim3((unsigned)std::min<i64>(4096, (total + 255) / 256)),
                           dim3(256), 0, c->stream, Tm, c->LD, c->sp_Tt, (i64)c->kp, (i64)m, c->d);
        hipLaunchKernelGGL((k_spx_xtt<SX>), dim3((unsigned)((c->n + 3) / 4)), dim3(256), 0, c->stream,
                           (const i64*)c->sp_rowptr, (const int*)c->sp_col, (const SX*)c->sp_x, c->n,
                           (const double*)c->sp_Tt, m, c->kp, out, c->ldw);
        if (c->sparse_x && c->uni_n > 0)
            hipLaunchKernelGGL(k_spu_xtt, dim3(m), dim3(256), 0, c->stream, (const int*)c->uni_rows, (int)c->uni_n, c->uni_value,
                               Tm, c->LD, c->d, out, c->ldw);
    }
    static void sp_spmm(rri_ctx* c, int which, const double* B, int m, double* part, double* out) {
        const rri_ctx::SpCopy& cp = c->sp[which];
        const i64 waves = (i64)cp.nblk * cp.nseg;
        hipLaunchKernelGGL((k_sp_spmm<SX>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream,
                           (const i64*)cp.segptr, cp.nseg, cp.nblk, (const unsigned short*)cp.idx, (const int*)cp.perm,
                           (const SX*)c->sp_x, cp.bw, B, m, part);
        const i64 count = cp.nseg * m;
        hipLaunchKernelGGL(k_sp_sum_blocks, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)part, count, cp.nblk, out);
        spu_spmm(c, which, B, m, out);
    }
    // the uniform rows' share of a product: X B gets c (1^T B) in the rows of U, X^T Q gets c (e_U^T Q) in every row j < d
    static void spu_spmm(rri_ctx* c, int which, const double* B, int m, double* out) {
        if (!c->sparse_x || c->uni_n < 1) return;
        const int* U = c->uni_rows;
        const int nu = (int)c->uni_n;
        if (which == 0) {
            const i64 chunk = std::max<i64>(1024, (c->d + 63) / 64);
            const int nb = (int)((c->d + chunk - 1) / chunk);      // <= 64 rows of uni_part
            hipLaunchKernelGGL(k_spu_panel_part, dim3(nb), dim3(1024), 0, c->stream, B, c->d, m, chunk, c->uni_part);
            hipLaunchKernelGGL(k_spu_panel_rows, dim3((unsigned)((nu + 3) / 4)), dim3(256), 0, c->stream, U, nu, c->uni_value,
                               (const double*)c->uni_part, nb, m, out);
        } else {
            hipLaunchKernelGGL(k_spu_panel_all, dim3((unsigned)((c->d + 255) / 256)), dim3(1024), 0, c->stream, U, nu, c->uni_value,
                               B, m, c->d, out);
        }
    }
    // the same product between two device panels of the range finder (rri_sparse_range_finder): with one block the sum over the
    // blocks is a copy, and the product is written where it is wanted
    static void sp_spmm_panel(rri_ctx* c, int which, const double* B, int m, double* part, double* out) {
        const rri_ctx::SpCopy& cp = c->sp[which];
        if (cp.nblk > 1) { sp_spmm(c, which, B, m, part, out); return; }
        hipLaunchKernelGGL((k_sp_spmm<SX>), dim3((unsigned)((cp.nseg + 3) / 4)), dim3(256), 0, c->stream,
                           (const i64*)cp.segptr, cp.nseg, 1, (const unsigned short*)cp.idx, (const int*)cp.perm,
                           (const SX*)c->sp_x, cp.bw, B, m, out);
        spu_spmm(c, which, B, m, out);
    }
    static void sp_resid(rri_ctx* c, bool write_e, double* rowobj, double* rowpos, double* rowhat = nullptr) {
        const i64 total = (i64)c->k * c->d;
        hipLaunchKernelGGL((k_convert2d<double, double, true>), dim3((unsigned)std::min<i64>(4096, (total + 255) / 256)),
                           dim3(256), 0, c->stream, (const double*)c->T, c->LD, c->sp_Tt, (i64)c->kp, (i64)c->k, c->d);
        hipLaunchKernelGGL((k_sp_resid<SX>), dim3((unsigned)((c->n + 3) / 4)), dim3(256), 4 * (size_t)c->kp * sizeof(double),
                           c->stream, (const i64*)c->sp_rowptr, (const int*)c->sp_col, (const SX*)c->sp_x, c->n,
                           (const double*)c->W, c->ldw, (const double*)c->sp_Tt, c->k, c->kp,
                           write_e ? (SX*)c->sp_e : (SX*)nullptr, rowobj, rowpos, rowhat);
        if (c->sparse_x && c->uni_n > 0 && (rowobj || rowpos || rowhat))     // the dense rows of U replace their entries
            hipLaunchKernelGGL(k_spu_resid, dim3((unsigned)c->uni_n), dim3(256), (size_t)c->k * sizeof(double), c->stream,
                               (const int*)c->uni_rows, c->uni_value, (const double*)c->W, c->ldw, (const double*)c->T, c->LD, c->d,
                               c->k, rowobj, rowpos, rowhat);
        if (write_e && c->nnz > 0)
            for (int w = 0; w < 2; ++w)
                hipLaunchKernelGGL((k_sp_permute<SX>), dim3(2048), dim3(256), 0, c->stream, (const SX*)c->sp_e,
                                   (const int*)c->sp[w].perm, c->sp[w].count, (SX*)c->sp[w].val);
    }
    // k_wfold_rows over the canonical CSR: topics [t0, k) of every row, nwg = ceil(n / FOLD_ROWS) workgroups; false: the opt-in to
    // its dynamic LDS was refused
    static bool wfold(rri_ctx* c, int t0, int nwg) {
        return pick_int<1, 2, 3, 4>(fold_kt(c->k), [&](auto kt) {
            constexpr int KT = kt;
            if (allow_lds<k_wfold_rows<SX, KT>>(c, (int)FOLD_LDS_LIMIT) != hipSuccess) return false;
            hipLaunchKernelGGL((k_wfold_rows<SX, KT>), dim3((unsigned)nwg), dim3(64 * FOLD_WAVES), wfold_lds_bytes(c->k, FOLD_ROWS), c->stream,
                               c->W, c->Wsweep0, c->ldw, (int)c->n, c->k, t0, (const i64*)c->sp_rowptr, (const int*)c->sp_col,
                               (const SX*)c->sp_x, (const double*)c->sp_Tt, c->kp, c->fold_part, c->fold_part + (size_t)c->k * nwg, nwg,
                               kparams(c), (const DevState*)c->st);
            return true;
        });
    }
    // 0/1 masks are bit-packed (32 columns per word): the mask then costs 1/32 of its fp32 bytes per pass
    static rri_status pack_mask_if_binary(rri_ctx* c) {
        dev_release(c, c->Mbits);
        dev_release(c, c->Mcols);
        c->mcols_tried = false;
        if (!c->sw.mask_bits) return RRI_OK;
        hipError_t err = hipMemsetAsync(c->itmp, 0, sizeof(i64), c->stream);
        if (err != hipSuccess) return RRI_ERR_HIP;
        hipLaunchKernelGGL((k_mask_nonbinary<SX>), dim3(2048), dim3(256), 0, c->stream, (const SX*)c->M, c->ldm,
                           c->n, c->d, (int*)c->itmp);
        int bad = 1;
        err = hipMemcpyAsync(&bad, c->itmp, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
        if (err != hipSuccess) return RRI_ERR_HIP;
        if (bad) return RRI_OK;
        c->ldb = (c->LD + 3) / 4;   // one word per 8 rows x 4 columns
        if (dev_alloc(c, c->Mbits, (size_t)((c->n + 7) / 8) * c->ldb * sizeof(unsigned)) != hipSuccess) return RRI_ERR_HIP;
        hipLaunchKernelGGL((k_mask_pack<SX>), dim3(4096), dim3(256), 0, c->stream, (const SX*)c->M, c->ldm, c->n,
                           c->d, c->Mbits, c->ldb);
        err = hipStreamSynchronize(c->stream);
        return err == hipSuccess ? RRI_OK : RRI_ERR_HIP;
    }
    template <int NT>
    static void xtt_mfma_k(rri_ctx* c, const double* Tm, int m, double* out) {
        constexpr int VN = XVec<SX>::N;
        const size_t sh = 2 * 64 * (size_t)(16 * NT + 1) * sizeof(double) + 4 * 16 * (size_t)(64 + VN) * sizeof(SX);
        (void)allow_lds<k_xtt_mfma<SX, NT>>(c, 160 * 1024);
        hipLaunchKernelGGL((k_xtt_mfma<SX, NT>), dim3((unsigned)((c->n + 63) / 64)), dim3(256), sh, c->stream,
                           (const SX*)c->X, c->ldx, Tm, c->LD, (int)c->n, (int)c->d, m, out, c->ldw, xscale(c));
    }
    static void xtt_any(rri_ctx* c, const double* Tm, int m, double* out) {   // out (m x n) = (X Tm^T)^T
        for (int l0 = 0; l0 < m; l0 += 64) {     // the product on the matrix cores, up to 64 rows of Tm per launch
            const int mm = std::min(64, m - l0);
            const double* Tp = Tm + (i64)l0 * c->LD;
            double* op = out + (i64)l0 * c->ldw;
            pick_int<1, 2, 3, 4>((mm + 15) / 16, [&](auto nt) { xtt_mfma_k<nt>(c, Tp, mm, op); });      // 16 rows of Tm per tile
        }
    }
    static void xtt(rri_ctx* c) {
        if constexpr (!RO) {
            if (c->sparse_x) { spx_xtt(c, c->T, c->k, c->Qt); return; }
        }
        xtt_any(c, c->T, c->k, c->Qt);
    }
    // column sums against NV = 8 row-vectors at once (Qt: 8 x n, stride ldw): out rows <- X^T q_v
    static void colsums8(rri_ctx* c, const double* Qt, int nv, double* zmulti, double* out_rows) {
        constexpr int NV = 8;
        const int ncols = (int)std::min<i64>(c->ldx, c->LD);
        hipLaunchKernelGGL((k_colsums<SX, NV>), dim3(c->npanels * c->nrb), dim3(256), (size_t)NV * c->rpb * sizeof(double),
                           c->stream, (const SX*)c->X, c->ldx, (int)c->n, ncols, Qt, c->ldw, nv, zmulti, c->LD, c->rpb,
                           c->npanels, c->nrb, xscale(c));
        const int nb = (int)((c->LD + 31) / 32);
        for (int v = 0; v < nv; ++v)
            hipLaunchKernelGGL(k_reduce, dim3(nb), dim3(1024), 0, c->stream,
                               (const double*)zmulti + (i64)v * c->nrb * c->LD, c->LD, c->nrb, (const double*)nullptr, 0,
                               c->k, out_rows + (i64)v * c->LD, (const DevState*)c->st);
    }
    static bool resid_w_resident(const rri_ctx* c) { return c->k <= 256; }   // 128 KiB of W tile at most
    static size_t resid_shmem(const rri_ctx* c) {
        return ((size_t)(resid_w_resident(c) ? c->k : 32) * 64 + 32 * 64) * sizeof(double) + 64 * 17 * sizeof(double);
    }
    // X - W T by 64-row blocks: its row sums (rowobj, rowpos; the objective and the max-residual reset) and, with write_e, the
    // residual itself into c->E (under the mask if masked).  A read-only handle has no mask and writes nothing, whatever is
    // asked: MASKED = WRITE_E = false with null mask and E arguments is all it launches, and all that is built for it.
    static void resid(rri_ctx* c, bool masked, bool write_e, double* rowobj, double* rowpos) {
        if constexpr (!RO) {
            if (c->sparse) { sp_resid(c, write_e, rowobj, rowpos); return; }   // outside the pattern nothing contributes
        }
        const SX* M = RO ? nullptr : (const SX*)c->M;
        const unsigned* Mbits = RO ? nullptr : (const unsigned*)c->Mbits;
        SX* E = RO ? nullptr : (SX*)c->E;
        const i64 ldm = RO ? 0 : c->ldm, ldb = RO ? 0 : c->ldb;
        auto flavour = [&](auto&& f) {     // f(MASKED, WRITE_E)
            if constexpr (RO) f(std::false_type{}, std::false_type{});
            else pick_bool(masked, [&](auto mk) { pick_bool(write_e, [&](auto we) { f(mk, we); }); });
        };
        const unsigned nb = (unsigned)((c->n + 63) / 64);
        if (c->k <= 64) {   // the k-panel product on the matrix cores
            const int ks = resid_ks(c->k);
            const size_t shm = 2 * (size_t)(4 * ks) * RESID_TS * sizeof(double);
            const bool sums = rowobj || rowpos;      // a plain rebuild wants neither: its epilogue is convert, subtract, store
            flavour([&](auto mk, auto we) {
                constexpr bool MK = mk, WE = we;
                pick_int<4, 8, 12, 13, 16>(ks, [&](auto KS) {
                    // a residual written without its row sums (the per-sweep rebuild of the explicit-residual schedule) skips them
                    pick_bool(sums || !WE, [&](auto sm) {
                        constexpr bool SM = sm;
                        // SM = false exists only for WRITE_E = true: no WRITE_E = false caller can reach it, so it is not built
                        if constexpr (SM || WE) {
                            const ResidGrid g = resid_grid(c->n, c->d, c->n_cu, SM);      // without the row sums: column ranges per row block
                            const int dchunk = g.dchunk;
                            hipLaunchKernelGGL((k_resid_mfma<SX, MK, WE, KS, 4, SM>), dim3(g.nb, g.ny), dim3(256), shm, c->stream,
                                               (const SX*)c->X, c->ldx, M, ldm, Mbits, ldb, (const double*)c->W, c->ldw,
                                               (const double*)c->T, c->LD, (int)c->n, (int)c->d, c->k, rowobj, rowpos, E, c->LD, dchunk, xscale(c));
                        }
                    });
                });
            });
            return;
        }
        const size_t sh = resid_shmem(c);
        flavour([&](auto mk, auto we) {
            hipLaunchKernelGGL((k_resid<SX, mk, we>), dim3(nb), dim3(256), sh, c->stream, (const SX*)c->X, c->ldx, M, ldm, Mbits, ldb,
                               (const double*)c->W, c->ldw, (const double*)c->T, c->LD, (int)c->n, (int)c->d, c->k, rowobj, rowpos, E,
                               c->LD, resid_w_resident(c) ? 1 : 0, xscale(c));
        });
    }
    static void reset_row(rri_ctx* c) {
        if constexpr (!RO) {
            if (c->sparse) {
                (void)hipMemsetAsync(c->xraw, 0, (size_t)c->LD * sizeof(double), c->stream);
                hipLaunchKernelGGL((k_sp_reset_row<SX>), dim3((unsigned)std::max(1, (c->sp_max_row + 255) / 256)), dim3(256), 0,
                                   c->stream, (const i64*)c->sp_rowptr, (const int*)c->sp_col, (const SX*)c->sp_x,
                                   (const double*)c->W, c->ldw, (const double*)c->T, c->LD, c->k, (const i64*)c->itmp,
                                   c->xraw);
                if (c->sparse_x && c->uni_n > 0)     // a uniform row won: its reset row is dense
                    hipLaunchKernelGGL(k_spu_reset_row, dim3((unsigned)((c->d + 255) / 256)), dim3(256), 0, c->stream,
                                       (const int*)c->uni_rows, (int)c->uni_n, c->uni_value, (const double*)c->W, c->ldw,
                                       (const double*)c->T, c->LD, c->d, c->k, (const i64*)c->itmp, c->xraw);
                return;
            }
        }
        hipLaunchKernelGGL((k_reset_row<SX>), dim3((unsigned)((c->d + 255) / 256)), dim3(256), 0, c->stream,
                           (const SX*)c->X, c->ldx, (const double*)c->W, c->ldw, (const double*)c->T, c->LD,
                           (int)c->d, c->k, (const i64*)c->itmp, c->xraw, xscale(c));
    }
    static hipError_t set_attrs(const rri_ctx* c) {
        hipError_t e = allow_lds<k_resid<SX, false, false>>(c, 160 * 1024);
        if constexpr (!RO) {
            if (e == hipSuccess) e = allow_lds<k_resid<SX, true, true>>(c, 160 * 1024);
            if (e == hipSuccess) e = allow_lds<k_resid<SX, true, false>>(c, 160 * 1024);
            if (e == hipSuccess) e = allow_lds<k_resid<SX, false, true>>(c, 160 * 1024);
            if (e == hipSuccess) e = allow_lds<k_spx_pass<SX>>(c, SP_BLOCK_BYTES + 64);
        }
        return e;
    }
};

// Everything that writes X, the mask or a residual, or reads a CSR store: float32 and float64 only.  A float16 handle
// (RRI_F16; RRI_U8 likewise) is refused at the entry points that lead here; should one arrive all the same, nothing is launched and the call
// that enqueued the sequence ends with RRI_ERR_UNSUPPORTED (f16_unreachable) -- never the double branch on 2-byte data.
#define DISPATCH(c, expr)                       \
    do {                                        \
        if ((c)->dtype == RRI_F32) {            \
            typedef LaunchX<float> L;           \
            expr;                               \
        } else if ((c)->dtype == RRI_F64) {     \
            typedef LaunchX<double> L;          \
            expr;                               \
        } else {                                \
            f16_unreachable(c);                 \
        }                                       \
    } while (0)
// The kernels that only READ a dense X (the pass with UPD = 0, X T^T, X^T Q, the residual's row sums, the reset row, ||X||^2):
// the four storage types (rri_create admits no other code).
#define DISPATCH_RO(c, expr)                    \
    do {                                        \
        if ((c)->dtype == RRI_F32) {            \
            typedef LaunchX<float> L;           \
            expr;                               \
        } else if ((c)->dtype == RRI_F64) {     \
            typedef LaunchX<double> L;          \
            expr;                               \
        } else if ((c)->dtype == RRI_F16) {     \
            typedef LaunchX<_Float16> L;        \
            expr;                               \
        } else {                                \
            typedef LaunchX<unsigned char> L;   \
            expr;                               \
        }                                       \
    } while (0)

struct LK {  // float64-only kernels
    // rows of Gpart a column update leaves: one per 64-row tile (k_wcol) or per 256-row block (k_wcol_resid)
    static int gpart_rows(const rri_ctx* c) { return c->gpart_n; }
    template <bool UPDATE>
    static void wcol_resid(rri_ctx* c, int t, int tn, int sweep) {
        TimedScope ts(c, 1);
        hipLaunchKernelGGL((k_wcol_resid<UPDATE>), dim3(c->nwb256), dim3(256), 0, c->stream, c->W, c->ldw, (int)c->n,
                           c->k, t, tn, (const double*)c->Ypart, c->npanels, (const double*)c->Ttpart, c->nsplit,
                           c->dwv, c->Gpart, sweep, kparams(c), c->st);
        c->gpart_n = c->nwb256;
    }
    static size_t wcol_shmem(const rri_ctx* c) { return (size_t)(2 * c->k + 2 + 256 + 64) * sizeof(double); }
    template <bool UPDATE, bool CARRY>
    static void wcol_src(rri_ctx* c, int t, int tn, int sweep, const double* ypart, int nslices) {
        TimedScope ts(c, 1);
        hipLaunchKernelGGL((k_wcol<UPDATE, CARRY>), dim3(c->nwb), dim3(256), wcol_shmem(c), c->stream, c->W, c->ldw,
                           (int)c->n, c->k, t, tn, ypart, nslices, (const double*)c->Ttpart, c->ttpart_n, c->Gpart,
                           c->XYpart + (i64)t * c->xy_stride, sweep, kparams(c), c->st);
        c->gpart_n = c->nwb;
        if (UPDATE) note_xy(c, t, c->nwb * WCOL_TILES);
    }
    // the cross terms <w_t, X t_t> of topic t were left in XYpart as `rows` block partials: the objective after the
    // sweep needs all k topics in order, written with the same block count
    static void note_xy(rri_ctx* c, int t, int rows) {
        if (t == 0) { c->xy_run = 1; c->xy_rows = rows; }
        else c->xy_run = (c->xy_run == t && c->xy_rows == rows) ? t + 1 : -1;
        c->xy_valid = c->xy_run == c->k;
    }
    template <bool UPDATE, bool CARRY>
    static void wcol(rri_ctx* c, int t, int tn, int sweep) {
        wcol_src<UPDATE, CARRY>(c, t, tn, sweep, (const double*)c->Ypart, c->npanels);
    }
    // the frozen rows' share of [w_t^T X | w_t^T W, ||w_t||^2, sum W[:,tprev]] into red (tprev < 0: no column check pending)
    static void frozen_add(rri_ctx* c, int t, int tprev) {
        if (!c->fzB) return;
        hipLaunchKernelGGL(k_frozen_add, dim3((unsigned)((c->LD + 255) / 256)), dim3(256), 0, c->stream, c->red, c->LD, c->k, t,
                           tprev, (const double*)c->fzB, (const double*)c->fzA, (const double*)c->fzs);
    }
    static void reduce(rri_ctx* c) {
        const int nb = (int)((c->LD + 31) / 32) + GRAM_SLICES;
        hipLaunchKernelGGL(k_reduce, dim3(nb), dim3(1024), 0, c->stream, (const double*)c->Zpart, c->LD, c->nrb,
                           (const double*)c->Gpart, gpart_rows(c), c->k, c->red, (const DevState*)c->st);
    }
    // no simplex projection configured: k_trow_numer stores the row itself and k_tgram finishes the checks
    static bool light(const rri_ctx* c) { return !(c->prm.project_T_each_iter && c->prm.has_t_row_sum); }
    // ---- the early-sums schedule (RRI_EARLY_SUMS): the W-sized sums of a topic step ride in the grid of its pass ----
    // The handles it is for: a dense unweighted X of the Gram form, every storage type; both factors moving, one device, no
    // projection, and not the launch-bound sizes that take k_trow_small.  Everything else keeps k_wcol.  (Frozen rows ride
    // along -- they add their share into red between k_wfin and k_trow_early, as between k_reduce and k_trow_numer -- so that a
    // handle with all-zero statistics keeps the bits of one without any.)
    static bool early_ok(const rri_ctx* c) {
        return c->sw.early_sums && c->Tearly && !c->weighted && !c->explicit_resid && !c->sparse && c->k > 1 && !c->prm.fix_T &&
               !c->prm.fix_W && !c->comm && light(c) && !(small(c) && !c->fzB && c->sw.trow_fused) && WCOL_TILES == 1 &&
               early_job_lds_doubles(c->k) <= 5 * (size_t)c->rpb + 4 * 8 * 72;     // the pass's own LDS (pass_shmem) holds the job
    }
    static EarlyJob early_job(const rri_ctx* c, int t, int tn) {
        return EarlyJob{(const double*)c->W, c->ldw, (int)c->n, c->k, t, tn, (const double*)c->Tearly, c->plan.nte, c->edot,
                        c->Gearly, c->ent, early_job_first(c->npanels * c->nrb, c->n_cu), c->plan.e_blocks, c->plan.e_tpb,
                        c->plan.e_stride};
    }
    // the launch after the pass: the column update from the early job's sums, k_reduce's blocks in the same grid
    static void wfin(rri_ctx* c, int t, int tn, int sweep) {
        TimedScope ts(c, 1);
        const int nredb = (int)((c->LD + 31) / 32) + GRAM_SLICES;
        hipLaunchKernelGGL(k_wfin, dim3(nredb + c->plan.nwfin), dim3(1024), 0, c->stream, c->W, c->ldw, (int)c->n, c->k, t, tn,
                           (const double*)c->Ypart, c->npanels, (const double*)c->edot, (const double*)c->ent, c->Gpart,
                           c->wfp, c->nwb, c->XYpart + (i64)t * c->xy_stride, (const double*)c->Zpart, c->LD, c->nrb, (const double*)c->Gearly,
                           c->plan.e_blocks, c->red, nredb, sweep, kparams(c), c->st);
        c->gpart_n = c->nwb;
        c->early_steps += 1;
        note_xy(c, t, c->nwb * WCOL_TILES);
    }
    // the T-row update that leaves T T[t,:]^T for the early job of the pass that follows
    static void trow_early(rri_ctx* c, int t, int check_prev, int tprev, int sweep) {
        hipLaunchKernelGGL(k_trow_early, dim3(c->plan.nte), dim3(1024), 0, c->stream, c->T, c->LD, (int)c->d, c->k, t,
                           (const double*)c->red, c->LD, c->carry_wfin ? (const double*)c->wfp : (const double*)nullptr, c->nwb,
                           c->wfin_topic, c->xraw, c->tpart, c->Tearly, check_prev, tprev, sweep, kparams(c), c->st);
        c->tpart_n = c->ntb;
    }
    static void trow(rri_ctx* c, int t, int check_prev, int tprev, int sweep, bool force_final) {
        hipLaunchKernelGGL(k_trow_numer, dim3(c->ntb), dim3(128), 0, c->stream, c->T, c->LD, (int)c->d, c->k, t,
                           (const double*)c->red, c->LD, c->xraw, c->tpart, c->tpart_idx, check_prev, tprev, sweep,
                           kparams(c), c->st, resid_sched(c) ? 1 : 0, resid_sched(c) ? c->told : (double*)nullptr);
        c->tpart_n = c->ntb;
        trow_final_if_needed(c, t, sweep, force_final);
    }
    // launch-bound sizes: k_reduce and k_trow_numer as one launch (every workgroup reduces the Gram partials itself)
    static bool small(const rri_ctx* c) { return rri::trow_small(gpart_rows(c), c->k, c->ntb32); }
    static void trow_small(rri_ctx* c, int t, int check_prev, int tprev, int sweep, bool force_final) {
        hipLaunchKernelGGL(k_trow_small, dim3(c->ntb32), dim3(1024), 0, c->stream, c->T, c->LD, (int)c->d, c->k, t,
                           (const double*)c->Zpart, c->nrb, (const double*)c->Gpart, gpart_rows(c), c->red, c->LD, c->xraw,
                           c->tpart, c->tpart_idx, check_prev, tprev, sweep, kparams(c), c->st, resid_sched(c) ? 1 : 0,
                           resid_sched(c) ? c->told : (double*)nullptr);
        c->tpart_n = c->ntb32;
        trow_final_if_needed(c, t, sweep, force_final);
    }
    static void trow_final_if_needed(rri_ctx* c, int t, int sweep, bool force_final) {
        if (!light(c) || force_final)
            hipLaunchKernelGGL(k_trow_final, dim3(1), dim3(1024), 0, c->stream, c->T, c->LD, (int)c->d, t, c->xraw,
                               (const double*)c->tpart, (const i64*)c->tpart_idx, c->tpart_n, sweep, kparams(c), c->st);
    }
    static void check_prev_only(rri_ctx* c, int tprev, int sweep, int pos) {
        hipLaunchKernelGGL(k_check_red, dim3(1), dim3(64), 0, c->stream, (const double*)c->red, c->LD, c->k, tprev,
                           sweep, pos, kparams(c), c->st);
    }
    static void tgram(rri_ctx* c, int t, int finish, int sweep) {
        c->ttpart_n = c->nsplit;
        hipLaunchKernelGGL(k_tgram, dim3(c->k, c->nsplit), dim3(256), 0, c->stream, (const double*)c->T, c->LD,
                           (int)c->d, c->k, t, c->Ttpart, (const double*)c->tpart, c->tpart_n, finish, sweep,
                           kparams(c), c->st);
    }
    static void scale_wcol(rri_ctx* c, int t) {
        hipLaunchKernelGGL(k_scale_wcol, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->W,
                           c->ldw, (int)c->n, t, (const DevState*)c->st);
    }
    static void check_wcol(rri_ctx* c, int tprev, int sweep, int pos) {
        hipLaunchKernelGGL(k_check_wcol, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, gpart_rows(c), c->k,
                           tprev, sweep, pos, kparams(c), c->st);
    }
    static void proj_rows(rri_ctx* c, double s, const double* svec) {
        hipLaunchKernelGGL(k_proj_rows, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->W, c->ldw, (int)c->n, c->k, s,
                           svec);
    }
    static void norms(rri_ctx* c, const double* A, i64 rows, i64 cols, i64 ld) {
        hipLaunchKernelGGL(k_norms, dim3(256), dim3(256), 0, c->stream, A, rows, cols, ld, c->normpart);
    }
    static void reset_commit(rri_ctx* c, int t) {
        const i64 m = std::max(c->n, c->d);
        hipLaunchKernelGGL(k_reset_commit, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, c->W, c->ldw,
                           c->T, c->LD, (int)c->n, (int)c->d, t, (const i64*)c->itmp, (const double*)c->xraw);
    }
    static void set_row_col(rri_ctx* c, int t, const double* trow, const double* wcolv) {
        const i64 m = std::max(c->n, c->d);
        hipLaunchKernelGGL(k_set_row_col, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, c->W, c->ldw,
                           c->T, c->LD, (int)c->n, (int)c->d, t, trow, wcolv);
    }
    static void argmax_rows(rri_ctx* c, int* out) {
        hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)c->W, c->ldw, (int)c->n, c->k, out);
    }
    static void masked_sqerr(rri_ctx* c, const i64* ij, const double* vals, i64 count, double lo, double hi) {
        hipLaunchKernelGGL(k_masked_sqerr, dim3(256), dim3(256), 0, c->stream, (const double*)c->W, c->ldw,
                           (const double*)c->T, c->LD, c->k, ij, vals, count, lo, hi, c->normpart);
    }
    // the N best columns of W T for `count` requested rows (rri_topn_kernels.hpp); reads W and T, writes the two outputs only
    static hipError_t topn_rows(rri_ctx* c, const i64* rows, i64 count, int N, const i64* eptr, const int* eidx, const i64* erow,
                                double lo, double hi, int* idx_out, double* val_out) {
        const hipError_t e = allow_lds<k_topn_rows>(c, 64 * 1024);
        if (e != hipSuccess) return e;
        TimedScope ts(c, 4);
        hipLaunchKernelGGL(k_topn_rows, dim3((unsigned)((count + TOPN_ROWS - 1) / TOPN_ROWS)), dim3(256), topn_lds_bytes(N),
                           c->stream, (const double*)c->W, c->ldw, (const double*)c->T, c->LD, (int)c->d, c->k, rows, count, N,
                           eptr, eidx, erow, lo, hi, idx_out, val_out);
        return hipGetLastError();
    }
    // the ranks of listed columns of W T, piece by piece (rri_rank_kernels.hpp); reads W and T, writes the three outputs only
    static hipError_t rank_entries(rri_ctx* c, const i64* rows, const RankPiece* pieces, i64 npieces, const int* tidx,
                                   const i64* eptr, const int* eidx, const i64* erow, double lo, double hi, int* rank_out,
                                   double* val_out, int* elig_out) {
        const hipError_t e = allow_lds<k_rank_entries>(c, (int)rank_lds_bytes());
        if (e != hipSuccess) return e;
        TimedScope ts(c, 5);
        hipLaunchKernelGGL(k_rank_entries, dim3((unsigned)((npieces + RANK_PIECES - 1) / RANK_PIECES)), dim3(256), rank_lds_bytes(),
                           c->stream, (const double*)c->W, c->ldw, (const double*)c->T, c->LD, (int)c->d, c->k, rows, pieces, npieces,
                           tidx, eptr, eidx, erow, lo, hi, rank_out, val_out, elig_out);
        return hipGetLastError();
    }
    // the masks of the rows [ch.r0, ch.r1) of a CSR pattern and the pair counts of those masks, added to codf
    // (rri_cooc_kernels.hpp); reads the call's temporaries and writes masks and codf only
    static hipError_t cooc_chunk(rri_ctx* c, const i64* indptr, const int* indices, const int* mptr, const int* ment,
                                 const CoocChunk& ch, int lps, int n_groups, int group_size, unsigned* masks,
                                 unsigned long long* codf) {
        const size_t lds = cooc_mask_lds_bytes(n_groups);
        hipError_t e = lps == 64 ? allow_lds<k_cooc_masks<64>>(c, (int)cooc_mask_lds_bytes(RRI_MAX_K))
                                 : allow_lds<k_cooc_masks<8>>(c, (int)cooc_mask_lds_bytes(RRI_MAX_K));
        if (e != hipSuccess) return e;
        const dim3 tiles((unsigned)(ch.rows_pad / COOC_TILE_ROWS));
        {
            TimedScope ts(c, 6);
            if (lps == 64)
                hipLaunchKernelGGL(k_cooc_masks<64>, tiles, dim3(256), lds, c->stream, indptr, indices, mptr, ment, ch.r0, ch.r1,
                                   n_groups, ch.rows_pad, masks);
            else
                hipLaunchKernelGGL(k_cooc_masks<8>, tiles, dim3(256), lds, c->stream, indptr, indices, mptr, ment, ch.r0, ch.r1,
                                   n_groups, ch.rows_pad, masks);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        {
            TimedScope ts(c, 6);
            const dim3 pieces((unsigned)((ch.rows_pad + COOC_COUNT_ROWS - 1) / COOC_COUNT_ROWS), (unsigned)n_groups);
            auto count = [&](auto ppt) {
                hipLaunchKernelGGL(k_cooc_count<decltype(ppt)::value>, pieces, dim3(256), 0, c->stream, (const unsigned*)masks,
                                   ch.rows_pad, group_size, codf);
            };
            switch (cooc_count_ppt(group_size)) {
                case 1: count(std::integral_constant<int, 1>()); break;
                case 2: count(std::integral_constant<int, 2>()); break;
                case 4: count(std::integral_constant<int, 4>()); break;
                default: count(std::integral_constant<int, 9>()); break;
            }
        }
        return hipGetLastError();
    }
    // the transposed copy of T that k_loglik_entries reads: Tt (d x kp), the pad column of an odd k zero
    static hipError_t loglik_transpose(rri_ctx* c, double* Tt) {
        const int kp = loglik_kp(c->k);
        const i64 total = (i64)c->k * c->d;
        TimedScope ts(c, 7);
        if (kp != c->k) {
            const hipError_t e = hipMemsetAsync(Tt, 0, (size_t)c->d * kp * sizeof(double), c->stream);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((k_convert2d<double, double, true>), dim3((unsigned)std::min<i64>(4096, (total + 255) / 256)),
                           dim3(256), 0, c->stream, (const double*)c->T, c->LD, Tt, (i64)kp, (i64)c->k, c->d);
        return hipGetLastError();
    }
    // the partials of a chunk's pieces and their sums per request (rri_loglik_kernels.hpp); reads W, Tt and the call's
    // temporaries, writes the partials and the chunk's three outputs only
    static hipError_t loglik_chunk(rri_ctx* c, const double* Tt, const i64* rows, i64 q0, i64 nreq, const LoglikPiece* pieces,
                                   i64 npieces, const i64* first, const int* indices, const double* values, double floor,
                                   double* pll, double* pmass, i64* pfl, double* ll, double* mass, i64* fl) {
        const size_t lds = 4 * (size_t)loglik_kp(c->k) * sizeof(double);
        {
            TimedScope ts(c, 7);
            const dim3 grid((unsigned)((npieces + 3) / 4));
            auto entries = [&](auto lanes) {
                hipLaunchKernelGGL(k_loglik_entries<decltype(lanes)::value>, grid, dim3(256), lds, c->stream, (const double*)c->W,
                                   c->ldw, Tt, c->k, rows, q0, pieces, npieces, indices, values, floor, pll, pmass, pfl);
            };
            switch (loglik_lanes(c->k)) {
                case 4: entries(std::integral_constant<int, 4>()); break;
                case 16: entries(std::integral_constant<int, 16>()); break;
                default: entries(std::integral_constant<int, 64>()); break;      // a measurement build (-DRRI_LOGLIK_LANES=64) only
            }
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        {
            TimedScope ts(c, 7);
            hipLaunchKernelGGL(k_loglik_sum, dim3((unsigned)((nreq + 255) / 256)), dim3(256), 0, c->stream, first, nreq,
                               (const double*)pll, (const double*)pmass, (const i64*)pfl, ll, mass, fl);
        }
        return hipGetLastError();
    }
};

// ---- upload / download with conversion -------------------------------------------------------
// dst (stride ldd) <- src (rows x cols, stride lds_), transposed if asked (dst is then cols x rows); the element types by
// their dtype codes, float32 or float64 each
void launch_convert(rri_ctx* c, int src_dtype, int dst_dtype, bool transpose, const void* src, i64 lds_, void* dst, i64 ldd,
                    i64 rows, i64 cols) {
    const i64 total = rows * cols;
    const unsigned nb = (unsigned)std::min<i64>(4096, (total + 255) / 256);
    pick_type<float, double>(src_dtype, [&](auto s) {
        typedef typename decltype(s)::type Src;
        pick_type<float, double>(dst_dtype, [&](auto d) {
            typedef typename decltype(d)::type Dst;
            pick_bool(transpose, [&](auto tr) {
                hipLaunchKernelGGL((k_convert2d<Src, Dst, tr>), dim3(nb ? nb : 1), dim3(256), 0, c->stream, (const Src*)src,
                                   lds_, (Dst*)dst, ldd, rows, cols);
            });
        });
    });
}

// host (rows x cols, stride ld; float32, float64 or float16) -> device float16 (the X of an RRI_F16 handle): one rounding to
// nearest even from the host type (k_store_half), with the cost of that rounding left in c->store_err.  A float16 host
// buffer takes the same route -- the conversion is then the identity -- so that inf / NaN in it are seen too.  A value that is
// not finite as a half fails the call with RRI_ERR_INVALID (the caller drops the X).
rri_status to_device_half(rri_ctx* c, const void* host, i64 ld, int host_dtype, void* dev, i64 ldd, i64 rows, i64 cols,
                          bool transpose) {
    if (transpose) return fail(c, RRI_ERR_INVALID, "float16 storage is for X only");
    const size_t hs = dtype_size(host_dtype);
    const i64 total = rows * cols;
    const unsigned nb = (unsigned)std::max<i64>(1, std::min<i64>(4096, (total + 255) / 256));
    DevTmp tmp, part;
    HIPCHK(c, tmp.alloc((size_t)rows * cols * hs));
    HIPCHK(c, part.alloc((size_t)nb * 3 * sizeof(double)));
    HIPCHK(c, hipMemcpy2DAsync(tmp.p, cols * hs, host, ld * hs, cols * hs, rows, hipMemcpyHostToDevice, c->stream));
    pick_type<float, double, _Float16>(host_dtype, [&](auto src) {
        typedef typename decltype(src)::type Src;
        hipLaunchKernelGGL((k_store_half<Src>), dim3(nb), dim3(256), 0, c->stream, (const Src*)tmp.p, cols, (_Float16*)dev, ldd,
                           rows, cols, (double*)part.p);
    });
    std::vector<double> h((size_t)nb * 3);
    HIPCHK(c, hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double se = 0.0, sx = 0.0, bad = 0.0;
    for (unsigned b = 0; b < nb; ++b) { se += h[3 * b]; sx += h[3 * b + 1]; bad += h[3 * b + 2]; }
    c->store_err[0] = se;
    c->store_err[1] = sx;
    if (bad > 0.0)
        return fail(c, RRI_ERR_INVALID, "value outside the float16 range at upload (%.0f of them: |x| >= 65520, inf or NaN)", bad);
    return RRI_OK;
}

// host (rows x cols, stride ld; float32, float64 or bytes) -> device bytes (the counts of an RRI_U8 handle).  Bytes are copied as
// they are; a floating type goes through k_store_u8, and one value that is not an integer in 0..255 fails the call with
// RRI_ERR_INVALID (the caller drops the X).  Nothing is rounded, so store_err stays zero.
rri_status to_device_u8(rri_ctx* c, const void* host, i64 ld, int host_dtype, void* dev, i64 ldd, i64 rows, i64 cols,
                        bool transpose) {
    if (transpose) return fail(c, RRI_ERR_INVALID, "uint8 storage is for X only");
    if (host_dtype == RRI_U8) {
        HIPCHK(c, hipMemcpy2DAsync(dev, ldd, host, ld, cols, rows, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return RRI_OK;
    }
    const size_t hs = dtype_size(host_dtype);
    const i64 total = rows * cols;
    const unsigned nb = (unsigned)std::max<i64>(1, std::min<i64>(4096, (total + 255) / 256));
    DevTmp tmp, part;
    HIPCHK(c, tmp.alloc((size_t)rows * cols * hs));
    HIPCHK(c, part.alloc((size_t)nb * sizeof(double)));
    HIPCHK(c, hipMemcpy2DAsync(tmp.p, cols * hs, host, ld * hs, cols * hs, rows, hipMemcpyHostToDevice, c->stream));
    pick_type<float, double>(host_dtype, [&](auto src) {
        typedef typename decltype(src)::type Src;
        hipLaunchKernelGGL((k_store_u8<Src>), dim3(nb), dim3(256), 0, c->stream, (const Src*)tmp.p, cols, (unsigned char*)dev, ldd,
                           rows, cols, (double*)part.p);
    });
    std::vector<double> h((size_t)nb);
    HIPCHK(c, hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double bad = 0.0;
    for (unsigned b = 0; b < nb; ++b) bad += h[b];
    if (bad > 0.0)
        return fail(c, RRI_ERR_INVALID, "value that is not an integer in 0..255 at upload (%.0f of them: fractions, negatives, > 255, inf or NaN)", bad);
    return RRI_OK;
}
// both scale vectors of an RRI_U8 handle back to ones (a new X)
rri_status reset_scales(rri_ctx* c) {
    if (c->dtype != RRI_U8) return RRI_OK;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->rscale, c->n, 1.0);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((c->LD + 255) / 256)), dim3(256), 0, c->stream, c->cscale, c->LD, 1.0);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

// the argument checks of to_device, for the callers that change the handle before they get there (rri_upload_X, rri_upload_mask):
// a refused call leaves the handle as it was
rri_status check_host_matrix(rri_ctx* c, const void* host, i64 ld, int host_dtype, i64 cols, int dev_dtype) {
    if (!host || ld < cols) return fail(c, RRI_ERR_INVALID, "bad host matrix (ld=%lld < cols=%lld)", ld, cols);
    // a float16 host buffer goes onto a float16 handle only (nothing else is ever given as halves)
    // ... and a buffer of bytes onto a uint8 handle only
    if (host_dtype != RRI_F32 && host_dtype != RRI_F64 && !(host_dtype == RRI_F16 && dev_dtype == RRI_F16) &&
        !(host_dtype == RRI_U8 && dev_dtype == RRI_U8))
        return fail(c, RRI_ERR_INVALID, "bad host dtype");
    return RRI_OK;
}

// host (rows x cols, stride ld, host_dtype) -> device (stride ldd, dev_dtype).
// transpose: the device image is cols x rows (dst[c][r] = host[r][c]).
rri_status to_device(rri_ctx* c, const void* host, i64 ld, int host_dtype, void* dev, i64 ldd, i64 rows,
                     i64 cols, int dev_dtype, bool transpose = false) {
    if (rri_status s = check_host_matrix(c, host, ld, host_dtype, cols, dev_dtype)) return s;
    const size_t hs = dtype_size(host_dtype);
    const size_t ds = dtype_size(dev_dtype);
    if (dev_dtype == RRI_F16) return to_device_half(c, host, ld, host_dtype, dev, ldd, rows, cols, transpose);
    if (dev_dtype == RRI_U8) return to_device_u8(c, host, ld, host_dtype, dev, ldd, rows, cols, transpose);
    if (host_dtype == dev_dtype && !transpose) {
        HIPCHK(c, hipMemcpy2DAsync(dev, ldd * ds, host, ld * hs, cols * hs, rows, hipMemcpyHostToDevice,
                                   c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return RRI_OK;
    }
    DevTmp tmp;
    HIPCHK(c, tmp.alloc((size_t)rows * cols * hs));
    hipError_t e = hipMemcpy2DAsync(tmp.p, cols * hs, host, ld * hs, cols * hs, rows, hipMemcpyHostToDevice,
                                    c->stream);
    if (e == hipSuccess) {
        launch_convert(c, host_dtype, dev_dtype, transpose, tmp.p, cols, dev, ldd, rows, cols);
        e = hipStreamSynchronize(c->stream);
    }
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

// device (dev_dtype, stride ldd) -> host rows x cols.  transpose: the device image is cols x rows.
rri_status to_host(rri_ctx* c, const void* dev, i64 ldd, void* host, i64 ld, int host_dtype, i64 rows, i64 cols,
                   int dev_dtype, bool transpose = false) {
    if (!host || ld < cols) return fail(c, RRI_ERR_INVALID, "bad host matrix (ld=%lld < cols=%lld)", ld, cols);
    if (host_dtype != RRI_F32 && host_dtype != RRI_F64) return fail(c, RRI_ERR_INVALID, "bad host dtype");
    if (dev_dtype != RRI_F32 && dev_dtype != RRI_F64) return fail(c, RRI_ERR_UNSUPPORTED, "nothing stored as float16 or uint8 is read back");
    const size_t hs = dtype_size(host_dtype);
    const size_t ds = dtype_size(dev_dtype);
    if (host_dtype == dev_dtype && !transpose) {
        HIPCHK(c, hipMemcpy2DAsync(host, ld * hs, dev, ldd * ds, cols * hs, rows, hipMemcpyDeviceToHost,
                                   c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return RRI_OK;
    }
    DevTmp tmp;
    HIPCHK(c, tmp.alloc((size_t)rows * cols * hs));
    // source is the device image; for a transposed image its shape is cols x rows
    launch_convert(c, dev_dtype, host_dtype, transpose, dev, ldd, tmp.p, cols, transpose ? cols : rows, transpose ? rows : cols);
    hipError_t e = hipMemcpy2DAsync(host, ld * hs, tmp.p, cols * hs, cols * hs, rows, hipMemcpyDeviceToHost,
                                    c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "download failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

// ---- the topic-step scheduler ------------------------------------------------------------------
// The column verdict of _check_reset_W / the assert of nmf.py:471-476 from the partial sums in Gpart, taken NOW
// (where no T-row step follows that would carry it).  Row-sharded: the column sum is global, so the local share is
// all-reduced first (2 doubles) and every rank reaches the same verdict.
void wcheck_now(rri_ctx* c, int tprev, int sweep, int pos) {
    if (!c->comm && c->fzB && !c->prm.fix_T) {
        // frozen rows: the communicator's route with the all-reduce replaced by the addend s[tprev]
        hipLaunchKernelGGL(k_colsum_tail, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, LK::gpart_rows(c),
                           c->k, c->fztail, (const DevState*)c->st);
        hipLaunchKernelGGL(k_frozen_add_tail, dim3(1), dim3(64), 0, c->stream, c->fztail, tprev, (const double*)c->fzs);
        hipLaunchKernelGGL(k_wcheck_tail, dim3(1), dim3(64), 0, c->stream, (const double*)c->fztail, tprev, sweep, pos,
                           kparams(c), c->st);
        return;
    }
    if (!c->comm) {
        if (c->weighted)
            hipLaunchKernelGGL(k_wcheck_wcol, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, c->nwb256, c->k,
                               tprev, sweep, pos, kparams(c), c->st, (double*)nullptr);
        else LK::check_wcol(c, tprev, sweep, pos);
        return;
    }
    if (c->weighted)
        hipLaunchKernelGGL(k_wcheck_wcol, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, c->nwb256, c->k,
                           tprev, sweep, pos, kparams(c), c->st, c->ctail);
    else
        hipLaunchKernelGGL(k_colsum_tail, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, LK::gpart_rows(c),
                           c->k, c->ctail, (const DevState*)c->st);
    comm_allreduce(c, c->ctail, 2);
    hipLaunchKernelGGL(k_wcheck_tail, dim3(1), dim3(64), 0, c->stream, (const double*)c->ctail, tprev, sweep, pos,
                       kparams(c), c->st);
}
// the pending column check reads Gpart: resolve it before a step that overwrites Gpart, or where no T-row step follows to carry it
void flush_wcheck(rri_ctx* c, int sweep, int pos) {
    if (c->pending_wcheck) wcheck_now(c, c->pending_wcheck_topic, sweep, pos);
    c->pending_wcheck = false;
}

// carry := Zpart/Gpart hold the partial sums of topic `carry_topic`.
void enqueue_prologue(rri_ctx* c, int t, int sweep) {
    flush_wcheck(c, sweep, t);
    LK::wcol<false, true>(c, t, t, sweep);                             // Gram row of w_t
    DISPATCH_RO(c, (L::template pass<false, true>(c, t, t)));         // w_t^T X
    c->carry_valid = true;
    c->carry_wfin = false;
    c->carry_topic = t;
}

void enqueue_T_half(rri_ctx* c, int sweep, int t, bool standalone) {
    // early-sums schedule: the row update that leaves T T[t,:]^T for the pass of this topic's W half.  (The k_trow_final of a lone
    // half step only takes the row checks here: without a projection it leaves the row as stored.)  What k_wfin left only
    // k_trow_early can take up: any other route starts from the prologue (the column check it owes is taken there first, from Gpart).
    const bool early = LK::early_ok(c);
    if (c->carry_wfin && !early) c->carry_valid = false;
    if (!c->carry_valid || c->carry_topic != t) enqueue_prologue(c, t, sweep);
    {
        TimedScope ts(c, 2);
        const int chk = c->pending_wcheck ? 1 : 0;
        if (early) {
            if (!c->carry_wfin) LK::reduce(c);      // the carry is k_wcol's or the prologue's
            LK::frozen_add(c, t, chk ? c->pending_wcheck_topic : -1);
            LK::trow_early(c, t, chk, c->pending_wcheck_topic, sweep);
            LK::trow_final_if_needed(c, t, sweep, standalone);
        } else if (LK::small(c) && !c->comm && !c->fzB && c->sw.trow_fused) {
            LK::trow_small(c, t, chk, c->pending_wcheck_topic, sweep, standalone);
        } else {
            // the one cross-row reduction of a topic step: [w_t^T X | slices of (w_t^T W, ||w_t||^2, sum W[:,t-1])];
            // row-sharded, the ranks all-reduce it here, on the stream, between the two kernels; frozen rows add
            // their share at the same place
            LK::reduce(c);
            comm_allreduce(c, c->red, c->LD + (i64)GRAM_SLICES * (c->k + 2));
            LK::frozen_add(c, t, chk ? c->pending_wcheck_topic : -1);
            LK::trow(c, t, chk, c->pending_wcheck_topic, sweep, standalone);
        }
        c->pending_wcheck = false;
        if (c->prm.fix_W && no_regs(c)) LK::scale_wcol(c, t);
    }
    changed(c, CH_T_ROW);
    if (early) { c->early_valid = true; c->early_topic = t; }
}

void enqueue_W_half(rri_ctx* c, int sweep, int t) {
    const int k = c->k;
    const bool carry_next = (k > 1) && !c->prm.fix_T;
    const int tn = (t + 1) % k;
    // T T[t,:]^T for k_wcol; the T-row checks ride along only when a T half of this topic just ran and left its sums.
    // Where a pass follows, the job joins its grid (no launch of its own); with T fixed there is no pass.
    const int finish = (LK::light(c) && !c->prm.fix_T && !c->skip_row_finish) ? 1 : 0;
    c->skip_row_finish = false;
    TgramJob job{};
    if (c->prm.fix_T || c->sparse_x) {
        TimedScope ts(c, 2);
        LK::tgram(c, t, finish, sweep);
    } else {
        job = TgramJob{(const double*)c->T, c->LD, (int)c->d, c->k, t, c->Ttpart, (const double*)c->tpart, c->tpart_n,
                       c->nsplit, finish, sweep, kparams(c), c->st, c->k * c->nsplit};
        c->ttpart_n = c->nsplit;
    }
    // early-sums schedule: the T half of this topic has just left T T[t,:]^T (nothing touched the handle since), so the W-sized
    // sums of k_wcol ride in the pass's grid and one launch, k_wfin, finishes the column and reduces the carry.  Any step whose
    // early partials are not there -- a lone half step, the first after rri_set_*, a reset, a resume -- runs k_wcol.
    const bool early = carry_next && LK::early_ok(c) && c->early_valid && c->early_topic == t;
    if (carry_next) {
        DISPATCH_RO(c, (L::template pass<true, true>(c, t, tn, job, early ? LK::early_job(c, t, tn) : EarlyJob{})));
        if (early) LK::wfin(c, t, tn, sweep);
        else LK::wcol<true, true>(c, t, tn, sweep);
        c->carry_valid = true;
        c->carry_topic = tn;
        c->pending_wcheck = true;
        c->pending_wcheck_topic = t;
    } else {
        if (c->prm.fix_T) {
            // T is fixed: X T^T is computed once (k_xtt) and reused by every topic and every sweep
            if (!c->q_valid) {
                DISPATCH_RO(c, L::xtt(c));
                c->q_valid = true;
            }
            LK::wcol_src<true, false>(c, t, tn, sweep, c->Qt + (i64)t * c->ldw, 1);
        } else {
            DISPATCH_RO(c, (L::template pass<true, false>(c, t, tn, job)));
            LK::wcol<true, false>(c, t, tn, sweep);
        }
        const StepPos next = next_step(sweep, t, k);
        wcheck_now(c, t, next.sweep, next.pos);
        c->carry_valid = false;
    }
    changed(c, CH_W_COL);
    c->carry_wfin = early;
    c->wfin_topic = t;
}

// ---- explicit-residual schedule (RRI_UNWEIGHTED_RESIDUAL; SURVEY 8a "explicit-residual variant") --------------
// R = X - W T is kept in HBM (c->E) and every topic step is ONE read-modify-write pass over it:
//     pass of step t   R <- R - dw_{t-1} t_{t-1}^T - w_t dt_t^T   (the two rank-one terms pending since the W half of
//                      step t-1 and the T half of step t), fused with  y = R t_t  and  z = R^T w_{t+1}  of the new R
//     W half           numer_W = y + w_t ||t_t||^2 ;  dw_t = w_t' - w_t stays pending
//     T half (t+1)     numer_T = z - t_t <dw_t, w_{t+1}> + t_{t+1} ||w_{t+1}||^2   (column t+1 of W is untouched by
//                      step t, so z needs only the rank-one correction for the term that is still pending)
// 2 n d s bytes per topic step.  R is rebuilt from X, W, T (the k-panel GEMM k_resid_mfma) once per sweep, so the
// rounding of the stored residual never accumulates over more than k updates.  carry := Zpart / Gpart hold z and
// the correction coefficients for topic `carry_topic`.
void r_refresh(rri_ctx* c) {
    DISPATCH(c, L::resid(c, false, true, nullptr, nullptr));   // R = X - W T
    resid_rebuilt(c);
}

void enqueue_rT_half(rri_ctx* c, int sweep, int t, bool standalone) {
    if (!c->resid_valid) r_refresh(c);
    if (!c->carry_valid || c->carry_topic != t) {
        flush_wcheck(c, sweep, t);
        if (c->dw_pending) r_refresh(c);    // no pass to fold the pending column change into: rebuild instead
        LK::wcol_resid<false>(c, t, t, sweep);             // ||w_t||^2
        DISPATCH(c, L::rpass_colsums(c, t));               // R^T w_t
        c->carry_valid = true;
        c->carry_topic = t;
    }
    {
        TimedScope ts(c, 2);
        const int chk = c->pending_wcheck ? 1 : 0;
        if (LK::small(c) && !c->comm) {
            LK::trow_small(c, t, chk, c->pending_wcheck_topic, sweep, standalone);
        } else {
            // row-sharded: every rank holds its rows of R; the column sums R^T w_t, <dw, w_t>, ||w_t||^2 and the column
            // sum of the last update are sums over rows, all-reduced in one message as in the Gram form
            LK::reduce(c);
            comm_allreduce(c, c->red, c->LD + (i64)GRAM_SLICES * (c->k + 2));
            LK::trow(c, t, chk, c->pending_wcheck_topic, sweep, standalone);
        }
        c->pending_wcheck = false;
    }
    changed(c, CH_T_ROW | CH_E_FOLLOWS);
    c->resid_fresh = false;
    c->dt_pending = true;     // told holds the previous row: R lacks w_t (T[t,:] - told)^T
}

void enqueue_rW_half(rri_ctx* c, int sweep, int t) {
    const int k = c->k;
    const int tn = (t + 1) % k;
    if (!c->resid_valid) r_refresh(c);
    const int finish = (LK::light(c) && !c->skip_row_finish) ? 1 : 0;
    c->skip_row_finish = false;
    const TgramJob job{(const double*)c->T, c->LD, (int)c->d, c->k, t, c->Ttpart, (const double*)c->tpart, c->tpart_n,
                       c->nsplit, finish, sweep, kparams(c), c->st, c->k * c->nsplit};
    c->ttpart_n = c->nsplit;
    const double* trow = c->T + (i64)t * c->LD;
    DISPATCH(c, {
        typename L::Upd u;
        u.a = c->dw_pending ? c->dwv : c->zeros;
        u.b = c->T + (i64)(c->dw_pending ? c->dw_topic : t) * c->LD;
        u.a2 = c->W + (i64)t * c->ldw;               // the column BEFORE its update below
        u.b2 = trow;
        u.b2sub = c->dt_pending ? c->told : trow;    // no T half since the last pass: dt = 0
        L::rank_update(c, c->E, c->LD, u, trow, c->W + (i64)tn * c->ldw, job);
    });
    LK::wcol_resid<true>(c, t, tn, sweep);
    changed(c, CH_W_COL | CH_E_FOLLOWS);
    c->dw_pending = true;
    c->dw_topic = t;
    c->dt_pending = false;
    c->resid_fresh = false;
    c->carry_valid = true;
    c->carry_topic = tn;
    c->pending_wcheck = true;
    c->pending_wcheck_topic = t;
}

// ---- weighted flavour (rri_wrri_kernels.hpp) ---------------------------------------------------------
// carry := Zpart / Z2part hold the column sums (a, nw) of topic `carry_topic` over the CURRENT E.
void w_refresh(rri_ctx* c) {
    DISPATCH(c, L::resid(c, true, true, nullptr, nullptr));   // E = M .* (X - W T)
    resid_rebuilt(c);          // (pattern-only handles: the row copy's pending column change is in it too)
    c->carry_valid = false;
}

// take_check: the pending column verdict of the last W update rides in this launch (one device, rri_sweep's own loop)
void w_reduce(rri_ctx* c, bool take_check = false, int sweep = 0, int pos = 0) {
    const int nb = (int)((c->LD + 63) / 64);
    const int chk = (take_check && c->pending_wcheck) ? 1 : 0;
    const bool nwm = c->nw_mask;     // (set by enqueue_wT_sums: the T-row step's nw lies in N2part, k_wmcorr_cols' row blocks)
    hipLaunchKernelGGL(k_wreduce, dim3(nb), dim3(1024), 0, c->stream, (const double*)c->Zpart,
                       (const double*)(nwm ? c->N2part : c->Z2part), c->LD, c->nrb, nwm ? c->wcorr_nrb : c->nrb, c->wcorr ? (const double*)c->Cpart : (const double*)nullptr, c->wcorr_nrb,
                       (const double*)(c->T + (i64)c->wcorr_topic * c->LD), c->red, (const double*)c->Gpart, c->nwb256, c->k, chk,
                       c->pending_wcheck_topic, sweep, pos, kparams(c), c->st);
    if (chk) c->pending_wcheck = false;
}

// few row blocks of partial column sums, one device: the column verdict, both reductions and the closed form of the T row are
// ONE launch (k_wtrow_small)
bool wtrow_small(const rri_ctx* c) { return rri::wtrow_small(c->comm != nullptr, c->nrb); }

// column sums (a, nw) of topic t over the current E into red[0 .. 2 LD)
// `fused`: the caller goes straight on to enqueue_wT_solve(..., fused) -- rri_sweep does; the split stepping of
// rri_topic_reduce_local / rri_topic_finish, where the host reads (and may rewrite) red in between, does not
void enqueue_wT_sums(rri_ctx* c, int t, bool fused = false, bool take_check = false, int sweep = 0) {
    const double* wt_t = c->W + (i64)t * c->ldw;
    if (!c->carry_valid || c->carry_topic != t)
        DISPATCH(c, (L::template wpass<false, true, false, false>(c, nullptr, wt_t, c->zeros, c->zeros, nullptr, nullptr)));
    // dense handles: E -- and with it these sums, carried or just taken -- lacks the rank-one term of the last W update
    // (dw T[dw_topic,:]^T under the mask; the next pass folds it in).  Its share of the sums comes from the mask alone.
    c->wcorr = !c->sparse && c->dw_pending;
    c->nw_mask = false;
    DISPATCH(c, c->nw_mask = L::nw_from_mask(c));      // sparse 0/1 mask: nw from the same mask-only launch (the passes skipped it)
    if (c->wcorr || c->nw_mask) {
        if (c->wcorr) c->wcorr_topic = c->dw_topic;
        DISPATCH(c, L::wmcorr(c, wt_t, c->wcorr ? c->dwv : nullptr));
    }
    if (fused) return;       // reduced inside k_wtrow_small
    TimedScope ts(c, 2);
    w_reduce(c, take_check, sweep, t);
}

// T row from red (local sums, or all-reduced ones on the row-sharded path)
void enqueue_wT_solve(rri_ctx* c, int sweep, int t, bool fused = false) {
    const double* wt_t = c->W + (i64)t * c->ldw;
    {
        TimedScope ts(c, 2);
        const int nb_small = (int)((c->LD + 127) / 128);
        if (fused) {
            const int nb = nb_small;
            hipLaunchKernelGGL(k_wtrow_small, dim3(nb), dim3(128), 0, c->stream, (const double*)c->T, c->LD, (int)c->d, t,
                               (const double*)c->Zpart, (const double*)(c->nw_mask ? c->N2part : c->Z2part), c->LD, c->nrb,
                               c->nw_mask ? c->wcorr_nrb : c->nrb, c->wcorr ? (const double*)c->Cpart : (const double*)nullptr, c->wcorr_nrb,
                               (const double*)(c->T + (i64)c->wcorr_topic * c->LD), (const double*)c->Gpart,
                               c->nwb256, c->k, c->pending_wcheck ? 1 : 0, c->pending_wcheck_topic, sweep, c->red, c->xraw,
                               c->tpart, c->tpart_idx, kparams(c), c->st);
            c->pending_wcheck = false;
        } else
        hipLaunchKernelGGL(k_wtrow, dim3(c->ntb), dim3(128), 0, c->stream, (const double*)c->T, c->LD, (int)c->d, t,
                           (const double*)c->red, c->LD, c->xraw, c->tpart, c->tpart_idx, kparams(c),
                           (const DevState*)c->st);
        const int scale_w = (c->prm.fix_W && no_regs(c)) ? 1 : 0;
        hipLaunchKernelGGL(k_wtrow_final, dim3(1), dim3(1024), 0, c->stream, c->T, c->LD, (int)c->d, t, c->xraw,
                           (const double*)c->tpart, (const i64*)c->tpart_idx, fused ? nb_small : c->ntb, c->dtv, scale_w, sweep,
                           kparams(c), c->st);
    }
    // a column change still pending on the row copy and no W half to fold it: rebuild
    const bool rebuild = c->prm.fix_W && c->dw_pending;
    changed(c, rebuild ? CH_T_ROW : CH_T_ROW | CH_E_FOLLOWS);
    c->resid_fresh = false;
    c->dt_pending = !rebuild;
    if (rebuild) {
        if (no_regs(c)) LK::scale_wcol(c, t);
    } else if (c->prm.fix_W) {   // no W half follows: fold dt into E now, then rescale the kept column (nmf.py:450-452)
        DISPATCH(c, (L::template wpass<false, false, false, true>(c, nullptr, nullptr, wt_t, c->dtv, nullptr, nullptr)));
        c->dt_pending = false;
        if (no_regs(c)) LK::scale_wcol(c, t);
    }
}

void enqueue_wT_half(rri_ctx* c, int sweep, int t) {
    const bool fused = wtrow_small(c);
    enqueue_wT_sums(c, t, fused, /*take_check=*/!c->comm, sweep);
    if (c->comm) {
        // row-sharded: red = [numerator | denominator | sum of the last updated column, its negative-denominator flag]
        // is all-reduced; the pending column verdict is taken from the reduced tail (option A)
        double* tail = c->red + 2 * c->LD;
        if (c->pending_wcheck)
            hipLaunchKernelGGL(k_wcheck_wcol, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, c->nwb256, c->k,
                               c->pending_wcheck_topic, sweep, t, kparams(c), c->st, tail);
        else
            (void)hipMemsetAsync(tail, 0, 2 * sizeof(double), c->stream);
        comm_allreduce(c, c->red, 2 * c->LD + 2);
        if (c->pending_wcheck)
            hipLaunchKernelGGL(k_wcheck_tail, dim3(1), dim3(64), 0, c->stream, (const double*)tail, c->pending_wcheck_topic,
                               sweep, t, kparams(c), c->st);
        c->pending_wcheck = false;
    }
    enqueue_wT_solve(c, sweep, t, fused);
}

void enqueue_wW_half(rri_ctx* c, int sweep, int t, bool defer_check = false) {
    const int k = c->k;
    const int tn = (t + 1) % k;
    const double* trow = c->T + (i64)t * c->LD;
    // pending T-row correction: none when T is fixed, or when E was rebuilt after the row changed (reset + resume)
    const double* b1 = (c->prm.fix_T || !c->dt_pending) ? c->zeros : c->dtv;
    c->dt_pending = false;
    c->resid_fresh = false;
    const bool sp_merged = c->sparse;
    if (sp_merged) {
        // Pattern-only handles keep two copies of the residual, and each copy serves ONE kind of sum: rows -> row
        // products, columns -> column sums.  So the row copy need not be current between its own passes: the W-column
        // change of a topic step (dw t^T) is folded into it by the row pass of the NEXT step, together with that step's
        // T-row change -- ONE read-modify-write pass per copy and topic step (20 B per observed entry) where the
        // schedule shared with the dense flavour takes a read pass and a read-modify-write pass over the row copy
        // (26 B).  The copies then differ by storage roundings only (each term is still applied exactly once to each).
        const double* a2 = c->dw_pending ? c->dwv : c->zeros;          // dw of the previous step: k_wwcol below overwrites it
        const double* b2 = c->T + (i64)(c->dw_pending ? c->dw_topic : t) * c->LD;
        TimedScope ts(c, 3);
        DISPATCH(c, (L::template sp_blk<true, true, true>(c, 0, b1, b2, trow, c->W + (i64)t * c->ldw, a2, c->Ypart, c->Y2part, c->n)));
    } else {
        // Dense handles: ONE read-modify-write pass per topic step (rri_wrri_kernels.hpp, "one read-modify-write pass").  It folds
        // the W-column change of the step before (still pending) and this step's T-row change into E, writes E, and takes the
        // row products of this W update AND the column sums of the next T row; what those lack -- the term the update below
        // leaves pending -- the next T-row step takes from the mask alone (enqueue_wT_sums).  Nothing pending (T fixed, first
        // step after a rebuild): the pass only reads.
        const bool pend_w = c->dw_pending;
        const double* a2 = pend_w ? c->dwv : c->zeros;                 // k_wwcol below overwrites dwv after the pass has read it
        const double* b2 = c->T + (i64)(pend_w ? c->dw_topic : t) * c->LD;
        const double* wt_t = c->W + (i64)t * c->ldw;
        const double* wnx = c->W + (i64)tn * c->ldw;
        const bool cn = (k > 1) && !c->prm.fix_T;
        const bool pend = pend_w || b1 != c->zeros;
        pick_bool(cn, [&](auto CN) {
            pick_bool(pend, [&](auto PEND) {
                DISPATCH(c, (L::template wpass<true, CN, PEND, PEND>(c, trow, CN ? wnx : nullptr, PEND ? wt_t : c->zeros, PEND ? b1 : c->zeros,
                                                                     PEND ? a2 : nullptr, PEND ? b2 : nullptr)));
            });
        });
    }
    {
        TimedScope ts(c, 1);
        hipLaunchKernelGGL(k_wwcol, dim3(c->nwb256), dim3(256), 0, c->stream, c->W, c->ldw, (int)c->n, k, t,
                           (const double*)c->Ypart, (const double*)c->Y2part, c->npanels, c->wold, c->dwv, c->Gpart,
                           kparams(c), (const DevState*)c->st);
    }
    const bool carry_next = (k > 1) && !c->prm.fix_T;
    const double* wn = c->W + (i64)tn * c->ldw;
    if (sp_merged) {
        TimedScope ts(c, 3);          // the column copy: both terms of this step, the column sums of the next topic
        pick_bool(carry_next, [&](auto CN) {
            DISPATCH(c, (L::template sp_blk<CN, true, true>(c, 1, c->wold, c->dwv, wn, b1, trow, c->Zpart, c->Z2part, c->LD)));
        });
    }
    changed(c, CH_W_COL | CH_E_FOLLOWS);
    c->dw_pending = true;     // dwv x T[t,:]: folded in by the pass of the next step (dense: into E, under the mask; pattern-only: the row copy)
    c->dw_topic = t;
    const StepPos next = next_step(sweep, t, k);
    if (defer_check) {   // row-sharded: the verdict needs the global column sum; it rides on the next topic's all-reduce
        c->pending_wcheck = true;
        c->pending_wcheck_topic = t;
    } else {
        wcheck_now(c, t, next.sweep, next.pos);
    }
    c->carry_valid = carry_next;
    c->carry_topic = tn;
}

// ---- which XCD gets which tile: the two speeds of the read-modify-write passes -------------------------------------------------
// The pass over a handle's stored residual runs at one of two speeds -- 1.35 against 1.50-1.57 ms for the rank-one update of
// BASELINE config 3, 1.39-1.41 against 1.55 ms for the weighted one-pass step -- and rounds 2-4 could only report which one a
// process had caught.  What decides it is which XCD is dealt which tile: the workgroups of a launch go round-robin over the 8
// XCDs, and rotating the tiles by ONE inside every group of 8 workgroups flips the speed -- every odd rotation fast and every
// even one slow, or the other way round in another process (tools/xcc_mode_probe.py, profiles/r04_xcc_mode_probe.log: the
// buffer's placement against the memory side's interleave, one would think; nothing a process can read).  So a handle that
// keeps a residual TIMES both before its first sweep: per rotation three null updates (a = 0: the residual is rewritten with
// its own values, bit for bit), the last two timed -- ~10 ms once per handle -- and keeps the faster.  The rotation changes
// which workgroup computes a tile and nothing in any sum: the results are the same bits whichever wins.
// (The read-only pass over X differs by ~1 % between the two: calibrated the same way, on X, for handles of the Gram form.)
void calibrate_rot(rri_ctx* c) {
    if (c->rot_done) return;
    c->rot_done = true;
    if (c->sw.pass_rot >= 0 || !c->sw.rot_cal) return;
    const bool resid = resid_sched(c);
    const bool wdense = c->weighted && !c->sparse;
    const bool plain = !c->weighted && !resid && !c->sparse && !c->prm.fix_T;      // the Gram form: the read-only pass over X
    if (!(resid || wdense || plain) || (double)c->n * (double)c->d < 1.0e8 || c->npanels * c->nrb < 64) return;
    EventPair ev;
    if (ev.create() != hipSuccess) { (void)hipGetLastError(); return; }
    // the better of the rotations 0 .. nrot-1 of `rot` by what `pass` takes: two warm passes at rotation 0 (the first passes of a
    // process run ~5 % slow: not the rotation's doing), then three per rotation, the last two timed; the first of equal times wins;
    // a launch or a wait that fails: rotation 0.  The passes leave their own row products and column sums in the scratch arrays
    auto pick = [&](int& rot, int nrot, const char* what, auto&& pass) {
        float best = -1.0f;
        int best_rot = 0;
        rot = 0;
        for (int rep = 0; rep < 2; ++rep) pass();
        for (rot = 0; rot < nrot; ++rot) {
            for (int rep = 0; rep < 3; ++rep) {
                if (rep == 1) (void)hipEventRecord(ev.a, c->stream);
                pass();
            }
            (void)hipEventRecord(ev.b, c->stream);
            float ms = 0.0f;
            if (hipEventSynchronize(ev.b) != hipSuccess || hipEventElapsedTime(&ms, ev.a, ev.b) != hipSuccess) { best = -1.0f; break; }
            if (c->sw.rot_debug) fprintf(stderr, "rri: tile rotation %d: %.4f ms per %s\n", rot, ms / 2.0f, what);
            if (best < 0.0f || ms < best) { best = ms; best_rot = rot; }
        }
        rot = best > 0.0f ? best_rot : 0;
        c->carry_valid = false;
        c->carry_topic = -1;
    };
    if (plain) {
        // the read-only pass moves by ~1 % with the rotation (0.643 against 0.650 ms at BASELINE config 3, the same way in every
        // round of three processes): the same calibration on X, 8 passes once per handle
        pick(c->rot_x, 2, "read-only pass", [&]() { DISPATCH_RO(c, (L::template pass<true, true>(c, 0, 0))); });
        return;
    }
    if (!c->resid_valid) {
        if (resid) r_refresh(c);
        else w_refresh(c);
    }
    auto null_update = [&]() {
        if (resid) {
            DISPATCH(c, {
                typename L::Upd u;
                u.a = c->zeros; u.b = c->zeros; u.a2 = c->zeros; u.b2 = c->zeros; u.b2sub = c->zeros;
                L::rank_update(c, c->E, c->LD, u, c->T, c->W);
            });
        } else {
            DISPATCH(c, (L::template wpass<true, true, true, true>(c, c->T, c->W, c->zeros, c->zeros, c->zeros, c->zeros)));
        }
    };
    // The level under the parity belongs to the BUFFER, not to the process (six residuals alive in one process: one at 1.34 ms,
    // one at 1.42, four at 1.50-1.53 whatever the rotation; physically contiguous memory: always 1.54 --
    // profiles/r04_rmw_buffer_probe.log).  Trying a large residual in several places until one ran fast found none in 40 places
    // (10 processes) on a box whose buffers were slow: the first allocation is kept.
    // rotations 0 and 1 (or 0 .. RRI_ROT_CAL-1), by null updates
    pick(c->rot_r, c->sw.rot_cal > 1 ? std::min(c->sw.rot_cal, 8) : 2, "null update", null_update);
}

// ---- T fixed: the W half of all topics of a sweep as one launch (k_wsweep_rows) ---------------------------------------
// k <= 256: k_wsweep_verdict keeps one column sum per topic in ssum[256].  The LDS bound is the tighter one today (k <= 109);
// the explicit term keeps the verdict's array safe if that bound ever moves.
// ... or, on a pattern-only handle that asked for it (rri_set_fold_schedule), k_wfold_rows: q and G per row from the row's own
// observed entries (wfold_ok of rri_fold.hpp)
bool wfold_sched(const rri_ctx* c) {
    return wfold_ok(c->fold_asked, c->weighted != 0, c->sparse, c->sparse_x, c->prm.fix_T != 0, c->prm.fix_W != 0, c->comm != nullptr, c->k);
}
bool wsweep_ok(const rri_ctx* c) {
    if (wfold_sched(c)) return true;
    return c->sw.wsweep && c->prm.fix_T && !c->prm.fix_W && !c->weighted && (!c->sparse || c->sparse_x) && c->k >= 1 &&
           c->k <= 256 && wsweep_lds_bytes(c->k) <= 150 * 1024;
}
// The launches of the fold sweep: sp_Tt once per T, k_wfold_rows, the verdicts in topic order, the repair.  What the launch
// leaves behind is announced by its caller, enqueue_wsweep.  false: a buffer or the LDS opt-in could not be had
bool launch_wfold(rri_ctx* c, int sweep, int t0) {
    const int k = c->k;
    const size_t f8 = sizeof(double);
    const int nwg = (int)((c->n + FOLD_ROWS - 1) / FOLD_ROWS);
    if (dev_ensure(c, c->Wsweep0, (size_t)k * c->ldw * f8) != hipSuccess || dev_ensure(c, c->fold_part, (size_t)2 * k * nwg * f8) != hipSuccess)
        return false;
    flush_wcheck(c, sweep, t0);     // (a column check left by steps before T was fixed)
    if (!c->tt_valid) {          // T transposed: once per T, reused by every sweep
        const i64 total = (i64)k * c->d;
        hipLaunchKernelGGL((k_convert2d<double, double, true>), dim3((unsigned)std::min<i64>(4096, (total + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)c->T, c->LD, c->sp_Tt, (i64)c->kp, (i64)k, c->d);
        c->tt_valid = true;
    }
    TimedScope ts(c, 1);
    bool ok = false;
    DISPATCH(c, ok = L::wfold(c, t0, nwg));
    if (!ok) return false;
    hipLaunchKernelGGL(k_wfold_verdict, dim3(1), dim3(1024), 0, c->stream, (const double*)c->fold_part,
                       (const double*)(c->fold_part + (size_t)k * nwg), nwg, k, t0, sweep, kparams(c), c->st);
    hipLaunchKernelGGL(k_wsweep_repair, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->W, (const double*)c->Wsweep0,
                       c->ldw, (int)c->n, k, (const DevState*)c->st);
    c->fold_launches += 1;
    return true;
}
// k_wsweep_rows leaves one column-sum partial and one cross-term partial per 64 rows (c->nwb of them), the count that
// note_xy(c, t, nwb * WCOL_TILES) and k_wsweep_verdict read back: that holds only with one 64-row tile per k_wcol block
static_assert(WCOL_TILES == 1, "enqueue_wsweep assumes one 64-row tile per k_wcol block");
// topics [t0, k) of sweep `sweep`; false: a buffer could not be had (the caller takes the launch-per-topic schedule)
bool enqueue_wsweep(rri_ctx* c, int sweep, int t0) {
    const int k = c->k;
    const size_t f8 = sizeof(double);
    if (wfold_sched(c)) {
        // a pattern-only handle: W changed and neither copy of the stored residual followed it, so the next objective or free
        // sweep rebuilds E (w_refresh); no carry, no column verdict owed
        if (!launch_wfold(c, sweep, t0)) return false;
        c->skip_row_finish = false;
        c->carry_valid = false;
        changed(c, CH_W_COL);
        return true;
    }
    if (dev_ensure(c, c->Gfull, (size_t)k * k * f8) != hipSuccess || dev_ensure(c, c->Wsweep0, (size_t)k * c->ldw * f8) != hipSuccess ||
        dev_ensure(c, c->wsum_part, (size_t)k * c->nwb * f8) != hipSuccess || dev_ensure(c, c->wsums, (size_t)k * f8) != hipSuccess)
        return false;
    if (allow_lds<k_wsweep_rows>(c, 152 * 1024) != hipSuccess) return false;
    flush_wcheck(c, sweep, t0);     // (a column check left by steps before T was fixed)
    if (!c->q_valid) {           // X T^T: once per T, reused by every topic and every sweep
        DISPATCH_RO(c, L::xtt(c));
        c->q_valid = true;
    }
    if (!c->gfull_valid) {
        hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->T, c->LD, c->d, k, c->Gfull);
        c->gfull_valid = true;
    }
    {
        TimedScope ts(c, 1);
        hipLaunchKernelGGL(k_wsweep_rows, dim3(c->nwb), dim3(64), wsweep_lds_bytes(k), c->stream, c->W, c->Wsweep0, c->ldw, (int)c->n, k,
                           t0, (const double*)c->Qt, (const double*)c->Gfull, c->wsum_part, c->nwb, c->XYpart, (i64)c->xy_stride,
                           kparams(c), (const DevState*)c->st);
        if (!c->comm)
            hipLaunchKernelGGL(k_wsweep_verdict, dim3(1), dim3(1024), 0, c->stream, (const double*)c->wsum_part, c->nwb, c->wsums,
                               (const double*)c->Gfull, k, t0, sweep, 3, kparams(c), c->st);
        else {      // row-sharded: the column sums of all k topics in ONE all-reduce (the launch-per-topic schedule takes k)
            hipLaunchKernelGGL(k_wsweep_verdict, dim3(1), dim3(1024), 0, c->stream, (const double*)c->wsum_part, c->nwb, c->wsums,
                               (const double*)c->Gfull, k, t0, sweep, 1, kparams(c), c->st);
            comm_allreduce(c, c->wsums, k);
            hipLaunchKernelGGL(k_wsweep_verdict, dim3(1), dim3(1024), 0, c->stream, (const double*)c->wsum_part, c->nwb, c->wsums,
                               (const double*)c->Gfull, k, t0, sweep, 2, kparams(c), c->st);
        }
        hipLaunchKernelGGL(k_wsweep_repair, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, c->W, (const double*)c->Wsweep0,
                           c->ldw, (int)c->n, k, (const DevState*)c->st);
    }
    for (int t = t0; t < k; ++t) LK::note_xy(c, t, c->nwb * WCOL_TILES);
    c->skip_row_finish = false;
    c->carry_valid = false;
    changed(c, CH_W_COL);
    return true;
}

// ---- the packed copy of an fp32 X (rri_xpack.hpp) ---------------------------------------------------------------------
// The read-only pass is at the HBM read ceiling and X never changes between sweeps, so the handle keeps a lossless copy of
// 3.5 bytes per element and the pass streams that.  Built lazily by the first sweep that would read it, for dense fp32 handles
// of the Gram form on the launch-per-phase schedule, plain or row-sharded; by default only where X does not fit the budget of
// pass_keep (a cached X gains nothing from fewer bytes).  Two kernels: the largest top byte (the window's base must be final
// before anything is encoded), then the encoder, which sets the flag byte of every tile that holds an element outside the
// window.  The host reads the flags once: with more than 1/8 of the tiles flagged the copy is released and the handle runs
// as it did before.  An allocation that fails means no copy, and no error.
// how the read-only pass loads X (rri_ctx::keep_q): the rule and its reasons are pass_keep of rri_layout.hpp
int pass_keep(const rri_ctx* c) { return rri::pass_keep(c->plan, c->k, c->ldw, c->es, c->xp_valid, c->sw.pass_cache_mb); }
void xnarrow_release(rri_ctx* c) {
    dev_release(c, c->xn); dev_release(c, c->xn_dir); dev_release(c, c->xn_exc);
    c->xn_valid = false;
}
void xpack_release(rri_ctx* c) {
    xnarrow_release(c);
    dev_release(c, c->xp); dev_release(c, c->xp_flags); dev_release(c, c->xp_hmax);
    c->xp_valid = false;
    c->xp_flagged = c->xp_tiles = 0;
    c->xp_base = 0;
    c->keep_q = pass_keep(c);
}
// The 26-bit copy (rri_xnarrow.hpp): RRI_X_PACK=2 wherever the 28-bit copy would be built under =1; with the switch unset where
// the 28-bit copy would be built and the elements of the window outside the 7-entry book are at most 1/16 of X (each costs 16
// bits, so at 1/16 the entries eat half of the two bits saved).  Three kernels, each a read of X: the histogram of the exponent
// byte with the window's top byte; the tile flags with the entry count of every record; the encoder.  The host picks the books
// (256 counts), applies the 1/8 rule of the flags and sums the counts into the directory.
// Returns 1: built (xp_valid, xn_valid);  0: not built, the caller builds the 28-bit copy (not wanted for this X, no memory, too
// many entries for 32-bit offsets);  -1: too many flagged tiles, no copy of either kind (everything released, the counts recorded).
int xnarrow_build(rri_ctx* c, i64 nitems, int ncols, unsigned grid) {
    const i64 nrec = nitems * 4;
    xnarrow_release(c);
    dev_release(c, c->xp);
    c->xn_exceptions = -1;
    DevTmp hist, cls, counts;
    if (dev_ensure(c, c->xp_flags, (size_t)nitems) != hipSuccess || dev_ensure(c, c->xp_hmax, sizeof(unsigned)) != hipSuccess ||
        hist.alloc(256 * sizeof(unsigned long long)) != hipSuccess || cls.alloc(256) != hipSuccess ||
        counts.alloc((size_t)nrec * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return 0; }
    unsigned hmax = 0;
    uint64_t h[256];
    (void)hipMemsetAsync(c->xp_hmax, 0, sizeof(unsigned), c->stream);
    (void)hipMemsetAsync(c->xp_flags, 0, (size_t)nitems, c->stream);
    (void)hipMemsetAsync(hist.p, 0, sizeof(h), c->stream);
    hipLaunchKernelGGL(k_xnarrow_hist, dim3(grid), dim3(256), 0, c->stream, (const float*)c->X, c->ldx, (int)c->n, ncols, c->npanels, nitems,
                       c->xp_hmax, (unsigned long long*)hist.p);
    if (hipMemcpyAsync(h, hist.p, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(&hmax, c->xp_hmax, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const unsigned base = xpack::base_of(hmax);
    xnarrow::Books books;
    uint8_t klass[256];
    int nrare = 0;
    const uint64_t exceptions = xnarrow::choose_books(h, base, books, klass, nrare);
    c->xn_exceptions = (i64)exceptions;
    if (c->sw.x_pack < 0 && (double)exceptions * 16.0 > (double)c->n * (double)ncols) return 0;
    std::vector<unsigned char> flags((size_t)nitems);
    std::vector<unsigned> cnt((size_t)nrec), dir((size_t)nrec + 1);
    if (hipMemcpyAsync(cls.p, klass, 256, hipMemcpyHostToDevice, c->stream) != hipSuccess) { (void)hipGetLastError(); return 0; }
    hipLaunchKernelGGL(k_xnarrow_encode<false>, dim3(grid), dim3(256), 0, c->stream, (const float*)c->X, c->ldx, (int)c->n, ncols, c->npanels,
                       nitems, base, (const unsigned char*)cls.p, (unsigned char*)nullptr, c->xp_flags, (unsigned*)counts.p,
                       (const unsigned*)nullptr, (unsigned short*)nullptr);
    if (hipMemcpyAsync(flags.data(), c->xp_flags, (size_t)nitems, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(cnt.data(), counts.p, (size_t)nrec * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return 0; }
    i64 flagged = 0;
    for (unsigned char f : flags) flagged += f != 0;
    if (xpack_too_many_flagged(flagged, nitems)) { xpack_release(c); c->xp_flagged = flagged; c->xp_tiles = nitems; return -1; }
    if (!xnarrow::build_directory(cnt.data(), (uint64_t)nrec, dir.data())) return 0;
    const size_t nexc = dir[(size_t)nrec];
    if (dev_alloc(c, c->xn, (size_t)nrec * xnarrow::RECORD_BYTES) != hipSuccess ||
        dev_alloc(c, c->xn_dir, ((size_t)nrec + 1) * sizeof(unsigned)) != hipSuccess ||
        dev_alloc(c, c->xn_exc, std::max<size_t>(nexc, 1) * sizeof(unsigned short)) != hipSuccess) { xnarrow_release(c); return 0; }
    if (hipMemcpyAsync(c->xn_dir, dir.data(), ((size_t)nrec + 1) * sizeof(unsigned), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipGetLastError(); xnarrow_release(c); return 0;
    }
    hipLaunchKernelGGL(k_xnarrow_encode<true>, dim3(grid), dim3(256), 0, c->stream, (const float*)c->X, c->ldx, (int)c->n, ncols, c->npanels,
                       nitems, base, (const unsigned char*)cls.p, c->xn, c->xp_flags, (unsigned*)nullptr, (const unsigned*)c->xn_dir, c->xn_exc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); xnarrow_release(c); return 0; }   // dir, cls: host and temporary
    c->xn_books = books;
    c->xp_base = (int)base;
    c->xp_flagged = flagged;
    c->xp_tiles = nitems;
    c->xp_valid = c->xn_valid = true;
    // priced as the 28-bit copy (3.5 bytes per element; tests/test_layout_cpu.py restates that rule for a handle with a copy): a
    // few percent fewer kept row blocks than would fit, the same loads under every value of RRI_X_PACK that builds a copy
    c->keep_q = pass_keep(c);
    return 1;
}
void xpack_ensure(rri_ctx* c) {
    if (c->xp_done) return;
    // sweeps with T fixed run the whole-sweep W half and no pass: nothing is built for them and nothing is settled, so that the
    // first sweep after the parameters change decides (a copy that exists stays: xp_done is set then)
    if (wsweep_ok(c)) return;
    c->xp_done = true;
    c->xp_valid = false;
    c->keep_q = pass_keep(c);
    const bool reads_x = c->dtype == RRI_F32 && !c->weighted && !c->explicit_resid && !c->sparse && c->have_X;
    if (!reads_x || c->sw.x_pack == 0 || (c->sw.x_pack < 0 && c->keep_q < 0)) { xpack_release(c); return; }
    const i64 nitems = xpack_tiles(c->n, c->npanels, xpack::ROWS);
    c->xn_valid = false;
    if (c->sw.x_pack != 1) {
        const int built = xnarrow_build(c, nitems, (int)std::min<i64>(c->ldx, c->LD), (unsigned)std::min<i64>(nitems, 8192));
        if (built != 0) return;
    } else xnarrow_release(c);
    if (dev_ensure(c, c->xp, (size_t)nitems * 4 * xpack::RECORD_BYTES) != hipSuccess || dev_ensure(c, c->xp_flags, (size_t)nitems) != hipSuccess ||
        dev_ensure(c, c->xp_hmax, sizeof(unsigned)) != hipSuccess) { xpack_release(c); return; }
    const int ncols = (int)std::min<i64>(c->ldx, c->LD);     // what the fp32 row loop reads (pass_k)
    const unsigned grid = (unsigned)std::min<i64>(nitems, 8192);
    std::vector<unsigned char> flags((size_t)nitems);
    unsigned hmax = 0;
    (void)hipMemsetAsync(c->xp_hmax, 0, sizeof(unsigned), c->stream);
    (void)hipMemsetAsync(c->xp_flags, 0, (size_t)nitems, c->stream);
    hipLaunchKernelGGL(k_xpack_max, dim3(grid), dim3(256), 0, c->stream, (const float*)c->X, c->ldx, (int)c->n, ncols, c->npanels, nitems, c->xp_hmax);
    hipLaunchKernelGGL(k_xpack_encode, dim3(grid), dim3(256), 0, c->stream, (const float*)c->X, c->ldx, (int)c->n, ncols, c->npanels, nitems,
                       (const unsigned*)c->xp_hmax, c->xp, c->xp_flags);
    if (hipMemcpyAsync(flags.data(), c->xp_flags, (size_t)nitems, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(&hmax, c->xp_hmax, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); xpack_release(c); return; }
    i64 flagged = 0;
    for (unsigned char f : flags) flagged += f != 0;
    if (xpack_too_many_flagged(flagged, nitems)) { xpack_release(c); c->xp_flagged = flagged; c->xp_tiles = nitems; return; }
    c->xp_base = (int)xpack::base_of(hmax);
    c->xp_flagged = flagged;
    c->xp_tiles = nitems;
    c->xp_valid = true;
    c->keep_q = pass_keep(c);      // row blocks of 3.5 bytes per element: more of them fit
}

// sweeps [cur .. s_end) of the current call
void enqueue_range(rri_ctx* c, Cursor cur, int s_end) {
    const int k = c->k;
    if (cur.sweep < s_end) { xpack_ensure(c); calibrate_rot(c); }
    if (c->weighted) {
        for (int s = cur.sweep; s < s_end; ++s) {
            const int t0 = (s == cur.sweep) ? cur.topic : 0;
            const int sa = s;
            if (wsweep_ok(c) && enqueue_wsweep(c, sa, t0)) continue;      // pattern-only, T fixed, asked for: the W half of every topic in one launch
            if (c->fold_asked) c->fold_stepped += 1;
            for (int t = t0; t < k; ++t) {
                const int ph = (s == cur.sweep && t == cur.topic) ? cur.phase : 0;
                // once per sweep (and after resets), unless rri_objective has just rebuilt it from the same W, T
                if (!c->resid_valid || (t == 0 && ph == 0 && !c->resid_fresh)) w_refresh(c);
                if (!c->prm.fix_T && ph == 0) enqueue_wT_half(c, sa, t);
                // the column verdict rides on the next T-row step where that step can take it: row-sharded (the all-reduce), or one
                // device with few row blocks (k_wtrow_small)
                // (or k_wreduce: every T-row step of this loop can take it now)
                if (!c->prm.fix_W) enqueue_wW_half(c, sa, t, !c->prm.fix_T);
            }
        }
        return;
    }
    if (resid_sched(c)) {
        for (int s = cur.sweep; s < s_end; ++s) {
            const int t0 = (s == cur.sweep) ? cur.topic : 0;
            const int sa = s;
            for (int t = t0; t < k; ++t) {
                const int ph = (s == cur.sweep && t == cur.topic) ? cur.phase : 0;
                // rebuilt once per sweep (and after anything changed W or T from outside), unless rri_objective has
                // just stored it for the same W, T
                if (!c->resid_valid || (t == 0 && ph == 0 && !c->resid_fresh)) r_refresh(c);
                if (ph == 0) enqueue_rT_half(c, sa, t, false);
                enqueue_rW_half(c, sa, t);
            }
        }
        return;
    }
    for (int s = cur.sweep; s < s_end; ++s) {
        const int t0 = (s == cur.sweep) ? cur.topic : 0;
        const int sa = s;
        if (wsweep_ok(c) && enqueue_wsweep(c, sa, t0)) continue;      // T fixed: the W half of every topic in one launch
        for (int t = t0; t < k; ++t) {
            const int ph = (s == cur.sweep && t == cur.topic) ? cur.phase : 0;
            if (!c->prm.fix_T && ph == 0) enqueue_T_half(c, sa, t, c->prm.fix_W != 0);
            if (!c->prm.fix_W) enqueue_W_half(c, sa, t);
        }
    }
}

// ---- register-resident persistent sweeps (rri_onchip_kernels.hpp) ---------------------------------------------
// (OnchipGeom, onchip_rpw and the limits of the geometry: rri_layout.hpp)
bool onchip_geometry(const rri_ctx* c, OnchipGeom* g) {
    return rri::onchip_geometry(c->n, c->LD, c->k, c->dtype == RRI_F32, !LK::light(c), c->n_cu, g);
}
// A persistent launch that gave up means the device is shared with somebody whose grids collide with ours: every handle of the
// process keeps off the persistent path until this time (steady clock, ns), so that a process that makes a handle per nmf()
// call does not walk into the same wait again and again (tools/onchip_two_processes.py).
std::atomic<long long> g_onchip_backoff_until{0};
long long steady_now_ns() { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// what the persistent kernel covers: the unweighted flavour, either storage type, both halves free (with or without the per-step
// simplex projection of T), 2 <= k <= ONCHIP_MAX_K, on one device
bool onchip_ok(const rri_ctx* c) {
    OnchipGeom g;
    // a handle that fell back tries the persistent path again once its own back-off has run out (a burst on another stream or
    // process must not cost a long-lived handle the launch-bound speed-up for good); eligibility therefore depends on the clock
    if (c->onchip_off && steady_now_ns() < c->onchip_off_until) return false;
    if (ro_store(c->dtype)) return false;       // the persistent kernel has register layouts for 4- and 8-byte X only
    if (c->fzB) return false;                   // frozen rows enter through red, which the persistent kernel does not have
    return c->sw.onchip && steady_now_ns() >= g_onchip_backoff_until.load() && !c->weighted && !c->explicit_resid && !c->comm && !c->sparse &&
           !c->prm.fix_W && !c->prm.fix_T && c->ldx % c->VN == 0 && ((uintptr_t)c->X) % 16 == 0 &&
           onchip_shape_ok(c->n, c->LD, c->k, c->dtype == RRI_F32, !LK::light(c), c->n_cu, &g);
}
// Two persistent grids on one device (two handles on two streams) must not each hold a part of the CUs while waiting for
// the rest: inside a process EVERY persistent launch -- whatever its instantiation -- waits for the one before it on the same
// device (one mutex, one event per device, both at file scope: round 2 kept them inside the launch template, one set per
// instantiation, so an fp32 and a float64 handle were not ordered against each other).  Across processes nothing orders
// two grids; there the bounded polls end the wait and the call falls back (run_and_collect).
// hipLaunchCooperativeKernel is NOT used: it gives no stronger residency than a plain launch of a grid checked against the
// occupancy query (same admission, same queue), costs 15-19 us per launch, and a process that has used it dies in the HIP
// runtime's own exit handler under rocprofv3 ("the exit-time fault").
std::mutex g_onchip_mu;
hipEvent_t g_onchip_last[64] = {};
hipError_t onchip_ordered_launch(rri_ctx* c, const void* fn, int grid, size_t shmem, const OnchipArgs& a) {
    std::lock_guard<std::mutex> lock(g_onchip_mu);
    const int dv = c->device & 63;
    if (!g_onchip_last[dv] && hipEventCreateWithFlags(&g_onchip_last[dv], hipEventDisableTiming) != hipSuccess) g_onchip_last[dv] = nullptr;
    if (g_onchip_last[dv]) (void)hipStreamWaitEvent(c->stream, g_onchip_last[dv], 0);
    OnchipArgs copy = a;
    void* args[] = {(void*)&copy};
    hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(ONCHIP_THREADS), args, shmem, c->stream);
    if (le == hipSuccess) le = hipGetLastError();
    if (le == hipSuccess && g_onchip_last[dv]) (void)hipEventRecord(g_onchip_last[dv], c->stream);
    return le;
}
template <typename SX, int RPW, bool DBG, bool PROJ, int KT>
hipError_t onchip_launch(rri_ctx* c, const OnchipGeom& g, const OnchipArgs& a) {
    const void* fn = (const void*)k_onchip_sweeps<SX, RPW, DBG, PROJ, KT>;
    hipError_t e = allow_lds<k_onchip_sweeps<SX, RPW, DBG, PROJ, KT>>(c, 152 * 1024);
    if (e != hipSuccess) { if (getenv("RRI_ONCHIP_DEBUG")) fprintf(stderr, "rri: hipFuncSetAttribute\n"); return e; }
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_onchip_sweeps<SX, RPW, DBG, PROJ, KT>, ONCHIP_THREADS, g.shmem);
    if (getenv("RRI_ONCHIP_DEBUG")) fprintf(stderr, "rri: occupancy %d per CU (%s), %d CUs\n", per_cu, hipGetErrorString(e), c->n_cu);
    if (e != hipSuccess) return e;
    if ((i64)per_cu * c->n_cu < g.G) return hipErrorCooperativeLaunchTooLarge;     // the hand-overs need every workgroup resident
    return onchip_ordered_launch(c, fn, g.G, g.shmem, a);
}
// sweeps [cur .. run_total) in one launch; false: not launched (the caller takes the launch-per-phase schedule)
bool enqueue_onchip(rri_ctx* c, Cursor cur) {
    OnchipGeom g;
    if (!onchip_geometry(c, &g)) return false;
    const int k = c->k;
    if (!c->mkZ) {
        const bool all = dev_alloc(c, c->mkZ, (size_t)2 * g.G * c->LD * 8, true) == hipSuccess &&
                         dev_alloc(c, c->mkG, (size_t)2 * g.G * (k + 2) * 8, true) == hipSuccess &&
                         dev_alloc(c, c->mkP, (size_t)2 * 64 * (k + 1) * 8, true) == hipSuccess &&
                         dev_alloc(c, c->mkbar, (size_t)(128 + g.G) * sizeof(unsigned)) == hipSuccess &&
                         dev_alloc(c, c->mkX, (size_t)2 * c->LD * 8) == hipSuccess && dev_alloc(c, c->mkT, (size_t)2 * c->LD * 8) == hipSuccess &&
                         dev_alloc(c, c->objE, (size_t)ONCHIP_UNTIL_CAP * 256 * 8) == hipSuccess &&
                         dev_alloc(c, c->objhist, (size_t)ONCHIP_UNTIL_CAP * 8) == hipSuccess &&
                         dev_alloc(c, c->objdec, (size_t)ONCHIP_UNTIL_CAP * 8) == hipSuccess;
        if (!all) {     // all nine or none: the next call starts from mkZ again
            dev_release(c, c->mkZ); dev_release(c, c->mkG); dev_release(c, c->mkP); dev_release(c, c->mkbar); dev_release(c, c->mkX);
            dev_release(c, c->mkT); dev_release(c, c->objE); dev_release(c, c->objhist); dev_release(c, c->objdec);
            return false;
        }
    }
    if (dev_ensure(c, c->Wsafe, (size_t)k * c->ldw * 8) != hipSuccess || dev_ensure(c, c->Tsafe, (size_t)k * c->LD * 8) != hipSuccess) return false;
    (void)hipMemsetAsync(c->mkbar, 0, (size_t)(128 + g.G) * sizeof(unsigned), c->stream);
    OnchipArgs a{};
    a.X = c->X; a.ldx = c->ldx; a.n = (int)c->n; a.d = (int)c->d; a.LD = (int)c->LD; a.k = k;
    a.Wt = c->W; a.ldw = c->ldw; a.T = c->T; a.ldt = c->LD;
    a.mkZ = c->mkZ; a.mkG = c->mkG; a.mkP = c->mkP; a.mkX = c->mkX; a.mkT = c->mkT; a.objE = c->objE; a.xyp = c->XYpart; a.xy_stride = c->xy_stride; a.bar = c->mkbar;
    a.G = g.G; a.NA = g.NA; a.rows_wg = g.rows_wg; a.CG = g.CG; a.RG = g.RG; a.kS = g.kS;
    a.s0 = cur.sweep; a.t0 = cur.topic; a.ph0 = cur.phase; a.s_end = c->run_total;
    a.skip_row_finish = c->skip_row_finish ? 1 : 0;
    a.spin_limit = 2000000u;            // polls of ~1 us: a grid that stands still for seconds gives up (HALT_ERR_GRID_SYNC)
    a.entry_spin_limit = 40000u;        // the hand-over at kernel entry: a grid that is not resident as a whole shows within ~40 ms
    if (const char* e = getenv("RRI_ONCHIP_SPIN_LIMIT")) a.spin_limit = a.entry_spin_limit = (unsigned)std::max(0, atoi(e));   // tests: 0 = give up at once
    if (const char* e = getenv("RRI_ONCHIP_ENTRY_SPIN_LIMIT")) a.entry_spin_limit = (unsigned)std::max(0, atoi(e));
    a.jitter = 0u;
    if (const char* e = getenv("RRI_ONCHIP_JITTER")) a.jitter = (unsigned)strtoul(e, nullptr, 10);     // tests: seeded sleeps before every exchange store and first poll
    a.fail_step = -1;
    if (const char* e = getenv("RRI_ONCHIP_FAIL_STEP")) a.fail_step = atoi(e);       // tests: give up inside the run, at this topic step of the launch
    // the last sweep of the launch runs from its topic 0: its objective can be left behind (see eacc in the kernel)
    a.track = (c->sw.onchip_obj && (c->run_total - 1 > cur.sweep || (cur.topic == 0 && cur.phase == 0))) ? 1 : 0;
    if (c->until.active && cur.topic == 0 && cur.phase == 0 && c->run_total - cur.sweep <= ONCHIP_UNTIL_CAP && c->x_sq_valid) {
        a.track = 2;
        a.objhist = c->objhist; a.dec = c->objdec;
        a.obj_prev = c->until.prev; a.stop_scale = c->until.scale; a.half_xsq = 0.5 * c->x_sq;
        // "not written" = NaN: the sweeps of the call whose objective the kernel did not leave are told by that
        (void)hipMemsetAsync(c->objhist, 0xFF, (size_t)(c->run_total - cur.sweep) * 8, c->stream);
    }
    a.nap_eighths = 5;
    if (const char* e = getenv("RRI_ONCHIP_NAP_EIGHTHS")) a.nap_eighths = std::min(7, std::max(0, atoi(e)));      // diagnostics
    a.p = kparams(c); a.st = c->st;
    a.dbg = nullptr;
    if (getenv("RRI_ONCHIP_TIMING")) {           // diagnostics: per-section ticks of the last launch, printed at the next one
        static long long* dbg = nullptr;     // no handle's buffer: it lives as long as the process and is never freed
        if (!dbg && hipMalloc((void**)&dbg, 32 * sizeof(long long)) != hipSuccess) dbg = nullptr;
        if (dbg) {
            long long h[32];
            if (c->onchip_launches > 0 && hipMemcpy(h, dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
                static const char* names[14] = {"carries arrive", "A rest", "next carry + workers arrive", "mark absent", "row dots", "W update", "carry_post", "to next step",
                                                "closed form", "-", "slices arrive", "-", "project", "-"};
                for (int w = 0; w < 2; ++w) {
                    fprintf(stderr, "rri on-chip sections, workgroup %s (us total):", w == 0 ? "0 (worker)" : "G-1");
                    for (int i = 0; i < 13; ++i) fprintf(stderr, " %s %.1f;", names[i], h[16 * w + i] * 0.01);
                    fprintf(stderr, "\n");
                }
            }
            (void)hipMemsetAsync(dbg, 0, 32 * sizeof(long long), c->stream);
            a.dbg = dbg;
        }
    }
    // what a launch that gives up is rolled back to (0.9 MB at 10000 x 1000, k = 20: two copies of a few microseconds)
    (void)hipMemcpyAsync(c->Wsafe, c->W, (size_t)k * c->ldw * 8, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemcpyAsync(c->Tsafe, c->T, (size_t)k * c->LD * 8, hipMemcpyDeviceToDevice, c->stream);
    c->onchip_saved_skip = c->skip_row_finish;
    hipError_t e;
    {
        TimedLaunch tl{nullptr, nullptr};
        const bool timed = c->timing > 0 && c->timed[0].size() < 400000;
        if (timed) { tl.a = get_event(c); tl.b = get_event(c); (void)hipEventRecord(tl.a, c->stream); }
        const bool proj = !LK::light(c);          // project_T_each_iter with a t_row_sum: the topic-model instantiation
        e = pick_type<double, float>(c->dtype, [&](auto sx) {
            typedef typename decltype(sx)::type SX;
            constexpr bool F32 = std::is_same<SX, float>::value;
            return pick_bool(c->k > ONCHIP_SMALL_K, [&](auto large_k) {
                constexpr int KT = large_k ? 8 : 3;      // k-term dots of 8 terms per lane (k <= 64), or of 3
                return pick_bool(proj, [&](auto PROJ) {
                    return pick_bool(g.rpw <= onchip_rpw(F32, PROJ, KT, true), [&](auto few) {
                        constexpr int RPW = onchip_rpw(F32, PROJ, KT, few);
                        return pick_bool(a.dbg != nullptr, [&](auto dbg) {
                            // the diagnostics build exists for fp32, KT = 3 only: everywhere else a.dbg is ignored
                            constexpr bool DBG = dbg && F32 && KT == 3;
                            return onchip_launch<SX, RPW, DBG, PROJ, KT>(c, g, a);
                        });
                    });
                });
            });
        });
        if (timed) { (void)hipEventRecord(tl.b, c->stream); c->timed[0].push_back(tl); }
    }
    if (e != hipSuccess) {
        if (getenv("RRI_ONCHIP_DEBUG")) fprintf(stderr, "rri: on-chip sweep not launched (%s): rows/wg %d, rows/wave %d, LDS %zu B\n", hipGetErrorString(e), g.rows_wg, g.rpw, g.shmem);
        (void)hipGetLastError();
        return false;
    }
    c->onchip_launches += 1;
    c->onchip_in_flight = true;
    if (const char* path = getenv("RRI_ONCHIP_LOG")) {      // tests: which configurations took this path (one line per launch)
        if (FILE* f = fopen(path, "a")) {
            fprintf(f, "%lld %lld %d %s %s sweeps %d..%d\n", (long long)c->n, (long long)c->d, k, c->dtype == RRI_F32 ? "f32" : "f64",
                    LK::light(c) ? "plain" : "simplex", cur.sweep, c->run_total);
            fclose(f);
        }
    }
    // what the launch-per-phase schedule would find after these sweeps: no carried sums, nothing pending (the kernel
    // ran the last column check itself); the objective's cross terms are complete when the last sweep ran from topic 0
    const bool whole_last = c->run_total - 1 > cur.sweep || (cur.topic == 0 && cur.phase == 0);
    changed(c, CH_W | CH_T | CH_ENDED);
    c->skip_row_finish = false;
    c->xy_run = whole_last ? k : -1;
    c->xy_rows = g.G;
    c->xy_valid = whole_last;
    c->obj_track_pending = a.track != 0;
    return true;
}

void enqueue_from(rri_ctx* c, Cursor cur) {
    if (cur.sweep < c->run_total && onchip_ok(c) && enqueue_onchip(c, cur)) return;
    // rri_sweep_until without the persistent kernel: nobody applies the stop rule between the sweeps, so the call ends after
    // the sweep it is in and the caller decides
    if (c->until.active && cur.sweep < c->run_total) c->run_total = cur.sweep + 1;
    enqueue_range(c, cur, c->run_total);
    flush_wcheck(c, c->run_total, 0);      // last column of the call: report it in this call
}

rri_status read_state(rri_ctx* c, DevState* out) {
    HIPCHK(c, hipMemcpyAsync(out, c->st, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_status != RRI_OK) {   // a collective of the sequence just run failed: its text is in c->err
        const rri_status r = c->comm_status;
        c->comm_status = RRI_OK;
        changed(c, CH_ENDED);
        return r;
    }
    return RRI_OK;
}

rri_status status_from_halt(rri_ctx* c, const DevState& s, int32_t* sweeps_done) {
    if (s.halt == 0) {
        c->paused = false;
        if (sweeps_done) *sweeps_done = c->run_total;
        return RRI_OK;
    }
    changed(c, CH_ENDED);
    if (s.halt == HALT_EVENT_STOP) {      // rri_sweep_until: the stop rule held after sweep halt_sweep - 1; nothing of the next one is stored
        c->paused = false;
        if (sweeps_done) *sweeps_done = s.halt_sweep;
        return RRI_OK;
    }
    if (s.halt > 0) {
        // rri_sweep_until: an event ends the call with the sweep it interrupts (position 0: the column check of the sweep before
        // -- nothing of sweep halt_sweep has begun); that sweep's objective is the caller's to take after the event is resolved
        if (c->until.active) c->run_total = std::min(c->run_total, (s.halt == HALT_EVENT_RESET_W && s.halt_pos == 0) ? s.halt_sweep : s.halt_sweep + 1);
        c->paused = true;
        c->pending.kind = s.halt == HALT_EVENT_RESET_T ? RRI_EVENT_RESET_T : RRI_EVENT_RESET_W;
        c->pending.topic = s.halt_topic;
        c->pending.sweep = s.halt_sweep;
        c->pending.resume_topic = s.halt_pos;
        if (s.halt == HALT_EVENT_RESET_T) c->resume_at = Cursor{s.halt_sweep, s.halt_topic, 1};
        else c->resume_at = Cursor{s.halt_sweep, s.halt_pos, 0};
        if (sweeps_done) *sweeps_done = s.halt_sweep;
        return RRI_PAUSED;
    }
    c->paused = false;
    if (sweeps_done) *sweeps_done = s.halt_sweep;
    switch (s.halt) {
        case HALT_ERR_UNBOUNDED:
            return fail(c, RRI_ERR_UNBOUNDED, "Minimum objective is unbounded (topic %d)", s.halt_topic);
        case HALT_ERR_W_COL_ZERO:
            return fail(c, RRI_ERR_W_COL_ZERO, "W[:, t] sums to 0 (topic %d)", s.halt_topic);
        case HALT_ERR_NOT_IMPLEMENTED:
            return fail(c, RRI_ERR_NOT_IMPLEMENTED, "s=%g is not yet implemented", c->prm.t_row_sum);
        case HALT_ERR_GRID_SYNC:
            return fail(c, RRI_ERR_HIP, "the persistent sweep's workgroups could not synchronise (not all resident); RRI_ONCHIP=0 selects the launch-per-phase schedule");
        default:
            return fail(c, RRI_ERR_INVALID, "unknown device status %d", s.halt);
    }
}

rri_status clear_halt(rri_ctx* c) {
    HIPCHK(c, hipMemsetAsync(c->st, 0, 32, c->stream));  // halt, halt_topic, halt_sweep, halt_pos, tmode, proj_iters
    return RRI_OK;
}

// The only place that reads the switches a handle keeps: an unset variable means the default, whatever the handles
// created before this one were created under
rri_switches read_switches() {
    rri_switches sw;
    if (const char* e = getenv("RRI_ONCHIP")) sw.onchip = atoi(e) != 0;
    if (const char* e = getenv("RRI_ONCHIP_OBJ")) sw.onchip_obj = atoi(e) != 0;
    if (const char* e = getenv("RRI_WSWEEP")) sw.wsweep = atoi(e) != 0;
    if (const char* e = getenv("RRI_TROW_SMALL")) sw.trow_fused = atoi(e) != 0;
    if (const char* e = getenv("RRI_OBJ_DIRECT")) sw.obj_direct = atoi(e) != 0;
    if (const char* e = getenv("RRI_WMCORR_COLS")) sw.wmcorr_cols = atoi(e) != 0;
    if (const char* e = getenv("RRI_WNW_MASK")) sw.wnw_mask = atoi(e) != 0;
    if (const char* e = getenv("RRI_PASS_ROT")) sw.pass_rot = atoi(e) & 7;
    if (const char* e = getenv("RRI_ROT_CAL")) sw.rot_cal = std::max(0, atoi(e));
    sw.rot_debug = getenv("RRI_ROT_DEBUG") != nullptr;
    if (const char* e = getenv("RRI_MASK_BITS")) sw.mask_bits = atoi(e) != 0;
    if (const char* e = getenv("RRI_PASS_CACHE_MB")) sw.pass_cache_mb = std::max(0.0, atof(e));
    if (const char* e = getenv("RRI_X_PACK")) sw.x_pack = atoi(e) == 2 ? 2 : atoi(e) != 0;
    if (const char* e = getenv("RRI_EARLY_SUMS")) sw.early_sums = atoi(e) != 0;
    if (const char* e = getenv("RRI_EARLY_DEAL")) sw.early_deal = atoi(e) != 0;
    if (const char* e = getenv("RRI_PASS_PK_GEOM")) {
        char* end = nullptr;
        sw.pk_rows = (int)std::min<long>(std::max<long>(0, strtol(e, &end, 10)), 1 << 20);
        sw.pk_il = (end && *end == 'i') ? 1 : (end && *end == 'c') ? 0 : -1;
    }
    return sw;
}

// what the data entry points of a dense handle say on a handle that keeps X on a pattern
const char* sparse_data_refusal(const rri_ctx* c) {
    return c->sparse_x ? "an RRI_UNWEIGHTED_SPARSE handle keeps X as CSR: it takes its data through rri_upload_X_csr only "
                         "(no dense X, no device binding, no mask)"
                       : "a sparse-pattern handle takes its data through rri_upload_observed_csr";
}

// the entry points that rewrite X in place, or need a mask, a residual, a CSR store or a scratch residual, on a handle of one of
// the two read-only stores (float16; uint8 counts with scales)
#define REFUSE_RO(c, what)                                                                                              \
    if (ro_store((c)->dtype))                                                                                           \
        return fail((c), RRI_ERR_UNSUPPORTED, "%s is not available on an %s handle (%s stores a dense X that is only read)", what, \
                    dtype_name((c)->dtype), (c)->dtype == RRI_F16 ? "float16" : "uint8")

// ---- frozen rows (rri_frozen.hpp) -----------------------------------------------------------------------------------------
// W fixed: the W[:,t] *= nt1 of a T-row step stays in the kept column, and would have to reach the frozen rows as well
const char* const FROZEN_FIX_W_TEXT = "frozen statistics are set and fix_W is: the W[:,t] *= nt1 transfer of a T-row step would have to "
                                      "reach the frozen rows (clear the statistics, or let W move)";
bool frozen_fix_W(const rri_ctx* c) { return c->fzB && c->have_params && c->prm.fix_W; }
// which handles take frozen statistics: unweighted, Gram form, dense float32 / float64 or CSR-resident X without uniform rows, one device
const char* frozen_refusal(const rri_ctx* c) {
    if (c->weighted == RRI_WEIGHTED_DENSE || c->weighted == RRI_WEIGHTED_SPARSE) return "a weighted handle sums its rows under a mask: frozen statistics are for unweighted handles";
    if (c->explicit_resid) return "the explicit-residual schedule keeps R = X - W T of its own rows: frozen statistics need the Gram form";
    if (ro_store(c->dtype)) return "frozen statistics are not available on an RRI_F16 or RRI_U8 handle";
    if (c->sparse_x && c->uni_n > 0) return "frozen statistics are not available on a CSR handle with uniform rows";
    if (c->comm) return "a communicator is attached: frozen statistics are for a handle on one device";
    return nullptr;
}
void frozen_release(rri_ctx* c) {
    dev_release(c, c->fzB); dev_release(c, c->fzA); dev_release(c, c->fzs); dev_release(c, c->fztail);
    c->fz_c = 0.0;
    c->fz_rows = 0;
}
// all four or none, zeroed
hipError_t frozen_alloc(rri_ctx* c) {
    if (c->fzB) return hipSuccess;
    hipError_t e = dev_alloc(c, c->fzB, (size_t)c->k * c->LD * sizeof(double), true);
    if (e == hipSuccess) e = dev_alloc(c, c->fzA, (size_t)c->k * c->k * sizeof(double), true);
    if (e == hipSuccess) e = dev_alloc(c, c->fzs, (size_t)c->k * sizeof(double), true);
    if (e == hipSuccess) e = dev_alloc(c, c->fztail, 2 * sizeof(double), true);
    if (e != hipSuccess) frozen_release(c);
    return e;
}
void frozen_clear_topic_dev(rri_ctx* c, int t) {
    if (!c->fzB) return;
    const i64 m = std::max<i64>(c->LD, c->k);
    hipLaunchKernelGGL(k_frozen_clear, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, c->fzB, c->LD, c->fzA, c->k, c->fzs, t);
}

rri_status ready(rri_ctx* c) {
    if (!c->have_X || !c->have_W || !c->have_T || !c->have_params)
        return fail(c, RRI_ERR_INVALID, "X, W, T and params must be set before stepping");
    if (c->weighted && !c->have_M) return fail(c, RRI_ERR_INVALID, "weighted handle without a mask");
    return RRI_OK;
}

}  // namespace

// ====================================================================================================
extern "C" {

uint32_t rri_abi_version(void) { return RRI_ABI_VERSION; }

const char* rri_last_error(const rri_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

rri_status rri_create(rri_ctx** out, int64_t n, int64_t d, int32_t k, int32_t dtype, int32_t weighted,
                      int32_t device, void* stream) {
    if (!out) return RRI_ERR_INVALID;
    *out = nullptr;
    if (n < 1 || d < 1 || k < 1) return fail(nullptr, RRI_ERR_INVALID, "need n,d,k >= 1 (got %lld,%lld,%d)", n, d, k);
    if (dtype != RRI_F32 && dtype != RRI_F64 && dtype != RRI_F16 && dtype != RRI_U8)
        return fail(nullptr, RRI_ERR_INVALID, "dtype must be RRI_F32, RRI_F64, RRI_F16 or RRI_U8");
    if (n > 2000000000LL || d > 2000000000LL) return fail(nullptr, RRI_ERR_INVALID, "n, d must fit int32");
    if (k > RRI_MAX_K) return fail(nullptr, RRI_ERR_UNSUPPORTED, "k=%d is above the rank limit RRI_MAX_K = %d of the device path", k, RRI_MAX_K);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, RRI_ERR_HIP, "no HIP device available (librri_hip needs an MI355X)");
    if (device < 0 || device >= ndev) return fail(nullptr, RRI_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    if (weighted < 0 || weighted > 4)
        return fail(nullptr, RRI_ERR_INVALID, "weighted must be RRI_UNWEIGHTED, RRI_WEIGHTED_DENSE, RRI_WEIGHTED_SPARSE, "
                                              "RRI_UNWEIGHTED_RESIDUAL or RRI_UNWEIGHTED_SPARSE");
    if (ro_store(dtype) && weighted != RRI_UNWEIGHTED) {
        // Both are stores for a dense X that is only ever read.  Counts are no store for a residual (signed, fractional); float16
        // would round the explicit residual and the dense weighted residual, which are rewritten at every topic step (k S
        // roundings to 11 bits over S sweeps); CSR values are a store of their own with its own layout, which has neither
        static const struct { int dtype; const char *stores, *rewritten, *csr; } refusal[] = {
            {RRI_U8, "RRI_U8 stores read-only dense counts (RRI_UNWEIGHTED)", "keeps a stored residual, which counts 0..255 cannot hold",
             "keeps its values in a CSR store, which has no uint8 layout"},
            {RRI_F16, "RRI_F16 stores a read-only dense X (RRI_UNWEIGHTED)",
             "rewrites its stored residual at every topic step, which float16 would round every time",
             "keeps its values in a CSR store, which has no float16 layout"}};
        static const char* const flavour[] = {"", "RRI_WEIGHTED_DENSE", "RRI_WEIGHTED_SPARSE", "RRI_UNWEIGHTED_RESIDUAL", "RRI_UNWEIGHTED_SPARSE"};
        const bool rewritten = weighted == RRI_WEIGHTED_DENSE || weighted == RRI_UNWEIGHTED_RESIDUAL;
        for (const auto& r : refusal)
            if (r.dtype == dtype)
                return fail(nullptr, RRI_ERR_UNSUPPORTED, "%s; %s %s", r.stores, flavour[weighted], rewritten ? r.rewritten : r.csr);
    }
    rri_ctx* c = new rri_ctx();
    c->device = device;
#define CR(call)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            fail(nullptr, RRI_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));             \
            rri_destroy(c);                                                                        \
            return RRI_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)
    CR(hipSetDevice(device));
    CR(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
    if (stream) c->stream = (hipStream_t)stream;
    else { CR(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }

    // the plan (rri_layout.hpp: every rule and its reasons), copied into the members the launch sites read
    c->sw = read_switches();
    const DensePlan p = c->plan = dense_plan(n, d, k, dtype, weighted, c->sw, c->n_cu);
    const bool explicit_resid = p.explicit_resid;
    weighted = p.weighted;   // the explicit-residual and the CSR-X handle are the unweighted flavour of the algorithm
    c->explicit_resid = p.explicit_resid; c->sparse_x = p.sparse_x; c->sparse = p.sparse;
    c->n = n; c->d = d; c->k = k; c->dtype = dtype; c->weighted = weighted;
    c->kp = p.kp; c->es = dtype_size(dtype); c->VN = p.VN; c->PW = p.PW; c->LD = p.LD;
    c->npanels = p.npanels; c->rpb = p.rpb; c->nrb = p.nrb; c->ro_il = p.ro_il;
    for (int w = 0; w < 2 && p.sparse; ++w) {
        rri_ctx::SpCopy& cp = c->sp[w];
        cp.gdim = p.sp[w].gdim; cp.nseg = p.sp[w].nseg; cp.nblk = p.sp[w].nblk; cp.bw = p.sp[w].bw;
    }
    c->nwb = p.nwb; c->nwb256 = p.nwb256; c->ntb = p.ntb; c->ntb32 = p.ntb32; c->nsplit = p.nsplit;
    c->red_elems = p.red_elems; c->xy_stride = p.xy_stride; c->cpart_rows = p.cpart_rows;
    c->ldw = n;
    c->keep_q = pass_keep(c);
    c->tpart_n = c->ntb;
    c->gpart_n = c->nwb;
    c->ttpart_n = c->nsplit;

    const size_t f8 = sizeof(double);
    CR(dev_alloc(c, c->W, (size_t)k * c->ldw * f8));
    CR(dev_alloc(c, c->T, (size_t)k * c->LD * f8, true));
    CR(dev_alloc(c, c->Ypart, (size_t)c->npanels * n * f8, true));
    CR(dev_alloc(c, c->Zpart, (size_t)c->nrb * c->LD * f8, true));
    CR(dev_alloc(c, c->Gpart, (size_t)p.gpart_rows * (k + 2) * f8, true));
    CR(dev_alloc(c, c->XYpart, (size_t)k * c->xy_stride * f8, true));
    CR(dev_alloc(c, c->red, (size_t)c->red_elems * f8, true));
    CR(dev_alloc(c, c->xraw, (size_t)c->LD * f8, true));
    CR(dev_alloc(c, c->Ttpart, (size_t)p.ttpart_rows * k * f8, true));
    CR(dev_alloc(c, c->Qt, (size_t)k * c->ldw * f8));
    const size_t ntp = (size_t)p.tpart_rows;
    CR(dev_alloc(c, c->tpart, ntp * f8, true));
    CR(dev_alloc(c, c->tpart_idx, ntp * sizeof(i64)));
    CR(dev_alloc(c, c->normpart, 256 * 3 * f8));
    CR(dev_alloc(c, c->objbuf, (size_t)(2 * k * k + k) * f8));
    CR(dev_alloc(c, c->dtmp, 16 * f8));
    CR(dev_alloc(c, c->itmp, 16 * sizeof(i64)));
    if (c->sw.early_sums && !weighted && !explicit_resid && !p.sparse && k > 1) {      // the early-sums schedule (LK::early_ok)
        CR(dev_alloc(c, c->Tearly, (size_t)p.nte * k * f8, true));
        CR(dev_alloc(c, c->edot, (size_t)n * f8, true));
        CR(dev_alloc(c, c->Gearly, (size_t)p.e_blocks * (k + 2) * f8, true));
        CR(dev_alloc(c, c->ent, 8 * f8, true));
        CR(dev_alloc(c, c->wfp, (size_t)2 * c->nwb * f8, true));
    }
    // The flavours' own buffers, each in the order its flavour has always asked for them (calibrate_rot: the speed of a
    // read-modify-write pass belongs to the buffer's placement).  The stored residual first: k_resid writes the d real columns only
    // and the passes stream all LD, so the pad columns must hold zeros (recycled memory there once held NaN patterns, which
    // fmax(numer, 0) turned into zero rows of W)
    const bool keeps_resid = explicit_resid || (weighted && !c->sparse);
    if (keeps_resid) CR(dev_alloc(c, c->E, (size_t)n * c->LD * c->es, c->LD != d));
    if (weighted) {
        CR(dev_alloc(c, c->Y2part, (size_t)c->npanels * n * f8, true));
        CR(dev_alloc(c, c->Z2part, (size_t)c->nrb * c->LD * f8, true));
        if (!c->sparse) {
            CR(dev_alloc(c, c->Cpart, (size_t)c->cpart_rows * c->LD * f8, true));
            CR(dev_alloc(c, c->N2part, (size_t)c->cpart_rows * c->LD * f8, true));
        }
        CR(dev_alloc(c, c->dtv, (size_t)c->LD * f8, true));
    }
    if (weighted || explicit_resid) CR(dev_alloc(c, c->dwv, (size_t)n * f8, explicit_resid));
    if (weighted) CR(dev_alloc(c, c->wold, (size_t)n * f8));
    if (explicit_resid) CR(dev_alloc(c, c->told, (size_t)c->LD * f8, true));
    if (weighted || explicit_resid) CR(dev_alloc(c, c->zeros, (size_t)std::max<i64>(c->LD, n) * f8, true));
    if (c->sparse) CR(dev_alloc(c, c->sp_Tt, (size_t)d * c->kp * f8, true));
    if (dtype == RRI_U8) {
        CR(dev_alloc(c, c->rscale, (size_t)n * f8));
        CR(dev_alloc(c, c->cscale, (size_t)c->LD * f8));
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->rscale, (i64)n, 1.0);
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((c->LD + 255) / 256)), dim3(256), 0, c->stream, c->cscale, c->LD, 1.0);
    }
    CR(dev_alloc(c, c->st, sizeof(DevState), true));
    // opt in to large dynamic LDS where a kernel needs it
    if (dtype == RRI_F32) CR(LaunchX<float>::set_attrs(c));
    else if (dtype == RRI_F64) CR(LaunchX<double>::set_attrs(c));
    else if (dtype == RRI_F16) CR(LaunchX<_Float16>::set_attrs(c));
    else CR(LaunchX<unsigned char>::set_attrs(c));
    CR(hipStreamSynchronize(c->stream));
#undef CR
    *out = c;
    return RRI_OK;
}

rri_status rri_destroy(rri_ctx* c) {
    if (!c) return RRI_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (const auto& o : c->owned) {
        (void)hipFree(o.p);
        dev_count(-1, o.bytes);
    }
    for (int i = 0; i < 9; ++i)
        for (auto& tl : c->timed[i]) { (void)hipEventDestroy(tl.a); (void)hipEventDestroy(tl.b); }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RRI_OK;
}

// ---- data ------------------------------------------------------------------------------------------
rri_status rri_upload_X(rri_ctx* c, const void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    if (rri_status s = check_host_matrix(c, host, ld, host_dtype, c->d, c->dtype)) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if (!dev_owned(c, &c->X)) HIPCHK(c, dev_alloc(c, c->X, (size_t)c->n * c->LD * c->es, c->LD != c->d));   // (none yet, or a bound one)
    c->ldx = c->LD;
    c->store_err[0] = c->store_err[1] = 0.0;
    rri_status s = to_device(c, host, ld, host_dtype, c->X, c->ldx, c->n, c->d, c->dtype);
    // (a float16 or uint8 upload that fails -- the range check -- has already overwritten the store: the handle then has no X)
    if (s == RRI_OK || ro_store(c->dtype)) { c->have_X = s == RRI_OK; changed(c, CH_X); }
    if (s == RRI_OK) s = reset_scales(c);
    return s;
}

rri_status rri_upload_mask(rri_ctx* c, const void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    REFUSE_RO(c, "a mask");
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    if (!c->weighted) return fail(c, RRI_ERR_INVALID, "handle was not created with weighted=1");
    if (rri_status s = check_host_matrix(c, host, ld, host_dtype, c->d, c->dtype)) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if (!dev_owned(c, &c->M)) HIPCHK(c, dev_alloc(c, c->M, (size_t)c->n * c->LD * c->es, c->LD != c->d));   // (none yet, or a bound one)
    c->ldm = c->LD;
    rri_status s = to_device(c, host, ld, host_dtype, c->M, c->ldm, c->n, c->d, c->dtype);
    if (s == RRI_OK) {
        c->have_M = true;
        changed(c, CH_M);
        DISPATCH(c, s = L::pack_mask_if_binary(c));
        if (s != RRI_OK) return fail(c, s, "packing the mask failed");
        if (c->Mbits) dev_release(c, c->M);   // bits replace it
    }
    return s;
}

namespace {
struct CsrDev {   // device copies of the host CSR arrays of one call
    DevTmp indptr, indices, data;
    const i64* ip() const { return (const i64*)indptr.p; }
    const int* ix() const { return (const int*)indices.p; }
};
rri_status csr_to_device(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* data, int64_t nnz,
                         int32_t data_dtype, CsrDev& out, CsrRules rules = CSR_COLUMNS) {
    const std::string bad = csr_check(indptr, indices, data, nnz, data_dtype, c->n, c->d, rules);
    if (!bad.empty()) return fail(c, RRI_ERR_INVALID, "%s", bad.c_str());
    const size_t ds = dtype_size(data_dtype);
    HIPCHK(c, out.indptr.alloc((size_t)(c->n + 1) * sizeof(i64)));
    HIPCHK(c, out.indices.alloc((size_t)std::max<i64>(nnz, 1) * sizeof(int)));
    HIPCHK(c, out.data.alloc((size_t)std::max<i64>(nnz, 1) * ds));
    HIPCHK(c, hipMemcpyAsync(out.indptr.p, indptr, (size_t)(c->n + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        HIPCHK(c, hipMemcpyAsync(out.indices.p, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(out.data.p, data, (size_t)nnz * ds, hipMemcpyHostToDevice, c->stream));
    }
    return RRI_OK;
}
}  // namespace

namespace {
struct CorpusArrays {   // the canonical arrays of an rri_corpus, where they are: int64 indptr, int32 indices, float64 values (device)
    const i64* indptr;
    const int* indices;
    const double* values;
};
}  // namespace
static rri_status upload_X_csr_kept(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* data,
                                    int64_t nnz, int32_t data_dtype, const CorpusArrays* resident = nullptr);

rri_status rri_upload_X_csr(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* data,
                            int64_t nnz, int32_t data_dtype) {
    CHECK_CTX(c);
    REFUSE_RO(c, "X from CSR arrays");
    if (c->sparse_x) return upload_X_csr_kept(c, indptr, indices, data, nnz, data_dtype);
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    HIPCHK(c, hipSetDevice(c->device));
    CsrDev dv;
    rri_status s = csr_to_device(c, indptr, indices, data, nnz, data_dtype, dv);
    if (s != RRI_OK) return s;
    if (!dev_owned(c, &c->X)) HIPCHK(c, dev_alloc(c, c->X, (size_t)c->n * c->LD * c->es));   // (none yet, or a bound one)
    c->ldx = c->LD;
    HIPCHK(c, hipMemsetAsync(c->X, 0, (size_t)c->n * c->LD * c->es, c->stream));
    const unsigned nb = (unsigned)((c->n + 3) / 4);
    pick_type<float, double>(data_dtype, [&](auto s) {
        typedef typename decltype(s)::type Src;
        pick_type<float, double>(c->dtype, [&](auto d) {
            typedef typename decltype(d)::type Dst;
            hipLaunchKernelGGL((k_csr_scatter<Src, Dst>), dim3(nb), dim3(256), 0, c->stream, dv.ip(), dv.ix(), (const Src*)dv.data.p, c->n, (Dst*)c->X, c->ldx);
        });
    });
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_X = true;
    changed(c, CH_X);
    return RRI_OK;
}

namespace {
rri_status build_sp_store(rri_ctx* c, const int64_t* indptr, const int32_t* indices, int64_t nnz, int32_t data_dtype,
                          CsrDev& dv, int target_items);
rri_status build_sp_store_device(rri_ctx* c, CsrDev& dv, const double* values, int64_t nnz, int target_items);
}
// RRI_UNWEIGHTED_SPARSE: X stays CSR -- the canonical copy and the two blocked copies with X's values (k_spx_pass).  Two ways in,
// one way out: host arrays (rri_upload_X_csr), which are checked, sorted and uploaded and whose blocked copies the host builds
// (build_sp_store); or `resident`, the canonical arrays of a corpus (rri_upload_X_corpus, which has checked the request), which
// are copied on the device and whose blocked copies are built there (build_sp_store_device).  The same bytes either way
static rri_status upload_X_csr_kept(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* data,
                                    int64_t nnz, int32_t data_dtype, const CorpusArrays* resident) {
    if (nnz >= 2147483647LL) return fail(c, RRI_ERR_UNSUPPORTED, "more than 2^31-1 stored entries");
    CsrDev dv;
    rri_status s = RRI_OK;
    std::vector<int32_t> sidx;
    std::vector<unsigned char> sval;
    if (resident) {
        HIPCHK(c, hipSetDevice(c->device));
        // the handle's own copies of the index arrays: the corpus is not kept and may go right after the call
        HIPCHK(c, dv.indptr.alloc((size_t)(c->n + 1) * sizeof(i64)));
        HIPCHK(c, dv.indices.alloc((size_t)std::max<i64>(nnz, 1) * sizeof(int)));
        HIPCHK(c, hipMemcpyAsync(dv.indptr.p, resident->indptr, (size_t)(c->n + 1) * sizeof(i64), hipMemcpyDeviceToDevice, c->stream));
        if (nnz > 0) HIPCHK(c, hipMemcpyAsync(dv.indices.p, resident->indices, (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    } else {
        std::string bad = csr_check(indptr, indices, data, nnz, data_dtype, c->n, c->d, CSR_ROWS);
        if (!bad.empty()) return fail(c, RRI_ERR_INVALID, "%s", bad.c_str());
        HIPCHK(c, hipSetDevice(c->device));
        // column indices sorted inside every row (a sorted host copy where the caller's are not); duplicates are refused
        if (csr_sort_rows(indptr, indices, data, c->n, nnz, dtype_size(data_dtype), sidx, sval)) { indices = sidx.data(); data = sval.data(); }
        bad = csr_duplicates(indptr, indices, c->n);
        if (!bad.empty()) return fail(c, RRI_ERR_INVALID, "%s", bad.c_str());
        s = csr_to_device(c, indptr, indices, data, nnz, data_dtype, dv);
        if (s != RRI_OK) return s;
    }
    // from here on the store is being replaced: the uniform rows were rows of the X that goes, and a new X has none -- cleared
    // first, so that an upload that fails further down leaves no list beside a store it does not describe
    dev_release(c, c->uni_rows);
    c->uni_n = 0;
    c->uni_value = 0.0;
    s = resident ? build_sp_store_device(c, dv, resident->values, nnz, sp_target_items(c->n_cu, true))
                 : build_sp_store(c, indptr, indices, nnz, data_dtype, dv, sp_target_items(c->n_cu, true));
    if (s != RRI_OK) return s;
    if (nnz > 0)
        DISPATCH(c, for (int w = 0; w < 2; ++w)
                        hipLaunchKernelGGL((k_sp_permute<typename L::Elem>), dim3(2048), dim3(256), 0, c->stream,
                                           (const typename L::Elem*)c->sp_x, (const int*)c->sp[w].perm, c->sp[w].count,
                                           (typename L::Elem*)c->sp[w].val));
    dev_release(c, c->spx_work);
    const int nw0 = c->sp[0].nwork, nw1 = c->sp[1].nwork;
    // every block of a copy has a work item, an empty one included, so every X pass writes all of its partials: the launches that
    // add to them afterwards (the uniform rows' share) rely on it
    if (nw0 < 1 || nw1 < 1) return fail(c, RRI_ERR_HIP, "a blocked copy of X has no work item (%d, %d)", nw0, nw1);
    HIPCHK(c, dev_alloc(c, c->spx_work, (size_t)std::max(1, nw0 + nw1) * sizeof(SpWork)));
    if (nw0 > 0) HIPCHK(c, hipMemcpyAsync(c->spx_work, c->sp[0].work, (size_t)nw0 * sizeof(SpWork), hipMemcpyDeviceToDevice, c->stream));
    if (nw1 > 0) HIPCHK(c, hipMemcpyAsync(c->spx_work + nw0, c->sp[1].work, (size_t)nw1 * sizeof(SpWork), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_X = true;
    changed(c, CH_X);
    return RRI_OK;
}

rri_status rri_upload_mask_csr_pattern(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* data,
                                       int64_t nnz, int32_t data_dtype) {
    CHECK_CTX(c);
    REFUSE_RO(c, "a mask");
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    if (!c->weighted) return fail(c, RRI_ERR_INVALID, "handle was not created with weighted=1");
    HIPCHK(c, hipSetDevice(c->device));
    CsrDev dv;
    rri_status s = csr_to_device(c, indptr, indices, data, nnz, data_dtype, dv);
    if (s != RRI_OK) return s;
    dev_release(c, c->M);
    c->ldm = c->LD;
    dev_release(c, c->Mbits);
    dev_release(c, c->Mcols);
    c->mcols_tried = false;
    c->ldb = (c->LD + 3) / 4;
    const size_t words = (size_t)((c->n + 7) / 8) * c->ldb;
    HIPCHK(c, dev_alloc(c, c->Mbits, words * sizeof(unsigned), true));
    const unsigned nb = (unsigned)((c->n + 3) / 4);
    pick_type<float, double>(data_dtype, [&](auto s) {
        typedef typename decltype(s)::type Src;
        hipLaunchKernelGGL((k_csr_pattern_bits<Src>), dim3(nb), dim3(256), 0, c->stream, dv.ip(), dv.ix(), (const Src*)dv.data.p, c->n, c->Mbits, c->ldb);
    });
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_M = true;
    changed(c, CH_M);
    return RRI_OK;
}

namespace {
// The canonical CSR (rowptr, col, values in the storage type) and the two blocked copies of a pattern, shared by the
// pattern-only weighted handle and the unweighted handle with X on CSR.  indptr / indices: the validated host arrays (column
// indices strictly increasing in every row); dv: their device copies (csr_to_device), taken over as the canonical CSR.
// `target_items`: work items per copy (SpWork.pad = the copy).  The blocked copies' values are left zero.
rri_status build_sp_store(rri_ctx* c, const int64_t* indptr, const int32_t* indices, int64_t nnz, int32_t data_dtype,
                          CsrDev& dv, int target_items) {
    i64 longest_row = 0;
    c->spb_ms = 0.0;
    dev_release(c, c->sp_rowptr); dev_release(c, c->sp_col); dev_release(c, c->sp_x); dev_release(c, c->sp_e);
    dev_adopt(c, c->sp_rowptr, dv.indptr);     // from here on they are the handle's, whatever fails below
    dev_adopt(c, c->sp_col, dv.indices);
    HIPCHK(c, dev_alloc(c, c->sp_x, (size_t)std::max<i64>(nnz, 1) * c->es));
    if (nnz > 0) {   // values -> storage type (dv.data holds them in the caller's type)
        launch_convert(c, data_dtype, c->dtype, false, dv.data.p, nnz, c->sp_x, nnz, 1, nnz);
    }
    // the two blocked copies, built on the host (build_sp_copy, rri_layout.hpp)
    for (int w = 0; w < 2; ++w) {
        rri_ctx::SpCopy& cp = c->sp[w];
        dev_release(c, cp.segptr); dev_release(c, cp.idx); dev_release(c, cp.val); dev_release(c, cp.perm); dev_release(c, cp.work);
        SpDims dims;
        dims.nblk = cp.nblk; dims.bw = cp.bw; dims.nseg = cp.nseg; dims.gdim = cp.gdim;
        const SpCopyHost h = build_sp_copy(indptr, indices, c->n, nnz, w, dims, target_items);
        const size_t cntp = h.idx.size();
        cp.count = h.count;
        cp.nwork = (int)h.work.size();
        cp.lps = h.lps;
        longest_row = h.longest_row;
        HIPCHK(c, dev_alloc(c, cp.segptr, h.segptr.size() * sizeof(i64)));
        HIPCHK(c, dev_alloc(c, cp.idx, cntp * sizeof(unsigned short)));
        HIPCHK(c, dev_alloc(c, cp.val, cntp * c->es, true));
        HIPCHK(c, dev_alloc(c, cp.perm, cntp * sizeof(int)));
        HIPCHK(c, dev_alloc(c, cp.work, std::max<size_t>(1, h.work.size()) * sizeof(SpWork)));
        HIPCHK(c, hipMemcpyAsync(cp.segptr, h.segptr.data(), h.segptr.size() * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cp.idx, h.idx.data(), cntp * sizeof(unsigned short), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cp.perm, h.perm.data(), cntp * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (!h.work.empty())
            HIPCHK(c, hipMemcpyAsync(cp.work, h.work.data(), h.work.size() * sizeof(SpWork), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vectors go out of scope
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->nnz = nnz;
    c->sp_max_row = (int)longest_row;
    return RRI_OK;
}
}  // namespace

rri_status rri_upload_observed_csr(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const void* values,
                                   int64_t nnz, int32_t data_dtype) {
    CHECK_CTX(c);
    // a request of rri_upload_observed_corpus: the canonical arrays of a checked corpus stand in for the host arrays, are copied on
    // the device and the blocked copies are built there (build_sp_store_device) -- the same bytes either way
    const rri_ctx::ObsReq* resident = c->obs_req;
    c->obs_req = nullptr;
    if (resident) nnz = resident->nnz;
    REFUSE_RO(c, "an observation pattern");
    if (!c->sparse || c->sparse_x) return fail(c, RRI_ERR_INVALID, "handle was not created with weighted=RRI_WEIGHTED_SPARSE");
    if (nnz >= 2147483647LL) return fail(c, RRI_ERR_UNSUPPORTED, "more than 2^31-1 observed entries");
    HIPCHK(c, hipSetDevice(c->device));
    CsrDev dv;   // validates the arrays; its device copies of indptr / indices become the CSR copy
    rri_status s = RRI_OK;
    if (resident) {
        // the handle's own copies of the index arrays: the corpus is not kept and may go right after the call
        HIPCHK(c, dv.indptr.alloc((size_t)(c->n + 1) * sizeof(i64)));
        HIPCHK(c, dv.indices.alloc((size_t)std::max<i64>(nnz, 1) * sizeof(int)));
        HIPCHK(c, hipMemcpyAsync(dv.indptr.p, resident->indptr, (size_t)(c->n + 1) * sizeof(i64), hipMemcpyDeviceToDevice, c->stream));
        if (nnz > 0) HIPCHK(c, hipMemcpyAsync(dv.indices.p, resident->indices, (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        s = build_sp_store_device(c, dv, resident->values, nnz, sp_target_items(c->n_cu, false));
    } else {
        s = csr_to_device(c, indptr, indices, values, nnz, data_dtype, dv, CSR_INCREASING);
        if (s != RRI_OK) return s;
        s = build_sp_store(c, indptr, indices, nnz, data_dtype, dv, sp_target_items(c->n_cu, false));
    }
    if (s != RRI_OK) return s;
    HIPCHK(c, dev_alloc(c, c->sp_e, (size_t)std::max<i64>(nnz, 1) * c->es));
    c->have_X = true;
    c->have_M = true;
    changed(c, CH_X | CH_M);
    return RRI_OK;
}

rri_status rri_storage_error(rri_ctx* c, double out[2]) {
    CHECK_CTX(c);
    if (!out) return fail(c, RRI_ERR_INVALID, "out is NULL");
    out[0] = c->store_err[0];
    out[1] = c->store_err[1];
    return RRI_OK;
}

rri_status rri_bind_X_device(rri_ctx* c, const void* dev, int64_t ld) {
    CHECK_CTX(c);
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    const i64 vb = load_bytes(c->dtype);      // 16 (uint8: 8)
    if (!dev || ld < c->d || (ld * (i64)c->es) % vb || ((uintptr_t)dev) % vb)
        return fail(c, RRI_ERR_INVALID, "device X must be %lld-byte aligned with a %lld-byte-multiple row stride >= d", vb, vb);
    if (c->d % c->VN) return fail(c, RRI_ERR_INVALID, "binding device X needs d %% %d == 0 (no pad columns)", c->VN);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());   // the memory may have been produced on another stream a moment ago
    dev_release(c, c->X);
    c->X = const_cast<void*>(dev);
    c->ldx = ld;
    c->store_err[0] = c->store_err[1] = 0.0;   // bound memory is taken as it is: nothing was rounded here
    c->have_X = true;
    changed(c, CH_X);
    return reset_scales(c);
}

rri_status rri_bind_mask_device(rri_ctx* c, const void* dev, int64_t ld) {
    CHECK_CTX(c);
    REFUSE_RO(c, "a mask");
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "%s", sparse_data_refusal(c));
    if (!c->weighted) return fail(c, RRI_ERR_INVALID, "handle was not created with weighted=1");
    const i64 vb = load_bytes(c->dtype);      // 16: a mask has the storage type of a weighted handle, fp32 or float64
    if (!dev || ld < c->d || (ld * (i64)c->es) % vb || ((uintptr_t)dev) % vb)
        return fail(c, RRI_ERR_INVALID, "device mask must be 16-byte aligned with a 16-byte-multiple row stride >= d");
    if (c->d % c->VN) return fail(c, RRI_ERR_INVALID, "binding a device mask needs d %% %d == 0", c->VN);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());   // the mask is read at once (bit-packing): it must be complete
    dev_release(c, c->M);
    c->M = const_cast<void*>(dev);
    c->ldm = ld;
    c->have_M = true;
    changed(c, CH_M);
    rri_status ps = RRI_OK;
    DISPATCH(c, ps = L::pack_mask_if_binary(c));
    if (ps != RRI_OK) return fail(c, ps, "packing the mask failed");
    return RRI_OK;
}

rri_status rri_set_W(rri_ctx* c, const void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    rri_status s = to_device(c, host, ld, host_dtype, c->W, c->ldw, c->n, c->k, RRI_F64, true);
    if (s == RRI_OK) { c->have_W = true; changed(c, CH_W | CH_ENDED); }
    return s;
}
rri_status rri_set_T(rri_ctx* c, const void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    rri_status s = to_device(c, host, ld, host_dtype, c->T, c->LD, c->k, c->d, RRI_F64);
    if (s == RRI_OK) { c->have_T = true; changed(c, CH_T); }
    return s;
}
rri_status rri_get_W(rri_ctx* c, void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, c->W, c->ldw, host, ld, host_dtype, c->n, c->k, RRI_F64, true);
}
rri_status rri_get_T(rri_ctx* c, void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, c->T, c->LD, host, ld, host_dtype, c->k, c->d, RRI_F64);
}

rri_status rri_set_params(rri_ctx* c, const rri_params* p) {
    CHECK_CTX(c);
    if (!p) return fail(c, RRI_ERR_INVALID, "params is NULL");
    if (p->has_t_row_sum && !(p->t_row_sum > 0)) return fail(c, RRI_ERR_INVALID, "t_row_sum must be > 0");
    if (p->has_w_row_sum && !(p->w_row_sum > 0)) return fail(c, RRI_ERR_INVALID, "w_row_sum must be > 0");
    if (p->reset_method < 0 || p->reset_method > 2) return fail(c, RRI_ERR_INVALID, "bad reset_method");
    if (p->fix_W && p->fix_T) return fail(c, RRI_ERR_INVALID, "fix_W and fix_T together leave nothing to update");
    const bool form_before = c->have_params && resid_sched(c);
    // the objective a persistent sweep left behind has the penalties of THAT launch folded in
    if (c->have_params && (c->prm.reg_w_l1 != p->reg_w_l1 || c->prm.reg_w_l2 != p->reg_w_l2 || c->prm.reg_t_l1 != p->reg_t_l1 ||
                           c->prm.reg_t_l2 != p->reg_t_l2))
        changed(c, CH_PENALTY);
    c->prm = *p;
    c->have_params = true;
    if (c->explicit_resid && form_before != resid_sched(c)) {
        // the call that follows steps in the other form: the sums carried between calls belong to the form that left them,
        // and a residual the Gram form does not maintain is stale
        changed(c, CH_SCRATCH);
    }
    return RRI_OK;
}

// ---- the hot path ------------------------------------------------------------------------------------
static rri_status run_and_collect(rri_ctx* c, Cursor from, int32_t* sweeps_done) {
    HIPCHK(c, hipSetDevice(c->device));
    c->onchip_in_flight = false;
    c->obj_track_pending = false;
    enqueue_from(c, from);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(c, RRI_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    DevState s;
    rri_status r = read_state(c, &s);
    if (r != RRI_OK) return r;
    if (c->onchip_in_flight && s.halt == HALT_ERR_GRID_SYNC) {
        // The persistent launch gave up: its workgroups did not all run at the same time within the bound of the polls (a
        // device shared with another process, CUs masked away).  The reference's sweep cannot fail for scheduling reasons
        // (nmf.py:415-476), so neither may this one: W and T go back to what they were before the launch, and the same
        // range of steps runs on the launch-per-phase schedule, which needs no co-residency.  The handle stays there.
        c->onchip_in_flight = false;
        c->onchip_fallbacks += 1;
        c->onchip_off = true;
        c->onchip_off_until = steady_now_ns() + (2000000000LL << std::min<long>(c->onchip_fallbacks - 1, 5));
        long long backoff_ms = 2000;                                        // the whole process: 2 s off the persistent path
        if (const char* e = getenv("RRI_ONCHIP_BACKOFF_MS")) backoff_ms = std::max(0, atoi(e));      // tests: 0
        g_onchip_backoff_until.store(steady_now_ns() + backoff_ms * 1000000LL);
        if (getenv("RRI_ONCHIP_DEBUG")) fprintf(stderr, "rri: the persistent sweep gave up; sweeps %d.. rerun launch by launch\n", from.sweep);
        HIPCHK(c, hipMemcpyAsync(c->W, c->Wsafe, (size_t)c->k * c->ldw * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->T, c->Tsafe, (size_t)c->k * c->LD * 8, hipMemcpyDeviceToDevice, c->stream));
        // A launch that gave up IN the run (not at its entry) has left more than W and T behind: objective slots of the sweeps it
        // finished (rri_sweep_until's history: "NaN = no value from the kernel" must hold for the sweeps rerun below) and
        // DevState.obj_track.  The history goes back to "not written"; obj_track is never read for this call (onchip_in_flight is
        // off, CH_ENDED drops obj_track_valid), XYpart is rewritten by the rerun's own W halves.
        if (c->objhist && c->until.active)
            HIPCHK(c, hipMemsetAsync(c->objhist, 0xFF, (size_t)std::min(std::max(c->until.n, 0), ONCHIP_UNTIL_CAP) * 8, c->stream));
        c->obj_track_pending = false;
        changed(c, CH_ENDED);
        c->skip_row_finish = c->onchip_saved_skip;
        r = clear_halt(c);
        if (r != RRI_OK) return r;
        if (c->until.active) c->run_total = std::min(c->run_total, from.sweep + 1);     // no stop rule on this schedule: one sweep, then the caller
        enqueue_range(c, from, c->run_total);
        flush_wcheck(c, c->run_total, 0);
        le = hipGetLastError();
        if (le != hipSuccess) return fail(c, RRI_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(le));
        r = read_state(c, &s);
        if (r != RRI_OK) return r;
    }
    if (c->onchip_in_flight && c->obj_track_pending && s.halt == 0 && c->xy_valid) {
        c->obj_track_value = s.obj_track;       // came with the state read above: no kernel, no second trip for rri_objective
        c->obj_track_valid = true;
    }
    c->obj_track_pending = false;
    c->onchip_in_flight = false;
    if (s.halt != 0 && s.pad1 == 1) {     // k_wfold_verdict halted the queue: the fold launches enqueued behind that sweep returned at once
        const int at = s.halt_pos == 0 ? s.halt_sweep - 1 : s.halt_sweep;
        c->fold_halts += 1;
        c->fold_launches -= std::max(0, c->run_total - 1 - at);
    }
    return status_from_halt(c, s, sweeps_done);
}

rri_status rri_sweep(rri_ctx* c, int32_t n_sweeps, int32_t* sweeps_done) {
    CHECK_CTX(c);
    rri_status r = ready(c);
    if (r != RRI_OK) return r;
    if (c->paused) return fail(c, RRI_ERR_INVALID, "a paused run is pending: resolve the event and call rri_resume");
    if (n_sweeps < 0) return fail(c, RRI_ERR_INVALID, "n_sweeps < 0");
    if (frozen_fix_W(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", FROZEN_FIX_W_TEXT);
    c->until.active = false;
    c->run_total = n_sweeps;
    r = clear_halt(c);
    if (r != RRI_OK) return r;
    return run_and_collect(c, Cursor{0, 0, 0}, sweeps_done);
}

static rri_status ensure_x_sq(rri_ctx* c);
// the objective history of a finished rri_sweep_until call: what the kernel left (NaN where it left nothing)
static rri_status until_finish(rri_ctx* c, rri_status r, const int32_t* sweeps_done) {
    if (!c->until.active || r == RRI_PAUSED) return r;
    c->until.active = false;
    if (r != RRI_OK || !c->until.out) return r;
    const int done = sweeps_done ? std::min(std::max(*sweeps_done, 0), c->until.n) : 0;
    for (int i = 0; i < c->until.n; ++i) c->until.out[i] = std::nan("");
    if (done > 0 && c->objhist && c->onchip_launches > 0) {
        hipError_t e = hipMemcpyAsync(c->until.out, c->objhist, (size_t)done * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "objective history: %s", hipGetErrorString(e));
    }
    return r;
}

rri_status rri_sweep_until(rri_ctx* c, int32_t n_sweeps, double obj_prev, double stop_scale, double* obj_hist, int32_t* sweeps_done) {
    CHECK_CTX(c);
    rri_status r = ready(c);
    if (r != RRI_OK) return r;
    if (c->paused) return fail(c, RRI_ERR_INVALID, "a paused run is pending: resolve the event and call rri_resume");
    if (n_sweeps < 1 || !obj_hist || !sweeps_done) return fail(c, RRI_ERR_INVALID, "n_sweeps < 1, or no place for the history / the count");
    HIPCHK(c, hipSetDevice(c->device));
    if (!onchip_ok(c) || n_sweeps > ONCHIP_UNTIL_CAP || !c->sw.onchip_obj)
        return fail(c, RRI_ERR_UNSUPPORTED, "rri_sweep_until needs the register-resident sweep (rri_onchip_info) and at most %d sweeps", ONCHIP_UNTIL_CAP);
    r = ensure_x_sq(c);
    if (r != RRI_OK) return r;
    // the slots of the history the kernel writes must read "nothing" if no persistent launch of this call wrote them
    if (c->objhist) HIPCHK(c, hipMemsetAsync(c->objhist, 0xFF, (size_t)n_sweeps * 8, c->stream));
    c->until.active = true; c->until.prev = obj_prev; c->until.scale = stop_scale; c->until.n = n_sweeps; c->until.out = obj_hist;
    c->run_total = n_sweeps;
    r = clear_halt(c);
    if (r != RRI_OK) { c->until.active = false; return r; }
    r = run_and_collect(c, Cursor{0, 0, 0}, sweeps_done);
    if (r != RRI_OK && r != RRI_PAUSED) c->until.active = false;
    return until_finish(c, r, sweeps_done);
}

rri_status rri_resume(rri_ctx* c, int32_t* sweeps_done) {
    CHECK_CTX(c);
    if (!c->paused) return fail(c, RRI_ERR_INVALID, "nothing to resume");
    if (c->pending.kind != RRI_EVENT_NONE) return fail(c, RRI_ERR_INVALID, "pending event not resolved");
    c->paused = false;
    rri_status r = clear_halt(c);
    if (r != RRI_OK) return r;
    int32_t done_local = 0;
    r = run_and_collect(c, c->resume_at, sweeps_done ? sweeps_done : &done_local);
    if (r != RRI_OK && r != RRI_PAUSED) c->until.active = false;
    return until_finish(c, r, sweeps_done ? sweeps_done : &done_local);
}

rri_status rri_pending_event(rri_ctx* c, rri_event* ev) {
    CHECK_CTX(c);
    if (!ev) return fail(c, RRI_ERR_INVALID, "ev is NULL");
    *ev = c->paused ? c->pending : rri_event{RRI_EVENT_NONE, -1, 0, 0};
    return RRI_OK;
}

// a reset rewrote T[t,:] and W[:,t] (T[t,:] even when T is otherwise fixed, nmf.py:808,814); in a paused run it resolves the event
static void reset_applied(rri_ctx* c) {
    if (c->paused && c->pending.kind != RRI_EVENT_NONE) {
        if (c->pending.kind == RRI_EVENT_RESET_T) c->skip_row_finish = true;
        c->pending.kind = RRI_EVENT_NONE;
        if (c->prm.resets_left > 0) c->prm.resets_left -= 1;
    }
    changed(c, CH_W | CH_T);
}

rri_status rri_apply_reset_max_resid(rri_ctx* c, int32_t t, int64_t* row_chosen) {
    CHECK_CTX(c);
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->rowpos, (size_t)c->n * sizeof(double)));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    DISPATCH_RO(c, L::resid(c, false, false, nullptr, c->rowpos));
    hipLaunchKernelGGL(k_vec_sum_argmax, dim3(1), dim3(1024), 0, c->stream, (const double*)c->rowpos, c->n,
                       (double*)nullptr, c->itmp);
    if (c->comm) {
        // row-sharded (nmf.py:771-776 over all rows): every rank offers its largest row-residual norm, the global
        // winner -- lowest global row index on ties, as np.argmax -- broadcasts max(X[mi,:] - W[mi,:] T, 0); T[t,:]
        // becomes that row on every rank, W[:,t] the unit vector of the winning row
        rri_comm* m = c->comm;
        hipLaunchKernelGGL(k_pack_candidate, dim3(1), dim3(1), 0, c->stream, (const double*)c->rowpos,
                           (const i64*)c->itmp, c->row_offset, c->ctail);
        comm_allgather(c, c->ctail, 2, c->cand);
        std::vector<double> cand((size_t)2 * m->world);
        // the peers go on to the broadcast below: a failure here must not just return (comm_abort)
        hipError_t he = hipMemcpyAsync(cand.data(), c->cand, cand.size() * 8, hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
        if (he != hipSuccess) return comm_abort(c, "reading the reset candidates", he);
        int win = 0;
        for (int r = 1; r < m->world; ++r)
            if (cand[2 * r] > cand[2 * win] || (cand[2 * r] == cand[2 * win] && cand[2 * r + 1] < cand[2 * win + 1])) win = r;
        if (m->rank == win) DISPATCH_RO(c, L::reset_row(c));          // xraw = the reset row (d doubles)
        comm_broadcast(c, c->xraw, c->LD, win);
        if (m->rank != win) {
            const i64 none = -1;
            HIPCHK(c, hipMemcpyAsync(c->itmp, &none, sizeof(i64), hipMemcpyHostToDevice, c->stream));
        }
        LK::reset_commit(c, t);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->comm_status != RRI_OK) { const rri_status r = c->comm_status; c->comm_status = RRI_OK; return r; }
        if (row_chosen) *row_chosen = (int64_t)cand[2 * win + 1];
        reset_applied(c);
        return RRI_OK;
    }
    DISPATCH_RO(c, L::reset_row(c));
    LK::reset_commit(c, t);
    frozen_clear_topic_dev(c, t);      // W[:,t] = 0 (nmf.py:775) reaches the frozen rows: only the handle's rows were candidates
    i64 mi = -1;
    HIPCHK(c, hipMemcpyAsync(&mi, c->itmp, sizeof(i64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (row_chosen) *row_chosen = mi;
    reset_applied(c);
    return RRI_OK;
}

rri_status rri_apply_reset_vectors(rri_ctx* c, int32_t t, const double* T_row, const double* W_col) {
    CHECK_CTX(c);
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->resetT, (size_t)c->d * sizeof(double)));
    HIPCHK(c, dev_ensure(c, c->resetW, (size_t)c->n * sizeof(double)));
    if (T_row) HIPCHK(c, hipMemcpyAsync(c->resetT, T_row, (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (W_col) HIPCHK(c, hipMemcpyAsync(c->resetW, W_col, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LK::set_row_col(c, t, T_row ? c->resetT : nullptr, W_col ? c->resetW : nullptr);
    frozen_clear_topic_dev(c, t);      // the frozen rows get no share of a column drawn anew
    HIPCHK(c, hipStreamSynchronize(c->stream));
    reset_applied(c);
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    return RRI_OK;
}

rri_status rri_skip_reset(rri_ctx* c) {
    CHECK_CTX(c);
    if (!c->paused) return fail(c, RRI_ERR_INVALID, "no pending event");
    c->pending.kind = RRI_EVENT_NONE;
    c->prm.resets_left = 0;
    rri_status r = clear_halt(c);
    if (r != RRI_OK) return r;
    return RRI_OK;
}

rri_status rri_update_T_row(rri_ctx* c, int32_t t) {
    CHECK_CTX(c);
    rri_status r = ready(c);
    if (r != RRI_OK) return r;
    if (c->weighted) return fail(c, RRI_ERR_UNSUPPORTED, "half steps are not exposed for the weighted flavour");
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    if (frozen_fix_W(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", FROZEN_FIX_W_TEXT);
    HIPCHK(c, hipSetDevice(c->device));
    c->run_total = 1;
    r = clear_halt(c);
    if (r != RRI_OK) return r;
    if (resid_sched(c)) enqueue_rT_half(c, 0, t, true);
    else enqueue_T_half(c, 0, t, true);
    DevState s;
    r = read_state(c, &s);
    if (r != RRI_OK) return r;
    return status_from_halt(c, s, nullptr);
}

rri_status rri_update_W_col(rri_ctx* c, int32_t t) {
    CHECK_CTX(c);
    rri_status r = ready(c);
    if (r != RRI_OK) return r;
    if (c->weighted) return fail(c, RRI_ERR_UNSUPPORTED, "half steps are not exposed for the weighted flavour");
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    HIPCHK(c, hipSetDevice(c->device));
    c->run_total = 1;
    r = clear_halt(c);
    if (r != RRI_OK) return r;
    c->skip_row_finish = true;   // a lone W half: the T-row checks belong to rri_update_T_row
    if (resid_sched(c)) enqueue_rW_half(c, 0, t);
    else enqueue_W_half(c, 0, t);
    flush_wcheck(c, 1, 0);
    DevState s;
    r = read_state(c, &s);
    if (r != RRI_OK) return r;
    return status_from_halt(c, s, nullptr);
}

// ---- around the loop ------------------------------------------------------------------------------------
rri_status rri_project_W_rows(rri_ctx* c, double s, const double* s_vec) {
    CHECK_CTX(c);
    if (!c->have_W) return fail(c, RRI_ERR_INVALID, "W not set");
    if (!s_vec && !(s > 0)) return fail(c, RRI_ERR_INVALID, "Radius s must be strictly positive");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp dv;
    double* dvec = nullptr;
    if (s_vec) {
        HIPCHK(c, dv.alloc((size_t)c->n * sizeof(double)));
        dvec = (double*)dv.p;
        HIPCHK(c, hipMemcpyAsync(dvec, s_vec, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    LK::proj_rows(c, s, dvec);
    hipError_t e = hipStreamSynchronize(c->stream);
    changed(c, CH_W);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "projection failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

static rri_status norms_of(rri_ctx* c, const double* A, i64 rows, i64 cols, i64 ld, double out[3]) {
    LK::norms(c, A, rows, cols, ld);
    double h[256 * 3];
    HIPCHK(c, hipMemcpyAsync(h, c->normpart, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = 0.0;
    for (int b = 0; b < 256; ++b) { out[0] += h[3 * b]; out[1] += h[3 * b + 1]; out[2] += h[3 * b + 2]; }
    return RRI_OK;
}

// out = {data term, ||W||^2, ||W||_1}; tn (optional) = {., ||T||^2, ||T||_1}: everything rri_objective needs, with
// ONE synchronisation on the path taken after a complete sweep
// ||X||^2, once per X (the constant of the objective's Gram form)
static rri_status ensure_x_sq(rri_ctx* c) {
    if (c->x_sq_valid) return RRI_OK;
    if (c->sparse_x)    // the stored entries as one row
        DISPATCH(c, hipLaunchKernelGGL((k_sqsum<typename L::Elem>), dim3(256), dim3(256), 0, c->stream,
                                       (const typename L::Elem*)c->sp_x, std::max<i64>(c->nnz, 1), (i64)1, c->nnz, c->normpart, XScale{nullptr, nullptr}));
    else
        DISPATCH_RO(c, hipLaunchKernelGGL((k_sqsum<typename L::Elem>), dim3(256), dim3(256), 0, c->stream,
                                       (const typename L::Elem*)c->X, c->ldx, c->n, c->d, c->normpart, L::xscale(c)));
    double h[256];
    HIPCHK(c, hipMemcpyAsync(h, c->normpart, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->x_sq = 0.0;
    for (int b = 0; b < 256; ++b) c->x_sq += h[b];
    if (c->sparse_x && c->uni_n > 0) c->x_sq += (double)c->uni_n * (double)c->d * (c->uni_value * c->uni_value);   // the rows of U
    c->x_sq_valid = true;
    return RRI_OK;
}

static rri_status objective_terms(rri_ctx* c, double out[3], double* tn) {
    CHECK_CTX(c);
    if (!c->have_X || !c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "X, W, T must be set");
    if (c->weighted && !c->have_M) return fail(c, RRI_ERR_INVALID, "weighted handle without a mask");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->rowobj, (size_t)c->n * sizeof(double)));
    if (c->weighted) {
        // the objective needs M .* (X - W T) -- which is the maintained residual: store it while it is being
        // computed, and the sweep that follows skips its own rebuild (nmf() asks for the objective after
        // every sweep, nmf.py:488-490)
        DISPATCH(c, L::resid(c, true, true, c->rowobj, nullptr));
        resid_rebuilt(c);
        c->carry_valid = false;
    } else if (c->xy_valid && !c->sw.obj_direct) {
        // 1/2 ||X - W T||^2 = 1/2 ||X||^2 - sum_t <w_t, X t_t> + 1/2 <W^T W, T T^T>: the cross terms were left by
        // the W halves of the sweep that has just ended (k_wcol), ||X||^2 is taken once per X -- no pass over X.
        // The terms are of the size of ||X||^2: the result carries an absolute error of a few ulp of that
        // (relative 1e-11 at a residual of 0.5 %), far below what the stop rule of nmf.py:510 resolves.
        const int k = c->k;
        rri_status rx = ensure_x_sq(c);
        if (rx != RRI_OK) return rx;
        double* gw = c->objbuf;
        double* gt = gw + k * k;
        double* xy = gt + k * k;
        hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->W, c->ldw, c->n, k, gw);
        hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->T, c->LD, c->d, k, gt);
        hipLaunchKernelGGL(k_rows_sum, dim3(k), dim3(256), 0, c->stream, (const double*)c->XYpart, c->xy_rows, c->xy_stride, xy);
        // ||.||^2 are the traces of the Gram matrices; the 1-norms are only needed with an l1 penalty
        const bool need_l1 = c->prm.reg_w_l1 != 0.0 || c->prm.reg_t_l1 != 0.0 || !tn;
        double hw[256 * 3], ht[256 * 3];
        if (need_l1) {
            LK::norms(c, c->W, c->k, c->n, c->ldw);
            HIPCHK(c, hipMemcpyAsync(hw, c->normpart, sizeof hw, hipMemcpyDeviceToHost, c->stream));
            if (tn) {
                LK::norms(c, c->T, c->k, c->d, c->LD);
                HIPCHK(c, hipMemcpyAsync(ht, c->normpart, sizeof ht, hipMemcpyDeviceToHost, c->stream));
            }
        }
        std::vector<double> h((size_t)(2 * k * k + k));
        HIPCHK(c, hipMemcpyAsync(h.data(), gw, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double cross = 0.0, quad = 0.0, w2 = 0.0, t2 = 0.0;
        for (int t = 0; t < k; ++t) cross += h[(size_t)2 * k * k + t];
        for (int a = 0; a < k * k; ++a) quad += h[(size_t)a] * h[(size_t)k * k + a];
        for (int t = 0; t < k; ++t) { w2 += h[(size_t)t * k + t]; t2 += h[(size_t)k * k + (size_t)t * k + t]; }
        double w1 = 0.0, t1 = 0.0;
        if (need_l1) {
            for (int b = 0; b < 256; ++b) w1 += hw[3 * b + 2];
            if (tn) for (int b = 0; b < 256; ++b) t1 += ht[3 * b + 2];
        }
        out[0] = 0.5 * c->x_sq - cross + 0.5 * quad;
        out[1] = w2;
        out[2] = w1;
        if (tn) { tn[0] = 0.0; tn[1] = t2; tn[2] = t1; }
        return RRI_OK;
    } else if (c->explicit_resid) {
        // the objective is 1/2 ||R||^2 of the residual this schedule keeps: store it while it is computed, and the
        // sweep that follows skips its own rebuild
        DISPATCH(c, L::resid(c, false, true, c->rowobj, nullptr));
        resid_rebuilt(c);
    } else if (c->sparse_x) {
        // X on CSR, without the cross terms of a complete sweep: ||X - W T||^2 = sum_pattern r^2 + (<W^T W, T T^T> -
        // sum_pattern (W T)_ij^2) -- outside the pattern the residual is -(W T)_ij, whose squares are the Gram term less the
        // pattern's share
        HIPCHK(c, dev_ensure(c, c->rowhat, (size_t)c->n * sizeof(double)));
        DISPATCH(c, L::sp_resid(c, false, c->rowobj, nullptr, c->rowhat));
        const int k = c->k;
        double* gw = c->objbuf;
        double* gt = gw + k * k;
        hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->W, c->ldw, c->n, k, gw);
        hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->T, c->LD, c->d, k, gt);
        hipLaunchKernelGGL(k_vec_sum_argmax, dim3(1), dim3(1024), 0, c->stream, (const double*)c->rowobj, c->n,
                           c->dtmp, (i64*)nullptr);
        hipLaunchKernelGGL(k_vec_sum_argmax, dim3(1), dim3(1024), 0, c->stream, (const double*)c->rowhat, c->n,
                           c->dtmp + 1, (i64*)nullptr);
        std::vector<double> h((size_t)2 * k * k);
        double sums[2] = {0.0, 0.0};
        HIPCHK(c, hipMemcpyAsync(h.data(), gw, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(sums, c->dtmp, sizeof sums, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double quad = 0.0;
        for (int q = 0; q < k * k; ++q) quad += h[(size_t)q] * h[(size_t)k * k + q];
        double nw[3];
        rri_status r = norms_of(c, c->W, c->k, c->n, c->ldw, nw);
        if (r != RRI_OK) return r;
        out[0] = 0.5 * (sums[0] + (quad - sums[1]));
        out[1] = nw[1];
        out[2] = nw[2];
        if (tn) return norms_of(c, c->T, c->k, c->d, c->LD, tn);
        return RRI_OK;
    } else {
        DISPATCH_RO(c, L::resid(c, false, false, c->rowobj, nullptr));
    }
    hipLaunchKernelGGL(k_vec_sum_argmax, dim3(1), dim3(1024), 0, c->stream, (const double*)c->rowobj, c->n,
                       c->dtmp, (i64*)nullptr);
    double base = 0.0;
    HIPCHK(c, hipMemcpyAsync(&base, c->dtmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double nw[3];
    rri_status r = norms_of(c, c->W, c->k, c->n, c->ldw, nw);
    if (r != RRI_OK) return r;
    out[0] = 0.5 * base;
    out[1] = nw[1];
    out[2] = nw[2];
    if (tn) return norms_of(c, c->T, c->k, c->d, c->LD, tn);
    return RRI_OK;
}

// the frozen rows' share of the stacked objective, 1/2 (c - 2 <B, T> + <A, T T^T>), added to the data term
static rri_status frozen_objective_add(rri_ctx* c, double* data_term) {
    if (!c->fzB) return RRI_OK;
    const int k = c->k;
    DevTmp tt, part;
    HIPCHK(c, tt.alloc((size_t)k * k * sizeof(double)));
    HIPCHK(c, part.alloc(256 * sizeof(double)));
    hipLaunchKernelGGL(k_gram, dim3(k, k), dim3(256), 0, c->stream, (const double*)c->T, c->LD, c->d, k, (double*)tt.p);
    hipLaunchKernelGGL(k_frozen_dot, dim3(256), dim3(256), 0, c->stream, (const double*)c->fzB, (const double*)c->T, (i64)k * c->LD,
                       (double*)part.p);
    std::vector<double> hA((size_t)k * k), hT((size_t)k * k);
    double hp[256];
    HIPCHK(c, hipMemcpyAsync(hA.data(), c->fzA, hA.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hT.data(), tt.p, hT.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hp, part.p, sizeof hp, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double bt = 0.0;
    for (int b = 0; b < 256; ++b) bt += hp[b];
    *data_term += frozen_objective_share(k, hA.data(), hT.data(), bt, c->fz_c);
    return RRI_OK;
}

rri_status rri_objective_parts(rri_ctx* c, double out[3]) {
    const rri_status r = objective_terms(c, out, nullptr);
    return r == RRI_OK ? frozen_objective_add(c, &out[0]) : r;
}

rri_status rri_objective(rri_ctx* c, double* out) {
    CHECK_CTX(c);
    if (!out) return fail(c, RRI_ERR_INVALID, "out is NULL");
    if (c->obj_track_valid && c->xy_valid && !c->weighted && !c->comm && !c->sw.obj_direct && !c->fzB) {
        // the persistent sweep that has just ended left its objective (all terms but the constant): nothing to launch
        if (!c->have_X || !c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "X, W, T must be set");
        HIPCHK(c, hipSetDevice(c->device));
        rri_status rx = ensure_x_sq(c);
        if (rx != RRI_OK) return rx;
        *out = 0.5 * c->x_sq + c->obj_track_value;
        return RRI_OK;
    }
    double parts[3], nt[3];
    rri_status r = objective_terms(c, parts, nt);
    if (r != RRI_OK) return r;
    r = frozen_objective_add(c, &parts[0]);
    if (r != RRI_OK) return r;
    r = comm_allreduce_host(c, parts, 3);    // row-sharded: the terms over rows are sums over the ranks; T is replicated
    if (r != RRI_OK) return r;
    const rri_params& q = c->prm;
    // base + wr2 + tr2 + tr1 + wr1 (nmf.py:83-91)
    *out = parts[0] + 0.5 * q.reg_w_l2 * parts[1] + 0.5 * q.reg_t_l2 * nt[1] + q.reg_t_l1 * nt[2] +
           q.reg_w_l1 * parts[2];
    return RRI_OK;
}

rri_status rri_argmax_rows(rri_ctx* c, int32_t* out_host) {
    CHECK_CTX(c);
    if (!out_host) return fail(c, RRI_ERR_INVALID, "out is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp dv;
    HIPCHK(c, dv.alloc((size_t)c->n * sizeof(int)));
    int* dev = (int*)dv.p;
    LK::argmax_rows(c, dev);
    hipError_t e = hipMemcpyAsync(out_host, dev, (size_t)c->n * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "argmax failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

rri_status rri_masked_rmse(rri_ctx* c, const int64_t* ij, const double* vals, int64_t count, double lo, double hi,
                           double* out) {
    CHECK_CTX(c);
    // row-sharded (a communicator attached): collective; (i, j) are LOCAL rows, a rank may hold no entry at all, and the
    // score is sqrt(sum over the ranks of the squared errors / sum of the counts): the same number on every rank, so
    // the early-stop decision of nmf.py:381-407 is the same on every rank
    // With a communicator this call is a collective: a rank that found its own arguments bad must not leave before the
    // all-reduce its peers are about to enter (they would block inside it).  It contributes nothing, raises an error flag that
    // travels with the sums, and EVERY rank returns the error afterwards -- the ranks stay in step.
    const char* bad = nullptr;
    i64 bad_entry = -1;
    if (!out || count < 0 || (count > 0 && (!ij || !vals)) || (count < 1 && !c->comm)) bad = "bad entry list";
    if (!bad)
        for (i64 e = 0; e < count && !bad; ++e)
            if (ij[2 * e] < 0 || ij[2 * e] >= c->n || ij[2 * e + 1] < 0 || ij[2 * e + 1] >= c->d) { bad = "entry out of range"; bad_entry = e; }
    if (bad && !c->comm) return bad_entry >= 0 ? fail(c, RRI_ERR_INVALID, "entry %lld out of range", bad_entry) : fail(c, RRI_ERR_INVALID, "%s", bad);
    HIPCHK(c, hipSetDevice(c->device));
    double s = 0.0;
    hipError_t e = hipSuccess;
    if (count > 0 && !bad) {
        DevTmp tij, tv;
        e = tij.alloc((size_t)count * 2 * sizeof(i64));
        if (e == hipSuccess) e = tv.alloc((size_t)count * sizeof(double));
        i64* dij = (i64*)tij.p;
        double* dv = (double*)tv.p;
        if (e == hipSuccess) e = hipMemcpyAsync(dij, ij, (size_t)count * 2 * sizeof(i64), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dv, vals, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream);
        double h[256];
        if (e == hipSuccess) {
            LK::masked_sqerr(c, dij, dv, count, lo, hi);
            e = hipMemcpyAsync(h, c->normpart, sizeof h, hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess)
            for (int b = 0; b < 256; ++b) s += h[b];
    }
    // [squared errors, count, ranks whose arguments were bad, ranks whose device work failed]
    double tot[4] = {bad ? 0.0 : s, bad ? 0.0 : (double)count, bad ? 1.0 : 0.0, e != hipSuccess ? 1.0 : 0.0};
    if (c->comm) {
        // a rank whose validation or device work failed still takes part in the collective (its peers would wait for it
        // otherwise); the failure is reported on every rank afterwards
        const rri_status r = comm_allreduce_host(c, tot, 4);
        if (r != RRI_OK) return r;
    }
    if (bad) return bad_entry >= 0 ? fail(c, RRI_ERR_INVALID, "entry %lld out of range", bad_entry) : fail(c, RRI_ERR_INVALID, "%s", bad);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "masked rmse failed: %s", hipGetErrorString(e));
    if (tot[2] > 0.0) return fail(c, RRI_ERR_INVALID, "bad entry list on another rank (%d of them)", (int)tot[2]);
    if (tot[3] > 0.0) return fail(c, RRI_ERR_HIP, "masked rmse failed on another rank");
    if (!(tot[1] > 0.0)) return fail(c, RRI_ERR_INVALID, "no entry on any rank");
    *out = std::sqrt(tot[0] / tot[1]);
    return RRI_OK;
}

// The N best columns of W T per requested row (rri_topn.hpp has the order).  Reads the handle's W and T; everything else it
// needs -- row list, exclusion CSR, outputs -- lives in temporaries of the call, so no sum a later sweep reads is touched and
// rri_device_memory reports what it reported before.  Rank-local on a row-sharded handle: no collective.
rri_status rri_topn_rows(rri_ctx* c, const int64_t* rows, int64_t count, int32_t topn, const int64_t* excl_indptr,
                         const int32_t* excl_indices, double clip_lo, double clip_hi, int32_t* idx_out, double* val_out) {
    CHECK_CTX(c);
    char why[200] = "";
    const int bad = topn_check_request(c->n, c->d, rows, count, topn, RRI_MAX_TOPN, excl_indptr, excl_indices, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    if (count == 0) return RRI_OK;
    if (!idx_out || !val_out) return fail(c, RRI_ERR_INVALID, "an output array is NULL");
    if (!c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    if ((count + TOPN_ROWS - 1) / TOPN_ROWS > 0x7fffffffLL) return fail(c, RRI_ERR_INVALID, "count %lld is too large for one call", (long long)count);
    HIPCHK(c, hipSetDevice(c->device));
    const i64 nex = excl_indptr ? excl_indptr[count] : 0;
    DevTmp trows, tptr, tidx, tj, tv;
    if (rows) HIPCHK(c, trows.alloc((size_t)count * sizeof(i64)));
    if (excl_indptr) {
        HIPCHK(c, tptr.alloc((size_t)(count + 1) * sizeof(i64)));
        HIPCHK(c, tidx.alloc((size_t)std::max<i64>(nex, 1) * sizeof(int)));
    }
    HIPCHK(c, tj.alloc((size_t)count * topn * sizeof(int)));
    HIPCHK(c, tv.alloc((size_t)count * topn * sizeof(double)));
    if (rows) HIPCHK(c, hipMemcpyAsync(trows.p, rows, (size_t)count * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    if (excl_indptr) {
        HIPCHK(c, hipMemcpyAsync(tptr.p, excl_indptr, (size_t)(count + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        if (nex > 0) HIPCHK(c, hipMemcpyAsync(tidx.p, excl_indices, (size_t)nex * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    hipError_t e = LK::topn_rows(c, (const i64*)trows.p, count, topn, (const i64*)tptr.p, (const int*)tidx.p, nullptr, clip_lo,
                                 clip_hi, (int*)tj.p, (double*)tv.p);
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, tj.p, (size_t)count * topn * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(val_out, tv.p, (size_t)count * topn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "top-N rows failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

// The rank of listed columns in the total order of their rows of W T (rri_rank.hpp has the semantics).  Reads the handle's W
// and T; row list, target and exclusion CSR, the pieces and the outputs live in temporaries of the call, so no sum a later sweep
// reads is touched and rri_device_memory reports what it reported before.  Rank-local on a row-sharded handle: no collective.
rri_status rri_rank_entries(rri_ctx* c, const int64_t* rows, int64_t count, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                            const int64_t* excl_indptr, const int32_t* excl_indices, double clip_lo, double clip_hi,
                            int32_t* rank_out, double* val_out, int32_t* eligible_out) {
    CHECK_CTX(c);
    char why[200] = "";
    if (rank_check_request(c->n, c->d, rows, count, tgt_indptr, tgt_indices, excl_indptr, excl_indices, why, sizeof why) != TOPN_REQ_OK)
        return fail(c, RRI_ERR_INVALID, "%s", why);
    const i64 ntg = count > 0 ? tgt_indptr[count] : 0;
    if (count == 0 || ntg == 0) return RRI_OK;
    if (!rank_out || !val_out) return fail(c, RRI_ERR_INVALID, "an output array is NULL");
    if (!c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    std::vector<RankPiece> pieces((size_t)rank_cut_pieces(tgt_indptr, count, nullptr));
    const i64 npieces = rank_cut_pieces(tgt_indptr, count, pieces.data());
    if ((npieces + RANK_PIECES - 1) / RANK_PIECES > 0x7fffffffLL) return fail(c, RRI_ERR_INVALID, "count %lld is too large for one call", (long long)count);
    HIPCHK(c, hipSetDevice(c->device));
    const i64 nex = excl_indptr ? excl_indptr[count] : 0;
    DevTmp trows, tpc, ttg, tptr, tidx, tr, tv, te;
    if (rows) HIPCHK(c, trows.alloc((size_t)count * sizeof(i64)));
    HIPCHK(c, tpc.alloc((size_t)npieces * sizeof(RankPiece)));
    HIPCHK(c, ttg.alloc((size_t)ntg * sizeof(int)));
    if (excl_indptr) {
        HIPCHK(c, tptr.alloc((size_t)(count + 1) * sizeof(i64)));
        HIPCHK(c, tidx.alloc((size_t)std::max<i64>(nex, 1) * sizeof(int)));
    }
    HIPCHK(c, tr.alloc((size_t)ntg * sizeof(int)));
    HIPCHK(c, tv.alloc((size_t)ntg * sizeof(double)));
    if (eligible_out) HIPCHK(c, te.alloc((size_t)count * sizeof(int)));
    if (rows) HIPCHK(c, hipMemcpyAsync(trows.p, rows, (size_t)count * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tpc.p, pieces.data(), (size_t)npieces * sizeof(RankPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ttg.p, tgt_indices, (size_t)ntg * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (excl_indptr) {
        HIPCHK(c, hipMemcpyAsync(tptr.p, excl_indptr, (size_t)(count + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        if (nex > 0) HIPCHK(c, hipMemcpyAsync(tidx.p, excl_indices, (size_t)nex * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    hipError_t e = LK::rank_entries(c, (const i64*)trows.p, (const RankPiece*)tpc.p, npieces, (const int*)ttg.p, (const i64*)tptr.p,
                                    (const int*)tidx.p, nullptr, clip_lo, clip_hi, (int*)tr.p, (double*)tv.p, (int*)te.p);
    if (e == hipSuccess) e = hipMemcpyAsync(rank_out, tr.p, (size_t)ntg * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(val_out, tv.p, (size_t)ntg * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && eligible_out) e = hipMemcpyAsync(eligible_out, te.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // the pieces (host memory of this call) have been read by now too
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "rank entries failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

// Document and co-document frequencies of groups of words over a CSR pattern (rri_cooc.hpp has the semantics).  The handle gives
// the device, the stream and the error text: nothing it holds is read or written, so the call needs no X, W or T, touches no sum
// a later sweep reads, and is not collective (counts of row blocks add).  The pattern, the membership table, the masks of a row
// chunk and the counts live in temporaries of the call: rri_device_memory reports what it reported before.  The request is
// checked before the handle and before any HIP call.
// what rri_cooccurrence_counts and rri_corpus_cooccurrence_counts share: everything after the request check.  The pattern is the
// host's (d_indptr NULL: uploaded into temporaries of the call) or a resident one (d_indptr, d_indices: device pointers)
static rri_status cooc_counts(rri_ctx* c, const int64_t* indptr, const int32_t* indices, const i64* d_indptr, const int* d_indices,
                              int64_t n_rows, int64_t n_cols, i64 nnz, const int32_t* words, int32_t n_groups, int32_t group_size,
                              int64_t* df_out, int64_t* codf_out) {
    if (!df_out || !codf_out) return fail(c, RRI_ERR_INVALID, "an output array is NULL");
    const size_t M = (size_t)group_size, ndf = (size_t)n_groups * M, nco = ndf * M;
    std::fill(df_out, df_out + ndf, (int64_t)0);
    std::fill(codf_out, codf_out + nco, (int64_t)0);
    if (n_rows == 0 || nnz == 0) return RRI_OK;
    const CoocMemb memb = cooc_build_memb(words, n_groups, group_size, n_cols);
    if (memb.ent.empty()) return RRI_OK;            // every slot is empty
    std::vector<CoocChunk> chunks;
    cooc_cut_rows(n_rows, n_groups, COOC_MASK_BUDGET, &chunks);
    i64 pad_max = 0;
    for (const CoocChunk& ch : chunks) pad_max = std::max(pad_max, ch.rows_pad);
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp tptr, tidx, tmp, tme, tmask, tco;
    if (!d_indptr) {
        HIPCHK(c, tptr.alloc((size_t)(n_rows + 1) * sizeof(i64)));
        HIPCHK(c, tidx.alloc((size_t)nnz * sizeof(int)));
    }
    HIPCHK(c, tmp.alloc(memb.ptr.size() * sizeof(int)));
    HIPCHK(c, tme.alloc(memb.ent.size() * sizeof(int)));
    HIPCHK(c, tmask.alloc((size_t)pad_max * n_groups * sizeof(unsigned)));
    HIPCHK(c, tco.alloc(nco * sizeof(unsigned long long)));
    if (!d_indptr) {
        HIPCHK(c, hipMemcpyAsync(tptr.p, indptr, (size_t)(n_rows + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(tidx.p, indices, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, c->stream));
        d_indptr = (const i64*)tptr.p;
        d_indices = (const int*)tidx.p;
    }
    HIPCHK(c, hipMemcpyAsync(tmp.p, memb.ptr.data(), memb.ptr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tme.p, memb.ent.data(), memb.ent.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(tco.p, 0, nco * sizeof(unsigned long long), c->stream));
    const int lps = cooc_lps(nnz, n_rows);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < chunks.size() && e == hipSuccess; ++i)
        e = LK::cooc_chunk(c, d_indptr, d_indices, (const int*)tmp.p, (const int*)tme.p, chunks[i], lps, n_groups,
                           group_size, (unsigned*)tmask.p, (unsigned long long*)tco.p);
    if (e == hipSuccess) e = hipMemcpyAsync(codf_out, tco.p, nco * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // the membership table (host memory of this call) has been read by now too
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "co-occurrence counts failed: %s", hipGetErrorString(e));
    for (size_t g = 0; g < (size_t)n_groups; ++g)
        for (size_t a = 0; a < M; ++a) df_out[g * M + a] = codf_out[(g * M + a) * M + a];
    return RRI_OK;
}

rri_status rri_cooccurrence_counts(rri_ctx* c, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                   const int32_t* words, int32_t n_groups, int32_t group_size, int64_t* df_out, int64_t* codf_out) {
    char why[200] = "";
    const int bad = cooc_check_request(indptr, indices, n_rows, n_cols, words, n_groups, group_size, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    CHECK_CTX(c);
    return cooc_counts(c, indptr, indices, nullptr, nullptr, n_rows, n_cols, indptr[n_rows], words, n_groups, group_size, df_out, codf_out);
}

// The log-likelihood of stored counts under the rows of W T (rri_loglik.hpp has the semantics).  Reads the handle's W and T; the
// transposed copy of T, the row list, the entries of a chunk, its pieces, their partials and the outputs live in temporaries of
// the call, sized for the largest chunk and reused by the next one, so no sum a later sweep reads is touched and
// rri_device_memory reports what it reported before.  Rank-local on a row-sharded handle: no collective.  The request is
// checked before any HIP call.
// what rri_entries_loglik and rri_corpus_entries_loglik share: everything after the request check.  The entries are the host's
// (d_indices NULL: a chunk's entries are uploaded into temporaries of the call) or resident ones, which the kernels read in place
static rri_status loglik_entries(rri_ctx* c, const int64_t* rows, int64_t count, const int64_t* indptr, const int32_t* indices,
                                 const double* values, const int* d_indices, const double* d_values, double floor, double* ll_out,
                                 double* mass_out, int64_t* floored_out) {
    if (count == 0) return RRI_OK;
    std::fill(ll_out, ll_out + count, 0.0);
    std::fill(mass_out, mass_out + count, 0.0);
    std::fill(floored_out, floored_out + count, (int64_t)0);
    if (indptr[count] == 0) return RRI_OK;
    if (!c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    std::vector<LoglikChunk> chunks;
    loglik_cut_chunks(indptr, count, LL_UPLOAD_BUDGET, &chunks);
    i64 req_max = 0, ent_max = 0, pc_max = 0;
    for (const LoglikChunk& ch : chunks) {
        req_max = std::max<i64>(req_max, ch.q1 - ch.q0);
        ent_max = std::max<i64>(ent_max, indptr[ch.q1] - indptr[ch.q0]);
        pc_max = std::max<i64>(pc_max, loglik_cut_pieces(indptr, ch.q0, ch.q1, nullptr, nullptr));
    }
    if (req_max > 0x7fffffffLL) return fail(c, RRI_ERR_INVALID, "count %lld is too large for one call", (long long)count);
    HIPCHK(c, hipSetDevice(c->device));
    const int kp = loglik_kp(c->k);
    DevTmp tTt, trows, tpc, tfirst, tidx, tval, tpl, tpm, tpf, tll, tms, tfl;
    HIPCHK(c, tTt.alloc((size_t)c->d * kp * sizeof(double)));
    if (rows) HIPCHK(c, trows.alloc((size_t)req_max * sizeof(i64)));
    HIPCHK(c, tpc.alloc((size_t)pc_max * sizeof(LoglikPiece)));
    HIPCHK(c, tfirst.alloc((size_t)(req_max + 1) * sizeof(i64)));
    if (!d_indices) {
        HIPCHK(c, tidx.alloc((size_t)ent_max * sizeof(int)));
        HIPCHK(c, tval.alloc((size_t)ent_max * sizeof(double)));
    }
    HIPCHK(c, tpl.alloc((size_t)pc_max * sizeof(double)));
    HIPCHK(c, tpm.alloc((size_t)pc_max * sizeof(double)));
    HIPCHK(c, tpf.alloc((size_t)pc_max * sizeof(i64)));
    HIPCHK(c, tll.alloc((size_t)req_max * sizeof(double)));
    HIPCHK(c, tms.alloc((size_t)req_max * sizeof(double)));
    HIPCHK(c, tfl.alloc((size_t)req_max * sizeof(i64)));
    hipError_t e = LK::loglik_transpose(c, (double*)tTt.p);
    std::vector<LoglikPiece> pieces((size_t)pc_max);
    std::vector<int64_t> first((size_t)req_max + 1);
    for (size_t i = 0; i < chunks.size() && e == hipSuccess; ++i) {
        const i64 q0 = chunks[i].q0, nreq = chunks[i].q1 - q0, e0 = indptr[q0], nent = indptr[chunks[i].q1] - e0;
        if (nent == 0) continue;                                // only requests without entries: their outputs are 0 already
        const i64 npieces = loglik_cut_pieces(indptr, q0, chunks[i].q1, pieces.data(), first.data());
        if (rows) e = hipMemcpyAsync(trows.p, rows + q0, (size_t)nreq * sizeof(i64), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tpc.p, pieces.data(), (size_t)npieces * sizeof(LoglikPiece), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tfirst.p, first.data(), (size_t)(nreq + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && !d_indices) e = hipMemcpyAsync(tidx.p, indices + e0, (size_t)nent * sizeof(int), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && !d_indices) e = hipMemcpyAsync(tval.p, values + e0, (size_t)nent * sizeof(double), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess)
            e = LK::loglik_chunk(c, (const double*)tTt.p, (const i64*)trows.p, q0, nreq, (const LoglikPiece*)tpc.p, npieces,
                                 (const i64*)tfirst.p, d_indices ? d_indices + e0 : (const int*)tidx.p,
                                 d_indices ? d_values + e0 : (const double*)tval.p, floor, (double*)tpl.p,
                                 (double*)tpm.p, (i64*)tpf.p, (double*)tll.p, (double*)tms.p, (i64*)tfl.p);
        if (e == hipSuccess) e = hipMemcpyAsync(ll_out + q0, tll.p, (size_t)nreq * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(mass_out + q0, tms.p, (size_t)nreq * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(floored_out + q0, tfl.p, (size_t)nreq * sizeof(i64), hipMemcpyDeviceToHost, c->stream);
        // the pieces (host memory that the next chunk rewrites) have been read, and the temporaries are free for the next chunk
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "entries log-likelihood failed: %s", hipGetErrorString(e));
    return RRI_OK;
}

rri_status rri_entries_loglik(rri_ctx* c, const int64_t* rows, int64_t count, const int64_t* indptr, const int32_t* indices,
                              const double* values, double floor, double* ll_out, double* mass_out, int64_t* floored_out) {
    CHECK_CTX(c);
    char why[200] = "";
    const int bad = loglik_check_request(c->n, c->d, rows, count, indptr, indices, values, floor, ll_out, mass_out, floored_out, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    return loglik_entries(c, rows, count, indptr, indices, values, nullptr, nullptr, floor, ll_out, mass_out, floored_out);
}

// ---- a CSR corpus that lives on the device (rri_corpus.hpp has the semantics, rri_corpus_kernels.hpp the kernels) ----------------
// The canonical arrays belong to the corpus, not to a handle: rri_device_memory does not count them, rri_corpus_memory does.
struct rri_corpus {
    int device = 0;
    i64 n_rows = 0, n_cols = 0, stored = 0, nnz = 0, rewritten = 0, dup = 0, zeros = 0, neg = 0, long_rows = 0;
    i64* indptr = nullptr;       // n_rows + 1
    int* indices = nullptr;      // nnz
    double* values = nullptr;    // nnz
    size_t bytes = 0;
    std::vector<int64_t> h_indptr;   // the host's copy of the canonical indptr: the chunk and piece cutters run on it
    double ingest_ms = 0.0;
};
std::atomic<long long> g_corpora{0}, g_corpus_bytes{0};
// the corpora alive in the process: what rri_upload_X_corpus holds a caller's pointer against before it reads through it
std::mutex g_corpus_lock;
std::set<const rri_corpus*> g_corpus_alive;
bool corpus_alive(const rri_corpus* k) {
    std::lock_guard<std::mutex> hold(g_corpus_lock);
    return k && g_corpus_alive.count(k) != 0;
}

namespace {
// grid of a grid-stride kernel of 256 threads over `items`
unsigned corpus_grid(i64 items) { return (unsigned)std::max<i64>(1, std::min<i64>(8192, (items + 255) / 256)); }
size_t at_least(size_t bytes) { return bytes ? bytes : 8; }
}  // namespace

rri_status rri_corpus_create(rri_ctx* c, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* indptr,
                             int32_t indptr_dtype, const void* indices, int32_t indices_dtype, const void* values,
                             int32_t values_dtype, int32_t on_device) {
    CHECK_CTX(c);
    if (!out) return fail(c, RRI_ERR_INVALID, "the output pointer is NULL");
    *out = nullptr;
    const CorpusRaw raw{n_rows, n_cols, nnz, indptr, indptr_dtype, indices, indices_dtype, values, values_dtype};
    char why[200] = "";
    if (corpus_check_args(raw, why, sizeof why) != TOPN_REQ_OK) return fail(c, RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t psz = corpus_dtype_size(indptr_dtype), isz = corpus_dtype_size(indices_dtype), vsz = corpus_dtype_size(values_dtype);
    // the raw arrays on the device: the caller's own, or an upload as they are
    DevTmp rp, ri, rv;
    const void *dp = indptr, *di = indices, *dv = values;
    if (!on_device) {
        HIPCHK(c, rp.alloc((size_t)(n_rows + 1) * psz));
        HIPCHK(c, hipMemcpyAsync(rp.p, indptr, (size_t)(n_rows + 1) * psz, hipMemcpyHostToDevice, c->stream));
        dp = rp.p;
        if (nnz > 0) {
            HIPCHK(c, ri.alloc((size_t)nnz * isz));
            HIPCHK(c, hipMemcpyAsync(ri.p, indices, (size_t)nnz * isz, hipMemcpyHostToDevice, c->stream));
            di = ri.p;
            if (values) {
                HIPCHK(c, rv.alloc((size_t)nnz * vsz));
                HIPCHK(c, hipMemcpyAsync(rv.p, values, (size_t)nnz * vsz, hipMemcpyHostToDevice, c->stream));
                dv = rv.p;
            }
        }
    }
    const i64 words = (nnz + 63) / 64;
    DevTmp tstat, tzb, tdb, tptr, tflag, tclen;
    HIPCHK(c, tstat.alloc(CORPUS_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, tzb.alloc(at_least((size_t)words * sizeof(u64))));
    HIPCHK(c, tdb.alloc(at_least((size_t)words * sizeof(u64))));
    HIPCHK(c, tptr.alloc((size_t)(n_rows + 1) * sizeof(i64)));
    HIPCHK(c, tflag.alloc(at_least((size_t)n_rows)));
    HIPCHK(c, tclen.alloc(at_least((size_t)n_rows * sizeof(i64))));
    u64* stats = (u64*)tstat.p;
    HIPCHK(c, hipMemsetAsync(stats, 0xff, 8 * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(stats + 8, 0, 8 * sizeof(u64), c->stream));
    EventPair ev[4];          // the phases between two reads of the host: check, rows, copy and sorts, compaction
    int phases = 0;
    for (EventPair& p : ev) HIPCHK(c, p.create());
    u64 h_stat[CORPUS_STAT_WORDS];

    // 1. the check, by position only; nothing else runs before its verdict is read
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    hipLaunchKernelGGL(k_corpus_check, dim3(corpus_grid(std::max<i64>(nnz, n_rows + 1))), dim3(256), 0, c->stream, dp, (int)indptr_dtype, di,
                       (int)indices_dtype, dv, (int)values_dtype, (i64)n_rows, (i64)n_cols, (i64)nnz, stats, (u64*)tzb.p, (u64*)tdb.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat, stats, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int rule = 0; rule < 5; ++rule)
        if (h_stat[rule] != ~0ull) {           // the first broken rule at its smallest position; the offending number is one element
            const i64 pos = (i64)h_stat[rule];
            int64_t ival = 0;
            double dval = 0.0;
            unsigned char el[8] = {0};
            if (rule == 0 || rule == 2) {
                HIPCHK(c, hipMemcpy(el, (const char*)dp + (size_t)pos * psz, psz, hipMemcpyDeviceToHost));
                ival = corpus_idx(el, indptr_dtype, 0);
            } else if (rule == 3) {
                HIPCHK(c, hipMemcpy(el, (const char*)di + (size_t)pos * isz, isz, hipMemcpyDeviceToHost));
                ival = corpus_idx(el, indices_dtype, 0);
            } else if (rule == 4) {
                HIPCHK(c, hipMemcpy(el, (const char*)dv + (size_t)pos * vsz, vsz, hipMemcpyDeviceToHost));
                dval = corpus_val(el, values_dtype, 0);
            }
            corpus_rule_text(rule, pos, ival, dval, rule == 2 ? nnz : n_cols, why, sizeof why);
            return fail(c, RRI_ERR_INVALID, "%s", why);
        }
    if (n_cols > 0x7fffffffLL) {
        corpus_rule_text(5, 0, 0, 0.0, n_cols, why, sizeof why);
        return fail(c, RRI_ERR_UNSUPPORTED, "%s", why);
    }

    // 2. a flag and a stored length per row from the marks of the check; indptr as int64
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    hipLaunchKernelGGL(k_corpus_rows, dim3(corpus_grid(n_rows + 1)), dim3(256), 0, c->stream, dp, (int)indptr_dtype, (i64)n_rows,
                       (const u64*)tzb.p, (const u64*)tdb.p, (i64*)tptr.p, (unsigned char*)tflag.p, (i64*)tclen.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    std::vector<int64_t> h_ptr((size_t)n_rows + 1);
    std::vector<unsigned char> h_flag((size_t)n_rows);
    HIPCHK(c, hipMemcpyAsync(h_ptr.data(), tptr.p, (size_t)(n_rows + 1) * sizeof(i64), hipMemcpyDeviceToHost, c->stream));
    if (n_rows > 0) HIPCHK(c, hipMemcpyAsync(h_flag.data(), tflag.p, (size_t)n_rows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the rows to rewrite, by class, ascending: [short | medium by padded length | long], and the long rows' places in the key buffer
    std::vector<int64_t> list_short, list_long, keyoff;
    std::vector<std::vector<int64_t>> list_medium;          // [log2 of the padded length]
    i64 rewritten = 0, key_total = 0;
    for (i64 r = 0; r < n_rows; ++r) {
        const i64 len = h_ptr[(size_t)r + 1] - h_ptr[(size_t)r];
        const int cls = corpus_row_class(h_flag[(size_t)r] != 0, len);
        if (cls == CORPUS_ROW_CANONICAL) continue;
        ++rewritten;
        if (len > CORPUS_ROW_MAX) return fail(c, RRI_ERR_UNSUPPORTED, "row %lld has %lld stored entries and is not canonical: more than %lld are not rewritten", (long long)r, (long long)len, (long long)CORPUS_ROW_MAX);
        if (cls == CORPUS_ROW_SHORT) list_short.push_back(r);
        else if (cls == CORPUS_ROW_MEDIUM) {
            int lg = 0;
            while ((1ll << lg) < corpus_pad(len)) ++lg;
            if (list_medium.size() <= (size_t)lg) list_medium.resize((size_t)lg + 1);
            list_medium[(size_t)lg].push_back(r);
        } else {
            list_long.push_back(r);
            keyoff.push_back(key_total);
            key_total += corpus_pad(len);
        }
    }

    // 3. the converting copy: the corpus itself when no row is to be rewritten, the staging otherwise
    DevTmp sidx, sval;
    HIPCHK(c, sidx.alloc(at_least((size_t)nnz * sizeof(int))));
    HIPCHK(c, sval.alloc(at_least((size_t)nnz * sizeof(double))));
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_corpus_copy, dim3(corpus_grid(nnz)), dim3(256), 0, c->stream, di, (int)indices_dtype, dv, (int)values_dtype,
                           (i64)nnz, (int*)sidx.p, (double*)sval.p, rewritten ? (u64*)nullptr : stats + CORPUS_STAT_NEG);
        HIPCHK(c, hipGetLastError());
    }
    DevTmp tlist, tkoff, tkeys, fptr, fidx, fval;
    std::vector<int64_t> h_cptr;
    i64 nnz_c = nnz;
    if (rewritten) {
        // 4. sort and merge the flagged rows into the staging, each at its raw offset
        std::vector<int64_t> all(list_short);
        for (const auto& l : list_medium) all.insert(all.end(), l.begin(), l.end());
        all.insert(all.end(), list_long.begin(), list_long.end());
        HIPCHK(c, tlist.alloc(all.size() * sizeof(i64)));
        HIPCHK(c, hipMemcpyAsync(tlist.p, all.data(), all.size() * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        const i64* dl = (const i64*)tlist.p;
        if (!list_short.empty()) {
            hipLaunchKernelGGL(k_corpus_sort_wave, dim3((unsigned)((list_short.size() + 3) / 4)), dim3(256), 0, c->stream, dl,
                               (i64)list_short.size(), (const i64*)tptr.p, di, (int)indices_dtype, dv, (int)values_dtype, (int*)sidx.p,
                               (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
        }
        dl += list_short.size();
        HIPCHK(c, allow_lds<k_corpus_sort_block<true>>(c, CORPUS_LDS_MAX * (int)sizeof(u64)));
        for (size_t lg = 0; lg < list_medium.size(); ++lg) {
            const size_t cnt = list_medium[lg].size();
            if (!cnt) continue;
            const i64 P = 1ll << lg;
            hipLaunchKernelGGL(k_corpus_sort_block<true>, dim3((unsigned)cnt), dim3(P <= 1024 ? 256 : 1024), (size_t)P * sizeof(u64), c->stream,
                               dl, (const i64*)nullptr, (u64*)nullptr, P, (const i64*)tptr.p, di, (int)indices_dtype, dv, (int)values_dtype,
                               (int*)sidx.p, (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
            dl += cnt;
        }
        if (!list_long.empty()) {
            HIPCHK(c, tkoff.alloc(keyoff.size() * sizeof(i64)));
            HIPCHK(c, tkeys.alloc((size_t)key_total * sizeof(u64)));
            HIPCHK(c, hipMemcpyAsync(tkoff.p, keyoff.data(), keyoff.size() * sizeof(i64), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_corpus_sort_block<false>, dim3((unsigned)list_long.size()), dim3(1024), 0, c->stream, dl, (const i64*)tkoff.p,
                               (u64*)tkeys.p, (i64)0, (const i64*)tptr.p, di, (int)indices_dtype, dv, (int)values_dtype, (int*)sidx.p,
                               (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
        // 5. the canonical lengths go to the host, which takes the prefix sum; the final arrays are written once
        std::vector<int64_t> h_len((size_t)n_rows);
        HIPCHK(c, hipMemcpyAsync(h_len.data(), tclen.p, (size_t)n_rows * sizeof(i64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));       // (the lists, host memory of this call, have been read by now too)
        h_cptr.assign((size_t)n_rows + 1, 0);
        for (i64 r = 0; r < n_rows; ++r) h_cptr[(size_t)r + 1] = h_cptr[(size_t)r] + h_len[(size_t)r];
        nnz_c = h_cptr[(size_t)n_rows];
        HIPCHK(c, fptr.alloc((size_t)(n_rows + 1) * sizeof(i64)));
        HIPCHK(c, fidx.alloc(at_least((size_t)nnz_c * sizeof(int))));
        HIPCHK(c, fval.alloc(at_least((size_t)nnz_c * sizeof(double))));
        HIPCHK(c, hipMemcpyAsync(fptr.p, h_cptr.data(), (size_t)(n_rows + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
        if (nnz_c > 0) {
            hipLaunchKernelGGL(k_corpus_compact, dim3(corpus_grid(nnz_c)), dim3(256), 0, c->stream, (const i64*)fptr.p, (const i64*)tptr.p,
                               (i64)n_rows, nnz_c, (const int*)sidx.p, (const double*)sval.p, (int*)fidx.p, (double*)fval.p,
                               stats + CORPUS_STAT_NEG);
            HIPCHK(c, hipGetLastError());
        }
    } else {
        h_cptr = h_ptr;
    }
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat, stats, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (int i = 0; i < phases; ++i) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, ev[i].a, ev[i].b));
        ms += t;
    }
    rri_corpus* k = new rri_corpus();
    DevTmp &optr = rewritten ? fptr : tptr, &oidx = rewritten ? fidx : sidx, &oval = rewritten ? fval : sval;
    k->device = c->device;
    k->n_rows = n_rows; k->n_cols = n_cols; k->stored = nnz; k->nnz = nnz_c; k->rewritten = rewritten;
    k->dup = (i64)h_stat[CORPUS_STAT_DUP]; k->zeros = (i64)h_stat[CORPUS_STAT_ZERO]; k->neg = (i64)h_stat[CORPUS_STAT_NEG];
    k->long_rows = (i64)list_long.size();
    k->indptr = (i64*)optr.p; k->indices = (int*)oidx.p; k->values = (double*)oval.p;
    k->bytes = optr.bytes + oidx.bytes + oval.bytes;
    optr.p = oidx.p = oval.p = nullptr;                      // the corpus owns them from here on
    k->h_indptr = std::move(h_cptr);
    k->ingest_ms = ms;
    g_corpora += 1;
    g_corpus_bytes += (long long)k->bytes;
    {
        std::lock_guard<std::mutex> hold(g_corpus_lock);
        g_corpus_alive.insert(k);
    }
    *out = k;
    return RRI_OK;
}

rri_status rri_corpus_destroy(rri_corpus* k) {
    if (!k) return RRI_ERR_INVALID;
    {
        std::lock_guard<std::mutex> hold(g_corpus_lock);
        g_corpus_alive.erase(k);
    }
    int before = 0;
    const bool had = hipGetDevice(&before) == hipSuccess;
    (void)hipSetDevice(k->device);
    (void)hipFree(k->indptr);
    (void)hipFree(k->indices);
    (void)hipFree(k->values);
    if (had) (void)hipSetDevice(before);
    g_corpora -= 1;
    g_corpus_bytes -= (long long)k->bytes;
    delete k;
    return RRI_OK;
}

rri_status rri_corpus_info(const rri_corpus* k, int64_t* out, int32_t n, double* ingest_ms) {
    if (!k || (n > 0 && !out) || n < 0) return RRI_ERR_INVALID;
    const int64_t f[RRI_CORPUS_INFO_FIELDS] = {k->n_rows, k->n_cols, k->stored, k->nnz, k->rewritten, k->dup, k->zeros, k->neg,
                                               (int64_t)k->bytes, k->long_rows};
    for (int i = 0; i < n && i < RRI_CORPUS_INFO_FIELDS; ++i) out[i] = f[i];
    for (int i = RRI_CORPUS_INFO_FIELDS; i < n; ++i) out[i] = 0;
    if (ingest_ms) *ingest_ms = k->ingest_ms;
    return RRI_OK;
}

rri_status rri_corpus_memory(int64_t* corpora, int64_t* bytes) {
    if (corpora) *corpora = g_corpora.load();
    if (bytes) *bytes = g_corpus_bytes.load();
    return RRI_OK;
}

// the handle gives the device, the stream and the error text; the corpus must live on the handle's device
#define CHECK_CORPUS(c, k)                                                                                              \
    do {                                                                                                                \
        CHECK_CTX(c);                                                                                                   \
        if (!(k)) return fail((c), RRI_ERR_INVALID, "the corpus is NULL");                                              \
        if ((k)->device != (c)->device)                                                                                 \
            return fail((c), RRI_ERR_INVALID, "the corpus lives on device %d, the handle on device %d", (k)->device, (c)->device); \
    } while (0)

rri_status rri_corpus_get(rri_ctx* c, const rri_corpus* k, int64_t* indptr_out, int32_t* indices_out, double* values_out) {
    CHECK_CORPUS(c, k);
    HIPCHK(c, hipSetDevice(c->device));
    if (indptr_out) std::copy(k->h_indptr.begin(), k->h_indptr.end(), indptr_out);
    if (indices_out && k->nnz > 0) HIPCHK(c, hipMemcpyAsync(indices_out, k->indices, (size_t)k->nnz * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (values_out && k->nnz > 0) HIPCHK(c, hipMemcpyAsync(values_out, k->values, (size_t)k->nnz * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_corpus_cooccurrence_counts(rri_ctx* c, const rri_corpus* k, const int32_t* words, int32_t n_groups, int32_t group_size,
                                          int64_t* df_out, int64_t* codf_out) {
    CHECK_CORPUS(c, k);
    char why[200] = "";
    const int bad = cooc_check_groups(k->n_cols, words, n_groups, group_size, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    return cooc_counts(c, nullptr, nullptr, k->indptr, k->indices, k->n_rows, k->n_cols, k->nnz, words, n_groups, group_size, df_out,
                       codf_out);
}

rri_status rri_corpus_entries_loglik(rri_ctx* c, const rri_corpus* k, const int64_t* rows, double floor, double* ll_out,
                                     double* mass_out, int64_t* floored_out) {
    CHECK_CORPUS(c, k);
    if (!(floor >= 0.0) || std::isinf(floor)) return fail(c, RRI_ERR_INVALID, "floor %g is not a finite number >= 0", floor);
    if (LL_ENTRY_BYTES * c->d > LL_UPLOAD_BUDGET)
        return fail(c, RRI_ERR_UNSUPPORTED, "a full row of d = %lld entries does not fit the upload budget of %lld bytes", (long long)c->d, (long long)LL_UPLOAD_BUDGET);
    if (k->n_cols != c->d) return fail(c, RRI_ERR_INVALID, "the corpus has %lld columns, W T has %lld", (long long)k->n_cols, (long long)c->d);
    if (k->neg > 0) return fail(c, RRI_ERR_INVALID, "the corpus holds %lld negative values: counts are finite and >= 0", (long long)k->neg);
    const i64 count = k->n_rows;
    if (!rows && count > c->n) return fail(c, RRI_ERR_INVALID, "rows is NULL and count %lld exceeds the %lld rows of W", (long long)count, (long long)c->n);
    if (count > 0 && (!ll_out || !mass_out || !floored_out)) return fail(c, RRI_ERR_INVALID, "an output array is NULL with %lld requests", (long long)count);
    for (i64 q = 0; rows && q < count; ++q)
        if (rows[q] < 0 || rows[q] >= c->n) return fail(c, RRI_ERR_INVALID, "rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
    return loglik_entries(c, rows, count, k->h_indptr.data(), nullptr, nullptr, k->indices, k->values, floor, ll_out, mass_out, floored_out);
}

// ---- corpora derived from a resident corpus (rri_derive.hpp has the semantics, rri_derive_kernels.hpp the kernels) ----------------
namespace {
// grid of a kernel that gives a wave to a piece, four pieces per workgroup, wave-stride beyond
unsigned derive_grid(i64 pieces) { return (unsigned)std::max<i64>(1, std::min<i64>(16384, (pieces + 3) / 4)); }
hipError_t derive_upload_bytes(DevTmp& t, const void* data, size_t bytes, hipStream_t s) {
    const hipError_t e = t.alloc(at_least(bytes));
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpyAsync(t.p, data, bytes, hipMemcpyHostToDevice, s);
}
// a host vector into a temporary of its own size (at least 8 bytes); the vector outlives the call's next synchronisation
#define derive_upload(t, v, s) derive_upload_bytes((t), (v).data(), (v).size() * sizeof((v)[0]), (s))
// the three arrays become a corpus that owns them; no HIP call, nothing fails in here
rri_corpus* corpus_adopt(int device, i64 n_rows, i64 n_cols, i64 nnz, i64 neg, DevTmp& ptr, DevTmp& idx, DevTmp& val,
                         std::vector<int64_t>&& h_ptr, double ms) {
    rri_corpus* k = new rri_corpus();
    k->device = device;
    k->n_rows = n_rows; k->n_cols = n_cols; k->stored = nnz; k->nnz = nnz; k->neg = neg;
    k->indptr = (i64*)ptr.p; k->indices = (int*)idx.p; k->values = (double*)val.p;
    k->bytes = ptr.bytes + idx.bytes + val.bytes;
    ptr.p = idx.p = val.p = nullptr;
    k->h_indptr = std::move(h_ptr);
    k->ingest_ms = ms;
    g_corpora += 1;
    g_corpus_bytes += (long long)k->bytes;
    std::lock_guard<std::mutex> hold(g_corpus_lock);
    g_corpus_alive.insert(k);
    return k;
}
// the output offset of every piece and the indptr of the output from the pieces' counts: the pieces stand in output order
void derive_offsets(const DerivePieces& pieces, const std::vector<int>& cnt, i64 rows_out, std::vector<int64_t>* piece_out,
                    std::vector<int64_t>* indptr) {
    piece_out->assign(pieces.row.size(), 0);
    indptr->assign((size_t)rows_out + 1, 0);
    i64 total = 0;
    for (size_t p = 0; p < pieces.row.size(); ++p) {
        (*piece_out)[p] = total;
        total += cnt[p];
        (*indptr)[(size_t)pieces.row[p] + 1] += cnt[p];
    }
    for (i64 r = 0; r < rows_out; ++r) (*indptr)[(size_t)r + 1] += (*indptr)[(size_t)r];
}
}  // namespace

#define CHECK_DERIVE_CORPUS(c, k)                                                                                      \
    do {                                                                                                               \
        const bool alive_ = corpus_alive(k);                                                                           \
        char why_[200] = "";                                                                                           \
        if (derive_check_corpus(alive_, alive_ ? (k)->device : 0, (c)->device, why_, sizeof why_) != TOPN_REQ_OK)      \
            return fail((c), RRI_ERR_INVALID, "%s", why_);                                                             \
    } while (0)

rri_status rri_corpus_select(rri_ctx* c, const rri_corpus* k, const int64_t* rows, int64_t m, const int32_t* keep, int64_t dk,
                             rri_corpus** out) {
    CHECK_CTX(c);
    if (!out) return fail(c, RRI_ERR_INVALID, "the output pointer is NULL");
    *out = nullptr;
    CHECK_DERIVE_CORPUS(c, k);
    char why[200] = "";
    if (derive_check_select(k->n_rows, k->n_cols, rows, m, keep, dk, why, sizeof why) != TOPN_REQ_OK) return fail(c, RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const i64 rows_out = rows ? m : k->n_rows, cols_out = keep ? dk : k->n_cols;
    const DerivePieces pieces = derive_cut_pieces(k->h_indptr.data(), k->n_rows, rows, m);
    const i64 np = (i64)pieces.row.size();
    DevTmp tsrc, tlen, tmap, tcnt, tout, tstat, optr, oidx, oval;
    EventPair ev[2];
    for (EventPair& p : ev) HIPCHK(c, p.create());
    HIPCHK(c, derive_upload(tsrc, pieces.src, c->stream));
    HIPCHK(c, derive_upload(tlen, pieces.len, c->stream));
    HIPCHK(c, tstat.alloc(DERIVE_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, hipMemsetAsync(tstat.p, 0, DERIVE_STAT_WORDS * sizeof(u64), c->stream));
    std::vector<int> cnt(pieces.len);              // without keep a piece keeps all it has
    std::vector<int> map;
    HIPCHK(c, hipEventRecord(ev[0].a, c->stream));
    if (keep) {
        map.assign((size_t)k->n_cols, -1);
        for (i64 j = 0; j < dk; ++j) map[(size_t)keep[j]] = (int)j;
        HIPCHK(c, derive_upload(tmap, map, c->stream));
        HIPCHK(c, tcnt.alloc(at_least((size_t)np * sizeof(int))));
        if (np > 0) {
            hipLaunchKernelGGL(k_derive_count, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)tsrc.p, (const int*)tlen.p, np,
                               (const int*)k->indices, (const int*)tmap.p, (int*)tcnt.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(cnt.data(), tcnt.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipEventRecord(ev[0].b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int64_t> piece_out, h_ptr;
    derive_offsets(pieces, cnt, rows_out, &piece_out, &h_ptr);
    const i64 nnz_o = h_ptr[(size_t)rows_out];
    HIPCHK(c, derive_upload(tout, piece_out, c->stream));
    HIPCHK(c, derive_upload(optr, h_ptr, c->stream));
    HIPCHK(c, oidx.alloc(at_least((size_t)nnz_o * sizeof(int))));
    HIPCHK(c, oval.alloc(at_least((size_t)nnz_o * sizeof(double))));
    HIPCHK(c, hipEventRecord(ev[1].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_derive_write, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)tsrc.p, (const int*)tlen.p,
                           (const i64*)tout.p, np, (const int*)k->indices, (const double*)k->values, keep ? (const int*)tmap.p : (const int*)nullptr,
                           (int*)oidx.p, (double*)oval.p, (u64*)tstat.p + DERIVE_STAT_NEG);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[1].b, c->stream));
    u64 h_stat[DERIVE_STAT_WORDS];
    HIPCHK(c, hipMemcpyAsync(h_stat, tstat.p, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (EventPair& p : ev) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t;
    }
    *out = corpus_adopt(c->device, rows_out, cols_out, nnz_o, (i64)h_stat[DERIVE_STAT_NEG], optr, oidx, oval, std::move(h_ptr), ms);
    return RRI_OK;
}

rri_status rri_corpus_column_counts(rri_ctx* c, const rri_corpus* k, int64_t* df_out) {
    CHECK_CTX(c);
    CHECK_DERIVE_CORPUS(c, k);
    if (!df_out && k->n_cols > 0) return fail(c, RRI_ERR_INVALID, "the output pointer is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    if (k->n_cols == 0) return RRI_OK;
    DevTmp tdf;
    HIPCHK(c, tdf.alloc((size_t)k->n_cols * sizeof(u64)));
    HIPCHK(c, hipMemsetAsync(tdf.p, 0, (size_t)k->n_cols * sizeof(u64), c->stream));
    if (k->nnz > 0) {
        hipLaunchKernelGGL(k_derive_column_counts, dim3(corpus_grid(k->nnz)), dim3(256), 0, c->stream, (const int*)k->indices, k->nnz, (u64*)tdf.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(df_out, tdf.p, (size_t)k->n_cols * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_corpus_split(rri_ctx* c, const rri_corpus* k, uint32_t thr, uint64_t seed, rri_corpus** observed, rri_corpus** held) {
    CHECK_CTX(c);
    if (observed) *observed = nullptr;
    if (held) *held = nullptr;
    char why[200] = "";
    if (!observed || !held) return derive_check_split(thr, observed != nullptr, held != nullptr, why, sizeof why), fail(c, RRI_ERR_INVALID, "%s", why);
    CHECK_DERIVE_CORPUS(c, k);
    if (derive_check_split(thr, true, true, why, sizeof why) != TOPN_REQ_OK) return fail(c, RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const i64 nnz = k->nnz;
    DevTmp tstat;
    EventPair ev[3];
    for (EventPair& p : ev) HIPCHK(c, p.create());
    HIPCHK(c, tstat.alloc(DERIVE_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, hipMemsetAsync(tstat.p, 0xff, DERIVE_STAT_WORDS * sizeof(u64), c->stream));
    // 1. the values are counts; nothing of the outputs exists before this verdict
    HIPCHK(c, hipEventRecord(ev[0].a, c->stream));
    if (nnz > 0) {
        hipLaunchKernelGGL(k_split_check, dim3(corpus_grid(nnz)), dim3(256), 0, c->stream, (const double*)k->values, nnz, (u64*)tstat.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[0].b, c->stream));
    u64 h_stat[DERIVE_STAT_WORDS];
    HIPCHK(c, hipMemcpyAsync(h_stat, tstat.p, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int rule = 0; rule < SPLIT_RULES; ++rule)
        if (h_stat[rule] != ~0ull) {
            const i64 pos = (i64)h_stat[rule];
            double v = 0.0;
            HIPCHK(c, hipMemcpy(&v, k->values + pos, sizeof v, hipMemcpyDeviceToHost));
            split_rule_text(rule, pos, v, why, sizeof why);
            return fail(c, split_rule_code(rule) == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
        }
    // 2. pass A: the held part of every entry, and what every piece leaves on either side
    const DerivePieces pieces = derive_cut_pieces(k->h_indptr.data(), k->n_rows, nullptr, 0);
    const i64 np = (i64)pieces.row.size();
    DevTmp trow, tsrc, tlen, theld, tnh, tno, toh, too, hptr, hidx, hval, optr, oidx, oval;
    HIPCHK(c, derive_upload(trow, pieces.row, c->stream));
    HIPCHK(c, derive_upload(tsrc, pieces.src, c->stream));
    HIPCHK(c, derive_upload(tlen, pieces.len, c->stream));
    HIPCHK(c, theld.alloc(at_least((size_t)nnz * sizeof(int))));
    HIPCHK(c, tnh.alloc(at_least((size_t)np * sizeof(int))));
    HIPCHK(c, tno.alloc(at_least((size_t)np * sizeof(int))));
    std::vector<int> nh((size_t)np), no((size_t)np);
    HIPCHK(c, hipEventRecord(ev[1].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_split_held, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)trow.p, (const i64*)tsrc.p, (const int*)tlen.p, np,
                           (const int*)k->indices, (const double*)k->values, (unsigned)thr, (u64)seed, (int*)theld.p, (int*)tnh.p, (int*)tno.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(nh.data(), tnh.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(no.data(), tno.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(ev[1].b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // 3. the prefix sums on the host, then pass B writes both outputs once
    std::vector<int64_t> piece_oh, piece_oo, h_hptr, h_optr;
    derive_offsets(pieces, nh, k->n_rows, &piece_oh, &h_hptr);
    derive_offsets(pieces, no, k->n_rows, &piece_oo, &h_optr);
    const i64 nnz_h = h_hptr[(size_t)k->n_rows], nnz_o = h_optr[(size_t)k->n_rows];
    HIPCHK(c, derive_upload(toh, piece_oh, c->stream));
    HIPCHK(c, derive_upload(too, piece_oo, c->stream));
    HIPCHK(c, derive_upload(hptr, h_hptr, c->stream));
    HIPCHK(c, derive_upload(optr, h_optr, c->stream));
    HIPCHK(c, hidx.alloc(at_least((size_t)nnz_h * sizeof(int))));
    HIPCHK(c, hval.alloc(at_least((size_t)nnz_h * sizeof(double))));
    HIPCHK(c, oidx.alloc(at_least((size_t)nnz_o * sizeof(int))));
    HIPCHK(c, oval.alloc(at_least((size_t)nnz_o * sizeof(double))));
    HIPCHK(c, hipEventRecord(ev[2].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_split_write, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)tsrc.p, (const int*)tlen.p, (const i64*)toh.p,
                           (const i64*)too.p, np, (const int*)k->indices, (const double*)k->values, (const int*)theld.p, (int*)hidx.p,
                           (double*)hval.p, (int*)oidx.p, (double*)oval.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[2].b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (EventPair& p : ev) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t;
    }
    *observed = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_o, 0, optr, oidx, oval, std::move(h_optr), ms);
    *held = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_h, 0, hptr, hidx, hval, std::move(h_hptr), ms);
    return RRI_OK;
}

// ---- a corpus from pairs, a split by entry (rri_corpus_build.hpp has the semantics, rri_corpus_build_kernels.hpp the kernels) ------
rri_status rri_corpus_from_pairs(rri_ctx* c, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t n_pairs, const void* rows,
                                 const void* cols, int32_t index_dtype, int64_t index_stride, const void* values,
                                 int32_t values_dtype, int32_t on_device) {
    CHECK_CTX(c);
    if (!out) return fail(c, RRI_ERR_INVALID, "the output pointer is NULL");
    *out = nullptr;
    const CorpusPairs req{n_rows, n_cols, n_pairs, rows, cols, index_dtype, index_stride, values, values_dtype};
    char why[200] = "";
    const int bad = pairs_check_args(req, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t isz = corpus_dtype_size(index_dtype), vsz = corpus_dtype_size(values_dtype);
    const i64 stride = index_stride;
    // the arrays on the device: the caller's own, or an upload as they lie -- an interleaved pair of index arrays travels once
    DevTmp ra, rb, rv;
    const void *dr = rows, *dc = cols, *dv = values;
    if (!on_device && n_pairs > 0) {
        const size_t span = ((size_t)(n_pairs - 1) * (size_t)stride + 1) * isz;
        const uintptr_t r0 = (uintptr_t)rows, c0 = (uintptr_t)cols, lo = std::min(r0, c0), hi = std::max(r0, c0) + span;
        if (std::max(r0, c0) - lo < span) {            // the two spans overlap: one upload covers both
            HIPCHK(c, ra.alloc(hi - lo));
            HIPCHK(c, hipMemcpyAsync(ra.p, (const void*)lo, hi - lo, hipMemcpyHostToDevice, c->stream));
            dr = (const char*)ra.p + (r0 - lo);
            dc = (const char*)ra.p + (c0 - lo);
        } else {
            HIPCHK(c, ra.alloc(span));
            HIPCHK(c, rb.alloc(span));
            HIPCHK(c, hipMemcpyAsync(ra.p, rows, span, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(rb.p, cols, span, hipMemcpyHostToDevice, c->stream));
            dr = ra.p;
            dc = rb.p;
        }
        if (values) {
            HIPCHK(c, rv.alloc((size_t)n_pairs * vsz));
            HIPCHK(c, hipMemcpyAsync(rv.p, values, (size_t)n_pairs * vsz, hipMemcpyHostToDevice, c->stream));
            dv = rv.p;
        }
    }
    DevTmp tstat, tcnt, tfill, tptr, tslots, tclen, sidx, sval;
    HIPCHK(c, tstat.alloc(CORPUS_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, tcnt.alloc(at_least((size_t)n_rows * sizeof(unsigned))));
    u64* stats = (u64*)tstat.p;
    HIPCHK(c, hipMemsetAsync(stats, 0xff, 8 * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(stats + 8, 0, 8 * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(tcnt.p, 0, at_least((size_t)n_rows * sizeof(unsigned)), c->stream));
    EventPair ev[4];          // the phases between two reads of the host: check, count, claim and sorts, compaction
    int phases = 0;
    for (EventPair& p : ev) HIPCHK(c, p.create());
    u64 h_stat[CORPUS_STAT_WORDS];
    const dim3 pgrid(pairs_grid(n_pairs));

    // 1. the check, by position only; nothing else runs before its verdict is read
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_pairs_check, pgrid, dim3(256), 0, c->stream, dr, dc, (int)index_dtype, stride, dv, (int)values_dtype,
                           (i64)n_rows, (i64)n_cols, (i64)n_pairs, stats);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat, stats, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int rule = 0; rule < CB_RULES; ++rule)
        if (h_stat[rule] != ~0ull) {           // the first broken rule at its smallest position; the offending number is one element
            const i64 pos = (i64)h_stat[rule];
            int64_t ival = 0;
            double dval = 0.0;
            unsigned char el[8] = {0};
            if (rule < 2) {
                HIPCHK(c, hipMemcpy(el, (const char*)(rule == 0 ? dr : dc) + (size_t)pos * (size_t)stride * isz, isz, hipMemcpyDeviceToHost));
                ival = corpus_idx(el, index_dtype, 0);
            } else {
                HIPCHK(c, hipMemcpy(el, (const char*)dv + (size_t)pos * vsz, vsz, hipMemcpyDeviceToHost));
                dval = corpus_val(el, values_dtype, 0);
            }
            pairs_rule_text(rule, pos, ival, dval, why, sizeof why);
            return fail(c, RRI_ERR_INVALID, "%s", why);
        }

    // 2. the pairs of every row, one integer atomic per run of equal rows inside a wave; the host takes the exclusive scan
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_pairs_count, pgrid, dim3(256), 0, c->stream, dr, (int)index_dtype, stride, (i64)n_pairs, (unsigned*)tcnt.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    std::vector<unsigned> h_cnt((size_t)n_rows);
    if (n_rows > 0) HIPCHK(c, hipMemcpyAsync(h_cnt.data(), tcnt.p, (size_t)n_rows * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int64_t> h_ptr((size_t)n_rows + 1, 0);
    // every row with a pair is sorted, by class, ascending: [short | medium by padded length | long], and the long rows' places in the key buffer
    std::vector<int64_t> list_short, list_long, keyoff;
    std::vector<std::vector<int64_t>> list_medium;          // [log2 of the padded length]
    i64 key_total = 0;
    for (i64 r = 0; r < n_rows; ++r) {
        const i64 len = h_cnt[(size_t)r];
        h_ptr[(size_t)r + 1] = h_ptr[(size_t)r] + len;
        if (len == 0) continue;
        if (len > CORPUS_ROW_MAX) return fail(c, RRI_ERR_UNSUPPORTED, "row %lld has %lld pairs: more than %lld are not sorted", (long long)r, (long long)len, (long long)CORPUS_ROW_MAX);
        const int cls = corpus_row_class(true, len);
        if (cls == CORPUS_ROW_SHORT) list_short.push_back(r);
        else if (cls == CORPUS_ROW_MEDIUM) {
            int lg = 0;
            while ((1ll << lg) < corpus_pad(len)) ++lg;
            if (list_medium.size() <= (size_t)lg) list_medium.resize((size_t)lg + 1);
            list_medium[(size_t)lg].push_back(r);
        } else {
            list_long.push_back(r);
            keyoff.push_back(key_total);
            key_total += corpus_pad(len);
        }
    }
    if (h_ptr[(size_t)n_rows] != n_pairs) return fail(c, RRI_ERR_HIP, "the rows' counts add up to %lld, not to the %lld pairs", (long long)h_ptr[(size_t)n_rows], (long long)n_pairs);

    // 3. every pair claims a slot of its row; every row is sorted by (column, pair position) and merged into the staging at its raw offset
    DevTmp tlist, tkoff, tkeys, fptr, fidx, fval;
    HIPCHK(c, derive_upload(tptr, h_ptr, c->stream));
    HIPCHK(c, tfill.alloc(at_least((size_t)n_rows * sizeof(unsigned))));
    HIPCHK(c, tslots.alloc(at_least((size_t)n_pairs * sizeof(unsigned))));
    HIPCHK(c, tclen.alloc(at_least((size_t)n_rows * sizeof(i64))));
    HIPCHK(c, sidx.alloc(at_least((size_t)n_pairs * sizeof(int))));
    HIPCHK(c, sval.alloc(at_least((size_t)n_pairs * sizeof(double))));
    HIPCHK(c, hipMemsetAsync(tfill.p, 0, at_least((size_t)n_rows * sizeof(unsigned)), c->stream));
    HIPCHK(c, hipMemsetAsync(tclen.p, 0, at_least((size_t)n_rows * sizeof(i64)), c->stream));
    std::vector<int64_t> all(list_short);
    for (const auto& l : list_medium) all.insert(all.end(), l.begin(), l.end());
    all.insert(all.end(), list_long.begin(), list_long.end());
    HIPCHK(c, derive_upload(tlist, all, c->stream));
    HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_pairs_claim, pgrid, dim3(256), 0, c->stream, dr, (int)index_dtype, stride, (i64)n_pairs, (const i64*)tptr.p,
                           (unsigned*)tfill.p, (unsigned*)tslots.p);
        HIPCHK(c, hipGetLastError());
        const i64* dl = (const i64*)tlist.p;
        if (!list_short.empty()) {
            hipLaunchKernelGGL(k_pairs_sort_wave, dim3((unsigned)((list_short.size() + 3) / 4)), dim3(256), 0, c->stream, dl,
                               (i64)list_short.size(), (const i64*)tptr.p, (const unsigned*)tslots.p, dc, (int)index_dtype, stride, dv,
                               (int)values_dtype, (int*)sidx.p, (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
        }
        dl += list_short.size();
        HIPCHK(c, allow_lds<k_pairs_sort_block<true>>(c, CORPUS_LDS_MAX * (int)sizeof(u64)));
        for (size_t lg = 0; lg < list_medium.size(); ++lg) {
            const size_t cnt = list_medium[lg].size();
            if (!cnt) continue;
            const i64 P = 1ll << lg;
            hipLaunchKernelGGL(k_pairs_sort_block<true>, dim3((unsigned)cnt), dim3(P <= 1024 ? 256 : 1024), (size_t)P * sizeof(u64), c->stream,
                               dl, (const i64*)nullptr, (u64*)nullptr, P, (const i64*)tptr.p, (const unsigned*)tslots.p, dc, (int)index_dtype,
                               stride, dv, (int)values_dtype, (int*)sidx.p, (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
            dl += cnt;
        }
        if (!list_long.empty()) {
            HIPCHK(c, derive_upload(tkoff, keyoff, c->stream));
            HIPCHK(c, tkeys.alloc((size_t)key_total * sizeof(u64)));
            hipLaunchKernelGGL(k_pairs_sort_block<false>, dim3((unsigned)list_long.size()), dim3(1024), 0, c->stream, dl, (const i64*)tkoff.p,
                               (u64*)tkeys.p, (i64)0, (const i64*)tptr.p, (const unsigned*)tslots.p, dc, (int)index_dtype, stride, dv,
                               (int)values_dtype, (int*)sidx.p, (double*)sval.p, (i64*)tclen.p, stats);
            HIPCHK(c, hipGetLastError());
        }
    }
    HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_stat, stats, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // (the lists, host memory of this call, have been read by now too)
    const bool shorter = h_stat[CORPUS_STAT_DUP] + h_stat[CORPUS_STAT_ZERO] > 0;
    std::vector<int64_t> h_cptr;
    i64 nnz_c = n_pairs;
    if (shorter) {
        // 4. a row became shorter: the canonical lengths go to the host, which takes the prefix sum; the final arrays are written once
        std::vector<int64_t> h_len((size_t)n_rows);
        HIPCHK(c, hipMemcpy(h_len.data(), tclen.p, (size_t)n_rows * sizeof(i64), hipMemcpyDeviceToHost));
        h_cptr.assign((size_t)n_rows + 1, 0);
        for (i64 r = 0; r < n_rows; ++r) h_cptr[(size_t)r + 1] = h_cptr[(size_t)r] + h_len[(size_t)r];
        nnz_c = h_cptr[(size_t)n_rows];
        HIPCHK(c, derive_upload(fptr, h_cptr, c->stream));
        HIPCHK(c, fidx.alloc(at_least((size_t)nnz_c * sizeof(int))));
        HIPCHK(c, fval.alloc(at_least((size_t)nnz_c * sizeof(double))));
        HIPCHK(c, hipEventRecord(ev[phases].a, c->stream));
        if (nnz_c > 0) {
            hipLaunchKernelGGL(k_corpus_compact, dim3(corpus_grid(nnz_c)), dim3(256), 0, c->stream, (const i64*)fptr.p, (const i64*)tptr.p,
                               (i64)n_rows, nnz_c, (const int*)sidx.p, (const double*)sval.p, (int*)fidx.p, (double*)fval.p,
                               stats + PAIRS_STAT_SCRATCH);          // the negatives were counted where the sums were formed
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipEventRecord(ev[phases++].b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        h_cptr = h_ptr;
    }
    double ms = 0.0;
    for (int i = 0; i < phases; ++i) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, ev[i].a, ev[i].b));
        ms += t;
    }
    rri_corpus* k = corpus_adopt(c->device, n_rows, n_cols, nnz_c, (i64)h_stat[CORPUS_STAT_NEG], shorter ? fptr : tptr, shorter ? fidx : sidx,
                                 shorter ? fval : sval, std::move(h_cptr), ms);
    k->stored = n_pairs;
    k->rewritten = (i64)h_stat[PAIRS_STAT_REWRITTEN];
    k->dup = (i64)h_stat[CORPUS_STAT_DUP];
    k->zeros = (i64)h_stat[CORPUS_STAT_ZERO];
    k->long_rows = (i64)h_stat[PAIRS_STAT_LONG];
    *out = k;
    return RRI_OK;
}

rri_status rri_corpus_split_entries(rri_ctx* c, const rri_corpus* k, uint32_t thr, uint64_t seed, rri_corpus** observed, rri_corpus** held) {
    CHECK_CTX(c);
    if (observed) *observed = nullptr;
    if (held) *held = nullptr;
    char why[200] = "";
    if (!observed || !held) return derive_check_split(thr, observed != nullptr, held != nullptr, why, sizeof why), fail(c, RRI_ERR_INVALID, "%s", why);
    CHECK_DERIVE_CORPUS(c, k);
    if (derive_check_split(thr, true, true, why, sizeof why) != TOPN_REQ_OK) return fail(c, RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    // 1. pass A: what every piece holds out
    const DerivePieces pieces = derive_cut_pieces(k->h_indptr.data(), k->n_rows, nullptr, 0);
    const i64 np = (i64)pieces.row.size();
    DevTmp tstat, trow, tsrc, tlen, tnh, toh, too, hptr, hidx, hval, optr, oidx, oval;
    EventPair ev[2];
    for (EventPair& p : ev) HIPCHK(c, p.create());
    HIPCHK(c, tstat.alloc(DERIVE_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, hipMemsetAsync(tstat.p, 0, DERIVE_STAT_WORDS * sizeof(u64), c->stream));
    HIPCHK(c, derive_upload(trow, pieces.row, c->stream));
    HIPCHK(c, derive_upload(tsrc, pieces.src, c->stream));
    HIPCHK(c, derive_upload(tlen, pieces.len, c->stream));
    HIPCHK(c, tnh.alloc(at_least((size_t)np * sizeof(int))));
    std::vector<int> nh((size_t)np), no((size_t)np);
    HIPCHK(c, hipEventRecord(ev[0].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_entries_count, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)trow.p, (const i64*)tsrc.p,
                           (const int*)tlen.p, np, (const int*)k->indices, (unsigned)thr, (u64)seed, (int*)tnh.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(nh.data(), tnh.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(ev[0].b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (i64 p = 0; p < np; ++p) no[(size_t)p] = pieces.len[(size_t)p] - nh[(size_t)p];
    // 2. the prefix sums on the host, then pass B writes both outputs once
    std::vector<int64_t> piece_oh, piece_oo, h_hptr, h_optr;
    derive_offsets(pieces, nh, k->n_rows, &piece_oh, &h_hptr);
    derive_offsets(pieces, no, k->n_rows, &piece_oo, &h_optr);
    const i64 nnz_h = h_hptr[(size_t)k->n_rows], nnz_o = h_optr[(size_t)k->n_rows];
    HIPCHK(c, derive_upload(toh, piece_oh, c->stream));
    HIPCHK(c, derive_upload(too, piece_oo, c->stream));
    HIPCHK(c, derive_upload(hptr, h_hptr, c->stream));
    HIPCHK(c, derive_upload(optr, h_optr, c->stream));
    HIPCHK(c, hidx.alloc(at_least((size_t)nnz_h * sizeof(int))));
    HIPCHK(c, hval.alloc(at_least((size_t)nnz_h * sizeof(double))));
    HIPCHK(c, oidx.alloc(at_least((size_t)nnz_o * sizeof(int))));
    HIPCHK(c, oval.alloc(at_least((size_t)nnz_o * sizeof(double))));
    HIPCHK(c, hipEventRecord(ev[1].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_entries_write, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)trow.p, (const i64*)tsrc.p,
                           (const int*)tlen.p, (const i64*)toh.p, (const i64*)too.p, np, (const int*)k->indices, (const double*)k->values,
                           (unsigned)thr, (u64)seed, (int*)hidx.p, (double*)hval.p, (int*)oidx.p, (double*)oval.p, (u64*)tstat.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[1].b, c->stream));
    u64 h_stat[DERIVE_STAT_WORDS];
    HIPCHK(c, hipMemcpyAsync(h_stat, tstat.p, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (EventPair& p : ev) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t;
    }
    *observed = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_o, (i64)h_stat[ENTRIES_STAT_NEG_OBS], optr, oidx, oval, std::move(h_optr), ms);
    *held = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_h, (i64)h_stat[ENTRIES_STAT_NEG_HELD], hptr, hidx, hval, std::move(h_hptr), ms);
    return RRI_OK;
}

// the split by row (rri_rowsplit.hpp has the semantics, rri_rowsplit_kernels.hpp the kernels): the quotas and the bounds of the rows
// that give up nothing or everything on the host, the other bounds by class, then the count and write of the split by entry
rri_status rri_corpus_split_rows(rri_ctx* c, const rri_corpus* k, int64_t n_held, double fraction, int64_t min_observed, uint64_t seed,
                                 rri_corpus** observed, rri_corpus** held) {
    CHECK_CTX(c);
    if (observed) *observed = nullptr;
    if (held) *held = nullptr;
    char why[200] = "";
    if (!observed || !held) return rowsplit_check_request(n_held, fraction, min_observed, observed != nullptr, held != nullptr, why, sizeof why), fail(c, RRI_ERR_INVALID, "%s", why);
    CHECK_DERIVE_CORPUS(c, k);
    if (rowsplit_check_request(n_held, fraction, min_observed, true, true, why, sizeof why) != TOPN_REQ_OK) return fail(c, RRI_ERR_INVALID, "%s", why);
    HIPCHK(c, hipSetDevice(c->device));
    // 1. the quotas; the rows whose bound must be looked for, by class
    std::vector<uint64_t> h_bound((size_t)k->n_rows, ROWSPLIT_BOUND_NONE);
    std::vector<int64_t> list, quota, list_block, quota_block;
    for (i64 r = 0; r < k->n_rows; ++r) {
        const i64 L = k->h_indptr[(size_t)r + 1] - k->h_indptr[(size_t)r], h = rowsplit_quota(L, n_held, fraction, min_observed);
        const int cls = rowsplit_class(L, h);
        if (cls == ROWSPLIT_CLASS_NONE) {
            if (h > 0) h_bound[(size_t)r] = ROWSPLIT_BOUND_ALL;           // h == L > 0
        } else {
            (cls == ROWSPLIT_CLASS_WAVE ? list : list_block).push_back(r);
            (cls == ROWSPLIT_CLASS_WAVE ? quota : quota_block).push_back(h);
        }
    }
    const i64 n_wave = (i64)list.size(), n_block = (i64)list_block.size();
    list.insert(list.end(), list_block.begin(), list_block.end());
    quota.insert(quota.end(), quota_block.begin(), quota_block.end());
    const DerivePieces pieces = derive_cut_pieces(k->h_indptr.data(), k->n_rows, nullptr, 0);
    const i64 np = (i64)pieces.row.size();
    DevTmp tstat, tbound, tlist, tquota, trow, tsrc, tlen, tnh, toh, too, hptr, hidx, hval, optr, oidx, oval;
    EventPair ev[2];
    for (EventPair& p : ev) HIPCHK(c, p.create());
    HIPCHK(c, tstat.alloc(DERIVE_STAT_WORDS * sizeof(u64)));
    HIPCHK(c, hipMemsetAsync(tstat.p, 0, DERIVE_STAT_WORDS * sizeof(u64), c->stream));
    HIPCHK(c, derive_upload(tbound, h_bound, c->stream));
    HIPCHK(c, derive_upload(tlist, list, c->stream));
    HIPCHK(c, derive_upload(tquota, quota, c->stream));
    HIPCHK(c, derive_upload(trow, pieces.row, c->stream));
    HIPCHK(c, derive_upload(tsrc, pieces.src, c->stream));
    HIPCHK(c, derive_upload(tlen, pieces.len, c->stream));
    HIPCHK(c, tnh.alloc(at_least((size_t)np * sizeof(int))));
    std::vector<int> nh((size_t)np), no((size_t)np);
    // 2. the bounds, then pass A: what every piece holds out
    HIPCHK(c, hipEventRecord(ev[0].a, c->stream));
    if (n_wave > 0) {
        hipLaunchKernelGGL(k_rowsplit_select_wave, dim3(derive_grid(n_wave)), dim3(256), 0, c->stream, (const i64*)tlist.p, (const i64*)tquota.p,
                           n_wave, (const i64*)k->indptr, (const int*)k->indices, (u64)seed, (u64*)tbound.p);
        HIPCHK(c, hipGetLastError());
    }
    if (n_block > 0) {
        hipLaunchKernelGGL(k_rowsplit_select_block, dim3((unsigned)std::min<i64>(n_block, 1 << 20)), dim3(ROWSPLIT_BLOCK_THREADS), 0, c->stream,
                           (const i64*)tlist.p + n_wave, (const i64*)tquota.p + n_wave, n_block, (const i64*)k->indptr, (const int*)k->indices,
                           (u64)seed, (u64*)tbound.p);
        HIPCHK(c, hipGetLastError());
    }
    if (np > 0) {
        hipLaunchKernelGGL(k_rowsplit_count, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)trow.p, (const i64*)tsrc.p,
                           (const int*)tlen.p, np, (const int*)k->indices, (const u64*)tbound.p, (u64)seed, (int*)tnh.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(nh.data(), tnh.p, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(ev[0].b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (i64 p = 0; p < np; ++p) no[(size_t)p] = pieces.len[(size_t)p] - nh[(size_t)p];
    // 3. the prefix sums on the host, then pass B writes both outputs once
    std::vector<int64_t> piece_oh, piece_oo, h_hptr, h_optr;
    derive_offsets(pieces, nh, k->n_rows, &piece_oh, &h_hptr);
    derive_offsets(pieces, no, k->n_rows, &piece_oo, &h_optr);
    const i64 nnz_h = h_hptr[(size_t)k->n_rows], nnz_o = h_optr[(size_t)k->n_rows];
    for (i64 r = 0; r < k->n_rows; ++r) {       // every row gave up its quota, or a selection went wrong: nothing is written then
        const i64 L = k->h_indptr[(size_t)r + 1] - k->h_indptr[(size_t)r], got = h_hptr[(size_t)r + 1] - h_hptr[(size_t)r];
        if (got != rowsplit_quota(L, n_held, fraction, min_observed))
            return fail(c, RRI_ERR_HIP, "row %lld holds %lld entries out, not its quota of %lld", (long long)r, (long long)got,
                        (long long)rowsplit_quota(L, n_held, fraction, min_observed));
    }
    HIPCHK(c, derive_upload(toh, piece_oh, c->stream));
    HIPCHK(c, derive_upload(too, piece_oo, c->stream));
    HIPCHK(c, derive_upload(hptr, h_hptr, c->stream));
    HIPCHK(c, derive_upload(optr, h_optr, c->stream));
    HIPCHK(c, hidx.alloc(at_least((size_t)nnz_h * sizeof(int))));
    HIPCHK(c, hval.alloc(at_least((size_t)nnz_h * sizeof(double))));
    HIPCHK(c, oidx.alloc(at_least((size_t)nnz_o * sizeof(int))));
    HIPCHK(c, oval.alloc(at_least((size_t)nnz_o * sizeof(double))));
    HIPCHK(c, hipEventRecord(ev[1].a, c->stream));
    if (np > 0) {
        hipLaunchKernelGGL(k_rowsplit_write, dim3(derive_grid(np)), dim3(256), 0, c->stream, (const i64*)trow.p, (const i64*)tsrc.p,
                           (const int*)tlen.p, (const i64*)toh.p, (const i64*)too.p, np, (const int*)k->indices, (const double*)k->values,
                           (const u64*)tbound.p, (u64)seed, (int*)hidx.p, (double*)hval.p, (int*)oidx.p, (double*)oval.p, (u64*)tstat.p);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(ev[1].b, c->stream));
    u64 h_stat[DERIVE_STAT_WORDS];
    HIPCHK(c, hipMemcpyAsync(h_stat, tstat.p, sizeof h_stat, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double ms = 0.0;
    for (EventPair& p : ev) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t;
    }
    *observed = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_o, (i64)h_stat[ENTRIES_STAT_NEG_OBS], optr, oidx, oval, std::move(h_optr), ms);
    *held = corpus_adopt(c->device, k->n_rows, k->n_cols, nnz_h, (i64)h_stat[ENTRIES_STAT_NEG_HELD], hptr, hidx, hval, std::move(h_hptr), ms);
    return RRI_OK;
}

// ---- the blocked store of a CSR-X handle from a corpus (rri_spbuild.hpp has the steps, rri_spbuild_kernels.hpp the kernels) --------
namespace {
// build_sp_store for canonical arrays that are on the device: dv.indptr / dv.indices, the handle's own copies, are taken over as
// the canonical CSR, `values` (float64, device) is converted into sp_x, and both blocked copies are counted, scanned, claimed and
// sorted there.  What crosses to the host is segptr, 8 nblk (nseg + 1) bytes per copy, from which the work items are cut by the
// cutter of the host route (sp_cut_work) and the segments too long for a wave's sort are listed; and the longest row.
rri_status build_sp_store_device(rri_ctx* c, CsrDev& dv, const double* values, int64_t nnz, int target_items) {
    c->spb_ms = 0.0;
    dev_release(c, c->sp_rowptr); dev_release(c, c->sp_col); dev_release(c, c->sp_x); dev_release(c, c->sp_e);
    dev_adopt(c, c->sp_rowptr, dv.indptr);     // from here on they are the handle's, whatever fails below
    dev_adopt(c, c->sp_col, dv.indices);
    HIPCHK(c, dev_alloc(c, c->sp_x, (size_t)std::max<i64>(nnz, 1) * c->es));
    if (nnz > 0) launch_convert(c, RRI_F64, c->dtype, false, values, nnz, c->sp_x, nnz, 1, nnz);
    DevTmp tlong;
    HIPCHK(c, tlong.alloc(sizeof(int)));
    HIPCHK(c, hipMemsetAsync(tlong.p, 0, sizeof(int), c->stream));
    EventPair ev[4];          // per copy: count and scan; fill, claim and sort -- the phases between two reads of the host
    for (EventPair& p : ev) HIPCHK(c, p.create());
    const i64* rowptr = c->sp_rowptr;
    const int* col = c->sp_col;
    for (int w = 0; w < 2; ++w) {
        rri_ctx::SpCopy& cp = c->sp[w];
        dev_release(c, cp.segptr); dev_release(c, cp.idx); dev_release(c, cp.val); dev_release(c, cp.perm); dev_release(c, cp.work);
        SpDims dims;
        dims.nblk = cp.nblk; dims.bw = cp.bw; dims.nseg = cp.nseg; dims.gdim = cp.gdim;
        const i64 stride = cp.nseg + 1, flat = (i64)cp.nblk * stride, tiles = (flat + SPB_SCAN_TILE - 1) / SPB_SCAN_TILE;
        HIPCHK(c, dev_alloc(c, cp.segptr, (size_t)flat * sizeof(i64), true));
        DevTmp part;
        HIPCHK(c, part.alloc((size_t)tiles * sizeof(i64)));
        // 1, 2: count, padded scan
        HIPCHK(c, hipEventRecord(ev[2 * w].a, c->stream));
        if (w == 0)
            hipLaunchKernelGGL(k_spb_count_rows, dim3(corpus_grid(c->n * cp.nblk)), dim3(256), 0, c->stream, rowptr, col, c->n, cp.nblk, cp.bw,
                               stride, cp.segptr, (int*)tlong.p);
        else if (nnz > 0)
            hipLaunchKernelGGL(k_spb_count_cols, dim3(corpus_grid(nnz)), dim3(256), 0, c->stream, rowptr, col, c->n, (i64)nnz, cp.bw, stride,
                               (u64*)cp.segptr);
        hipLaunchKernelGGL(k_spb_scan_part, dim3((unsigned)tiles), dim3(256), 0, c->stream, (const i64*)cp.segptr, flat, (i64*)part.p);
        hipLaunchKernelGGL(k_spb_scan_top, dim3(1), dim3(1024), 0, c->stream, (i64*)part.p, tiles);
        hipLaunchKernelGGL(k_spb_scan_apply, dim3((unsigned)tiles), dim3(256), 0, c->stream, cp.segptr, flat, (const i64*)part.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev[2 * w].b, c->stream));
        std::vector<i64> h_seg((size_t)flat);
        HIPCHK(c, hipMemcpyAsync(h_seg.data(), cp.segptr, (size_t)flat * sizeof(i64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const i64 count = h_seg[(size_t)flat - 1];
        if (count < nnz || count > nnz + 3 * (i64)cp.nblk * cp.nseg)
            return fail(c, RRI_ERR_HIP, "the blocked copy %d counts %lld padded entries for %lld stored ones", w, (long long)count, (long long)nnz);
        const size_t cntp = (size_t)std::max<i64>(count, 4);
        cp.count = count;
        HIPCHK(c, dev_alloc(c, cp.idx, cntp * sizeof(unsigned short)));
        HIPCHK(c, dev_alloc(c, cp.val, cntp * c->es, true));
        HIPCHK(c, dev_alloc(c, cp.perm, cntp * sizeof(int)));
        // the work items, and the segments of copy 1 that a workgroup sorts, by the power of two they are padded to
        std::vector<SpWork> work;
        sp_cut_work(h_seg.data(), dims, w, target_items, work);
        cp.nwork = (int)work.size();
        cp.lps = sp_lanes_per_segment(nnz, dims);
        HIPCHK(c, dev_alloc(c, cp.work, std::max<size_t>(1, work.size()) * sizeof(SpWork)));
        if (!work.empty()) HIPCHK(c, hipMemcpyAsync(cp.work, work.data(), work.size() * sizeof(SpWork), hipMemcpyHostToDevice, c->stream));
        std::vector<std::vector<i64>> lists;          // [log2 of the padded length]
        std::vector<i64> all;
        if (w == 1 && nnz > 0) {
            for (int b = 0; b < cp.nblk; ++b)
                for (i64 sg = 0; sg < cp.nseg; ++sg) {
                    const i64 at = (i64)b * stride + sg, len = h_seg[(size_t)at + 1] - h_seg[(size_t)at];
                    if (spbuild_wave_sorted(len)) continue;
                    if (len > CORPUS_LDS_MAX) return fail(c, RRI_ERR_HIP, "a segment of %lld entries exceeds the block width", (long long)len);
                    int lg = 0;
                    while ((1ll << lg) < corpus_pad(len)) ++lg;
                    if (lists.size() <= (size_t)lg) lists.resize((size_t)lg + 1);
                    lists[(size_t)lg].push_back(at);
                }
            for (const auto& l : lists) all.insert(all.end(), l.begin(), l.end());
        }
        DevTmp keys, fill, tlist;
        // 3, 4: the pads, the claim, the sort
        HIPCHK(c, hipEventRecord(ev[2 * w + 1].a, c->stream));
        hipLaunchKernelGGL(k_spb_fill, dim3(corpus_grid((i64)cntp)), dim3(256), 0, c->stream, cp.idx, cp.perm, (i64)cntp, cp.bw);
        if (nnz > 0 && w == 0) {
            hipLaunchKernelGGL(k_spb_claim_rows, dim3(corpus_grid(nnz)), dim3(256), 0, c->stream, rowptr, col, c->n, (i64)nnz, cp.nblk, cp.bw,
                               stride, (const i64*)cp.segptr, cp.idx, cp.perm);
        } else if (nnz > 0) {
            const size_t nfill = (size_t)cp.nblk * (size_t)cp.nseg;
            HIPCHK(c, keys.alloc(cntp * sizeof(u64)));
            HIPCHK(c, fill.alloc(nfill * sizeof(int)));
            HIPCHK(c, hipMemsetAsync(keys.p, 0xff, cntp * sizeof(u64), c->stream));        // CORPUS_KEY_PAD everywhere
            HIPCHK(c, hipMemsetAsync(fill.p, 0, nfill * sizeof(int), c->stream));
            hipLaunchKernelGGL(k_spb_claim_cols, dim3(corpus_grid(nnz)), dim3(256), 0, c->stream, rowptr, col, c->n, (i64)nnz, cp.bw, stride,
                               cp.nseg, (const i64*)cp.segptr, (int*)fill.p, (u64*)keys.p);
            hipLaunchKernelGGL(k_spb_sort_wave, dim3(corpus_grid((i64)nfill * 64)), dim3(256), 0, c->stream, (const i64*)cp.segptr, (i64)nfill,
                               cp.nseg, (const u64*)keys.p, cp.idx, cp.perm, cp.bw);
            HIPCHK(c, hipGetLastError());
            if (!all.empty()) {
                HIPCHK(c, tlist.alloc(all.size() * sizeof(i64)));
                HIPCHK(c, hipMemcpyAsync(tlist.p, all.data(), all.size() * sizeof(i64), hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, allow_lds<k_spb_sort_block>(c, CORPUS_LDS_MAX * (int)sizeof(u64)));
                const i64* dl = (const i64*)tlist.p;
                for (size_t lg = 0; lg < lists.size(); ++lg) {
                    const size_t cnt = lists[lg].size();
                    if (!cnt) continue;
                    const i64 P = 1ll << lg;
                    hipLaunchKernelGGL(k_spb_sort_block, dim3((unsigned)cnt), dim3(P <= 1024 ? 256 : 1024), (size_t)P * sizeof(u64), c->stream, dl,
                                       (const i64*)cp.segptr, P, (const u64*)keys.p, cp.idx, cp.perm, cp.bw);
                    HIPCHK(c, hipGetLastError());
                    dl += cnt;
                }
            }
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev[2 * w + 1].b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vectors and the temporaries go out of scope
    }
    int longest = 0;
    HIPCHK(c, hipMemcpy(&longest, tlong.p, sizeof(int), hipMemcpyDeviceToHost));
    double ms = 0.0;
    for (EventPair& p : ev) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, p.a, p.b));
        ms += t;
    }
    c->spb_ms = ms;
    c->nnz = nnz;
    c->sp_max_row = longest;
    return RRI_OK;
}
}  // namespace

rri_status rri_upload_X_corpus(rri_ctx* c, const rri_corpus* k) {
    CHECK_CTX(c);
    REFUSE_RO(c, "X from a corpus");
    if (!c->sparse_x)
        return fail(c, RRI_ERR_INVALID, "%s", c->sparse ? sparse_data_refusal(c)
                                                         : "rri_upload_X_corpus builds the store of an RRI_UNWEIGHTED_SPARSE handle (X kept as CSR): "
                                                           "this handle keeps a dense X");
    const bool alive = corpus_alive(k);
    char why[200] = "";
    const int bad = spbuild_check_corpus(alive, alive ? k->n_rows : 0, alive ? k->n_cols : 0, alive ? k->nnz : 0, alive ? k->device : 0, c->n,
                                         c->d, c->device, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    // the rest is the CSR upload's own: copies on the device, the store built there, the uniform rows cleared, the cached state reset
    const CorpusArrays resident{k->indptr, k->indices, k->values};
    return upload_X_csr_kept(c, nullptr, nullptr, nullptr, k->nnz, RRI_F64, &resident);
}

// ---- the recommender side of the corpus chain (include/rri_corpus_fit.h; rri_fiterr.hpp has the semantics, rri_fiterr_kernels.hpp
// the kernels) -----------------------------------------------------------------------------------------------------------------
// The pattern and ratings of a pattern-only handle from a corpus.  Everything is checked here, before the handle is touched; the
// store itself is replaced where it always is: the request left on the handle is served by rri_upload_observed_csr, which also
// drops what the handle has cached of X and of the pattern.
rri_status rri_upload_observed_corpus(rri_ctx* c, const rri_corpus* k) {
    CHECK_CTX(c);
    REFUSE_RO(c, "an observation pattern from a corpus");
    if (!c->sparse || c->sparse_x) return fail(c, RRI_ERR_INVALID, "handle was not created with weighted=RRI_WEIGHTED_SPARSE");
    const bool alive = corpus_alive(k);
    char why[200] = "";
    const int bad = spbuild_check_corpus(alive, alive ? k->n_rows : 0, alive ? k->n_cols : 0, alive ? k->nnz : 0, alive ? k->device : 0, c->n,
                                         c->d, c->device, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    const rri_ctx::ObsReq req{k->indptr, k->indices, k->values, k->nnz};
    c->obs_req = &req;
    const rri_status s = rri_upload_observed_csr(c, nullptr, nullptr, nullptr, k->nnz, RRI_F64);
    c->obs_req = nullptr;       // (served and cleared there already: no return path leaves a pointer to this frame)
    return s;
}

namespace {
// the two launches of a chunk: the partials of its pieces (and the predictions, when asked for), and their sums per request
hipError_t fiterr_chunk(rri_ctx* c, const double* Tt, const i64* rows, i64 q0, i64 nreq, const LoglikPiece* pieces, i64 npieces,
                        const i64* first, const int* indices, const double* values, double lo, double hi, double* pred, double* psq,
                        double* pabs, double* sq, double* ab) {
    const size_t lds = 4 * (size_t)loglik_kp(c->k) * sizeof(double);
    const dim3 grid((unsigned)((npieces + 3) / 4));
    auto entries = [&](auto lanes) {
        hipLaunchKernelGGL(k_fiterr_entries<decltype(lanes)::value>, grid, dim3(256), lds, c->stream, (const double*)c->W, c->ldw, Tt,
                           c->k, rows, q0, pieces, npieces, indices, values, lo, hi, pred, psq, pabs);
    };
    switch (loglik_lanes(c->k)) {
        case 4: entries(std::integral_constant<int, 4>()); break;
        case 16: entries(std::integral_constant<int, 16>()); break;
        default: entries(std::integral_constant<int, 64>()); break;      // a measurement build (-DRRI_LOGLIK_LANES=64) only
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fiterr_sum, dim3((unsigned)((nreq + 255) / 256)), dim3(256), 0, c->stream, first, nreq, (const double*)psq,
                       (const double*)pabs, sq, ab);
    return hipGetLastError();
}
}  // namespace

// Reads the handle's W and T; the transposed copy of T, the row list, a chunk's pieces, their partials, its predictions and its
// sums live in temporaries of the call, so no sum a later sweep reads is touched and rri_device_memory reports what it reported
// before.  The corpus's indices and values are read where they lie.  The request is checked before any HIP call.
rri_status rri_corpus_entries_error(rri_ctx* c, const rri_corpus* k, const int64_t* rows, double clip_lo, double clip_hi,
                                    double* sq_out, double* abs_out, double* pred_out, double totals[3], double* kernel_ms) {
    CHECK_CORPUS(c, k);
    char why[200] = "";
    const int bad = fiterr_check_request(c->n, c->d, k->n_rows, k->n_cols, rows, clip_lo, clip_hi, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    const i64 count = k->n_rows;
    const int64_t* indptr = k->h_indptr.data();
    if (sq_out) std::fill(sq_out, sq_out + count, 0.0);
    if (abs_out) std::fill(abs_out, abs_out + count, 0.0);
    if (totals) totals[0] = totals[1] = totals[2] = 0.0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (count == 0 || k->nnz == 0) return RRI_OK;
    if (!c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    std::vector<LoglikChunk> chunks;
    loglik_cut_chunks(indptr, count, LL_UPLOAD_BUDGET, &chunks);
    i64 req_max = 0, ent_max = 0, pc_max = 0;
    for (const LoglikChunk& ch : chunks) {
        req_max = std::max<i64>(req_max, ch.q1 - ch.q0);
        ent_max = std::max<i64>(ent_max, indptr[ch.q1] - indptr[ch.q0]);
        pc_max = std::max<i64>(pc_max, loglik_cut_pieces(indptr, ch.q0, ch.q1, nullptr, nullptr));
    }
    if (req_max > 0x7fffffffLL) return fail(c, RRI_ERR_INVALID, "%lld requests are too many for one call", (long long)count);
    HIPCHK(c, hipSetDevice(c->device));
    const int kp = loglik_kp(c->k);
    DevTmp tTt, trows, tpc, tfirst, tpred, tps, tpa, tsq, tab;
    HIPCHK(c, tTt.alloc((size_t)c->d * kp * sizeof(double)));
    if (rows) HIPCHK(c, trows.alloc((size_t)req_max * sizeof(i64)));
    HIPCHK(c, tpc.alloc((size_t)pc_max * sizeof(LoglikPiece)));
    HIPCHK(c, tfirst.alloc((size_t)(req_max + 1) * sizeof(i64)));
    if (pred_out) HIPCHK(c, tpred.alloc((size_t)ent_max * sizeof(double)));
    HIPCHK(c, tps.alloc((size_t)pc_max * sizeof(double)));
    HIPCHK(c, tpa.alloc((size_t)pc_max * sizeof(double)));
    HIPCHK(c, tsq.alloc((size_t)req_max * sizeof(double)));
    HIPCHK(c, tab.alloc((size_t)req_max * sizeof(double)));
    EventPair ev;
    HIPCHK(c, ev.create());
    std::vector<double> h_sq((size_t)count, 0.0), h_ab((size_t)count, 0.0);
    double ms = 0.0;
    auto timed = [&]() {      // after a synchronise: the kernels between the two records
        float t = 0.0f;
        if (hipEventElapsedTime(&t, ev.a, ev.b) == hipSuccess) ms += t;
    };
    hipError_t e = hipEventRecord(ev.a, c->stream);
    if (e == hipSuccess) e = LK::loglik_transpose(c, (double*)tTt.p);
    if (e == hipSuccess) e = hipEventRecord(ev.b, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) timed();
    std::vector<LoglikPiece> pieces((size_t)pc_max);
    std::vector<int64_t> first((size_t)req_max + 1);
    for (size_t i = 0; i < chunks.size() && e == hipSuccess; ++i) {
        const i64 q0 = chunks[i].q0, nreq = chunks[i].q1 - q0, e0 = indptr[q0], nent = indptr[chunks[i].q1] - e0;
        if (nent == 0) continue;                                // only requests without entries: their outputs are 0 already
        const i64 npieces = loglik_cut_pieces(indptr, q0, chunks[i].q1, pieces.data(), first.data());
        if (rows) e = hipMemcpyAsync(trows.p, rows + q0, (size_t)nreq * sizeof(i64), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tpc.p, pieces.data(), (size_t)npieces * sizeof(LoglikPiece), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(tfirst.p, first.data(), (size_t)(nreq + 1) * sizeof(i64), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(ev.a, c->stream);
        if (e == hipSuccess)
            e = fiterr_chunk(c, (const double*)tTt.p, (const i64*)trows.p, q0, nreq, (const LoglikPiece*)tpc.p, npieces, (const i64*)tfirst.p,
                             k->indices + e0, k->values + e0, clip_lo, clip_hi, (double*)tpred.p, (double*)tps.p, (double*)tpa.p,
                             (double*)tsq.p, (double*)tab.p);
        if (e == hipSuccess) e = hipEventRecord(ev.b, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_sq.data() + q0, tsq.p, (size_t)nreq * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h_ab.data() + q0, tab.p, (size_t)nreq * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && pred_out) e = hipMemcpyAsync(pred_out + e0, tpred.p, (size_t)nent * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        // the pieces (host memory that the next chunk rewrites) have been read, and the temporaries are free for the next chunk
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess) timed();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "entries error failed: %s", hipGetErrorString(e));
    double tot_sq = 0.0, tot_ab = 0.0;
    for (i64 q = 0; q < count; ++q) {
        tot_sq += h_sq[(size_t)q];
        tot_ab += h_ab[(size_t)q];
    }
    if (sq_out) std::copy(h_sq.begin(), h_sq.end(), sq_out);
    if (abs_out) std::copy(h_ab.begin(), h_ab.end(), abs_out);
    if (totals) { totals[0] = tot_sq; totals[1] = tot_ab; totals[2] = (double)k->nnz; }
    if (kernel_ms) *kernel_ms = ms;
    return RRI_OK;
}

rri_status rri_corpus_value_range(rri_ctx* c, const rri_corpus* k, double out[2]) {
    CHECK_CORPUS(c, k);
    if (!out) return fail(c, RRI_ERR_INVALID, "out is NULL");
    if (k->nnz == 0) return fail(c, RRI_ERR_INVALID, "the corpus is empty: it has no value range");
    HIPCHK(c, hipSetDevice(c->device));
    const unsigned nb = (unsigned)std::min<i64>(1024, (k->nnz + 255) / 256);
    DevTmp part;
    HIPCHK(c, part.alloc((size_t)(nb + 1) * 2 * sizeof(double)));
    double* p = (double*)part.p;
    hipLaunchKernelGGL(k_value_range, dim3(nb), dim3(256), 0, c->stream, (const double*)k->values, (const double*)k->values, (i64)1, k->nnz, p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_value_range, dim3(1), dim3(256), 0, c->stream, (const double*)p, (const double*)(p + 1), (i64)2, (i64)nb, p + 2 * (size_t)nb);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, p + 2 * (size_t)nb, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

// ---- top-N lists, ranks and ranking metrics against resident corpora (include/rri_corpus_rank.h; rri_corpus_rank.hpp has the
// semantics, rri_corpus_rank_kernels.hpp the kernels) --------------------------------------------------------------------------------
namespace {
CrankCorpus crank_view(const rri_corpus* k) {
    const bool alive = corpus_alive(k);
    return CrankCorpus{k != nullptr, alive, alive ? k->n_rows : 0, alive ? k->n_cols : 0, alive ? k->device : 0};
}
// the HIP-event time of the kernels enqueued between begin() and end(); end() synchronises the stream
struct CrankTimer {
    rri_ctx* c;
    EventPair ev;
    double ms = 0.0;
    hipError_t begin() { return hipEventRecord(ev.a, c->stream); }
    hipError_t end() {
        hipError_t e = hipEventRecord(ev.b, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        float t = 0.0f;
        if (e == hipSuccess && hipEventElapsedTime(&t, ev.a, ev.b) == hipSuccess) ms += t;
        return e;
    }
};
// the ranks, values and eligible counts of every stored entry of `tg`, left on the device: the pieces are counted, scanned and cut
// there, their number is the one value read back, and k_rank_entries reads targets and exclusion where they lie.  rows: the
// device row list (NULL: request q scores row q).  The caller has checked the request and that there is something to score.
hipError_t crank_rank_device(rri_ctx* c, const rri_corpus* tg, const i64* rows, const rri_corpus* ex, double lo, double hi, DevTmp& rank,
                             DevTmp& val, DevTmp& elig, CrankTimer& tm) {
    const i64 m = tg->n_rows, len = m + 1, tiles = (len + CRANK_SCAN_TILE - 1) / CRANK_SCAN_TILE;
    DevTmp first, part, pieces;
    hipError_t e = first.alloc((size_t)len * sizeof(i64));
    if (e == hipSuccess) e = part.alloc((size_t)tiles * sizeof(i64));
    if (e == hipSuccess) e = rank.alloc((size_t)tg->nnz * sizeof(int));
    if (e == hipSuccess) e = val.alloc((size_t)tg->nnz * sizeof(double));
    if (e == hipSuccess) e = elig.alloc((size_t)m * sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(elig.p, 0xff, (size_t)m * sizeof(int), c->stream);      // -1: a row without entries
    if (e == hipSuccess) e = tm.begin();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_crank_count, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, (const i64*)tg->indptr, m, (i64*)first.p);
    hipLaunchKernelGGL(k_crank_scan_part, dim3((unsigned)tiles), dim3(256), 0, c->stream, (const i64*)first.p, len, (i64*)part.p);
    hipLaunchKernelGGL(k_crank_scan_top, dim3(1), dim3(256), 0, c->stream, (i64*)part.p, tiles);
    hipLaunchKernelGGL(k_crank_scan_apply, dim3((unsigned)tiles), dim3(256), 0, c->stream, (i64*)first.p, len, (const i64*)part.p);
    e = hipGetLastError();
    i64 npieces = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&npieces, (const i64*)first.p + m, sizeof(i64), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = tm.end();
    if (e != hipSuccess) return e;
    if (npieces < 1 || npieces > tg->nnz || (npieces + RANK_PIECES - 1) / RANK_PIECES > 0x7fffffffLL) return hipErrorInvalidValue;
    e = pieces.alloc((size_t)npieces * sizeof(RankPiece));
    if (e == hipSuccess) e = tm.begin();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_crank_cut, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (const i64*)tg->indptr, m, (const i64*)first.p,
                       (RankPiece*)pieces.p);
    e = hipGetLastError();
    if (e == hipSuccess)
        e = LK::rank_entries(c, rows, (const RankPiece*)pieces.p, npieces, (const int*)tg->indices, ex ? (const i64*)ex->indptr : nullptr,
                             ex ? (const int*)ex->indices : nullptr, rows, lo, hi, (int*)rank.p, (double*)val.p, (int*)elig.p);
    const hipError_t es = tm.end();      // the pieces are released behind the kernel that reads them
    return e == hipSuccess ? es : e;
}
}  // namespace

rri_status rri_corpus_topn_rows(rri_ctx* c, const int64_t* rows, int64_t count, int32_t topn, const rri_corpus* exclude, double clip_lo,
                                double clip_hi, int32_t* idx_out, double* val_out, double* kernel_ms) {
    CHECK_CTX(c);
    char why[200] = "";
    const int bad = crank_check_request(CRANK_CALL_TOPN, c->n, c->d, c->device, CrankCorpus{false, false, 0, 0, 0}, crank_view(exclude), rows,
                                        count, topn, RRI_MAX_TOPN, 1, clip_lo, clip_hi, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    if (count > 0) {
        if (!idx_out || !val_out) return fail(c, RRI_ERR_INVALID, "an output array is NULL");
        if (!c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
        if ((count + TOPN_ROWS - 1) / TOPN_ROWS > 0x7fffffffLL) return fail(c, RRI_ERR_INVALID, "count %lld is too large for one call", (long long)count);
    }
    if (kernel_ms) *kernel_ms = 0.0;
    if (count == 0) return RRI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp trows, tj, tv;
    CrankTimer tm{c};
    HIPCHK(c, tm.ev.create());
    if (rows) HIPCHK(c, trows.alloc((size_t)count * sizeof(i64)));
    HIPCHK(c, tj.alloc((size_t)count * topn * sizeof(int)));
    HIPCHK(c, tv.alloc((size_t)count * topn * sizeof(double)));
    if (rows) HIPCHK(c, hipMemcpyAsync(trows.p, rows, (size_t)count * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    hipError_t e = tm.begin();
    if (e == hipSuccess)
        e = LK::topn_rows(c, (const i64*)trows.p, count, topn, exclude ? (const i64*)exclude->indptr : nullptr,
                          exclude ? (const int*)exclude->indices : nullptr, (const i64*)trows.p, clip_lo, clip_hi, (int*)tj.p, (double*)tv.p);
    const hipError_t et = tm.end();
    if (e == hipSuccess) e = et;
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, tj.p, (size_t)count * topn * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(val_out, tv.p, (size_t)count * topn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "top-N rows against a corpus failed: %s", hipGetErrorString(e));
    if (kernel_ms) *kernel_ms = tm.ms;
    return RRI_OK;
}

rri_status rri_corpus_rank_entries(rri_ctx* c, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude, double clip_lo,
                                   double clip_hi, int32_t* rank_out, double* val_out, int32_t* eligible_out, double* kernel_ms) {
    CHECK_CTX(c);
    char why[200] = "";
    const int bad = crank_check_request(CRANK_CALL_RANK, c->n, c->d, c->device, crank_view(targets), crank_view(exclude), rows, 0, 1,
                                        RRI_MAX_TOPN, 1, clip_lo, clip_hi, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    const i64 m = targets->n_rows, nnz = targets->nnz;
    if (nnz > 0 && (!c->have_W || !c->have_T)) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    if (kernel_ms) *kernel_ms = 0.0;
    if (eligible_out) std::fill(eligible_out, eligible_out + m, -1);
    if (m == 0 || nnz == 0) return RRI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp trows, tr, tv, te;
    CrankTimer tm{c};
    HIPCHK(c, tm.ev.create());
    if (rows) {
        HIPCHK(c, trows.alloc((size_t)m * sizeof(i64)));
        HIPCHK(c, hipMemcpyAsync(trows.p, rows, (size_t)m * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    }
    hipError_t e = crank_rank_device(c, targets, (const i64*)trows.p, exclude, clip_lo, clip_hi, tr, tv, te, tm);
    if (e == hipSuccess && rank_out) e = hipMemcpyAsync(rank_out, tr.p, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && val_out) e = hipMemcpyAsync(val_out, tv.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && eligible_out) e = hipMemcpyAsync(eligible_out, te.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "rank entries of a corpus failed: %s", hipGetErrorString(e));
    if (kernel_ms) *kernel_ms = tm.ms;
    return RRI_OK;
}

rri_status rri_corpus_ranking_metrics(rri_ctx* c, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude,
                                      int64_t n_items, double relevant_from, double out[16], double* kernel_ms) {
    CHECK_CTX(c);
    char why[200] = "";
    const int bad = crank_check_request(CRANK_CALL_METRICS, c->n, c->d, c->device, crank_view(targets), crank_view(exclude), rows, 0, 1,
                                        RRI_MAX_TOPN, n_items, 0.0, 0.0, why, sizeof why);
    if (bad != TOPN_REQ_OK) return fail(c, bad == TOPN_REQ_UNSUPPORTED ? RRI_ERR_UNSUPPORTED : RRI_ERR_INVALID, "%s", why);
    if (!out) return fail(c, RRI_ERR_INVALID, "out is NULL");
    const i64 m = targets->n_rows, nnz = targets->nnz;
    if (nnz > 0 && (!c->have_W || !c->have_T)) return fail(c, RRI_ERR_INVALID, "W and T must be set first");
    std::fill(out, out + CRANK_OUT, 0.0);
    if (kernel_ms) *kernel_ms = 0.0;
    if (m == 0 || nnz == 0) return RRI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> table, ideal;
    const i64 tl = crank_table_len(n_items, c->d);
    crank_table(tl, &table, &ideal);
    const i64 nb = (m + CRANK_SUM_ROWS - 1) / CRANK_SUM_ROWS;
    DevTmp trows, tr, tv, te, ttab, tideal, tterms, tpart;
    CrankTimer tm{c};
    HIPCHK(c, tm.ev.create());
    if (rows) {
        HIPCHK(c, trows.alloc((size_t)m * sizeof(i64)));
        HIPCHK(c, hipMemcpyAsync(trows.p, rows, (size_t)m * sizeof(i64), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, ttab.alloc((size_t)tl * sizeof(double)));
    HIPCHK(c, tideal.alloc((size_t)(tl + 1) * sizeof(double)));
    HIPCHK(c, tterms.alloc((size_t)m * CRANK_TERMS * sizeof(double)));
    HIPCHK(c, tpart.alloc((size_t)(nb + 1) * CRANK_TERMS * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(ttab.p, table.data(), (size_t)tl * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tideal.p, ideal.data(), (size_t)(tl + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double inf = (double)INFINITY;
    hipError_t e = crank_rank_device(c, targets, (const i64*)trows.p, exclude, -inf, inf, tr, tv, te, tm);
    if (e == hipSuccess) e = tm.begin();
    if (e == hipSuccess) {
        double* part = (double*)tpart.p;
        hipLaunchKernelGGL(k_crank_rows, dim3((unsigned)std::min<i64>(65536, (m + 3) / 4)), dim3(256), 0, c->stream, (const i64*)targets->indptr,
                           (const double*)targets->values, m, (const int*)tr.p, (const int*)te.p, (i64)n_items, relevant_from,
                           (const double*)ttab.p, (const double*)tideal.p, (double*)tterms.p);
        hipLaunchKernelGGL(k_crank_sum, dim3((unsigned)nb), dim3(256), 0, c->stream, (const double*)tterms.p, m, (i64)CRANK_SUM_ROWS, part);
        hipLaunchKernelGGL(k_crank_sum, dim3(1), dim3(256), 0, c->stream, (const double*)part, nb, nb, part + (size_t)nb * CRANK_TERMS);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, part + (size_t)nb * CRANK_TERMS, CRANK_TERMS * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        const hipError_t et = tm.end();
        if (e == hipSuccess) e = et;
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // the table (host memory of this call) has been read by now too
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        std::fill(out, out + CRANK_OUT, 0.0);
        return fail(c, RRI_ERR_HIP, "ranking metrics of a corpus failed: %s", hipGetErrorString(e));
    }
    if (kernel_ms) *kernel_ms = tm.ms;
    return RRI_OK;
}

rri_status rri_sparse_store_get(rri_ctx* c, int32_t which, int64_t* info, int32_t n_info, int64_t* segptr, uint16_t* idx, int32_t* perm,
                                void* val, int32_t* work) {
    CHECK_CTX(c);
    if (which != 0 && which != 1) return fail(c, RRI_ERR_INVALID, "which = %d: a handle has the blocked copies 0 and 1", (int)which);
    if (n_info < 0 || (n_info > 0 && !info)) return fail(c, RRI_ERR_INVALID, "info is NULL with %d fields asked for", (int)n_info);
    const rri_ctx::SpCopy& cp = c->sp[which];
    if (!c->sparse || !c->have_X || !cp.segptr) return fail(c, RRI_ERR_INVALID, "the handle has no blocked store");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t f[RRI_SPARSE_STORE_INFO_FIELDS] = {cp.nblk, cp.bw, cp.nseg, cp.gdim, cp.count, cp.nwork, cp.lps, c->nnz, c->sp_max_row,
                                                     (int64_t)std::llround(c->spb_ms * 1000.0)};
    for (int i = 0; i < n_info && i < RRI_SPARSE_STORE_INFO_FIELDS; ++i) info[i] = f[i];
    for (int i = RRI_SPARSE_STORE_INFO_FIELDS; i < n_info; ++i) info[i] = 0;
    const size_t cntp = (size_t)std::max<i64>(cp.count, 4);
    if (segptr) HIPCHK(c, hipMemcpyAsync(segptr, cp.segptr, (size_t)cp.nblk * (size_t)(cp.nseg + 1) * sizeof(i64), hipMemcpyDeviceToHost, c->stream));
    if (idx) HIPCHK(c, hipMemcpyAsync(idx, cp.idx, cntp * sizeof(unsigned short), hipMemcpyDeviceToHost, c->stream));
    if (perm) HIPCHK(c, hipMemcpyAsync(perm, cp.perm, cntp * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (val) HIPCHK(c, hipMemcpyAsync(val, cp.val, cntp * c->es, hipMemcpyDeviceToHost, c->stream));
    if (work && cp.nwork > 0) HIPCHK(c, hipMemcpyAsync(work, cp.work, (size_t)cp.nwork * sizeof(SpWork), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_snapshot(rri_ctx* c) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->Wprev, (size_t)c->k * c->ldw * 8));
    HIPCHK(c, dev_ensure(c, c->Tprev, (size_t)c->k * c->LD * 8));
    HIPCHK(c, hipMemcpyAsync(c->Wprev, c->W, (size_t)c->k * c->ldw * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->Tprev, c->T, (size_t)c->k * c->LD * 8, hipMemcpyDeviceToDevice, c->stream));
    return RRI_OK;
}

rri_status rri_rollback(rri_ctx* c) {
    CHECK_CTX(c);
    if (!c->Wprev || !c->Tprev) return fail(c, RRI_ERR_INVALID, "no snapshot taken");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->W, c->Wprev, (size_t)c->k * c->ldw * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->T, c->Tprev, (size_t)c->k * c->LD * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    changed(c, CH_W | CH_T | CH_ENDED);
    return RRI_OK;
}

// ---- the explicit residual (RRI_UNWEIGHTED_RESIDUAL handles) --------------------------------------------------
rri_status rri_residual_rebuild(rri_ctx* c) {
    CHECK_CTX(c);
    REFUSE_RO(c, "the explicit residual");
    if (!c->explicit_resid) return fail(c, RRI_ERR_INVALID, "handle was not created with RRI_UNWEIGHTED_RESIDUAL");
    if (!c->have_X || !c->have_W || !c->have_T) return fail(c, RRI_ERR_INVALID, "X, W, T must be set");
    HIPCHK(c, hipSetDevice(c->device));
    r_refresh(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_get_residual(rri_ctx* c, void* host, int64_t ld, int32_t host_dtype) {
    CHECK_CTX(c);
    REFUSE_RO(c, "the explicit residual");
    if (!c->explicit_resid) return fail(c, RRI_ERR_INVALID, "handle was not created with RRI_UNWEIGHTED_RESIDUAL");
    HIPCHK(c, hipSetDevice(c->device));
    return to_host(c, c->E, c->LD, host, ld, host_dtype, c->n, c->d, c->dtype);
}

rri_status rri_residual_update(rri_ctx* c, const double* a, const double* b, const double* a2, const double* b2,
                               const double* trow, const double* wcol, double* y_out, double* z_out) {
    CHECK_CTX(c);
    REFUSE_RO(c, "the explicit residual");
    if (!c->explicit_resid) return fail(c, RRI_ERR_INVALID, "handle was not created with RRI_UNWEIGHTED_RESIDUAL");
    if (!a || !b || !trow || !wcol || ((a2 == nullptr) != (b2 == nullptr)))
        return fail(c, RRI_ERR_INVALID, "a, b, trow, wcol are required; a2 and b2 come together");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    // row vectors (n) and column vectors (padded to LD with zeros) on the device
    DevTmp rows, cols;
    HIPCHK(c, rows.alloc((size_t)3 * c->n * sizeof(double)));
    HIPCHK(c, cols.alloc((size_t)3 * c->LD * sizeof(double)));
    double* dr = (double*)rows.p;
    double* dc = (double*)cols.p;
    HIPCHK(c, hipMemsetAsync(dc, 0, (size_t)3 * c->LD * sizeof(double), c->stream));
    const double* hr[3] = {a, a2, wcol};
    const double* hc[3] = {b, b2, trow};
    for (int q = 0; q < 3; ++q) {
        if (hr[q]) HIPCHK(c, hipMemcpyAsync(dr + (i64)q * c->n, hr[q], (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (hc[q]) HIPCHK(c, hipMemcpyAsync(dc + (i64)q * c->LD, hc[q], (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    DISPATCH(c, {
        typename L::Upd u;
        u.a = dr;
        u.b = dc;
        if (a2) { u.a2 = dr + c->n; u.b2 = dc + c->LD; u.b2sub = c->zeros; }
        L::rank_update(c, c->E, c->LD, u, dc + 2 * c->LD, dr + 2 * c->n);
    });
    // z: the row-block partials in a fixed order (k_reduce); y: the column-panel partials, added here in panel order
    const int nb = (int)((c->LD + 31) / 32);
    hipLaunchKernelGGL(k_reduce, dim3(nb), dim3(1024), 0, c->stream, (const double*)c->Zpart, c->LD, c->nrb,
                       (const double*)nullptr, 0, c->k, c->red, (const DevState*)c->st);
    if (z_out) HIPCHK(c, hipMemcpyAsync(z_out, c->red, (size_t)c->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> yp;
    if (y_out) {
        yp.resize((size_t)c->npanels * c->n);
        HIPCHK(c, hipMemcpyAsync(yp.data(), c->Ypart, yp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (y_out)
        for (i64 i = 0; i < c->n; ++i) {
            double sacc = 0.0;
            for (int pgi = 0; pgi < c->npanels; ++pgi) sacc += yp[(size_t)pgi * c->n + i];
            y_out[i] = sacc;
        }
    changed(c, CH_SCRATCH | CH_ENDED);    // Zpart / red were used, and R no longer equals X - W T for the handle's factors
    return RRI_OK;
}

// ---- products with X for the initialisation -------------------------------------------------------------------
// out (nseg x m) = X B or X^T B on a pattern-only handle; B: gdim x m host row-major
static rri_status sparse_times(rri_ctx* c, int which, const double* B, int32_t m, double* out) {
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "X not set");
    if (!B || !out || m < 1 || m > 64) return fail(c, RRI_ERR_INVALID, "bad operand (1 <= m <= 64 columns on a pattern-only handle)");
    HIPCHK(c, hipSetDevice(c->device));
    const rri_ctx::SpCopy& cp = c->sp[which];
    // B is padded with zero rows up to nblk * bw so that a block's offsets always land inside it
    const i64 brows = (i64)cp.nblk * cp.bw;
    DevTmp bd, part, res;
    HIPCHK(c, bd.alloc((size_t)brows * m * sizeof(double)));
    HIPCHK(c, part.alloc((size_t)cp.nblk * cp.nseg * m * sizeof(double)));
    HIPCHK(c, res.alloc((size_t)cp.nseg * m * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(bd.p, 0, (size_t)brows * m * sizeof(double), c->stream));
    HIPCHK(c, hipMemcpyAsync(bd.p, B, (size_t)cp.gdim * m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DISPATCH(c, L::sp_spmm(c, which, (const double*)bd.p, m, (double*)part.p, (double*)res.p));
    HIPCHK(c, hipMemcpyAsync(out, res.p, (size_t)cp.nseg * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_X_times(rri_ctx* c, const double* B, int32_t m, double* out) {
    CHECK_CTX(c);
    if (c->sparse) return sparse_times(c, 0, B, m, out);
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "X not set");
    if (!B || !out || m < 1) return fail(c, RRI_ERR_INVALID, "bad operand");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp tm, outm;
    HIPCHK(c, tm.alloc((size_t)m * c->LD * sizeof(double)));      // B^T as an m x LD "T-like" operand
    HIPCHK(c, outm.alloc((size_t)m * c->ldw * sizeof(double)));   // (X B)^T, m x n
    HIPCHK(c, hipMemsetAsync(tm.p, 0, (size_t)m * c->LD * sizeof(double), c->stream));
    rri_status s = to_device(c, B, m, RRI_F64, tm.p, c->LD, c->d, m, RRI_F64, true);
    if (s != RRI_OK) return s;
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    DISPATCH_RO(c, L::xtt_any(c, (const double*)tm.p, m, (double*)outm.p));
    return to_host(c, outm.p, c->ldw, out, m, RRI_F64, c->n, m, RRI_F64, true);
}

rri_status rri_Xt_times(rri_ctx* c, const double* Q, int32_t m, double* out) {
    CHECK_CTX(c);
    if (c->sparse) return sparse_times(c, 1, Q, m, out);
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "X not set");
    if (!Q || !out || m < 1) return fail(c, RRI_ERR_INVALID, "bad operand");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp qm, outm;
    HIPCHK(c, qm.alloc((size_t)m * c->ldw * sizeof(double)));     // Q^T, m x n: every column contiguous
    HIPCHK(c, outm.alloc((size_t)m * c->LD * sizeof(double)));    // (X^T Q)^T, m x LD
    rri_status s = to_device(c, Q, m, RRI_F64, qm.p, c->ldw, c->n, m, RRI_F64, true);
    if (s != RRI_OK) return s;
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    const bool tm_on = c->timing != 0;
    const int tsave = c->timing;
    c->timing = 0;
    DevTmp zm;      // partial column sums of 8 vectors at a time: X is read once per 8 vectors
    HIPCHK(c, zm.alloc((size_t)8 * c->nrb * c->LD * sizeof(double)));
    for (int l = 0; l < m; l += 8)
        DISPATCH_RO(c, L::colsums8(c, (const double*)qm.p + (i64)l * c->ldw, std::min(8, m - l), (double*)zm.p,
                                (double*)outm.p + (i64)l * c->LD));
    c->timing = tsave;
    (void)tm_on;
    changed(c, CH_SCRATCH);
    return to_host(c, outm.p, c->LD, out, m, RRI_F64, c->d, m, RRI_F64, true);
}

// ---- the range finder of the randomized SVD, on the device ---------------------------------------------------------------
// sklearn.utils.extmath.randomized_svd (what initialization.py:105 calls) is: Q <- normalise(A Q), Q <- normalise(A^T Q), n_iter
// times; Q <- qr(A Q); B = Q^T A; small SVD of B.  All of its work is the products with X (rri_X_times / rri_Xt_times), and
// between them the (n or d) x m panels were normalised by LAPACK on the host: 0.7 of the 1.1 s of the start at 100000 x 10000
// (DESIGN 8).  Here the panels never leave the device: every normalisation is Cholesky-QR (G = Y^T Y by k_gram, its m x m
// Cholesky factor on the host -- 60 x 60 --, Y <- Y L^-T by k_lsolve_rows; shifted in its first of three passes) -- another basis of the same range than LU / QR give,
// so U, S, V of the SVD that follows are scikit-learn's up to rounding (the row-sharded start has done the same since round 2).
namespace {
// Lower Cholesky factor of the symmetric m x m G + shift_rel trace(G) I (row-major) in place.  A pivot that falls below 1e-14 of
// its diagonal entry -- a panel that is rank-deficient to working precision: a direction the rounding of G has already lost -- is
// held at that floor, so the factor stays finite and the direction comes out as normalised noise, as a QR would leave it.
bool host_cholesky(std::vector<double>& G, int m, double shift_rel) {
    double tr = 0.0;
    for (int i = 0; i < m; ++i) tr += G[(size_t)i * m + i];
    std::vector<double> d0((size_t)m);
    for (int i = 0; i < m; ++i) { d0[(size_t)i] = G[(size_t)i * m + i] + shift_rel * tr; G[(size_t)i * m + i] = d0[(size_t)i]; }
    for (int j = 0; j < m; ++j) {
        double dj = G[(size_t)j * m + j];
        for (int q = 0; q < j; ++q) dj -= G[(size_t)j * m + q] * G[(size_t)j * m + q];
        const double floor_j = d0[(size_t)j] > 0.0 ? 1e-14 * d0[(size_t)j] : 1e-300;
        if (!(dj > floor_j)) dj = floor_j;
        if (!std::isfinite(dj)) return false;
        const double ljj = std::sqrt(dj);
        G[(size_t)j * m + j] = ljj;
        for (int i = j + 1; i < m; ++i) {
            double v = G[(size_t)i * m + j];
            for (int q = 0; q < j; ++q) v -= G[(size_t)i * m + q] * G[(size_t)j * m + q];
            G[(size_t)i * m + j] = v / ljj;
            if (!std::isfinite(G[(size_t)i * m + j])) return false;
        }
        for (int i = 0; i < j; ++i) G[(size_t)i * m + j] = 0.0;
    }
    return true;
}
// The rows of At (m x len, stride ld, device) made orthonormal by shifted Cholesky-QR, three passes (Fukaya et al.: the first
// pass factorises G + s I, s = 1e-9 trace(G), which a panel of any condition number survives and which leaves it conditioned
// like 1e4; the next two are plain Cholesky-QR2).  A Gaussian test matrix times a matrix with one dominant direction -- rows
// normalised to sum 1, every document close to the mean -- is conditioned like 1e8 and worse: plain Cholesky-QR2 broke there.
rri_status cholqr2_rows(rri_ctx* c, double* At, i64 ld, i64 len, int m, double* Gdev) {
    std::vector<double> G((size_t)m * m);
    for (int round = 0; round < 3; ++round) {
        hipLaunchKernelGGL(k_gram, dim3(m, m), dim3(256), 0, c->stream, (const double*)At, ld, len, m, Gdev);
        HIPCHK(c, hipMemcpyAsync(G.data(), Gdev, G.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!host_cholesky(G, m, round == 0 ? 1e-9 : 0.0)) return fail(c, RRI_ERR_INVALID, "range finder: the panel holds a non-finite value");
        HIPCHK(c, hipMemcpyAsync(Gdev, G.data(), G.size() * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_lsolve_rows, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, c->stream, At, ld, len, m, (const double*)Gdev);
    }
    return RRI_OK;
}
}  // namespace

rri_status rri_range_finder(rri_ctx* c, const double* Q0, int32_t m, int32_t n_iter, int32_t transpose, double* Q_out,
                            double* B_out) {
    CHECK_CTX(c);
    if (c->sparse) return fail(c, RRI_ERR_UNSUPPORTED, "a pattern-only handle takes the products one by one (rri_X_times / rri_Xt_times)");
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "X not set");
    if (!Q0 || !Q_out || !B_out || m < 1 || m > 64 || n_iter < 0) return fail(c, RRI_ERR_INVALID, "bad operand (1 <= m <= 64)");
    HIPCHK(c, hipSetDevice(c->device));
    // panels, transposed as the product kernels take them: Pd (m x LD) lives on the column side of X, Pn (m x ldw) on the row side
    DevTmp pd, pn, zm, gd;
    HIPCHK(c, pd.alloc((size_t)m * c->LD * sizeof(double)));
    HIPCHK(c, pn.alloc((size_t)m * c->ldw * sizeof(double)));
    HIPCHK(c, zm.alloc((size_t)8 * c->nrb * c->LD * sizeof(double)));
    HIPCHK(c, gd.alloc((size_t)64 * 64 * sizeof(double)));
    double *Pd = (double*)pd.p, *Pn = (double*)pn.p;
    HIPCHK(c, hipMemsetAsync(Pd, 0, (size_t)m * c->LD * sizeof(double), c->stream));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    const int tsave = c->timing;
    c->timing = 0;
    auto X_times_dev = [&]() { DISPATCH_RO(c, L::xtt_any(c, (const double*)Pd, m, Pn)); };                 // Pn = (X Pd^T)^T
    auto Xt_times_dev = [&]() {                                                                          // Pd = (X^T Pn^T)^T
        for (int l = 0; l < m; l += 8)
            DISPATCH_RO(c, L::colsums8(c, (const double*)Pn + (i64)l * c->ldw, std::min(8, m - l), (double*)zm.p, Pd + (i64)l * c->LD));
    };
    rri_status s;
    // A = X (transpose == 0: Q0 is d x m) or A = X^T (Q0 is n x m), as scikit-learn transposes when n < d
    if (!transpose) s = to_device(c, Q0, m, RRI_F64, Pd, c->LD, c->d, m, RRI_F64, true);
    else s = to_device(c, Q0, m, RRI_F64, Pn, c->ldw, c->n, m, RRI_F64, true);
    for (int it = 0; it < n_iter && s == RRI_OK; ++it) {
        if (!transpose) {
            X_times_dev();  s = cholqr2_rows(c, Pn, c->ldw, c->n, m, (double*)gd.p);
            if (s == RRI_OK) { Xt_times_dev(); s = cholqr2_rows(c, Pd, c->LD, c->d, m, (double*)gd.p); }
        } else {
            Xt_times_dev(); s = cholqr2_rows(c, Pd, c->LD, c->d, m, (double*)gd.p);
            if (s == RRI_OK) { X_times_dev(); s = cholqr2_rows(c, Pn, c->ldw, c->n, m, (double*)gd.p); }
        }
    }
    if (s == RRI_OK) {
        if (!transpose) {       // Q = orth(X Q) (n x m), B = Q^T X (m x d)
            X_times_dev();  s = cholqr2_rows(c, Pn, c->ldw, c->n, m, (double*)gd.p);
            if (s == RRI_OK) Xt_times_dev();
        } else {                // Q = orth(X^T Q) (d x m), B = Q^T X^T (m x n)
            Xt_times_dev(); s = cholqr2_rows(c, Pd, c->LD, c->d, m, (double*)gd.p);
            if (s == RRI_OK) X_times_dev();
        }
    }
    c->timing = tsave;
    changed(c, CH_SCRATCH);
    if (s != RRI_OK) return s;
    if (!transpose) {
        s = to_host(c, Pn, c->ldw, Q_out, m, RRI_F64, c->n, m, RRI_F64, true);
        if (s == RRI_OK) s = to_host(c, Pd, c->LD, B_out, c->d, RRI_F64, m, c->d, RRI_F64, false);
    } else {
        s = to_host(c, Pd, c->LD, Q_out, m, RRI_F64, c->d, m, RRI_F64, true);
        if (s == RRI_OK) s = to_host(c, Pn, c->ldw, B_out, c->n, RRI_F64, m, c->n, RRI_F64, false);
    }
    return s;
}

// ---- the same range finder on a handle that keeps X sparse (RRI_UNWEIGHTED_SPARSE: the CSR X; RRI_WEIGHTED_SPARSE: the observed
// values on the pattern) ----------------------------------------------------------------------------------------------------
// There the 16 products went through rri_X_times / rri_Xt_times one by one, every (n or d) x m panel travelling to the host for
// LU / QR and back.  Here both panels live on the device as TALL row-major matrices (rows x m), the layout k_sp_spmm reads and
// writes, so a product's result is the next product's operand as it stands; they are allocated once, with the zero rows up to
// nblk * bw that a copy's operand needs, as are the block partials.  The normalisation is the shifted Cholesky-QR of
// cholqr2_rows (same host_cholesky, same three passes) on that layout: k_tall_gram_part / k_tall_gram_sum, k_tall_lsolve.
// Nothing of the handle is borrowed -- no Ypart / Zpart / red, no state of a sweep --, so a factorisation in progress is left
// as it is and nothing is invalidated.
namespace {
struct TallQR {
    double *part = nullptr, *Gdev = nullptr, *Lp = nullptr;   // gram partials [npart_max][64][64], G (m x m), packed L (64 x 64 + 64)
    std::vector<double> G, L = std::vector<double>((size_t)64 * 64 + 64, 0.0);   // L: the same entries are written for a given m
};

rri_status cholqr_tall(rri_ctx* c, double* Y, i64 rows, int m, TallQR& q) {
    const int npart = tall_gram_parts(rows);
    q.G.resize((size_t)m * m);
    for (int round = 0; round < 3; ++round) {
        hipLaunchKernelGGL(k_tall_gram_part, dim3(npart), dim3(256), 0, c->stream, (const double*)Y, rows, m, q.part);
        hipLaunchKernelGGL(k_tall_gram_sum, dim3((unsigned)((m * m + 255) / 256)), dim3(256), 0, c->stream, (const double*)q.part,
                           npart, m, q.Gdev);
        HIPCHK(c, hipMemcpyAsync(q.G.data(), q.Gdev, q.G.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!host_cholesky(q.G, m, round == 0 ? 1e-9 : 0.0)) return fail(c, RRI_ERR_INVALID, "range finder: the panel holds a non-finite value");
        for (int i = 0; i < m; ++i) {       // as k_tall_lsolve reads it: column j of the strictly lower part contiguous, then 1 / L_ii
            for (int j = 0; j < i; ++j) q.L[(size_t)j * 64 + i] = q.G[(size_t)i * m + j];
            q.L[(size_t)4096 + i] = 1.0 / q.G[(size_t)i * m + i];
        }
        HIPCHK(c, hipMemcpyAsync(q.Lp, q.L.data(), q.L.size() * 8, hipMemcpyHostToDevice, c->stream));
        const i64 groups = (rows + 4 * TS_ROWS - 1) / (4 * TS_ROWS);
        hipLaunchKernelGGL(k_tall_lsolve, dim3((unsigned)std::max<i64>(1, std::min<i64>(1024, groups))), dim3(256), 0, c->stream, Y,
                           rows, m, (const double*)q.Lp);      // (q.L is next written after the synchronise that follows this copy)
    }
    return RRI_OK;
}
}  // namespace

rri_status rri_sparse_range_finder(rri_ctx* c, const double* Q0, int32_t m, int32_t n_iter, int32_t transpose, double* Q_out,
                                   double* B_out) {
    CHECK_CTX(c);
    if (!c->sparse) return fail(c, RRI_ERR_INVALID, "a dense handle has rri_range_finder");
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "X not set");
    if (!Q0 || !Q_out || !B_out || m < 1 || m > 64 || n_iter < 0) return fail(c, RRI_ERR_INVALID, "bad operand (1 <= m <= 64)");
    HIPCHK(c, hipSetDevice(c->device));
    // Pd (d rows) is the operand of the row copy (X Pd), Pn (n rows) that of the column copy (X^T Pn)
    const rri_ctx::SpCopy &cr = c->sp[0], &cc = c->sp[1];
    const i64 rows_d = std::max<i64>(c->d, (i64)cr.nblk * cr.bw), rows_n = std::max<i64>(c->n, (i64)cc.nblk * cc.bw);
    const i64 part_elems = std::max<i64>(cr.nblk > 1 ? (i64)cr.nblk * cr.nseg : 1, cc.nblk > 1 ? (i64)cc.nblk * cc.nseg : 1) * m;
    DevTmp pd, pn, part, gpart, gd, lp;
    HIPCHK(c, pd.alloc((size_t)rows_d * m * sizeof(double)));
    HIPCHK(c, pn.alloc((size_t)rows_n * m * sizeof(double)));
    HIPCHK(c, part.alloc((size_t)part_elems * sizeof(double)));
    HIPCHK(c, gpart.alloc((size_t)tall_gram_parts(std::max(c->n, c->d)) * 4096 * sizeof(double)));
    HIPCHK(c, gd.alloc((size_t)64 * 64 * sizeof(double)));
    HIPCHK(c, lp.alloc((size_t)(64 * 64 + 64) * sizeof(double)));
    double *Pd = (double*)pd.p, *Pn = (double*)pn.p;
    HIPCHK(c, hipMemsetAsync(Pd, 0, (size_t)rows_d * m * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(Pn, 0, (size_t)rows_n * m * sizeof(double), c->stream));
    TallQR q;
    q.part = (double*)gpart.p; q.Gdev = (double*)gd.p; q.Lp = (double*)lp.p;
    auto X_times_dev = [&]() { DISPATCH(c, L::sp_spmm_panel(c, 0, (const double*)Pd, m, (double*)part.p, Pn)); };    // Pn = X Pd
    auto Xt_times_dev = [&]() { DISPATCH(c, L::sp_spmm_panel(c, 1, (const double*)Pn, m, (double*)part.p, Pd)); };   // Pd = X^T Pn
    auto orth_n = [&]() { return cholqr_tall(c, Pn, c->n, m, q); };
    auto orth_d = [&]() { return cholqr_tall(c, Pd, c->d, m, q); };
    // A = X (transpose == 0: Q0 is d x m) or A = X^T (Q0 is n x m), as scikit-learn transposes when n < d
    HIPCHK(c, hipMemcpyAsync(transpose ? Pn : Pd, Q0, (size_t)(transpose ? c->n : c->d) * m * sizeof(double), hipMemcpyHostToDevice,
                             c->stream));
    rri_status s = RRI_OK;
    for (int it = 0; it < n_iter && s == RRI_OK; ++it) {
        if (!transpose) {
            X_times_dev();  s = orth_n();
            if (s == RRI_OK) { Xt_times_dev(); s = orth_d(); }
        } else {
            Xt_times_dev(); s = orth_d();
            if (s == RRI_OK) { X_times_dev(); s = orth_n(); }
        }
    }
    if (s == RRI_OK) {
        if (!transpose) {       // Q = orth(X Q) (n x m), B = Q^T X: Pd = X^T Q is its transpose (d x m)
            X_times_dev();  s = orth_n();
            if (s == RRI_OK) Xt_times_dev();
        } else {                // Q = orth(X^T Q) (d x m), B = Q^T X^T: Pn = X Q is its transpose (n x m)
            Xt_times_dev(); s = orth_d();
            if (s == RRI_OK) X_times_dev();
        }
    }
    if (s != RRI_OK) { (void)hipStreamSynchronize(c->stream); return s; }
    const double* Qd = transpose ? Pd : Pn;
    const double* Bt = transpose ? Pn : Pd;
    const i64 rows_q = transpose ? c->d : c->n, cols_a = transpose ? c->n : c->d;
    HIPCHK(c, hipMemcpyAsync(Q_out, Qd, (size_t)rows_q * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return to_host(c, Bt, m, B_out, cols_a, RRI_F64, m, cols_a, RRI_F64, true);   // synchronises
}

// ---- preprocessing of the resident X ---------------------------------------------------------------------------
// rri_scale_X on an RRI_U8 handle: no matrix is written.  cscale .*= col_scale; with normalize_rows the row totals of the scaled
// matrix come from the streaming pass against a row of ones (the scales are folded in there) and rscale_i *= 1 / (tot_i +
// spacing(1)).  A row whose total is below 1e-10 would have to become the dense row 1/d: the column scales are then put back,
// nothing has changed, and the call fails with the number of such rows at the start of its message.  What the handle has cached
// of X is dropped by the caller, rri_scale_X, as for every other store.
static rri_status scale_counts(rri_ctx* c, const double* col_scale, int32_t normalize_rows) {
    if (!col_scale && !normalize_rows) return RRI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    DevTmp sd, keep, ones, nz;
    const unsigned nbd = (unsigned)((c->d + 255) / 256);
    if (col_scale) {
        HIPCHK(c, sd.alloc((size_t)c->d * sizeof(double)));
        HIPCHK(c, keep.alloc((size_t)c->LD * sizeof(double)));
        HIPCHK(c, hipMemcpyAsync(sd.p, col_scale, (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(keep.p, c->cscale, (size_t)c->LD * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_vec_mul, dim3(nbd), dim3(256), 0, c->stream, c->cscale, (const double*)sd.p, c->d);
    }
    if (normalize_rows) {
        HIPCHK(c, ones.alloc((size_t)c->LD * sizeof(double)));
        HIPCHK(c, nz.alloc(sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(nz.p, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_fill, dim3((unsigned)((c->LD + 255) / 256)), dim3(256), 0, c->stream, (double*)ones.p, c->LD, 1.0);
        const int tsave = c->timing;
        c->timing = 0;
        typedef LaunchX<unsigned char> L;
        L::pass_cfg<true, false, 0>(c, c->X, c->ldx, (const double*)ones.p, c->W, L::stream_whole(c));
        c->timing = tsave;
        const unsigned nbn = (unsigned)((c->n + 255) / 256);
        hipLaunchKernelGGL((k_row_scale_update<false>), dim3(nbn), dim3(256), 0, c->stream, (const double*)c->Ypart, c->npanels,
                           (int)c->n, c->rscale, (unsigned long long*)nz.p);
        unsigned long long zero_rows = 0;
        HIPCHK(c, hipMemcpyAsync(&zero_rows, nz.p, sizeof(zero_rows), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (zero_rows > 0) {
            if (col_scale) {
                HIPCHK(c, hipMemcpyAsync(c->cscale, keep.p, (size_t)c->LD * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
            return fail(c, RRI_ERR_INVALID, "%llu row(s) sum to less than 1e-10: normalisation would make them the dense row 1/d, which "
                                            "counts cannot hold; X and its scales are unchanged", zero_rows);
        }
        hipLaunchKernelGGL((k_row_scale_update<true>), dim3(nbn), dim3(256), 0, c->stream, (const double*)c->Ypart, c->npanels,
                           (int)c->n, c->rscale, (unsigned long long*)nullptr);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_set_X_scales(rri_ctx* c, const double* row_scale, const double* col_scale) {
    CHECK_CTX(c);
    if (c->dtype != RRI_U8) return fail(c, RRI_ERR_INVALID, "only an RRI_U8 handle has scale vectors");
    HIPCHK(c, hipSetDevice(c->device));
    if (row_scale) HIPCHK(c, hipMemcpyAsync(c->rscale, row_scale, (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (col_scale) HIPCHK(c, hipMemcpyAsync(c->cscale, col_scale, (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // a changed scale is a changed X: through the one call that rescales an X, with nothing more to multiply in
    if (!c->have_X || (!row_scale && !col_scale)) return RRI_OK;
    return rri_scale_X(c, nullptr, 0);
}

rri_status rri_get_X_scales(rri_ctx* c, double* row_out, double* col_out) {
    CHECK_CTX(c);
    if (c->dtype != RRI_U8) return fail(c, RRI_ERR_INVALID, "only an RRI_U8 handle has scale vectors");
    HIPCHK(c, hipSetDevice(c->device));
    if (row_out) HIPCHK(c, hipMemcpyAsync(row_out, c->rscale, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (col_out) HIPCHK(c, hipMemcpyAsync(col_out, c->cscale, (size_t)c->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_column_positive_counts(rri_ctx* c, double* df_out) {
    CHECK_CTX(c);
    if (c->dtype == RRI_F16) REFUSE_RO(c, "preprocessing of the resident X (it ends in a rewrite of X, a second rounding: preprocess on the host)");
    if (!df_out) return fail(c, RRI_ERR_INVALID, "df_out is NULL");
    if (c->weighted || !c->have_X || c->sparse_x) return fail(c, RRI_ERR_INVALID, "needs an unweighted handle with a dense X");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    const int ncols = (int)std::min<i64>(c->ldx, c->LD);
    HIPCHK(c, hipMemsetAsync(c->Zpart, 0, (size_t)c->nrb * c->LD * sizeof(double), c->stream));
    if (c->dtype == RRI_U8)     // the stored counts, whatever the scales are (matrixops.tfidf counts on the raw matrix)
        hipLaunchKernelGGL((k_col_count<unsigned char>), dim3(c->npanels * c->nrb), dim3(256), 0, c->stream,
                           (const unsigned char*)c->X, c->ldx, (int)c->n, ncols, c->Zpart, c->LD, c->rpb, c->npanels);
    else
    DISPATCH(c, hipLaunchKernelGGL((k_col_count<typename L::Elem>), dim3(c->npanels * c->nrb), dim3(256), 0, c->stream,
                                   (const typename L::Elem*)c->X, c->ldx, (int)c->n, ncols, c->Zpart, c->LD, c->rpb,
                                   c->npanels));
    LK::reduce(c);
    HIPCHK(c, hipMemcpyAsync(df_out, c->red, (size_t)c->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    changed(c, CH_SCRATCH);
    return RRI_OK;
}

rri_status rri_scale_X(rri_ctx* c, const double* col_scale, int32_t normalize_rows) {
    CHECK_CTX(c);
    if (c->dtype == RRI_F16) REFUSE_RO(c, "rewriting X in place (a second rounding: preprocess on the host, X is then rounded once at upload)");
    if (c->weighted || !c->have_X || c->sparse_x) return fail(c, RRI_ERR_INVALID, "needs an unweighted handle with a dense X");
    if (c->dtype == RRI_U8) {       // no matrix is written: the two scale vectors take it (the pass behind the row totals borrows Ypart)
        const rri_status s = scale_counts(c, col_scale, normalize_rows);
        changed(c, CH_X | CH_SCRATCH);
        return s;
    }
    if (!dev_owned(c, &c->X)) return fail(c, RRI_ERR_INVALID, "X is bound caller memory: it is not rewritten in place");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    DevTmp sd, inv;
    double* sdev = nullptr;
    HIPCHK(c, sd.alloc((size_t)c->LD * sizeof(double)));
    sdev = (double*)sd.p;
    if (col_scale) {
        HIPCHK(c, hipMemsetAsync(sdev, 0, (size_t)c->LD * sizeof(double), c->stream));
        HIPCHK(c, hipMemcpyAsync(sdev, col_scale, (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    } else {
        std::vector<double> ones((size_t)c->LD, 0.0);
        std::fill(ones.begin(), ones.begin() + c->d, 1.0);
        HIPCHK(c, hipMemcpyAsync(sdev, ones.data(), (size_t)c->LD * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    double* invdev = nullptr;
    if (normalize_rows) {
        HIPCHK(c, inv.alloc((size_t)c->n * sizeof(double)));
        invdev = (double*)inv.p;
        // row sums of X * col_scale = the row dots of the streaming pass against col_scale
        const int tsave = c->timing;
        c->timing = 0;
        DISPATCH(c, (L::template pass_cfg<true, false, 0>(c, c->X, c->ldx, sdev, c->W, L::stream_whole(c))));
        c->timing = tsave;
        hipLaunchKernelGGL(k_row_inverse, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)c->Ypart, c->npanels, (int)c->n, invdev);
    }
    DISPATCH(c, hipLaunchKernelGGL((k_scale2d<typename L::Elem>), dim3(8192), dim3(256), 0, c->stream,
                                   (typename L::Elem*)c->X, c->ldx, c->n, (int)c->d, col_scale ? (const double*)sdev : nullptr,
                                   (const double*)invdev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    changed(c, CH_X);
    return RRI_OK;
}

// ... and of an X kept as CSR (rri_sparse_kernels.hpp: k_spx_poscount, k_spx_rowtot, k_spx_scale)
static const char* const uni_refusal = "the handle has uniform rows: its X was preprocessed already, and a second preprocessing of "
                                       "such an X is not built (rri_upload_X_csr starts again)";
rri_status rri_csr_column_positive_counts(rri_ctx* c, double* df_out) {
    CHECK_CTX(c);
    if (!df_out) return fail(c, RRI_ERR_INVALID, "df_out is NULL");
    if (!c->sparse_x || !c->have_X) return fail(c, RRI_ERR_INVALID, "needs an RRI_UNWEIGHTED_SPARSE handle with an X");
    if (c->uni_n > 0) return fail(c, RRI_ERR_INVALID, "%s", uni_refusal);
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp out;
    HIPCHK(c, out.alloc((size_t)c->d * sizeof(double)));
    const rri_ctx::SpCopy& cc = c->sp[1];      // columns as segments; its values are X's (k_sp_permute after every rewrite)
    DISPATCH(c, hipLaunchKernelGGL((k_spx_poscount<typename L::Elem>), dim3((unsigned)((c->d + 3) / 4)), dim3(256), 0, c->stream,
                                   (const i64*)cc.segptr, cc.nseg, cc.nblk, (const typename L::Elem*)cc.val, (double*)out.p));
    HIPCHK(c, hipMemcpyAsync(df_out, out.p, (size_t)c->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

// Every rewrite of the resident CSR X ends HERE -- the stored values written, both blocked copies gathered again, the cached
// state dropped (changed) --, the calls about uniform rows included: they leave their request in c->uni_req and call this function,
// as rri_set_X_scales ends in rri_scale_X.
//   UNI_REQ_COLLECT    (rri_csr_scale_X_uniform) rows whose total is below 1e-10 do not stop the call: they take zeros and become
//                      the handle's uniform rows, value 1 / d
//   UNI_REQ_ZERO       (rri_set_uniform_rows) the rows uni_req_rows[0 .. uni_req_n) take zeros; nothing is scaled.  The caller
//                      makes them the handle's list once this has succeeded
// The handle's list, its length and its value change only after the last step that can fail: a call that fails leaves them alone.
rri_status rri_csr_scale_X(rri_ctx* c, const double* col_scale, int32_t normalize_rows, int64_t* zero_rows_out) {
    CHECK_CTX(c);
    const int req = c->uni_req;
    c->uni_req = rri_ctx::UNI_REQ_NONE;
    const bool uni = req == rri_ctx::UNI_REQ_COLLECT, zeroing = req == rri_ctx::UNI_REQ_ZERO;
    const int* zero_rows_list = c->uni_req_rows;
    const i64 zero_rows_n = zeroing ? c->uni_req_n : 0;
    c->uni_req_rows = nullptr;
    c->uni_req_n = 0;
    if (!c->sparse_x || !c->have_X) return fail(c, RRI_ERR_INVALID, "needs an RRI_UNWEIGHTED_SPARSE handle with an X");
    if (c->uni_n > 0 && !zeroing) return fail(c, RRI_ERR_INVALID, "%s", uni_refusal);
    if (zero_rows_out) *zero_rows_out = 0;
    if (!col_scale && !normalize_rows && !zeroing) return RRI_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, clear_halt(c) == RRI_OK ? hipSuccess : hipErrorUnknown);
    DevTmp sd, tt, nz, list, keep;
    i64 nuni = 0;
    if (col_scale) {
        HIPCHK(c, sd.alloc((size_t)c->d * sizeof(double)));
        HIPCHK(c, hipMemcpyAsync(sd.p, col_scale, (size_t)c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (normalize_rows) {
        HIPCHK(c, tt.alloc((size_t)c->n * sizeof(double)));
        HIPCHK(c, nz.alloc(sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(nz.p, 0, sizeof(unsigned long long), c->stream));
        DISPATCH(c, L::spx_scale(c, (const double*)sd.p, (double*)tt.p, (unsigned long long*)nz.p, true));
        unsigned long long zero_rows = 0;
        HIPCHK(c, hipMemcpyAsync(&zero_rows, nz.p, sizeof(zero_rows), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (zero_rows > 0 && !uni) {      // normalize would make these rows dense (1/d): nothing has been written, X is what it was
            if (!zero_rows_out) return fail(c, RRI_ERR_INVALID, "%llu rows sum to less than 1e-10 and zero_rows_out is NULL", zero_rows);
            *zero_rows_out = (int64_t)zero_rows;
            return RRI_OK;
        }
        // frozen statistics and uniform rows do not go together (frozen_refusal, the other order): nothing has been written
        if (zero_rows > 0 && c->fzB)
            return fail(c, RRI_ERR_UNSUPPORTED, "frozen statistics are set and %llu rows would become uniform rows: clear the statistics first", zero_rows);
        if (zero_rows > 0) {              // their list, in row order (k_spu_collect), before anything is written
            const size_t list_bytes = ((size_t)c->n * sizeof(int) + 7) & ~(size_t)7;      // the count sits behind the list, aligned
            HIPCHK(c, list.alloc(list_bytes + sizeof(i64)));
            i64* cnt = (i64*)((char*)list.p + list_bytes);
            hipLaunchKernelGGL(k_spu_collect, dim3(1), dim3(1024), 0, c->stream, (const double*)tt.p, c->n, (int*)list.p, cnt);
            HIPCHK(c, hipMemcpyAsync(&nuni, cnt, sizeof(i64), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (nuni != (i64)zero_rows) return fail(c, RRI_ERR_HIP, "uniform rows: %lld listed, %llu counted", (long long)nuni, zero_rows);
            HIPCHK(c, dev_ensure(c, c->uni_part, (size_t)64 * 64 * sizeof(double)));
            HIPCHK(c, keep.alloc((size_t)nuni * sizeof(int)));      // (becomes the handle's at the end)
            HIPCHK(c, hipMemcpyAsync(keep.p, list.p, (size_t)nuni * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        }
    }
    if (zeroing) {
        if (zero_rows_n > 0 && c->nnz > 0)
            DISPATCH(c, hipLaunchKernelGGL((k_spu_zero_rows<typename L::Elem>), dim3((unsigned)((zero_rows_n + 3) / 4)), dim3(256), 0, c->stream,
                                           zero_rows_list, (int)zero_rows_n, (const i64*)c->sp_rowptr, (typename L::Elem*)c->sp_x));
    } else {
        DISPATCH(c, L::spx_scale(c, (const double*)sd.p, (double*)tt.p, nullptr, false, nuni > 0));
    }
    if (c->nnz > 0)
        DISPATCH(c, for (int w = 0; w < 2; ++w)
                        hipLaunchKernelGGL((k_sp_permute<typename L::Elem>), dim3(2048), dim3(256), 0, c->stream,
                                           (const typename L::Elem*)c->sp_x, (const int*)c->sp[w].perm, c->sp[w].count,
                                           (typename L::Elem*)c->sp[w].val));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nuni > 0) {
        dev_adopt(c, c->uni_rows, keep);
        c->uni_n = nuni;
        c->uni_value = 1.0 / (double)c->d;      // as the reference writes it (matrixops.py:146)
        if (zero_rows_out) *zero_rows_out = (int64_t)nuni;
    }
    changed(c, CH_X);
    return RRI_OK;
}

rri_status rri_csr_scale_X_uniform(rri_ctx* c, const double* col_scale, int32_t normalize_rows, int64_t* uniform_rows_out) {
    CHECK_CTX(c);
    c->uni_req = rri_ctx::UNI_REQ_COLLECT;
    return rri_csr_scale_X(c, col_scale, normalize_rows, uniform_rows_out);
}

// ---- uniform rows of an RRI_UNWEIGHTED_SPARSE handle: X = S + value e_U 1^T ---------------------------------------------------
rri_status rri_set_uniform_rows(rri_ctx* c, const int32_t* rows, int64_t count, double value) {
    CHECK_CTX(c);
    if (!c->sparse_x) return fail(c, RRI_ERR_INVALID, "uniform rows need an RRI_UNWEIGHTED_SPARSE handle");
    if (!c->have_X) return fail(c, RRI_ERR_INVALID, "uniform rows are rows of the resident X: call rri_upload_X_csr first");
    if (count < 0 || count > c->n || (count > 0 && !rows)) return fail(c, RRI_ERR_INVALID, "bad list of uniform rows (0 <= count <= n)");
    if (!std::isfinite(value)) return fail(c, RRI_ERR_INVALID, "the value of the uniform rows is not finite");
    std::vector<int32_t> u(rows, rows + count);
    std::sort(u.begin(), u.end());
    for (int64_t q = 0; q < count; ++q) {
        if (u[(size_t)q] < 0 || (i64)u[(size_t)q] >= c->n) return fail(c, RRI_ERR_INVALID, "uniform row %d is out of range (n = %lld)", (int)u[(size_t)q], (long long)c->n);
        if (q > 0 && u[(size_t)q] == u[(size_t)q - 1]) return fail(c, RRI_ERR_INVALID, "uniform row %d is listed twice", (int)u[(size_t)q]);
    }
    // frozen statistics and uniform rows do not go together (frozen_refusal, the other order): nothing is changed
    if (count > 0 && c->fzB) return fail(c, RRI_ERR_UNSUPPORTED, "frozen statistics are set: clear them before rows are declared uniform");
    HIPCHK(c, hipSetDevice(c->device));
    if (count == 0 && c->uni_n == 0) return RRI_OK;      // nothing to clear: nothing changes, nothing is dropped
    DevTmp t;
    if (count > 0) {
        HIPCHK(c, t.alloc((size_t)count * sizeof(int)));
        HIPCHK(c, hipMemcpyAsync(t.p, u.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, dev_ensure(c, c->uni_part, (size_t)64 * 64 * sizeof(double)));
    }
    // the stored values of these rows become 0 (rows of an earlier list hold zeros already and stay ordinary rows of zeros), the
    // copies are gathered again and what the handle has cached of X is dropped: where every rewrite of this X ends
    c->uni_req = rri_ctx::UNI_REQ_ZERO;
    c->uni_req_rows = (const int*)t.p;
    c->uni_req_n = count;
    if (rri_status s = rri_csr_scale_X(c, nullptr, 0, nullptr)) return s;      // (the handle keeps the list it had)
    if (count > 0) dev_adopt(c, c->uni_rows, t);
    else dev_release(c, c->uni_rows);
    c->uni_n = count;
    c->uni_value = count > 0 ? value : 0.0;
    return RRI_OK;
}

rri_status rri_get_uniform_rows(rri_ctx* c, int32_t* rows_out, int64_t capacity, int64_t* count_out, double* value_out) {
    CHECK_CTX(c);
    if (!c->sparse_x) return fail(c, RRI_ERR_INVALID, "uniform rows need an RRI_UNWEIGHTED_SPARSE handle");
    if (count_out) *count_out = (int64_t)c->uni_n;
    if (value_out) *value_out = c->uni_value;
    if (!rows_out || c->uni_n == 0) return RRI_OK;      // a query of the count, or nothing to copy
    if (capacity < c->uni_n) return fail(c, RRI_ERR_INVALID, "rows_out holds %lld entries, the handle has %lld uniform rows", (long long)capacity, (long long)c->uni_n);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(rows_out, c->uni_rows, (size_t)c->uni_n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

// ---- row-sharded multi-GPU ---------------------------------------------------------------------------------
rri_status rri_reduce_buffer(rri_ctx* c, void** dev_ptr, int64_t* n_elems) {
    CHECK_CTX(c);
    if (dev_ptr) *dev_ptr = (void*)c->red;
    if (n_elems) *n_elems = c->red_elems;
    return RRI_OK;
}

rri_status rri_bind_reduce_buffer(rri_ctx* c, void* dev_ptr, int64_t n_elems) {
    CHECK_CTX(c);
    if (!dev_ptr || n_elems < c->red_elems || ((uintptr_t)dev_ptr) % 16)
        return fail(c, RRI_ERR_INVALID, "reduce buffer needs >= %lld elements, 16-byte aligned", c->red_elems);
    dev_release(c, c->red);
    c->red = (double*)dev_ptr;
    changed(c, CH_SCRATCH);
    return RRI_OK;
}

rri_status rri_topic_reduce_local(rri_ctx* c, int32_t t) {
    CHECK_CTX(c);
    rri_status r = ready(c);
    if (r != RRI_OK) return r;
    if (c->prm.fix_T) return fail(c, RRI_ERR_UNSUPPORTED, "split stepping is the T-row step taken apart: T must be free");
    if (c->explicit_resid) return fail(c, RRI_ERR_UNSUPPORTED, "row-sharded stepping runs the Gram-form schedule only");
    if (c->comm) return fail(c, RRI_ERR_INVALID, "a communicator is attached: rri_sweep does the collectives itself");
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    if (frozen_fix_W(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", FROZEN_FIX_W_TEXT);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->weighted) {
        // red = [a (LD) | nw (LD) | sum and negative-denominator flag of the last updated column]
        if (!c->resid_valid || (t == 0 && !c->resid_fresh)) w_refresh(c);     // once per sweep, as rri_sweep
        enqueue_wT_sums(c, t);
        if (c->pending_wcheck)
            hipLaunchKernelGGL(k_wcheck_wcol, dim3(1), dim3(256), 0, c->stream, (const double*)c->Gpart, c->nwb256, c->k,
                               c->pending_wcheck_topic, 0, t, kparams(c), c->st, c->red + 2 * c->LD);
        else
            HIPCHK(c, hipMemsetAsync(c->red + 2 * c->LD, 0, 2 * sizeof(double), c->stream));
        return RRI_OK;
    }
    if (c->carry_wfin) c->carry_valid = false;      // k_wfin's carry is not k_reduce's input (a run has taken its column check)
    if (!c->carry_valid || c->carry_topic != t) {
        // a local column check would see only this rank's rows: keep it pending for the reduced buffer
        const bool pend = c->pending_wcheck;
        const int pt = c->pending_wcheck_topic;
        c->pending_wcheck = false;
        enqueue_prologue(c, t, 0);
        c->pending_wcheck = pend;
        c->pending_wcheck_topic = pt;
        if (pend) return fail(c, RRI_ERR_INVALID, "carry lost while a sharded column check was pending");
    }
    LK::reduce(c);
    LK::frozen_add(c, t, c->pending_wcheck ? c->pending_wcheck_topic : -1);
    return RRI_OK;
}

rri_status rri_reduce_read(rri_ctx* c, double* out, int64_t count) {
    CHECK_CTX(c);
    if (!out || count < 0 || count > c->red_elems) return fail(c, RRI_ERR_INVALID, "bad reduce-buffer range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->red, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_reduce_write(rri_ctx* c, const double* in, int64_t count) {
    CHECK_CTX(c);
    if (!in || count < 0 || count > c->red_elems) return fail(c, RRI_ERR_INVALID, "bad reduce-buffer range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->red, in, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_topic_finish(rri_ctx* c, int32_t t) {
    CHECK_CTX(c);
    if (t >= 0 && frozen_fix_W(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", FROZEN_FIX_W_TEXT);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->weighted) {
        if (t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
        if (c->pending_wcheck)
            hipLaunchKernelGGL(k_wcheck_tail, dim3(1), dim3(64), 0, c->stream, (const double*)(c->red + 2 * c->LD),
                               c->pending_wcheck_topic, 0, t < 0 ? 0 : t, kparams(c), c->st);
        c->pending_wcheck = false;
        if (t < 0) return RRI_OK;
        enqueue_wT_solve(c, 0, t);
        if (!c->prm.fix_W) enqueue_wW_half(c, 0, t, true);      // W fixed: the T row alone (nmf.py:417-458 without :460-476)
        return RRI_OK;
    }
    if (t < 0) {  // only the pending column check, against the (all-reduced) buffer
        if (c->pending_wcheck) {
            LK::check_prev_only(c, c->pending_wcheck_topic, 0, 0);
            c->pending_wcheck = false;
        }
        return RRI_OK;
    }
    if (t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    const int chk = c->pending_wcheck ? 1 : 0;
    // W fixed: no W half follows that would finish the row checks (they ride with the Gram row of T there), and the kept
    // column takes the row's scale (nmf.py:450-452) -- as enqueue_T_half does
    LK::trow(c, t, chk, c->pending_wcheck_topic, 0, c->prm.fix_W != 0);
    c->pending_wcheck = false;
    changed(c, CH_T_ROW);
    if (c->prm.fix_W) {
        if (no_regs(c)) LK::scale_wcol(c, t);
        return RRI_OK;
    }
    enqueue_W_half(c, 0, t);
    return RRI_OK;
}

rri_status rri_topic_finish_w(rri_ctx* c, int32_t t) {
    CHECK_CTX(c);
    if (t < 0 || t >= c->k) return fail(c, RRI_ERR_INVALID, "topic out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->prm.fix_W) return RRI_OK;   // W fixed: the step has no W half (the reset has rewritten row and column, nmf.py:770-783)
    if (c->weighted) {           // after a T-row reset: E is rebuilt from the new row and column
        if (!c->resid_valid) w_refresh(c);
        enqueue_wW_half(c, 0, t, true);
        return RRI_OK;
    }
    c->skip_row_finish = true;   // the T-row sums of this topic predate the reset
    enqueue_W_half(c, 0, t);
    return RRI_OK;
}

rri_status rri_resid_row_argmax(rri_ctx* c, double* value, int64_t* local_row) {
    CHECK_CTX(c);
    if (!value || !local_row) return fail(c, RRI_ERR_INVALID, "NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->rowpos, (size_t)c->n * sizeof(double)));
    DISPATCH_RO(c, L::resid(c, false, false, nullptr, c->rowpos));
    hipLaunchKernelGGL(k_vec_sum_argmax, dim3(1), dim3(1024), 0, c->stream, (const double*)c->rowpos, c->n,
                       (double*)nullptr, c->itmp);
    i64 mi = -1;
    HIPCHK(c, hipMemcpyAsync(&mi, c->itmp, sizeof(i64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mi < 0 || mi >= c->n) return fail(c, RRI_ERR_INVALID, "arg-max out of range");
    HIPCHK(c, hipMemcpyAsync(value, c->rowpos + mi, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *local_row = mi;
    return RRI_OK;
}

rri_status rri_reset_row(rri_ctx* c, int64_t local_row, double* row_out_host) {
    CHECK_CTX(c);
    if (!row_out_host || local_row < 0 || local_row >= c->n) return fail(c, RRI_ERR_INVALID, "bad row");
    HIPCHK(c, hipSetDevice(c->device));
    const i64 mi = local_row;
    HIPCHK(c, hipMemcpyAsync(c->itmp, &mi, sizeof(i64), hipMemcpyHostToDevice, c->stream));
    DISPATCH_RO(c, L::reset_row(c));
    HIPCHK(c, hipMemcpyAsync(row_out_host, c->xraw, (size_t)c->d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_poll(rri_ctx* c) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    DevState s;
    rri_status r = read_state(c, &s);
    if (r != RRI_OK) return r;
    c->run_total = 0;
    r = status_from_halt(c, s, nullptr);
    if (s.halt < 0) (void)clear_halt(c);   // an event stays latched until rri_apply_reset_* / rri_skip_reset
    return r;
}

// ---- the communicator (one per process and group of ranks) ------------------------------------------------------
rri_status rri_comm_unique_id(uint8_t* id_out) {
    if (!id_out) return RRI_ERR_INVALID;
    RcclApi& a = rccl_api();
    if (!a.ok) return fail(nullptr, RRI_ERR_COMM, "%s", a.err.c_str());
    static_assert(sizeof(ncclUniqueId) == RRI_COMM_ID_BYTES, "RRI_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    ncclUniqueId id;
    ncclResult_t r = a.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, RRI_ERR_COMM, "ncclGetUniqueId: %s", a.GetErrorString(r));
    memcpy(id_out, &id, sizeof id);
    return RRI_OK;
}

rri_status rri_comm_create(rri_comm** out, const uint8_t* id, int32_t rank, int32_t world, int32_t device) {
    if (!out) return RRI_ERR_INVALID;
    *out = nullptr;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(nullptr, RRI_ERR_INVALID, "bad rank / world / id");
    RcclApi& a = rccl_api();
    if (!a.ok) return fail(nullptr, RRI_ERR_COMM, "%s", a.err.c_str());
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, RRI_ERR_HIP, "hipSetDevice(%d) failed", device);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclComm_t comm = nullptr;
    ncclResult_t r = a.CommInitRank(&comm, world, uid, rank);
    if (r != ncclSuccess) return fail(nullptr, RRI_ERR_COMM, "ncclCommInitRank(rank %d of %d): %s", rank, world, a.GetErrorString(r));
    rri_comm* m = new rri_comm();
    m->rank = rank; m->world = world; m->device = device; m->nccl = comm;
    *out = m;
    return RRI_OK;
}

rri_status rri_comm_create_host(rri_comm** out, int32_t rank, int32_t world, rri_allreduce_fn allreduce,
                                rri_allgather_fn allgather, rri_broadcast_fn broadcast, void* user) {
    if (!out) return RRI_ERR_INVALID;
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world || !allreduce || !allgather || !broadcast)
        return fail(nullptr, RRI_ERR_INVALID, "bad rank / world / callbacks");
    rri_comm* m = new rri_comm();
    m->rank = rank; m->world = world;
    m->h_allreduce = allreduce; m->h_allgather = allgather; m->h_broadcast = broadcast; m->user = user;
    *out = m;
    return RRI_OK;
}

rri_status rri_comm_destroy(rri_comm* m) {
    if (!m) return RRI_OK;
    if (m->nccl) {
        (void)hipSetDevice(m->device);
        (void)rccl_api().CommDestroy(m->nccl);
    }
    delete m;
    return RRI_OK;
}

rri_status rri_attach_comm(rri_ctx* c, rri_comm* comm, int64_t row_offset, int64_t n_global) {
    CHECK_CTX(c);
    if (comm && c->sparse_x) return fail(c, RRI_ERR_UNSUPPORTED, "an RRI_UNWEIGHTED_SPARSE handle is not row-sharded");
    if (comm && ro_store(c->dtype)) return fail(c, RRI_ERR_UNSUPPORTED, "an %s handle is not row-sharded (the combination has no test yet)", dtype_name(c->dtype));
    if (comm && c->fzB) return fail(c, RRI_ERR_UNSUPPORTED, "frozen statistics are set: clear them before a communicator is attached");
    if (!comm) {              // detach
        c->comm = nullptr;
        c->row_offset = 0;
        c->n_global = 0;
        changed(c, CH_SCRATCH);
        return RRI_OK;
    }
    if (row_offset < 0 || n_global < row_offset + c->n) return fail(c, RRI_ERR_INVALID, "row block [%lld, %lld) outside 0..%lld", (long long)row_offset, (long long)(row_offset + c->n), (long long)n_global);
    if (comm->nccl && comm->device != c->device) return fail(c, RRI_ERR_INVALID, "communicator lives on device %d, handle on %d", comm->device, c->device);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, dev_ensure(c, c->ctail, 8 * sizeof(double), true));
    dev_release(c, c->cand);
    HIPCHK(c, dev_alloc(c, c->cand, (size_t)2 * comm->world * sizeof(double)));
    c->comm = comm;
    c->row_offset = row_offset;
    c->n_global = n_global;
    c->comm_status = RRI_OK;
    changed(c, CH_SCRATCH);
    return RRI_OK;
}

rri_status rri_comm_broadcast(rri_ctx* c, double* host, int64_t count, int32_t root) {
    CHECK_CTX(c);
    if (!c->comm) return RRI_OK;                       // one rank: nothing to do
    if (!host || count < 1 || root < 0 || root >= c->comm->world) return fail(c, RRI_ERR_INVALID, "bad broadcast arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp buf;
    HIPCHK(c, buf.alloc((size_t)count * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(buf.p, host, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
    comm_broadcast(c, (double*)buf.p, count, root);
    HIPCHK(c, hipMemcpyAsync(host, buf.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_status != RRI_OK) { const rri_status r = c->comm_status; c->comm_status = RRI_OK; return r; }
    return RRI_OK;
}

rri_status rri_comm_allreduce_sum(rri_ctx* c, double* host, int64_t count) {
    CHECK_CTX(c);
    if (!host || count < 1) return fail(c, RRI_ERR_INVALID, "bad all-reduce arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (count <= 8 || !c->comm) return comm_allreduce_host(c, host, count);
    DevTmp buf;                                        // larger host arrays (the d x m panels of a row-sharded start)
    HIPCHK(c, buf.alloc((size_t)count * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(buf.p, host, (size_t)count * 8, hipMemcpyHostToDevice, c->stream));
    comm_allreduce(c, (double*)buf.p, count);
    HIPCHK(c, hipMemcpyAsync(host, buf.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_status != RRI_OK) { const rri_status r = c->comm_status; c->comm_status = RRI_OK; return r; }
    return RRI_OK;
}

rri_status rri_comm_stats(rri_ctx* c, int32_t* rank, int32_t* world, int64_t* allreduce_calls) {
    CHECK_CTX(c);
    if (rank) *rank = c->comm ? c->comm->rank : 0;
    if (world) *world = c->comm ? c->comm->world : 1;
    if (allreduce_calls) *allreduce_calls = c->comm ? c->comm->n_allreduce : 0;
    return RRI_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------------
rri_status rri_onchip_info(rri_ctx* c, int32_t* eligible, int64_t* launches) {
    CHECK_CTX(c);
    if (eligible) *eligible = (c->have_X && c->have_params && onchip_ok(c)) ? 1 : 0;
    if (launches) *launches = c->onchip_launches;
    return RRI_OK;
}

// ---- include/rri_fold.h: the one-launch fold sweep of a pattern-only handle, per handle and opt-in ------------------------------
// Remembered for the handle's life; nothing the handle keeps between calls was computed from it, so no cached state is touched:
// the next sweep simply takes the schedule wsweep_ok finds.
rri_status rri_set_fold_schedule(rri_ctx* c, int on) {
    const char* why = nullptr;
    if (fold_check_args(c != nullptr, c && c->weighted && c->sparse && !c->sparse_x, true, &why) != 0) return fail(c, RRI_ERR_INVALID, "rri_set_fold_schedule: %s", why);
    c->fold_asked = on != 0;
    return RRI_OK;
}

rri_status rri_fold_info(const rri_ctx* c, int64_t out[6]) {
    const char* why = nullptr;
    if (fold_check_args(c != nullptr, c && c->weighted && c->sparse && !c->sparse_x, out != nullptr, &why) != 0) {
        return fail(const_cast<rri_ctx*>(c), RRI_ERR_INVALID, "rri_fold_info: %s", why);     // (the error text is no state of the run)
    }
    out[0] = c->fold_asked ? 1 : 0;
    out[1] = (c->have_params && wfold_sched(c)) ? 1 : 0;
    out[2] = c->fold_launches;
    out[3] = c->fold_stepped;
    out[4] = c->fold_halts;
    out[5] = FOLD_ROWS;
    return RRI_OK;
}

// what the handle decided about its layout and routes (read-only; the order is the header's)
rri_status rri_layout_info(rri_ctx* c, int64_t* out, int32_t n) {
    CHECK_CTX(c);
    if (!out || n < 1) return fail(c, RRI_ERR_INVALID, "rri_layout_info needs room for at least one value");
    const bool dense_w = c->weighted == RRI_WEIGHTED_DENSE;
    const int64_t v[RRI_LAYOUT_FIELDS] = {
        c->sparse ? c->sp[0].nblk : 0, c->sparse ? c->sp[0].bw : 0, c->sparse ? c->sp[0].lps : 0, c->sparse ? c->sp[0].nwork : 0,
        c->sparse ? c->sp[1].nblk : 0, c->sparse ? c->sp[1].bw : 0, c->sparse ? c->sp[1].lps : 0, c->sparse ? c->sp[1].nwork : 0,
        c->rpb, c->nrb, c->npanels,
        c->Mbits ? 1 : 0, c->Mcols ? 1 : 0,
        c->mcols_tried && c->Mbits ? (int64_t)(c->mask_density * 1.0e9 + 0.5) : -1,
        dense_w && wtrow_small(c) ? 1 : 0,
        dense_w && c->nw_mask ? 1 : 0,
        !c->sparse && ro_pass_interleaved(c) ? 1 : 0,
        c->wcorr_nrb, c->n_cu,
        c->xp_valid ? 1 : 0, c->xp_valid ? c->xp_base : 0, c->xp_flagged, c->xp_tiles,
        c->xp_valid ? (c->xn_valid ? 26 : 28) : 0, c->xn_valid ? (int64_t)((uint64_t)c->xn_books.hi << 32 | c->xn_books.lo) : 0,
        c->xn_exceptions,
        LK::early_ok(c) ? 1 : 0, c->early_steps,
        c->sw.early_deal ? 1 : 0, c->plan.e_stride};
    for (int i = 0; i < n && i < RRI_LAYOUT_FIELDS; ++i) out[i] = v[i];
    return RRI_OK;
}

rri_status rri_device_memory(int64_t* buffers, int64_t* bytes) {
    if (buffers) *buffers = g_dev_buffers.load();
    if (bytes) *bytes = g_dev_bytes.load();
    return RRI_OK;
}

rri_status rri_debug_xcc(rri_ctx* c, int32_t* out, int32_t count) {
    CHECK_CTX(c);
    if (!out || count < 1 || count > 4096) return fail(c, RRI_ERR_INVALID, "bad count");
    HIPCHK(c, hipSetDevice(c->device));
    DevTmp dv;
    HIPCHK(c, dv.alloc((size_t)count * sizeof(int)));
    hipLaunchKernelGGL(k_xcc_probe, dim3((unsigned)count), dim3(64), 0, c->stream, (int*)dv.p);
    HIPCHK(c, hipMemcpyAsync(out, dv.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_onchip_fallbacks(rri_ctx* c, int64_t* fallbacks) {
    CHECK_CTX(c);
    if (fallbacks) *fallbacks = c->onchip_fallbacks;
    return RRI_OK;
}

rri_status rri_timing_enable(rri_ctx* c, int32_t on) {
    CHECK_CTX(c);
    c->timing = on < 0 ? 0 : on;
    for (int i = 0; i < 9; ++i) c->timing_seq[i] = 0;
    return RRI_OK;
}

rri_status rri_timing_read(rri_ctx* c, int32_t id, int64_t* launches, double* total_ms) {
    CHECK_CTX(c);
    if (id < 0 || id > 8) return fail(c, RRI_ERR_INVALID, "kernel_id out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (auto& tl : c->timed[id]) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, tl.a, tl.b));
        tot += ms;
        c->event_pool.push_back(tl.a);
        c->event_pool.push_back(tl.b);
    }
    if (launches) *launches = (int64_t)c->timed[id].size();
    if (total_ms) *total_ms = tot;
    c->timed[id].clear();
    return RRI_OK;
}

rri_status rri_synchronize(rri_ctx* c) {
    CHECK_CTX(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

// Bytes from the first element of X to the end of its last row: n - 1 strides and one row of LD elements (a bound X has LD = d
// and may be a slice of a wider array: the ldx - d elements behind its last row are not the handle's to read).
static size_t x_span_bytes(const rri_ctx* c) { return ((size_t)(c->n - 1) * c->ldx + c->LD) * c->es; }

rri_status rri_bench_stream_copy(rri_ctx* c, int32_t reps, double* avg_ms) {
    CHECK_CTX(c);
    REFUSE_RO(c, "the stream-copy yardstick");
    if (!c->have_X || reps < 1 || c->sparse) return fail(c, RRI_ERR_INVALID, "a dense X must be set and reps >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = x_span_bytes(c);
    DevTmp dst;
    EventPair ev;
    HIPCHK(c, dst.alloc(bytes));
    HIPCHK(c, ev.create());
    const i64 nvec = (i64)(bytes / 16);
    hipLaunchKernelGGL(k_stream_copy, dim3(256 * 8), dim3(256), 0, c->stream, (const float4*)c->X, (float4*)dst.p, nvec);
    (void)hipEventRecord(ev.a, c->stream);
    for (int r = 0; r < reps; ++r)
        hipLaunchKernelGGL(k_stream_copy, dim3(256 * 8), dim3(256), 0, c->stream, (const float4*)c->X, (float4*)dst.p, nvec);
    (void)hipEventRecord(ev.b, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "stream copy failed: %s", hipGetErrorString(e));
    if (avg_ms) *avg_ms = ms / reps;
    return RRI_OK;
}

rri_status rri_bench_rank1_update(rri_ctx* c, int32_t reps, double* avg_ms) {
    CHECK_CTX(c);
    REFUSE_RO(c, "the rank-one residual update");
    if (!c->have_X || !c->have_W || !c->have_T || reps < 1 || c->weighted || c->sparse_x)
        return fail(c, RRI_ERR_INVALID, "an unweighted handle with a dense X, W, T set and reps >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    // scratch residual R = copy of X; every repetition folds the rank-one term w_0 t_0^T of the handle's own factors
    // into it (non-trivial row and column factors; R stays finite: it moves by reps * w_0 t_0^T) and takes the row
    // dots against T[0,:] and the column sums against W[:,0] of the result -- the work of rri_residual_update
    const size_t bytes = x_span_bytes(c);
    DevTmp R;
    EventPair ev;
    HIPCHK(c, R.alloc(bytes));
    HIPCHK(c, ev.create());
    (void)hipMemcpyAsync(R.p, c->X, bytes, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemsetAsync(c->st, 0, 16, c->stream);
    const int tm = c->timing;
    c->timing = 0;
    auto once = [&]() {
        DISPATCH(c, {
            typename L::Upd u;
            u.a = c->W;
            u.b = c->T;
            L::rank_update(c, R.p, c->ldx, u, c->T, c->W);
        });
    };
    once();
    (void)hipEventRecord(ev.a, c->stream);
    for (int r = 0; r < reps; ++r) once();
    (void)hipEventRecord(ev.b, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    c->timing = tm;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    changed(c, CH_SCRATCH);
    if (e != hipSuccess) return fail(c, RRI_ERR_HIP, "rank-one bench failed: %s", hipGetErrorString(e));
    if (avg_ms) *avg_ms = ms / reps;
    return RRI_OK;
}

// ---- rows that left the device: frozen statistics (rri_frozen.hpp, rri_frozen_kernels.hpp) ---------------------------------
// None of the three invalidates anything the handle keeps: the statistics are read where a step uses them, and the sums a
// handle carries between steps (Zpart, Gpart, XYpart) are those of its own rows with or without them.
rri_status rri_frozen_set(rri_ctx* c, const double* B, const double* A, const double* s, double cval) {
    CHECK_CTX(c);
    if (!B) {      // clear
        (void)hipSetDevice(c->device);
        if (c->fzB) (void)hipStreamSynchronize(c->stream);      // a step still reading them
        frozen_release(c);
        return RRI_OK;
    }
    if (const char* why = frozen_refusal(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", why);
    char msg[200] = "";
    if (frozen_check_stats(c->k, c->d, B, A, s, cval, msg, sizeof msg) != FROZEN_OK) return fail(c, RRI_ERR_INVALID, "%s", msg);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, frozen_alloc(c));
    HIPCHK(c, hipMemcpy2DAsync(c->fzB, (size_t)c->LD * 8, B, (size_t)c->d * 8, (size_t)c->d * 8, (size_t)c->k, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->fzA, A, (size_t)c->k * c->k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->fzs, s, (size_t)c->k * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fz_c = cval;
    c->fz_rows = 0;
    return RRI_OK;
}

rri_status rri_frozen_get(rri_ctx* c, double* B_out, double* A_out, double* s_out, double* c_out, int64_t* rows_out) {
    CHECK_CTX(c);
    if (!c->fzB) return fail(c, RRI_ERR_INVALID, "no frozen statistics are set");
    HIPCHK(c, hipSetDevice(c->device));
    if (B_out) HIPCHK(c, hipMemcpy2DAsync(B_out, (size_t)c->d * 8, c->fzB, (size_t)c->LD * 8, (size_t)c->d * 8, (size_t)c->k, hipMemcpyDeviceToHost, c->stream));
    if (A_out) HIPCHK(c, hipMemcpyAsync(A_out, c->fzA, (size_t)c->k * c->k * 8, hipMemcpyDeviceToHost, c->stream));
    if (s_out) HIPCHK(c, hipMemcpyAsync(s_out, c->fzs, (size_t)c->k * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c_out) *c_out = c->fz_c;
    if (rows_out) *rows_out = c->fz_rows;
    return RRI_OK;
}

// the panel W^T X of the handle's rows into fzB: F <- decay F + W^T X
static rri_status frozen_absorb_panel(rri_ctx* c, double decay) {
    const int k = c->k;
    if (c->sparse_x) {
        // X on CSR: the blocked store's X^T Q (what rri_Xt_times runs), <= 64 topics per call; Q = the topics' columns of W
        const rri_ctx::SpCopy& cp = c->sp[1];
        const i64 brows = (i64)cp.nblk * cp.bw;
        const int mmax = std::min(k, 64);
        DevTmp q, part, res;
        HIPCHK(c, q.alloc((size_t)brows * mmax * sizeof(double)));
        HIPCHK(c, part.alloc((size_t)cp.nblk * cp.nseg * mmax * sizeof(double)));
        HIPCHK(c, res.alloc((size_t)cp.nseg * mmax * sizeof(double)));
        for (int t0 = 0; t0 < k; t0 += 64) {
            const int m = std::min(64, k - t0);
            const i64 total = (i64)m * c->n;
            TimedScope ts(c, 8);
            HIPCHK(c, hipMemsetAsync(q.p, 0, (size_t)brows * m * sizeof(double), c->stream));
            hipLaunchKernelGGL((k_convert2d<double, double, true>), dim3((unsigned)std::max<i64>(1, std::min<i64>(4096, (total + 255) / 256))),
                               dim3(256), 0, c->stream, (const double*)c->W + (i64)t0 * c->ldw, c->ldw, (double*)q.p, (i64)m, (i64)m, c->n);
            DISPATCH(c, L::sp_spmm(c, 1, (const double*)q.p, m, (double*)part.p, (double*)res.p));
            hipLaunchKernelGGL(k_frozen_axpy_t, dim3((unsigned)((c->d + 255) / 256), (unsigned)m), dim3(256), 0, c->stream,
                               (const double*)res.p, m, (int)c->d, t0, decay, c->fzB, c->LD);
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));      // the temporaries go with this scope
        return RRI_OK;
    }
    // dense: row blocks of whole 32-row steps.  Two workgroups fit a CU (128 accumulator registers per lane), and the grid is cut
    // to at most two full rounds of them -- a handful of workgroups in a third round would cost half a round
    const int cols_per_wg = std::min(k, FZ_CHUNK) <= 64 ? 256 : 128;
    const i64 ncb = (c->d + cols_per_wg - 1) / cols_per_wg;
    const i64 want = std::max<i64>(1, 4 * (i64)std::max(c->n_cu, 1) / ncb);
    const i64 steps = (c->n + FZ_RCH - 1) / FZ_RCH;
    const i64 nrb0 = std::max<i64>(1, std::min<i64>(std::min<i64>(want, 64), steps));
    const int rows_per_block = (int)((steps + nrb0 - 1) / nrb0) * FZ_RCH;
    const int nrb = (int)((c->n + rows_per_block - 1) / rows_per_block);
    DevTmp part;
    HIPCHK(c, part.alloc((size_t)nrb * std::min(k, FZ_CHUNK) * c->LD * sizeof(double)));
    for (int t0 = 0; t0 < k; t0 += FZ_CHUNK) {
        const int kc = std::min(FZ_CHUNK, k - t0);
        TimedScope ts(c, 8);
        DISPATCH(c, {
            typedef typename L::Elem SX;
            if (kc <= 64)
                hipLaunchKernelGGL((k_wtx_panel<SX, 4, 4>), dim3((unsigned)((c->d + 255) / 256), (unsigned)nrb), dim3(256), 0, c->stream,
                                   (const SX*)c->X, c->ldx, (int)c->n, (int)c->d, (const double*)c->W, c->ldw, t0, kc, rows_per_block,
                                   (double*)part.p, c->LD);
            else
                hipLaunchKernelGGL((k_wtx_panel<SX, 8, 2>), dim3((unsigned)((c->d + 127) / 128), (unsigned)nrb), dim3(256), 0, c->stream,
                                   (const SX*)c->X, c->ldx, (int)c->n, (int)c->d, (const double*)c->W, c->ldw, t0, kc, rows_per_block,
                                   (double*)part.p, c->LD);
        });
        hipLaunchKernelGGL(k_panel_sum, dim3((unsigned)((c->d + 255) / 256), (unsigned)kc), dim3(256), 0, c->stream,
                           (const double*)part.p, nrb, kc, c->LD, (int)c->d, t0, decay, c->fzB);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RRI_OK;
}

rri_status rri_frozen_absorb(rri_ctx* c, double decay) {
    CHECK_CTX(c);
    char msg[200] = "";
    if (frozen_check_decay(decay, msg, sizeof msg) != FROZEN_OK) return fail(c, RRI_ERR_INVALID, "%s", msg);
    if (const char* why = frozen_refusal(c)) return fail(c, RRI_ERR_UNSUPPORTED, "%s", why);
    if (!c->have_X || !c->have_W) return fail(c, RRI_ERR_INVALID, "X and W must be set before their rows are absorbed");
    HIPCHK(c, hipSetDevice(c->device));
    rri_status r = ensure_x_sq(c);       // ||X||^2: what the objective keeps per X
    if (r != RRI_OK) return r;
    const bool fresh = !c->fzB;
    HIPCHK(c, frozen_alloc(c));
    r = frozen_absorb_panel(c, decay);
    if (r == RRI_OK) {
        TimedScope ts(c, 8);
        hipLaunchKernelGGL(k_frozen_gram, dim3(c->k, c->k + 1), dim3(256), 0, c->stream, (const double*)c->W, c->ldw, c->n, c->k, decay,
                           c->fzA, c->fzs);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (r == RRI_OK && e != hipSuccess) r = fail(c, RRI_ERR_HIP, "absorbing the handle's rows failed: %s", hipGetErrorString(e));
    if (r == RRI_OK && c->comm_status != RRI_OK) { r = c->comm_status; c->comm_status = RRI_OK; }
    if (r != RRI_OK) {
        if (fresh) frozen_release(c);      // (statistics that were set before a failed absorb are no longer theirs: the caller sets them anew)
        return r;
    }
    c->fz_c = decay * c->fz_c + c->x_sq;
    c->fz_rows += c->n;
    return RRI_OK;
}

}  // extern "C"
