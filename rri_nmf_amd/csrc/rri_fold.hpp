// rri_fold.hpp -- the fold-in of rows against a fixed T on a pattern-only handle, written once.
//
// With T fixed the W half of a sweep touches row i of W through row i's own observed entries alone.  For the stored entries
// Omega_i of the row (columns j, values x_ij) take, once per row and sweep,
//     q = sum_j x_ij T[:,j]            (k)
//     G = sum_j T[:,j] T[:,j]^T        (k x k; nt of topic t is G[t][t])
// and the update of k_wwcol, whose  b + W[i,t] nt  is  s_t = q_t - sum_{l != t} G[t][l] W[i,l], becomes a walk over the topics
// t0 .. k-1 with no further pass over the entries:
//     numer = s_t - reg_w_l1 ,  c = G[t][t] + reg_w_l2
//     W[i,t] = (c > 0) ? max(numer, 0) / (c + eps) : 0 ;  has_wrs: W[i,t] = min(W[i,t], w_row_sum) ;  neg = (c < 0)
//     s_l   -= G[l][t] (W[i,t] - old W[i,t])   for every l != t
// After each topic comes the verdict wwcol_code(sum_i W[i,t], sum_i neg, p) of rri_halt.hpp, in topic order (k_wfold_verdict).
//
// The kernel (rri_fold_kernels.hpp), the schedule (enqueue_wsweep of rri_hip.hip), the two entry points of include/rri_fold.h
// and the stand-alone CPU test (tests/c/fold_main.cpp) take the update of one entry, the eligibility rule, the LDS formula and
// the argument check from here.  fold_rows_plain is the definition as a host loop.  Plain inline functions, host and device;
// nothing in this file needs HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_halt.hpp"

#define RRI_FOLD_FN RRI_HALT_FN

namespace rri {

constexpr int FOLD_MAX_K = 64;              // one lane per topic in the update walk
constexpr int FOLD_WAVES = 4;               // waves of a workgroup; a wave takes a row at a time
constexpr int FOLD_ROWS = 16;               // rows per workgroup: 128 contiguous bytes of every k-major column of W
constexpr size_t FOLD_LDS_LIMIT = 150 * 1024;   // the bound allow_lds and wsweep_ok use

// topics in tiles of 16 (the matrix-core tile); a wave's G in LDS has 16 kt rows of fold_gld doubles, an odd count so that the
// 64 lanes of the walk, which read one row each at the same offset, fall on different banks
RRI_FOLD_FN constexpr int fold_kt(int k) { return (k + 15) / 16; }
RRI_FOLD_FN constexpr int fold_kpad(int k) { return 16 * fold_kt(k); }
RRI_FOLD_FN constexpr int fold_gld(int k) { return fold_kpad(k) + 1; }
// dynamic LDS of k_wfold_rows: G per wave | the workgroup's tile of W, kpad x (rows + 1) doubles (the odd stride again) | its
// negative-denominator flags, a byte each
RRI_FOLD_FN constexpr size_t wfold_lds_bytes(int k, int rows_per_group) {
    return ((size_t)FOLD_WAVES * fold_kpad(k) * fold_gld(k) + (size_t)fold_kpad(k) * (rows_per_group + 1)) * sizeof(double) +
           (size_t)fold_kpad(k) * rows_per_group;
}

// the handle takes the one-launch schedule: asked for, pattern-only weighted flavour, T fixed and W free, one device, a rank the
// walk covers, LDS inside the bound
RRI_FOLD_FN constexpr bool wfold_ok(bool asked, bool weighted, bool sparse, bool sparse_x, bool fix_T, bool fix_W, bool comm, int k) {
    return asked && weighted && sparse && !sparse_x && fix_T && !fix_W && !comm && k >= 1 && k <= FOLD_MAX_K &&
           wfold_lds_bytes(k, FOLD_ROWS) <= FOLD_LDS_LIMIT;
}

// the update of one entry of W (k_wwcol's, nmf.py:464-469 with the vector c of the weighted flavour): s = b + W[i,t] nt
RRI_FOLD_FN double fold_entry(double s, double nt, const KParams& p, int* neg) {
    const double numer = s - p.reg_w_l1;
    const double c = nt + p.reg_w_l2;
    *neg = c < 0.0 ? 1 : 0;
    double w = 0.0;
    if (c > 0.0) w = fmax(numer, 0.0) / (c + p.eps);
    if (p.has_wrs) w = fmin(w, p.w_row_sum);
    return w;
}

// ---- the arguments of rri_set_fold_schedule / rri_fold_info, checked before any device call -------------------------------------
constexpr const char* FOLD_TEXT_NULL = "the handle is NULL";
constexpr const char* FOLD_TEXT_FLAVOUR = "the fold schedule belongs to a pattern-only handle (RRI_WEIGHTED_SPARSE): this handle is of another flavour";
constexpr const char* FOLD_TEXT_OUT = "out is NULL";
// 0: fine; -1: refused, with the text of the first broken rule in *msg
inline int fold_check_args(bool have_handle, bool pattern_only, bool have_out, const char** msg) {
    const char* m = !have_handle ? FOLD_TEXT_NULL : !pattern_only ? FOLD_TEXT_FLAVOUR : !have_out ? FOLD_TEXT_OUT : nullptr;
    if (msg) *msg = m;
    return m ? -1 : 0;
}

// ---- the definition as a host loop ----------------------------------------------------------------------------------------------
// One sweep of the W half for topics [t0, k) of every row of a canonical CSR (indptr, indices, values; n rows), T k x d and
// W n x k row-major.  W is updated in place; colsum[t] = sum_i W[i,t] and negs[t] = the number of rows with c < 0, for t in
// [t0, k), rows in ascending order (entries of colsum and negs below t0 are left alone).  Entries, topics and rows ascending.
inline void fold_rows_plain(int64_t n, int64_t d, int k, int t0, const int64_t* indptr, const int32_t* indices, const double* values,
                            const double* T, double* W, const KParams& p, double* colsum, double* negs) {
    std::vector<double> q((size_t)k), G((size_t)k * k), s((size_t)k);
    for (int t = t0; t < k; ++t) { colsum[t] = 0.0; negs[t] = 0.0; }
    for (int64_t i = 0; i < n; ++i) {
        std::fill(q.begin(), q.end(), 0.0);
        std::fill(G.begin(), G.end(), 0.0);
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int64_t j = indices[e];
            for (int a = 0; a < k; ++a) {
                const double ta = T[(int64_t)a * d + j];
                q[a] += values[e] * ta;
                for (int b = 0; b < k; ++b) G[(size_t)a * k + b] += ta * T[(int64_t)b * d + j];
            }
        }
        double* w = W + i * k;
        for (int t = 0; t < k; ++t) {
            double acc = q[t];
            for (int l = 0; l < k; ++l)
                if (l != t) acc -= G[(size_t)t * k + l] * w[l];
            s[t] = acc;
        }
        for (int t = t0; t < k; ++t) {
            int neg = 0;
            const double wnew = fold_entry(s[t], G[(size_t)t * k + t], p, &neg);
            const double dw = wnew - w[t];
            w[t] = wnew;
            for (int l = 0; l < k; ++l)
                if (l != t) s[l] -= G[(size_t)l * k + t] * dw;
            colsum[t] += wnew;
            negs[t] += neg;
        }
    }
}

}  // namespace rri
