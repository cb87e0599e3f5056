// rri_frozen.hpp -- rows that left the device, kept as frozen statistics, written once (DESIGN 4.11 "Frozen rows").
//
// A T-row step sees the rows of X and W only through three sums, the payload of the row-sharded all-reduce
//     red = [w_t^T X | w_t^T W, ||w_t||^2, sum W[:,t-1]].
// Rows O whose W no longer changes can therefore be replaced by those sums -- one more rank that never moves:
//     B = W_O^T X_O (k x d)    A = W_O^T W_O (k x k)    s = 1^T W_O (k)    c = ||X_O||^2
// and the step of topic t on the handle's own rows H reads
//     wR = (w_t^T X_H + B[t,:]) - sum_{j != t} (w_t^T W_H[:,j] + A[t,j]) T[j,:]
//     nw = ||w_t||^2 + A[t,t]
//     the check of column t takes  sum W_H[:,t] + s[t].
// The W half is unchanged: it reads the handle's rows only.  The frozen rows are never rescaled: the `W[:,t] *= nt1` of a
// step without penalties (nmf.py:450-452) reaches W_H alone, where the W half that follows overwrites it.  With W fixed
// nothing overwrites it, the transfer would have to reach the frozen rows, and such runs are refused while statistics are set.
// The frozen rows' share of the stacked objective 1/2 ||[X_O; X_H] - [W_O; W_H] T||^2 is  1/2 (c - 2 <B, T> + <A, T T^T>).
// A reset of topic t sets W[:,t] = 0 in the stacked problem (nmf.py:775): row t of B, row and column t of A and s[t] become 0.
//
// This file holds the argument check of rri_frozen_set / rri_frozen_absorb, the place of the addend inside `red`, and the
// definition as a host loop (frozen_sweep_plain).  rri_frozen_kernels.hpp, the entry points and the stand-alone CPU test
// (tests/c/frozen_main.cpp) take them from here.  Plain inline functions, host only but for the three index functions of the
// addend, which k_frozen_add calls too; nothing in this file needs HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_halt.hpp"

namespace rri {

enum { FROZEN_OK = 0, FROZEN_INVALID = -1 };
// what frozen_sweep_plain answers besides 0 and the halt codes of rri_halt.hpp: a branch of qf_min with c <= 0 that the plain
// loop does not restate (the device takes it; the cases of the test never meet it)
enum { FROZEN_PLAIN_RARE_BRANCH = -100 };

// ---- the addend inside red ------------------------------------------------------------------------------------------------
// red = [ldz columns | GRAM_SLICES slices of (k + 2) entries]; the consumers add the slices, so the Gram terms of the frozen
// rows go to slice 0 alone: entry l < k takes A[t,l], entry k takes A[t,t], entry k + 1 takes s[tprev] while a column
// check of topic tprev is pending (and nothing otherwise).  Column j < ldz takes B[t,j]; B is kept with the row stride ldz and
// zeros in its pad columns.
// (the only functions of this file that a kernel calls)
RRI_HALT_FN long long frozen_red_col(long long j) { return j; }
RRI_HALT_FN long long frozen_red_gram(long long ldz, int l) { return ldz + l; }
RRI_HALT_FN long long frozen_red_count(long long ldz, int k) { return ldz + k + 2; }

// ---- the arguments, checked on the host before any HIP call ------------------------------------------------------------------
// B: k x d row-major, A: k x k, s: k, all finite and >= 0; A symmetric (to the rounding of a product taken in two orders:
// |A[a,b] - A[b,a]| <= 1e-12 max(|A[a,b]|, |A[b,a]|)); c finite and >= 0.  The first broken rule goes to msg.
inline int frozen_check_stats(int k, int64_t d, const double* B, const double* A, const double* s, double c, char* msg,
                              size_t msg_len) {
    auto say = [&](const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return (int)FROZEN_INVALID;
    };
    if (k < 1 || d < 1) return say("k = %lld and d = %lld must be >= 1", k, (long long)d);
    if (!B || !A || !s) return say("B, A and s must all be given (B == NULL alone clears the statistics)", 0, 0);
    if (!std::isfinite(c) || c < 0.0) return say("c = ||X_O||^2 must be finite and >= 0", 0, 0);
    for (int t = 0; t < k; ++t)
        for (int64_t j = 0; j < d; ++j) {
            const double v = B[(int64_t)t * d + j];
            if (!std::isfinite(v) || v < 0.0) return say("B[%lld, %lld] is negative or not finite", t, (long long)j);
        }
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b) {
            const double v = A[(int64_t)a * k + b], w = A[(int64_t)b * k + a];
            if (!std::isfinite(v) || v < 0.0) return say("A[%lld, %lld] is negative or not finite", a, b);
            if (std::isfinite(w) && std::fabs(v - w) > 1e-12 * std::max(std::fabs(v), std::fabs(w)))
                return say("A is not symmetric at [%lld, %lld]", a, b);
        }
    for (int t = 0; t < k; ++t)
        if (!std::isfinite(s[t]) || s[t] < 0.0) return say("s[%lld] is negative or not finite", t, 0);
    return FROZEN_OK;
}
// F <- decay F + (the handle's sums): decay inside (0, 1]
inline int frozen_check_decay(double decay, char* msg, size_t msg_len) {
    if (decay > 0.0 && decay <= 1.0) return FROZEN_OK;
    if (msg && msg_len) snprintf(msg, msg_len, "decay %g is outside (0, 1]", decay);
    return FROZEN_INVALID;
}

// a reset of topic t on the host copies: what W_O[:,t] = 0 does to the sums
inline void frozen_clear_topic(int k, int64_t ldb, double* B, double* A, double* s, int t) {
    for (int64_t j = 0; j < ldb; ++j) B[(int64_t)t * ldb + j] = 0.0;
    for (int l = 0; l < k; ++l) A[(int64_t)t * k + l] = A[(int64_t)l * k + t] = 0.0;
    s[t] = 0.0;
}

// the frozen rows' share of the stacked objective; TT = T T^T (k x k), BT = <B, T>
inline double frozen_objective_share(int k, const double* A, const double* TT, double BT, double c) {
    double q = 0.0;
    for (int a = 0; a < k * k; ++a) q += A[a] * TT[a];
    return 0.5 * ((c - 2.0 * BT) + q);
}

// ---- the definition: one sweep of nmf.py:415-476 on the rows H with the frozen sums, as a plain host loop ----------------------
// X: n x d, W: n x k, T: k x d, all row-major float64, W and T updated in place; B (k x d), A, s read.  Returns 0, or the code
// and topic of the first step that the device would halt at (rri_halt.hpp: a reset event, an error) -- the state is then that
// of the halt --, or FROZEN_PLAIN_RARE_BRANCH for a denominator <= 0.
namespace frozen_detail {
// matrixops.py:5-69 (sort based, with its early exit)
inline void proj_simplex(std::vector<double>& v, double s) {
    double sum = 0.0;
    bool nonneg = true;
    for (double x : v) { sum += x; nonneg = nonneg && x >= 0.0; }
    if (sum == s && nonneg) return;
    std::vector<double> desc(v);
    std::sort(desc.begin(), desc.end(), [](double a, double b) { return a > b; });
    double csum = 0.0, theta = 0.0;
    for (size_t i = 0; i < desc.size(); ++i) {
        csum += desc[i];
        if (desc[i] * (double)(i + 1) > csum - s) theta = (csum - s) / (double)(i + 1);
    }
    for (double& x : v) x = std::max(x - theta, 0.0);
}
}  // namespace frozen_detail

inline int frozen_sweep_plain(int64_t n, int64_t d, int k, const double* X, double* W, double* T, const double* B,
                              const double* A, const double* s, const KParams& p, int* halt_topic) {
    const bool no_regs = std::fabs(p.reg_w_l1) + std::fabs(p.reg_w_l2) + std::fabs(p.reg_t_l1) + std::fabs(p.reg_t_l2) == 0.0;
    const bool project = p.project_T && p.has_trs;
    std::vector<double> g((size_t)k), x((size_t)d);
    auto halt = [&](int code, int t) { if (halt_topic) *halt_topic = t; return code; };
    for (int t = 0; t < k; ++t) {
        // T row: the sums over H plus the frozen rows' share
        for (int l = 0; l < k; ++l) {
            double a = 0.0;
            for (int64_t i = 0; i < n; ++i) a += W[i * k + t] * W[i * k + l];
            g[(size_t)l] = a + A[(int64_t)t * k + l];
        }
        const double nw = g[(size_t)t];
        g[(size_t)t] = 0.0;
        const double c = nw + p.reg_t_l2;
        const int mode = trow_denominator_mode(c, p);
        if (mode != 0) return halt(mode < 0 ? mode : (int)FROZEN_PLAIN_RARE_BRANCH, t);
        double nt1 = 0.0;
        for (int64_t j = 0; j < d; ++j) {
            double wx = 0.0, acc = 0.0;
            for (int64_t i = 0; i < n; ++i) wx += W[i * k + t] * X[i * d + j];
            wx += B[(int64_t)t * d + j];
            for (int l = 0; l < k; ++l) acc += g[(size_t)l] * T[(int64_t)l * d + j];
            const double numer = (wx - acc) - p.reg_t_l1;
            x[(size_t)j] = std::max(numer, 0.0) / (c + p.eps);
            nt1 += x[(size_t)j];
        }
        if (project) frozen_detail::proj_simplex(x, p.t_row_sum);
        for (int64_t j = 0; j < d; ++j) T[(int64_t)t * d + j] = x[(size_t)j];
        if (no_regs)
            for (int64_t i = 0; i < n; ++i) W[i * k + t] *= nt1;
        double sumT = 0.0;
        for (int64_t j = 0; j < d; ++j) sumT += T[(int64_t)t * d + j];
        if (trow_resets(sumT, p)) return halt(HALT_EVENT_RESET_T, t);
        if (trow_kept(sumT, p) && project && std::fabs(sumT - p.t_row_sum) > 1e-15) {
            frozen_detail::proj_simplex(x, p.t_row_sum);
            for (int64_t j = 0; j < d; ++j) T[(int64_t)t * d + j] = x[(size_t)j];
        }
        // W column: the handle's rows only
        for (int l = 0; l < k; ++l) {
            double a = 0.0;
            for (int64_t j = 0; j < d; ++j) a += T[(int64_t)l * d + j] * T[(int64_t)t * d + j];
            g[(size_t)l] = a;
        }
        const double nt = g[(size_t)t];
        g[(size_t)t] = 0.0;
        const double cden = nt + p.reg_w_l2;
        const int wmode = wcol_denominator_mode(cden, p);
        if (wmode != 0) return halt(wmode < 0 ? wmode : (int)FROZEN_PLAIN_RARE_BRANCH, t);
        double colsum = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            double xt = 0.0, acc = 0.0;
            for (int64_t j = 0; j < d; ++j) xt += X[i * d + j] * T[(int64_t)t * d + j];
            for (int l = 0; l < k; ++l) acc += W[i * k + l] * g[(size_t)l];
            const double numer = (xt - acc) - p.reg_w_l1;
            W[i * k + t] = std::max(numer, 0.0) / (cden + p.eps);
            colsum += W[i * k + t];
        }
        const int code = wcol_code(colsum + s[t], p);
        if (code != 0) return halt(code, t);
    }
    return 0;
}

}  // namespace rri
