// rri_fiterr.hpp -- the clipped prediction error of W T at the stored entries of a resident corpus, written once (DESIGN "Fit from a
// resident corpus").
//
// A call has `count` REQUESTS, one per row of a canonical CSR corpus (strictly ascending columns inside [0, d), finite values of
// either sign).  Request q has a row i = rows[q] of W (rows NULL: i = q; duplicates allowed, any order) and the segment
// indices[indptr[q] .. indptr[q + 1]) with its values.  For entry e of the segment, with column j and value v,
//   p_e    = sum_t W[i,t] T[t,j] in float64; the order of that sum depends on k only;
//   c_e    = p_e clipped to [lo, hi]: lo where p_e < lo, hi where p_e > hi, p_e otherwise -- a NaN p_e stays NaN, and
//            lo = -inf, hi = +inf clip nothing;
//   r_e    = c_e - v;
// and the request's outputs are
//   sq[q]   = sum_e r_e^2
//   abs[q]  = sum_e |r_e|
//   pred[e] = c_e, per entry in corpus order.
// Both sums are taken in an order that depends on k and on the request's own segment only, so a request scored alone and among
// others returns the same bits.
//
// On the device the segments are cut into the pieces of rri_loglik.hpp (loglik_cut_pieces: at most LL_SEG entries, one wave each),
// loglik_lanes(k) lanes share an entry, the staged row of W and the rows of the transposed copy of T are loglik_kp(k) wide, and a
// call is cut into chunks of whole requests by loglik_cut_chunks: the pieces, their partials and the predictions of one chunk are
// the call's temporaries.  The kernels (rri_fiterr_kernels.hpp), the entry point (rri_corpus_entries_error) and the stand-alone
// CPU test (tests/c/fiterr_main.cpp) take the term and the request check from here.  fiterr_plain is the definition as a host
// loop.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "rri_loglik.hpp"

namespace rri {

// the clipped prediction: comparisons, so that a NaN passes through and an open side (-inf, +inf) never binds
RRI_TOPN_FN double fiterr_clip(double p, double lo, double hi) {
    const double a = p < lo ? lo : p;
    return a > hi ? hi : a;
}
// the term of one entry: clipped prediction minus the stored value
RRI_TOPN_FN double fiterr_term(double v, double p, double lo, double hi) { return fiterr_clip(p, lo, hi) - v; }

// ---- a request, checked on the host before any device call ----------------------------------------------------------------------
// n, d: the shape of W T; c_rows, c_cols: the shape of the corpus (c_rows requests).  Returns TOPN_REQ_OK, TOPN_REQ_INVALID or
// TOPN_REQ_UNSUPPORTED (a d whose full row does not fit one chunk) and writes the first broken rule to msg.
inline int fiterr_check_request(int64_t n, int64_t d, int64_t c_rows, int64_t c_cols, const int64_t* rows, double lo, double hi,
                                char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    if (std::isnan(lo) || std::isnan(hi)) return say(TOPN_REQ_INVALID, "a clip bound is NaN (an open side is -inf or +inf)", 0, 0);
    if (lo > hi) {
        if (msg && msg_len) snprintf(msg, msg_len, "clip_lo %g is above clip_hi %g", lo, hi);
        return TOPN_REQ_INVALID;
    }
    if (LL_ENTRY_BYTES * d > LL_UPLOAD_BUDGET)
        return say(TOPN_REQ_UNSUPPORTED, "a full row of d = %lld entries does not fit the budget of %lld bytes", (long long)d, (long long)LL_UPLOAD_BUDGET);
    if (c_cols != d) return say(TOPN_REQ_INVALID, "the corpus has %lld columns, W T has %lld", (long long)c_cols, (long long)d);
    if (!rows && c_rows > n) return say(TOPN_REQ_INVALID, "rows is NULL and the corpus has %lld rows, W has %lld", (long long)c_rows, (long long)n);
    for (int64_t q = 0; rows && q < c_rows; ++q)
        if (rows[q] < 0 || rows[q] >= n) return say(TOPN_REQ_INVALID, "rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
    return TOPN_REQ_OK;
}

// ---- the definition as a host loop ----------------------------------------------------------------------------------------------
// W n x k and T k x d, row-major; the request is a checked one.  Topics and entries in ascending order.  Any output may be NULL.
inline void fiterr_plain(const double* W, const double* T, int64_t d, int k, const int64_t* rows, int64_t count, const int64_t* indptr,
                         const int32_t* indices, const double* values, double lo, double hi, double* sq, double* ab, double* pred) {
    for (int64_t q = 0; q < count; ++q) {
        const int64_t i = rows ? rows[q] : q;
        double s = 0.0, a = 0.0;
        for (int64_t e = indptr[q]; e < indptr[q + 1]; ++e) {
            double p = 0.0;
            for (int t = 0; t < k; ++t) p += W[i * k + t] * T[(int64_t)t * d + indices[e]];
            const double r = fiterr_term(values[e], p, lo, hi);
            s += r * r;
            a += fabs(r);
            if (pred) pred[e] = fiterr_clip(p, lo, hi);
        }
        if (sq) sq[q] = s;
        if (ab) ab[q] = a;
    }
}

}  // namespace rri
