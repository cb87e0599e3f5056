// rri_loglik.hpp -- the log-likelihood of stored counts under the rows of W T, written once (DESIGN "Log-likelihood of entries").
//
// A call has `count` REQUESTS.  Request q has a row i = rows[q] of W (rows NULL: i = q; duplicates allowed, any order) and a
// segment of a CSR matrix WITH values: indices[indptr[q] .. indptr[q + 1]) and values[...], the columns strictly ascending inside
// [0, d), the values finite and >= 0.  For entry e of the segment, with column j and value v,
//   p_e     = sum_t W[i,t] T[t,j] in float64; the order of that sum depends on k only;
//   term_e  = 0 exactly when v == 0, else v * log(p_e < floor ? floor : p_e): a NaN p_e stays NaN, and with floor == 0 and
//             p_e == 0 the term is -inf;
// and the request's three outputs are
//   ll[q]      = sum_e term_e
//   mass[q]    = sum_e v
//   floored[q] = #{e : v > 0 and p_e < floor}, int64.
// Both sums are taken in an order that depends on k and on the request's own segment only -- not on the other requests of the
// call, the grid, or the chunks the call is cut into --, so a request scored alone and among others returns the same bits.
//
// On the device a request's segment is cut into PIECES of at most LL_SEG entries, one wave each; loglik_lanes(k) lanes share an
// entry, a wave's G = 64 / lanes lane groups stride over the piece's entries, a piece leaves three partials and a request's
// pieces are added in ascending order.  A call is cut into CHUNKS of whole requests whose entries (12 bytes each: column and
// value) fit an upload budget.  The kernels (rri_loglik_kernels.hpp), the entry point (rri_entries_loglik) and the stand-alone
// CPU test (tests/c/loglik_main.cpp) take the term, the request check, the pieces, the chunks and the lane rule from here.
// loglik_plain is the definition as a host loop.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_topn.hpp"

namespace rri {

constexpr int LL_SEG = 256;                          // entries per piece: what one wave sums before it stores its partials
constexpr int64_t LL_ENTRY_BYTES = 12;               // an uploaded entry: int32 column, float64 value
constexpr int64_t LL_UPLOAD_BUDGET = 64ll << 20;     // entries of one chunk on the device, in bytes (cooc's 64 MiB)

// lanes of a wave that share one entry: each takes pairs of topics, lane l the pairs l, l + lanes, ...  Four lanes up to k = 128,
// sixteen above: measured (tools/loglik_probe.py, profiles/r21_loglik_probe.jsonl) at k = 16 .. 1024 with 4, 16 and 64 lanes, the
// narrower group wins while a lane's share of an entry is short -- more entries of a piece are in flight --: 4 lanes are the
// fastest up to k = 129, 16 lanes from k = 192 to 1024, and a whole wave per entry nowhere (the kernel keeps that instantiation
// for the measurement build).
#ifdef RRI_LOGLIK_LANES      // a measurement build (tools/loglik_probe.py --forced-lanes): one lane count, 4, 16 or 64, for every k
RRI_TOPN_FN int loglik_lanes(int) { return RRI_LOGLIK_LANES; }
#else
RRI_TOPN_FN int loglik_lanes(int k) { return k <= 128 ? 4 : 16; }
#endif
// the width of a row of the transposed copy of T and of the staged row of W: k rounded up to whole pairs, the pad zero
RRI_TOPN_FN int loglik_kp(int k) { return (k + 1) & ~1; }

// the term of one entry, and whether it counts as floored
RRI_TOPN_FN double loglik_term(double v, double p, double floor) { return v == 0.0 ? 0.0 : v * log(p < floor ? floor : p); }
RRI_TOPN_FN int loglik_floored(double v, double p, double floor) { return (int)(v > 0.0) & (int)(p < floor); }

// ---- a request, checked on the host before anything is copied -------------------------------------------------------------------
// One pass over the arrays.  n, d: the shape of W T.  Returns TOPN_REQ_OK, TOPN_REQ_INVALID or TOPN_REQ_UNSUPPORTED (a d whose
// full row does not fit one chunk) and writes the first broken rule to msg.
inline int loglik_check_request(int64_t n, int64_t d, const int64_t* rows, int64_t count, const int64_t* indptr,
                                const int32_t* indices, const double* values, double floor, const double* ll_out,
                                const double* mass_out, const int64_t* floored_out, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    if (count < 0) return say(TOPN_REQ_INVALID, "count %lld is negative", (long long)count, 0);
    if (!(floor >= 0.0) || std::isinf(floor)) {
        if (msg && msg_len) snprintf(msg, msg_len, "floor %g is not a finite number >= 0", floor);
        return TOPN_REQ_INVALID;
    }
    if (LL_ENTRY_BYTES * d > LL_UPLOAD_BUDGET)
        return say(TOPN_REQ_UNSUPPORTED, "a full row of d = %lld entries does not fit the upload budget of %lld bytes", (long long)d, (long long)LL_UPLOAD_BUDGET);
    if (!indptr) return say(TOPN_REQ_INVALID, "indptr is NULL", 0, 0);
    if (!rows && count > n) return say(TOPN_REQ_INVALID, "rows is NULL and count %lld exceeds the %lld rows of W", (long long)count, (long long)n);
    if (count > 0 && (!ll_out || !mass_out || !floored_out)) return say(TOPN_REQ_INVALID, "an output array is NULL with %lld requests", (long long)count, 0);
    if (indptr[0] != 0) return say(TOPN_REQ_INVALID, "indptr[0] = %lld, not 0", (long long)indptr[0], 0);
    for (int64_t q = 0; q < count; ++q) {
        if (rows && (rows[q] < 0 || rows[q] >= n)) return say(TOPN_REQ_INVALID, "rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
        const int64_t p0 = indptr[q], p1 = indptr[q + 1];
        if (p1 < p0) return say(TOPN_REQ_INVALID, "indptr decreases at %lld", (long long)q + 1, 0);
        if (p1 > p0 && !indices) return say(TOPN_REQ_INVALID, "indices is NULL with entries in request %lld", (long long)q, 0);
        if (p1 > p0 && !values) return say(TOPN_REQ_INVALID, "values is NULL with entries in request %lld", (long long)q, 0);
        for (int64_t p = p0; p < p1; ++p) {
            if (indices[p] < 0 || indices[p] >= d) return say(TOPN_REQ_INVALID, "column %lld of request %lld is out of range", (long long)indices[p], (long long)q);
            if (p > p0 && indices[p] <= indices[p - 1]) return say(TOPN_REQ_INVALID, "columns of request %lld do not ascend strictly at entry %lld", (long long)q, (long long)p);
            if (!(values[p] >= 0.0) || std::isinf(values[p])) {
                if (msg && msg_len) snprintf(msg, msg_len, "value %g at entry %lld of request %lld is not a finite number >= 0", values[p], (long long)p, (long long)q);
                return TOPN_REQ_INVALID;
            }
        }
    }
    return TOPN_REQ_OK;
}

// ---- chunks: whole requests whose entries are on the device at a time ------------------------------------------------------------
// chunk c holds the requests [q0, q1) and with them the entries [indptr[q0], indptr[q1]): as many requests as fit `budget` bytes
// at LL_ENTRY_BYTES per entry, at least one.  Requests without entries ride along with the chunk in front of them.
struct LoglikChunk {
    int64_t q0, q1;
};
// the number of chunks of `count` requests; out (NULL: count only) takes them.  No request, no chunk.
inline int64_t loglik_cut_chunks(const int64_t* indptr, int64_t count, int64_t budget, std::vector<LoglikChunk>* out) {
    const int64_t cap = budget / LL_ENTRY_BYTES;
    int64_t nc = 0;
    for (int64_t q0 = 0; q0 < count; ++nc) {
        int64_t q1 = q0 + 1;
        while (q1 < count && indptr[q1 + 1] - indptr[q0] <= cap) ++q1;
        if (out) out->push_back(LoglikChunk{q0, q1});
        q0 = q1;
    }
    return nc;
}

// ---- pieces: what one wave sums -------------------------------------------------------------------------------------------------
// The segments of the requests [q0, q1) of a chunk, each cut into pieces of at most LL_SEG entries, in order.  A request without
// entries gets no piece.  req and e0 are relative to the chunk: request q0 + req, entry indptr[q0] + e0.
struct LoglikPiece {
    int64_t e0;       // its first entry inside the chunk's entries
    int32_t req;      // the request inside the chunk
    int32_t cnt;      // 1 .. LL_SEG entries
};
// the number of pieces; out (NULL: count only) takes them, and first (NULL or q1 - q0 + 1 entries) the index of every request's
// first piece: the pieces of request r are first[r] .. first[r + 1])
inline int64_t loglik_cut_pieces(const int64_t* indptr, int64_t q0, int64_t q1, LoglikPiece* out, int64_t* first) {
    int64_t np = 0;
    for (int64_t q = q0; q < q1; ++q) {
        if (first) first[q - q0] = np;
        for (int64_t t = indptr[q]; t < indptr[q + 1]; t += LL_SEG, ++np)
            if (out) {
                const int64_t c = indptr[q + 1] - t < LL_SEG ? indptr[q + 1] - t : LL_SEG;
                out[np] = LoglikPiece{t - indptr[q0], (int32_t)(q - q0), (int32_t)c};
            }
    }
    if (first) first[q1 - q0] = np;
    return np;
}

// ---- the definition as a host loop ----------------------------------------------------------------------------------------------
// W n x k and T k x d, row-major; the request is a checked one.  Topics and entries in ascending order.
inline void loglik_plain(const double* W, const double* T, int64_t d, int k, const int64_t* rows, int64_t count, const int64_t* indptr,
                         const int32_t* indices, const double* values, double floor, double* ll, double* mass, int64_t* floored) {
    for (int64_t q = 0; q < count; ++q) {
        const int64_t i = rows ? rows[q] : q;
        double s = 0.0, m = 0.0;
        int64_t f = 0;
        for (int64_t e = indptr[q]; e < indptr[q + 1]; ++e) {
            double p = 0.0;
            for (int t = 0; t < k; ++t) p += W[i * k + t] * T[(int64_t)t * d + indices[e]];
            s += loglik_term(values[e], p, floor);
            m += values[e];
            f += loglik_floored(values[e], p, floor);
        }
        ll[q] = s;
        mass[q] = m;
        floored[q] = f;
    }
}

}  // namespace rri
