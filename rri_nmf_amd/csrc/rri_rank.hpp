// rri_rank.hpp -- the rank of a held-out column in a row's total order, written once (DESIGN "Ranks of entries").
//
// A request q has a row i of W, an optional exclusion segment (as in rri_topn.hpp) and a TARGET segment: columns strictly
// ascending inside [0, d).  Eligibility and order are rri_topn.hpp's: a column is eligible if the request does not exclude it
// and its score s_ij = sum_t W[i,t] T[t,j] is not NaN; the larger score stands first and, among equal scores, the smaller column.
// For a target column j of request q
//   rank(q, j)   the number of eligible columns j' != j that stand before (s_ij, j) -- topn_before(s_ij', j', s_ij, j) --: the
//                0-based place j would have in an unbounded top-N list.  Other targets of the row count as competitors.  -1 when
//                j itself is not eligible (excluded, or its score is NaN);
//   val(q, j)    topn_clip(s_ij, lo, hi) when j is eligible, else NaN: the number a top-N list would return for the column;
//   eligible(q)  the number of eligible columns of the request.
//
// The kernel (k_rank_entries, rri_rank_kernels.hpp), the entry point (rri_rank_entries) and the stand-alone CPU test
// (tests/c/rank_main.cpp) take the predicates, the validation of a request and the cut of the target segments into pieces from
// here.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include "rri_topn.hpp"

namespace rri {

constexpr int RANK_SEG = 64;     // targets per piece: one per lane of the wave that counts for the piece

// does column jc with score vc (not excluded by the request: the caller has looked) count towards the rank of target (vt, jt)?
// It does when  vc == vc && jc != jt && topn_before(vc, jc, vt, jt).  rank_counts is that sentence without a branch -- the kernel
// asks it 400 times per chunk and wave, and the short-circuit form compiled to eight branches per question --: a NaN vc fails
// both comparisons, so vc == vc need not be asked.  tests/c/rank_main.cpp holds the two forms against each other.
RRI_TOPN_FN bool rank_counts_plain(double vc, int jc, double vt, int jt) { return vc == vc && jc != jt && topn_before(vc, jc, vt, jt); }
RRI_TOPN_FN bool rank_counts(double vc, int jc, double vt, int jt) {
    return (bool)((int)(jc != jt) & ((int)(vc > vt) | ((int)(vc == vt) & (int)(jc < jt))));
}
// the rank that leaves: the count when the target is eligible itself, else -1; and its value
RRI_TOPN_FN int rank_result(int counted, double vt, bool excluded) { return (vt == vt && !excluded) ? counted : -1; }
RRI_TOPN_FN double rank_value(double vt, bool excluded, double lo, double hi) {
    return (vt == vt && !excluded) ? topn_clip(vt, lo, hi) : __builtin_nan("");
}

// ---- a request, checked on the host before anything is copied -------------------------------------------------------------------
// rows, count and the exclusion as topn_check_request has them; the targets a CSR pattern with one row per request whose indptr
// is REQUIRED: tgt_indptr[0] = 0, monotone, count + 1 entries; the columns of a request strictly ascending and inside [0, d).
// Returns TOPN_REQ_OK or TOPN_REQ_INVALID and writes what is wrong to msg.
inline int rank_check_request(int64_t n, int64_t d, const int64_t* rows, int64_t count, const int64_t* tgt_indptr,
                              const int32_t* tgt_indices, const int64_t* excl_indptr, const int32_t* excl_indices, char* msg,
                              size_t msg_len) {
    auto say = [&](const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return (int)TOPN_REQ_INVALID;
    };
    const int bad = topn_check_request(n, d, rows, count, 1, 1, excl_indptr, excl_indices, msg, msg_len);
    if (bad != TOPN_REQ_OK) return bad;
    if (!tgt_indptr) return say("tgt_indptr is NULL", 0, 0);
    if (tgt_indptr[0] != 0) return say("tgt_indptr[0] = %lld, not 0", (long long)tgt_indptr[0], 0);
    for (int64_t q = 0; q < count; ++q)
        if (tgt_indptr[q + 1] < tgt_indptr[q]) return say("tgt_indptr decreases at %lld", (long long)q + 1, 0);
    if (tgt_indptr[count] > 0 && !tgt_indices) return say("tgt_indices is NULL with %lld entries", (long long)tgt_indptr[count], 0);
    for (int64_t q = 0; q < count; ++q)
        for (int64_t p = tgt_indptr[q]; p < tgt_indptr[q + 1]; ++p) {
            if (tgt_indices[p] < 0 || tgt_indices[p] >= d) return say("target column %lld of request %lld is out of range", (long long)tgt_indices[p], (long long)q);
            if (p > tgt_indptr[q] && tgt_indices[p] <= tgt_indices[p - 1]) return say("target columns of request %lld do not ascend strictly at entry %lld", (long long)q, (long long)p);
        }
    return TOPN_REQ_OK;
}

// ---- pieces: what one wave counts for at a time -------------------------------------------------------------------------------
// A request's target segment is cut into pieces of at most RANK_SEG targets, in order; a request without a target still gets one
// (empty) piece, so that its eligible count is taken.  `first` marks the piece that reports eligible(q).
struct RankPiece {
    int64_t req;      // the request
    int64_t t0;       // its first target: an index into tgt_indices (and into the outputs)
    int32_t cnt;      // 0 .. RANK_SEG targets
    int32_t first;    // 1: the request's first piece
};
// the number of pieces of `count` requests; out (NULL: count only) takes them
inline int64_t rank_cut_pieces(const int64_t* tgt_indptr, int64_t count, RankPiece* out) {
    int64_t np = 0;
    for (int64_t q = 0; q < count; ++q) {
        int64_t t = tgt_indptr[q];
        const int64_t t1 = tgt_indptr[q + 1];
        bool first = true;
        do {
            const int64_t c = t1 - t < RANK_SEG ? t1 - t : RANK_SEG;
            if (out) out[np] = RankPiece{q, t, (int32_t)c, first ? 1 : 0};
            ++np;
            t += c;
            first = false;
        } while (t < t1);
    }
    return np;
}

}  // namespace rri
