// rri_topn.hpp -- the order of a top-N list, written once (DESIGN "Top-N rows").
//
// A requested row i has the scores s_ij = sum_t W[i,t] T[t,j], float64.  Its ELIGIBLE columns are 0 .. d-1 without the row's
// excluded columns and without the columns whose score is NaN.  The order among them: the larger score first, and among equal
// scores the smaller column first -- a total order, so a list does not depend on the order in which its candidates arrive.
// The answer is the first min(N, eligible) columns of that order with their scores; the slots after them hold the index -1
// and the value NaN.  The scores are ranked UNCLIPPED (a clip to the rating range would tie every strong item at the upper
// bound); topn_clip is applied to the values that leave, and a NaN bound leaves that side open.
//
// The kernel (k_topn_rows, rri_topn_kernels.hpp), the entry point (rri_topn_rows) and the stand-alone CPU test
// (tests/c/topn_main.cpp) all take the comparison, the place of a candidate, the exclusion search, the clip and the validation
// of a request from here.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <cstdint>
#include <cstdio>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RRI_TOPN_FN __host__ __device__ inline
#else
#define RRI_TOPN_FN inline
#endif

namespace rri {

// does candidate (v1, column j1) stand before (v2, j2)?  Neither value is NaN (a NaN score is not eligible).
RRI_TOPN_FN bool topn_before(double v1, int j1, double v2, int j2) { return v1 > v2 || (v1 == v2 && j1 < j2); }

// A list of N slots, sorted, its filled slots first; an empty slot has the index -1 (and the value NaN).
// May (v, j) enter a list whose LAST slot holds (vl, jl)?  Yes while that slot is empty, else when it stands before it.
RRI_TOPN_FN bool topn_enters(double v, int j, double vl, int jl) { return v == v && (jl < 0 || topn_before(v, j, vl, jl)); }
// does slot (vs, js) stay in front of the candidate (v, j)?  The candidate's place is the number of slots that do.
RRI_TOPN_FN bool topn_stays_ahead(double vs, int js, double v, int j) { return js >= 0 && topn_before(vs, js, v, j); }

// Bounded sorted insertion: (v, j) goes to its place, what stood there and behind moves one slot back, the last slot drops
// out.  Returns whether the list changed: a NaN v, or a candidate that does not stand before a full list's last slot, leaves it.
RRI_TOPN_FN bool topn_insert(double* vals, int* idx, int N, double v, int j) {
    if (N < 1 || !topn_enters(v, j, vals[N - 1], idx[N - 1])) return false;
    int pos = 0;
    while (pos < N && topn_stays_ahead(vals[pos], idx[pos], v, j)) ++pos;
    for (int p = N - 1; p > pos; --p) { vals[p] = vals[p - 1]; idx[p] = idx[p - 1]; }
    vals[pos] = v;
    idx[pos] = j;
    return true;
}

// the value that leaves: clipped to [lo, hi], a NaN bound leaving its side open
RRI_TOPN_FN double topn_clip(double v, double lo, double hi) {
    if (lo == lo && v < lo) v = lo;
    if (hi == hi && v > hi) v = hi;
    return v;
}

// first position in the ascending segment e[lo .. hi) whose entry is not below j (hi when there is none): j is excluded when
// that position is inside the segment and holds j
RRI_TOPN_FN int64_t topn_lower_bound(const int32_t* e, int64_t lo, int64_t hi, int j) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (e[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
RRI_TOPN_FN bool topn_excluded(const int32_t* e, int64_t lo, int64_t hi, int j) {
    const int64_t p = topn_lower_bound(e, lo, hi, j);
    return p < hi && e[p] == j;
}

// ---- a request, checked on the host before anything is copied -------------------------------------------------------------------
// rows (NULL: rows 0 .. count-1, so count <= n) inside [0, n), in any order, duplicates allowed; 1 <= topn <= max_topn; the
// exclusion (indptr NULL: none) a CSR pattern with one row per request: indptr[0] = 0, monotone, count + 1 entries; the indices
// of a row strictly ascending and inside [0, d).  Returns 0, TOPN_REQ_INVALID or TOPN_REQ_UNSUPPORTED (a topn outside
// 1 .. max_topn: a list length this library does not build) and writes what is wrong to msg.
enum { TOPN_REQ_OK = 0, TOPN_REQ_INVALID = -1, TOPN_REQ_UNSUPPORTED = -3 };   // = RRI_OK, RRI_ERR_INVALID, RRI_ERR_UNSUPPORTED
inline int topn_check_request(int64_t n, int64_t d, const int64_t* rows, int64_t count, int32_t topn, int32_t max_topn,
                              const int64_t* indptr, const int32_t* indices, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return code;
    };
    if (count < 0) return say(TOPN_REQ_INVALID, "count %lld is negative", (long long)count, 0);
    if (topn < 1 || topn > max_topn) return say(TOPN_REQ_UNSUPPORTED, "topn %lld outside 1 .. %lld", (long long)topn, (long long)max_topn);
    if (!rows && count > n) return say(TOPN_REQ_INVALID, "rows is NULL and count %lld exceeds the %lld rows of W", (long long)count, (long long)n);
    if (rows)
        for (int64_t q = 0; q < count; ++q)
            if (rows[q] < 0 || rows[q] >= n) return say(TOPN_REQ_INVALID, "rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
    if (!indptr) return TOPN_REQ_OK;
    if (indptr[0] != 0) return say(TOPN_REQ_INVALID, "excl_indptr[0] = %lld, not 0", (long long)indptr[0], 0);
    for (int64_t q = 0; q < count; ++q)
        if (indptr[q + 1] < indptr[q]) return say(TOPN_REQ_INVALID, "excl_indptr decreases at %lld", (long long)q + 1, 0);
    if (indptr[count] > 0 && !indices) return say(TOPN_REQ_INVALID, "excl_indices is NULL with %lld entries", (long long)indptr[count], 0);
    for (int64_t q = 0; q < count; ++q)
        for (int64_t p = indptr[q]; p < indptr[q + 1]; ++p) {
            if (indices[p] < 0 || indices[p] >= d) return say(TOPN_REQ_INVALID, "excluded column %lld of request %lld is out of range", (long long)indices[p], (long long)q);
            if (p > indptr[q] && indices[p] <= indices[p - 1]) return say(TOPN_REQ_INVALID, "excluded columns of request %lld do not ascend strictly at entry %lld", (long long)q, (long long)p);
        }
    return TOPN_REQ_OK;
}

}  // namespace rri
