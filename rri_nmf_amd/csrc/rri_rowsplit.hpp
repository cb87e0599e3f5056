// rri_rowsplit.hpp -- the split of a resident corpus that holds out an exact number of entries of every row, written once (DESIGN
// "A split by row"): leave-k-out, and the per-user split of users a fit never saw.
//
// KEY.  Entry (i, j) of the canonical source has the 64-bit key K = (word0 << 32) | (uint32)j, word0 being word 0 of
// split_block(i, j, seed, 0) -- the Philox4x32-10 of rri_derive.hpp with the key and the counter rri_corpus_split_entries uses.  The
// columns of a canonical row are distinct, so the keys of a row are distinct; every comparison is on the whole key, never on word0
// alone, and there is no separate path for ties: two entries of one word0 are ordered by their column.  j < 2^31, so the largest key
// is below 2^64 - 1 and K + 1 never wraps.
// QUOTA.  Row i with L stored entries gives up h = rowsplit_quota(L, n_held, fraction, min_observed) of them:
//   want = n_held                           (count mode: n_held >= 1, fraction == 0)
//   want = floor(fraction * L + 0.5)        (fraction mode: n_held == -1, 0 < fraction <= 1; in double)
//   h    = min(want, max(L - min_observed, 0))
// so a row never keeps fewer than min_observed entries unless it has fewer, and then it gives up none.
// SPLIT (src, n_held, fraction, min_observed, seed) -> (observed, held).  The h entries of the row with the smallest keys go to
// `held`, the others to `observed`, each in source order.  Values are copied bit for bit and are not looked at.  Both outputs have the
// source's shape and are canonical, their patterns are disjoint, their union is the source's, and row i of `held` has exactly h
// entries.  In terms of a per-row BOUND: bound = 0 for h = 0, all ones for h = L, and otherwise K* + 1 with K* the h-th smallest key
// of the row; entry (i, j) is held iff K < bound.
// Two properties follow from "the h smallest of one fixed order" and the tests use them:
//   NESTED IN THE QUOTA.  The held set of a row for h is inside its held set for h + 1, under one seed.
//   AGREES WITH split_entries.  split_entries(thr, seed) holds the entries with word0 < thr, and every key with word0 < thr is below
//   every key with word0 >= thr.  So if it holds m entries of row i, those are the m smallest keys of the row: a split of rows whose
//   quota for row i is m holds the same m entries under the same seed.
// REFUSALS (rowsplit_check_request, all INVALID): a NULL output; n_held == 0; n_held below -1; both modes at once (a count with a
// fraction that is not 0, NaN included); in fraction mode a fraction outside (0, 1], NaN included; a negative min_observed.
//
// On the device (rri_rowsplit_kernels.hpp) the host computes the quotas from its copy of indptr and lists the rows with 0 < h < L by
// class: up to ROWSPLIT_WAVE_MAX entries (a wave ranks the keys) and longer (a workgroup runs a radix select, ROWSPLIT_PASSES passes
// of ROWSPLIT_DIGIT_BITS bits from the top).  Count and write walk the pieces of derive_cut_pieces with the predicate K < bound.
//
// split_rows_plain is the definition as a host loop; the word0 of an entry is a template parameter so that a test can make every
// word0 equal and see the columns decide.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_corpus_build.hpp"
#include "rri_derive.hpp"

namespace rri {

constexpr int ROWSPLIT_WAVE_MAX = 64;               // the longest row a wave ranks: a key per lane
constexpr int ROWSPLIT_BLOCK_THREADS = 256;         // the workgroup of the radix select: a thread per bin
constexpr int ROWSPLIT_DIGIT_BITS = 8;
constexpr int ROWSPLIT_BINS = 1 << ROWSPLIT_DIGIT_BITS;
constexpr int ROWSPLIT_PASSES = 64 / ROWSPLIT_DIGIT_BITS;
constexpr uint64_t ROWSPLIT_BOUND_NONE = 0ull, ROWSPLIT_BOUND_ALL = ~0ull;
enum { ROWSPLIT_CLASS_NONE = 0, ROWSPLIT_CLASS_WAVE = 1, ROWSPLIT_CLASS_BLOCK = 2 };

// ---- the key and the quota -----------------------------------------------------------------------------------------------------
RRI_TOPN_FN uint64_t rowsplit_key_of(uint32_t word0, int32_t col) { return ((uint64_t)word0 << 32) | (uint64_t)(uint32_t)col; }
struct RowsplitWord0 {
    RRI_TOPN_FN uint32_t operator()(int64_t row, int32_t col, uint64_t seed) const { return split_block(row, col, seed, 0).w[0]; }
};
RRI_TOPN_FN uint64_t rowsplit_key(int64_t row, int32_t col, uint64_t seed) { return rowsplit_key_of(RowsplitWord0()(row, col, seed), col); }

// a checked request: what a row of L entries gives up
inline int64_t rowsplit_quota(int64_t L, int64_t n_held, double fraction, int64_t min_observed) {
    const int64_t want = n_held >= 1 ? n_held : (int64_t)std::floor(fraction * (double)L + 0.5);
    const int64_t spare = L - min_observed > 0 ? L - min_observed : 0;
    return want < spare ? want : spare;
}
// which selection a row needs: none (its bound is known: nothing or everything), a wave's, a workgroup's
inline int rowsplit_class(int64_t L, int64_t h) { return h <= 0 || h >= L ? ROWSPLIT_CLASS_NONE : L <= ROWSPLIT_WAVE_MAX ? ROWSPLIT_CLASS_WAVE : ROWSPLIT_CLASS_BLOCK; }

// ---- the request, checked on the host before any device call -------------------------------------------------------------------
inline int rowsplit_check_request(int64_t n_held, double fraction, int64_t min_observed, bool has_observed, bool has_held, char* msg,
                                  size_t msg_len) {
    auto say = [&](const char* what, long long a, double b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return (int)TOPN_REQ_INVALID;
    };
    if (!has_observed || !has_held) return say("the output pointer is NULL", 0, 0.0);
    if (n_held == 0) return say("n_held 0 holds nothing out: a count is at least 1", 0, 0.0);
    if (n_held < -1) return say("n_held %lld is neither a count nor -1, which asks for a fraction", (long long)n_held, 0.0);
    if (n_held >= 1 && !(fraction == 0.0)) return say("n_held %lld and fraction %g are both given: a split of rows takes one of them", (long long)n_held, fraction);
    if (n_held == -1 && !(fraction > 0.0 && fraction <= 1.0)) {
        if (msg && msg_len) snprintf(msg, msg_len, "fraction %g is outside (0, 1]", fraction);
        return (int)TOPN_REQ_INVALID;
    }
    if (min_observed < 0) return say("min_observed %lld is negative", (long long)min_observed, 0.0);
    return TOPN_REQ_OK;
}

// ---- the definition as a host loop ---------------------------------------------------------------------------------------------
// the bound of a row from its keys (any order): entry is held iff key < bound
inline uint64_t rowsplit_bound_plain(std::vector<uint64_t> keys, int64_t h) {
    if (h <= 0) return ROWSPLIT_BOUND_NONE;
    if (h >= (int64_t)keys.size()) return ROWSPLIT_BOUND_ALL;
    std::nth_element(keys.begin(), keys.begin() + (h - 1), keys.end());
    return keys[(size_t)h - 1] + 1;
}
// a checked request on a canonical source: observed and held
template <typename Word0 = RowsplitWord0>
inline void split_rows_plain(const DeriveCsr& a, int64_t n_held, double fraction, int64_t min_observed, uint64_t seed, DeriveCsr* observed,
                             DeriveCsr* held, Word0 word0 = Word0()) {
    for (DeriveCsr* o : {observed, held}) {
        o->n_rows = a.n_rows;
        o->n_cols = a.n_cols;
        o->indptr.assign(1, 0);
        o->indices.clear();
        o->values.clear();
    }
    std::vector<uint64_t> keys;
    for (int64_t r = 0; r < a.n_rows; ++r) {
        const int64_t lo = a.indptr[(size_t)r], hi = a.indptr[(size_t)r + 1];
        keys.clear();
        for (int64_t p = lo; p < hi; ++p) keys.push_back(rowsplit_key_of(word0(r, a.indices[(size_t)p], seed), a.indices[(size_t)p]));
        const uint64_t bound = rowsplit_bound_plain(keys, rowsplit_quota(hi - lo, n_held, fraction, min_observed));
        for (int64_t p = lo; p < hi; ++p) {
            DeriveCsr* o = keys[(size_t)(p - lo)] < bound ? held : observed;
            o->indices.push_back(a.indices[(size_t)p]);
            o->values.push_back(a.values[(size_t)p]);
        }
        held->indptr.push_back((int64_t)held->indices.size());
        observed->indptr.push_back((int64_t)observed->indices.size());
    }
}

}  // namespace rri
