// rri_corpus_build.hpp -- the two ends of the resident-corpus chain, written once (DESIGN "A corpus from pairs; a split by entry"):
// a corpus from a list of (row, column, value) pairs, and a split of a corpus that sends every entry, whole, to one of two parts.
//
// FROM PAIRS.  Pair p (0 <= p < n_pairs) is (rows[p * stride], cols[p * stride], values[p]): the two index arrays share a dtype
// (RRI_I32 or RRI_I64) and a stride in elements (1: two arrays; 2 with cols == rows + 1: an interleaved (m, 2) array), the values
// are RRI_F32, RRI_F64 or absent (NULL: every pair counts 1).  The result is, byte for byte, the corpus rri_corpus_create makes of
// the raw CSR matrix whose row i holds the pairs of row i in the order they were given -- a stable sort of the pairs by row -- and
// so the canonical form of rri_corpus.hpp: the values of one (i, j) added in float64 in the order given, starting from the first;
// a sum that is exactly 0 dropped; float32 widened exactly.  The statistics are that matrix's too: stored = n_pairs; rows
// REWRITTEN = rows whose pairs, as given, do not ascend strictly by column or hold a zero value; duplicates, zeros, negatives,
// long rows.  Before any array is read the arguments are held against (INVALID) a negative size, an unknown dtype code, a stride
// below 1 and a NULL index array with pairs, then (UNSUPPORTED) n_cols >= 2^31 and n_pairs > CB_PAIRS_MAX: the pair position is
// half of a sort key.  Then the CHECK tests, each rule over all positions before the next,
//   0  a row outside [0, n_rows)           1  a column outside [0, n_cols)           2  a NaN or infinite value
// and names the smallest offending pair position of the first broken rule, so the host loop here and the device (an integer
// minimum per rule) give the same text.  It reads by position only, and nothing else runs before it has passed.
// One thing differs from rri_corpus_create: a row of more than CORPUS_ROW_MAX pairs is refused (UNSUPPORTED) whether or not its
// pairs were given in canonical order, because every row is sorted here.
//
// On the device (rri_corpus_build_kernels.hpp): check; count the pairs of every row; the host takes the exclusive scan; every pair
// claims a slot of its row; every row is sorted by the 64-bit key (column << 32 | pair position), which carries the given order,
// so the arbitrary order in which slots are claimed cannot reach the result (the argument of corpus_key in rri_corpus.hpp, with
// the global position in place of the position inside the row); merge, compact, count.  Count and claim walk the list in
// consecutive runs of CB_WAVE_PAIRS pairs, a wave each, CB_BLOCK_PAIRS per workgroup, at most CB_GRID_MAX workgroups and
// grid-stride beyond: inside a wave a run of equal rows issues ONE integer atomic.  The classes of a row by its length are
// rri_corpus.hpp's.  After the sort a row was canonical as given iff its positions ascend, no column repeats and no value is 0.
//
// SPLIT BY ENTRY (src, thr, seed) -> (observed, held).  Entry (i, j) of the canonical source goes to `held` when word 0 of
// split_block(i, j, seed, 0) -- the Philox4x32-10 of rri_derive.hpp, same key and counter -- is below thr, and to `observed`
// otherwise: a function of (row, column, seed) alone, so an entry whose count is 1 goes the same way here and in
// rri_corpus_split.  Values are copied bit for bit and are not looked at.  Both outputs have the source's shape and are canonical,
// their patterns are disjoint and their union is the source's.  INVALID for a threshold of 0 (derive_check_split).  On the
// device the source is walked in the pieces of derive_cut_pieces: count per piece, scan on the host, write.
//
// corpus_from_pairs_plain and split_entries_plain are the definitions as host loops.  Plain inline functions; nothing in this
// file needs HIP.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_corpus.hpp"
#include "rri_derive.hpp"

namespace rri {

constexpr int CB_WAVE_PAIRS = 64;                  // consecutive pairs of one wave: the reach of the aggregation of equal rows
constexpr int CB_BLOCK_PAIRS = 256;                // ... of one workgroup: four waves
constexpr int CB_GRID_MAX = 1024;                  // the most workgroups of a pass over the pairs: grid-stride beyond
constexpr int64_t CB_SWEEP_PAIRS = (int64_t)CB_BLOCK_PAIRS * CB_GRID_MAX;      // the pairs of one stride of the full grid
constexpr int64_t CB_PAIRS_MAX = 0x7fffffffLL;     // the most pairs of a list: the position is the low half of a key
enum { CB_RULES = 3 };

struct CorpusPairs {
    int64_t n_rows, n_cols, n_pairs;
    const void* rows;
    const void* cols;
    int index_dtype;
    int64_t index_stride;
    const void* values;      // NULL: every pair counts 1
    int values_dtype;
};
RRI_TOPN_FN int64_t pairs_index(const void* a, int dtype, int64_t stride, int64_t p) { return corpus_idx(a, dtype, p * stride); }

// the workgroups of a pass over n_pairs pairs
inline unsigned pairs_grid(int64_t n_pairs) {
    const int64_t g = (n_pairs + CB_BLOCK_PAIRS - 1) / CB_BLOCK_PAIRS;
    return (unsigned)(g < 1 ? 1 : g > CB_GRID_MAX ? CB_GRID_MAX : g);
}

// ---- the check -----------------------------------------------------------------------------------------------------------------
inline void pairs_rule_text(int rule, int64_t pos, int64_t ival, double dval, char* msg, size_t msg_len) {
    if (!msg || !msg_len) return;
    switch (rule) {
        case 0: snprintf(msg, msg_len, "row %lld at pair %lld is out of range", (long long)ival, (long long)pos); break;
        case 1: snprintf(msg, msg_len, "column %lld at pair %lld is out of range", (long long)ival, (long long)pos); break;
        default: snprintf(msg, msg_len, "value %g at pair %lld is not finite", dval, (long long)pos); break;
    }
}
// The sizes, the codes and the pointers, before any array is read: TOPN_REQ_OK, TOPN_REQ_INVALID or TOPN_REQ_UNSUPPORTED and the text
inline int pairs_check_args(const CorpusPairs& m, char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a);
        return code;
    };
    if (m.n_rows < 0) return say(TOPN_REQ_INVALID, "n_rows %lld is negative", (long long)m.n_rows);
    if (m.n_cols < 0) return say(TOPN_REQ_INVALID, "n_cols %lld is negative", (long long)m.n_cols);
    if (m.n_pairs < 0) return say(TOPN_REQ_INVALID, "n_pairs %lld is negative", (long long)m.n_pairs);
    if (!corpus_index_dtype(m.index_dtype)) return say(TOPN_REQ_INVALID, "index dtype code %lld is neither RRI_I32 nor RRI_I64", (long long)m.index_dtype);
    if (m.values && !corpus_value_dtype(m.values_dtype)) return say(TOPN_REQ_INVALID, "values dtype code %lld is neither RRI_F32 nor RRI_F64", (long long)m.values_dtype);
    if (m.index_stride < 1) return say(TOPN_REQ_INVALID, "index_stride %lld is below 1", (long long)m.index_stride);
    if (m.n_pairs > 0 && !m.rows) return say(TOPN_REQ_INVALID, "rows is NULL with %lld pairs", (long long)m.n_pairs);
    if (m.n_pairs > 0 && !m.cols) return say(TOPN_REQ_INVALID, "cols is NULL with %lld pairs", (long long)m.n_pairs);
    if (m.n_cols > 0x7fffffffLL) return say(TOPN_REQ_UNSUPPORTED, "n_cols %lld is 2^31 or more", (long long)m.n_cols);
    if (m.n_pairs > CB_PAIRS_MAX) return say(TOPN_REQ_UNSUPPORTED, "n_pairs %lld is above 2^31 - 1: the pair position is half of a sort key", (long long)m.n_pairs);
    return TOPN_REQ_OK;
}
// The arguments, then the three rules over host arrays, each over all positions before the next.  Reads by position only
inline int pairs_check(const CorpusPairs& m, char* msg, size_t msg_len) {
    const int bad = pairs_check_args(m, msg, msg_len);
    if (bad != TOPN_REQ_OK) return bad;
    for (int64_t p = 0; p < m.n_pairs; ++p) {
        const int64_t i = pairs_index(m.rows, m.index_dtype, m.index_stride, p);
        if (i < 0 || i >= m.n_rows) return pairs_rule_text(0, p, i, 0.0, msg, msg_len), TOPN_REQ_INVALID;
    }
    for (int64_t p = 0; p < m.n_pairs; ++p) {
        const int64_t j = pairs_index(m.cols, m.index_dtype, m.index_stride, p);
        if (j < 0 || j >= m.n_cols) return pairs_rule_text(1, p, j, 0.0, msg, msg_len), TOPN_REQ_INVALID;
    }
    for (int64_t p = 0; m.values && p < m.n_pairs; ++p) {
        const double v = corpus_val(m.values, m.values_dtype, p);
        if (!corpus_finite(v)) return pairs_rule_text(2, p, 0, v, msg, msg_len), TOPN_REQ_INVALID;
    }
    return TOPN_REQ_OK;
}

// ---- the definitions as host loops ---------------------------------------------------------------------------------------------
// a checked list: the canonical form of the raw CSR matrix whose row i holds the pairs of row i in the order given
inline CorpusCanonical corpus_from_pairs_plain(const CorpusPairs& m) {
    std::vector<int64_t> indptr((size_t)m.n_rows + 1, 0), at, indices((size_t)m.n_pairs);
    std::vector<double> values((size_t)m.n_pairs);
    for (int64_t p = 0; p < m.n_pairs; ++p) indptr[(size_t)pairs_index(m.rows, m.index_dtype, m.index_stride, p) + 1] += 1;
    for (int64_t r = 0; r < m.n_rows; ++r) indptr[(size_t)r + 1] += indptr[(size_t)r];
    at.assign(indptr.begin(), indptr.end() - 1);
    for (int64_t p = 0; p < m.n_pairs; ++p) {          // in the order given: stable by row
        const int64_t slot = at[(size_t)pairs_index(m.rows, m.index_dtype, m.index_stride, p)]++;
        indices[(size_t)slot] = pairs_index(m.cols, m.index_dtype, m.index_stride, p);
        values[(size_t)slot] = corpus_val(m.values, m.values_dtype, p);
    }
    const CorpusRaw raw{m.n_rows, m.n_cols, m.n_pairs, indptr.data(), RRI_I64, indices.data(), RRI_I64, values.data(), RRI_F64};
    return corpus_canonical_plain(raw);
}
// every entry of a canonical source, whole, to one side
RRI_TOPN_FN bool split_entry_held(int64_t row, int32_t col, uint32_t thr, uint64_t seed) { return split_block(row, col, seed, 0).w[0] < thr; }
inline void split_entries_plain(const DeriveCsr& a, uint32_t thr, uint64_t seed, DeriveCsr* observed, DeriveCsr* held) {
    for (DeriveCsr* o : {observed, held}) {
        o->n_rows = a.n_rows;
        o->n_cols = a.n_cols;
        o->indptr.assign(1, 0);
        o->indices.clear();
        o->values.clear();
    }
    for (int64_t r = 0; r < a.n_rows; ++r) {
        for (int64_t p = a.indptr[(size_t)r]; p < a.indptr[(size_t)r + 1]; ++p) {
            DeriveCsr* o = split_entry_held(r, a.indices[(size_t)p], thr, seed) ? held : observed;
            o->indices.push_back(a.indices[(size_t)p]);
            o->values.push_back(a.values[(size_t)p]);
        }
        held->indptr.push_back((int64_t)held->indices.size());
        observed->indptr.push_back((int64_t)observed->indices.size());
    }
}

}  // namespace rri
