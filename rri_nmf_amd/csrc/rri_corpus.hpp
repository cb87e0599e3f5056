// rri_corpus.hpp -- a CSR corpus that lives on the device: what may come in, and what is kept, written once (DESIGN "A corpus on
// the device").
//
// The RAW matrix is n_rows x n_cols with nnz_stored entries: indptr (n_rows + 1 entries, RRI_I32 or RRI_I64), indices (RRI_I32 or
// RRI_I64) and values (RRI_F32, RRI_F64, or absent -- NULL: a pattern, every stored entry has the value 1).  Its rows may be
// unsorted, may hold a column several times and may hold explicit zeros.  It may not have, and the CHECK tests in this order,
//   0  indptr[0] != 0                      1  a decreasing indptr                  2  indptr[n_rows] != nnz_stored
//   3  a column outside [0, n_cols)        4  a NaN or infinite value              5  n_cols >= 2^31
// and names the smallest offending position of the first broken rule, so the host loop here and the device (which finds the
// smallest position of every rule by an integer minimum) give the same text for the same matrix.
//
// The CANONICAL form, row by row: the columns ascend strictly; the stored entries of one column are added in float64 in their
// stored order (a stable order by column, then a sequential sum that starts from the first of them); an entry whose sum is
// exactly 0 is dropped; a float32 value widens exactly.  Indices int32, values float64, indptr int64.  Beside it a corpus records
// how many rows were REWRITTEN (rows that were not strictly ascending without a stored zero: all others are copied as they
// are), how many DUPLICATES were merged (stored entries minus distinct columns per row), how many ZEROS were dropped (distinct
// columns whose sum is 0) and how many canonical values are NEGATIVE.  stored = canonical + duplicates + zeros.
//
// On the device a row that is to be rewritten is sorted by the 64-bit key (column << 32 | position inside the row), which makes
// any sorting network stable; the row's length picks its CLASS: up to CORPUS_WAVE_MAX entries one wave sorts it in registers, up
// to CORPUS_LDS_MAX a workgroup sorts it in LDS, padded to a power of two (at least CORPUS_PAD_MIN) with CORPUS_KEY_PAD, and a
// longer row is sorted by one workgroup in global memory.  The kernels (rri_corpus_kernels.hpp), the entry point
// (rri_corpus_create), the stand-alone CPU test (tests/c/corpus_main.cpp) and tests/corpus_cases.py, which mirrors the
// constants, take the loads, the check and its texts, the key, the classes and the pad from here.  corpus_canonical_plain is the
// definition as a host loop.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_hip.h"
#include "rri_topn.hpp"

namespace rri {

constexpr int CORPUS_WAVE_MAX = 64;            // B_wave: the longest row one wave sorts in registers, a key per lane
constexpr int CORPUS_LDS_MAX = 16384;          // B_lds: the longest row a workgroup sorts in LDS: 16384 keys of 8 bytes = 128 KiB of the CU's 160
constexpr int CORPUS_PAD_MIN = 128;            // the shortest padded row of the LDS class
constexpr int64_t CORPUS_ROW_MAX = 1ll << 30;  // the longest row that is rewritten at all (the position is half of a key)
constexpr unsigned long long CORPUS_KEY_PAD = ~0ull;        // above every real key: a column is below 2^31

enum { CORPUS_ROW_CANONICAL = 0, CORPUS_ROW_SHORT = 1, CORPUS_ROW_MEDIUM = 2, CORPUS_ROW_LONG = 3 };
enum { CORPUS_RULES = 6 };

// entry p of an index array and of the values, by their dtype codes
RRI_TOPN_FN int64_t corpus_idx(const void* a, int dtype, int64_t p) {
    return dtype == RRI_I32 ? (int64_t) reinterpret_cast<const int32_t*>(a)[p] : reinterpret_cast<const int64_t*>(a)[p];
}
RRI_TOPN_FN double corpus_val(const void* v, int dtype, int64_t p) {
    return !v ? 1.0 : dtype == RRI_F32 ? (double)reinterpret_cast<const float*>(v)[p] : reinterpret_cast<const double*>(v)[p];
}
RRI_TOPN_FN bool corpus_finite(double v) { return v - v == 0.0; }      // false for NaN and for either infinity

// the sort key of the stored entry at position pos of its row, and its halves
RRI_TOPN_FN unsigned long long corpus_key(int64_t col, int64_t pos) { return ((unsigned long long)col << 32) | (unsigned long long)pos; }
RRI_TOPN_FN unsigned corpus_key_col(unsigned long long key) { return (unsigned)(key >> 32); }
RRI_TOPN_FN unsigned corpus_key_pos(unsigned long long key) { return (unsigned)(key & 0xffffffffull); }

// the class of a row of `len` stored entries; flagged: it is not strictly ascending, or it holds a stored zero
RRI_TOPN_FN int corpus_row_class(bool flagged, int64_t len) {
    return !flagged ? CORPUS_ROW_CANONICAL : len <= CORPUS_WAVE_MAX ? CORPUS_ROW_SHORT : len <= CORPUS_LDS_MAX ? CORPUS_ROW_MEDIUM : CORPUS_ROW_LONG;
}
// the keys a row of the LDS or the global class is sorted as: the power of two at or above len, at least CORPUS_PAD_MIN
RRI_TOPN_FN int64_t corpus_pad(int64_t len) {
    int64_t p = CORPUS_PAD_MIN;
    while (p < len) p <<= 1;
    return p;
}

// ---- the check ---------------------------------------------------------------------------------------------------------------
struct CorpusRaw {
    int64_t n_rows, n_cols, nnz;
    const void* indptr;
    int indptr_dtype;
    const void* indices;
    int indices_dtype;
    const void* values;      // NULL: a pattern
    int values_dtype;
};
inline bool corpus_index_dtype(int dt) { return dt == RRI_I32 || dt == RRI_I64; }
inline bool corpus_value_dtype(int dt) { return dt == RRI_F32 || dt == RRI_F64; }
inline size_t corpus_dtype_size(int dt) { return dt == RRI_I32 || dt == RRI_F32 ? 4 : 8; }

// the text of broken rule `rule` at position pos; ival / dval: the offending number, bound: what it is held against
inline void corpus_rule_text(int rule, int64_t pos, int64_t ival, double dval, int64_t bound, char* msg, size_t msg_len) {
    if (!msg || !msg_len) return;
    switch (rule) {
        case 0: snprintf(msg, msg_len, "indptr[0] = %lld, not 0", (long long)ival); break;
        case 1: snprintf(msg, msg_len, "indptr decreases at %lld", (long long)pos); break;
        case 2: snprintf(msg, msg_len, "indptr ends at %lld, not at the %lld stored entries", (long long)ival, (long long)bound); break;
        case 3: snprintf(msg, msg_len, "column %lld at entry %lld is out of range", (long long)ival, (long long)pos); break;
        case 4: snprintf(msg, msg_len, "value %g at entry %lld is not finite", dval, (long long)pos); break;
        default: snprintf(msg, msg_len, "n_cols %lld is 2^31 or more", (long long)bound); break;
    }
}
// The shape and the pointers, before any array is read: TOPN_REQ_OK or TOPN_REQ_INVALID with its text
inline int corpus_check_args(const CorpusRaw& m, char* msg, size_t msg_len) {
    auto say = [&](const char* what, long long a) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a);
        return (int)TOPN_REQ_INVALID;
    };
    if (m.n_rows < 0) return say("n_rows %lld is negative", (long long)m.n_rows);
    if (m.n_cols < 0) return say("n_cols %lld is negative", (long long)m.n_cols);
    if (m.nnz < 0) return say("nnz_stored %lld is negative", (long long)m.nnz);
    if (!corpus_index_dtype(m.indptr_dtype)) return say("indptr dtype code %lld is neither RRI_I32 nor RRI_I64", (long long)m.indptr_dtype);
    if (!corpus_index_dtype(m.indices_dtype)) return say("indices dtype code %lld is neither RRI_I32 nor RRI_I64", (long long)m.indices_dtype);
    if (m.values && !corpus_value_dtype(m.values_dtype)) return say("values dtype code %lld is neither RRI_F32 nor RRI_F64", (long long)m.values_dtype);
    if (!m.indptr) return say("indptr is NULL", 0);
    if (m.nnz > 0 && !m.indices) return say("indices is NULL with %lld entries", (long long)m.nnz);
    return TOPN_REQ_OK;
}
// The six rules over host arrays, each over all its positions before the next: TOPN_REQ_OK, TOPN_REQ_INVALID or
// TOPN_REQ_UNSUPPORTED (rule 5) and the text.  Reads by position only: 0 .. n_rows and 0 .. nnz - 1.
inline int corpus_check(const CorpusRaw& m, char* msg, size_t msg_len) {
    const int bad = corpus_check_args(m, msg, msg_len);
    if (bad != TOPN_REQ_OK) return bad;
    const int64_t p0 = corpus_idx(m.indptr, m.indptr_dtype, 0), pn = corpus_idx(m.indptr, m.indptr_dtype, m.n_rows);
    if (p0 != 0) return corpus_rule_text(0, 0, p0, 0.0, 0, msg, msg_len), TOPN_REQ_INVALID;
    for (int64_t r = 1; r <= m.n_rows; ++r)
        if (corpus_idx(m.indptr, m.indptr_dtype, r) < corpus_idx(m.indptr, m.indptr_dtype, r - 1))
            return corpus_rule_text(1, r, 0, 0.0, 0, msg, msg_len), TOPN_REQ_INVALID;
    if (pn != m.nnz) return corpus_rule_text(2, m.n_rows, pn, 0.0, m.nnz, msg, msg_len), TOPN_REQ_INVALID;
    for (int64_t p = 0; p < m.nnz; ++p) {
        const int64_t j = corpus_idx(m.indices, m.indices_dtype, p);
        if (j < 0 || j >= m.n_cols) return corpus_rule_text(3, p, j, 0.0, m.n_cols, msg, msg_len), TOPN_REQ_INVALID;
    }
    for (int64_t p = 0; m.values && p < m.nnz; ++p) {
        const double v = corpus_val(m.values, m.values_dtype, p);
        if (!corpus_finite(v)) return corpus_rule_text(4, p, 0, v, 0, msg, msg_len), TOPN_REQ_INVALID;
    }
    if (m.n_cols > 0x7fffffffLL) return corpus_rule_text(5, 0, 0, 0.0, m.n_cols, msg, msg_len), TOPN_REQ_UNSUPPORTED;
    return TOPN_REQ_OK;
}

// ---- the definition as a host loop ----------------------------------------------------------------------------------------------
struct CorpusCanonical {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
    int64_t rows_rewritten = 0, duplicates = 0, zeros = 0, negatives = 0, long_rows = 0;
};
// is row [lo, hi) of a checked matrix one that is rewritten?
inline bool corpus_row_flagged(const CorpusRaw& m, int64_t lo, int64_t hi) {
    for (int64_t p = lo; p < hi; ++p) {
        if (corpus_val(m.values, m.values_dtype, p) == 0.0) return true;
        if (p > lo && corpus_idx(m.indices, m.indices_dtype, p) <= corpus_idx(m.indices, m.indices_dtype, p - 1)) return true;
    }
    return false;
}
// the canonical form of a checked matrix
inline CorpusCanonical corpus_canonical_plain(const CorpusRaw& m) {
    CorpusCanonical c;
    c.indptr.assign(1, 0);
    std::vector<unsigned long long> keys;
    for (int64_t r = 0; r < m.n_rows; ++r) {
        const int64_t lo = corpus_idx(m.indptr, m.indptr_dtype, r), hi = corpus_idx(m.indptr, m.indptr_dtype, r + 1);
        const int cls = corpus_row_class(corpus_row_flagged(m, lo, hi), hi - lo);
        c.rows_rewritten += cls != CORPUS_ROW_CANONICAL;
        c.long_rows += cls == CORPUS_ROW_LONG;
        keys.clear();
        for (int64_t p = lo; p < hi; ++p) keys.push_back(corpus_key(corpus_idx(m.indices, m.indices_dtype, p), p - lo));
        std::sort(keys.begin(), keys.end());           // the position is part of the key: any sort is stable
        for (size_t i = 0; i < keys.size();) {
            const unsigned col = corpus_key_col(keys[i]);
            double s = corpus_val(m.values, m.values_dtype, lo + corpus_key_pos(keys[i]));
            size_t e = i + 1;
            for (; e < keys.size() && corpus_key_col(keys[e]) == col; ++e) s += corpus_val(m.values, m.values_dtype, lo + corpus_key_pos(keys[e]));
            c.duplicates += (int64_t)(e - i) - 1;
            if (s == 0.0) c.zeros += 1;
            else {
                c.indices.push_back((int32_t)col);
                c.values.push_back(s);
                c.negatives += s < 0.0;
            }
            i = e;
        }
        c.indptr.push_back((int64_t)c.indices.size());
    }
    return c;
}

}  // namespace rri
