// rri_derive.hpp -- corpora derived from a resident canonical corpus: a row and column selection, the document frequencies and a
// binomial split of the counts, written once (DESIGN "Corpora derived on the device").
//
// SELECT (src, rows, keep) -> out.  rows: NULL (with a count of 0: all rows, in order) or m >= 0 row numbers in [0, n_rows), in
// any order, repeats allowed.  keep: NULL (with a count of 0: all columns) or d' >= 0 source columns, strictly ascending, each in
// [0, n_cols).  out is m x d': its row q holds the entries of source row rows[q] whose column is in keep, the column renumbered to
// its place in keep, the value copied bit for bit.  keep ascends, so out is canonical without a sort.
// COLUMN COUNTS: df[j] = the rows with a canonical entry in column j (int64).
// SPLIT (src, thr, seed) -> (observed, held): a binomial thinning by a counter-based generator whose integer arithmetic is the
// same on the host and on the device.  Philox4x32-10, key (seed low word, seed high word), counter (column, row low word, row high
// word, block b); token t of an entry (0 <= t < count) uses word t % 4 of block t / 4 and goes to `held` when that word is below
// thr = floor(held_out 2^32).  held and observed have the source's shape, hold the entries whose part is above 0 and are
// canonical; observed + held == src exactly.  The values must be counts; the check tests, in this order,
//   0  a negative value (INVALID)         1  a value that is not whole (INVALID)         2  a value above SPLIT_COUNT_MAX (UNSUPPORTED)
// and names the smallest offending canonical position of the first broken rule.
//
// On the device all three walk the source in PIECES: up to DERIVE_PIECE consecutive entries of one row, a wave each, so that one
// long row is many waves' work (derive_cut_pieces; the host cuts them from its copy of indptr).  An entry whose count is above
// SPLIT_LANE_MAX has its Philox blocks shared by the 64 lanes of its wave (split_held_blocks with a stride of 64) and summed as
// integers.  The kernels (rri_derive_kernels.hpp), the entry points (rri_corpus_select, rri_corpus_column_counts,
// rri_corpus_split), the stand-alone CPU test (tests/c/derive_main.cpp) and tests/derive_cases.py, which mirrors the constants,
// take the rules and the texts from here.  Plain inline functions, host and device; nothing in this file needs HIP.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_hip.h"
#include "rri_topn.hpp"

namespace rri {

constexpr int DERIVE_PIECE = 1024;                 // the most source entries of one piece: 16 strides of a wave
constexpr int SPLIT_LANE_MAX = 256;                // the largest count one lane thins alone: 64 Philox blocks
constexpr int64_t SPLIT_COUNT_MAX = 1ll << 20;     // the largest count that is split at all: 4096 blocks per lane of a wave
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
enum { SPLIT_RULES = 3 };

// ---- the generator -----------------------------------------------------------------------------------------------------------
struct Philox4 {
    uint32_t w[4];
};
RRI_TOPN_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}
// block b of the entry (row, col) under the seed
RRI_TOPN_FN Philox4 split_block(int64_t row, int32_t col, uint64_t seed, uint32_t b) {
    return philox4x32_10((uint32_t)col, (uint32_t)((uint64_t)row & 0xffffffffull), (uint32_t)((uint64_t)row >> 32), b,
                         (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
}
// the held tokens among those of blocks b0, b0 + step, ... of an entry of `count` tokens
RRI_TOPN_FN int64_t split_held_blocks(int64_t row, int32_t col, int64_t count, uint32_t thr, uint64_t seed, int64_t b0, int64_t step) {
    int64_t held = 0;
    for (int64_t b = b0; 4 * b < count; b += step) {
        const Philox4 r = split_block(row, col, seed, (uint32_t)b);
        const int64_t left = count - 4 * b;
        held += (int)(r.w[0] < thr) + (int)(left > 1 && r.w[1] < thr) + (int)(left > 2 && r.w[2] < thr) + (int)(left > 3 && r.w[3] < thr);
    }
    return held;
}
// the held part of an entry: token by token, on one thread
RRI_TOPN_FN int64_t split_held(int64_t row, int32_t col, int64_t count, uint32_t thr, uint64_t seed) {
    return split_held_blocks(row, col, count, thr, seed, 0, 1);
}
// thr = floor(held_out 2^32); false: held_out is outside (0, 1) or below 2^-32
inline bool split_threshold(double held_out, uint32_t* thr) {
    if (!(held_out > 0.0 && held_out < 1.0)) return false;
    const double scaled = std::floor(held_out * 4294967296.0);          // a power of two: exact
    if (scaled < 1.0) return false;
    *thr = (uint32_t)scaled;
    return true;
}

// ---- the value check of a split ------------------------------------------------------------------------------------------------
RRI_TOPN_FN int split_value_rule(double v) { return v < 0.0 ? 0 : v != floor(v) ? 1 : v > (double)SPLIT_COUNT_MAX ? 2 : -1; }
inline int split_rule_code(int rule) { return rule == 2 ? (int)TOPN_REQ_UNSUPPORTED : (int)TOPN_REQ_INVALID; }
inline void split_rule_text(int rule, int64_t pos, double v, char* msg, size_t msg_len) {
    if (!msg || !msg_len) return;
    switch (rule) {
        case 0: snprintf(msg, msg_len, "value %.17g at entry %lld is negative: a split takes counts", v, (long long)pos); break;
        case 1: snprintf(msg, msg_len, "value %.17g at entry %lld is not a whole number: a split takes counts", v, (long long)pos); break;
        default: snprintf(msg, msg_len, "value %.17g at entry %lld is above %lld, the largest count that is split", v, (long long)pos, (long long)SPLIT_COUNT_MAX); break;
    }
}
// each rule over all canonical positions before the next: TOPN_REQ_OK or the code and the text of the first broken rule
inline int split_check_values(const double* values, int64_t nnz, char* msg, size_t msg_len) {
    for (int rule = 0; rule < SPLIT_RULES; ++rule)
        for (int64_t p = 0; p < nnz; ++p) {
            const double v = values[p];
            const bool broken = rule == 0 ? v < 0.0 : rule == 1 ? v != std::floor(v) : v > (double)SPLIT_COUNT_MAX;
            if (broken) return split_rule_text(rule, p, v, msg, msg_len), split_rule_code(rule);
        }
    return TOPN_REQ_OK;
}

// ---- the requests, checked on the host before any device call -----------------------------------------------------------------
// what every call asks of its corpus: alive (neither NULL nor destroyed) and on the handle's device
inline int derive_check_corpus(bool alive, int corpus_device, int handle_device, char* msg, size_t msg_len) {
    if (!alive) {
        if (msg && msg_len) snprintf(msg, msg_len, "the corpus is NULL or has been destroyed");
        return TOPN_REQ_INVALID;
    }
    if (corpus_device != handle_device) {
        if (msg && msg_len) snprintf(msg, msg_len, "the corpus lives on device %d, the handle on device %d", corpus_device, handle_device);
        return TOPN_REQ_INVALID;
    }
    return TOPN_REQ_OK;
}
inline int derive_check_select(int64_t n_rows, int64_t n_cols, const int64_t* rows, int64_t m, const int32_t* keep, int64_t dk, char* msg,
                               size_t msg_len) {
    auto say = [&](const char* what, long long a, long long b) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b);
        return (int)TOPN_REQ_INVALID;
    };
    if (m < 0) return say("n_rows_out %lld is negative", (long long)m, 0);
    if (dk < 0) return say("n_cols_out %lld is negative", (long long)dk, 0);
    if (!rows && m != 0) return say("rows is NULL with a count of %lld (NULL takes all rows: the count is 0)", (long long)m, 0);
    if (!keep && dk != 0) return say("keep is NULL with a count of %lld (NULL keeps all columns: the count is 0)", (long long)dk, 0);
    for (int64_t q = 0; rows && q < m; ++q)
        if (rows[q] < 0 || rows[q] >= n_rows) return say("rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
    for (int64_t j = 0; keep && j < dk; ++j)
        if (keep[j] < 0 || keep[j] >= n_cols) return say("keep[%lld] = %lld is out of range", (long long)j, (long long)keep[j]);
    for (int64_t j = 1; keep && j < dk; ++j)
        if (keep[j] <= keep[j - 1]) return say("keep[%lld] = %lld does not ascend strictly", (long long)j, (long long)keep[j]);
    return TOPN_REQ_OK;
}
inline int derive_check_split(uint32_t thr, bool has_observed, bool has_held, char* msg, size_t msg_len) {
    if (!has_observed || !has_held) {
        if (msg && msg_len) snprintf(msg, msg_len, "the output pointer is NULL");
        return TOPN_REQ_INVALID;
    }
    if (thr == 0) {
        if (msg && msg_len) snprintf(msg, msg_len, "threshold 0 holds nothing out: held_out is at least 2^-32");
        return TOPN_REQ_INVALID;
    }
    return TOPN_REQ_OK;
}

// ---- the pieces -------------------------------------------------------------------------------------------------------------------
// Output row q = source row rows[q] (rows NULL: q) is cut into pieces of up to DERIVE_PIECE entries, in order; an empty row has none
struct DerivePieces {
    std::vector<int64_t> row, src;     // the output row of a piece, and where it starts in the source arrays
    std::vector<int32_t> len;          // 1 .. DERIVE_PIECE
};
inline DerivePieces derive_cut_pieces(const int64_t* indptr, int64_t n_rows, const int64_t* rows, int64_t m) {
    DerivePieces p;
    const int64_t count = rows ? m : n_rows;
    for (int64_t q = 0; q < count; ++q) {
        const int64_t r = rows ? rows[q] : q;
        for (int64_t lo = indptr[r], hi = indptr[r + 1]; lo < hi; lo += DERIVE_PIECE) {
            p.row.push_back(q);
            p.src.push_back(lo);
            p.len.push_back((int32_t)(hi - lo < DERIVE_PIECE ? hi - lo : DERIVE_PIECE));
        }
    }
    return p;
}

// ---- the definitions as host loops ------------------------------------------------------------------------------------------------
struct DeriveCsr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};
inline DeriveCsr derive_select_plain(const DeriveCsr& a, const int64_t* rows, int64_t m, const int32_t* keep, int64_t dk) {
    DeriveCsr o;
    o.n_rows = rows ? m : a.n_rows;
    o.n_cols = keep ? dk : a.n_cols;
    std::vector<int32_t> map((size_t)a.n_cols, keep ? -1 : 0);
    for (int64_t j = 0; j < a.n_cols; ++j)
        if (!keep) map[(size_t)j] = (int32_t)j;
    for (int64_t j = 0; keep && j < dk; ++j) map[(size_t)keep[j]] = (int32_t)j;
    o.indptr.assign(1, 0);
    for (int64_t q = 0; q < o.n_rows; ++q) {
        const int64_t r = rows ? rows[q] : q;
        for (int64_t p = a.indptr[(size_t)r]; p < a.indptr[(size_t)r + 1]; ++p) {
            const int32_t j = map[(size_t)a.indices[(size_t)p]];
            if (j < 0) continue;
            o.indices.push_back(j);
            o.values.push_back(a.values[(size_t)p]);
        }
        o.indptr.push_back((int64_t)o.indices.size());
    }
    return o;
}
inline std::vector<int64_t> derive_column_counts_plain(const DeriveCsr& a) {
    std::vector<int64_t> df((size_t)a.n_cols, 0);
    for (int32_t j : a.indices) df[(size_t)j] += 1;
    return df;
}
// a checked source (split_check_values): observed and held
inline void derive_split_plain(const DeriveCsr& a, uint32_t thr, uint64_t seed, DeriveCsr* observed, DeriveCsr* held) {
    for (DeriveCsr* o : {observed, held}) {
        o->n_rows = a.n_rows;
        o->n_cols = a.n_cols;
        o->indptr.assign(1, 0);
        o->indices.clear();
        o->values.clear();
    }
    for (int64_t r = 0; r < a.n_rows; ++r) {
        for (int64_t p = a.indptr[(size_t)r]; p < a.indptr[(size_t)r + 1]; ++p) {
            const int32_t j = a.indices[(size_t)p];
            const int64_t count = (int64_t)a.values[(size_t)p], h = split_held(r, j, count, thr, seed);
            if (h > 0) {
                held->indices.push_back(j);
                held->values.push_back((double)h);
            }
            if (count - h > 0) {
                observed->indices.push_back(j);
                observed->values.push_back((double)(count - h));
            }
        }
        held->indptr.push_back((int64_t)held->indices.size());
        observed->indptr.push_back((int64_t)observed->indices.size());
    }
}

}  // namespace rri
