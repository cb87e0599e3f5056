// rri_corpus_rank.hpp -- top-N lists, ranks and ranking metrics against resident corpora, written once (DESIGN "Rank and recommend
// against resident corpora").
//
// Order, eligibility, rank, value and clip are rri_topn.hpp's and rri_rank.hpp's; nothing there changes.  What is new is where the
// lists lie and what leaves the device.
//
// EXCLUSION.  A canonical corpus of the handle's shape (n, d): per row strictly ascending columns inside [0, d), checked once at
// ingest, so nothing of it is checked, copied or cut again.  Request q, scoring row i = rows[q] of W (rows NULL: i = q), excludes
// the stored columns of row i of that corpus: the exclusion is indexed by the row of W, not by the request, and serves any list of
// rows, in any order, with repeats.
// TARGETS.  A canonical corpus with d columns.  Request q is row q of it, scored against row rows[q] of W (rows NULL: row q, and
// then the corpus has at most n rows); every stored entry is a target.  Outputs per entry are in corpus order.  A row without
// stored entries is not scored: it gets no piece and its eligible count stays -1.  The pieces (crank_cut_plain) are
// rank_cut_pieces' restricted to the rows that have entries.
// METRICS.  With N = n_items, over the targets whose stored value is >= relevant_from (NaN: every entry) -- the RELEVANT ones --
// a row u has T_u relevant targets, of which P_u are eligible (rank >= 0), h_u = #{rank < N} hits, the smallest rank r0, the sum
// of ranks S_u and the eligible count L_u.  The rank of an entry does not depend on which entries are relevant (other targets
// compete like any column), so relevant_from only selects what is read.  A row with P_u >= 1 is a USER and leaves the terms
//   [h > 0],  h / N,  h / P,  dcg / ideal[min(N, P)],  1 / (1 + r0),  L > P: 1 - (S - P (P - 1) / 2) / (P (L - P)),  [L > P],
//   L > 1: S / (L - 1),  L > 1: P
// where dcg = sum over hits of table[rank], table[p] = 1 / log2(p + 2) and ideal[m] = table[0] + ... + table[m - 1] in ascending
// order.  The table is made once per call on the host (crank_table) for p < min(N, d): the device takes no logarithm, so the plain
// loop and the kernel read the same bits.  sum_a (r_a - a) over a row's ascending ranks is S - P (P - 1) / 2 in int64: no sort.
// Every integer is reduced exactly.  dcg is the one floating sum of a row, and its order is the LANE RULE: lane l of 64 adds
// table[rank] of the row's entries l, l + 64, ... that are hits, in ascending order, from 0.0, and the 64 lane sums are combined
// by crank_tree64.  Divisions are IEEE float64 divisions of exactly converted integers (or of dcg by a table entry); no expression
// here has a multiply that feeds an add or a subtract -- P (L - P) and P (P - 1) / 2 are int64 --, so contraction to fused
// multiply-adds cannot change a bit between the host loop and the kernel.
// TOTALS.  out[16] = {users, targets, targets_not_eligible, sum [h > 0], sum h / N, sum h / P, sum dcg / ideal, sum 1 / (1 + r0),
// sum auc term, users with L > P, sum S / (L - 1), targets with L > 1, 0, 0, 0, 0}: the CRANK_TERMS = 12 row terms added over the
// rows in ascending order by a fixed tree (crank_sum_plain): blocks of CRANK_SUM_ROWS rows, in a block slot t of 256 adds the rows
// t, t + 256, ... ascending and the 256 slots are combined by crank_tree256; the block sums are added the same way (slot t the
// blocks t, t + 256, ...) by one workgroup.  Counts are exact as doubles.  The caller divides.
//
// The kernels (rri_corpus_rank_kernels.hpp), the entry points (rri_corpus_topn_rows, rri_corpus_rank_entries,
// rri_corpus_ranking_metrics) and the stand-alone CPU test (tests/c/corpus_rank_main.cpp) take the classification, the term
// formulas, the trees, the request check and the plain loops from here.  Plain inline functions, host and device; nothing in this
// file needs HIP.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rri_rank.hpp"

namespace rri {

constexpr int CRANK_TERMS = 12;          // terms a row leaves, and sums of a call
constexpr int CRANK_OUT = 16;            // doubles of the metrics call's output
constexpr int CRANK_SUM_ROWS = 1024;     // rows (or block sums) per workgroup of the totals
enum { CRANK_USER = 0, CRANK_TARGETS, CRANK_NOT_ELIGIBLE, CRANK_HIT, CRANK_PRECISION, CRANK_RECALL, CRANK_NDCG, CRANK_MRR, CRANK_AUC,
       CRANK_ROOM, CRANK_MPR, CRANK_WIDE };

// ---- an entry ----------------------------------------------------------------------------------------------------------------
RRI_TOPN_FN bool crank_relevant(double v, double relevant_from) { return !(relevant_from == relevant_from) || v >= relevant_from; }
RRI_TOPN_FN bool crank_eligible(int rank) { return rank >= 0; }
RRI_TOPN_FN bool crank_hit(int rank, int64_t n_items) { return rank >= 0 && (int64_t)rank < n_items; }

// ---- a row -------------------------------------------------------------------------------------------------------------------
// what a row's entries reduce to: all exact
struct CrankRow {
    int64_t T;        // relevant targets
    int64_t P;        // ... that are eligible
    int64_t hits;     // ... with rank < N
    int64_t rmin;     // the smallest rank among the P (any value when P = 0)
    int64_t S;        // the sum of the P ranks
    int64_t L;        // the row's eligible count (-1: not scored)
};
// the CRANK_TERMS terms of a row; ideal has min(N, d) + 1 entries and P <= d
RRI_TOPN_FN void crank_row_terms(const CrankRow& w, double dcg, int64_t n_items, const double* ideal, double* t) {
    for (int i = 0; i < CRANK_TERMS; ++i) t[i] = 0.0;
    t[CRANK_TARGETS] = (double)w.T;
    t[CRANK_NOT_ELIGIBLE] = (double)(w.T - w.P);
    if (w.P < 1) return;
    const double P = (double)w.P, h = (double)w.hits;
    t[CRANK_USER] = 1.0;
    t[CRANK_HIT] = w.hits > 0 ? 1.0 : 0.0;
    t[CRANK_PRECISION] = h / (double)n_items;
    t[CRANK_RECALL] = h / P;
    t[CRANK_NDCG] = dcg / ideal[n_items < w.P ? n_items : w.P];
    t[CRANK_MRR] = 1.0 / (double)(1 + w.rmin);
    if (w.L > w.P) {
        const int64_t above = w.S - w.P * (w.P - 1) / 2, pairs = w.P * (w.L - w.P);
        const double frac = (double)above / (double)pairs;
        t[CRANK_AUC] = 1.0 - frac;
        t[CRANK_ROOM] = 1.0;
    }
    if (w.L > 1) {
        t[CRANK_MPR] = (double)w.S / (double)(w.L - 1);
        t[CRANK_WIDE] = P;
    }
}

// ---- the fixed trees ---------------------------------------------------------------------------------------------------------
// 64 sums into s[0]: s[l] += s[l + off] for off = 32, 16, .. 1 -- what lane 0 of a wave holds after the xor butterfly at those
// distances, in which every lane adds its partner's value to its own
inline double crank_tree64(double* s) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) s[l] = s[l] + s[l + off];
    return s[0];
}
// 256 sums: the four waves' trees, then (w0 + w1) + (w2 + w3)
inline double crank_tree256(double* s) {
    const double w0 = crank_tree64(s), w1 = crank_tree64(s + 64), w2 = crank_tree64(s + 128), w3 = crank_tree64(s + 192);
    return (w0 + w1) + (w2 + w3);
}

// ---- the table ---------------------------------------------------------------------------------------------------------------
// table[p] = 1 / log2(p + 2) for p < m = min(n_items, d) and ideal[0 .. m], its running sum from 0.0
inline int64_t crank_table_len(int64_t n_items, int64_t d) { return n_items < d ? n_items : d; }
inline void crank_table(int64_t m, std::vector<double>* table, std::vector<double>* ideal) {
    table->assign((size_t)m, 0.0);
    ideal->assign((size_t)m + 1, 0.0);
    for (int64_t p = 0; p < m; ++p) {
        (*table)[(size_t)p] = 1.0 / std::log2((double)p + 2.0);
        (*ideal)[(size_t)p + 1] = (*ideal)[(size_t)p] + (*table)[(size_t)p];
    }
}

// ---- a request, checked on the host before any device call ----------------------------------------------------------------------
// what the check sees of a corpus argument
struct CrankCorpus {
    bool given;       // the pointer is not NULL
    bool alive;       // ... and names a corpus that has not been destroyed
    int64_t rows, cols;
    int device;
};
enum { CRANK_CALL_TOPN = 0, CRANK_CALL_RANK = 1, CRANK_CALL_METRICS = 2 };
// n, d, device: the handle's.  `targets` is read by the rank and metrics calls (their requests are its rows), `count` and `topn` by
// the top-N call, `n_items` by the metrics call, the clip by the other two.  Returns TOPN_REQ_OK, TOPN_REQ_INVALID or
// TOPN_REQ_UNSUPPORTED and writes the first broken rule to msg.
inline int crank_check_request(int call, int64_t n, int64_t d, int device, const CrankCorpus& targets, const CrankCorpus& exclude,
                               const int64_t* rows, int64_t count, int32_t topn, int32_t max_topn, int64_t n_items, double lo, double hi,
                               char* msg, size_t msg_len) {
    auto say = [&](int code, const char* what, long long a, long long b, long long c2 = 0, long long d2 = 0) {
        if (msg && msg_len) snprintf(msg, msg_len, what, a, b, c2, d2);
        return code;
    };
    const bool topn_call = call == CRANK_CALL_TOPN;
    if (!topn_call) {
        if (!targets.given || !targets.alive) return say(TOPN_REQ_INVALID, "the targets corpus is NULL or has been destroyed", 0, 0);
        if (targets.device != device) return say(TOPN_REQ_INVALID, "the targets corpus lives on device %lld, the handle on device %lld", targets.device, device);
    }
    if (exclude.given) {
        if (!exclude.alive) return say(TOPN_REQ_INVALID, "the exclusion corpus has been destroyed", 0, 0);
        if (exclude.device != device) return say(TOPN_REQ_INVALID, "the exclusion corpus lives on device %lld, the handle on device %lld", exclude.device, device);
        if (exclude.rows != n || exclude.cols != d)
            return say(TOPN_REQ_INVALID, "the exclusion corpus is %lld x %lld, the handle %lld x %lld", (long long)exclude.rows, (long long)exclude.cols, (long long)n, (long long)d);
    }
    if (topn_call) {
        if (count < 0) return say(TOPN_REQ_INVALID, "count %lld is negative", (long long)count, 0);
        if (topn < 1 || topn > max_topn) return say(TOPN_REQ_UNSUPPORTED, "topn %lld outside 1 .. %lld", (long long)topn, (long long)max_topn);
        if (!rows && count > n) return say(TOPN_REQ_INVALID, "rows is NULL and count %lld exceeds the %lld rows of W", (long long)count, (long long)n);
    } else {
        if (targets.cols != d) return say(TOPN_REQ_INVALID, "the corpus has %lld columns, W T has %lld", (long long)targets.cols, (long long)d);
        if (!rows && targets.rows > n) return say(TOPN_REQ_INVALID, "rows is NULL and the corpus has %lld rows, W has %lld", (long long)targets.rows, (long long)n);
        count = targets.rows;
    }
    if (call == CRANK_CALL_METRICS) {
        if (n_items < 1) return say(TOPN_REQ_INVALID, "n_items %lld is not a positive integer", (long long)n_items, 0);
    } else {
        if (std::isnan(lo) || std::isnan(hi)) return say(TOPN_REQ_INVALID, "a clip bound is NaN (an open side is -inf or +inf)", 0, 0);
        if (lo > hi) {
            if (msg && msg_len) snprintf(msg, msg_len, "clip_lo %g is above clip_hi %g", lo, hi);
            return TOPN_REQ_INVALID;
        }
    }
    for (int64_t q = 0; rows && q < count; ++q)
        if (rows[q] < 0 || rows[q] >= n) return say(TOPN_REQ_INVALID, "rows[%lld] = %lld is out of range", (long long)q, (long long)rows[q]);
    return TOPN_REQ_OK;
}

// ---- the plain loops -----------------------------------------------------------------------------------------------------------
// pieces per corpus row, and the pieces: rank_cut_pieces restricted to the rows that have entries.  first (NULL, or n_rows + 1
// entries) takes the exclusive scan of the counts.  Returns the number of pieces.
RRI_TOPN_FN int64_t crank_row_pieces(int64_t len) { return (len + RANK_SEG - 1) / RANK_SEG; }
RRI_TOPN_FN RankPiece crank_piece(const int64_t* indptr, int64_t row, int64_t p) {
    const int64_t t0 = indptr[row] + (int64_t)RANK_SEG * p, left = indptr[row + 1] - t0;
    return RankPiece{row, t0, (int32_t)(left < RANK_SEG ? left : RANK_SEG), p == 0 ? 1 : 0};
}
inline int64_t crank_cut_plain(const int64_t* indptr, int64_t n_rows, int64_t* first, RankPiece* out) {
    int64_t np = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (first) first[r] = np;
        const int64_t c = crank_row_pieces(indptr[r + 1] - indptr[r]);
        for (int64_t p = 0; p < c; ++p, ++np)
            if (out) out[np] = crank_piece(indptr, r, p);
    }
    if (first) first[n_rows] = np;
    return np;
}

// the terms of every row (terms: n_rows x CRANK_TERMS) from the ranks per entry and the eligible counts per row
inline void crank_rows_plain(const int64_t* indptr, const double* values, int64_t n_rows, const int32_t* rank, const int32_t* eligible,
                             int64_t n_items, double relevant_from, const double* table, const double* ideal, double* terms) {
    for (int64_t r = 0; r < n_rows; ++r) {
        CrankRow w{0, 0, 0, INT64_MAX, 0, eligible[r]};
        double lane_sum[64];
        for (int l = 0; l < 64; ++l) lane_sum[l] = 0.0;
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if (!crank_relevant(values[e], relevant_from)) continue;
            ++w.T;
            if (!crank_eligible(rank[e])) continue;
            ++w.P;
            w.S += rank[e];
            if (rank[e] < w.rmin) w.rmin = rank[e];
            if (crank_hit(rank[e], n_items)) {
                ++w.hits;
                double& s = lane_sum[(e - indptr[r]) & 63];
                s = s + table[rank[e]];
            }
        }
        if (w.P < 1) w.rmin = 0;
        crank_row_terms(w, crank_tree64(lane_sum), n_items, ideal, terms + r * CRANK_TERMS);
    }
}

// one level of the totals: out[b * CRANK_TERMS + i] = the sum of term i over the items [b R, (b + 1) R), R = CRANK_SUM_ROWS
inline void crank_sum_level(const double* in, int64_t items, double* out) {
    const int64_t nb = (items + CRANK_SUM_ROWS - 1) / CRANK_SUM_ROWS;
    for (int64_t b = 0; b < nb; ++b)
        for (int i = 0; i < CRANK_TERMS; ++i) {
            double s[256];
            for (int t = 0; t < 256; ++t) {
                s[t] = 0.0;
                for (int64_t r = b * CRANK_SUM_ROWS + t; r < items && r < (b + 1) * CRANK_SUM_ROWS; r += 256) s[t] = s[t] + in[r * CRANK_TERMS + i];
            }
            out[b * CRANK_TERMS + i] = crank_tree256(s);
        }
}
// the CRANK_OUT totals of n_rows rows of terms: block sums, then the sum of the blocks with slot t taking the blocks t, t + 256, ...
inline void crank_sum_plain(const double* terms, int64_t n_rows, double* out) {
    for (int i = 0; i < CRANK_OUT; ++i) out[i] = 0.0;
    if (n_rows < 1) return;
    const int64_t nb = (n_rows + CRANK_SUM_ROWS - 1) / CRANK_SUM_ROWS;
    std::vector<double> part((size_t)nb * CRANK_TERMS);
    crank_sum_level(terms, n_rows, part.data());
    for (int i = 0; i < CRANK_TERMS; ++i) {
        double s[256];
        for (int t = 0; t < 256; ++t) {
            s[t] = 0.0;
            for (int64_t b = t; b < nb; b += 256) s[t] = s[t] + part[(size_t)b * CRANK_TERMS + i];
        }
        out[i] = crank_tree256(s);
    }
}

}  // namespace rri
