// Stand-alone check of rri_nmf_amd/csrc/rri_corpus_build.hpp (own main, host compiler, sanitizers): the constants, the verdict and
// text of every refusal of a list of pairs, and the two plain loops -- a corpus from pairs and the split by entry -- on seeded
// lists and matrices, whose inputs and results are printed for tests/test_corpus_build_cpu.py to hold against the numpy
// restatement (tests/corpus_build_cases.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_corpus_build.hpp"

using namespace rri;

static unsigned long long g_state = 0x2545f4914f6cdd1dull;
static unsigned rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33);
}

template <typename V>
static void row(const char* kind, int id, const std::vector<V>& v) {
    printf("%s %d :", kind, id);
    for (const V& x : v) printf(" %.17g", (double)x);
    printf("\n");
}
static void csr(const char* name, int id, const DeriveCsr& a) {
    char kind[40];
    printf("%sshape %d : %lld %lld\n", name, id, (long long)a.n_rows, (long long)a.n_cols);
    snprintf(kind, sizeof kind, "%sptr", name); row(kind, id, a.indptr);
    snprintf(kind, sizeof kind, "%sidx", name); row(kind, id, a.indices);
    snprintf(kind, sizeof kind, "%sval", name); row(kind, id, a.values);
}

struct List {
    int64_t n_rows, n_cols;
    std::vector<int64_t> rows, cols;
    std::vector<double> vals;
    bool pattern;
};

static int g_lists = 0, g_splits = 0;
// the list in one of its representations: int32 or int64 indices, two arrays or one interleaved, float32 / float64 / no values
static CorpusCanonical list_case(const List& l, int idt, int stride, int vdt) {
    const size_t m = l.rows.size();
    std::vector<int32_t> a32, b32;
    std::vector<int64_t> a64, b64;
    std::vector<float> v32;
    std::vector<double> v64;
    const void *rp, *cp;
    if (stride == 2) {              // interleaved: cols == rows + 1
        for (size_t p = 0; p < m; ++p) {
            a32.push_back((int32_t)l.rows[p]); a32.push_back((int32_t)l.cols[p]);
            a64.push_back(l.rows[p]); a64.push_back(l.cols[p]);
        }
        a32.push_back(0); a64.push_back(0);       // (so that data() + 1 is inside the array for an empty list too)
        rp = idt == RRI_I32 ? (const void*)a32.data() : (const void*)a64.data();
        cp = idt == RRI_I32 ? (const void*)(a32.data() + 1) : (const void*)(a64.data() + 1);
    } else {
        for (size_t p = 0; p < m; ++p) {
            a32.push_back((int32_t)l.rows[p]); b32.push_back((int32_t)l.cols[p]);
            a64.push_back(l.rows[p]); b64.push_back(l.cols[p]);
        }
        a32.push_back(0); b32.push_back(0); a64.push_back(0); b64.push_back(0);
        rp = idt == RRI_I32 ? (const void*)a32.data() : (const void*)a64.data();
        cp = idt == RRI_I32 ? (const void*)b32.data() : (const void*)b64.data();
    }
    for (double v : l.vals) {
        v32.push_back((float)v);
        v64.push_back(v);
    }
    v32.push_back(0.0f); v64.push_back(0.0);
    const void* vp = l.pattern ? nullptr : vdt == RRI_F32 ? (const void*)v32.data() : (const void*)v64.data();
    const CorpusPairs req{l.n_rows, l.n_cols, (int64_t)m, rp, cp, idt, stride, vp, vdt};
    char msg[200] = "";
    if (pairs_check(req, msg, sizeof msg) != TOPN_REQ_OK) {
        printf("list case %d refused: %s\n", g_lists, msg);
        exit(1);
    }
    const CorpusCanonical c = corpus_from_pairs_plain(req);
    const int id = g_lists++;
    printf("pairs %d : %lld %lld %lld %d %d %d\n", id, (long long)l.n_rows, (long long)l.n_cols, (long long)m, stride, idt, l.pattern ? -1 : vdt);
    row("prow", id, l.rows);
    row("pcol", id, l.cols);
    if (l.pattern) row("pval", id, std::vector<double>());
    else if (vdt == RRI_F32) row("pval", id, std::vector<float>(v32.begin(), v32.end() - 1));
    else row("pval", id, l.vals);
    row("cptr", id, c.indptr);
    row("cidx", id, c.indices);
    row("cval", id, c.values);
    printf("cstat %d : %lld %lld %lld %lld %lld\n", id, (long long)c.rows_rewritten, (long long)c.duplicates, (long long)c.zeros,
           (long long)c.negatives, (long long)c.long_rows);
    return c;
}

// m pairs over n_rows x n_cols in random order; a share of the values is an explicit 0, the others are reals of either sign
static List seeded_list(int64_t n_rows, int64_t n_cols, int m, unsigned zero_share, bool pattern) {
    List l{n_rows, n_cols, {}, {}, {}, pattern};
    for (int p = 0; p < m; ++p) {
        l.rows.push_back((int64_t)(rnd() % (unsigned)n_rows));
        l.cols.push_back((int64_t)(rnd() % (unsigned)n_cols));
        l.vals.push_back(rnd() % 16 < zero_share ? 0.0 : ((int)(rnd() % 4001) - 1500) / 8.0);
    }
    return l;
}

static DeriveCsr seeded_csr(int64_t n_rows, int64_t n_cols, unsigned share, bool counts, int64_t empty) {
    DeriveCsr a;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.indptr.assign(1, 0);
    for (int64_t r = 0; r < n_rows; ++r) {
        for (int64_t j = 0; r != empty && j < n_cols; ++j) {
            if (rnd() % 16 >= share) continue;
            double v = counts ? 1.0 : ((int)(rnd() % 2000001) - 1000000) / 1024.0 / 7.0;
            if (v == 0.0) v = 1.5;
            a.indices.push_back((int32_t)j);
            a.values.push_back(v);
        }
        a.indptr.push_back((int64_t)a.indices.size());
    }
    return a;
}
static void split_case(const DeriveCsr& a, double held_out, uint64_t seed) {
    uint32_t thr = 0;
    if (!split_threshold(held_out, &thr)) exit(1);
    DeriveCsr obs, held;
    split_entries_plain(a, thr, seed, &obs, &held);
    const int id = g_splits++;
    printf("split %d : %u %llu\n", id, thr, (unsigned long long)seed);
    csr("from", id, a);
    csr("obs", id, obs);
    csr("held", id, held);
    // an entry whose count is 1 goes the same way in the binomial split of rri_derive.hpp
    int same = 1;
    for (int64_t r = 0; r < a.n_rows; ++r)
        for (int64_t p = a.indptr[(size_t)r]; p < a.indptr[(size_t)r + 1]; ++p)
            same = same && (split_held(r, a.indices[(size_t)p], 1, thr, seed) == 1) == split_entry_held(r, a.indices[(size_t)p], thr, seed);
    printf("asone %d : %d\n", id, same);
}

static void req(const char* name, int64_t n_rows, int64_t n_cols, const std::vector<int64_t>& rows, const std::vector<int64_t>& cols,
                const std::vector<double>& vals, int idt = RRI_I64, int64_t stride = 1, int vdt = RRI_F64, int64_t n_pairs = -7,
                bool null_rows = false, bool null_cols = false) {
    char msg[200] = "";
    const int64_t dummy = 0;
    const CorpusPairs q{n_rows, n_cols, n_pairs == -7 ? (int64_t)rows.size() : n_pairs, null_rows ? nullptr : rows.empty() ? (const void*)&dummy : (const void*)rows.data(),
                        null_cols ? nullptr : cols.empty() ? (const void*)&dummy : (const void*)cols.data(), idt, stride, vals.empty() ? nullptr : (const void*)vals.data(), vdt};
    const int code = pairs_check(q, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

int main() {
    printf("consts : %d %d %d %lld %lld %d\n", CB_WAVE_PAIRS, CB_BLOCK_PAIRS, CB_GRID_MAX, (long long)CB_SWEEP_PAIRS, (long long)CB_PAIRS_MAX, (int)CB_RULES);
    printf("grid : %u %u %u %u %u\n", pairs_grid(0), pairs_grid(1), pairs_grid(CB_BLOCK_PAIRS + 1), pairs_grid(CB_SWEEP_PAIRS), pairs_grid(CB_SWEEP_PAIRS + 1));
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const std::vector<int64_t> R{0, 2, 1, 2}, Cc{5, 0, 3, 0};
    const std::vector<double> V{1.0, 2.0, -1.5, 0.0};
    // the arguments, before any array is read: every refusal at two places, and the first broken one wins
    req("fine", 3, 6, R, Cc, V);
    req("fine_without_values", 3, 6, R, Cc, {});
    req("empty", 0, 0, {}, {}, {});
    req("empty_null_arrays", 5, 5, {}, {}, {}, RRI_I32, 1, RRI_F64, 0, true, true);
    req("negative_rows", -1, 6, R, Cc, V);
    req("negative_rows_first", -4, -6, R, Cc, V);
    req("negative_cols", 3, -2, R, Cc, V);
    req("negative_cols_first", 3, -9, R, Cc, V, RRI_I64, 1, RRI_F64, -1);
    req("negative_pairs", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, -1);
    req("negative_pairs_first", 3, 6, R, Cc, V, 77, 1, RRI_F64, -3);
    req("index_dtype_unknown", 3, 6, R, Cc, V, RRI_F64);
    req("index_dtype_unknown_first", 3, 6, R, Cc, V, 77, 1, 78);
    req("values_dtype_unknown", 3, 6, R, Cc, V, RRI_I64, 1, RRI_I32);
    req("values_dtype_unknown_first", 3, 6, R, Cc, V, RRI_I64, 0, 55);
    req("values_dtype_unread_without_values", 3, 6, R, Cc, {}, RRI_I64, 1, 55);
    req("stride_zero", 3, 6, R, Cc, V, RRI_I64, 0);
    req("stride_negative_first", 3, 6, R, Cc, V, RRI_I64, -2, RRI_F64, -7, true);
    req("rows_null", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, -7, true);
    req("rows_null_first", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, 2, true, true);
    req("cols_null", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, -7, false, true);
    req("cols_null_first", 3, 1ll << 31, R, Cc, V, RRI_I64, 1, RRI_F64, 9, false, true);
    req("n_cols_2_31", 3, 1ll << 31, R, Cc, V);
    req("n_cols_above_2_31_first", 3, (1ll << 31) + 5, R, Cc, V, RRI_I64, 1, RRI_F64, 1ll << 31);
    req("n_pairs_2_31", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, 1ll << 31);
    req("n_pairs_above_2_31", 3, 6, R, Cc, V, RRI_I64, 1, RRI_F64, (1ll << 31) + 7);
    // the three rules, each over all positions before the next
    req("row_3_at_1", 3, 6, {0, 3, 1, 2}, Cc, V);
    req("row_negative_at_2", 3, 6, {0, 2, -1, 5}, Cc, V);
    req("column_6_at_0", 3, 6, R, {6, 0, 3, -1}, V);
    req("column_negative_at_3", 3, 6, R, {5, 0, 3, -1}, V);
    req("rows_before_columns", 3, 6, {0, 2, 1, 7}, {9, 0, 3, 0}, V);
    req("value_nan_at_2", 3, 6, R, Cc, {1.0, 2.0, nan, inf});
    req("value_minus_inf_at_3", 3, 6, R, Cc, {1.0, 2.0, 3.0, -inf});
    req("columns_before_values", 3, 6, R, {5, 0, 3, 8}, {nan, 2.0, 3.0, 1.0});
    req("rows_before_values", 3, 6, {0, 2, 1, 3}, Cc, {inf, 2.0, 3.0, 1.0});
    req("no_rows_at_all", 0, 6, {0}, {1}, {1.0});
    {   // a strided read: the offender is named by its pair position, not by its element
        const std::vector<int64_t> il{0, 5, 2, 0, 1, 9, 2, 0};
        char msg[200] = "";
        const CorpusPairs q{3, 6, 4, il.data(), il.data() + 1, RRI_I64, 2, nullptr, RRI_F64};
        const int code = pairs_check(q, msg, sizeof msg);
        printf("req interleaved_column_9_at_2 : %d : %s\n", code, msg);
    }

    // a corpus from pairs: one seeded list in every representation, then lists of each kind
    const List mixed = seeded_list(7, 12, 90, 2, false);
    const CorpusCanonical first = list_case(mixed, RRI_I64, 1, RRI_F64);
    for (int idt : {RRI_I32, RRI_I64})
        for (int stride : {1, 2}) {
            const CorpusCanonical again = list_case(mixed, idt, stride, RRI_F64);
            if (again.indptr != first.indptr || again.indices != first.indices || again.values != first.values) return printf("representations differ\n"), 1;
        }
    list_case(mixed, RRI_I32, 2, RRI_F32);
    list_case(seeded_list(5, 9, 60, 0, true), RRI_I32, 1, RRI_F64);              // tokens: every pair counts 1
    list_case(seeded_list(4, 300, 40, 0, false), RRI_I64, 2, RRI_F64);           // hardly a duplicate
    {   // grouped by row, the columns ascending: no row is rewritten
        List l{6, 40, {}, {}, {}, false};
        for (int64_t r : {0, 0, 0, 2, 2, 3, 5, 5, 5, 5}) l.rows.push_back(r);
        for (int64_t j : {1, 7, 39, 0, 3, 8, 2, 4, 6, 30}) l.cols.push_back(j);
        for (int p = 0; p < 10; ++p) l.vals.push_back(p % 3 ? 1.25 * p : -2.0 - p);
        list_case(l, RRI_I64, 1, RRI_F64);
        // the same pairs, the rows interleaved but every row's columns still ascending as given: still none
        List k{6, 40, {}, {}, {}, false};
        for (int p : {6, 0, 3, 7, 5, 1, 8, 4, 2, 9}) {
            k.rows.push_back(l.rows[(size_t)p]); k.cols.push_back(l.cols[(size_t)p]); k.vals.push_back(l.vals[(size_t)p]);
        }
        list_case(k, RRI_I64, 1, RRI_F64);
        // one stored zero: its row is rewritten
        l.vals[4] = 0.0;
        list_case(l, RRI_I64, 1, RRI_F64);
    }
    {   // the order of summation: one (i, j) many times between other rows' pairs, and the same set permuted
        const double seq[8] = {1e16, 1.0, -1e16, 1.0, 1e16, 1.0, -1e16, 1.0};
        for (int perm = 0; perm < 2; ++perm) {
            List l{3, 5, {}, {}, {}, false};
            for (int p = 0; p < 8; ++p) {
                l.rows.push_back(1); l.cols.push_back(2); l.vals.push_back(seq[perm ? (p * 3) % 8 : p]);
                l.rows.push_back(p % 2 ? 0 : 2); l.cols.push_back(p % 5); l.vals.push_back(0.5 * (p + 1));
            }
            l.rows.push_back(0); l.cols.push_back(4); l.vals.push_back(3.0);         // a group that sums to exactly 0
            l.rows.push_back(0); l.cols.push_back(4); l.vals.push_back(-3.0);
            list_case(l, RRI_I64, 1, RRI_F64);
        }
    }
    list_case(List{0, 0, {}, {}, {}, false}, RRI_I64, 1, RRI_F64);
    list_case(List{3, 4, {}, {}, {}, true}, RRI_I32, 2, RRI_F64);
    {   // all pairs in one row, the last row and the last column used
        List l = seeded_list(1, 50, 70, 1, false);
        for (auto& r : l.rows) r = 3;
        l.n_rows = 4;
        l.cols[0] = 49;
        list_case(l, RRI_I32, 1, RRI_F32);
    }

    // the split by entry: reals of either sign with an empty row under two seeds and two thresholds, the extreme thresholds, a
    // pattern of ones, and about 12000 entries for the sanity bound
    const DeriveCsr small = seeded_csr(6, 20, 7, false, 2);
    split_case(small, 0.5, 12345ull);
    split_case(small, 0.5, 12346ull);
    split_case(small, 0.3, (5ull << 32) | 12345ull);
    split_case(small, std::ldexp(1.0, -32), 3ull);
    split_case(small, std::nextafter(1.0, 0.0), 3ull);
    split_case(seeded_csr(9, 30, 8, true, -1), 0.5, 77ull);
    const DeriveCsr large = seeded_csr(150, 160, 8, false, 10);
    split_case(large, 0.05, 12345ull);
    split_case(large, 0.3, 12345ull);
    split_case(seeded_csr(0, 5, 8, false, -1), 0.5, 1ull);
    printf("ok %d %d cases\n", g_lists, g_splits);
    return 0;
}
