// Stand-alone check of rri_nmf_amd/csrc/rri_corpus.hpp (own main, host compiler, sanitizers): the verdict and text of every
// refusal, each rule at two places and the order among the rules; the class and the pad of row lengths on both sides of every
// border; and the plain loop on seeded raw matrices of every dtype, whose arrays and results are printed for
// tests/test_corpus_cpu.py to hold against the numpy restatement.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_corpus.hpp"

using namespace rri;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33);
}

struct Raw {
    int64_t n_rows = 3, n_cols = 6;
    std::vector<int64_t> indptr{0, 2, 2, 5};
    std::vector<int64_t> indices{0, 3, 1, 2, 5};
    std::vector<double> values{1.0, 2.0, 3.0, 1.0, 4.0};
    bool pattern = false, null_indptr = false, null_indices = false;
    int pdt = RRI_I64, idt = RRI_I64, vdt = RRI_F64;
    bool own_nnz = false;
    int64_t nnz = 0;       // own_nnz: this instead of indices.size()
};
// the arrays in the dtypes the case asks for
struct Typed {
    std::vector<int32_t> p32, i32;
    std::vector<float> v32;
    CorpusRaw m;
    explicit Typed(const Raw& r) {
        p32.assign(r.indptr.begin(), r.indptr.end());
        i32.assign(r.indices.begin(), r.indices.end());
        v32.assign(r.values.begin(), r.values.end());
        m = CorpusRaw{r.n_rows, r.n_cols, r.own_nnz ? r.nnz : (int64_t)r.indices.size(),
                      r.null_indptr ? nullptr : r.pdt == RRI_I32 ? (const void*)p32.data() : (const void*)r.indptr.data(), r.pdt,
                      r.null_indices ? nullptr : r.idt == RRI_I32 ? (const void*)i32.data() : (const void*)r.indices.data(), r.idt,
                      r.pattern ? nullptr : r.vdt == RRI_F32 ? (const void*)v32.data() : (const void*)r.values.data(), r.vdt};
    }
};
static void req(const char* name, const Raw& r) {
    char msg[200] = "";
    const Typed t(r);
    const int code = corpus_check(t.m, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

template <typename V>
static void row(const char* kind, int id, const std::vector<V>& v) {
    printf("%s %d :", kind, id);
    for (const V& x : v) printf(" %.17g", (double)x);
    printf("\n");
}

// a seeded raw matrix: rows of the given lengths over n_cols columns, columns drawn with repeats, in random order; `special`
// plants the two rows whose float64 sum depends on the order
static int g_case = 0;
static void seeded(const std::vector<int64_t>& lengths, int64_t n_cols, int pdt, int idt, int vdt, bool pattern, int zero_of, bool special) {
    Raw r;
    r.n_rows = (int64_t)lengths.size() + (special ? 2 : 0);
    r.n_cols = n_cols;
    r.pdt = pdt; r.idt = idt; r.vdt = vdt; r.pattern = pattern;
    r.indptr.assign(1, 0);
    r.indices.clear();
    r.values.clear();
    for (int64_t L : lengths) {
        for (int64_t e = 0; e < L; ++e) {
            r.indices.push_back((int64_t)(rnd() % (unsigned)n_cols));
            double v = vdt == RRI_F32 ? (double)(float)((int)(rnd() % 2001) - 1000) / 64.0 : ((int)(rnd() % 2000001) - 1000000) / 1024.0 / 7.0;
            if (zero_of && rnd() % (unsigned)zero_of == 0) v = 0.0;
            r.values.push_back(vdt == RRI_F32 ? (double)(float)v : v);
        }
        r.indptr.push_back((int64_t)r.indices.size());
    }
    if (special) {
        const double a[3] = {1e16, 1.0, -1e16}, b[3] = {1e16, -1e16, 1.0};
        for (const double* s : {a, b}) {
            r.indices.push_back(2);                                // another column in front and between: the sort has to bring them together
            r.values.push_back(5.0);
            for (int e = 0; e < 3; ++e) {
                r.indices.push_back(1);
                r.values.push_back(s[e]);
            }
            r.indptr.push_back((int64_t)r.indices.size());
        }
    }
    const Typed t(r);
    char msg[200] = "";
    if (corpus_check(t.m, msg, sizeof msg) != TOPN_REQ_OK) { printf("seeded case %d refused: %s\n", g_case, msg); exit(1); }
    const CorpusCanonical c = corpus_canonical_plain(t.m);
    const int id = g_case++;
    printf("case %d : %lld %lld %d %d %d %d\n", id, (long long)r.n_rows, (long long)r.n_cols, pdt, idt, vdt, (int)pattern);
    row("rawptr", id, r.indptr);
    row("rawidx", id, r.indices);
    row("rawval", id, r.values);
    row("indptr", id, c.indptr);
    row("indices", id, c.indices);
    row("values", id, c.values);
    printf("stats %d : %lld %lld %lld %lld %lld\n", id, (long long)c.rows_rewritten, (long long)c.duplicates, (long long)c.zeros,
           (long long)c.negatives, (long long)c.long_rows);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    Raw r;
    req("fine", r);
    r = Raw(); r.indices = {3, 0, 5, 1, 1}; r.values = {0.0, 2.0, -3.0, 1.0, 4.0}; req("unsorted_duplicates_zeros_negatives", r);
    r = Raw(); r.pattern = true; req("pattern", r);
    r = Raw(); r.pdt = RRI_I32; r.idt = RRI_I32; r.vdt = RRI_F32; req("narrow_dtypes", r);
    r = Raw(); r.n_rows = 0; r.indptr = {0}; r.indices.clear(); r.values.clear(); req("no_rows", r);
    r = Raw(); r.indptr = {0, 0, 0, 0}; r.indices.clear(); r.values.clear(); r.null_indices = true; req("no_entries", r);
    r = Raw(); r.n_cols = 0x7fffffffLL; req("widest_n_cols", r);
    // the arguments, before any array is read
    r = Raw(); r.n_rows = -1; req("negative_n_rows", r);
    r = Raw(); r.n_cols = -1; req("negative_n_cols", r);
    r = Raw(); r.own_nnz = true; r.nnz = -1; req("negative_nnz", r);
    r = Raw(); r.pdt = RRI_F32; req("indptr_dtype", r);
    r = Raw(); r.idt = 7; req("indices_dtype", r);
    r = Raw(); r.vdt = RRI_I32; req("values_dtype", r);
    r = Raw(); r.null_indptr = true; req("indptr_null", r);
    r = Raw(); r.null_indices = true; req("indices_null", r);
    // the six rules, each at two places
    r = Raw(); r.indptr = {1, 2, 2, 5}; req("indptr_from_one", r);
    r = Raw(); r.indptr = {-2, 2, 2, 5}; req("indptr_from_minus_two", r);
    r = Raw(); r.indptr = {0, 2, 1, 5}; req("indptr_decreases_at_2", r);
    r = Raw(); r.indptr = {0, 2, 6, 5}; req("indptr_decreases_at_3", r);
    r = Raw(); r.indptr = {0, 2, 2, 4}; req("indptr_ends_short", r);
    r = Raw(); r.indptr = {0, 2, 2, 7}; req("indptr_ends_long", r);
    r = Raw(); r.indices = {0, 6, 1, 2, 5}; req("column_6_at_entry_1", r);
    r = Raw(); r.indices = {0, 3, 1, 2, -1}; req("column_negative_at_entry_4", r);
    r = Raw(); r.indices = {0, 3, 7, 2, -1}; req("two_columns_the_first_is_named", r);
    r = Raw(); r.values = {1.0, 2.0, 3.0, nan, 4.0}; req("value_nan_at_entry_3", r);
    r = Raw(); r.values = {inf, 2.0, 3.0, 1.0, nan}; req("value_inf_at_entry_0", r);
    r = Raw(); r.values = {1.0, 2.0, 3.0, 1.0, -inf}; req("value_minus_inf_at_entry_4", r);
    r = Raw(); r.indptr = {0, 2, 1, 5}; r.indices = {0, 9, 1, 2, 5}; req("indptr_before_columns", r);
    r = Raw(); r.indices = {0, 3, 1, 2, 6}; r.values = {nan, 2.0, 3.0, 1.0, 4.0}; req("columns_before_values", r);
    r = Raw(); r.n_cols = 1ll << 31; req("n_cols_2_31", r);
    r = Raw(); r.n_cols = (1ll << 31) + 5; req("n_cols_above_2_31", r);
    // a bad value is no refusal of a pattern, and the narrow dtypes are read as what they are
    r = Raw(); r.values[2] = nan; r.pattern = true; req("pattern_ignores_values", r);
    r = Raw(); r.pdt = RRI_I32; r.idt = RRI_I32; r.indices = {0, 3, 1, 6, 5}; req("narrow_column_6_at_entry_3", r);
    r = Raw(); r.vdt = RRI_F32; r.values[1] = inf; req("narrow_value_inf_at_entry_1", r);

    printf("borders : %d %d %d\n", CORPUS_WAVE_MAX, CORPUS_LDS_MAX, CORPUS_PAD_MIN);
    for (int64_t len : {0ll, 1ll, 2ll, 63ll, 64ll, 65ll, 127ll, 128ll, 129ll, 16383ll, 16384ll, 16385ll, 1ll << 20})
        printf("class %lld : %d %d %lld\n", (long long)len, corpus_row_class(false, len), corpus_row_class(true, len), (long long)corpus_pad(len));
    const unsigned long long k = corpus_key(0x7fffffff, 0xfffffffell);
    printf("key : %u %u %d %d\n", corpus_key_col(k), corpus_key_pos(k), (int)(k < CORPUS_KEY_PAD), (int)(corpus_key(3, 9) < corpus_key(4, 0)));

    seeded({5, 0, 9, 1, 30}, 8, RRI_I64, RRI_I64, RRI_F64, false, 5, false);
    seeded({5, 0, 9, 1, 30}, 8, RRI_I32, RRI_I32, RRI_F32, false, 4, false);
    seeded({3, 70, 2}, 20, RRI_I32, RRI_I64, RRI_F64, true, 0, false);
    seeded({4, 4}, 1000, RRI_I64, RRI_I32, RRI_F64, false, 0, true);
    seeded({}, 5, RRI_I64, RRI_I64, RRI_F64, false, 0, false);
    seeded({200, 17}, 40, RRI_I64, RRI_I32, RRI_F32, false, 3, false);
    printf("ok %d cases\n", g_case);
    return 0;
}
