// Stand-alone check of rri_nmf_amd/csrc/rri_rowsplit.hpp (own main, host compiler, sanitizers): the constants, the quota at its
// edges, the verdict and text of every refusal, and the plain loop of the split by row -- against a full sort of every row written
// here, with a degenerate key whose word0 is one number, for the nesting of the held sets in the quota and for the agreement with
// split_entries_plain -- on seeded matrices, whose inputs and results are printed for tests/test_rowsplit_cpu.py to hold against the
// numpy restatement (tests/rowsplit_cases.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "rri_rowsplit.hpp"

using namespace rri;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
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
[[noreturn]] static void die(const char* what, long long a = 0, long long b = 0) {
    printf("FAILED: %s (%lld, %lld)\n", what, a, b);
    exit(1);
}

// rows of the given lengths over n_cols columns, ascending random columns, reals of either sign
static DeriveCsr seeded_csr(const std::vector<int>& lengths, int64_t n_cols) {
    DeriveCsr a;
    a.n_rows = (int64_t)lengths.size();
    a.n_cols = n_cols;
    a.indptr.assign(1, 0);
    for (int L : lengths) {
        std::set<int32_t> cols;
        while ((int)cols.size() < L) cols.insert((int32_t)(rnd() % (unsigned)n_cols));
        for (int32_t j : cols) {
            double v = ((int)(rnd() % 2000001) - 1000000) / 1024.0 / 7.0;
            if (v == 0.0) v = 1.5;
            a.indices.push_back(j);
            a.values.push_back(v);
        }
        a.indptr.push_back((int64_t)a.indices.size());
    }
    return a;
}

struct OneWord0 {          // every word0 equal: the column alone orders a row
    uint32_t operator()(int64_t, int32_t, uint64_t) const { return 0x89abcdefu; }
};

// the split by a full sort of (key, position) per row, written apart from the header's selection
template <typename Word0>
static void brute(const DeriveCsr& a, int64_t n_held, double fraction, int64_t min_observed, uint64_t seed, DeriveCsr* observed, DeriveCsr* held,
                  Word0 word0) {
    for (DeriveCsr* o : {observed, held}) {
        o->n_rows = a.n_rows;
        o->n_cols = a.n_cols;
        o->indptr.assign(1, 0);
        o->indices.clear();
        o->values.clear();
    }
    for (int64_t r = 0; r < a.n_rows; ++r) {
        const int64_t lo = a.indptr[(size_t)r], hi = a.indptr[(size_t)r + 1], L = hi - lo;
        int64_t want = n_held >= 1 ? n_held : (int64_t)std::floor(fraction * (double)L + 0.5);
        const int64_t h = std::min(want, std::max<int64_t>(L - min_observed, 0));
        std::vector<std::pair<uint64_t, int64_t>> order;
        for (int64_t p = lo; p < hi; ++p) order.push_back({((uint64_t)word0(r, a.indices[(size_t)p], seed) << 32) | (uint32_t)a.indices[(size_t)p], p});
        std::sort(order.begin(), order.end());
        std::vector<char> out((size_t)L, 0);
        for (int64_t q = 0; q < h; ++q) out[(size_t)(order[(size_t)q].second - lo)] = 1;
        for (int64_t p = lo; p < hi; ++p) {
            DeriveCsr* o = out[(size_t)(p - lo)] ? held : observed;
            o->indices.push_back(a.indices[(size_t)p]);
            o->values.push_back(a.values[(size_t)p]);
        }
        held->indptr.push_back((int64_t)held->indices.size());
        observed->indptr.push_back((int64_t)observed->indices.size());
    }
}
static bool equal(const DeriveCsr& a, const DeriveCsr& b) {
    if (a.n_rows != b.n_rows || a.n_cols != b.n_cols || a.indptr != b.indptr || a.indices != b.indices || a.values.size() != b.values.size()) return false;
    for (size_t p = 0; p < a.values.size(); ++p)
        if (a.values[p] != b.values[p]) return false;
    return true;
}

static int g_cases = 0;
static void split_case(const DeriveCsr& a, int64_t n_held, double fraction, int64_t min_observed, uint64_t seed) {
    char msg[200] = "";
    if (rowsplit_check_request(n_held, fraction, min_observed, true, true, msg, sizeof msg) != TOPN_REQ_OK) die(msg);
    DeriveCsr obs, held, bobs, bheld;
    split_rows_plain(a, n_held, fraction, min_observed, seed, &obs, &held);
    brute(a, n_held, fraction, min_observed, seed, &bobs, &bheld, RowsplitWord0());
    if (!equal(obs, bobs) || !equal(held, bheld)) die("the plain loop differs from the full sort", g_cases);
    for (int64_t r = 0; r < a.n_rows; ++r) {
        const int64_t L = a.indptr[(size_t)r + 1] - a.indptr[(size_t)r], h = held.indptr[(size_t)r + 1] - held.indptr[(size_t)r];
        if (h != rowsplit_quota(L, n_held, fraction, min_observed)) die("a row does not give up its quota", g_cases, r);
        if (h + obs.indptr[(size_t)r + 1] - obs.indptr[(size_t)r] != L) die("a row loses an entry", g_cases, r);
    }
    const int id = g_cases++;
    printf("rsplit %d : %lld %.17g %lld %llu\n", id, (long long)n_held, fraction, (long long)min_observed, (unsigned long long)seed);
    csr("from", id, a);
    csr("obs", id, obs);
    csr("held", id, held);
}

static void req(const char* name, int64_t n_held, double fraction, int64_t min_observed, bool has_observed = true, bool has_held = true) {
    char msg[200] = "";
    const int code = rowsplit_check_request(n_held, fraction, min_observed, has_observed, has_held, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

// the held columns of row r
static std::vector<int32_t> held_cols(const DeriveCsr& held, int64_t r) {
    return std::vector<int32_t>(held.indices.begin() + held.indptr[(size_t)r], held.indices.begin() + held.indptr[(size_t)r + 1]);
}

int main() {
    printf("consts : %d %d %d %d %d %llu %llu\n", ROWSPLIT_WAVE_MAX, ROWSPLIT_BLOCK_THREADS, ROWSPLIT_DIGIT_BITS, ROWSPLIT_BINS, ROWSPLIT_PASSES,
           (unsigned long long)ROWSPLIT_BOUND_NONE, (unsigned long long)ROWSPLIT_BOUND_ALL);
    printf("classes : %d %d %d %d %d %d %d\n", rowsplit_class(0, 0), rowsplit_class(5, 0), rowsplit_class(5, 5), rowsplit_class(2, 1),
           rowsplit_class(64, 63), rowsplit_class(65, 1), rowsplit_class(65, 65));
    // the quota: the shortest rows under every min_observed, a count above the length, the whole row, the half-way cases
    for (int64_t L : {0, 1, 2})
        for (int64_t mo : {0, 1, 5})
            for (int64_t k : {1, 3}) printf("quota %lld %lld 0 %lld : %lld\n", (long long)L, (long long)k, (long long)mo, (long long)rowsplit_quota(L, k, 0.0, mo));
    for (int64_t L : {0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 1000, 1001})
        for (double f : {1.0, 0.5, 0.25, 0.1, 0.2})
            for (int64_t mo : {0, 1, 5}) printf("quota %lld -1 %.17g %lld : %lld\n", (long long)L, f, (long long)mo, (long long)rowsplit_quota(L, -1, f, mo));
    // the key: word 0 above, the column below; below all ones, so the bound of the largest key does not wrap
    {
        const uint64_t K = rowsplit_key((5ll << 32) | 7, 9, (3ull << 32) | 2);
        const Philox4 b = philox4x32_10(9, 7, 5, 0, 2, 3);
        if (K != (((uint64_t)b.w[0] << 32) | 9ull)) die("the key is not word 0 of block 0 above the column");
        if (rowsplit_key_of(0xffffffffu, 0x7fffffff) + 1 == 0) die("the largest key wraps");
        printf("key : %llu\n", (unsigned long long)K);
    }
    // the refusals, each text at two places, and the first broken rule wins
    req("count_one", 1, 0.0, 1);
    req("count_large", 1ll << 40, 0.0, 0);
    req("fraction_small", -1, 1e-9, 3);
    req("fraction_one", -1, 1.0, 1);
    req("min_observed_zero", 2, 0.0, 0);
    req("observed_null", 1, 0.0, 1, false, true);
    req("held_null_first", 0, 2.0, -1, true, false);
    req("count_zero", 0, 0.0, 1);
    req("count_zero_first", 0, 0.5, -1);
    req("count_minus_two", -2, 0.0, 1);
    req("count_minus_nine_first", -9, 0.5, -1);
    req("both_modes", 3, 0.5, 1);
    req("count_with_nan", 1, std::nan(""), 1);
    req("fraction_zero", -1, 0.0, 1);
    req("fraction_above_one", -1, 1.5, -1);
    req("fraction_negative", -1, -0.25, 1);
    req("fraction_nan", -1, std::nan(""), 1);
    req("min_observed_negative", 1, 0.0, -1);
    req("min_observed_negative_last", -1, 0.5, -4);

    // the plain loop against the full sort, and printed for the restatement
    const DeriveCsr small = seeded_csr({0, 1, 2, 3, 7, 0, 12, 30, 5, 64, 65, 1}, 90);
    split_case(small, 1, 0.0, 1, 12345ull);
    split_case(small, 1, 0.0, 0, 12345ull);
    split_case(small, 2, 0.0, 1, (5ull << 32) | 12345ull);
    split_case(small, 64, 0.0, 5, 3ull);
    split_case(small, 3000, 0.0, 0, 3ull);
    split_case(small, -1, 0.2, 1, 77ull);
    split_case(small, -1, 0.5, 0, 77ull);
    split_case(small, -1, 1.0, 1, 78ull);
    split_case(small, -1, 1.0, 0, 78ull);
    const DeriveCsr large = seeded_csr({200, 0, 129, 300, 17, 256, 257, 90}, 400);
    split_case(large, -1, 0.2, 1, 12345ull);
    split_case(large, 5, 0.0, 1, (9ull << 32) | 1ull);
    split_case(seeded_csr({}, 5), 1, 0.0, 1, 1ull);
    split_case(seeded_csr({0, 0, 0}, 5), -1, 0.5, 1, 1ull);

    // the degenerate key: one word0 for every entry, so a row gives up its h lowest columns
    {
        DeriveCsr obs, held, bobs, bheld;
        for (int64_t k : {1, 3, 40}) {
            split_rows_plain(small, k, 0.0, 1, 5ull, &obs, &held, OneWord0());
            brute(small, k, 0.0, 1, 5ull, &bobs, &bheld, OneWord0());
            if (!equal(obs, bobs) || !equal(held, bheld)) die("degenerate key: the plain loop differs from the full sort", k);
            for (int64_t r = 0; r < small.n_rows; ++r) {
                const int64_t lo = small.indptr[(size_t)r], h = held.indptr[(size_t)r + 1] - held.indptr[(size_t)r];
                if (h != rowsplit_quota(small.indptr[(size_t)r + 1] - lo, k, 0.0, 1)) die("degenerate key: quota", k, r);
                if (held_cols(held, r) != std::vector<int32_t>(small.indices.begin() + lo, small.indices.begin() + lo + h)) die("degenerate key: not the lowest columns", k, r);
            }
        }
        printf("degenerate : 1\n");
    }
    // nested in the quota: the held set for h is inside that for h + 1
    {
        long long pairs = 0;
        for (const DeriveCsr* a : {&small, &large})
            for (uint64_t seed : {1ull, (7ull << 32) | 2ull})
                for (int64_t k = 1; k < 70; ++k) {
                    DeriveCsr o1, h1, o2, h2;
                    split_rows_plain(*a, k, 0.0, 0, seed, &o1, &h1);
                    split_rows_plain(*a, k + 1, 0.0, 0, seed, &o2, &h2);
                    for (int64_t r = 0; r < a->n_rows; ++r) {
                        const std::vector<int32_t> s1 = held_cols(h1, r), s2 = held_cols(h2, r);
                        if (!std::includes(s2.begin(), s2.end(), s1.begin(), s1.end())) die("the held sets are not nested", k, r);
                        pairs += s2.size() > s1.size();
                    }
                }
        printf("nested : %lld\n", pairs);
    }
    // agrees with the split by entry: where split_entries holds m entries of a row, a quota of m holds the same ones
    {
        long long rows_seen = 0, by_m[4] = {0, 0, 0, 0};
        for (const DeriveCsr* a : {&small, &large})
            for (double q : {0.02, 0.1, 0.3, 0.7})
                for (uint64_t seed : {12345ull, (5ull << 32) | 9ull, 0ull}) {
                    uint32_t thr = 0;
                    if (!split_threshold(q, &thr)) die("threshold");
                    DeriveCsr eo, eh;
                    split_entries_plain(*a, thr, seed, &eo, &eh);
                    for (int64_t m = 1; m <= 300; ++m) {
                        bool any = false;
                        for (int64_t r = 0; r < a->n_rows && !any; ++r) any = eh.indptr[(size_t)r + 1] - eh.indptr[(size_t)r] == m;
                        if (!any) continue;
                        DeriveCsr o, h;
                        split_rows_plain(*a, m, 0.0, 0, seed, &o, &h);
                        for (int64_t r = 0; r < a->n_rows; ++r) {
                            if (eh.indptr[(size_t)r + 1] - eh.indptr[(size_t)r] != m) continue;
                            if (held_cols(h, r) != held_cols(eh, r)) die("a quota of m does not hold what split_entries holds", m, r);
                            rows_seen += 1;
                            by_m[m < 3 ? m : 3] += 1;
                        }
                    }
                }
        printf("agree : %lld %lld %lld %lld\n", rows_seen, by_m[1], by_m[2], by_m[3]);
    }
    printf("ok %d cases\n", g_cases);
    return 0;
}
