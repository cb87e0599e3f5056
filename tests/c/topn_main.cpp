// Stand-alone driver of rri_topn.hpp for tests/test_topn_cpu.py: built with the host compiler under AddressSanitizer and
// UndefinedBehaviorSanitizer, run once.  It prints
//   stream <id> <N> <len> : <column>:<bits of the score> ...      a seeded stream in ARRIVAL order (heavy ties, NaN, +-inf)
//   list <id> : <column>:<bits> ...                                 the N slots after every pair went through topn_insert
//   clip <bits v> <bits lo> <bits hi> : <bits of topn_clip>
//   req <name> : <code of topn_check_request>
// and checks topn_excluded against a linear scan itself.  The test compares the lists with the numpy restatement.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rri_hip.h"
#include "rri_topn.hpp"

static uint64_t g_state = 0;
static uint32_t rnd() {
    g_state = g_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(g_state >> 33);
}
static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

static int run_stream(int id, int N, int len, int flavour) {
    g_state = 1000003ULL * (uint64_t)(id + 1);
    std::vector<double> v((size_t)len);
    std::vector<int> order((size_t)len);
    for (int j = 0; j < len; ++j) {
        order[(size_t)j] = j;
        const uint32_t r = rnd();
        double x;
        if (flavour == 0) x = (double)(r % 3u);                                          // three values: ties everywhere
        else if (flavour == 1) x = (double)(r % 1000u) / 7.0 - 50.0;                     // mostly distinct, both signs
        else x = (r % 5u == 0) ? std::numeric_limits<double>::quiet_NaN()                 // NaN, both infinities, ties
                 : (r % 5u == 1) ? std::numeric_limits<double>::infinity()
                 : (r % 5u == 2) ? -std::numeric_limits<double>::infinity() : (double)(r % 4u) - 1.5;
        v[(size_t)j] = x;
    }
    for (int j = len - 1; j > 0; --j) {                     // the arrival order: a seeded permutation of the columns
        const int o = (int)(rnd() % (uint32_t)(j + 1));
        const int t = order[(size_t)j];
        order[(size_t)j] = order[(size_t)o];
        order[(size_t)o] = t;
    }
    std::vector<double> vals((size_t)N, std::numeric_limits<double>::quiet_NaN());
    std::vector<int> idx((size_t)N, -1);
    printf("stream %d %d %d :", id, N, len);
    for (int a = 0; a < len; ++a) {
        const int j = order[(size_t)a];
        printf(" %d:%016" PRIx64, j, bits(v[(size_t)j]));
        (void)rri::topn_insert(vals.data(), idx.data(), N, v[(size_t)j], j);
    }
    printf("\nlist %d :", id);
    for (int p = 0; p < N; ++p) printf(" %d:%016" PRIx64, idx[(size_t)p], bits(vals[(size_t)p]));
    printf("\n");
    return 0;
}

static int check_excluded() {
    g_state = 77;
    for (int trial = 0; trial < 200; ++trial) {
        const int d = 1 + (int)(rnd() % 300u);
        std::vector<int32_t> e;
        e.push_back(-7);                                    // a guard entry in front: the segment starts at 1
        for (int j = 0; j < d; ++j)
            if (rnd() % 3u == 0) e.push_back(j);
        e.push_back(d + 5);                                 // ... and one behind it
        const int64_t lo = 1, hi = (int64_t)e.size() - 1;
        for (int j = -1; j <= d; ++j) {
            bool lin = false;
            for (int64_t p = lo; p < hi; ++p) lin = lin || e[(size_t)p] == j;
            if (rri::topn_excluded(e.data(), lo, hi, j) != lin) {
                printf("topn_excluded wrong: trial %d column %d\n", trial, j);
                return 1;
            }
        }
    }
    return 0;
}

static void req(const char* name, int64_t n, int64_t d, const int64_t* rows, int64_t count, int32_t topn, const int64_t* ptr,
                const int32_t* ind) {
    char msg[200] = "";
    const int code = rri::topn_check_request(n, d, rows, count, topn, RRI_MAX_TOPN, ptr, ind, msg, sizeof msg);
    printf("req %s : %d\n", name, code);
    if ((code != 0) != (msg[0] != 0)) printf("req %s : message and code disagree\n", name);
}

int main() {
    int id = 0;
    const int Ns[] = {1, 2, 10, 64};
    const int lens[] = {0, 1, 5, 64, 300};
    for (int flavour = 0; flavour < 3; ++flavour)
        for (int N : Ns)
            for (int len : lens)
                if (run_stream(id++, N, len, flavour)) return 1;
    if (check_excluded()) return 1;

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double vs[] = {-inf, -2.0, 0.5, 3.0, inf}, los[] = {nan, 1.0}, his[] = {nan, 2.5};
    for (double v : vs)
        for (double lo : los)
            for (double hi : his)
                printf("clip %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " : %016" PRIx64 "\n", bits(v), bits(lo), bits(hi),
                       bits(rri::topn_clip(v, lo, hi)));

    // requests on n = 5 rows, d = 7 columns
    const int64_t rows_ok[] = {4, 0, 0, 3}, rows_hi[] = {0, 5}, rows_neg[] = {-1, 0};
    const int64_t ptr_ok[] = {0, 2, 2, 5, 5}, ptr_empty[] = {0, 0, 0, 0, 0}, ptr_start[] = {1, 2, 2, 5, 5}, ptr_down[] = {0, 3, 2, 5, 5};
    const int32_t ind_ok[] = {1, 6, 0, 3, 4}, ind_hi[] = {1, 7, 0, 3, 4}, ind_neg[] = {-1, 6, 0, 3, 4}, ind_eq[] = {1, 6, 0, 3, 3},
                  ind_down[] = {6, 1, 0, 3, 4};
    req("all_rows", 5, 7, nullptr, 5, 10, nullptr, nullptr);
    req("listed_rows_with_duplicates", 5, 7, rows_ok, 4, 1, nullptr, nullptr);
    req("longest_list", 5, 7, rows_ok, 4, RRI_MAX_TOPN, nullptr, nullptr);
    req("no_rows", 5, 7, nullptr, 0, 10, nullptr, nullptr);
    req("exclusion", 5, 7, rows_ok, 4, 10, ptr_ok, ind_ok);
    req("exclusion_all_rows", 5, 7, nullptr, 4, 10, ptr_ok, ind_ok);
    req("empty_exclusion", 5, 7, rows_ok, 4, 10, ptr_empty, nullptr);
    req("negative_count", 5, 7, nullptr, -1, 10, nullptr, nullptr);
    req("topn_zero", 5, 7, nullptr, 5, 0, nullptr, nullptr);
    req("topn_too_long", 5, 7, nullptr, 5, RRI_MAX_TOPN + 1, nullptr, nullptr);
    req("more_rows_than_W_has", 5, 7, nullptr, 6, 10, nullptr, nullptr);
    req("row_n", 5, 7, rows_hi, 2, 10, nullptr, nullptr);
    req("row_negative", 5, 7, rows_neg, 2, 10, nullptr, nullptr);
    req("indptr_not_from_zero", 5, 7, rows_ok, 4, 10, ptr_start, ind_ok);
    req("indptr_decreases", 5, 7, rows_ok, 4, 10, ptr_down, ind_ok);
    req("indices_null", 5, 7, rows_ok, 4, 10, ptr_ok, nullptr);
    req("column_d", 5, 7, rows_ok, 4, 10, ptr_ok, ind_hi);
    req("column_negative", 5, 7, rows_ok, 4, 10, ptr_ok, ind_neg);
    req("column_twice", 5, 7, rows_ok, 4, 10, ptr_ok, ind_eq);
    req("columns_descend", 5, 7, rows_ok, 4, 10, ptr_ok, ind_down);
    printf("ok %d streams\n", id);
    return 0;
}
