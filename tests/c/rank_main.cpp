// Stand-alone driver of rri_rank.hpp for tests/test_rank_cpu.py: built with the host compiler under AddressSanitizer and
// UndefinedBehaviorSanitizer, run once.  It prints
//   stream <id> <len> <bits lo> <bits hi> : <bits of the score of column 0> ...   a seeded row of scores
//   excl <id> : <column> ...                                                     its exclusion segment (ascending)
//   tgt <id> : <column> ...                                                      its targets (ascending)
//   rank <id> : <rank>:<bits of val> ...        per target, a serial count written from the header's predicates
//   elig <id> : <eligible>
//   cut <name> : <req>:<t0>:<cnt>:<first> ...                                    the pieces of a target indptr
//   req <name> : <code of rank_check_request>
// The test compares ranks, values and eligible counts with the numpy restatement and the pieces with what it expects.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rri_rank.hpp"

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

// flavour 0: three values only; 1: mostly distinct; 2: NaN, both infinities and ties.  tkind 0: random targets; 1: every
// excluded column and a few others; 2: every column
static void run_stream(int id, int len, int flavour, int tkind, double lo, double hi) {
    g_state = 2000003ULL * (uint64_t)(id + 1);
    std::vector<double> v((size_t)len);
    std::vector<int32_t> excl, tgt;
    excl.push_back(-3);                                     // a guard entry in front: the segment starts at 1
    for (int j = 0; j < len; ++j) {
        const uint32_t r = rnd();
        double x;
        if (flavour == 0) x = (double)(r % 3u);
        else if (flavour == 1) x = (double)(r % 1000u) / 7.0 - 50.0;
        else x = (r % 5u == 0) ? std::numeric_limits<double>::quiet_NaN()
                 : (r % 5u == 1) ? std::numeric_limits<double>::infinity()
                 : (r % 5u == 2) ? -std::numeric_limits<double>::infinity() : (double)(r % 4u) - 1.5;
        v[(size_t)j] = x;
        const bool ex = rnd() % 4u == 0;
        if (ex) excl.push_back(j);
        const bool t = tkind == 2 || (tkind == 1 && (ex || rnd() % 8u == 0)) || (tkind == 0 && rnd() % 3u == 0);
        if (t) tgt.push_back(j);
    }
    excl.push_back(len + 2);                                // ... and one behind it
    const int64_t e0 = 1, e1 = (int64_t)excl.size() - 1;
    printf("stream %d %d %016" PRIx64 " %016" PRIx64 " :", id, len, bits(lo), bits(hi));
    for (int j = 0; j < len; ++j) printf(" %016" PRIx64, bits(v[(size_t)j]));
    printf("\nexcl %d :", id);
    for (int64_t p = e0; p < e1; ++p) printf(" %d", excl[(size_t)p]);
    printf("\ntgt %d :", id);
    for (int32_t j : tgt) printf(" %d", j);
    printf("\nrank %d :", id);
    int eligible = 0;
    for (int j = 0; j < len; ++j)
        if (!rri::topn_excluded(excl.data(), e0, e1, j) && v[(size_t)j] == v[(size_t)j]) ++eligible;
    for (int32_t jt : tgt) {
        const double vt = v[(size_t)jt];
        const bool out = rri::topn_excluded(excl.data(), e0, e1, jt);
        int counted = 0;
        for (int j = 0; j < len; ++j) {
            if (rri::rank_counts(v[(size_t)j], j, vt, jt) != rri::rank_counts_plain(v[(size_t)j], j, vt, jt))
                printf(" rank_counts and its plain form disagree at column %d", j);
            if (!rri::topn_excluded(excl.data(), e0, e1, j) && rri::rank_counts(v[(size_t)j], j, vt, jt)) ++counted;
        }
        printf(" %d:%016" PRIx64, rri::rank_result(counted, vt, out), bits(rri::rank_value(vt, out, lo, hi)));
    }
    printf("\nelig %d : %d\n", id, eligible);
}

static int cut(const char* name, const std::vector<int64_t>& counts) {
    std::vector<int64_t> ptr(1, 0);
    for (int64_t c : counts) ptr.push_back(ptr.back() + c);
    const int64_t np = rri::rank_cut_pieces(ptr.data(), (int64_t)counts.size(), nullptr);
    std::vector<rri::RankPiece> pc((size_t)np);
    if (rri::rank_cut_pieces(ptr.data(), (int64_t)counts.size(), pc.data()) != np) {
        printf("cut %s : the two passes disagree\n", name);
        return 1;
    }
    printf("cut %s :", name);
    for (const rri::RankPiece& p : pc) printf(" %lld:%lld:%d:%d", (long long)p.req, (long long)p.t0, p.cnt, p.first);
    printf("\n");
    return 0;
}

static void req(const char* name, int64_t n, int64_t d, const int64_t* rows, int64_t count, const int64_t* tptr, const int32_t* tind,
                const int64_t* eptr, const int32_t* eind) {
    char msg[200] = "";
    const int code = rri::rank_check_request(n, d, rows, count, tptr, tind, eptr, eind, msg, sizeof msg);
    printf("req %s : %d\n", name, code);
    if ((code != 0) != (msg[0] != 0)) printf("req %s : message and code disagree\n", name);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int id = 0;
    const int lens[] = {1, 5, 64, 65, 300};
    for (int flavour = 0; flavour < 3; ++flavour)
        for (int tkind = 0; tkind < 3; ++tkind)
            for (int len : lens) {
                const bool clip = (id % 2) == 1;
                run_stream(id, len, flavour, tkind, clip ? -0.5 : nan, clip ? 1.0 : nan);
                ++id;
            }

    if (cut("none", {})) return 1;
    if (cut("empty_requests", {0, 0, 3, 0})) return 1;
    if (cut("borders", {1, 63, 64, 65, 128, 129, 0, 257})) return 1;

    // requests on n = 5 rows, d = 7 columns
    const int64_t rows_ok[] = {4, 0, 0, 3}, rows_hi[] = {0, 5}, rows_neg[] = {-1, 0};
    const int64_t ptr_ok[] = {0, 2, 2, 5, 5}, ptr_empty[] = {0, 0, 0, 0, 0}, ptr_start[] = {1, 2, 2, 5, 5}, ptr_down[] = {0, 3, 2, 5, 5};
    const int32_t ind_ok[] = {1, 6, 0, 3, 4}, ind_hi[] = {1, 7, 0, 3, 4}, ind_neg[] = {-1, 6, 0, 3, 4}, ind_eq[] = {1, 6, 0, 3, 3},
                  ind_down[] = {6, 1, 0, 3, 4};
    req("all_rows", 5, 7, nullptr, 4, ptr_ok, ind_ok, nullptr, nullptr);
    req("listed_rows_with_duplicates", 5, 7, rows_ok, 4, ptr_ok, ind_ok, nullptr, nullptr);
    req("no_rows", 5, 7, nullptr, 0, ptr_empty, nullptr, nullptr, nullptr);
    req("no_targets", 5, 7, rows_ok, 4, ptr_empty, nullptr, nullptr, nullptr);
    req("targets_and_exclusion", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_ok, ind_ok);
    req("empty_exclusion", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_empty, nullptr);
    req("negative_count", 5, 7, nullptr, -1, ptr_ok, ind_ok, nullptr, nullptr);
    req("more_rows_than_W_has", 5, 7, nullptr, 6, ptr_ok, ind_ok, nullptr, nullptr);
    req("row_n", 5, 7, rows_hi, 2, ptr_ok, ind_ok, nullptr, nullptr);
    req("row_negative", 5, 7, rows_neg, 2, ptr_ok, ind_ok, nullptr, nullptr);
    req("tgt_indptr_null", 5, 7, rows_ok, 4, nullptr, ind_ok, nullptr, nullptr);
    req("tgt_indptr_not_from_zero", 5, 7, rows_ok, 4, ptr_start, ind_ok, nullptr, nullptr);
    req("tgt_indptr_decreases", 5, 7, rows_ok, 4, ptr_down, ind_ok, nullptr, nullptr);
    req("tgt_indices_null", 5, 7, rows_ok, 4, ptr_ok, nullptr, nullptr, nullptr);
    req("target_d", 5, 7, rows_ok, 4, ptr_ok, ind_hi, nullptr, nullptr);
    req("target_negative", 5, 7, rows_ok, 4, ptr_ok, ind_neg, nullptr, nullptr);
    req("target_twice", 5, 7, rows_ok, 4, ptr_ok, ind_eq, nullptr, nullptr);
    req("targets_descend", 5, 7, rows_ok, 4, ptr_ok, ind_down, nullptr, nullptr);
    req("excl_indptr_decreases", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_down, ind_ok);
    req("excl_indices_null", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_ok, nullptr);
    req("excluded_column_d", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_ok, ind_hi);
    req("excluded_columns_descend", 5, 7, rows_ok, 4, ptr_ok, ind_ok, ptr_ok, ind_down);
    printf("ok %d streams\n", id);
    return 0;
}
