// Stand-alone check of rri_nmf_amd/csrc/rri_loglik.hpp (own main, host compiler, sanitizers): the request check rule by rule, the
// pieces of segments around LL_SEG, the chunks at small budgets, the lane rule for every k, and the plain loop on seeded cases
// whose factors, requests and results are printed for tests/test_loglik_cpu.py to hold against numpy.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_loglik.hpp"

using namespace rri;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33);
}
static double unif() { return (rnd() % 1000000 + 1) / 1000001.0; }      // inside (0, 1)

struct Req {
    int64_t n = 4, d = 6, count = 3;
    std::vector<int64_t> rows{2, 0, 3};
    std::vector<int64_t> indptr{0, 2, 2, 5};
    std::vector<int32_t> indices{0, 3, 1, 2, 5};
    std::vector<double> values{1.0, 2.0, 3.0, 1.0, 4.0};
    double floor = 1e-12;
    bool null_rows = false, null_indptr = false, null_indices = false, null_values = false;
    bool null_ll = false, null_mass = false, null_floored = false;
};
static void req(const char* name, const Req& r) {
    char msg[200] = "";
    std::vector<double> ll(4), mass(4);
    std::vector<int64_t> fl(4);
    const int code = loglik_check_request(r.n, r.d, r.null_rows ? nullptr : r.rows.data(), r.count, r.null_indptr ? nullptr : r.indptr.data(),
                                          r.null_indices ? nullptr : r.indices.data(), r.null_values ? nullptr : r.values.data(), r.floor,
                                          r.null_ll ? nullptr : ll.data(), r.null_mass ? nullptr : mass.data(),
                                          r.null_floored ? nullptr : fl.data(), msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

static void pieces(int64_t len) {
    // three requests: one without entries in front, the segment, one entry behind
    const std::vector<int64_t> indptr{7, 7, 7 + len, 8 + len};
    std::vector<int64_t> first(4, -1);
    const int64_t np = loglik_cut_pieces(indptr.data(), 0, 3, nullptr, nullptr);
    std::vector<LoglikPiece> pc((size_t)np);
    if (loglik_cut_pieces(indptr.data(), 0, 3, pc.data(), first.data()) != np) { printf("piece count of %lld\n", (long long)len); exit(1); }
    printf("pieces %lld :", (long long)len);
    for (const LoglikPiece& p : pc) printf(" %d:%lld:%d", p.req, (long long)p.e0, p.cnt);
    printf(" |");
    for (int64_t f : first) printf(" %lld", (long long)f);
    printf("\n");
}

static void chunks(const char* name, const std::vector<int64_t>& lengths, int64_t budget) {
    std::vector<int64_t> indptr{0};
    for (int64_t L : lengths) indptr.push_back(indptr.back() + L);
    std::vector<LoglikChunk> ch;
    const int64_t nc = loglik_cut_chunks(indptr.data(), (int64_t)lengths.size(), budget, &ch);
    if (nc != (int64_t)ch.size() || nc != loglik_cut_chunks(indptr.data(), (int64_t)lengths.size(), budget, nullptr)) { printf("chunk count of %s\n", name); exit(1); }
    printf("chunks %s :", name);
    for (const LoglikChunk& c : ch) printf(" %lld:%lld", (long long)c.q0, (long long)c.q1);
    printf("\n");
}

template <typename V>
static void row(const char* kind, int id, const std::vector<V>& v) {
    printf("%s %d :", kind, id);
    for (const V& x : v) printf(" %.17g", (double)x);
    printf("\n");
}

// a seeded case: factors, `count` requests with repeated rows, segments of up to max_len entries, explicit zeros, and per mode
// 1: a row of W and a column of T with disjoint supports (p exactly 0), 2: a NaN in a row of W
static void plain(int id, int n, int d, int k, int count, int max_len, double floor, int mode) {
    std::vector<double> W((size_t)n * k), T((size_t)k * d);
    for (double& w : W) w = unif();
    for (double& t : T) t = unif();
    if (mode == 1)
        for (int t = 0; t < k; ++t) {
            if (t % 2) W[(size_t)0 * k + t] = 0.0; else T[(size_t)t * d + 0] = 0.0;
        }
    if (mode == 2) W[0] = std::numeric_limits<double>::quiet_NaN();
    std::vector<int64_t> rows, indptr{0};
    std::vector<int32_t> indices;
    std::vector<double> values;
    for (int q = 0; q < count; ++q) {
        rows.push_back(q < 2 ? (q * (n - 1)) % n : (int64_t)(rnd() % (unsigned)n));
        const int len = q == 1 ? 0 : (int)(rnd() % (unsigned)(max_len + 1));
        int left = len;
        for (int j = 0; j < d && left > 0; ++j)
            if ((int)(rnd() % (unsigned)(d - j)) < left) {
                indices.push_back(j);
                values.push_back(rnd() % 5 == 0 ? 0.0 : (id % 2 ? (double)(rnd() % 9 + 1) : 3.0 * unif()));
                --left;
            }
        indptr.push_back((int64_t)indices.size());
    }
    if (mode == 1 && indptr[1] == 0) {                       // request 0 (row 0) holds column 0
        indices.insert(indices.begin(), 0);
        values.insert(values.begin(), 2.0);
        for (size_t q = 1; q < indptr.size(); ++q) indptr[q] += 1;
    } else if (mode == 1) {
        indices[0] = 0;
        values[0] = 2.0;
    }
    std::vector<double> ll((size_t)count, -1.0), mass((size_t)count, -1.0);
    std::vector<int64_t> fl((size_t)count, -1);
    char msg[200] = "";
    if (loglik_check_request(n, d, rows.data(), count, indptr.data(), indices.data(), values.data(), floor, ll.data(), mass.data(), fl.data(),
                             msg, sizeof msg) != TOPN_REQ_OK) {
        printf("case %d is refused: %s\n", id, msg);
        exit(1);
    }
    loglik_plain(W.data(), T.data(), d, k, rows.data(), count, indptr.data(), indices.data(), values.data(), floor, ll.data(), mass.data(), fl.data());
    printf("case %d : %d %d %d %d %.17g\n", id, n, d, k, count, floor);
    row("W", id, W);
    row("T", id, T);
    row("rows", id, rows);
    row("indptr", id, indptr);
    row("indices", id, indices);
    row("values", id, values);
    row("ll", id, ll);
    row("mass", id, mass);
    row("floored", id, fl);
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- the request check: every rule has its own text
    req("fine", Req());
    { Req r; r.count = 0; r.indptr = {0}; r.null_indices = r.null_values = r.null_ll = r.null_mass = r.null_floored = true; req("no_requests", r); }
    { Req r; r.indptr = {0, 0, 0, 0}; r.null_indices = r.null_values = true; req("no_entries", r); }
    { Req r; r.null_rows = true; req("rows_null", r); }
    { Req r; r.rows = {1, 1, 1}; req("duplicate_rows", r); }
    { Req r; r.values[1] = 0.0; req("explicit_zero_value", r); }
    { Req r; r.floor = 0.0; req("floor_zero", r); }
    { Req r; r.d = (64ll << 20) / 12; req("widest_d", r); }
    { Req r; r.d = (64ll << 20) / 12 + 1; req("d_too_wide", r); }
    { Req r; r.count = -1; req("negative_count", r); }
    { Req r; r.floor = -1e-300; req("floor_negative", r); }
    { Req r; r.floor = nan; req("floor_nan", r); }
    { Req r; r.floor = inf; req("floor_infinite", r); }
    { Req r; r.null_indptr = true; req("indptr_null", r); }
    { Req r; r.null_rows = true; r.n = 2; req("rows_null_count_above_n", r); }
    { Req r; r.rows[1] = 4; req("row_n", r); }
    { Req r; r.rows[2] = -1; req("row_negative", r); }
    { Req r; r.indptr = {1, 2, 2, 5}; req("indptr_not_from_zero", r); }
    { Req r; r.indptr = {0, 2, 1, 5}; req("indptr_decreases", r); }
    { Req r; r.null_indices = true; req("indices_null", r); }
    { Req r; r.null_values = true; req("values_null", r); }
    { Req r; r.indices[1] = 6; req("column_d", r); }
    { Req r; r.indices[0] = -1; req("column_negative", r); }
    { Req r; r.indices = {0, 3, 2, 2, 5}; req("column_twice", r); }
    { Req r; r.indices = {3, 0, 1, 2, 5}; req("columns_descend", r); }
    { Req r; r.values[2] = -0.5; req("value_negative", r); }
    { Req r; r.values[3] = nan; req("value_nan", r); }
    { Req r; r.values[4] = inf; req("value_infinite", r); }
    { Req r; r.null_ll = true; req("ll_null", r); }
    { Req r; r.null_mass = true; req("mass_null", r); }
    { Req r; r.null_floored = true; req("floored_null", r); }

    // ---- the pieces of a segment: at most LL_SEG entries each, in order; no entry, no piece
    printf("seg : %d\n", LL_SEG);
    for (int64_t len : {(int64_t)0, (int64_t)1, (int64_t)LL_SEG - 1, (int64_t)LL_SEG, (int64_t)LL_SEG + 1, (int64_t)2 * LL_SEG + 3}) pieces(len);

    // ---- the chunks: whole requests while their entries fit budget / 12, at least one request
    printf("budget : %lld %lld\n", (long long)LL_UPLOAD_BUDGET, (long long)LL_ENTRY_BYTES);
    chunks("none", {}, 1200);
    chunks("budget_below_one_request", {5, 0, 7, 3}, 24);          // 2 entries fit: every request with entries alone
    chunks("exactly_one_chunk", {40, 0, 50, 10, 0}, 1200);         // 100 entries fit
    chunks("one_entry_more", {40, 0, 50, 11, 0}, 1200);
    chunks("budget_not_a_multiple", {40, 0, 50, 10, 1}, 1211);     // still 100
    chunks("empty_requests_in_front", {0, 0, 100, 1}, 1200);

    // ---- lanes that share an entry
    printf("lanes :");
    for (int k = 1; k <= 1024; ++k) printf(" %d", loglik_lanes(k));
    printf("\nkp :");
    for (int k = 1; k <= 9; ++k) printf(" %d", loglik_kp(k));
    printf("\n");

    // ---- the plain loop on seeded cases
    int id = 0;
    plain(id++, 1, 1, 1, 3, 1, 1e-12, 0);
    plain(id++, 5, 7, 2, 6, 7, 1e-12, 0);
    plain(id++, 9, 40, 3, 12, 40, 1e-12, 0);
    plain(id++, 6, 33, 17, 9, 20, 1e-12, 1);                 // an exact zero, floored
    plain(id++, 6, 33, 16, 9, 20, 0.0, 1);                   // an exact zero and no floor: -inf
    plain(id++, 4, 12, 5, 8, 12, 1e-12, 2);                  // a NaN in row 0 of W
    plain(id++, 3, 300, 50, 4, 300, 12.0, 0);                // a floor that many p fall below (p is about k / 4)
    plain(id++, 7, 20, 129, 10, 20, 1e-12, 0);
    printf("ok %d cases\n", id);
    return 0;
}
