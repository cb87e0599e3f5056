// Stand-alone check of rri_nmf_amd/csrc/rri_fiterr.hpp (own main, host compiler, sanitizers): the clip and the term case by case,
// the request check rule by rule with its texts, and the plain loop on a 3 x 4 case whose results are computed by hand in
// tests/test_corpus_fit_cpu.py, which reads what this program prints.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_fiterr.hpp"

using namespace rri;

struct Req {
    int64_t n = 4, d = 6, c_rows = 3, c_cols = 6;
    std::vector<int64_t> rows{2, 0, 3};
    double lo = 1.0, hi = 5.0;
    bool null_rows = false;
};
static void req(const char* name, const Req& r) {
    char msg[200] = "";
    const int code = fiterr_check_request(r.n, r.d, r.c_rows, r.c_cols, r.null_rows ? nullptr : r.rows.data(), r.lo, r.hi, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

static void term(const char* name, double v, double p, double lo, double hi) {
    printf("term %s : %.17g %.17g\n", name, fiterr_clip(p, lo, hi), fiterr_term(v, p, lo, hi));
}

template <typename V>
static void row(const char* kind, const std::vector<V>& v) {
    printf("%s :", kind);
    for (const V& x : v) printf(" %.17g", (double)x);
    printf("\n");
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- the clip and the term
    term("inside", 3.0, 2.5, 1.0, 5.0);
    term("below", 3.0, 0.25, 1.0, 5.0);
    term("above", 3.0, 7.5, 1.0, 5.0);
    term("at_lo", 1.0, 1.0, 1.0, 5.0);
    term("at_hi", 4.0, 5.0, 1.0, 5.0);
    term("open", -2.0, -7.5, -inf, inf);
    term("open_below", 2.0, -7.5, -inf, 5.0);
    term("open_above", 2.0, 1e300, 1.0, inf);
    term("lo_is_hi", 2.0, 9.0, 3.0, 3.0);
    term("negative_value", -1.5, 0.5, -1.0, 1.0);
    term("nan_p", 2.0, nan, 1.0, 5.0);
    term("nan_p_open", 2.0, nan, -inf, inf);

    // ---- the request check: every rule has its own text
    req("fine", Req());
    { Req r; r.null_rows = true; req("rows_null", r); }
    { Req r; r.rows = {1, 1, 1}; req("duplicate_rows", r); }
    { Req r; r.lo = -inf; r.hi = inf; req("open", r); }
    { Req r; r.lo = r.hi = 3.0; req("lo_is_hi", r); }
    { Req r; r.c_rows = 0; r.null_rows = true; req("no_requests", r); }
    { Req r; r.d = r.c_cols = (64ll << 20) / 12; req("widest_d", r); }
    { Req r; r.d = r.c_cols = (64ll << 20) / 12 + 1; req("d_too_wide", r); }
    { Req r; r.lo = nan; req("lo_nan", r); }
    { Req r; r.hi = nan; req("hi_nan", r); }
    { Req r; r.lo = 5.5; req("lo_above_hi", r); }
    { Req r; r.c_cols = 7; req("other_columns", r); }
    { Req r; r.null_rows = true; r.n = 2; req("rows_null_corpus_above_n", r); }
    { Req r; r.rows[1] = 4; req("row_n", r); }
    { Req r; r.rows[2] = -1; req("row_negative", r); }

    // ---- the plain loop: W 3 x 2, T 2 x 4, a corpus of 3 rows (the second without entries) scored against the rows 2, 0, 1
    const std::vector<double> W{1.0, 2.0, 0.5, 0.0, 3.0, 1.0};
    const std::vector<double> T{1.0, 0.0, 2.0, 0.5, 0.5, 1.0, 0.0, 4.0};
    const std::vector<int64_t> rows{2, 0, 1}, indptr{0, 3, 3, 5};
    const std::vector<int32_t> indices{0, 2, 3, 1, 3};
    const std::vector<double> values{3.0, -1.0, 4.5, 2.0, 0.25};
    for (int pass = 0; pass < 3; ++pass) {
        const double lo = pass == 0 ? -inf : pass == 1 ? 1.0 : 2.0, hi = pass == 0 ? inf : pass == 1 ? 5.0 : 2.0;
        std::vector<double> sq(3, -1.0), ab(3, -1.0), pred(5, -1.0);
        fiterr_plain(W.data(), T.data(), 4, 2, pass == 2 ? nullptr : rows.data(), 3, indptr.data(), indices.data(), values.data(), lo, hi,
                     sq.data(), ab.data(), pred.data());
        printf("plain %d\n", pass);
        row("sq", sq);
        row("abs", ab);
        row("pred", pred);
    }
    // any output may be NULL
    fiterr_plain(W.data(), T.data(), 4, 2, rows.data(), 3, indptr.data(), indices.data(), values.data(), 1.0, 5.0, nullptr, nullptr, nullptr);
    printf("ok\n");
    return 0;
}
