// Stand-alone check of rri_nmf_amd/csrc/rri_corpus_rank.hpp (own main, host compiler, sanitizers): the request check rule by rule
// with its texts, the piece list cut per corpus row against rank_cut_pieces, the classification of an entry, and the plain loops
// (row terms and totals) on a case whose results are computed by hand in tests/test_corpus_rank_cpu.py, which reads what this
// program prints.  With a file name as argument the cases in that file are run through the plain loops as well and printed as
// hexadecimal floats: the Python side compares them bit for bit with its numpy restatement (tests/corpus_rank_cases.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_corpus_rank.hpp"

using namespace rri;

struct Req {
    int call = CRANK_CALL_RANK;
    int64_t n = 4, d = 6;
    int device = 0;
    CrankCorpus targets{true, true, 3, 6, 0}, exclude{true, true, 4, 6, 0};
    std::vector<int64_t> rows{2, 0, 3};
    bool null_rows = false;
    int64_t count = 3, n_items = 10;
    int32_t topn = 10;
    double lo = 1.0, hi = 5.0;
};
static void req(const char* name, const Req& r) {
    char msg[200] = "";
    const int code = crank_check_request(r.call, r.n, r.d, r.device, r.targets, r.exclude, r.null_rows ? nullptr : r.rows.data(), r.count,
                                         r.topn, 64, r.n_items, r.lo, r.hi, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

static void pieces(const char* kind, const std::vector<RankPiece>& p) {
    printf("%s :", kind);
    for (const RankPiece& x : p) printf(" %lld,%lld,%d,%d", (long long)x.req, (long long)x.t0, (int)x.cnt, (int)x.first);
    printf("\n");
}

static void run_case(const char* tag, bool hex, int64_t m, int64_t d, int64_t n_items, double rf, const std::vector<int64_t>& indptr,
                     const std::vector<double>& values, const std::vector<int32_t>& rank, const std::vector<int32_t>& elig) {
    std::vector<double> table, ideal, terms((size_t)m * CRANK_TERMS, -1.0);
    crank_table(crank_table_len(n_items, d), &table, &ideal);
    crank_rows_plain(indptr.data(), values.data(), m, rank.data(), elig.data(), n_items, rf, table.data(), ideal.data(), terms.data());
    double out[CRANK_OUT];
    crank_sum_plain(terms.data(), m, out);
    printf("%s\nterms :", tag);
    for (double t : terms) printf(hex ? " %a" : " %.17g", t);
    printf("\ntotals :");
    for (double t : out) printf(hex ? " %a" : " %.17g", t);
    printf("\n");
}

int main(int argc, char** argv) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // ---- the request check: every rule has its own text
    req("fine", Req());
    { Req r; r.null_rows = true; req("rows_null", r); }
    { Req r; r.rows = {1, 1, 1}; req("duplicate_rows", r); }
    { Req r; r.exclude.given = false; r.exclude.alive = false; req("no_exclusion", r); }
    { Req r; r.lo = -inf; r.hi = inf; req("open", r); }
    { Req r; r.lo = r.hi = 3.0; req("lo_is_hi", r); }
    { Req r; r.call = CRANK_CALL_METRICS; r.lo = nan; r.hi = nan; req("metrics_fine", r); }
    { Req r; r.call = CRANK_CALL_METRICS; r.n_items = 1000000; req("metrics_many_items", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.targets = CrankCorpus{false, false, 0, 0, 0}; req("topn_fine", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.topn = 64; r.count = 0; r.null_rows = true; req("topn_no_requests", r); }
    { Req r; r.targets.given = false; r.targets.alive = false; req("targets_null", r); }
    { Req r; r.targets.alive = false; req("targets_destroyed", r); }
    { Req r; r.targets.device = 1; req("targets_other_device", r); }
    { Req r; r.exclude.alive = false; req("exclusion_destroyed", r); }
    { Req r; r.exclude.device = 2; req("exclusion_other_device", r); }
    { Req r; r.exclude.rows = 3; req("exclusion_other_rows", r); }
    { Req r; r.exclude.cols = 7; req("exclusion_other_columns", r); }
    { Req r; r.targets.cols = 7; req("other_columns", r); }
    { Req r; r.null_rows = true; r.n = 2; r.exclude.rows = 2; req("rows_null_corpus_above_n", r); }
    { Req r; r.rows[1] = 4; req("row_n", r); }
    { Req r; r.rows[2] = -1; req("row_negative", r); }
    { Req r; r.lo = nan; req("lo_nan", r); }
    { Req r; r.hi = nan; req("hi_nan", r); }
    { Req r; r.lo = 5.5; req("lo_above_hi", r); }
    { Req r; r.call = CRANK_CALL_METRICS; r.n_items = 0; req("no_items", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.count = -1; req("topn_negative_count", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.topn = 0; req("topn_zero", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.topn = 65; req("topn_65", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.null_rows = true; r.count = 5; req("topn_rows_null_count_above_n", r); }
    { Req r; r.call = CRANK_CALL_TOPN; r.rows[0] = 4; req("topn_row_n", r); }

    // ---- the pieces: rows of 0, 1, 63, 64, 65 and 129 entries, against rank_cut_pieces without the rows that have none
    {
        const int lens[6] = {0, 1, 63, 64, 65, 129};
        std::vector<int64_t> indptr{0};
        for (int l : lens) indptr.push_back(indptr.back() + l);
        std::vector<int64_t> first(7, -1);
        std::vector<RankPiece> mine((size_t)crank_cut_plain(indptr.data(), 6, nullptr, nullptr));
        const int64_t np = crank_cut_plain(indptr.data(), 6, first.data(), mine.data());
        std::vector<RankPiece> all((size_t)rank_cut_pieces(indptr.data(), 6, nullptr)), kept;
        rank_cut_pieces(indptr.data(), 6, all.data());
        for (const RankPiece& p : all)
            if (indptr[p.req + 1] > indptr[p.req]) kept.push_back(p);
        pieces("pieces", mine);
        pieces("rank_cut_pieces", kept);
        printf("first :");
        for (int64_t f : first) printf(" %lld", (long long)f);
        printf("\n");
        if (np != (int64_t)mine.size() || kept.size() != mine.size()) return 1;
    }

    // ---- an entry
    printf("entry : %d %d %d %d %d %d %d %d\n", (int)crank_relevant(3.0, nan), (int)crank_relevant(3.0, 3.0), (int)crank_relevant(2.5, 3.0),
           (int)crank_eligible(0), (int)crank_eligible(-1), (int)crank_hit(9, 10), (int)crank_hit(10, 10), (int)crank_hit(-1, 10));

    // ---- the plain loops on the case worked out by hand: five rows, d = 20
    {
        const std::vector<int64_t> indptr{0, 3, 3, 5, 6, 7};
        const std::vector<double> values{5.0, 3.0, 1.0, 2.0, 3.0, 5.0, 5.0};
        const std::vector<int32_t> rank{0, 9, -1, 1, 2, 0, -1}, elig{10, -1, 3, 1, 0};
        run_case("hand 0", false, 5, 20, 1, nan, indptr, values, rank, elig);
        run_case("hand 1", false, 5, 20, 2, 4.0, indptr, values, rank, elig);
    }

    // ---- the cases of a file: m d n_items relevant_from, then indptr, values, ranks, eligible counts
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        long long m, d, n_items;
        char rf_text[64];
        int at = 0;
        while (fscanf(f, "%lld %lld %lld %63s", &m, &d, &n_items, rf_text) == 4) {
            const double rf = strtod(rf_text, nullptr);
            std::vector<int64_t> indptr((size_t)m + 1);
            for (auto& x : indptr) { long long v; if (fscanf(f, "%lld", &v) != 1) return 3; x = v; }
            const size_t nnz = (size_t)indptr.back();
            std::vector<double> values(nnz);
            std::vector<int32_t> rank(nnz), elig((size_t)m);
            for (auto& x : values) if (fscanf(f, "%lf", &x) != 1) return 3;
            for (auto& x : rank) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = v; }
            for (auto& x : elig) { int v; if (fscanf(f, "%d", &v) != 1) return 3; x = v; }
            char tag[32];
            snprintf(tag, sizeof tag, "file %d", at++);
            run_case(tag, true, m, d, n_items, rf, indptr, values, rank, elig);
        }
        fclose(f);
    }
    printf("ok\n");
    return 0;
}
