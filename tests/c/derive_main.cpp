// Stand-alone check of rri_nmf_amd/csrc/rri_derive.hpp (own main, host compiler, sanitizers): the generator's known answers, the
// threshold, the held part of single entries on both sides of every limit (token by token, and as the 64 lanes of a wave share
// it), the pieces, the verdict and text of every refusal, and the three plain loops on seeded canonical matrices, whose arrays
// and results are printed for tests/test_derive_cpu.py to hold against scipy and the numpy restatement (tests/derive_cases.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rri_derive.hpp"

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

// a seeded canonical matrix: every column of a row is present with probability share / 16; counts: whole numbers 1 .. top,
// otherwise reals of either sign; an empty row where `empty` says so
static DeriveCsr seeded(int64_t n_rows, int64_t n_cols, unsigned share, int top, const std::vector<int64_t>& empty) {
    DeriveCsr a;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.indptr.assign(1, 0);
    for (int64_t r = 0; r < n_rows; ++r) {
        bool skip = false;
        for (int64_t e : empty) skip = skip || e == r;
        for (int64_t j = 0; !skip && j < n_cols; ++j) {
            if (rnd() % 16 >= share) continue;
            double v = top ? (double)(1 + rnd() % (unsigned)top) : ((int)(rnd() % 2000001) - 1000000) / 1024.0 / 7.0;
            if (v == 0.0) v = 1.5;
            a.indices.push_back((int32_t)j);
            a.values.push_back(v);
        }
        a.indptr.push_back((int64_t)a.indices.size());
    }
    return a;
}

static int g_sel = 0, g_split = 0;
static void select_case(const DeriveCsr& a, bool all_rows, const std::vector<int64_t>& rows, bool all_cols, const std::vector<int32_t>& keep) {
    char msg[200] = "";
    const int64_t* rp = all_rows ? nullptr : rows.data() ? rows.data() : (const int64_t*)&g_state;      // an empty list is not NULL
    const int32_t* kp = all_cols ? nullptr : keep.data() ? keep.data() : (const int32_t*)&g_state;
    if (derive_check_select(a.n_rows, a.n_cols, rp, all_rows ? 0 : (int64_t)rows.size(), kp, all_cols ? 0 : (int64_t)keep.size(), msg, sizeof msg) != TOPN_REQ_OK) {
        printf("select case %d refused: %s\n", g_sel, msg);
        exit(1);
    }
    const DeriveCsr o = derive_select_plain(a, rp, (int64_t)rows.size(), kp, (int64_t)keep.size());
    const int id = g_sel++;
    printf("select %d : %d %d\n", id, (int)all_rows, (int)all_cols);
    csr("src", id, a);
    row("rows", id, rows);
    row("keep", id, keep);
    csr("out", id, o);
    row("df", id, derive_column_counts_plain(a));
}
static void split_case(const DeriveCsr& a, double held_out, uint64_t seed) {
    char msg[200] = "";
    uint32_t thr = 0;
    if (!split_threshold(held_out, &thr) || split_check_values(a.values.data(), (int64_t)a.values.size(), msg, sizeof msg) != TOPN_REQ_OK) {
        printf("split case %d refused: %s\n", g_split, msg);
        exit(1);
    }
    DeriveCsr obs, held;
    derive_split_plain(a, thr, seed, &obs, &held);
    const int id = g_split++;
    printf("split %d : %u %llu\n", id, thr, (unsigned long long)seed);
    csr("from", id, a);
    csr("obs", id, obs);
    csr("held", id, held);
}

static void thr_line(const char* name, double held_out) {
    uint32_t thr = 0;
    const bool ok = split_threshold(held_out, &thr);
    printf("thr %s : %d %u\n", name, (int)ok, thr);
}
static void sel_req(const char* name, int64_t n_rows, int64_t n_cols, const int64_t* rows, int64_t m, const int32_t* keep, int64_t dk) {
    char msg[200] = "";
    const int code = derive_check_select(n_rows, n_cols, rows, m, keep, dk, msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}
static void val_req(const char* name, const std::vector<double>& v) {
    char msg[200] = "";
    const int code = split_check_values(v.data(), (int64_t)v.size(), msg, sizeof msg);
    printf("req %s : %d : %s\n", name, code, msg);
}

int main() {
    printf("consts : %d %d %lld %d\n", DERIVE_PIECE, SPLIT_LANE_MAX, (long long)SPLIT_COUNT_MAX, (int)SPLIT_RULES);
    // the generator's known answers
    const uint32_t kat[3][6] = {{0, 0, 0, 0, 0, 0},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (int i = 0; i < 3; ++i) {
        const Philox4 r = philox4x32_10(kat[i][0], kat[i][1], kat[i][2], kat[i][3], kat[i][4], kat[i][5]);
        printf("philox %d : %08x %08x %08x %08x\n", i, r.w[0], r.w[1], r.w[2], r.w[3]);
    }
    {   // the counter and the key of an entry: (column, row low, row high, block; seed low, seed high)
        const Philox4 a = split_block((5ll << 32) | 7, 9, (3ull << 32) | 2, 11), b = philox4x32_10(9, 7, 5, 11, 2, 3);
        printf("block : %d\n", (int)(a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3]));
    }
    thr_line("half", 0.5);
    thr_line("three_tenths", 0.3);
    thr_line("smallest", std::ldexp(1.0, -32));
    thr_line("below_smallest", std::nextafter(std::ldexp(1.0, -32), 0.0));
    thr_line("below_one", std::nextafter(1.0, 0.0));
    thr_line("one", 1.0);
    thr_line("zero", 0.0);
    thr_line("negative", -0.25);
    thr_line("nan", std::nan(""));
    // the held part of one entry: token by token, and as 64 lanes share the blocks
    const struct { int64_t row; int32_t col; uint64_t seed; uint32_t thr; } where[2] = {{3, 17, 12345ull, 0x80000000u},
                                                                                     {(1ll << 32) + 5, 2999, (77ull << 32) | 9ull, 0x4ccccccdu}};
    for (const auto& w : where)
        for (int64_t count : {0ll, 1ll, 3ll, 4ll, 5ll, 8ll, 9ll, (long long)SPLIT_LANE_MAX - 1, (long long)SPLIT_LANE_MAX, (long long)SPLIT_LANE_MAX + 1,
                              (long long)SPLIT_COUNT_MAX}) {
            int64_t lanes = 0;
            for (int lane = 0; lane < 64; ++lane) lanes += split_held_blocks(w.row, w.col, count, w.thr, w.seed, lane, 64);
            printf("held %lld %d %llu %u %lld : %lld %lld\n", (long long)w.row, w.col, (unsigned long long)w.seed, w.thr, (long long)count,
                   (long long)split_held(w.row, w.col, count, w.thr, w.seed), (long long)lanes);
        }
    {   // the pieces of rows on both sides of the piece length, one of them taken twice
        const std::vector<int64_t> lengths{0, 1, DERIVE_PIECE - 1, DERIVE_PIECE, DERIVE_PIECE + 1, 2 * DERIVE_PIECE + 1};
        std::vector<int64_t> ptr{0};
        for (int64_t L : lengths) ptr.push_back(ptr.back() + L);
        const DerivePieces all = derive_cut_pieces(ptr.data(), (int64_t)lengths.size(), nullptr, 0);
        row("piecerow", 0, all.row); row("piecesrc", 0, all.src); row("piecelen", 0, all.len);
        const std::vector<int64_t> rows{5, 0, 4, 4, 1};
        const DerivePieces some = derive_cut_pieces(ptr.data(), (int64_t)lengths.size(), rows.data(), (int64_t)rows.size());
        row("piecerow", 1, some.row); row("piecesrc", 1, some.src); row("piecelen", 1, some.len);
    }
    // the requests: every refusal at two places, and the first broken rule wins
    {
        const int64_t r_ok[3] = {4, 0, 4}, r_neg[3] = {4, -1, 9}, r_big[3] = {0, 1, 5};
        const int32_t k_ok[3] = {0, 2, 5}, k_neg[3] = {-2, 2, 5}, k_big[3] = {0, 2, 6}, k_same[3] = {0, 2, 2}, k_down[3] = {3, 1, 2};
        sel_req("fine", 5, 6, r_ok, 3, k_ok, 3);
        sel_req("all_rows_all_columns", 5, 6, nullptr, 0, nullptr, 0);
        sel_req("empty_lists", 5, 6, r_ok, 0, k_ok, 0);
        sel_req("negative_rows_out", 5, 6, r_ok, -1, k_ok, 3);
        sel_req("negative_rows_out_first", 5, 6, r_ok, -7, k_ok, -2);
        sel_req("negative_cols_out", 5, 6, r_ok, 3, k_ok, -2);
        sel_req("negative_cols_out_first", 5, 6, nullptr, 3, k_ok, -5);
        sel_req("rows_null_with_count", 5, 6, nullptr, 3, k_ok, 3);
        sel_req("rows_null_with_count_first", 5, 6, nullptr, 2, nullptr, 3);
        sel_req("keep_null_with_count", 5, 6, r_ok, 3, nullptr, 3);
        sel_req("keep_null_with_count_first", 5, 6, r_neg, 3, nullptr, 1);
        sel_req("row_negative_at_1", 5, 6, r_neg, 3, k_ok, 3);
        sel_req("row_5_at_2", 5, 6, r_big, 3, k_ok, 3);
        sel_req("rows_before_keep", 5, 6, r_big, 3, k_big, 3);
        sel_req("keep_negative_at_0", 5, 6, r_ok, 3, k_neg, 3);
        sel_req("keep_6_at_2", 5, 6, r_ok, 3, k_big, 3);
        sel_req("range_before_order", 5, 3, r_ok, 3, k_down, 3);
        sel_req("keep_repeats_at_2", 5, 6, r_ok, 3, k_same, 3);
        sel_req("keep_descends_at_1", 5, 6, r_ok, 3, k_down, 3);
    }
    {
        char msg[200] = "";
        int code = derive_check_corpus(false, 0, 0, msg, sizeof msg);
        printf("req corpus_dead : %d : %s\n", code, msg);
        code = derive_check_corpus(true, 2, 1, msg, sizeof msg);
        printf("req corpus_elsewhere : %d : %s\n", code, msg);
        code = derive_check_corpus(true, 0, 3, msg, sizeof msg);
        printf("req corpus_elsewhere_too : %d : %s\n", code, msg);
        msg[0] = 0;
        code = derive_check_corpus(true, 1, 1, msg, sizeof msg);
        printf("req corpus_fine : %d : %s\n", code, msg);
        code = derive_check_split(0, true, true, msg, sizeof msg);
        printf("req threshold_zero : %d : %s\n", code, msg);
        code = derive_check_split(5, false, true, msg, sizeof msg);
        printf("req observed_null : %d : %s\n", code, msg);
        code = derive_check_split(0, true, false, msg, sizeof msg);
        printf("req held_null_first : %d : %s\n", code, msg);
        msg[0] = 0;
        code = derive_check_split(1, true, true, msg, sizeof msg);
        printf("req split_fine : %d : %s\n", code, msg);
    }
    val_req("counts_fine", {1.0, 2.0, 1048576.0, 7.0});
    val_req("no_values", {});
    val_req("negative_at_2", {1.0, 2.0, -1.0, 3.0});
    val_req("negative_at_0", {-3.0, 2.0, -1.0, 3.0});
    val_req("half_at_1", {1.0, 0.5, 2.0, 2.25});
    val_req("fraction_at_3", {1.0, 5.0, 2.0, 1048576.5});
    val_req("too_large_at_0", {1048577.0, 5.0, 2.0, 3.0});
    val_req("too_large_at_3", {1.0, 5.0, 2.0, 2097152.0});
    val_req("negative_before_fraction", {0.5, 5.0, -2.0, 3.0});
    val_req("fraction_before_too_large", {4194304.0, 5.0, 2.5, 3.0});
    val_req("negative_fraction_is_negative", {1.0, -0.5, 0.25, 3.0});

    // select and the column counts: real values of either sign, empty rows
    select_case(seeded(7, 12, 6, 0, {1, 4}), false, {3, 0, 0, 6, 2, 1}, false, {1, 4, 5, 11});
    {
        std::vector<int32_t> every_other;
        for (int32_t j = 0; j < 40; j += 2) every_other.push_back(j);
        select_case(seeded(5, 40, 9, 0, {0}), true, {}, false, every_other);
    }
    select_case(seeded(4, 9, 8, 0, {}), false, {}, true, {});
    select_case(seeded(4, 9, 8, 0, {3}), false, {3, 2, 1, 0}, false, {});
    select_case(seeded(0, 5, 8, 0, {}), true, {}, true, {});
    select_case(seeded(6, 30, 16, 3, {}), false, {5, 5, 5}, false, {0, 29});
    // split: small counts with an empty row under two seeds and two thresholds; the limits of a lane and of the split; and a
    // matrix of about 12000 tokens for the sanity bound
    const DeriveCsr small = seeded(6, 20, 7, 9, {2});
    split_case(small, 0.5, 12345ull);
    split_case(small, 0.5, 12346ull);
    split_case(small, 0.3, (5ull << 32) | 12345ull);
    DeriveCsr limits = seeded(3, 8, 16, 5, {});
    const double planted[6] = {(double)SPLIT_LANE_MAX - 1, (double)SPLIT_LANE_MAX, (double)SPLIT_LANE_MAX + 1, 1024.0, (double)SPLIT_COUNT_MAX, 1.0};
    for (int i = 0; i < 6; ++i) limits.values[(size_t)(3 * i)] = planted[i];
    split_case(limits, 0.5, 7ull);
    const DeriveCsr large = seeded(60, 50, 8, 15, {10});
    split_case(large, 0.5, 12345ull);
    split_case(large, 0.3, 12345ull);
    printf("ok %d %d cases\n", g_sel, g_split);
    return 0;
}
