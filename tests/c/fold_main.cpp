// fold_main.cpp -- rri_fold.hpp with the host compiler, under the sanitizers (tests/test_fold_cpu.py builds and runs it).
//
//   fold_main cases.txt
//
// Prints, for the Python side to check:
//   lds k bytes                      wfold_lds_bytes(k, FOLD_ROWS) for k = 1 .. 64, and the geometry it is made of
//   rule a w s x T W c k : 0|1       wfold_ok over the cross product of its inputs
//   entry name : w neg               fold_entry on the listed inputs, one per branch (hex floats)
//   args name : code : text          fold_check_args
//   case c / W : ... / colsum : ... / negs : ...     fold_rows_plain on the cases of the file (hex floats)
// The file: per case a line "n d k t0 reg_w_l1 reg_w_l2 has_wrs w_row_sum eps", then indptr, indices, values, T (k x d) and
// W (n x k), one line each.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rri_fold.hpp"

using namespace rri;

static bool read_doubles(FILE* f, size_t count, std::vector<double>& out) {
    out.resize(count);
    for (size_t i = 0; i < count; ++i) {
        char tok[64];
        if (fscanf(f, "%63s", tok) != 1) return false;
        out[i] = strtod(tok, nullptr);
    }
    return true;
}
template <typename I>
static bool read_ints(FILE* f, size_t count, std::vector<I>& out) {
    out.resize(count);
    for (size_t i = 0; i < count; ++i) {
        long long v;
        if (fscanf(f, "%lld", &v) != 1) return false;
        out[i] = (I)v;
    }
    return true;
}
static void print_hex(const char* name, const double* v, size_t count) {
    printf("%s :", name);
    for (size_t i = 0; i < count; ++i) printf(" %a", v[i]);
    printf("\n");
}

static KParams params(double l1, double l2, int has_wrs, double wrs, double eps) {
    KParams p{};
    p.fix_T = 1;
    p.reg_w_l1 = l1; p.reg_w_l2 = l2; p.has_wrs = has_wrs; p.w_row_sum = wrs; p.eps = eps;
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: fold_main cases.txt\n"); return 2; }
    static_assert(FOLD_MAX_K == 64 && FOLD_ROWS == 16 && FOLD_WAVES == 4, "the limits the header documents");
    for (int k = 1; k <= FOLD_MAX_K; ++k)
        printf("lds %d %zu %d %d %d\n", k, wfold_lds_bytes(k, FOLD_ROWS), fold_kt(k), fold_kpad(k), fold_gld(k));
    printf("limit %zu\n", FOLD_LDS_LIMIT);
    const int ks[] = {0, 1, 16, 17, 64, 65};
    for (int bitsv = 0; bitsv < 128; ++bitsv)
        for (int k : ks) {
            const bool a = bitsv & 1, w = bitsv & 2, s = bitsv & 4, x = bitsv & 8, fT = bitsv & 16, fW = bitsv & 32, c = bitsv & 64;
            printf("rule %d %d %d %d %d %d %d %d : %d\n", a, w, s, x, fT, fW, c, k, wfold_ok(a, w, s, x, fT, fW, c, k) ? 1 : 0);
        }
    // the update of one entry, branch by branch: s, nt, l1, l2, has_wrs, wrs
    const double eps = 0x1p-49;
    const struct { const char* name; double s, nt, l1, l2; int has; double wrs; } entries[] = {
        {"closed_form", 3.0, 2.0, 0.5, 0.5, 0, 0.0},      {"numerator_below_zero", 0.25, 2.0, 0.5, 0.0, 0, 0.0},
        {"denominator_zero", 3.0, 0.0, 0.0, 0.0, 0, 0.0}, {"denominator_negative", 3.0, 1.0, 0.0, -2.0, 0, 0.0},
        {"bounded_above", 30.0, 2.0, 0.0, 0.0, 1, 0.7},   {"bound_not_reached", 1.0, 2.0, 0.0, 0.0, 1, 0.7},
        {"negative_with_bound", 3.0, 1.0, 0.0, -2.0, 1, 0.7}, {"nan_numerator", NAN, 2.0, 0.0, 0.0, 0, 0.0}};
    for (const auto& e : entries) {
        int neg = -1;
        const double w = fold_entry(e.s, e.nt, params(e.l1, e.l2, e.has, e.wrs, eps), &neg);
        printf("entry %s : %a %d\n", e.name, w, neg);
    }
    const struct { const char* name; bool h, p, o; } args[] = {{"fine", true, true, true}, {"null_handle", false, false, true},
                                                               {"other_flavour", true, false, true}, {"null_out", true, true, false}};
    for (const auto& a : args) {
        const char* msg = "?";
        const int code = fold_check_args(a.h, a.p, a.o, &msg);
        printf("args %s : %d : %s\n", a.name, code, msg ? msg : "");
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    for (int c = 0;; ++c) {
        long long n, d;
        int k, t0, has;
        char t1[64], t2[64], t3[64], t4[64];
        if (fscanf(f, "%lld %lld %d %d %63s %63s %d %63s %63s", &n, &d, &k, &t0, t1, t2, &has, t3, t4) != 9) break;
        std::vector<int64_t> indptr;
        std::vector<int32_t> indices;
        std::vector<double> values, T, W;
        if (!read_ints(f, (size_t)n + 1, indptr) || !read_ints(f, (size_t)indptr[(size_t)n], indices) ||
            !read_doubles(f, (size_t)indptr[(size_t)n], values) || !read_doubles(f, (size_t)k * d, T) || !read_doubles(f, (size_t)n * k, W)) {
            fprintf(stderr, "case %d: short file\n", c);
            return 2;
        }
        std::vector<double> colsum((size_t)k, -1.0), negs((size_t)k, -1.0);
        fold_rows_plain(n, d, k, t0, indptr.data(), indices.data(), values.data(), T.data(), W.data(),
                        params(strtod(t1, nullptr), strtod(t2, nullptr), has, strtod(t3, nullptr), strtod(t4, nullptr)), colsum.data(), negs.data());
        printf("case %d\n", c);
        print_hex("W", W.data(), W.size());
        print_hex("colsum", colsum.data(), colsum.size());
        print_hex("negs", negs.data(), negs.size());
    }
    fclose(f);
    printf("ok\n");
    return 0;
}
