// Stand-alone check of rri_nmf_amd/csrc/rri_frozen.hpp (own main, host compiler, sanitizers): the argument check rule by rule,
// the place of the addend inside red, what a reset does to the sums, the objective's share, and the plain sweep on seeded cases
// whose inputs and results are printed for tests/test_frozen_cpu.py to hold against the numpy restatement of the stacked problem.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rri_frozen.hpp"

using namespace rri;

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 33);
}
static double unif() { return (rnd() % 1000000 + 1) / 1000001.0; }      // inside (0, 1)

static void row(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) printf(" %.17g", x);
    printf("\n");
}

struct Stats {
    int k = 2;
    int64_t d = 3;
    std::vector<double> B{1.0, 0.0, 2.0, 0.5, 0.25, 0.0}, A{2.0, 0.5, 0.5, 1.0}, s{1.5, 0.75};
    double c = 4.0;
    bool null_B = false, null_A = false, null_s = false;
};
static void chk(const char* name, const Stats& q) {
    char msg[200] = "";
    const int code = frozen_check_stats(q.k, q.d, q.null_B ? nullptr : q.B.data(), q.null_A ? nullptr : q.A.data(),
                                        q.null_s ? nullptr : q.s.data(), q.c, msg, sizeof msg);
    printf("chk %s : %d : %s\n", name, code, msg);
}
static void decay(const char* name, double v) {
    char msg[200] = "";
    printf("decay %s : %d : %s\n", name, frozen_check_decay(v, msg, sizeof msg), msg);
}

// one seeded case: the frozen rows' factors and data, the live rows, the flags; the sums are taken here by plain loops
static void sweep_case(const char* name, int64_t no, int64_t nh, int64_t d, int k, const KParams& p, int cleared, int n_sweeps) {
    std::vector<double> Xo((size_t)(no * d)), Wo((size_t)(no * k)), Xh((size_t)(nh * d)), Wh((size_t)(nh * k)), T((size_t)(k * d));
    for (double& x : Xo) x = unif() < 0.5 ? 0.0 : 2.0 * unif();
    for (double& x : Xh) x = unif() < 0.5 ? 0.0 : 2.0 * unif();
    for (double& x : Wo) x = 0.1 + unif();
    for (double& x : Wh) x = 0.1 + unif();
    for (double& x : T) x = 0.1 + unif();
    if (p.project_T && p.has_trs)
        for (int t = 0; t < k; ++t) {
            double sum = 0.0;
            for (int64_t j = 0; j < d; ++j) sum += T[(size_t)(t * d + j)];
            for (int64_t j = 0; j < d; ++j) T[(size_t)(t * d + j)] *= p.t_row_sum / sum;
        }
    std::vector<double> B((size_t)(k * d), 0.0), A((size_t)(k * k), 0.0), s((size_t)k, 0.0);
    double c = 0.0;
    for (int64_t i = 0; i < no; ++i) {
        for (int t = 0; t < k; ++t) {
            for (int64_t j = 0; j < d; ++j) B[(size_t)(t * d + j)] += Wo[(size_t)(i * k + t)] * Xo[(size_t)(i * d + j)];
            for (int l = 0; l < k; ++l) A[(size_t)(t * k + l)] += Wo[(size_t)(i * k + t)] * Wo[(size_t)(i * k + l)];
            s[(size_t)t] += Wo[(size_t)(i * k + t)];
        }
        for (int64_t j = 0; j < d; ++j) c += Xo[(size_t)(i * d + j)] * Xo[(size_t)(i * d + j)];
    }
    if (cleared >= 0) frozen_clear_topic(k, d, B.data(), A.data(), s.data(), cleared);
    printf("case %s %lld %lld %lld %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", name, (long long)no, (long long)nh, (long long)d, k,
           n_sweeps, cleared, p.project_T, p.has_trs, p.t_row_sum, p.reg_w_l1, p.reg_w_l2, p.reg_t_l1, p.reg_t_l2);
    row("Xo", Xo); row("Wo", Wo); row("Xh", Xh); row("Wh0", Wh); row("T0", T);
    row("B", B); row("A", A); row("s", s);
    int code = 0, topic = -1;
    for (int it = 0; it < n_sweeps && code == 0; ++it)
        code = frozen_sweep_plain(nh, d, k, Xh.data(), Wh.data(), T.data(), B.data(), A.data(), s.data(), p, &topic);
    printf("code %d %d\n", code, topic);
    row("Wh", Wh); row("T", T);
    // the objective's share against its definition 1/2 ||Xo - Wo T||^2 (cleared topic: that column of Wo is zero)
    std::vector<double> TT((size_t)(k * k), 0.0);
    double BT = 0.0, direct = 0.0;
    for (int a = 0; a < k; ++a)
        for (int b = 0; b < k; ++b)
            for (int64_t j = 0; j < d; ++j) TT[(size_t)(a * k + b)] += T[(size_t)(a * d + j)] * T[(size_t)(b * d + j)];
    for (size_t q = 0; q < B.size(); ++q) BT += B[q] * T[q];
    for (int64_t i = 0; i < no; ++i)
        for (int64_t j = 0; j < d; ++j) {
            double r = Xo[(size_t)(i * d + j)];
            for (int t = 0; t < k; ++t) r -= (t == cleared ? 0.0 : Wo[(size_t)(i * k + t)]) * T[(size_t)(t * d + j)];
            direct += 0.5 * r * r;
        }
    printf("share %.17g %.17g %.17g\n", frozen_objective_share(k, A.data(), TT.data(), BT, c), direct, c);
}

int main() {
    // ---- the argument check, rule by rule ----
    chk("ok", Stats{});
    { Stats q; q.null_A = true; chk("null_A", q); }
    { Stats q; q.null_s = true; chk("null_s", q); }
    { Stats q; q.null_B = true; chk("null_B", q); }
    { Stats q; q.k = 0; chk("k_zero", q); }
    { Stats q; q.B[4] = -1e-300; chk("B_negative", q); }
    { Stats q; q.B[5] = std::numeric_limits<double>::quiet_NaN(); chk("B_nan", q); }
    { Stats q; q.A[3] = std::numeric_limits<double>::infinity(); chk("A_inf", q); }
    { Stats q; q.A[0] = -2.0; chk("A_negative", q); }
    { Stats q; q.A[1] = 0.5000001; chk("A_asymmetric", q); }
    { Stats q; q.A[1] = 0.5 * (1.0 + 1e-14); chk("A_symmetric_to_rounding", q); }
    { Stats q; q.s[1] = -0.5; chk("s_negative", q); }
    { Stats q; q.c = -1.0; chk("c_negative", q); }
    { Stats q; q.c = std::numeric_limits<double>::quiet_NaN(); chk("c_nan", q); }
    { Stats q; q.B.assign(6, 0.0); q.A.assign(4, 0.0); q.s.assign(2, 0.0); q.c = 0.0; chk("all_zero", q); }
    decay("one", 1.0); decay("half", 0.5); decay("zero", 0.0); decay("negative", -0.5); decay("above", 1.0000001);
    decay("nan", std::numeric_limits<double>::quiet_NaN());

    // ---- the addend inside red: columns first, then slice 0 of the Gram part ----
    printf("layout %lld %lld %lld %lld %lld\n", frozen_red_col(5), frozen_red_gram(304, 0), frozen_red_gram(304, 17), frozen_red_gram(304, 18),
           frozen_red_count(304, 17));

    // ---- a reset of topic 1 of 3 ----
    {
        std::vector<double> B(3 * 4, 1.0), A(9, 2.0), s(3, 3.0);
        frozen_clear_topic(3, 4, B.data(), A.data(), s.data(), 1);
        row("clearB", B); row("clearA", A); row("clears", s);
    }

    // ---- the plain sweep ----
    KParams plain{};
    plain.eps = 1.7763568394002505e-15;       // np.spacing(10)
    KParams tm = plain;
    tm.project_T = 1; tm.has_trs = 1; tm.has_wrs = 1; tm.t_row_sum = 1.0; tm.w_row_sum = 1.0;
    KParams pen = plain;
    pen.reg_w_l1 = 0.02; pen.reg_w_l2 = 0.3; pen.reg_t_l1 = 0.01; pen.reg_t_l2 = 0.2;
    int cases = 0;
    sweep_case("plain", 7, 9, 6, 3, plain, -1, 2); ++cases;
    sweep_case("plain_k1", 4, 5, 7, 1, plain, -1, 2); ++cases;
    sweep_case("simplex", 8, 6, 9, 4, tm, -1, 2); ++cases;
    sweep_case("penalties", 5, 11, 5, 3, pen, -1, 2); ++cases;
    sweep_case("cleared_topic", 7, 9, 6, 3, plain, 1, 2); ++cases;
    sweep_case("no_frozen_rows", 0, 9, 6, 3, tm, -1, 1); ++cases;
    printf("ok %d cases\n", cases);
    return 0;
}
