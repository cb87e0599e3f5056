// Stand-alone program over rri_nmf_amd/csrc/rri_halt.hpp, the header every kernel takes its halting rules from.  It prints the
// verdict of every rule for the full cross product of the inputs; tests/test_halt_rules_cpu.py compares each line with a Python
// restatement of the reference's rules.  Built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "rri_halt.hpp"

using namespace rri;

// the layouts the host and the kernels share
static_assert(sizeof(DevState) == 72 && offsetof(DevState, halt) == 0 && offsetof(DevState, halt_topic) == 4 &&
              offsetof(DevState, halt_sweep) == 8 && offsetof(DevState, halt_pos) == 12 && offsetof(DevState, tmode) == 16 &&
              offsetof(DevState, nt1) == 32 && offsetof(DevState, obj_track) == 64, "DevState layout");
static_assert(sizeof(KParams) == 88 && offsetof(KParams, reset_method) == 20 && offsetof(KParams, resets_left) == 24 &&
              offsetof(KParams, t_row_sum) == 32 && offsetof(KParams, eps) == 80, "KParams layout");

static int check_halt_set() {
    DevState st;
    unsigned char before[sizeof(DevState)], after[sizeof(DevState)];
    std::memset(&st, 0xA5, sizeof st);
    std::memcpy(before, &st, sizeof st);
    halt_set(&st, HALT_ERR_W_COL_ZERO, 7, 11, 13);
    std::memcpy(after, &st, sizeof st);
    if (st.halt != HALT_ERR_W_COL_ZERO || st.halt_topic != 7 || st.halt_sweep != 11 || st.halt_pos != 13) return 1;
    for (size_t i = offsetof(DevState, tmode); i < sizeof st; ++i)
        if (after[i] != before[i]) return 1;
    return 0;
}

int main() {
    const double vals[9] = {std::numeric_limits<double>::quiet_NaN(), -1.0, -0.0, 0.0, 5e-324, 1e-10, std::nextafter(1e-10, 1.0),
                            1.0, std::numeric_limits<double>::infinity()};
    for (int i = 0; i < 9; ++i) {
        uint64_t bits;
        std::memcpy(&bits, &vals[i], 8);
        std::printf("value %d %016llx\n", i, (unsigned long long)bits);
    }
    const int resets_left[3] = {0, 1, 3};
    long cases = 0;
    for (int vi = 0; vi < 9; ++vi)
    for (int rm = 0; rm < 3; ++rm)
    for (int rl = 0; rl < 3; ++rl)
    for (int negflag = 0; negflag < 2; ++negflag)
    for (int has_wrs = 0; has_wrs < 2; ++has_wrs)
    for (int wrs = 0; wrs < 2; ++wrs)
    for (int project_T = 0; project_T < 2; ++project_T)
    for (int has_trs = 0; has_trs < 2; ++has_trs)
    for (int trs = 0; trs < 3; ++trs) {
        KParams p = {};
        p.reset_method = rm; p.resets_left = resets_left[rl]; p.has_wrs = has_wrs; p.w_row_sum = wrs;
        p.project_T = project_T; p.has_trs = has_trs; p.t_row_sum = trs;
        const double v = vals[vi];
        std::printf("case %d %d %d %d %d %d %d %d %d : %d %d %d %d %d %d\n", vi, rm, resets_left[rl], negflag, has_wrs, wrs, project_T,
                    has_trs, trs, wcol_code(v, p), wwcol_code(v, (double)negflag, p), (int)trow_kept(v, p), (int)trow_resets(v, p),
                    trow_denominator_mode(v, p), wcol_denominator_mode(v, p));
        ++cases;
    }
    // next_step(sweep, t, k): t = 0, k - 2, k - 1, and k = 1
    const int steps[][3] = {{4, 0, 5}, {4, 3, 5}, {4, 4, 5}, {0, 0, 2}, {0, 1, 2}, {4, 0, 1}, {0, 0, 1}};
    for (const auto& q : steps) {
        const StepPos n = next_step(q[0], q[1], q[2]);
        std::printf("next %d %d %d : %d %d\n", q[0], q[1], q[2], n.sweep, n.pos);
    }
    if (check_halt_set()) {
        std::printf("halt_set FAILED\n");
        return 1;
    }
    std::printf("ok %ld cases\n", cases);
    return 0;
}
