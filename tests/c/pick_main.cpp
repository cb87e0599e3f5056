// Stand-alone program over rri_nmf_amd/csrc/rri_pick.hpp, the header that turns run-time values into the template arguments of
// the kernels rri_hip.hip launches.  It prints what every pick reached; tests/test_pick_cpu.py compares each line with the
// rule.  Built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "rri_hip.h"
#include "rri_pick.hpp"

using namespace rri;

// the 2-byte element type: the compiler's own where it has one, a stand-in with the same dtype code elsewhere
#ifdef __FLT16_MANT_DIG__
typedef _Float16 half_t;
#else
struct half_t { unsigned short bits; };
namespace rri { template <> constexpr int dtype_code<half_t> = RRI_F16; }
#endif

template <typename T> constexpr const char* type_name() {
    return std::is_same<T, float>::value ? "float" : std::is_same<T, double>::value ? "double" : std::is_same<T, half_t>::value ? "half" : "?";
}

// a stand-in for a kernel template: an instantiation that must not exist fails to compile
template <bool MK, bool WE, int KS, bool SM>
int resid_kernel() {
    static_assert(SM || WE, "SM = false exists only for WRITE_E = true");
    return 1000 * MK + 100 * WE + 10 * SM + KS;
}

int main() {
    int calls = 0;
    // pick_int: the residual's rank buckets (default 16) and the LPS of sp_blk (default 64); listed values, unlisted ones, extremes
    for (int v : {-2147483647 - 1, -1, 0, 4, 5, 8, 12, 13, 14, 16, 17, 2147483647}) {
        calls = 0;
        const int got = pick_int<4, 8, 12, 13, 16>(v, [&](auto ks) { ++calls; return (int)ks * 3; });
        std::printf("int5 %d -> %d calls %d\n", v, got, calls);
    }
    for (int v : {8, 16, 32, 64, 7, 0, 128}) {
        calls = 0;
        const int got = pick_int<8, 16, 32, 64>(v, [&](auto lps) { ++calls; constexpr int LPS = lps; return LPS; });
        std::printf("int4 %d -> %d calls %d\n", v, got, calls);
    }
    calls = 0;
    const int only = pick_int<7>(3, [&](auto one) { ++calls; return (int)one; });
    std::printf("int1 %d -> %d calls %d\n", 3, only, calls);
    for (int b = 0; b < 2; ++b) {
        calls = 0;
        const bool got = pick_bool(b != 0, [&](auto flag) { ++calls; return std::is_same<decltype(flag), std::true_type>::value; });
        std::printf("bool %d -> %d calls %d\n", b, (int)got, calls);
    }
    // pick_type: the three codes and codes that are none of them, over the lists the library uses
    for (int code : {(int)RRI_F32, (int)RRI_F64, (int)RRI_F16, -1, 3}) {
        calls = 0;
        const char* t3 = pick_type<float, double, half_t>(code, [&](auto t) { ++calls; return type_name<typename decltype(t)::type>(); });
        const char* t2 = pick_type<float, double>(code, [&](auto t) {
            ++calls;
            static_assert(!std::is_same<typename decltype(t)::type, half_t>::value, "a list without the half type never reaches it");
            return type_name<typename decltype(t)::type>();
        });
        const char* r2 = pick_type<double, float>(code, [&](auto t) { ++calls; return type_name<typename decltype(t)::type>(); });
        std::printf("type %d -> %s %s %s calls %d\n", code, t3, t2, r2, calls);
    }
    // the return value comes back as it is: a reference stays a reference, void stays void
    int slot[2] = {0, 0};
    int& ref = pick_bool(true, [&](auto flag) -> int& { return slot[flag ? 1 : 0]; });
    ref = 7;
    pick_int<1, 2>(2, [&](auto v) { slot[0] = v; });
    std::printf("ref %d %d %d\n", slot[0], slot[1], (int)(&ref == &slot[1]));
    // a nest of three picks, driven over all inputs: each point of the cross product once
    int visits[2][3][2] = {};
    for (int b = 0; b < 2; ++b)
        for (int v = 0; v < 3; ++v)
            for (int code = 0; code < 2; ++code)
                pick_bool(b != 0, [&](auto B) {
                    pick_int<0, 1, 2>(v, [&](auto V) {
                        pick_type<float, double>(code, [&](auto t) {
                            visits[B ? 1 : 0][V][std::is_same<typename decltype(t)::type, double>::value ? 1 : 0] += 1;
                        });
                    });
                });
    for (int b = 0; b < 2; ++b)
        for (int v = 0; v < 3; ++v) std::printf("nest %d %d -> %d %d\n", b, v, visits[b][v][0], visits[b][v][1]);
    // a nest shaped like the residual's: masked x write_e x rank bucket x row sums, where SM = false exists only with WRITE_E
    for (int masked = 0; masked < 2; ++masked)
        for (int write_e = 0; write_e < 2; ++write_e)
            for (int ks : {4, 8, 12, 13, 16})
                for (int sums = 0; sums < 2; ++sums) {
                    int got = -1;
                    calls = 0;
                    pick_bool(masked != 0, [&](auto MK) {
                        pick_bool(write_e != 0, [&](auto WE) {
                            pick_int<4, 8, 12, 13, 16>(ks, [&](auto KS) {
                                pick_bool(sums || !WE, [&](auto SM) {
                                    ++calls;
                                    if constexpr (SM || WE) got = resid_kernel<MK, WE, KS, SM>();
                                });
                            });
                        });
                    });
                    std::printf("site %d %d %d %d -> %d calls %d\n", masked, write_e, ks, sums, got, calls);
                }
    std::printf("ok\n");
    return 0;
}
