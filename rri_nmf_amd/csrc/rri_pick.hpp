// rri_pick.hpp -- from a run-time value to a compile-time constant: the one way the launch layer of rri_hip.hip chooses a
// kernel instantiation.  Each pick calls the generic lambda f exactly once, with a tag that carries the chosen constant, and
// returns what f returns:
//     pick_bool(keep >= 0, [&](auto nt) { constexpr bool NT = nt; launch<NT>(...); });
// Nested picks instantiate f for the whole cross product of their domains.  Where a combination must not exist as a kernel, the
// innermost lambda leaves it out with `if constexpr` and says why.
// No HIP header is needed: a plain host compiler builds this file (tests/c/pick_main.cpp).
#pragma once
#include <type_traits>

#include "rri_hip.h"

namespace rri {

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
decltype(auto) pick_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// f(std::integral_constant<int, V>{}) for the listed V equal to v; no V equal to v: the last one (the `default:` of a switch)
template <int V0, int... Vs, typename F>
decltype(auto) pick_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return pick_int<Vs...>(v, f);
    }
}

// The element types behind the dtype codes of rri_hip.h.  f(type_tag<T>{}) for the listed T whose code is `code`; no such T:
// the last one.  The list is the caller's: a site that lists float and double cannot instantiate anything for halves.
template <typename T> struct type_tag { typedef T type; };
template <typename T> constexpr int dtype_code = -1;
template <> constexpr int dtype_code<float> = RRI_F32;
template <> constexpr int dtype_code<double> = RRI_F64;
template <> constexpr int dtype_code<unsigned char> = RRI_U8;
#ifdef __FLT16_MANT_DIG__      // (a host compiler without the type still builds the rest)
template <> constexpr int dtype_code<_Float16> = RRI_F16;
#endif

template <typename T0, typename... Ts, typename F>
decltype(auto) pick_type(int code, F&& f) {
    static_assert(dtype_code<T0> >= 0, "not an element type of rri_hip.h");
    if constexpr (sizeof...(Ts) == 0) {
        return f(type_tag<T0>{});
    } else {
        if (code == dtype_code<T0>) return f(type_tag<T0>{});
        return pick_type<Ts...>(code, f);
    }
}

}  // namespace rri
