// Run-time switches -> template arguments.  A launch site writes its kernel once, inside a generic lambda, and names the switches:
//
//     lbmpm::dispatch([&](auto first, auto mrt) { kernel<decltype(first)::value, decltype(mrt)::value><<<...>>>(...); }, p.first != 0, p.mrt != 0);
//
// Every combination is instantiated (2^n for n switches), exactly one is called.  Plain C++17, nothing of HIP: tests/test_dispatch_cpu.py
// builds this header alone with the host compiler.
#pragma once
#include <type_traits>
#include <utility>

namespace lbmpm {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): one constant per switch, in argument order
template <typename F>
decltype(auto) dispatch(F &&f) { return std::forward<F>(f)(); }

template <typename F, typename... Rest>
decltype(auto) dispatch(F &&f, bool b, Rest... rest)
{
    if (b) return dispatch([&](auto... cs) -> decltype(auto) { return f(std::true_type{}, cs...); }, rest...);
    return dispatch([&](auto... cs) -> decltype(auto) { return f(std::false_type{}, cs...); }, rest...);
}

// f(std::integral_constant<int, v>{}) for v in Lo .. Hi; a value outside the range goes to Hi
template <int Lo, int Hi, typename F>
decltype(auto) dispatch_int(F &&f, int v)
{
    static_assert(Lo <= Hi, "dispatch_int<Lo, Hi>: an empty range");
    if constexpr (Lo < Hi) {
        if (v == Lo) return f(std::integral_constant<int, Lo>{});
        return dispatch_int<Lo + 1, Hi>(std::forward<F>(f), v);
    } else {
        return f(std::integral_constant<int, Hi>{});
    }
}

}  // namespace lbmpm
