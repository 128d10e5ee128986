// cmx_dispatch.hpp — run-time selectors → template arguments of ONE kernel instantiation: host code only, no HIP
// (tests/native/dispatch_host.cpp compiles it with g++).  Every entry point picks its kernel through dispatch().
#pragma once
#include <type_traits>

namespace cmx {

// A selector carries a run-time value and the compile-time values it may take.  flag(b): true / false.  one_of<V0, V1, …>(v): the
// listed values only — a mode that is not a product of flags (three ice-nucleation modes, 1…8 aerosol modes, the velocity kinds
// an entry supports) is one one_of over its values, so nothing else is instantiated.
struct Flag { bool v; };
inline Flag flag(bool v) { return {v}; }
template <typename T, auto... Vs> struct OneOf { T v; };
template <auto... Vs, typename T> inline OneOf<T, Vs...> one_of(T v) { return {v}; }

// dispatch_or(miss, f, selectors…): calls the generic lambda f ONCE with one tag per selector, in the selectors' order —
// std::true_type / std::false_type for a flag, std::integral_constant<decltype(V), V> for the listed value V that equals the run-time
// value — and returns what f returns; f is not called and `miss` is returned if a one_of value is not listed.  f is instantiated for
// the product of the listed values; a combination that must not exist stays an `if constexpr` inside f.  A tag's value is
// decltype(tag)::value: spell every template argument of the kernel out, defaulted ones included.
template <typename R, typename F> inline R dispatch_or(R, F &&f) { return f(); }
template <typename R, typename F, typename... Rest> inline R dispatch_or(R miss, F &&f, Flag s, Rest... rest);
template <typename R, typename F, typename T, auto... Vs, typename... Rest> inline R dispatch_or(R miss, F &&f, OneOf<T, Vs...> s, Rest... rest);

namespace detail {
// f with its first tag bound, dispatched over the remaining selectors
template <typename R, typename F, typename Tag, typename... Rest> inline R dispatch_bound(R miss, F &f, Tag tag, Rest... rest) {
    return dispatch_or(miss, [&](auto... more) { return f(tag, more...); }, rest...);
}
}  // namespace detail

template <typename R, typename F, typename... Rest> inline R dispatch_or(R miss, F &&f, Flag s, Rest... rest) {
    return s.v ? detail::dispatch_bound(miss, f, std::true_type{}, rest...) : detail::dispatch_bound(miss, f, std::false_type{}, rest...);
}
template <typename R, typename F, typename T, auto... Vs, typename... Rest> inline R dispatch_or(R miss, F &&f, OneOf<T, Vs...> s, Rest... rest) {
    R out = miss;
    // the fold stops at the first listed value that matches
    (void)((s.v == Vs && (out = detail::dispatch_bound(miss, f, std::integral_constant<decltype(Vs), Vs>{}, rest...), true)) || ...);
    return out;
}

// dispatch(f, selectors…): for an f that returns nothing (it launches).  True if f was called, false if a one_of value is not listed.
template <typename F, typename... S> inline bool dispatch(F &&f, S... selectors) {
    return dispatch_or(false, [&](auto... tags) { f(tags...); return true; }, selectors...);
}

}  // namespace cmx
