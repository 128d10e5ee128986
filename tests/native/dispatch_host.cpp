// dispatch_host.cpp — the flag-to-instantiation rule of the entry points (csrc/cmx_dispatch.hpp) compiled by g++ for
// tests/test_dispatch_host.py.  Each case dispatches its selectors to a lambda that records how often it ran and which tags it got; the tags
// reach the record as TEMPLATE arguments (tags<…>), as a kernel's would, so a tag that were not a compile-time constant would not compile.
#include <cstdint>
#include <type_traits>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_dispatch.hpp"

namespace {

struct Record { int32_t calls = 0; int32_t tag[3] = {-99, -99, -99}; };
template <int... V> void tags(Record &r) {
    const int v[] = {V...};
    ++r.calls;
    for (unsigned k = 0; k < sizeof...(V); ++k) r.tag[k] = v[k];
}
template <typename T> constexpr bool is_flag_tag = std::is_same_v<T, std::true_type> || std::is_same_v<T, std::false_type>;

enum : int { KIND_A = 0, KIND_B = 1, KIND_C = 2, KIND_D = 3 };      // an unnamed enum, as the kernels' velocity kinds are
constexpr uint32_t kLow = 0x4003u, kAll = 0xffffffffu;                // unsigned values of which one does not fit an int

}  // namespace

using namespace cmx;

// case: selectors (a, b, c are the run-time values)
//  0: flag(a)                                      1: one_of<3, 5, 9>(a)                       2: flag(a), one_of<KIND_A … KIND_D>(b)
//  3: one_of<1, 2, 4>(a), flag(b)                  4: flag(a), one_of<10, 20, 30>(b), flag(c)  5: one_of<1, 2>(a), one_of<7, 8, 9>(b), one_of<-1, 0>(c)
//  6: one_of<kLow, kAll>(a) (tag recorded as 0 / 1)
//  7: dispatch_or(miss, …) with case 4's selectors, the lambda returns 1000 + 100 a + b + c
//  8: dispatch_or(miss, …) with case 1's selector and an excluded combination as `if constexpr` inside (9 returns -9 without recording)
// out: calls, tag[0..2], and what dispatch / dispatch_or returned
extern "C" void dispatch_host(int32_t which, int64_t a, int64_t b, int64_t c, int32_t miss, int32_t *out) {
    Record r;
    int32_t ret = -12345;
    switch (which) {
    case 0:
        ret = dispatch([&](auto A) {
            static_assert(is_flag_tag<decltype(A)>);
            tags<decltype(A)::value>(r);
        }, flag(a != 0));
        break;
    case 1:
        ret = dispatch([&](auto A) {
            static_assert(std::is_same_v<typename decltype(A)::value_type, int>);
            tags<decltype(A)::value>(r);
        }, one_of<3, 5, 9>((int)a));
        break;
    case 2:
        ret = dispatch([&](auto A, auto B) {
            static_assert(is_flag_tag<decltype(A)> && !is_flag_tag<decltype(B)>);
            tags<decltype(A)::value, decltype(B)::value>(r);
        }, flag(a != 0), one_of<KIND_A, KIND_B, KIND_C, KIND_D>((int)b));
        break;
    case 3:
        ret = dispatch([&](auto A, auto B) {
            static_assert(!is_flag_tag<decltype(A)> && is_flag_tag<decltype(B)>);
            tags<decltype(A)::value, decltype(B)::value>(r);
        }, one_of<1, 2, 4>((int)a), flag(b != 0));
        break;
    case 4:
        ret = dispatch([&](auto A, auto B, auto C) {
            static_assert(is_flag_tag<decltype(A)> && !is_flag_tag<decltype(B)> && is_flag_tag<decltype(C)>);
            tags<decltype(A)::value, decltype(B)::value, decltype(C)::value>(r);
        }, flag(a != 0), one_of<10, 20, 30>((int)b), flag(c != 0));
        break;
    case 5:
        ret = dispatch([&](auto A, auto B, auto C) { tags<decltype(A)::value, decltype(B)::value, decltype(C)::value>(r); },
                       one_of<1, 2>((int)a), one_of<7, 8, 9>((int)b), one_of<-1, 0>((int)c));
        break;
    case 6:
        ret = dispatch([&](auto A) {
            static_assert(std::is_same_v<typename decltype(A)::value_type, uint32_t>);
            tags<decltype(A)::value == kAll>(r);
        }, one_of<kLow, kAll>((uint32_t)a));
        break;
    case 7:
        ret = dispatch_or(miss, [&](auto A, auto B, auto C) {
            tags<decltype(A)::value, decltype(B)::value, decltype(C)::value>(r);
            return (int32_t)(1000 + 100 * decltype(A)::value + decltype(B)::value + decltype(C)::value);
        }, flag(a != 0), one_of<10, 20, 30>((int)b), flag(c != 0));
        break;
    case 8:
        ret = dispatch_or(miss, [&](auto A) -> int32_t {
            if constexpr (decltype(A)::value == 9) return -9;
            else {
                tags<decltype(A)::value>(r);
                return 0;
            }
        }, one_of<3, 5, 9>((int)a));
        break;
    default: break;
    }
    out[0] = r.calls;
    out[1] = r.tag[0];
    out[2] = r.tag[1];
    out[3] = r.tag[2];
    out[4] = ret;
}
