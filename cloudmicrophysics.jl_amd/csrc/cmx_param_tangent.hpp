// cmx_param_tangent.hpp — the HOST side of the parameter derivatives (include/cmx.h §(22)): exact forward mode in double through the functions that fold a
// parameter struct into a scheme's constants (make_sb_consts_from, cmx_sb2006.hpp; make_mp1m_consts_from, cmx_mp1m.hpp).  No HIP in here, no difference quotient.
//
//   ParamTan            a value and ONE tangent in double.  The value part of every operation is the plain double operation, so the value parts of a folded
//                       constants struct are the plain instantiation's in every bit; the tangent follows the analytic rule.  fmax carries the tangent of the
//                       operand it returns (the first one on a tie), like the branching operations of cmx_dual.hpp.  lgamma carries ψ(x)·ẋ (digamma
//                       below: the cloud fall-speed fold make_cloud_vel_consts_from, cmx_sb2006.hpp).
//   ParamReader         reads a field of a parameter struct as ParamTan: the value from the struct, the tangent from the field at the same offset of the
//                       DIRECTION struct (the same C type holding δθ; NULL: zero).  The parameter structs are plain aggregates of one float type.
//   pack_param_consts   a constants struct of ParamTan members → tangent slot k of the same struct of Dual<FT, KP> members (value parts rounded to FT exactly
//                       as the plain fold rounds them).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "cmx_dual.hpp"

namespace cmx {

struct ParamTan {
    double v, d;
    ParamTan() = default;
    ParamTan(double x) : v(x), d(0.0) {}      // a literal of the fold: no tangent
    ParamTan(double x, double t) : v(x), d(t) {}
    explicit operator double() const { return v; }      // the value, for the branches of a fold
};
inline ParamTan operator-(ParamTan a) { return {-a.v, -a.d}; }
inline ParamTan operator+(ParamTan a, ParamTan b) { return {a.v + b.v, a.d + b.d}; }
inline ParamTan operator-(ParamTan a, ParamTan b) { return {a.v - b.v, a.d - b.d}; }
inline ParamTan operator*(ParamTan a, ParamTan b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
inline ParamTan operator/(ParamTan a, ParamTan b) {
    const double q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
inline ParamTan log2(ParamTan x) { return {std::log2(x.v), x.d / (x.v * 0.69314718055994530942)}; }
inline ParamTan log(ParamTan x) { return {std::log(x.v), x.d / x.v}; }
inline ParamTan exp(ParamTan x) {
    const double e = std::exp(x.v);
    return {e, e * x.d};
}
inline ParamTan expm1(ParamTan x) { return {std::expm1(x.v), std::exp(x.v) * x.d}; }
inline ParamTan sqrt(ParamTan x) {
    const double s = std::sqrt(x.v);
    return {s, x.d / (2.0 * s)};
}
inline ParamTan cbrt(ParamTan x) {
    const double c = std::cbrt(x.v);
    return {c, x.d / (3.0 * c * c)};
}
inline ParamTan pow(ParamTan x, ParamTan y) {      // x > 0
    const double p = std::pow(x.v, y.v);
    return {p, p * (y.d * std::log(x.v) + y.v * x.d / x.v)};
}
// ψ(x) = d log Γ(x)/dx for x > 0 in double: the recurrence ψ(x) = ψ(x + 1) − 1/x up to x ≥ 6, then the asymptotic series through B₁₄ (its first omitted
// term, B₁₆/(16 x¹⁶), is below 2e-13 there).  NaN for x ≤ 0: no fold takes log Γ there.
inline double digamma(double x) {
    if (!(x > 0.0)) return std::nan("");
    double s = 0.0;
    while (x < 6.0) {
        s -= 1.0 / x;
        x += 1.0;
    }
    const double f = 1.0 / (x * x);
    const double series = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
    return s + std::log(x) - 0.5 / x - series;
}
inline ParamTan lgamma(ParamTan x) { return {std::lgamma(x.v), digamma(x.v) * x.d}; }
// Γ(x) with Γ·ψ(x)·ẋ (the Chen-2022 large-ice fold add_sedimentation_consts_from, cmx_mp1m_vel.hpp: Γ(C_l + 4), Γ(F_l + 4)); an argument that does not
// move carries the literal zero, so ψ's NaN at x ≤ 0 stays out of a direction that does not touch it
inline ParamTan tgamma(ParamTan x) {
    const double g = std::tgamma(x.v);
    return {g, x.d == 0.0 ? 0.0 : g * digamma(x.v) * x.d};
}
inline ParamTan exp2(ParamTan x) {
    const double e = std::exp2(x.v);
    return {e, 0.69314718055994530942 * e * x.d};
}
inline ParamTan fmax(ParamTan a, ParamTan b) { return (b.v > a.v || a.v != a.v) ? ParamTan{std::fmax(a.v, b.v), b.d} : ParamTan{std::fmax(a.v, b.v), a.d}; }

// every floating member of a parameter struct or of a direction is finite (the structs hold nothing else)
template <typename FT, typename S> inline bool all_finite(const S &s) {
    static_assert(sizeof(S) % sizeof(FT) == 0, "a parameter struct is an aggregate of one float type");
    const FT *p = reinterpret_cast<const FT *>(&s);
    for (size_t i = 0; i < sizeof(S) / sizeof(FT); ++i)
        if (!(p[i] - p[i] == FT(0))) return false;
    return true;
}

template <typename S> struct ParamReader {
    const S &params;
    const S *direction;      // NULL: a zero direction
    template <typename F> ParamTan operator()(const F &field) const {
        const ptrdiff_t off = reinterpret_cast<const char *>(&field) - reinterpret_cast<const char *>(&params);
        return {(double)field, direction ? (double)*reinterpret_cast<const F *>(reinterpret_cast<const char *>(direction) + off) : 0.0};
    }
};
// CT<ParamTan> → slot k of CT<Dual<FT, KP>>, member by member: both are aggregates of their scalar type with the same members
template <int KP, typename FT, template <typename> class CT> inline void pack_param_consts(const CT<ParamTan> &src, int k, CT<Dual<FT, KP>> &dst) {
    constexpr size_t N = sizeof(CT<ParamTan>) / sizeof(ParamTan);
    static_assert(sizeof(CT<ParamTan>) == N * sizeof(ParamTan) && sizeof(CT<Dual<FT, KP>>) == N * sizeof(Dual<FT, KP>), "constants structs hold scalars only");
    const ParamTan *s = reinterpret_cast<const ParamTan *>(&src);
    Dual<FT, KP> *d = reinterpret_cast<Dual<FT, KP> *>(&dst);
    for (size_t m = 0; m < N; ++m) {
        d[m].v = (FT)s[m].v;
        d[m].d[k] = (FT)s[m].d;
    }
}

// the same for a constants struct with a header in front of its scalars (Mp1mConsts: the flags word): the members from `first` on
template <int KP, typename FT, typename SRC, typename DST>
inline void pack_param_members(const SRC &src, const ParamTan *first_src, int k, DST &dst, Dual<FT, KP> *first_dst) {
    const size_t N = (size_t)(reinterpret_cast<const char *>(&src + 1) - reinterpret_cast<const char *>(first_src)) / sizeof(ParamTan);
    for (size_t m = 0; m < N; ++m) {
        first_dst[m].v = (FT)first_src[m].v;
        first_dst[m].d[k] = (FT)first_src[m].d;
    }
}

}  // namespace cmx
