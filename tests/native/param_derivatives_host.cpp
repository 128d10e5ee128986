// param_derivatives_host.cpp — TEST INFRASTRUCTURE: the host build of the parameter derivatives (include/cmx.h §(22)).  What the device entries run, compiled by
// g++ (CMX_HOST_BUILD): the host fold of the constants with their tangents (csrc/cmx_param_tangent.hpp, make_sb_param_consts, make_mp1m_param_consts) and the point body
// param_jvp_point / param_vjp_point of csrc/cmx_jacobian.hpp on SbJac and Mp1mJac, set up by the functions the device entries call (with_sb2006_param,
// with_mp1m_param).  Checked in
// tests/test_param_derivatives_host.py against central differences of the plain fold and of the Float64 oracle.  Like tests/native/derivatives_host.cpp it is
// NOT part of libcmx.so and no CPU fallback.  With -DCMX_PARAM_HOST_MAIN it has a main() of its own (a stand-alone run, e.g. under a sanitizer).
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_jacobian.hpp"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_jacobian.hpp"

namespace {
using namespace cmx;

// kp directions per evaluation (1, 2, 4; 0: the device kernel's own); returns 1 if the integer-exponent instantiation ran, 0 for the general one, or a status.
// jvp: ndir·4 NULL-able columns, tend: NULL or 4 NULL-able columns
template <typename FT, typename WR, typename TH>
int32_t sb2006_param_jvp(const WR *wr, const TH *tps, uint32_t flags, int kp, int64_t n, const FT *const *x, int32_t ndir, const WR *d_wr, const TH *d_tps,
                         FT *const *jvp, FT *const *tend) {
    if (!wr || !tps || !jvp) return CMX_ERR_BAD_ARG;
    return with_sb2006_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) {
        using SJ = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
            constexpr int KP = decltype(K)::value;
            for (int d0 = 0; d0 < ndir; d0 += KP) {
                const auto cd = make_sb_param_consts<FT, KP>(*wr, *tps, d_wr, d_tps, d0, ndir);
                ParamJvpArgs<FT, KP, SJ::NOUT, SJ::NWRT> a{};
                for (int j = 0; j < SJ::NWRT + 1; ++j) a.in[j] = x[j];
                for (int q = 0; q < SJ::NOUT; ++q) a.tend[q] = d0 == 0 && tend ? tend[q] : nullptr;
                for (int k = 0; k < KP && d0 + k < ndir; ++k)
                    for (int q = 0; q < SJ::NOUT; ++q) a.jvp[k][q] = jvp[(d0 + k) * SJ::NOUT + q];
                for (int64_t i = 0; i < n; ++i) {
                    FT xi[SJ::NWRT + 1];
                    for (int j = 0; j < SJ::NWRT + 1; ++j) xi[j] = x[j][i];
                    param_jvp_point<SJ, FT, KP>(cd, a, xi, i);
                }
            }
            return (int32_t)std::is_same<SJ, SbJac<true, true>>::value | (int32_t)std::is_same<SJ, SbJac<false, true>>::value;
        }, one_of<1, 2, 4>(kp ? kp : kParamK<FT>));
    });
}

// grad[d] in the decomposition of the device reduction (param_vjp_chunk with 256 lanes per workgroup): per lane in index order, the 64 lanes of a wave in
// the shuffle tree, the four waves left to right, four partials per lane of the finish, the same tree
inline double tree256(const double *lane) {
    double part[4];
    for (int w = 0; w < 4; ++w) {
        double t[128] = {};
        for (int l = 0; l < 64; ++l) t[l] = lane[64 * w + l];
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < 64; ++l) t[l] = t[l] + t[l + off];      // lanes past 63 read as their own value on the device; lane 0's sum never uses them
        part[w] = t[0];
    }
    double s = 0.0;
    for (int w = 0; w < 4; ++w) s += part[w];
    return s;
}
template <typename FT, typename WR, typename TH>
int32_t sb2006_param_vjp(const WR *wr, const TH *tps, uint32_t flags, int64_t n, const FT *const *x, const FT *const *cot, int32_t ndir, const WR *d_wr,
                         const TH *d_tps, double *grad, FT *const *tend) {
    if (!wr || !tps || !cot || !grad) return CMX_ERR_BAD_ARG;
    return with_sb2006_param<FT>(*wr, *tps, flags, ndir, d_wr, d_tps, [&](auto S) {
        using SJ = decltype(S);
        constexpr int BS = 256;
        const int64_t chunk = param_vjp_chunk(n, BS);
        for (int d = 0; d < ndir; ++d) {
            const auto cd = make_sb_param_consts<FT, 1>(*wr, *tps, d_wr, d_tps, d, ndir);
            ParamVjpArgs<FT, SJ::NOUT, SJ::NWRT> a{};
            for (int j = 0; j < SJ::NWRT + 1; ++j) a.in[j] = x[j];
            for (int q = 0; q < SJ::NOUT; ++q) {
                a.cot[q] = cot[q];
                a.ncot += cot[q] != nullptr;
                a.tend[q] = d == 0 && tend ? tend[q] : nullptr;
            }
            std::vector<double> ws(CMX_PARAM_VJP_PARTIALS);
            for (int64_t b = 0; b < CMX_PARAM_VJP_PARTIALS; ++b) {
                double lane[BS];
                const int64_t lo = b * chunk, hi = lo + chunk < n ? lo + chunk : n;
                for (int t = 0; t < BS; ++t) {
                    double acc[1] = {0.0};
                    for (int64_t i = lo + t; i < hi; i += BS) {
                        FT xi[SJ::NWRT + 1];
                        for (int j = 0; j < SJ::NWRT + 1; ++j) xi[j] = x[j][i];
                        param_vjp_point<SJ, FT, 1>(cd, a, xi, i, acc);
                    }
                    lane[t] = acc[0];
                }
                ws[b] = tree256(lane);
            }
            double lane[BS];
            for (int t = 0; t < BS; ++t) lane[t] = ((ws[4 * t] + ws[4 * t + 1]) + ws[4 * t + 2]) + ws[4 * t + 3];
            grad[d] = tree256(lane);
        }
        return (int32_t)CMX_OK;
    });
}

// the folded constants as doubles: out[m] = member m of make_sb_consts<double> (plain), val[m] / tan[m] = the ParamTan fold along one direction.  Returns the
// number of members.
int32_t sb2006_consts(const cmx_warm_rain_2m_f64 *wr, const cmx_thermo_f64 *tps, const cmx_warm_rain_2m_f64 *d_wr, const cmx_thermo_f64 *d_tps, double *out,
                      double *val, double *tan) {
    constexpr int N = sizeof(SbConsts<double>) / sizeof(double);
    static_assert(sizeof(SbConsts<ParamTan>) == N * sizeof(ParamTan), "the same members");
    const SbConsts<double> c = make_sb_consts<double>(*wr, *tps, (const cmx_rain_vel_f64 *)nullptr, (double)Math<double>::eps_1m());
    const SbConsts<ParamTan> ct = make_sb_consts_from<double, ParamTan>(*wr, *tps, (const cmx_rain_vel_f64 *)nullptr, (double)Math<double>::eps_1m(),
                                                                        ParamReader<cmx_warm_rain_2m_f64>{*wr, d_wr}, ParamReader<cmx_thermo_f64>{*tps, d_tps});
    for (int m = 0; m < N; ++m) {
        if (out) out[m] = reinterpret_cast<const double *>(&c)[m];
        if (val) val[m] = reinterpret_cast<const ParamTan *>(&ct)[m].v;
        if (tan) tan[m] = reinterpret_cast<const ParamTan *>(&ct)[m].d;
    }
    return N;
}
// ---- 1-moment: returns 1 if the default-options / default-exponents instantiation ran, 0 for the run-time-flags one, or a status -------------------------
template <typename FT, typename MP, typename TH>
int32_t mp1m_param_jvp(const MP *mp, const TH *tps, uint32_t flags, int kp, int64_t n, const FT *const *x, int32_t ndir, const MP *d_mp, const TH *d_tps,
                       FT *const *jvp, FT *const *tend) {
    if (!mp || !tps || !jvp) return CMX_ERR_BAD_ARG;
    if (const int32_t st = check_flags_1m(flags)) return st;
    return with_mp1m_param<FT>(*mp, *tps, flags, ndir, d_mp, d_tps, [&](auto S) {
        using SJ = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto K) -> int32_t {
            constexpr int KP = decltype(K)::value;
            for (int d0 = 0; d0 < ndir; d0 += KP) {
                const auto cd = make_mp1m_param_consts<FT, KP>(*mp, *tps, flags, d_mp, d_tps, d0, ndir);
                ParamJvpArgs<FT, KP, SJ::NOUT, SJ::NWRT> a{};
                for (int j = 0; j < SJ::NWRT + 1; ++j) a.in[j] = x[j];
                for (int q = 0; q < SJ::NOUT; ++q) a.tend[q] = d0 == 0 && tend ? tend[q] : nullptr;
                for (int k = 0; k < KP && d0 + k < ndir; ++k)
                    for (int q = 0; q < SJ::NOUT; ++q) a.jvp[k][q] = jvp[(d0 + k) * SJ::NOUT + q];
                for (int64_t i = 0; i < n; ++i) {
                    FT xi[SJ::NWRT + 1];
                    for (int j = 0; j < SJ::NWRT + 1; ++j) xi[j] = x[j][i];
                    param_jvp_point<SJ, FT, KP>(cd, a, xi, i);
                }
            }
            return (int32_t)std::is_same<SJ, Mp1mJac<kDefaultFlags>>::value;
        }, one_of<1, 2, 4>(kp ? kp : kParamK<FT>));
    });
}

// the folded 1-moment constants as doubles (the members after the flags word): plain fold, and value / tangent of the ParamTan fold along one direction
int32_t mp1m_consts(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, const cmx_microphysics_1m_f64 *d_mp, const cmx_thermo_f64 *d_tps,
                    double *out, double *val, double *tan) {
    const Mp1mConsts<double> c = make_mp1m_consts<double>(*mp, *tps, flags, (double)Math<double>::eps_1m());
    const Mp1mConsts<ParamTan> ct = make_mp1m_tangent_consts<double>(*mp, *tps, flags, d_mp, d_tps);
    const int N = (int)((reinterpret_cast<const char *>(&c + 1) - reinterpret_cast<const char *>(&c.eps_1m)) / sizeof(double));
    for (int m = 0; m < N; ++m) {
        if (out) out[m] = (&c.eps_1m)[m];
        if (val) val[m] = (&ct.eps_1m)[m].v;
        if (tan) tan[m] = (&ct.eps_1m)[m].d;
    }
    return N;
}
}  // namespace

#define CMX_HOST_PARAM_DERIVATIVES(SFX, FT)                                                                                                                    \
    int32_t host_sb2006_param_jvp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int kp, int64_t n, const FT *const *x,   \
                                        int32_t ndir, const cmx_warm_rain_2m_##SFX *d_wr, const cmx_thermo_##SFX *d_tps, FT *const *jvp, FT *const *tend) {     \
        return sb2006_param_jvp<FT>(wr, tps, flags, kp, n, x, ndir, d_wr, d_tps, jvp, tend);                                                                    \
    }                                                                                                                                                          \
    int32_t host_sb2006_param_vjp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, uint32_t flags, int64_t n, const FT *const *x,           \
                                        const FT *const *cot, int32_t ndir, const cmx_warm_rain_2m_##SFX *d_wr, const cmx_thermo_##SFX *d_tps, double *grad,    \
                                        FT *const *tend) {                                                                                                     \
        return sb2006_param_vjp<FT>(wr, tps, flags, n, x, cot, ndir, d_wr, d_tps, grad, tend);                                                                  \
    }                                                                                                                                                          \
    int32_t host_mp1m_param_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, uint32_t flags, int kp, int64_t n, const FT *const *x,  \
                                      int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp, const cmx_thermo_##SFX *d_tps, FT *const *jvp, FT *const *tend) {    \
        return mp1m_param_jvp<FT>(mp, tps, flags, kp, n, x, ndir, d_mp, d_tps, jvp, tend);                                                                      \
    }

extern "C" {
int32_t host_param_k_f32(void) { return kParamK<float>; }
int32_t host_param_k_f64(void) { return kParamK<double>; }
int32_t host_sb2006_consts_f64(const cmx_warm_rain_2m_f64 *wr, const cmx_thermo_f64 *tps, const cmx_warm_rain_2m_f64 *d_wr, const cmx_thermo_f64 *d_tps,
                               double *out, double *val, double *tan) {
    return sb2006_consts(wr, tps, d_wr, d_tps, out, val, tan);
}
int32_t host_mp1m_consts_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, const cmx_microphysics_1m_f64 *d_mp,
                             const cmx_thermo_f64 *d_tps, double *out, double *val, double *tan) {
    return mp1m_consts(mp, tps, flags, d_mp, d_tps, out, val, tan);
}
CMX_HOST_PARAM_DERIVATIVES(f32, float)
CMX_HOST_PARAM_DERIVATIVES(f64, double)
}

#if defined(CMX_PARAM_HOST_MAIN)
// A stand-alone run of the fold and of both point bodies on a handful of states with zero-initialised parameter structs filled by hand: every array the
// harness indexes is touched, for a sanitizer build (-fsanitize=address,undefined).  It checks no value.
int main() {
    cmx_warm_rain_2m_f64 wr{}, d[3] = {};
    cmx_thermo_f64 tps{};
    double *w = reinterpret_cast<double *>(&wr), *t = reinterpret_cast<double *>(&tps);
    for (size_t m = 0; m < sizeof(wr) / sizeof(double); ++m) w[m] = 1.0 + 0.01 * m;
    for (size_t m = 0; m < sizeof(tps) / sizeof(double); ++m) t[m] = 300.0 + m;
    d[0].seifert_beheng.acnv.kcc = 1.0;
    d[1].seifert_beheng.accr.c = 1.0;
    d[2].condevap_tau_relax = 1.0;
    const int n = 1000;
    std::vector<double> col[7], out[12], tend[4], cot[4];
    const double *x[7], *g[4];
    double *jvp[12], *td[4], grad[3];
    for (int j = 0; j < 7; ++j) { col[j].assign(n, j == 1 ? 285.0 : 1e-3 * (j + 1)); x[j] = col[j].data(); }
    for (int q = 0; q < 12; ++q) { out[q].assign(n, 0.0); jvp[q] = out[q].data(); }
    for (int q = 0; q < 4; ++q) { tend[q].assign(n, 0.0); td[q] = tend[q].data(); cot[q].assign(n, 1.0); g[q] = cot[q].data(); }
    int32_t st = 0;
    for (int kp : {1, 2, 4}) st |= host_sb2006_param_jvp_f64(&wr, &tps, 0, kp, n, x, 3, d, nullptr, jvp, td) < 0;
    st |= host_sb2006_param_vjp_f64(&wr, &tps, 0, n, x, g, 3, d, nullptr, grad, td) < 0;
    std::printf("param_derivatives_host: %s (grad %g %g %g)\n", st ? "a call failed" : "ok", grad[0], grad[1], grad[2]);
    return st;
}
#endif
