// column_param_host.cpp — TEST INFRASTRUCTURE: the host build of the derivatives of the SB2006 column step with respect to the PARAMETERS (include/cmx.h §(26)).
// The bodies of one point and the host folds with tangents (csrc/cmx_sb2006_column_param.hpp, cmx_sb2006.hpp, cmx_param_tangent.hpp) compiled by g++ for the
// HOST (CMX_HOST_BUILD: libm stand-ins for the hardware transcendental instructions) and run over columns by plain loops, set up by the functions the device
// entries call (with_sb2006_column_param, make_column_param_consts), so that the mathematics — the fall-speed constants with tangents, ψ, the coupling of a
// level with the one above, λ — is tested against central differences of the Float64 oracle without a GPU (tests/test_column_param_host.py).
// NOT part of libcmx.so and no CPU fallback.
//
// With -DCMX_COLUMN_PARAM_MAIN it is a stand-alone program (its own main: a few columns through both entries, the gradient checked against the sum over the
// jvp columns) — the one to build with host sanitizer flags.
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_column_param.hpp"

namespace {
using namespace cmx;
constexpr int NW = CMX_SB2006_JAC_NWRT, NO = CMX_SB2006_JAC_NOUT;

// Both functions return the statuses of the device entries — the parameter structs, the entry's status function (the ladder of column_entry_status with its
// columns), then with_sb2006_column_param — or what ran.

// J_θ δθ: the levels of a column from the top down.  kp: directions per evaluation (0: the device kernel's choice); the split into launches is the device
// entry's.  Returns the velocity kind that ran.
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t jvp(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,
            int32_t ndir, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cv, FT *const *jv, FT *const *jv_precip, FT *const *tend, FT *precip) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_param_jvp_status(flags, n_col, n_lev, inv_dz, x, ndir, d_wr, jv, jv_precip, tend, precip); st != kColumnEntryRun) return st;
    return with_sb2006_column_param<FT>(*wr, *tps, *vel, cloud_vel, flags, ndir, d_wr, d_tps, d_vel, d_cv, [&](auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int KW = decltype(KT)::value;
            const FT *in[NW + 1];
            for (int j = 0; j < NW + 1; ++j) in[j] = x[j];
            for_each_column_param_launch<KW>(ndir, [&](auto K, int d0) {
                constexpr int KP = decltype(K)::value;
                SbConsts<Dual<FT, KP>> cd;
                CloudVelConsts<Dual<FT, KP>> cvd;
                make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cv, d0, ndir, cd, cvd);
                ColParamJvpArgs<FT, KP> a;
                if (!make_column_param_jvp_args(a, in, inv_dz, n_col * n_lev, n_lev, d0, ndir, jv, jv_precip, tend, precip)) return;
                for (int64_t col = 0; col < n_col; ++col) {
                    FT upv[4] = {}, upd[KP][4] = {};
                    for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                        const int64_t i = col * n_lev + lev;
                        FT xi[NW + 1];
                        for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                        ColParamPoint<FT, KP> p;
                        column_param_eval<SC, FT, KP>(cd, cvd, xi, inv_dz[lev], p);
                        column_param_jvp_store<SC, FT, KP>(a, p, upv, upd, lev == n_lev - 1, lev == 0, i, col);
                        for (int s = 0; s < 4; ++s) {
                            upv[s] = p.Fv[s];
                            for (int k = 0; k < KP; ++k) upd[k][s] = p.Fd[k][s];
                        }
                    }
                }
            });
            return SC::vel;
        }, one_of<1, 2, 3, 4>(kp ? kp : kColParamK<FT, SC::vel>));
    });
}

// The gradient: pointwise, the points in index order into ONE accumulator per direction (the device's decomposition is the reduction's, tested on the device)
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t vjp(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,
            const FT *const *cot, const FT *cot_precip, int32_t ndir, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cv, double *grad, FT *const *tend,
            FT *precip) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    // (the mirror reduces in place and has no workspace: grad stands in for it)
    if (const int32_t st = sb2006_column_param_vjp_status(flags, n_col, n_lev, inv_dz, x, cot, cot_precip, ndir, d_wr, grad, grad, tend, precip); st != kColumnEntryRun)
        return st;
    return with_sb2006_column_param<FT>(*wr, *tps, *vel, cloud_vel, flags, ndir, d_wr, d_tps, d_vel, d_cv, [&](auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int KW = decltype(KT)::value;
            const FT *in[NW + 1];
            for (int j = 0; j < NW + 1; ++j) in[j] = n_col ? x[j] : nullptr;
            for_each_column_param_launch<KW>(ndir, [&](auto K, int d0) {
                constexpr int KP = decltype(K)::value;
                SbConsts<Dual<FT, KP>> cd;
                CloudVelConsts<Dual<FT, KP>> cvd;
                make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cv, d0, ndir, cd, cvd);
                ColParamVjpArgs<FT> a;
                make_column_param_vjp_args<SC>(a, in, inv_dz, n_col * n_lev, n_lev, cot, cot_precip, d0 == 0, tend, precip);
                double acc[KP] = {};
                for (int64_t col = 0; col < n_col; ++col)
                    for (int32_t lev = 0; lev < n_lev; ++lev) {
                        const int64_t i = col * n_lev + lev;
                        FT xi[NW + 1];
                        for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                        column_param_vjp_point<SC, FT, KP>(cd, cvd, a, xi, i, col, lev, acc);
                    }
                for (int k = 0; k < KP && d0 + k < ndir; ++k) grad[d0 + k] = acc[k];
            });
            return SC::vel;
        }, one_of<1, 2, 3, 4>(kp ? kp : kColParamK<FT, SC::vel>));
    });
}

// the folded constants of ONE direction as doubles, value parts then tangents: SbConsts then CloudVelConsts (zeros without cloud_vel).  Returns the count
// of scalars per part, or the count alone when out is NULL.
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t consts(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cv, double *out) {
    constexpr int NS = sizeof(SbConsts<ParamTan>) / sizeof(ParamTan), NC = sizeof(CloudVelConsts<ParamTan>) / sizeof(ParamTan);
    if (!out) return NS + NC;
    const ParamReader<WR> P{*wr, d_wr};
    const SbConsts<ParamTan> ct = make_sb_consts_from<FT, ParamTan>(*wr, *tps, vel, (double)Math<FT>::eps_1m(), P, ParamReader<TH>{*tps, d_tps}, ParamReader<VL>{*vel, d_vel});
    CloudVelConsts<ParamTan> cvt{};
    if (cloud_vel) cvt = make_cloud_vel_consts_from<FT, ParamTan>(wr->seifert_beheng.pdf_c, *cloud_vel, P, ParamReader<ST>{*cloud_vel, d_cv});
    const ParamTan *a = reinterpret_cast<const ParamTan *>(&ct), *b = reinterpret_cast<const ParamTan *>(&cvt);
    for (int m = 0; m < NS; ++m) { out[m] = a[m].v; out[NS + NC + m] = a[m].d; }
    for (int m = 0; m < NC; ++m) { out[NS + m] = b[m].v; out[NS + NC + NS + m] = b[m].d; }
    return NS + NC;
}
// the PLAIN fold's constants, as the bytes of SbConsts<FT> then CloudVelConsts<FT>; returns the byte count (out NULL: the count alone).  packed: the value
// parts of the fold with tangents, rounded as pack_param_consts rounds them — member by member of the same structs, except that ChenLog holds the
// Float64 degree there (cmx_math.hpp), so the fitted coefficients are compared through their own members.
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t plain_consts(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, bool packed, unsigned char *out) {
    const int32_t bytes = (int32_t)(sizeof(SbConsts<FT>) + sizeof(CloudVelConsts<FT>));
    if (!out) return bytes;
    SbConsts<FT> c{};
    CloudVelConsts<FT> cv{};
    if (!packed) {
        c = make_sb_consts<FT>(*wr, *tps, vel, (double)Math<FT>::eps_1m());
        if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr->seifert_beheng.pdf_c, *cloud_vel);
    } else {
        SbConsts<Dual<FT, 1>> cd;
        CloudVelConsts<Dual<FT, 1>> cvd;
        make_column_param_consts<FT, 1>(*wr, *tps, *vel, cloud_vel, (const WR *)nullptr, (const TH *)nullptr, (const VL *)nullptr, (const ST *)nullptr, 0, 0, cd, cvd);
        // every scalar in front of chl has the same position in both structs
        const size_t nfront = offsetof(SbConsts<FT>, chl) / sizeof(FT);
        const Dual<FT, 1> *s = reinterpret_cast<const Dual<FT, 1> *>(&cd);
        FT *d = reinterpret_cast<FT *>(&c);
        for (size_t m = 0; m < nfront; ++m) d[m] = s[m].v;
        for (int i = 0; i < 3; ++i) {
            for (int kk = 0; kk < 2; ++kk)
                for (int m = 0; m <= ChenLog<FT>::D; ++m) c.chl.c[kk][i][m] = cd.chl.c[kk][i][m].v;
            c.chl.sgn[i] = cd.chl.sgn[i].v;
            c.chl.b1[i] = cd.chl.b1[i].v;
            c.chl.b4[i] = cd.chl.b4[i].v;
        }
        cv.pre_c = cvd.pre_c.v; cv.rho_w = cvd.rho_w.v; cv.K23 = cvd.K23.v; cv.K53 = cvd.K53.v;
    }
    std::memcpy(out, &c, sizeof c);
    std::memcpy(out + sizeof c, &cv, sizeof cv);
    return bytes;
}
}  // namespace

#define CMX_HOST_COLUMN_PARAM(SFX, FT)                                                                                                                                 \
    int32_t host_sb2006_column_param_jvp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                           \
                                               const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz,          \
                                               const FT *const *x, int32_t ndir, const cmx_warm_rain_2m_##SFX *d_wr, const cmx_thermo_##SFX *d_tps,                    \
                                               const cmx_rain_vel_##SFX *d_vel, const cmx_stokes_vel_##SFX *d_cv, FT *const *jv, FT *const *jv_precip,                 \
                                               FT *const *tend, FT *precip) {                                                                                          \
        return jvp<FT>(wr, tps, vel, cloud_vel, flags, kp, n_col, n_lev, inv_dz, x, ndir, d_wr, d_tps, d_vel, d_cv, jv, jv_precip, tend, precip);                      \
    }                                                                                                                                                                  \
    int32_t host_sb2006_column_param_vjp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                           \
                                               const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz,          \
                                               const FT *const *x, const FT *const *cot, const FT *cot_precip, int32_t ndir, const cmx_warm_rain_2m_##SFX *d_wr,       \
                                               const cmx_thermo_##SFX *d_tps, const cmx_rain_vel_##SFX *d_vel, const cmx_stokes_vel_##SFX *d_cv, double *grad,         \
                                               FT *const *tend, FT *precip) {                                                                                          \
        return vjp<FT>(wr, tps, vel, cloud_vel, flags, kp, n_col, n_lev, inv_dz, x, cot, cot_precip, ndir, d_wr, d_tps, d_vel, d_cv, grad, tend, precip);              \
    }                                                                                                                                                                  \
    int32_t host_column_param_consts_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                               \
                                           const cmx_stokes_vel_##SFX *cloud_vel, const cmx_warm_rain_2m_##SFX *d_wr, const cmx_thermo_##SFX *d_tps,                   \
                                           const cmx_rain_vel_##SFX *d_vel, const cmx_stokes_vel_##SFX *d_cv, double *out) {                                           \
        return consts<FT>(wr, tps, vel, cloud_vel, d_wr, d_tps, d_vel, d_cv, out);                                                                                     \
    }                                                                                                                                                                  \
    int32_t host_column_plain_consts_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                               \
                                           const cmx_stokes_vel_##SFX *cloud_vel, int packed, unsigned char *out) {                                                    \
        return plain_consts<FT>(wr, tps, vel, cloud_vel, packed != 0, out);                                                                                            \
    }

extern "C" {
int32_t host_column_param_k_f32(int vel) { return vel == VEL_CHEN_GEN ? kColParamK<float, VEL_CHEN_GEN> : kColParamK<float, VEL_SB>; }
int32_t host_column_param_k_f64(int vel) { return vel == VEL_CHEN_GEN ? kColParamK<double, VEL_CHEN_GEN> : kColParamK<double, VEL_SB>; }
double host_digamma(double x) { return cmx::digamma(x); }
CMX_HOST_COLUMN_PARAM(f32, float)
CMX_HOST_COLUMN_PARAM(f64, double)
}

#if defined(CMX_COLUMN_PARAM_MAIN)
#include <cmath>
#include <cstdio>
#include <vector>

// The parameter structs come from a file the Python side writes (tests/test_column_param_host.py: the raw bytes of cmx_warm_rain_2m, cmx_thermo, cmx_rain_vel
// and cmx_stokes_vel of one float type, in this order); the columns and the directions (each parameter field times a pseudo-random factor) are made here.
// Checks grad[d] = Σ ḡ·jvp_d + Σ p̄·ṗ_d and exits 0.
template <typename FT, typename WR, typename TH, typename VL, typename ST> static int self_check(const char *path, uint32_t flags, bool cloud) {
    WR wr; TH tps; VL vel; ST st;
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    const bool ok = std::fread(&wr, sizeof wr, 1, f) == 1 && std::fread(&tps, sizeof tps, 1, f) == 1 && std::fread(&vel, sizeof vel, 1, f) == 1 &&
                    std::fread(&st, sizeof st, 1, f) == 1;
    std::fclose(f);
    if (!ok) return 2;
    const int64_t n_col = 5;
    const int32_t n_lev = 7, ndir = 5;
    const int64_t n = n_col * n_lev;
    std::vector<std::vector<FT>> x(NW + 1, std::vector<FT>(n)), gb(NO, std::vector<FT>(n)), tend(NO, std::vector<FT>(n)), jv(ndir * NO, std::vector<FT>(n)),
        jp(ndir, std::vector<FT>(n_col));
    std::vector<FT> inv_dz(n_lev), pb(n_col), precip(n_col);
    uint32_t seed = 12345u;
    auto u = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / 16777216.0; };
    for (int32_t k = 0; k < n_lev; ++k) inv_dz[k] = (FT)(1.0 / (50.0 + 30.0 * k));
    for (int64_t i = 0; i < n; ++i) {
        x[0][i] = (FT)(0.7 + 0.5 * u());
        x[1][i] = (FT)(278.0 + 15.0 * u());
        x[3][i] = (FT)(1e-4 + 1e-3 * u());
        x[5][i] = (FT)(1e-5 + 1e-3 * u());
        x[4][i] = (FT)(x[3][i] / 1e-11);
        x[6][i] = (FT)(x[5][i] / 1e-8);
        x[2][i] = (FT)(x[3][i] + x[5][i] + 6e-3);
        for (int q = 0; q < NO; ++q) gb[q][i] = (FT)(u() - 0.5);
    }
    for (int64_t c = 0; c < n_col; ++c) pb[c] = (FT)(u() - 0.5);
    // directions: every field of the structs (the Chen-2022 table and the exponents excepted) times a factor in ±1e-2
    std::vector<WR> d_wr(ndir); std::vector<TH> d_tps(ndir); std::vector<VL> d_vel(ndir); std::vector<ST> d_st(ndir);
    auto scaled = [&](auto &dst, const auto &src) {
        FT *d = reinterpret_cast<FT *>(&dst);
        const FT *s = reinterpret_cast<const FT *>(&src);
        for (size_t m = 0; m < sizeof(src) / sizeof(FT); ++m) d[m] = (FT)(s[m] * 2e-2 * (u() - 0.5));
    };
    for (int d = 0; d < ndir; ++d) {
        scaled(d_wr[d], wr); scaled(d_tps[d], tps); scaled(d_vel[d], vel); scaled(d_st[d], st);
        std::memset(&d_vel[d].chen2022, 0, sizeof d_vel[d].chen2022);
        d_wr[d].seifert_beheng.acnv.b = d_wr[d].seifert_beheng.accr.c = d_wr[d].seifert_beheng.self.d = 0;
    }
    const FT *xp[NW + 1], *gp[NO];
    FT *to[NO];
    std::vector<FT *> jo(ndir * NO), po(ndir);
    for (int j = 0; j < NW + 1; ++j) xp[j] = x[j].data();
    for (int q = 0; q < NO; ++q) { gp[q] = gb[q].data(); to[q] = tend[q].data(); }
    for (int q = 0; q < ndir * NO; ++q) jo[q] = jv[q].data();
    for (int d = 0; d < ndir; ++d) po[d] = jp[d].data();
    const ST *cv = cloud ? &st : nullptr;
    if (jvp<FT>(&wr, &tps, &vel, cv, flags, 0, n_col, n_lev, inv_dz.data(), xp, ndir, d_wr.data(), d_tps.data(), d_vel.data(), d_st.data(), jo.data(), po.data(), to,
                precip.data()) < 0)
        return 3;
    std::vector<double> grad(ndir);
    if (vjp<FT>(&wr, &tps, &vel, cv, flags, 0, n_col, n_lev, inv_dz.data(), xp, gp, pb.data(), ndir, d_wr.data(), d_tps.data(), d_vel.data(), d_st.data(), grad.data(),
                nullptr, nullptr) < 0)
        return 3;
    double worst = 0;
    for (int d = 0; d < ndir; ++d) {
        double sum = 0, scale = 0;
        for (int64_t i = 0; i < n; ++i)
            for (int q = 0; q < NO; ++q) { sum += (double)gb[q][i] * jv[d * NO + q][i]; scale += std::fabs((double)gb[q][i] * jv[d * NO + q][i]); }
        for (int64_t c = 0; c < n_col; ++c) { sum += (double)pb[c] * jp[d][c]; scale += std::fabs((double)pb[c] * jp[d][c]); }
        if (!(std::fabs(sum - grad[d]) <= (sizeof(FT) == 4 ? 1e-4 : 1e-12) * scale) || !(scale > 0)) return 4;
        worst = std::fmax(worst, std::fabs(sum - grad[d]) / scale);
    }
    std::printf("gradient against the jvp columns, %s flags %u cloud %d: worst %.3g of the terms' size\n", sizeof(FT) == 4 ? "f32" : "f64", flags, (int)cloud, worst);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    int rc = 0;
    for (uint32_t flags : {CMX_SB2006_LIMITED | CMX_VEL_SB2006, CMX_VEL_SB2006, CMX_SB2006_LIMITED | CMX_VEL_CHEN2022})
        for (bool cloud : {false, true}) {
            rc |= self_check<float, cmx_warm_rain_2m_f32, cmx_thermo_f32, cmx_rain_vel_f32, cmx_stokes_vel_f32>(argv[1], flags, cloud);
            rc |= self_check<double, cmx_warm_rain_2m_f64, cmx_thermo_f64, cmx_rain_vel_f64, cmx_stokes_vel_f64>(argv[2], flags, cloud);
        }
    return rc;
}
#endif
