// column_param_1m_host.cpp — TEST INFRASTRUCTURE: the host build of the derivatives of the 1-moment column step with respect to the PARAMETERS (include/cmx.h
// §(28)).  The bodies of one point and the host folds with tangents (csrc/cmx_mp1m_column_param.hpp, cmx_mp1m_vel.hpp, cmx_mp1m.hpp, cmx_param_tangent.hpp)
// compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the hardware transcendental instructions) and run over columns by plain loops, set up by
// the functions the device entries call (with_mp1m_column_param, make_col1m_param_consts), so that the mathematics — the fall-speed constants with tangents,
// Γ·ψ, the coupling of a level with the one above, λ — is tested against central differences of the Float64 oracle without a GPU
// (tests/test_column_param_1m_host.py).  NOT part of libcmx.so and no CPU fallback.
//
// With -DCMX_COLUMN_PARAM_1M_MAIN it is a stand-alone program (its own main: a few columns through both entries, the gradient checked against the sum over
// the jvp columns) — the one to build with host sanitizer flags.
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_column_param.hpp"

namespace {
using namespace cmx;
constexpr int NW = CMX_MP1M_JAC_NWRT, NO = CMX_MP1M_JAC_NOUT;

// what ran: bit 0 the default-options instantiation, bit 1 the general Γ of the Chen-2022 rain table
template <typename S> constexpr int32_t kind_of() { return (S::flags == kDefaultFlags ? 1 : 0) | (S::general ? 2 : 0); }

// Both functions return the statuses of the device entries — the parameter structs, the entry's status function (the ladder of column_entry_status with its
// columns), then with_mp1m_column_param — or what ran.

// J_θ δθ: the levels of a column from the top down.  kp: directions per evaluation (0: the device kernel's choice); the split into launches is the device
// entry's.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t jvp(const MP *mp, const TH *tps, const ST *st, const CH *cr, const CI *ci, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz,
            const FT *const *x, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_st, const CH *d_cr, const CI *d_ci, FT *const *jv, FT *const *jpr,
            FT *const *jps, FT *const *tend, FT *pr, FT *ps) {
    if (!mp || !tps || !st || !cr || !ci) return CMX_ERR_BAD_ARG;
    if (const int32_t s = mp1m_column_param_jvp_status(flags, n_col, n_lev, inv_dz, x, ndir, d_mp, jv, jpr, jps, tend, pr, ps); s != kColumnEntryRun) return s;
    return with_mp1m_column_param<FT>(*mp, *tps, *st, *cr, *ci, flags, ndir, d_mp, d_tps, d_st, d_cr, d_ci, [&](auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int KW = decltype(KT)::value;
            const FT *in[NW + 1];
            for (int j = 0; j < NW + 1; ++j) in[j] = x[j];
            for_each_column_param_launch<KW>(ndir, [&](auto K, int d0) {
                constexpr int KP = decltype(K)::value;
                Col1mParamJvpArgs<FT, KP> a;
                if (!make_col1m_param_jvp_args(a, in, inv_dz, n_col * n_lev, n_lev, d0, ndir, jv, jpr, jps, tend, pr, ps)) return;
                Col1mParamConsts<FT, KP> c;
                make_col1m_param_consts<FT, KP>(*mp, *tps, *st, *cr, *ci, flags, d_mp, d_tps, d_st, d_cr, d_ci, d0, ndir, c);
                for (int64_t col = 0; col < n_col; ++col) {
                    FT upv[4] = {}, upd[KP][4] = {};
                    for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                        const int64_t i = col * n_lev + lev;
                        FT xi[NW + 1];
                        for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                        Col1mParamPoint<FT, KP> p;
                        column1m_param_eval<SC, FT, KP>(c, xi, inv_dz[lev], p);
                        column1m_param_jvp_store<SC, FT, KP>(a, p, upv, upd, lev == n_lev - 1, lev == 0, i, col);
                        for (int s = 0; s < 4; ++s) {
                            upv[s] = p.Fv[s];
                            for (int k = 0; k < KP; ++k) upd[k][s] = p.Fd[k][s];
                        }
                    }
                }
            });
            return kind_of<SC>();
        }, one_of<1, 2, 3, 4>(kp ? kp : kCol1mParamK<FT, SC::general>));
    });
}

// The gradient: pointwise, the points in index order into ONE accumulator per direction (the device's decomposition is the reduction's, tested on the device)
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t vjp(const MP *mp, const TH *tps, const ST *st, const CH *cr, const CI *ci, uint32_t flags, int kp, int64_t n_col, int32_t n_lev, const FT *inv_dz,
            const FT *const *x, const FT *const *cot, const FT *cpr, const FT *cps, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_st, const CH *d_cr,
            const CI *d_ci, double *grad, FT *const *tend, FT *pr, FT *ps) {
    if (!mp || !tps || !st || !cr || !ci) return CMX_ERR_BAD_ARG;
    // (the mirror reduces in place and has no workspace: grad stands in for it)
    if (const int32_t s = mp1m_column_param_vjp_status(flags, n_col, n_lev, inv_dz, x, cot, cpr, cps, ndir, d_mp, grad, grad, tend, pr, ps); s != kColumnEntryRun)
        return s;
    return with_mp1m_column_param<FT>(*mp, *tps, *st, *cr, *ci, flags, ndir, d_mp, d_tps, d_st, d_cr, d_ci, [&](auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int KW = decltype(KT)::value;
            const FT *in[NW + 1];
            for (int j = 0; j < NW + 1; ++j) in[j] = n_col ? x[j] : nullptr;
            for_each_column_param_launch<KW>(ndir, [&](auto K, int d0) {
                constexpr int KP = decltype(K)::value;
                Col1mParamConsts<FT, KP> c;
                make_col1m_param_consts<FT, KP>(*mp, *tps, *st, *cr, *ci, flags, d_mp, d_tps, d_st, d_cr, d_ci, d0, ndir, c);
                Col1mParamVjpArgs<FT> a;
                make_col1m_param_vjp_args(a, in, inv_dz, n_col * n_lev, n_lev, cot, cpr, cps, d0 == 0, tend, pr, ps);
                double acc[KP] = {};
                for (int64_t col = 0; col < n_col; ++col)
                    for (int32_t lev = 0; lev < n_lev; ++lev) {
                        const int64_t i = col * n_lev + lev;
                        FT xi[NW + 1];
                        for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                        column1m_param_vjp_point<SC, FT, KP>(c, a, xi, i, col, lev, acc);
                    }
                for (int k = 0; k < KP && d0 + k < ndir; ++k) grad[d0 + k] = acc[k];
            });
            return kind_of<SC>();
        }, one_of<1, 2, 3, 4>(kp ? kp : kCol1mParamK<FT, SC::general>));
    });
}

// ---- the folded constants ---------------------------------------------------------------------------------------------------------------------------
constexpr int NPT = (int)((sizeof(Mp1mConsts<ParamTan>) - offsetof(Mp1mConsts<ParamTan>, eps_1m)) / sizeof(ParamTan)), NVT = (int)(sizeof(Vel1mTanPart<ParamTan>) / sizeof(ParamTan));

// the folded constants of ONE direction as doubles, value parts then tangents: Mp1mConsts (from eps_1m on) then Vel1mTanPart.  Returns the count of scalars
// per part, or the count alone when out is NULL.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t consts(const MP *mp, const TH *tps, const ST *st, const CH *cr, const CI *ci, uint32_t flags, const MP *d_mp, const TH *d_tps, const ST *d_st, const CH *d_cr,
               const CI *d_ci, double *out) {
    if (!out) return NPT + NVT;
    Mp1mConsts<ParamTan> ct;
    Vel1mTanConsts<ParamTan, FT> vt;
    make_col1m_tangent_consts<FT>(*mp, *tps, *st, *cr, *ci, flags, d_mp, d_tps, d_st, d_cr, d_ci, ct, vt);
    const ParamTan *a = &ct.eps_1m, *b = reinterpret_cast<const ParamTan *>(static_cast<const Vel1mTanPart<ParamTan> *>(&vt));
    for (int m = 0; m < NPT; ++m) { out[m] = a[m].v; out[NPT + NVT + m] = a[m].d; }
    for (int m = 0; m < NVT; ++m) { out[NPT + m] = b[m].v; out[NPT + NVT + NPT + m] = b[m].d; }
    return NPT + NVT;
}

inline double value_of(double x) { return x; }
template <typename FT, int K> inline double value_of(const Dual<FT, K> &x) { return (double)x.v; }
// the fall-speed constants by NAME, in the order of Vel1mTanPart and then of the plain tail of Vel1mTanConsts, from either struct
template <typename FT, typename VC> void vel_values(const VC &c, FT *out) {
    int m = 0;
    auto put = [&](const auto &v) { out[m++] = (FT)value_of(v); };
    put(c.lam_a_rai); put(c.lam_b_rai); put(c.lam_floor_rai); put(c.lam_a_sno); put(c.lam_b_sno); put(c.lam_floor_sno); put(c.sno_l2_mu); put(c.sno_nu);
    put(c.ch_rho0_l2e); for (int k = 0; k < 3; ++k) put(c.ch_a[k]);
    put(c.ch_a3_pow); for (int k = 0; k < 3; ++k) put(c.ch_c1000[k]);
    put(c.st_pref); put(c.st_rho_w); put(c.st_D3);
    put(c.ci_D3); put(c.ci_A); put(c.ci_B); put(c.ci_C); put(c.ci_E); put(c.ci_F); put(c.ci_c2);
    put(c.sn_A); put(c.sn_a1); put(c.sn_b1); put(c.sn_a2); put(c.sn_H); put(c.sn_b2); put(c.sn_c2);
    put(c.eps_1m); put(c.l2_eps); put(c.l2_1000); for (int k = 0; k < 3; ++k) put(c.ch_b[k]);
    put(c.ch_b_rho);
    for (int i = 0; i < 3; ++i)
        for (int d = 0; d <= ChenGamma<FT>::D; ++d) put(c.chg.c[i][d]);
}
template <typename FT> constexpr int kPlainCount = NPT + NVT + 7 + 3 * (ChenGamma<FT>::D + 1);

// the PLAIN folds' constants — make_mp1m_consts, make_vel1m_consts + add_sedimentation_consts: what the primal column entry passes to its kernel — as FT
// values in the order above (out NULL: the count alone).  packed: the value parts of the fold with tangents as the kernels receive them
// (make_col1m_param_consts at KP = 1, no direction).
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t plain_consts(const MP *mp, const TH *tps, const ST *st, const CH *cr, const CI *ci, uint32_t flags, bool packed, FT *out) {
    if (!out) return kPlainCount<FT>;
    if (!packed) {
        const Mp1mConsts<FT> c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
        Vel1mConsts<FT> vc = make_vel1m_consts<FT>(*mp, cr);
        add_sedimentation_consts<FT>(vc, *mp, st, ci);
        std::memcpy(out, &c.eps_1m, NPT * sizeof(FT));
        vel_values<FT>(vc, out + NPT);
    } else {
        Col1mParamConsts<FT, 1> a;
        make_col1m_param_consts<FT, 1>(*mp, *tps, *st, *cr, *ci, flags, (const MP *)nullptr, (const TH *)nullptr, (const ST *)nullptr, (const CH *)nullptr,
                                       (const CI *)nullptr, 0, 0, a);
        const Dual<FT, 1> *s = &a.c.eps_1m;
        for (int m = 0; m < NPT; ++m) out[m] = s[m].v;
        vel_values<FT>(a.vc, out + NPT);
    }
    return kPlainCount<FT>;
}
}  // namespace

#define CMX_HOST_COLUMN_PARAM_1M(SFX, FT)                                                                                                                              \
    int32_t host_mp1m_column_param_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *st,                         \
                                             const cmx_chen2022_rain_vel_##SFX *cr, const cmx_chen2022_ice_vel_##SFX *ci, uint32_t flags, int kp, int64_t n_col,       \
                                             int32_t n_lev, const FT *inv_dz, const FT *const *x, int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                 \
                                             const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_st, const cmx_chen2022_rain_vel_##SFX *d_cr,                 \
                                             const cmx_chen2022_ice_vel_##SFX *d_ci, FT *const *jv, FT *const *jpr, FT *const *jps, FT *const *tend, FT *pr,           \
                                             FT *ps) {                                                                                                                 \
        return jvp<FT>(mp, tps, st, cr, ci, flags, kp, n_col, n_lev, inv_dz, x, ndir, d_mp, d_tps, d_st, d_cr, d_ci, jv, jpr, jps, tend, pr, ps);                      \
    }                                                                                                                                                                  \
    int32_t host_mp1m_column_param_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *st,                         \
                                             const cmx_chen2022_rain_vel_##SFX *cr, const cmx_chen2022_ice_vel_##SFX *ci, uint32_t flags, int kp, int64_t n_col,       \
                                             int32_t n_lev, const FT *inv_dz, const FT *const *x, const FT *const *cot, const FT *cpr, const FT *cps, int32_t ndir,    \
                                             const cmx_microphysics_1m_##SFX *d_mp, const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_st,                   \
                                             const cmx_chen2022_rain_vel_##SFX *d_cr, const cmx_chen2022_ice_vel_##SFX *d_ci, double *grad, FT *const *tend, FT *pr,   \
                                             FT *ps) {                                                                                                                 \
        return vjp<FT>(mp, tps, st, cr, ci, flags, kp, n_col, n_lev, inv_dz, x, cot, cpr, cps, ndir, d_mp, d_tps, d_st, d_cr, d_ci, grad, tend, pr, ps);               \
    }                                                                                                                                                                  \
    int32_t host_column_param_1m_consts_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *st,                        \
                                              const cmx_chen2022_rain_vel_##SFX *cr, const cmx_chen2022_ice_vel_##SFX *ci, uint32_t flags,                             \
                                              const cmx_microphysics_1m_##SFX *d_mp, const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_st,                  \
                                              const cmx_chen2022_rain_vel_##SFX *d_cr, const cmx_chen2022_ice_vel_##SFX *d_ci, double *out) {                          \
        return consts<FT>(mp, tps, st, cr, ci, flags, d_mp, d_tps, d_st, d_cr, d_ci, out);                                                                             \
    }                                                                                                                                                                  \
    int32_t host_column_param_1m_plain_consts_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *st,                  \
                                                    const cmx_chen2022_rain_vel_##SFX *cr, const cmx_chen2022_ice_vel_##SFX *ci, uint32_t flags, int packed,           \
                                                    FT *out) {                                                                                                         \
        return plain_consts<FT>(mp, tps, st, cr, ci, flags, packed != 0, out);                                                                                         \
    }

extern "C" {
int32_t host_column_param_1m_k_f32(int general) { return general ? kCol1mParamK<float, true> : kCol1mParamK<float, false>; }
int32_t host_column_param_1m_k_f64(int general) { return general ? kCol1mParamK<double, true> : kCol1mParamK<double, false>; }
int32_t host_column_param_1m_point_consts() { return NPT; }
CMX_HOST_COLUMN_PARAM_1M(f32, float)
CMX_HOST_COLUMN_PARAM_1M(f64, double)
}

#if defined(CMX_COLUMN_PARAM_1M_MAIN)
#include <cmath>
#include <cstdio>
#include <vector>

// The parameter structs come from a file the Python side writes (tests/test_column_param_1m_host.py: the raw bytes of cmx_microphysics_1m, cmx_thermo,
// cmx_stokes_vel, cmx_chen2022_rain_vel and cmx_chen2022_ice_vel of one float type, in this order); the columns and the directions (each parameter field
// times a pseudo-random factor) are made here.  Checks grad[d] = Σ ḡ·jvp_d + Σ p̄_rai·ṗ_rai,d + Σ p̄_sno·ṗ_sno,d and exits 0.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI> static int self_check(const char *path, uint32_t flags, bool cold) {
    MP mp; TH tps; ST st; CH cr; CI ci;
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    const bool ok = std::fread(&mp, sizeof mp, 1, f) == 1 && std::fread(&tps, sizeof tps, 1, f) == 1 && std::fread(&st, sizeof st, 1, f) == 1 &&
                    std::fread(&cr, sizeof cr, 1, f) == 1 && std::fread(&ci, sizeof ci, 1, f) == 1;
    std::fclose(f);
    if (!ok) return 2;
    const int64_t n_col = 5;
    const int32_t n_lev = 7, ndir = 5;
    const int64_t n = n_col * n_lev;
    std::vector<std::vector<FT>> x(NW + 1, std::vector<FT>(n)), gb(NO, std::vector<FT>(n)), tend(NO, std::vector<FT>(n)), jv(ndir * NO, std::vector<FT>(n)),
        jr(ndir, std::vector<FT>(n_col)), js(ndir, std::vector<FT>(n_col));
    std::vector<FT> inv_dz(n_lev), pbr(n_col), pbs(n_col), pr(n_col), ps(n_col);
    uint32_t seed = 12345u;
    auto u = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / 16777216.0; };
    for (int32_t k = 0; k < n_lev; ++k) inv_dz[k] = (FT)(1.0 / (50.0 + 30.0 * k));
    for (int64_t i = 0; i < n; ++i) {
        x[0][i] = (FT)(0.7 + 0.5 * u());
        x[1][i] = (FT)(cold ? 240.0 + 30.0 * u() : 275.0 + 15.0 * u());
        for (int s = 0; s < 4; ++s) x[3 + s][i] = (FT)(1e-5 + 1e-3 * u());
        x[2][i] = (FT)(x[3][i] + x[4][i] + x[5][i] + x[6][i] + (cold ? 1e-3 : 6e-3));
        for (int q = 0; q < NO; ++q) gb[q][i] = (FT)(u() - 0.5);
    }
    for (int64_t c = 0; c < n_col; ++c) { pbr[c] = (FT)(u() - 0.5); pbs[c] = (FT)(u() - 0.5); }
    // directions: every field of the structs (b and b_ρ of the rain table excepted) times a factor in ±1e-2
    std::vector<MP> d_mp(ndir); std::vector<TH> d_tps(ndir); std::vector<ST> d_st(ndir); std::vector<CH> d_cr(ndir); std::vector<CI> d_ci(ndir);
    auto scaled = [&](auto &dst, const auto &src) {
        FT *d = reinterpret_cast<FT *>(&dst);
        const FT *s = reinterpret_cast<const FT *>(&src);
        for (size_t m = 0; m < sizeof(src) / sizeof(FT); ++m) d[m] = (FT)(s[m] * 2e-2 * (u() - 0.5));
    };
    for (int d = 0; d < ndir; ++d) {
        scaled(d_mp[d], mp); scaled(d_tps[d], tps); scaled(d_st[d], st); scaled(d_cr[d], cr); scaled(d_ci[d], ci);
        d_cr[d].b[0] = d_cr[d].b[1] = d_cr[d].b[2] = d_cr[d].b_rho = 0;
    }
    const FT *xp[NW + 1], *gp[NO];
    FT *to[NO];
    std::vector<FT *> jo(ndir * NO), ro(ndir), so(ndir);
    for (int j = 0; j < NW + 1; ++j) xp[j] = x[j].data();
    for (int q = 0; q < NO; ++q) { gp[q] = gb[q].data(); to[q] = tend[q].data(); }
    for (int q = 0; q < ndir * NO; ++q) jo[q] = jv[q].data();
    for (int d = 0; d < ndir; ++d) { ro[d] = jr[d].data(); so[d] = js[d].data(); }
    if (jvp<FT>(&mp, &tps, &st, &cr, &ci, flags, 0, n_col, n_lev, inv_dz.data(), xp, ndir, d_mp.data(), d_tps.data(), d_st.data(), d_cr.data(), d_ci.data(), jo.data(),
                ro.data(), so.data(), to, pr.data(), ps.data()) < 0)
        return 3;
    std::vector<double> grad(ndir);
    if (vjp<FT>(&mp, &tps, &st, &cr, &ci, flags, 0, n_col, n_lev, inv_dz.data(), xp, gp, pbr.data(), pbs.data(), ndir, d_mp.data(), d_tps.data(), d_st.data(),
                d_cr.data(), d_ci.data(), grad.data(), nullptr, nullptr, nullptr) < 0)
        return 3;
    double worst = 0;
    for (int d = 0; d < ndir; ++d) {
        double sum = 0, scale = 0;
        for (int64_t i = 0; i < n; ++i)
            for (int q = 0; q < NO; ++q) { sum += (double)gb[q][i] * jv[d * NO + q][i]; scale += std::fabs((double)gb[q][i] * jv[d * NO + q][i]); }
        for (int64_t c = 0; c < n_col; ++c) {
            sum += (double)pbr[c] * jr[d][c] + (double)pbs[c] * js[d][c];
            scale += std::fabs((double)pbr[c] * jr[d][c]) + std::fabs((double)pbs[c] * js[d][c]);
        }
        if (!(std::fabs(sum - grad[d]) <= (sizeof(FT) == 4 ? 1e-4 : 1e-12) * scale) || !(scale > 0)) return 4;
        worst = std::fmax(worst, std::fabs(sum - grad[d]) / scale);
    }
    std::printf("gradient against the jvp columns, %s flags %u %s: worst %.3g of the terms' size\n", sizeof(FT) == 4 ? "f32" : "f64", flags, cold ? "cold" : "warm", worst);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 64;
    const uint32_t flags = (uint32_t)std::strtoul(argv[3], nullptr, 0);
    int rc = 0;
    for (bool cold : {false, true}) {
        rc |= self_check<float, cmx_microphysics_1m_f32, cmx_thermo_f32, cmx_stokes_vel_f32, cmx_chen2022_rain_vel_f32, cmx_chen2022_ice_vel_f32>(argv[1], flags, cold);
        rc |= self_check<double, cmx_microphysics_1m_f64, cmx_thermo_f64, cmx_stokes_vel_f64, cmx_chen2022_rain_vel_f64, cmx_chen2022_ice_vel_f64>(argv[2], flags, cold);
    }
    return rc;
}
#endif
