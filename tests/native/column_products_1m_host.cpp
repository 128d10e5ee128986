// column_products_1m_host.cpp — TEST INFRASTRUCTURE: the host build of the products with the Jacobian of the 1-moment column step (include/cmx.h §(27)).  The
// scheme Mp1mColJac and the bodies of one point (csrc/cmx_mp1m_column_jac.hpp) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the hardware
// transcendental instructions) and run over columns by plain loops, set up by the function the device entries call (with_mp1m_column_jac), so that the
// mathematics — the four dual fall speeds and fluxes, the coupling of a level with the one above, the two precipitation rows, the adjoint — is tested against
// finite differences of the Float64 oracle without a GPU (tests/test_column_products_1m_host.py).  host_mp1m_column_plain_* runs the PLAIN instantiation with
// the operations of the primal kernel (csrc/cmx_mp1m_column_body.inc): the value parts of the products must equal it bit for bit.  NOT part of libcmx.so and
// no CPU fallback.
//
// With -DCMX_COLUMN_PRODUCTS_1M_MAIN it is a stand-alone program (its own main: a few columns through every entry, the adjoint identity checked) — the one to
// build with host sanitizer flags.
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <initializer_list>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_mp1m_column_jac.hpp"

namespace {
using namespace cmx;
constexpr int NW = CMX_MP1M_JAC_NWRT, NO = CMX_MP1M_JAC_NOUT;

// what ran: bit 0 the default-options instantiation, bit 1 the general Γ of the Chen-2022 rain table
template <typename S> constexpr int32_t kind() { return (S::flags != kRuntimeFlags ? 1 : 0) | (S::general ? 2 : 0); }

// Every function returns the statuses of the device entries — the parameter structs, the entry's status function (the ladder of column_entry_status with its
// columns), then with_mp1m_column_jac — or what ran.

// J v: the levels of a column from the top down, so that the fluxes of the cell above are at hand
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t jvp(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
            const FT *const *x, const FT *const *tan, FT *const *jv, FT *jv_pr, FT *jv_ps, FT *const *tend, FT *pr, FT *ps) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice) return CMX_ERR_BAD_ARG;
    if (const int32_t st = mp1m_column_jvp_status(flags, n_col, n_lev, inv_dz, x, tan, jv, jv_pr, jv_ps, tend, pr, ps); st != kColumnEntryRun) return st;
    return with_mp1m_column_jac<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, [&](const Mp1mColJacConsts<FT> &c, auto S) -> int32_t {
        using SC = decltype(S);
        const FT *const in[NW + 1] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
        Col1mJvpArgs<FT> a;
        make_col1m_jvp_args(a, in, inv_dz, n_col * n_lev, n_lev, tan, jv, jv_pr, jv_ps, tend, pr, ps);
        for (int64_t col = 0; col < n_col; ++col) {
            FT upv[4] = {}, upd[4] = {};
            for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                const int64_t i = col * n_lev + lev;
                FT xi[NW + 1], ti[NW];
                for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                for (int j = 0; j < NW; ++j) ti[j] = a.tan[j] ? a.tan[j][i] : FT(0);
                Col1mJvpPoint<FT> p;
                column1m_jvp_eval<SC, FT>(c, xi, ti, inv_dz[lev], p);
                column1m_jvp_store<SC, FT>(a, p, upv, upd, lev == n_lev - 1, lev == 0, i, col);
                for (int s = 0; s < 4; ++s) { upv[s] = p.Fv[s]; upd[s] = p.Fd[s]; }
            }
        }
        return kind<SC>();
    });
}

// Jᵀḡ: pointwise.  k: tangents per pass (0: the device kernel's choice for the float type and the instantiation)
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t vjp(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int k, int64_t n_col, int32_t n_lev, const FT *inv_dz,
            const FT *const *x, const FT *const *cot, const FT *cot_pr, const FT *cot_ps, FT *const *grad, FT *const *tend, FT *pr, FT *ps) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice) return CMX_ERR_BAD_ARG;
    if (const int32_t st = mp1m_column_vjp_status(flags, n_col, n_lev, inv_dz, x, cot, cot_pr, cot_ps, grad, tend, pr, ps); st != kColumnEntryRun) return st;
    return with_mp1m_column_jac<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, [&](const Mp1mColJacConsts<FT> &c, auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int K = decltype(KT)::value;
            const FT *const in[NW + 1] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
            Col1mVjpArgs<FT, K> a;
            make_col1m_vjp_args(a, in, inv_dz, n_col * n_lev, n_lev, cot, cot_pr, cot_ps, grad, tend, pr, ps);
            for (int64_t col = 0; col < n_col; ++col)
                for (int32_t lev = 0; lev < n_lev; ++lev) {
                    const int64_t i = col * n_lev + lev;
                    FT xi[NW + 1];
                    for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                    column1m_vjp_point<SC, FT, K>(c, a, xi, i, col, lev);
                }
            return kind<SC>();
        }, one_of<1, 2, 3, 6>(k ? k : kCol1mVjpK<FT, SC::general>));
    });
}

// the plain instantiation: the operations of the primal kernel (csrc/cmx_mp1m_column_body.inc), one point at a time
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
int32_t plain(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
              const FT *const *x, FT *const *y, FT *pr, FT *ps) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice) return CMX_ERR_BAD_ARG;
    if (const int32_t st = mp1m_column_jvp_status<FT>(flags, n_col, n_lev, inv_dz, x, nullptr, nullptr, nullptr, nullptr, y, pr, ps); st != kColumnEntryRun) return st;
    return with_mp1m_column_jac<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, [&](const Mp1mColJacConsts<FT> &c, auto S) -> int32_t {
        using SC = decltype(S);
        using M = Math<FT>;
        for (int64_t col = 0; col < n_col; ++col) {
            SedFlux4<FT> up{{FT(0), FT(0), FT(0), FT(0)}};
            for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                const int64_t i = col * n_lev + lev;
                FT t[4];
                mp1m_tendencies_point<FT, SC::flags>(c.c, x[0][i], x[1][i], x[2][i], x[3][i], x[4][i], x[5][i], x[6][i], t[0], t[1], t[2], t[3]);
                const SedFlux4<FT> F = mp1m_sed_fluxes<FT, SC::general, false>(c.vc, x[0][i], x[3][i], x[4][i], x[5][i], x[6][i]);
                const FT g = inv_dz[lev] * M::rcp(max0(x[0][i]));
                const bool top = lev == n_lev - 1;
                for (int s = 0; s < 4; ++s) y[s][i] = M::fma(top ? FT(0) : up.f[s], g, M::fma(-F.f[s], g, t[s]));
                if (lev == 0) {
                    if (pr) pr[col] = F.f[2];
                    if (ps) ps[col] = F.f[3];
                }
                up = F;
            }
        }
        return kind<SC>();
    });
}
}  // namespace

#define CMX_HOST_COLUMN_PRODUCTS_1M(SFX, FT)                                                                                                                           \
    int32_t host_mp1m_column_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                          \
                                       const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,       \
                                       int32_t n_lev, const FT *inv_dz, const FT *const *x, const FT *const *tan, FT *const *jv, FT *jv_pr, FT *jv_ps,                 \
                                       FT *const *tend, FT *pr, FT *ps) {                                                                                              \
        return jvp<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, x, tan, jv, jv_pr, jv_ps, tend, pr, ps);                                     \
    }                                                                                                                                                                  \
    int32_t host_mp1m_column_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                          \
                                       const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int k,               \
                                       int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x, const FT *const *cot, const FT *cot_pr, const FT *cot_ps,  \
                                       FT *const *grad, FT *const *tend, FT *pr, FT *ps) {                                                                             \
        return vjp<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, k, n_col, n_lev, inv_dz, x, cot, cot_pr, cot_ps, grad, tend, pr, ps);                              \
    }                                                                                                                                                                  \
    int32_t host_mp1m_column_plain_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                        \
                                         const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,     \
                                         int32_t n_lev, const FT *inv_dz, const FT *const *x, FT *const *y, FT *pr, FT *ps) {                                          \
        return plain<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, x, y, pr, ps);                                                             \
    }

extern "C" {
int32_t host_column1m_vjp_k_f32(int general) { return general ? kCol1mVjpK<float, true> : kCol1mVjpK<float, false>; }
int32_t host_column1m_vjp_k_f64(int general) { return general ? kCol1mVjpK<double, true> : kCol1mVjpK<double, false>; }
CMX_HOST_COLUMN_PRODUCTS_1M(f32, float)
CMX_HOST_COLUMN_PRODUCTS_1M(f64, double)
}

#if defined(CMX_COLUMN_PRODUCTS_1M_MAIN)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// The parameter structs come from a file the Python side writes (tests/test_column_products_1m_host.py: the raw bytes of cmx_microphysics_1m, cmx_thermo,
// cmx_stokes_vel, cmx_chen2022_rain_vel and cmx_chen2022_ice_vel of one float type, in this order, then the uint32 flags); the columns are made here.  Checks
// the adjoint identity over whole columns, with both precipitation terms, and exits 0.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI> static int self_check(const char *path) {
    MP mp; TH tps; ST st; CH cr; CI ci;
    uint32_t flags = 0;
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    const bool ok = std::fread(&mp, sizeof mp, 1, f) == 1 && std::fread(&tps, sizeof tps, 1, f) == 1 && std::fread(&st, sizeof st, 1, f) == 1 &&
                    std::fread(&cr, sizeof cr, 1, f) == 1 && std::fread(&ci, sizeof ci, 1, f) == 1 && std::fread(&flags, sizeof flags, 1, f) == 1;
    std::fclose(f);
    if (!ok) return 2;
    const int64_t n_col = 5;
    const int32_t n_lev = 7;
    const int64_t n = n_col * n_lev;
    std::vector<std::vector<FT>> x(NW + 1, std::vector<FT>(n)), v(NW, std::vector<FT>(n)), gb(NO, std::vector<FT>(n)), y(NO, std::vector<FT>(n)),
        gr(NW, std::vector<FT>(n)), tend(NO, std::vector<FT>(n));
    std::vector<FT> inv_dz(n_lev), pbr(n_col), pbs(n_col), ypr(n_col), yps(n_col), pr(n_col), ps(n_col);
    uint32_t seed = 12345u;
    auto u = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / 16777216.0; };
    for (int32_t k = 0; k < n_lev; ++k) inv_dz[k] = (FT)(1.0 / (50.0 + 30.0 * k));
    for (int64_t i = 0; i < n; ++i) {
        x[0][i] = (FT)(0.7 + 0.5 * u());
        x[1][i] = (FT)(250.0 + 40.0 * u());
        for (int j = 3; j < 7; ++j) x[j][i] = (FT)(1e-5 + 1e-3 * u());
        x[2][i] = (FT)(x[3][i] + x[4][i] + x[5][i] + x[6][i] + 3e-3);
        for (int j = 0; j < NW; ++j) v[j][i] = (FT)((u() - 0.5) * x[j + 1][i]);
        for (int q = 0; q < NO; ++q) gb[q][i] = (FT)(u() - 0.5);
    }
    for (int64_t c = 0; c < n_col; ++c) { pbr[c] = (FT)(u() - 0.5); pbs[c] = (FT)(u() - 0.5); }
    const FT *xp[NW + 1], *vp[NW], *gp[NO];
    FT *yo[NO], *go[NW], *to[NO];
    for (int j = 0; j < NW + 1; ++j) xp[j] = x[j].data();
    for (int j = 0; j < NW; ++j) { vp[j] = v[j].data(); go[j] = gr[j].data(); }
    for (int q = 0; q < NO; ++q) { gp[q] = gb[q].data(); yo[q] = y[q].data(); to[q] = tend[q].data(); }
    if (jvp<FT>(&mp, &tps, &st, &cr, &ci, flags, n_col, n_lev, inv_dz.data(), xp, vp, yo, ypr.data(), yps.data(), to, pr.data(), ps.data()) < 0) return 3;
    if (vjp<FT>(&mp, &tps, &st, &cr, &ci, flags, 0, n_col, n_lev, inv_dz.data(), xp, gp, pbr.data(), pbs.data(), go, to, pr.data(), ps.data()) < 0) return 3;
    double worst = 0;
    for (int64_t c = 0; c < n_col; ++c) {
        double lhs = (double)pbr[c] * ypr[c] + (double)pbs[c] * yps[c], rhs = 0, scale = std::fabs((double)pbr[c] * ypr[c]) + std::fabs((double)pbs[c] * yps[c]);
        for (int64_t i = c * n_lev; i < (c + 1) * n_lev; ++i) {
            for (int q = 0; q < NO; ++q) { lhs += (double)gb[q][i] * y[q][i]; scale += std::fabs((double)gb[q][i] * y[q][i]); }
            for (int j = 0; j < NW; ++j) { rhs += (double)gr[j][i] * v[j][i]; scale += std::fabs((double)gr[j][i] * v[j][i]); }
        }
        if (!(std::fabs(lhs - rhs) <= (sizeof(FT) == 4 ? 1e-3 : 1e-9) * scale)) return 4;
        worst = std::fmax(worst, std::fabs(lhs - rhs) / scale);
    }
    std::printf("adjoint identity, %s flags %u: worst %.3g of the terms' size\n", sizeof(FT) == 4 ? "f32" : "f64", flags, worst);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 64;
    int rc = 0;
    rc |= self_check<float, cmx_microphysics_1m_f32, cmx_thermo_f32, cmx_stokes_vel_f32, cmx_chen2022_rain_vel_f32, cmx_chen2022_ice_vel_f32>(argv[1]);
    rc |= self_check<double, cmx_microphysics_1m_f64, cmx_thermo_f64, cmx_stokes_vel_f64, cmx_chen2022_rain_vel_f64, cmx_chen2022_ice_vel_f64>(argv[2]);
    return rc;
}
#endif
