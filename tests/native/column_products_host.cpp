// column_products_host.cpp — TEST INFRASTRUCTURE: the host build of the products with the Jacobian of the SB2006 column step (include/cmx.h §(25)).  The scheme
// SbColJac and the bodies of one point (csrc/cmx_sb2006_column_jac.hpp) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for the hardware
// transcendental instructions) and run over columns by plain loops, set up by the function the device entries call (with_sb2006_column_jac), so that the
// mathematics — the dual fall speeds and fluxes, the coupling of a level with the one above, the adjoint — is tested against finite differences of the Float64
// oracle without a GPU (tests/test_column_products_host.py).  host_sb2006_column_plain_* runs the PLAIN instantiation with the operations of
// sb2006_column_kernel: the value parts of the products must equal it bit for bit.  NOT part of libcmx.so and no CPU fallback.
//
// With -DCMX_COLUMN_PRODUCTS_MAIN it is a stand-alone program (its own main: a few columns through every entry, the adjoint identity checked) — the one to
// build with host sanitizer flags.
#define CMX_HOST_BUILD 1
#include <cstdint>
#include <initializer_list>

#include "../../cloudmicrophysics.jl_amd/csrc/cmx_sb2006_column_jac.hpp"

namespace {
using namespace cmx;
constexpr int NW = CMX_SB2006_JAC_NWRT, NO = CMX_SB2006_JAC_NOUT;

// Every function returns the statuses of the device entries — the parameter structs, the entry's status function (the ladder of column_entry_status with its
// columns), then with_sb2006_column_jac — or what ran.

// J v: the levels of a column from the top down, so that the fluxes of the cell above are at hand.  Returns the velocity kind that ran.
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t jvp(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,
            const FT *const *tan, FT *const *jv, FT *jv_precip, FT *const *tend, FT *precip) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_jvp_status(flags, n_col, n_lev, inv_dz, x, tan, jv, jv_precip, tend, precip); st != kColumnEntryRun) return st;
    return with_sb2006_column_jac<FT>(*wr, *tps, *vel, cloud_vel, flags, [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S) -> int32_t {
        using SC = decltype(S);
        const FT *in[NW + 1];
        for (int j = 0; j < NW + 1; ++j) in[j] = x[j];
        ColJvpArgs<FT> a;
        make_col_jvp_args(a, in, inv_dz, n_col * n_lev, n_lev, tan, jv, jv_precip, tend, precip);
        for (int64_t col = 0; col < n_col; ++col) {
            FT upv[4] = {}, upd[4] = {};
            for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                const int64_t i = col * n_lev + lev;
                FT xi[NW + 1], ti[NW];
                for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                for (int j = 0; j < NW; ++j) ti[j] = a.tan[j] ? a.tan[j][i] : FT(0);
                ColJvpPoint<FT> p;
                column_jvp_eval<SC, FT>(c, cv, xi, ti, inv_dz[lev], p);
                column_jvp_store<SC, FT>(a, p, upv, upd, lev == n_lev - 1, lev == 0, i, col);
                for (int s = 0; s < 4; ++s) { upv[s] = p.Fv[s]; upd[s] = p.Fd[s]; }
            }
        }
        return SC::vel;
    });
}

// Jᵀḡ: pointwise.  k: tangents per pass (0: the device kernel's choice for the float type)
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t vjp(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int k, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,
            const FT *const *cot, const FT *cot_precip, FT *const *grad, FT *const *tend, FT *precip) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_vjp_status(flags, n_col, n_lev, inv_dz, x, cot, cot_precip, grad, tend, precip); st != kColumnEntryRun) return st;
    return with_sb2006_column_jac<FT>(*wr, *tps, *vel, cloud_vel, flags, [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S) -> int32_t {
        using SC = decltype(S);
        return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto KT) -> int32_t {
            constexpr int K = decltype(KT)::value;
            const FT *in[NW + 1];
            for (int j = 0; j < NW + 1; ++j) in[j] = x[j];
            ColVjpArgs<FT, K> a;
            make_col_vjp_args(a, in, inv_dz, n_col * n_lev, n_lev, cot, cot_precip, grad, tend, precip);
            set_col_vjp_terms<SC>(a);
            for (int64_t col = 0; col < n_col; ++col)
                for (int32_t lev = 0; lev < n_lev; ++lev) {
                    const int64_t i = col * n_lev + lev;
                    FT xi[NW + 1];
                    for (int j = 0; j < NW + 1; ++j) xi[j] = a.in[j][i];
                    column_vjp_point<SC, FT, K>(c, cv, a, xi, i, col, lev);
                }
            return SC::vel;
        }, one_of<1, 2, 3, 6>(k ? k : kColVjpK<FT, SC::vel>));
    });
}

// the plain instantiation: the operations of sb2006_column_kernel (csrc/cmx_sb2006_column.hip), one point at a time
template <typename FT, typename WR, typename TH, typename VL, typename ST>
int32_t plain(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,
              FT *const *y, FT *precip) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_jvp_status<FT>(flags, n_col, n_lev, inv_dz, x, nullptr, nullptr, nullptr, y, precip); st != kColumnEntryRun) return st;
    return with_sb2006_column_jac<FT>(*wr, *tps, *vel, cloud_vel, flags, [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S) -> int32_t {
        using SC = decltype(S);
        using M = Math<FT>;
        for (int64_t col = 0; col < n_col; ++col) {
            SedFlux<FT> up{FT(0), FT(0), FT(0), FT(0)};
            for (int32_t lev = n_lev - 1; lev >= 0; --lev) {
                const int64_t i = col * n_lev + lev;
                const FT rho = x[0][i], T = x[1][i], q_tot = x[2][i], q_lcl = x[3][i], n_lcl = x[4][i], q_rai = x[5][i], n_rai = x[6][i];
                const FT r_ = max0(rho), qt = max0(q_tot), ql = max0(q_lcl), qr = max0(q_rai), nl = max0(n_lcl), nr = max0(n_rai);
                const SbRates<FT> p = sb2006_point<FT, SC::limited, SC::vel, false, SC::intpow>(c, r_, T, qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
                SedFlux<FT> F = sed_fluxes<FT, SC::cloud>(cv, r_, ql, nl, qr, nr, p.vt_n, p.vt_m);
                const FT g = inv_dz[lev] * p.inv_rho;
                FT A[4];
                A[0] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
                A[1] = M::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
                A[2] = M::fma(-F.q_rai, g, (p.evq + p.au_dq_rai) + p.ac_dq_rai);
                A[3] = M::fma(-F.n_rai, g, M::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai));
                if (SC::cloud) {
                    A[0] = M::fma(-F.q_lcl, g, A[0]);
                    A[1] = M::fma(-F.n_lcl, g, A[1]);
                }
                if (any_nan(rho, q_tot, q_lcl, n_lcl, q_rai, n_rai, T)) A[0] = A[1] = A[2] = A[3] = M::nan();
                if (any_nan(rho, q_lcl, n_lcl, q_rai, n_rai)) F.q_rai = F.n_rai = F.q_lcl = F.n_lcl = M::nan();
                const bool top = lev == n_lev - 1;
                y[0][i] = (top || !SC::cloud) ? A[0] : M::fma(up.q_lcl, g, A[0]);
                y[1][i] = (top || !SC::cloud) ? A[1] : M::fma(up.n_lcl, g, A[1]);
                y[2][i] = top ? A[2] : M::fma(up.q_rai, g, A[2]);
                y[3][i] = top ? A[3] : M::fma(up.n_rai, g, A[3]);
                if (lev == 0 && precip) precip[col] = F.q_rai;
                up = F;
            }
        }
        return SC::vel;
    });
}
}  // namespace

#define CMX_HOST_COLUMN_PRODUCTS(SFX, FT)                                                                                                                              \
    int32_t host_sb2006_column_jvp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                                 \
                                         const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,     \
                                         const FT *const *tan, FT *const *jv, FT *jv_precip, FT *const *tend, FT *precip) {                                            \
        return jvp<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, x, tan, jv, jv_precip, tend, precip);                                                     \
    }                                                                                                                                                                  \
    int32_t host_sb2006_column_vjp_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                                 \
                                         const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int k, int64_t n_col, int32_t n_lev, const FT *inv_dz,                 \
                                         const FT *const *x, const FT *const *cot, const FT *cot_precip, FT *const *grad, FT *const *tend, FT *precip) {               \
        return vjp<FT>(wr, tps, vel, cloud_vel, flags, k, n_col, n_lev, inv_dz, x, cot, cot_precip, grad, tend, precip);                                               \
    }                                                                                                                                                                  \
    int32_t host_sb2006_column_plain_##SFX(const cmx_warm_rain_2m_##SFX *wr, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                               \
                                           const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *x,   \
                                           FT *const *y, FT *precip) {                                                                                                 \
        return plain<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, x, y, precip);                                                                          \
    }

extern "C" {
int32_t host_column_vjp_k_f32(int vel) { return vel == VEL_CHEN_GEN ? kColVjpK<float, VEL_CHEN_GEN> : kColVjpK<float, VEL_SB>; }
int32_t host_column_vjp_k_f64(int vel) { return vel == VEL_CHEN_GEN ? kColVjpK<double, VEL_CHEN_GEN> : kColVjpK<double, VEL_SB>; }
CMX_HOST_COLUMN_PRODUCTS(f32, float)
CMX_HOST_COLUMN_PRODUCTS(f64, double)
}

#if defined(CMX_COLUMN_PRODUCTS_MAIN)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

// The parameter structs come from a file the Python side writes (tests/test_column_products_host.py: the raw bytes of cmx_warm_rain_2m, cmx_thermo,
// cmx_rain_vel and cmx_stokes_vel of one float type, in this order); the columns are made here.  Checks the adjoint identity over whole columns and exits 0.
template <typename FT, typename WR, typename TH, typename VL, typename ST> static int self_check(const char *path, uint32_t flags, bool cloud) {
    WR wr; TH tps; VL vel; ST st;
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    const bool ok = std::fread(&wr, sizeof wr, 1, f) == 1 && std::fread(&tps, sizeof tps, 1, f) == 1 && std::fread(&vel, sizeof vel, 1, f) == 1 &&
                    std::fread(&st, sizeof st, 1, f) == 1;
    std::fclose(f);
    if (!ok) return 2;
    const int64_t n_col = 5;
    const int32_t n_lev = 7;
    const int64_t n = n_col * n_lev;
    std::vector<std::vector<FT>> x(NW + 1, std::vector<FT>(n)), v(NW, std::vector<FT>(n)), gb(NO, std::vector<FT>(n)), y(NO, std::vector<FT>(n)),
        gr(NW, std::vector<FT>(n)), tend(NO, std::vector<FT>(n));
    std::vector<FT> inv_dz(n_lev), pb(n_col), yp(n_col), precip(n_col);
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
        for (int j = 0; j < NW; ++j) v[j][i] = (FT)((u() - 0.5) * x[j + 1][i]);
        for (int q = 0; q < NO; ++q) gb[q][i] = (FT)(u() - 0.5);
    }
    for (int64_t c = 0; c < n_col; ++c) pb[c] = (FT)(u() - 0.5);
    const FT *xp[NW + 1], *vp[NW], *gp[NO];
    FT *yo[NO], *go[NW], *to[NO];
    for (int j = 0; j < NW + 1; ++j) xp[j] = x[j].data();
    for (int j = 0; j < NW; ++j) { vp[j] = v[j].data(); go[j] = gr[j].data(); }
    for (int q = 0; q < NO; ++q) { gp[q] = gb[q].data(); yo[q] = y[q].data(); to[q] = tend[q].data(); }
    const ST *cv = cloud ? &st : nullptr;
    if (jvp<FT>(&wr, &tps, &vel, cv, flags, n_col, n_lev, inv_dz.data(), xp, vp, yo, yp.data(), to, precip.data()) < 0) return 3;
    if (vjp<FT>(&wr, &tps, &vel, cv, flags, 0, n_col, n_lev, inv_dz.data(), xp, gp, pb.data(), go, to, precip.data()) < 0) return 3;
    double worst = 0;
    for (int64_t c = 0; c < n_col; ++c) {
        double lhs = (double)pb[c] * yp[c], rhs = 0, scale = std::fabs((double)pb[c] * yp[c]);
        for (int64_t i = c * n_lev; i < (c + 1) * n_lev; ++i) {
            for (int q = 0; q < NO; ++q) { lhs += (double)gb[q][i] * y[q][i]; scale += std::fabs((double)gb[q][i] * y[q][i]); }
            for (int j = 0; j < NW; ++j) { rhs += (double)gr[j][i] * v[j][i]; scale += std::fabs((double)gr[j][i] * v[j][i]); }
        }
        if (!(std::fabs(lhs - rhs) <= (sizeof(FT) == 4 ? 1e-3 : 1e-9) * scale)) return 4;
        worst = std::fmax(worst, std::fabs(lhs - rhs) / scale);
    }
    std::printf("adjoint identity, %s flags %u cloud %d: worst %.3g of the terms' size\n", sizeof(FT) == 4 ? "f32" : "f64", flags, (int)cloud, worst);
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
