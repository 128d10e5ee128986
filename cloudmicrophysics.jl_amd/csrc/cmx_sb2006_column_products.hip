// cmx_sb2006_column_products.hip — J v and Jᵀḡ of the SB2006 column step with sedimentation (cmx_sb2006_column.hip), for gfx950: C-ABI entry points
// cmx_sb2006_column_jvp_* / cmx_sb2006_column_vjp_* (include/cmx.h §(25)).  What a Newton–Krylov solver over the column needs as its matvec, and what
// loss(precip_flux).backward() needs (cmx/autograd.py).  The scheme and the bodies of one point are cmx_sb2006_column_jac.hpp's, shared with the host test
// build; the kernels are the halo shell (J v) and the point shell (Jᵀḡ) of cmx_column_products.hpp, and here are their policy struct and the entries.
// (The packed pair and four points per lane of the primal's Float32 kernel were not built for J v: the dual point function with the fall speeds holds twice
// the primal's intermediates; the register counts are HISTORY.md's.)
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_sb2006_column_jac.hpp"

namespace cmx {

// The state derivatives of the scheme S_ in the shells: J v carries the caller's one tangent, Jᵀḡ K tangents per pass
template <typename S_, typename FT_> struct SbColState {
    using S = S_;
    using FT = FT_;
    using Consts = SbColConsts<FT>;
    using Args = ColJvpArgs<FT>;
    template <int K> using VjpArgs = ColVjpArgs<FT, K>;
    using Point = ColJvpPoint<FT>;
    static constexpr int NT = 1;
    static constexpr bool TANGENTS = true;
    static __device__ __forceinline__ FT Fd(const Point &p, int, int s) { return p.Fd[s]; }
    static __device__ __forceinline__ void eval(const Consts &k, const FT (&x)[S::NWRT + 1], const FT (&t)[S::NWRT], FT inv_dz, Point &p) {
        column_jvp_eval<S, FT>(k.c, k.cv, x, t, inv_dz, p);
    }
    static __device__ __forceinline__ void store(const Args &a, const Point &p, const FT (&upv)[4], const FT (&upd)[1][4], bool top, bool surface, int64_t i,
                                                 int64_t col) {
        column_jvp_store<S, FT>(a, p, upv, upd[0], top, surface, i, col);
    }
    template <int K> static __device__ __forceinline__ void vjp_point(const Consts &k, const VjpArgs<K> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev) {
        column_vjp_point<S, FT, K>(k.c, k.cv, a, x, i, col, lev);
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of both operations.  The statuses of the primal entry, in its order: the parameters, then `status` — the ladder of column_entry_status with
// the operation's columns — then the limiters and the fall-speed parameters (with_sb2006_column_jac).  run(k, S): fills the kernel's arguments and launches.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename RUN>
static int32_t entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int32_t status, RUN &&run) {
    if (!wr || !tps || !vel) return CMX_ERR_BAD_ARG;
    if (status != kColumnEntryRun) return status;
    return with_sb2006_column_jac<FT>(*wr, *tps, *vel, cloud_vel, flags, [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S) -> int32_t {
        run(SbColConsts<FT>{c, cv}, S);
        return launched();
    });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t jvp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                         const FT *const (&in)[7], const FT *const *tangents, FT *const *jvp, FT *jvp_precip, FT *const *tendencies, FT *precip, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(wr, tps, vel, cloud_vel, flags, sb2006_column_jvp_status(flags, n_col, n_lev, inv_dz, in, tangents, jvp, jvp_precip, tendencies, precip),
                     [&](const SbColConsts<FT> &k, auto S) {
                         ColJvpArgs<FT> a;
                         make_col_jvp_args(a, in, inv_dz, n_col * (int64_t)n_lev, n_lev, tangents, jvp, jvp_precip, tendencies, precip);
                         launch_column_halo<SbColState<decltype(S), FT>>(k, a, s);
                     });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t vjp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                         const FT *const (&in)[7], const FT *const *cotangents, const FT *cot_precip, FT *const *grad, FT *const *tendencies, FT *precip,
                         void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(wr, tps, vel, cloud_vel, flags, sb2006_column_vjp_status(flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip, grad, tendencies, precip),
                     [&](const SbColConsts<FT> &k, auto S) {
                         using SC = decltype(S);
                         constexpr int K = kColVjpK<FT, SC::vel>;
                         ColVjpArgs<FT, K> a;
                         make_col_vjp_args(a, in, inv_dz, n_col * (int64_t)n_lev, n_lev, cotangents, cot_precip, grad, tendencies, precip);
                         set_col_vjp_terms<SC>(a);
                         launch_column_point<SbColState<SC, FT>, K>(k, a, s);
                     });
}

}  // namespace cmx

#define CMX_COLUMN_PRODUCTS(SFX, FT)                                                                                                                                  \
    int32_t cmx_sb2006_column_jvp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                          \
                                        const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,         \
                                        const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai,                             \
                                        const FT *const tangents[CMX_SB2006_JAC_NWRT], FT *const jvp[CMX_SB2006_JAC_NOUT], FT *jvp_precip,                            \
                                        FT *const tendencies[CMX_SB2006_JAC_NOUT], FT *precip_flux, void *stream) {                                                   \
        return cmx::jvp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, tangents, jvp,            \
                                  jvp_precip, tendencies, precip_flux, stream);                                                                                       \
    }                                                                                                                                                                 \
    int32_t cmx_sb2006_column_vjp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                          \
                                        const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,         \
                                        const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai,                             \
                                        const FT *const cotangents[CMX_SB2006_JAC_NOUT], const FT *cot_precip, FT *const grad[CMX_SB2006_JAC_NWRT],                   \
                                        FT *const tendencies[CMX_SB2006_JAC_NOUT], FT *precip_flux, void *stream) {                                                   \
        return cmx::vjp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents, cot_precip,   \
                                  grad, tendencies, precip_flux, stream);                                                                                             \
    }

extern "C" {
CMX_COLUMN_PRODUCTS(f32, float)
CMX_COLUMN_PRODUCTS(f64, double)
}
