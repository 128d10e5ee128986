// cmx_mp1m_column_products.hip — J v and Jᵀḡ of the 1-moment column step with sedimentation (cmx_mp1m_column.hip, Instantaneous mode), for gfx950: C-ABI
// entry points cmx_mp1m_column_jvp_* / cmx_mp1m_column_vjp_* (include/cmx.h §(27)).  What a Newton–Krylov solver over a mixed-phase column needs as its
// matvec, and what loss(precip_rai + precip_sno).backward() needs (cmx/autograd.py).  The scheme and the bodies of one point are cmx_mp1m_column_jac.hpp's,
// shared with the host test build; the kernels are the halo shell (J v) and the point shell (Jᵀḡ) of cmx_column_products.hpp, and here are their policy
// struct and the entries.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_products.hpp"
#include "cmx_mp1m_column_jac.hpp"

namespace cmx {

// The state derivatives of the scheme S_ in the shells: J v carries the caller's one tangent, Jᵀḡ K tangents per pass
template <typename S_, typename FT_> struct Mp1mColState {
    using S = S_;
    using FT = FT_;
    using Consts = Mp1mColJacConsts<FT>;
    using Args = Col1mJvpArgs<FT>;
    template <int K> using VjpArgs = Col1mVjpArgs<FT, K>;
    using Point = Col1mJvpPoint<FT>;
    static constexpr int NT = 1;
    static constexpr bool TANGENTS = true;
    static __device__ __forceinline__ FT Fd(const Point &p, int, int s) { return p.Fd[s]; }
    static __device__ __forceinline__ void eval(const Consts &c, const FT (&x)[S::NWRT + 1], const FT (&t)[S::NWRT], FT inv_dz, Point &p) {
        column1m_jvp_eval<S, FT>(c, x, t, inv_dz, p);
    }
    static __device__ __forceinline__ void store(const Args &a, const Point &p, const FT (&upv)[4], const FT (&upd)[1][4], bool top, bool surface, int64_t i,
                                                 int64_t col) {
        column1m_jvp_store<S, FT>(a, p, upv, upd[0], top, surface, i, col);
    }
    template <int K> static __device__ __forceinline__ void vjp_point(const Consts &c, const VjpArgs<K> &a, const FT (&x)[S::NWRT + 1], int64_t i, int64_t col, int32_t lev) {
        column1m_vjp_point<S, FT, K>(c, a, x, i, col, lev);
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of both operations.  The statuses of the primal entry, in its order: the parameters, then `status` — the ladder of column_entry_status with
// the operation's columns (its flags: the primal's, then this entry's own, a snow-shape bit).  run(c, S, x): fills the kernel's arguments and launches.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename RUN>
static int32_t entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int32_t status, const FT *const *in,
                     RUN &&run) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice) return CMX_ERR_BAD_ARG;
    if (status != kColumnEntryRun) return status;
    const FT *const x[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
    return with_mp1m_column_jac<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, [&](const Mp1mColJacConsts<FT> &a, auto S) -> int32_t {
        run(a, S, x);
        return launched();
    });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t jvp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                         const FT *inv_dz, const FT *const *in, const FT *const *tangents, FT *const *jvp, FT *jvp_precip_rai, FT *jvp_precip_sno,
                         FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags,
                     mp1m_column_jvp_status(flags, n_col, n_lev, inv_dz, in, tangents, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai, precip_sno), in,
                     [&](const Mp1mColJacConsts<FT> &c, auto S, const FT *const (&x)[7]) {
                         Col1mJvpArgs<FT> a;
                         make_col1m_jvp_args(a, x, inv_dz, n_col * (int64_t)n_lev, n_lev, tangents, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai,
                                             precip_sno);
                         launch_column_halo<Mp1mColState<decltype(S), FT>>(c, a, s);
                     });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t vjp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                         const FT *inv_dz, const FT *const *in, const FT *const *cotangents, const FT *cot_precip_rai, const FT *cot_precip_sno, FT *const *grad,
                         FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags,
                     mp1m_column_vjp_status(flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip_rai, cot_precip_sno, grad, tendencies, precip_rai, precip_sno), in,
                     [&](const Mp1mColJacConsts<FT> &c, auto S, const FT *const (&x)[7]) {
                         using SC = decltype(S);
                         constexpr int K = kCol1mVjpK<FT, SC::general>;
                         Col1mVjpArgs<FT, K> a;
                         make_col1m_vjp_args(a, x, inv_dz, n_col * (int64_t)n_lev, n_lev, cotangents, cot_precip_rai, cot_precip_sno, grad, tendencies, precip_rai,
                                             precip_sno);
                         launch_column_point<Mp1mColState<SC, FT>, K>(c, a, s);
                     });
}

}  // namespace cmx

#define CMX_COLUMN_PRODUCTS_1M(SFX, FT)                                                                                                                               \
    int32_t cmx_mp1m_column_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                           \
                                      const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,        \
                                      int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const tangents[CMX_MP1M_JAC_NWRT],                              \
                                      FT *const jvp[CMX_MP1M_JAC_NOUT], FT *jvp_precip_rai, FT *jvp_precip_sno, FT *const tendencies[CMX_MP1M_JAC_NOUT],              \
                                      FT *precip_rai, FT *precip_sno, void *stream) {                                                                                 \
        return cmx::jvp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, tangents, jvp, jvp_precip_rai, jvp_precip_sno, tendencies,   \
                                  precip_rai, precip_sno, stream);                                                                                                    \
    }                                                                                                                                                                 \
    int32_t cmx_mp1m_column_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                           \
                                      const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,        \
                                      int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const cotangents[CMX_MP1M_JAC_NOUT],                            \
                                      const FT *cot_precip_rai, const FT *cot_precip_sno, FT *const grad[CMX_MP1M_JAC_NWRT],                                          \
                                      FT *const tendencies[CMX_MP1M_JAC_NOUT], FT *precip_rai, FT *precip_sno, void *stream) {                                        \
        return cmx::vjp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip_rai, cot_precip_sno, grad,            \
                                  tendencies, precip_rai, precip_sno, stream);                                                                                        \
    }

extern "C" {
CMX_COLUMN_PRODUCTS_1M(f32, float)
CMX_COLUMN_PRODUCTS_1M(f64, double)
}
