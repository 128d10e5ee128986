// cmx_mp1m_column_products.hip — J v and Jᵀḡ of the 1-moment column step with sedimentation (cmx_mp1m_column.hip, Instantaneous mode), for gfx950: C-ABI
// entry points cmx_mp1m_column_jvp_* / cmx_mp1m_column_vjp_* (include/cmx.h §(27)).  What a Newton–Krylov solver over a mixed-phase column needs as its
// matvec, and what loss(precip_rai + precip_sno).backward() needs (cmx/autograd.py).  The scheme and the bodies of one point are cmx_mp1m_column_jac.hpp's,
// shared with the host test build; here are the two kernels and the entries.  The shape is that of cmx_sb2006_column_products.hip:
//
// J v: lanes run along the flat index i = col·n_lev + k, workgroup b owns the points [b(BS−1), (b+1)(BS−1)), its lane BS−1 evaluates the first point of the
// next tile like any other lane and only supplies what that point sends down.  The LDS halo carries the value F and the tangent Ḟ of every lane's four fluxes.
// Every lane runs the same evaluation, so a result does not depend on where a tile boundary falls, bit for bit.  One point per lane in BOTH float types: 4- /
// 8-byte accesses, so any alignment and any n go through ONE launch, and the launch's last point is the top of the last column — no point follows the last tile.
//
// Jᵀḡ: pointwise, no LDS and no barrier beyond the Float64 math tables.  λ_k needs ρ and the cotangents of the point below, read raw.
//
// A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_geom.hpp"
#include "cmx_launch.hpp"
#include "cmx_mp1m_column_jac.hpp"

namespace cmx {

#ifndef CMX_COLPROD1M_BS
#define CMX_COLPROD1M_BS 256
#endif
constexpr int kColProd1mBS = CMX_COLPROD1M_BS;

// `c`, the scheme's constants struct, stays the FIRST kernel argument: front_consts reads it at offset 0 of the kernel-argument segment.
template <typename S, typename FT, int BS>
__global__ __launch_bounds__(BS) void column1m_jvp_kernel(const Mp1mColJacConsts<FT> c, const Col1mJvpArgs<FT> a, const ColGeom geom) {
    // value and tangent of the fluxes of every lane's point: [0 … 3] F, [4 … 7] Ḟ
    __shared__ __align__(16) FT halo[BS][8];
    const int64_t i = (int64_t)blockIdx.x * (BS - 1) + threadIdx.x;
    const bool active = i < a.n;
    const bool owner = threadIdx.x < BS - 1;      // lane BS−1 never stores: its point belongs to the next workgroup
    FT x[S::NWRT + 1], t[S::NWRT];
    if (active) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
#pragma unroll
        for (int j = 0; j < S::NWRT; ++j) t[j] = a.tan[j] ? __builtin_nontemporal_load(a.tan[j] + i) : FT(0);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    int64_t col = 0;
    int32_t lev = 0;
    Col1mJvpPoint<FT> p;
    if (active) {
        column_level(geom, i, col, lev);
        column1m_jvp_eval<S, FT>(c, x, t, a.inv_dz[lev], p);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            halo[threadIdx.x][s] = p.Fv[s];
            halo[threadIdx.x][4 + s] = p.Fd[s];
        }
    }
    __syncthreads();
    if (!active || !owner) return;
    const bool top = lev == a.n_lev - 1;
    // the cell above is the next lane's point (an owner's next lane exists in its workgroup; it is active unless this point is the launch's last, a top)
    FT upv[4] = {FT(0), FT(0), FT(0), FT(0)}, upd[4] = {FT(0), FT(0), FT(0), FT(0)};
    if (!top) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            upv[s] = halo[threadIdx.x + 1][s];
            upd[s] = halo[threadIdx.x + 1][4 + s];
        }
    }
    column1m_jvp_store<S, FT>(a, p, upv, upd, top, lev == 0, i, col);
}

template <typename S, typename FT, int K, int BS>
__global__ __launch_bounds__(BS) void column1m_vjp_kernel(const Mp1mColJacConsts<FT> c, const Col1mVjpArgs<FT, K> a, const ColGeom geom) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < a.n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= a.n) return;
    int64_t col;
    int32_t lev;
    column_level(geom, i, col, lev);
    column1m_vjp_point<S, FT, K>(c, a, x, i, col, lev);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of both operations.  The statuses of the primal entry, in its order: parameters and counts, the flags (then this entry's own: a snow-shape
// bit), the limit on n_col·n_lev, n = 0, the columns, no output at all, an output that is an input.  run(a, S, n): fills the kernel's arguments and launches.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename RUN>
static int32_t entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                     const FT *inv_dz, const FT *const *in, const void *const *given, int ngiven, void *const *outs, int nouts, RUN &&run) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (const int32_t st = mp1m_column_jac_flags_status(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !in) return CMX_ERR_BAD_ARG;
    const FT *const x[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
    for (const FT *p : x)
        if (!p) return CMX_ERR_BAD_ARG;
    // at least one output; outputs must not alias inputs: a lane reads its neighbours' state and cotangents
    bool any = false;
    for (int o = 0; o < nouts; ++o) {
        if (!outs[o]) continue;
        any = true;
        if (outs[o] == (const void *)inv_dz) return CMX_ERR_BAD_ARG;
        for (const FT *p : x)
            if (outs[o] == (const void *)p) return CMX_ERR_BAD_ARG;
        for (int g = 0; g < ngiven; ++g)
            if (outs[o] == given[g]) return CMX_ERR_BAD_ARG;
    }
    if (!any) return CMX_ERR_BAD_ARG;
    return with_mp1m_column_jac<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, [&](const Mp1mColJacConsts<FT> &a, auto S) -> int32_t {
        run(a, S, x, n);
        return launched();
    });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t jvp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                         const FT *inv_dz, const FT *const *in, const FT *const *tangents, FT *const *jvp, FT *jvp_precip_rai, FT *jvp_precip_sno,
                         FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    const void *given[6];
    void *outs[12];
    for (int j = 0; j < 6; ++j) given[j] = tangents ? tangents[j] : nullptr;
    for (int q = 0; q < 4; ++q) {
        outs[q] = jvp ? jvp[q] : nullptr;
        outs[4 + q] = tendencies ? tendencies[q] : nullptr;
    }
    outs[8] = jvp_precip_rai;
    outs[9] = jvp_precip_sno;
    outs[10] = precip_rai;
    outs[11] = precip_sno;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, given, 6, outs, 12,
                     [&](const Mp1mColJacConsts<FT> &c, auto S, const FT *const (&x)[7], int64_t n) {
                         Col1mJvpArgs<FT> a;
                         make_col1m_jvp_args(a, x, inv_dz, n, n_lev, tangents, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai, precip_sno);
                         const dim3 grid((unsigned)((n + (kColProd1mBS - 1) - 1) / (kColProd1mBS - 1))), block(kColProd1mBS);      // tiles overlap by one lane
                         launch_grid(column1m_jvp_kernel<decltype(S), FT, kColProd1mBS>, grid, block, 0, s, c, a, make_col_geom(n, n_lev));
                     });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t vjp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                         const FT *inv_dz, const FT *const *in, const FT *const *cotangents, const FT *cot_precip_rai, const FT *cot_precip_sno, FT *const *grad,
                         FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    const void *given[6];
    void *outs[12];
    for (int q = 0; q < 4; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[4] = cot_precip_rai;
    given[5] = cot_precip_sno;
    for (int j = 0; j < 6; ++j) outs[4 + j] = grad ? grad[j] : nullptr;
    outs[10] = precip_rai;
    outs[11] = precip_sno;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, given, 6, outs, 12,
                     [&](const Mp1mColJacConsts<FT> &c, auto S, const FT *const (&x)[7], int64_t n) {
                         using SC = decltype(S);
                         constexpr int K = kCol1mVjpK<FT, SC::general>;
                         Col1mVjpArgs<FT, K> a;
                         make_col1m_vjp_args(a, x, inv_dz, n, n_lev, cotangents, cot_precip_rai, cot_precip_sno, grad, tendencies, precip_rai, precip_sno);
                         launch<kColProd1mBS>(column1m_vjp_kernel<SC, FT, K, kColProd1mBS>, n, s, c, a, make_col_geom(n, n_lev));
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
