// cmx_sb2006_column_products.hip — J v and Jᵀḡ of the SB2006 column step with sedimentation (cmx_sb2006_column.hip), for gfx950: C-ABI entry points
// cmx_sb2006_column_jvp_* / cmx_sb2006_column_vjp_* (include/cmx.h §(25)).  What a Newton–Krylov solver over the column needs as its matvec, and what
// loss(precip_flux).backward() needs (cmx/autograd.py).  The scheme and the bodies of one point are cmx_sb2006_column_jac.hpp's, shared with the host test
// build; here are the two kernels and the entries.
//
// J v: tiled like sb2006_column_kernel — lanes run along the flat index i = col·n_lev + k, workgroup b owns the points [b(BS−1), (b+1)(BS−1)), its lane BS−1
// evaluates the first point of the next tile like any other lane and only supplies what that point sends down.  The LDS halo carries the tangent Ḟ and the
// value F of every lane's four fluxes.  Every lane runs the same evaluation, so a result does not depend on where a tile boundary falls, bit for bit.
// One point per lane in BOTH float types: 4- / 8-byte accesses, so any alignment and any n go through ONE launch (split_aligned with vec = 1 is the single
// range [0, n), cmx_split.hpp), and the launch's last point is the top of the last column — no point follows the last tile, and no flux-only evaluation of one
// is needed.  (The packed pair and four points per lane of the primal's Float32 kernel were not built: the dual point function with the fall speeds holds
// twice the primal's intermediates; the register counts are HISTORY.md's.)
//
// Jᵀḡ: pointwise, no LDS and no barrier beyond the Float64 math tables.  λ_k needs ρ and the falling species' cotangents of the point below, read raw.
//
// A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_geom.hpp"
#include "cmx_launch.hpp"
#include "cmx_sb2006_column_jac.hpp"

namespace cmx {

#ifndef CMX_COLPROD_BS
#define CMX_COLPROD_BS 256
#endif
constexpr int kColProdBS = CMX_COLPROD_BS;

// `c`, the scheme's constants struct, stays the FIRST kernel argument: front_consts reads it at offset 0 of the kernel-argument segment.
template <typename S, typename FT, int BS>
__global__ __launch_bounds__(BS) void column_jvp_kernel(const SbConsts<FT> c, const CloudVelConsts<FT> cv, const ColJvpArgs<FT> a, const ColGeom geom) {
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
    ColJvpPoint<FT> p;
    if (active) {
        column_level(geom, i, col, lev);
        column_jvp_eval<S, FT>(c, cv, x, t, a.inv_dz[lev], p);
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
    column_jvp_store<S, FT>(a, p, upv, upd, top, lev == 0, i, col);
}

template <typename S, typename FT, int K, int BS>
__global__ __launch_bounds__(BS) void column_vjp_kernel(const SbConsts<FT> c, const CloudVelConsts<FT> cv, const ColVjpArgs<FT, K> a, const ColGeom geom) {
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
    column_vjp_point<S, FT, K>(c, cv, a, x, i, col, lev);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The one entry of both operations.  The statuses of the primal entry, in its order: parameters and counts, the flags, the limit on n_col·n_lev, n = 0, the
// columns, no output at all (`any`), an output that is an input, the limiters, the fall-speed parameters.  run(c, cv, S, n): fills the kernel's arguments and launches.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename RUN>
static int32_t entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                     const FT *const (&in)[7], const void *const *given, int ngiven, void *const *outs, int nouts, RUN &&run) {
    if (!wr || !tps || !vel || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_flags_status(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz) return CMX_ERR_BAD_ARG;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    // at least one output; outputs must not alias inputs: a lane reads its neighbours' state and cotangents
    bool any = false;
    for (int o = 0; o < nouts; ++o) {
        if (!outs[o]) continue;
        any = true;
        if (outs[o] == (const void *)inv_dz) return CMX_ERR_BAD_ARG;
        for (const FT *p : in)
            if (outs[o] == (const void *)p) return CMX_ERR_BAD_ARG;
        for (int g = 0; g < ngiven; ++g)
            if (outs[o] == given[g]) return CMX_ERR_BAD_ARG;
    }
    if (!any) return CMX_ERR_BAD_ARG;
    return with_sb2006_column_jac<FT>(*wr, *tps, *vel, cloud_vel, flags, [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S) -> int32_t {
        run(c, cv, S, n);
        return launched();
    });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t jvp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                         const FT *const (&in)[7], const FT *const *tangents, FT *const *jvp, FT *jvp_precip, FT *const *tendencies, FT *precip, void *stream) {
    const void *given[6];
    void *outs[10];
    for (int j = 0; j < 6; ++j) given[j] = tangents ? tangents[j] : nullptr;
    for (int q = 0; q < 4; ++q) {
        outs[q] = jvp ? jvp[q] : nullptr;
        outs[4 + q] = tendencies ? tendencies[q] : nullptr;
    }
    outs[8] = jvp_precip;
    outs[9] = precip;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, in, given, 6, outs, 10,
                     [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S, int64_t n) {
                         ColJvpArgs<FT> a;
                         make_col_jvp_args(a, in, inv_dz, n, n_lev, tangents, jvp, jvp_precip, tendencies, precip);
                         const dim3 grid((unsigned)((n + (kColProdBS - 1) - 1) / (kColProdBS - 1))), block(kColProdBS);      // tiles overlap by one lane
                         launch_grid(column_jvp_kernel<decltype(S), FT, kColProdBS>, grid, block, 0, s, c, cv, a, make_col_geom(n, n_lev));
                     });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t vjp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                         const FT *const (&in)[7], const FT *const *cotangents, const FT *cot_precip, FT *const *grad, FT *const *tendencies, FT *precip,
                         void *stream) {
    const void *given[5];
    void *outs[11];
    for (int q = 0; q < 4; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[4] = cot_precip;
    for (int j = 0; j < 6; ++j) outs[4 + j] = grad ? grad[j] : nullptr;
    outs[10] = precip;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return entry<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, in, given, 5, outs, 11,
                     [&](const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, auto S, int64_t n) {
                         using SC = decltype(S);
                         constexpr int K = kColVjpK<FT, SC::vel>;
                         ColVjpArgs<FT, K> a;
                         make_col_vjp_args(a, in, inv_dz, n, n_lev, cotangents, cot_precip, grad, tendencies, precip);
                         set_col_vjp_terms<SC>(a);
                         launch<kColProdBS>(column_vjp_kernel<SC, FT, K, kColProdBS>, n, s, c, cv, a, make_col_geom(n, n_lev));
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
