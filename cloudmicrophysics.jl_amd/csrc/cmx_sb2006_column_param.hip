// cmx_sb2006_column_param.hip — the derivatives of the SB2006 column step with sedimentation (cmx_sb2006_column.hip) with respect to the PARAMETERS, the
// fall-speed parameters and the precipitation flux included, for gfx950: C-ABI entry points cmx_sb2006_column_param_jvp_* / _param_vjp_* (include/cmx.h
// §(26)).  What loss(precip_flux).backward() needs to reach theta (cmx/autograd.py).  The scheme and the bodies of one point are
// cmx_sb2006_column_param.hpp's, shared with the host test build; here are the two kernels and the entries.
//
// J_θ δθ: the LDS-halo form, tiled like column_jvp_kernel (cmx_sb2006_column_products.hip) — lanes run along the flat index i = col·n_lev + k, workgroup b
// owns the points [b(BS−1), (b+1)(BS−1)), its lane BS−1 evaluates the first point of the next tile like any other lane and only supplies what that point sends
// down.  The halo carries the value F and the KP tangents Ḟ of every lane's four fluxes: 4·(1 + KP) values per point.  Every lane runs the same evaluation, so
// a result does not depend on where a tile boundary falls, bit for bit.  (The alternative, a flux-only re-evaluation of the point above on duals, was not
// built: it repeats the rain PSD and both fall speeds with KP tangents for every point, where the halo costs one extra lane in 256 and at most 24 KiB of LDS
// per workgroup — below what limits the waves of kernels with these register counts.)
//
// Gradient: the pointwise body (column_param_vjp_point: λ_k needs ρ and the falling species' cotangents of the point below, read raw) feeding the
// deterministic reduction of the parameter gradients (param_vjp_chunk, param_vjp_reduce; param_vjp_finish_kernel through launch_param_vjp_finish): no atomics, no allocation.
//
// A call is a sequence of launches of kColParamK or one direction each (for_each_column_param_launch), for the gradient followed by one finish launch.
// A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_geom.hpp"
#include "cmx_launch.hpp"
#include "cmx_sb2006_column_param.hpp"

namespace cmx {

#ifndef CMX_COLPARAM_BS
#define CMX_COLPARAM_BS 256
#endif
constexpr int kColParamBS = CMX_COLPARAM_BS;

// stage 2 of the reduction: param_vjp_finish_kernel, launched by its one instantiation (cmx_sb2006_param.hip)
void launch_param_vjp_finish(int32_t ndir, const double *workspace, double *grad, hipStream_t stream);

template <typename S, typename FT, int KP, int BS, typename CD, typename CVD>
__global__ __launch_bounds__(BS) void column_param_jvp_kernel(const CD c, const CVD cv, const ColParamJvpArgs<FT, KP> a, const ColGeom geom) {
    // value and tangents of the fluxes of every lane's point: [0 … 3] F, [4(1 + k) … 4(1 + k) + 3] Ḟ of slot k
    __shared__ __align__(16) FT halo[BS][4 * (1 + KP)];
    const int64_t i = (int64_t)blockIdx.x * (BS - 1) + threadIdx.x;
    const bool active = i < a.n;
    const bool owner = threadIdx.x < BS - 1;      // lane BS−1 never stores: its point belongs to the next workgroup
    FT x[S::NWRT + 1];
    if (active) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    int64_t col = 0;
    int32_t lev = 0;
    ColParamPoint<FT, KP> p;
    if (active) {
        column_level(geom, i, col, lev);
        column_param_eval<S, FT, KP>(c, cv, x, a.inv_dz[lev], p);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            halo[threadIdx.x][s] = p.Fv[s];
#pragma unroll
            for (int k = 0; k < KP; ++k) halo[threadIdx.x][4 * (1 + k) + s] = p.Fd[k][s];
        }
    }
    __syncthreads();
    if (!active || !owner) return;
    const bool top = lev == a.n_lev - 1;
    // the cell above is the next lane's point (an owner's next lane exists in its workgroup; it is active unless this point is the launch's last, a top)
    FT upv[4] = {FT(0), FT(0), FT(0), FT(0)}, upd[KP][4];
#pragma unroll
    for (int k = 0; k < KP; ++k)
#pragma unroll
        for (int s = 0; s < 4; ++s) upd[k][s] = FT(0);
    if (!top) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            upv[s] = halo[threadIdx.x + 1][s];
#pragma unroll
            for (int k = 0; k < KP; ++k) upd[k][s] = halo[threadIdx.x + 1][4 * (1 + k) + s];
        }
    }
    column_param_jvp_store<S, FT, KP>(a, p, upv, upd, top, lev == 0, i, col);
}

// Stage 1 of the gradient: the decomposition of param_vjp_kernel (workgroup b owns the chunk [b·chunk, (b + 1)·chunk), lane t its points t, t + BS, … in index
// order), then param_vjp_reduce.
template <typename S, typename FT, int KP, int BS, typename CD, typename CVD>
__global__ __launch_bounds__(BS) void column_param_vjp_kernel(const CD c, const CVD cv, const ColParamVjpArgs<FT> a, const ColGeom geom, const int64_t chunk,
                                                              const int32_t nlive, double *__restrict__ ws) {
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < a.n ? lo + chunk : a.n;
    Math<FT>::prepare();
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int64_t i = lo + threadIdx.x; i < hi; i += BS) {
        FT x[S::NWRT + 1];
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
        int64_t col;
        int32_t lev;
        column_level(geom, i, col, lev);
        column_param_vjp_point<S, FT, KP>(c, cv, a, x, i, col, lev, acc);
    }
    param_vjp_reduce<KP, BS>(acc, nlive, ws);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses both entries share, in the order of the primal column entry and then of §(22): parameters and counts, the flags, the limit on n_col·n_lev,
// [n = 0 of the jvp entry], the columns, the direction table, the outputs (the gradient entry: grad and workspace; the other: at least one) and that none is an input, then
// with_sb2006_column_param: finite directions, the Chen-2022 table, the limiters, the fall-speed parameters.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename RUN>
static int32_t param_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                           const FT *const (&in)[7], int32_t ndir, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cloud_vel, const void *const *given,
                           int ngiven, void *const *outs, int nouts, bool gradient, RUN &&run) {
    if (!wr || !tps || !vel || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (const int32_t st = sb2006_column_flags_status(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0 && !gradient) return CMX_OK;
    if (n > 0) {      // n = 0 of the gradient entry writes grad, so it is checked like any other call except for the columns, which it does not read
        if (!inv_dz) return CMX_ERR_BAD_ARG;
        for (const FT *p : in)
            if (!p) return CMX_ERR_BAD_ARG;
    }
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_wr) return CMX_ERR_BAD_ARG;
    if (gradient && (!outs[nouts - 2] || !outs[nouts - 1])) return CMX_ERR_BAD_ARG;      // grad and workspace
    // outputs must not alias inputs: a lane reads its neighbours' state and cotangents
    bool any = gradient;
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
    return with_sb2006_column_param<FT>(*wr, *tps, *vel, cloud_vel, flags, ndir, d_wr, d_tps, d_vel, d_cloud_vel, [&](auto S) -> int32_t { return run(S, n); });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t param_jvp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                               const FT *const (&in)[7], int32_t ndir, const WR *d_wr, const TH *d_tps, const VL *d_vel, const ST *d_cloud_vel, FT *const *jvp,
                               FT *const *jvp_precip, FT *const *tendencies, FT *precip, void *stream) {
    void *outs[CMX_PARAM_MAX_DIRS * 5 + 5];
    int nouts = 0;
    const int nd = ndir < 0 ? 0 : (ndir > CMX_PARAM_MAX_DIRS ? CMX_PARAM_MAX_DIRS : ndir);
    for (int q = 0; q < nd * 4 && jvp; ++q) outs[nouts++] = jvp[q];
    for (int d = 0; d < nd && jvp_precip; ++d) outs[nouts++] = jvp_precip[d];
    for (int q = 0; q < 4 && tendencies; ++q) outs[nouts++] = tendencies[q];
    outs[nouts++] = precip;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, in, ndir, d_wr, d_tps, d_vel, d_cloud_vel, nullptr, 0, outs, nouts, false,
                           [&](auto S, int64_t n) -> int32_t {
                               using SC = decltype(S);
                               for_each_column_param_launch<kColParamK<FT, SC::vel>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   using CD = SbConsts<Dual<FT, KP>>;
                                   using CVD = CloudVelConsts<Dual<FT, KP>>;
                                   CD cd;
                                   CVD cvd;
                                   make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cloud_vel, d0, ndir, cd, cvd);
                                   ColParamJvpArgs<FT, KP> a;
                                   if (!make_column_param_jvp_args(a, in, inv_dz, n, n_lev, d0, ndir, jvp, jvp_precip, tendencies, precip)) return;
                                   const dim3 grid((unsigned)((n + (kColParamBS - 1) - 1) / (kColParamBS - 1))), block(kColParamBS);      // tiles overlap by one lane
                                   launch_grid(column_param_jvp_kernel<SC, FT, KP, kColParamBS, CD, CVD>, grid, block, 0, s, cd, cvd, a, make_col_geom(n, n_lev));
                               });
                               return launched();
                           });
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t param_vjp_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz,
                               const FT *const (&in)[7], const FT *const *cotangents, const FT *cot_precip, int32_t ndir, const WR *d_wr, const TH *d_tps,
                               const VL *d_vel, const ST *d_cloud_vel, double *grad, double *workspace, FT *const *tendencies, FT *precip, void *stream) {
    static_assert(kColParamBS * 4 == CMX_PARAM_VJP_PARTIALS, "the finish launch gives each lane four partials");
    const void *given[5];
    void *outs[7];
    for (int q = 0; q < 4; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[4] = cot_precip;
    outs[4] = precip;
    outs[5] = grad;
    outs[6] = workspace;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(wr, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, in, ndir, d_wr, d_tps, d_vel, d_cloud_vel, given, 5, outs, 7, true,
                           [&](auto S, int64_t n) -> int32_t {
                               if (n == 0) {      // no point: the sums are zeros
                                   CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
                                   return (int32_t)CMX_OK;
                               }
                               using SC = decltype(S);
                               // the Float64 gradient kernel of the general Chen-2022 instantiation (run-time Γ) needs 482–511 VGPRs at one direction per
                               // evaluation and spills 8: not shipped (cmx_sb2006_column_param.hpp has the table)
                               if constexpr (sizeof(FT) == 8 && SC::vel == VEL_CHEN_GEN) return (int32_t)CMX_ERR_UNSUPPORTED;
                               else {
                               const int64_t chunk = param_vjp_chunk(n, kColParamBS);
                               for_each_column_param_launch<kColParamK<FT, SC::vel>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   using CD = SbConsts<Dual<FT, KP>>;
                                   using CVD = CloudVelConsts<Dual<FT, KP>>;
                                   CD cd;
                                   CVD cvd;
                                   make_column_param_consts<FT, KP>(*wr, *tps, *vel, cloud_vel, d_wr, d_tps, d_vel, d_cloud_vel, d0, ndir, cd, cvd);
                                   ColParamVjpArgs<FT> a;
                                   make_column_param_vjp_args<SC>(a, in, inv_dz, n, n_lev, cotangents, cot_precip, d0 == 0, tendencies, precip);
                                   const int32_t nlive = ndir - d0 < KP ? ndir - d0 : KP;
                                   launch_grid(column_param_vjp_kernel<SC, FT, KP, kColParamBS, CD, CVD>, dim3(CMX_PARAM_VJP_PARTIALS), dim3(kColParamBS), 0, s, cd,
                                               cvd, a, make_col_geom(n, n_lev), chunk, nlive, workspace + (int64_t)d0 * CMX_PARAM_VJP_PARTIALS);
                               });
                               launch_param_vjp_finish(ndir, workspace, grad, s);
                               return launched();
                               }
                           });
}

}  // namespace cmx

#define CMX_COLUMN_PARAM(SFX, FT)                                                                                                                                      \
    int32_t cmx_sb2006_column_param_jvp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                     \
                                              const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,    \
                                              const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai, int32_t ndir,          \
                                              const cmx_warm_rain_2m_##SFX *d_warm_rain, const cmx_thermo_##SFX *d_tps, const cmx_rain_vel_##SFX *d_vel,               \
                                              const cmx_stokes_vel_##SFX *d_cloud_vel, FT *const *jvp, FT *const *jvp_precip,                                          \
                                              FT *const tendencies[CMX_SB2006_JAC_NOUT], FT *precip_flux, void *stream) {                                              \
        return cmx::param_jvp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, ndir, d_warm_rain,   \
                                        d_tps, d_vel, d_cloud_vel, jvp, jvp_precip, tendencies, precip_flux, stream);                                                  \
    }                                                                                                                                                                  \
    int32_t cmx_sb2006_column_param_vjp_##SFX(const cmx_warm_rain_2m_##SFX *warm_rain, const cmx_thermo_##SFX *tps, const cmx_rain_vel_##SFX *vel,                     \
                                              const cmx_stokes_vel_##SFX *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *rho,    \
                                              const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai,                        \
                                              const FT *const cotangents[CMX_SB2006_JAC_NOUT], const FT *cot_precip, int32_t ndir,                                     \
                                              const cmx_warm_rain_2m_##SFX *d_warm_rain, const cmx_thermo_##SFX *d_tps, const cmx_rain_vel_##SFX *d_vel,               \
                                              const cmx_stokes_vel_##SFX *d_cloud_vel, double *grad, double *workspace, FT *const tendencies[CMX_SB2006_JAC_NOUT],     \
                                              FT *precip_flux, void *stream) {                                                                                         \
        return cmx::param_vjp_entry<FT>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, cotangents,          \
                                        cot_precip, ndir, d_warm_rain, d_tps, d_vel, d_cloud_vel, grad, workspace, tendencies, precip_flux, stream);                   \
    }

extern "C" {
CMX_COLUMN_PARAM(f32, float)
CMX_COLUMN_PARAM(f64, double)
}
