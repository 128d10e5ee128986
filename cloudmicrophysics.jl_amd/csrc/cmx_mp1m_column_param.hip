// cmx_mp1m_column_param.hip — the derivatives of the 1-moment column step with sedimentation (cmx_mp1m_column.hip, Instantaneous mode) with respect to the
// PARAMETERS, the fall-speed parameters and the two precipitation fluxes included, for gfx950: C-ABI entry points cmx_mp1m_column_param_jvp_* / _param_vjp_*
// (include/cmx.h §(28)).  What loss(precip_rai + precip_sno).backward() needs to reach theta (cmx/autograd.py).  The scheme and the bodies of one point are
// cmx_mp1m_column_param.hpp's, shared with the host test build; here are the two kernels and the entries.
//
// J_θ δθ: the LDS-halo form, tiled like column1m_jvp_kernel (cmx_mp1m_column_products.hip) — lanes run along the flat index i = col·n_lev + k, workgroup b owns
// the points [b(BS−1), (b+1)(BS−1)), its lane BS−1 evaluates the first point of the next tile like any other lane and only supplies what that point sends
// down.  The halo carries the value F and the KP tangents Ḟ of every lane's four fluxes: 4·(1 + KP) values per point.  Every lane runs the same evaluation, so
// a result does not depend on where a tile boundary falls, bit for bit.
//
// Gradient: the pointwise body (column1m_param_vjp_point: λ_k needs ρ and the cotangents of the point below, read raw) feeding the deterministic reduction of
// the parameter gradients (param_vjp_chunk, param_vjp_reduce; param_vjp_finish_kernel through launch_param_vjp_finish): no atomics, no allocation.
//
// A call is a sequence of launches of kCol1mParamK or one direction each (for_each_column_param_launch), for the gradient followed by one finish launch.
// A translation unit of its own: no other kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_column_geom.hpp"
#include "cmx_launch.hpp"
#include "cmx_mp1m_column_param.hpp"

namespace cmx {

#ifndef CMX_COLPARAM1M_BS
#define CMX_COLPARAM1M_BS 256
#endif
constexpr int kColParam1mBS = CMX_COLPARAM1M_BS;

// stage 2 of the reduction: param_vjp_finish_kernel, launched by its one instantiation (cmx_sb2006_param.hip)
void launch_param_vjp_finish(int32_t ndir, const double *workspace, double *grad, hipStream_t stream);

template <typename S, typename FT, int KP, int BS>
__global__ __launch_bounds__(BS) void column1m_param_jvp_kernel(const Col1mParamConsts<FT, KP> c, const Col1mParamJvpArgs<FT, KP> a, const ColGeom geom) {
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
    Col1mParamPoint<FT, KP> p;
    if (active) {
        column_level(geom, i, col, lev);
        column1m_param_eval<S, FT, KP>(c, x, a.inv_dz[lev], p);
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
    column1m_param_jvp_store<S, FT, KP>(a, p, upv, upd, top, lev == 0, i, col);
}

// Stage 1 of the gradient: the decomposition of param_vjp_kernel (workgroup b owns the chunk [b·chunk, (b + 1)·chunk), lane t its points t, t + BS, … in index
// order), then param_vjp_reduce.
template <typename S, typename FT, int KP, int BS>
__global__ __launch_bounds__(BS) void column1m_param_vjp_kernel(const Col1mParamConsts<FT, KP> c, const Col1mParamVjpArgs<FT> a, const ColGeom geom,
                                                                const int64_t chunk, const int32_t nlive, double *__restrict__ ws) {
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
        column1m_param_vjp_point<S, FT, KP>(c, a, x, i, col, lev, acc);
    }
    param_vjp_reduce<KP, BS>(acc, nlive, ws);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The statuses both entries share, in the order of the §(27) entries and then of §(22): parameters and counts, the flags (both snow-shape bits, the option
// bits, a single snow-shape bit), the limit on n_col·n_lev, [n = 0 of the jvp entry], the columns, ndir and d_mp, [the gradient entry: grad and workspace],
// the outputs (the jvp entry: at least one) and that none is an input, then with_mp1m_column_param: finite directions, b and b_ρ of the Chen-2022 rain table.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename RUN>
static int32_t param_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                           const FT *inv_dz, const FT *const *in, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain,
                           const CI *d_chen_ice, const void *const *given, int ngiven, void *const *outs, int nouts, bool gradient, RUN &&run) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (const int32_t st = mp1m_column_jac_flags_status(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0 && !gradient) return CMX_OK;
    const FT *x[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (n > 0) {      // n = 0 of the gradient entry writes grad, so it is checked like any other call except for the columns, which it does not read
        if (!inv_dz || !in) return CMX_ERR_BAD_ARG;
        for (int j = 0; j < 7; ++j)
            if (!(x[j] = in[j])) return CMX_ERR_BAD_ARG;
    }
    if (ndir < 1 || ndir > CMX_PARAM_MAX_DIRS || !d_mp) return CMX_ERR_BAD_ARG;
    if (gradient && (!outs[nouts - 2] || !outs[nouts - 1])) return CMX_ERR_BAD_ARG;      // grad and workspace
    // outputs must not alias inputs: a lane reads its neighbours' state and cotangents
    bool any = gradient;
    for (int o = 0; o < nouts; ++o) {
        if (!outs[o]) continue;
        any = true;
        if (n > 0 && outs[o] == (const void *)inv_dz) return CMX_ERR_BAD_ARG;
        for (const FT *p : x)
            if (p && outs[o] == (const void *)p) return CMX_ERR_BAD_ARG;
        for (int g = 0; g < ngiven; ++g)
            if (outs[o] == given[g]) return CMX_ERR_BAD_ARG;
    }
    if (!any) return CMX_ERR_BAD_ARG;
    return with_mp1m_column_param<FT>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                      [&](auto S) -> int32_t { return run(S, x, n); });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t param_jvp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                               const FT *inv_dz, const FT *const *in, int32_t ndir, const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain,
                               const CI *d_chen_ice, FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno, FT *const *tendencies, FT *precip_rai,
                               FT *precip_sno, void *stream) {
    void *outs[CMX_PARAM_MAX_DIRS * 6 + 6];
    int nouts = 0;
    const int nd = ndir < 0 ? 0 : (ndir > CMX_PARAM_MAX_DIRS ? CMX_PARAM_MAX_DIRS : ndir);
    for (int q = 0; q < nd * 4 && jvp; ++q) outs[nouts++] = jvp[q];
    for (int d = 0; d < nd && jvp_precip_rai; ++d) outs[nouts++] = jvp_precip_rai[d];
    for (int d = 0; d < nd && jvp_precip_sno; ++d) outs[nouts++] = jvp_precip_sno[d];
    for (int q = 0; q < 4 && tendencies; ++q) outs[nouts++] = tendencies[q];
    outs[nouts++] = precip_rai;
    outs[nouts++] = precip_sno;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice, nullptr, 0,
                           outs, nouts, false, [&](auto S, const FT *const (&x)[7], int64_t n) -> int32_t {
                               using SC = decltype(S);
                               for_each_column_param_launch<kCol1mParamK<FT, SC::general>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   Col1mParamJvpArgs<FT, KP> a;
                                   if (!make_col1m_param_jvp_args(a, x, inv_dz, n, n_lev, d0, ndir, jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai,
                                                                  precip_sno))
                                       return;
                                   Col1mParamConsts<FT, KP> c;
                                   make_col1m_param_consts<FT, KP>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                                                   d0, ndir, c);
                                   const dim3 grid((unsigned)((n + (kColParam1mBS - 1) - 1) / (kColParam1mBS - 1))), block(kColParam1mBS);      // tiles overlap by one lane
                                   launch_grid(column1m_param_jvp_kernel<SC, FT, KP, kColParam1mBS>, grid, block, 0, s, c, a, make_col_geom(n, n_lev));
                               });
                               return launched();
                           });
}

template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t param_vjp_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int64_t n_col, int32_t n_lev,
                               const FT *inv_dz, const FT *const *in, const FT *const *cotangents, const FT *cot_precip_rai, const FT *cot_precip_sno, int32_t ndir,
                               const MP *d_mp, const TH *d_tps, const ST *d_stokes, const CH *d_chen_rain, const CI *d_chen_ice, double *grad, double *workspace,
                               FT *const *tendencies, FT *precip_rai, FT *precip_sno, void *stream) {
    static_assert(kColParam1mBS * 4 == CMX_PARAM_VJP_PARTIALS, "the finish launch gives each lane four partials");
    const void *given[6];
    void *outs[8];
    for (int q = 0; q < 4; ++q) {
        given[q] = cotangents ? cotangents[q] : nullptr;
        outs[q] = tendencies ? tendencies[q] : nullptr;
    }
    given[4] = cot_precip_rai;
    given[5] = cot_precip_sno;
    outs[4] = precip_rai;
    outs[5] = precip_sno;
    outs[6] = grad;
    outs[7] = workspace;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return param_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice, given, 6, outs,
                           8, true, [&](auto S, const FT *const (&x)[7], int64_t n) -> int32_t {
                               if (n == 0) {      // no point: the sums are zeros
                                   CMX_HIP_TRY(hipMemsetAsync(grad, 0, sizeof(double) * (size_t)ndir, s));
                                   return (int32_t)CMX_OK;
                               }
                               using SC = decltype(S);
                               const int64_t chunk = param_vjp_chunk(n, kColParam1mBS);
                               for_each_column_param_launch<kCol1mParamK<FT, SC::general>>(ndir, [&](auto K, int d0) {
                                   constexpr int KP = decltype(K)::value;
                                   Col1mParamConsts<FT, KP> c;
                                   make_col1m_param_consts<FT, KP>(*mp, *tps, *stokes, *chen_rain, *chen_ice, flags, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,
                                                                   d0, ndir, c);
                                   Col1mParamVjpArgs<FT> a;
                                   make_col1m_param_vjp_args(a, x, inv_dz, n, n_lev, cotangents, cot_precip_rai, cot_precip_sno, d0 == 0, tendencies, precip_rai,
                                                             precip_sno);
                                   const int32_t nlive = ndir - d0 < KP ? ndir - d0 : KP;
                                   launch_grid(column1m_param_vjp_kernel<SC, FT, KP, kColParam1mBS>, dim3(CMX_PARAM_VJP_PARTIALS), dim3(kColParam1mBS), 0, s, c, a,
                                               make_col_geom(n, n_lev), chunk, nlive, workspace + (int64_t)d0 * CMX_PARAM_VJP_PARTIALS);
                               });
                               launch_param_vjp_finish(ndir, workspace, grad, s);
                               return launched();
                           });
}

}  // namespace cmx

#define CMX_COLUMN_PARAM_1M(SFX, FT)                                                                                                                                   \
    int32_t cmx_mp1m_column_param_jvp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                      \
                                            const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,   \
                                            int32_t n_lev, const FT *inv_dz, const FT *const *in, int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                 \
                                            const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_stokes, const cmx_chen2022_rain_vel_##SFX *d_chen_rain,       \
                                            const cmx_chen2022_ice_vel_##SFX *d_chen_ice, FT *const *jvp, FT *const *jvp_precip_rai, FT *const *jvp_precip_sno,        \
                                            FT *const tendencies[CMX_MP1M_JAC_NOUT], FT *precip_rai, FT *precip_sno, void *stream) {                                   \
        return cmx::param_jvp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, ndir, d_mp, d_tps, d_stokes, d_chen_rain, d_chen_ice,   \
                                        jvp, jvp_precip_rai, jvp_precip_sno, tendencies, precip_rai, precip_sno, stream);                                              \
    }                                                                                                                                                                  \
    int32_t cmx_mp1m_column_param_vjp_##SFX(const cmx_microphysics_1m_##SFX *mp, const cmx_thermo_##SFX *tps, const cmx_stokes_vel_##SFX *stokes,                      \
                                            const cmx_chen2022_rain_vel_##SFX *chen_rain, const cmx_chen2022_ice_vel_##SFX *chen_ice, uint32_t flags, int64_t n_col,   \
                                            int32_t n_lev, const FT *inv_dz, const FT *const *in, const FT *const cotangents[CMX_MP1M_JAC_NOUT],                       \
                                            const FT *cot_precip_rai, const FT *cot_precip_sno, int32_t ndir, const cmx_microphysics_1m_##SFX *d_mp,                   \
                                            const cmx_thermo_##SFX *d_tps, const cmx_stokes_vel_##SFX *d_stokes, const cmx_chen2022_rain_vel_##SFX *d_chen_rain,       \
                                            const cmx_chen2022_ice_vel_##SFX *d_chen_ice, double *grad, double *workspace, FT *const tendencies[CMX_MP1M_JAC_NOUT],    \
                                            FT *precip_rai, FT *precip_sno, void *stream) {                                                                            \
        return cmx::param_vjp_entry<FT>(mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, in, cotangents, cot_precip_rai, cot_precip_sno, ndir, d_mp, \
                                        d_tps, d_stokes, d_chen_rain, d_chen_ice, grad, workspace, tendencies, precip_rai, precip_sno, stream);                        \
    }

extern "C" {
CMX_COLUMN_PARAM_1M(f32, float)
CMX_COLUMN_PARAM_1M(f64, double)
}
