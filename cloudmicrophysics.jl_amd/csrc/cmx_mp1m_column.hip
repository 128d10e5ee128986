// cmx_mp1m_column.hip — the OPERATIONAL 1-moment column step in one pass (SURVEY §8f-1 + §8f-4):
//   (1) tend = BMT.bulk_microphysics_tendencies(Instantaneous() | LinearizedAverage(), Microphysics1Moment(), mp, tps, ρ, T, q_tot,
//              q_lcl, q_icl, q_rai, q_sno [, Δt, nsub])                        /root/reference/src/BulkMicrophysicsTendencies.jl:505-514, 572-632
//   (2) the four bulk fall speeds a host model precomputes for sedimentation (ClimaAtmos set_sedimentation_precomputed_quantities;
//       test/gpu_clima_core_test.jl:36-45, KA kernel test/gpu_tests.jl:608-630):
//         w_lcl = CMNonEq.terminal_velocity(cloud_liquid, StokesRegimeVelType, ρ, q_lcl)       src/MicrophysicsNonEq.jl:250-265
//         w_icl = CMNonEq.terminal_velocity(cloud_ice, Chen2022VelTypeSmallIce, ρ, q_icl)      :267-281
//         w_rai = CM1.terminal_velocity(rain, Chen2022VelTypeRain, ρ, q_rai)                   src/Microphysics1M.jl:251-270
//         w_sno = CM1.terminal_velocity(snow, Chen2022VelTypeLargeIce, ρ, q_sno)               :272-297
//               … or, with a CMX_1M_SED_SNOW_* bit, (…, q_sno, CM1.Oblate() | CM1.Prolate())   :155-195, 299-324
//   (3) the host model's first-order upwind ("right-biased") flux divergence of the four falling species — NOT part of the reference
//       package (ClimaAtmos precipitation advection), the same operator as in cmx_sb2006_column.hip:
//           F_k = ρ_k χ_k w_k,   ∂χ_k/∂t |sed = (F_{k+1} − F_k)/(ρ_k Δz_k),   F_{n_lev} = 0,   level 0 = lowest level.
// Unfused that is three kernels: 7 in + 4 out, 5 in + 4 out, then 9 in + 4 read-modify-write = 148 B/point (f32); fused 44 B/point.
//
// Layout and tiling as in cmx_sb2006_column.hip: n_col columns of n_lev CONTIGUOUS levels, lanes along the flat index with 16-byte
// accesses, the flux of the cell above from the next point (registers inside a lane's vector, LDS across lanes, and for the point
// after the workgroup's tile an evaluation from the raw columns).  The fluxes of EVERY point — in the tile or after it — come from
// one function of (ρ, q_lcl, q_icl, q_rai, q_sno) only, so results do not depend on where tile boundaries fall; a NaN in ρ or in a
// species' q poisons that species' flux (and the cell below through it), a NaN in any input poisons the point's four tendencies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cmx_mp1m_column_kernel.hpp"

namespace cmx {

template <typename FT, uint32_t FLAGS, bool LIN, bool GENERAL_GAMMA, int VEC, int BS>
__global__ __launch_bounds__(BS) void mp1m_column_kernel(const Mp1mColKernArgs<FT> a0, const Mp1mColIO<FT> io, const int64_t first, const int64_t nvec) {
    constexpr bool SHAPED = false;
#define CMX_MP1M_COL_CONSTS front_consts<FT, true>(a0)
#define CMX_MP1M_COL_NSUB a0.k.a.nsub
#define CMX_MP1M_COL_LIN_ARGS(k, dep) (consts_after(k, dep).a)
#define CMX_MP1M_COL_NT_IN true
#include "cmx_mp1m_column_body.inc"
#undef CMX_MP1M_COL_CONSTS
#undef CMX_MP1M_COL_NSUB
#undef CMX_MP1M_COL_LIN_ARGS
#undef CMX_MP1M_COL_NT_IN
}
// with a snow shape (CMX_1M_SED_SNOW_*): the run-time-options instantiation only — the shape would double the kernels of the default-options
// one, a speed-up of the unshaped step whose integer exponents are not bit-identical to the run-time form
template <typename FT, bool LIN, bool GENERAL_GAMMA, int VEC, int BS>
__global__ __launch_bounds__(BS) void mp1m_column_shaped_kernel(const Mp1mColShapeKernArgs<FT> a0, const Mp1mColIO<FT> io, const int64_t first,
                                                                const int64_t nvec) {
    constexpr uint32_t FLAGS = kRuntimeFlags;
    constexpr bool SHAPED = true;
#define CMX_MP1M_COL_CONSTS front_consts<FT, true>(a0)
#define CMX_MP1M_COL_NSUB a0.k.a.nsub
#define CMX_MP1M_COL_LIN_ARGS(k, dep) (consts_after(k, dep).a)
#define CMX_MP1M_COL_NT_IN true
#include "cmx_mp1m_column_body.inc"
#undef CMX_MP1M_COL_CONSTS
#undef CMX_MP1M_COL_NSUB
#undef CMX_MP1M_COL_LIN_ARGS
#undef CMX_MP1M_COL_NT_IN
}


template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t column_1m_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, FT q_min, FT dt,
                               int32_t nsub, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *out, FT *precip_rai,
                               FT *precip_sno, void *stream) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice || n_col < 0 || n_lev < 1 || nsub < 0) return CMX_ERR_BAD_ARG;
    // the snow-shape bits belong to this entry alone: stripped before the option checks and the folding
    const uint32_t shape_bits = flags & (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE);
    if (shape_bits == (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE)) return CMX_ERR_BAD_ARG;
    const uint32_t snow_shape = shape_bits == CMX_1M_SED_SNOW_OBLATE ? CMX_SNOW_SHAPE_OBLATE : shape_bits ? CMX_SNOW_SHAPE_PROLATE : CMX_SNOW_SHAPE_ASPR;
    flags &= ~shape_bits;
    if (const int32_t st = check_flags_1m(flags)) return st;
    const bool lin = nsub > 0;
    if (lin && (!(dt > FT(0)) || !(q_min >= FT(0)))) return CMX_ERR_BAD_ARG;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !in || !out) return CMX_ERR_BAD_ARG;
    Mp1mColKernArgs<FT> a{};
    Mp1mLinKernArgs<FT> &k = a.k;
    k.c = make_mp1m_consts<FT>(*mp, *tps, flags, (double)Math<FT>::eps_1m());
    if (lin) k.a = make_mp1m_lin_args<FT>(q_min, dt, nsub, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d);
    bool general = false;
    a.vc = make_vel1m_consts<FT>(*mp, chen_rain, &general);
    add_sedimentation_consts<FT>(a.vc, *mp, stokes, chen_ice);
    Mp1mColIO<FT> io{};
    const void *ptrs[11];
    for (int j = 0; j < 7; ++j) { if (!in[j]) return CMX_ERR_BAD_ARG; io.in[j] = in[j]; ptrs[j] = in[j]; }
    for (int j = 0; j < 4; ++j) { if (!out[j]) return CMX_ERR_BAD_ARG; io.out[j] = out[j]; ptrs[7 + j] = out[j]; }
    io.inv_dz = inv_dz; io.precip_rai = precip_rai; io.precip_sno = precip_sno; io.n = n; io.n_lev = n_lev; io.inv_n_lev = 1.0 / (double)n_lev; io.lev_div = make_fastdiv((uint32_t)n_lev);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;     // Float64: one point per lane, as in the pointwise kernel
    // scalar head, vector body, scalar tail (cmx_split.hpp); the halo point of each range is read from the full columns, so the launches
    // compose exactly
    if (snow_shape != CMX_SNOW_SHAPE_ASPR) {
        Mp1mColShapeKernArgs<FT> as{};
        as.k = k;
        as.vc = make_snow_shape_consts<FT>(*mp, chen_rain, stokes, *chen_ice, snow_shape);
        for_each_range<FT, VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
            constexpr int V = decltype(vec_tag)::value;
            dispatch([&](auto LN, auto GG) {
                launch_grid(mp1m_column_shaped_kernel<FT, decltype(LN)::value, decltype(GG)::value, V, kColBS1m>, column_1m_grid(count / V), dim3(kColBS1m), 0, s, as, io, lo, count / V);
            }, flag(lin), flag(general));
        });
    } else {
        for_each_range<FT, VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
            constexpr int V = decltype(vec_tag)::value;
            dispatch([&](auto FL, auto LN, auto GG) {
                launch_grid(mp1m_column_kernel<FT, decltype(FL)::value, decltype(LN)::value, decltype(GG)::value, V, kColBS1m>, column_1m_grid(count / V), dim3(kColBS1m), 0, s, a, io, lo, count / V);
            }, flags_1m(flags, k.c), flag(lin), flag(general));
        });
    }
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_mp1m_column_tendencies_sedimentation_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                                     const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags,
                                                     float q_min, float dt, int32_t nsub, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                     const float *const *in, float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::column_1m_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, q_min, dt, nsub, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}
int32_t cmx_mp1m_column_tendencies_sedimentation_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                                     const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags,
                                                     double q_min, double dt, int32_t nsub, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                     const double *const *in, double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::column_1m_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, q_min, dt, nsub, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}

}  // extern "C"
