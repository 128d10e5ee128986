// cmx_sb2006_column.hip — SURVEY §8f-4: the 2M warm-rain tendencies FUSED with the sedimentation step that follows them in a
// host model, one pass over the columns.
//
// What is fused.  A host model (ClimaAtmos, KinematicDriver) evaluates per time step
//   (1) tend = BMT.bulk_microphysics_tendencies(Microphysics2Moment(), …)                       BMT:820-854 → :707-782
//   (2) w_r  = CM2.rain_terminal_velocity(sb, vel, q_rai, ρ, ρ n_rai)                           CM2:685-719
//       w_c  = CM2.cloud_terminal_velocity(pdf_c, StokesRegimeVelType, q_lcl, ρ, ρ n_lcl)       CM2:647-664   (optional)
//   (3) the vertical flux divergence of the falling species with those speeds — NOT part of the reference package: it lives in
//       the host model.  The scheme built here is the one ClimaAtmos uses for precipitation, first-order upwind with the value
//       taken from the cell above ("right-biased"), on a Cartesian column:
//           F_k = ρ_k χ_k w_k   (downward flux leaving cell k through its lower face; χ = q_rai, n_rai[, q_lcl, n_lcl])
//           ∂χ_k/∂t |sed = (F_{k+1} − F_k) / (ρ_k Δz_k),    F_{n_lev} = 0 (nothing enters through the model top),
//       level 0 = lowest level; F_0 of q_rai is the surface precipitation flux [kg m⁻² s⁻¹] (optional output, one per column).
//   Unfused, (1)+(2) write 6 columns and (3) reads them back together with ρ, q_rai, n_rai and read-modify-writes two tendencies:
//   88 B/point (f32).  Fused: 7 columns in, 4 out = 44 B/point — one full HBM round trip less.
//
// Layout: n_col columns of n_lev CONTIGUOUS levels (flat index i = col·n_lev + k; a ClimaCore VF / VIJFH(Ni=Nj=1) column field).
// Lanes run along the flat index (coalesced 16-byte accesses as in the pointwise kernel); the flux of the cell above is the next
// point: inside a lane's vector it is in registers, across lanes it goes through LDS (one 16-byte row per lane), and the point
// after the workgroup's tile is evaluated by a flux-only function (rain PSD + fall speeds: the same inline code as the point
// function, hence the same bits — results, NaN propagation included, do not depend on where tile boundaries fall).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cmx_sb2006_column_kernel.hpp"

namespace cmx {

template <typename FT, bool LIMITED, int VEL, bool CLOUD, int VEC, int BS, bool INTPOW = false>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(sizeof(FT) == 4 ? CMX_COL_F32_WAVES : CMX_COL_F64_WAVES))) void sb2006_column_kernel(const SbConsts<FT> c, const CloudVelConsts<FT> cv, const SbColIO<FT> io,
                                                           const int64_t first, const int64_t nvec) {
#define CMX_SB_COL_CONSTS(ALSO) front_consts<FT, ALSO>(c)
#define CMX_SB_COL_NT_IN true
#include "cmx_sb2006_column_body.inc"
#undef CMX_SB_COL_CONSTS
#undef CMX_SB_COL_NT_IN
}

// sizes the grid of one range and picks the instantiation; false for a velocity kind the column step has no kernel for (VEL_NONE)
template <typename FT, int VEC>
static bool launch_column(bool limited, int vel, bool cloud, bool intpow, const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, const SbColIO<FT> &io,
                          int64_t first, int64_t nvec, hipStream_t s) {
    if (nvec <= 0) return true;
    const dim3 grid((unsigned)((nvec + (kColBS - 1) - 1) / (kColBS - 1))), block(kColBS);      // tiles overlap by one lane (sb2006_column_kernel)
    // I: the integer-exponent instantiation of the point function (cmx_sb2006.hpp INTPOW)
    return dispatch([&](auto L, auto K, auto C, auto I) {
        launch_grid(sb2006_column_kernel<FT, decltype(L)::value, decltype(K)::value, decltype(C)::value, VEC, kColBS, decltype(I)::value>, grid, block, 0, s, c, cv, io, first, nvec);
    }, flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(vel), flag(cloud), flag(intpow));
}

template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t column_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev,
                            const FT *inv_dz, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai,
                            const FT *n_rai, FT *dq_lcl, FT *dn_lcl, FT *dq_rai, FT *dn_rai, FT *precip, void *stream) {
    if (!wr || !tps || !vel || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(CMX_SB2006_LIMITED | CMX_VEL_SB2006 | CMX_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_VEL_SB2006, chv = flags & CMX_VEL_CHEN2022;
    if (sbv == chv) return CMX_ERR_BAD_ARG;                      // exactly one rain fall-speed scheme
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !rho || !T || !q_tot || !q_lcl || !n_lcl || !q_rai || !n_rai || !dq_lcl || !dn_lcl || !dq_rai || !dn_rai)
        return CMX_ERR_BAD_ARG;
    if ((flags & CMX_SB2006_LIMITED) && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    if (sbv && !sb_rain_vel_ok(*vel, (flags & CMX_SB2006_LIMITED) != 0)) return CMX_ERR_BAD_ARG;      // the not-limited SB2006 fall speed needs aR < bR
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, vel, (double)Math<FT>::eps_1m());
    const bool intpow = sb_integer_exponents(*wr);
    CloudVelConsts<FT> cv{};
    if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr->seifert_beheng.pdf_c, *cloud_vel);
    const SbColIO<FT> io{rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl, dn_lcl, dq_rai, dn_rai, inv_dz, precip, n, n_lev, 1.0 / (double)n_lev, make_fastdiv((uint32_t)n_lev)};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool limited = flags & CMX_SB2006_LIMITED;
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel->chen2022);   // fitted Γ(b(ρ)+1) or the general instantiation (cmx_math.hpp ChenGamma)
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;     // Float64: one point per lane, as in the pointwise kernel
    // scalar head, vector body, scalar tail (cmx_split.hpp); the halo point of each range is read from the full columns, so the launches
    // compose exactly
    const void *ptrs[] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl, dn_lcl, dq_rai, dn_rai};
    const bool cloud = cloud_vel != nullptr;
    bool known = true;
    for_each_range<FT, VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
        constexpr int V = decltype(vec_tag)::value;
        known &= launch_column<FT, V>(limited, velk, cloud, intpow, c, cv, io, lo, count / V, s);
    });
    if (!known) return CMX_ERR_BAD_ARG;      // unreachable: velk is VEL_SB or what chen_vel_kind gives
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_sb2006_column_tendencies_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                                       const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev,
                                                       const float *inv_dz, const float *rho, const float *T, const float *q_tot,
                                                       const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                                       float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
                                                       float *precip_flux, void *stream) {
    return cmx::column_entry<float>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai,
                                    dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt, precip_flux, stream);
}
int32_t cmx_sb2006_column_tendencies_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                                       const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev,
                                                       const double *inv_dz, const double *rho, const double *T, const double *q_tot,
                                                       const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                                       double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                       double *precip_flux, void *stream) {
    return cmx::column_entry<double>(warm_rain, tps, vel, cloud_vel, flags, n_col, n_lev, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai,
                                     dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt, precip_flux, stream);
}

}  // extern "C"
