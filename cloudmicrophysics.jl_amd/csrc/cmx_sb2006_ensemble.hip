// cmx_sb2006_ensemble.hip — include/cmx.h §(29) for the SB2006 scheme: the host-side pack of a parameter ensemble into a constants table, and the
// ensemble form of the fused warm-rain tendencies (the column step: cmx_sb2006_column_ensemble.hip).  cmx_ensemble.hpp has the kernel shape.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "cmx_ensemble.hpp"
#include "cmx_sb2006_ensemble.hpp"
#include "cmx_sb2006_kernels.hpp"

namespace cmx {

// Member blockIdx.y's points of one part of the alignment split, tiled by blockIdx.x: the body of sb2006_tendencies_kernel on the member's slice of the
// columns, with the member's block of the table as constants.  Launch bounds and the waves-per-SIMD request are those of sb2006_tendencies_kernel.
// NT_IN: the input loads keep the non-temporal hint in the member-major layout only (a shared state is re-read by the other members' workgroups).
template <typename FT, bool LIMITED, int VEL, int VEC, int BS, bool NT_IN, bool INTPOW>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu((VEL <= VEL_SB && VEC * (int)sizeof(FT) <= 16) ? CMX_SB_WAVES : 1)))
void sb2006_tendencies_ensemble_kernel(const EnsArgs ea, const SbIn<FT> in0, const SbOut<FT> out0, const int64_t n) {
    constexpr int C = 1;
    constexpr bool NT = true;
    const uint32_t e = blockIdx.y;
    int64_t lo, count;
    ens_member_range(ea.part, ea.vec, ea.mis0, n, e, lo, count);
    const int64_t nvec = count / VEC;
    if ((int64_t)blockIdx.x * BS >= nvec) return;      // (the whole workgroup: a member whose part is shorter than the longest one)
    KernArg<SbEnsBlock<FT>> &blk = ens_block<SbEnsBlock<FT>>(ea, e);
    const int64_t oi = (int64_t)e * ea.in_stride + lo, oo = (int64_t)e * n + lo;
    const SbIn<FT> in{in0.rho + oi, in0.T + oi, in0.q_tot + oi, in0.q_lcl + oi, in0.n_lcl + oi, in0.q_rai + oi, in0.n_rai + oi};
    const SbOut<FT> out{out0.dq_lcl + oo, out0.dn_lcl + oo, out0.dq_rai + oo, out0.dn_rai + oo, out0.vt_n ? out0.vt_n + oo : nullptr,
                        out0.vt_m ? out0.vt_m + oo : nullptr};
    SbConsts<FT> cl{};
    if constexpr (sizeof(FT) == 4) cl = ens_load(blk.c);
#define CMX_SB_TEND_CONSTS ens_consts<FT, false>(blk.c, cl)
#define CMX_SB_TEND_NT_IN NT_IN
#include "cmx_sb2006_tend_body.inc"
#undef CMX_SB_TEND_CONSTS
#undef CMX_SB_TEND_NT_IN
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------------------
template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t sb_pack_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, int32_t n_members, void *table,
                             int64_t table_bytes, cmx_ensemble_desc *desc) {
    constexpr int32_t stride = ens_stride<SbEnsBlock<FT>>();
    if (!wr || !tps || !table || !desc || n_members < 1) return CMX_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(CMX_SB2006_LIMITED | CMX_VEL_SB2006 | CMX_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    if (table_bytes < (int64_t)n_members * stride) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_VEL_SB2006, chv = flags & CMX_VEL_CHEN2022;
    if (vel && sbv == chv) return CMX_ERR_BAD_ARG;                   // with fall-speed parameters: exactly one scheme
    const bool limited = flags & CMX_SB2006_LIMITED;
    cmx_ensemble_desc d{};
    d.magic = CMX_ENSEMBLE_MAGIC; d.scheme = CMX_ENSEMBLE_SCHEME_SB2006; d.float_type = (uint32_t)sizeof(FT); d.flags = flags;
    d.n_members = n_members; d.stride = (uint32_t)stride; d.cloud_vel = cloud_vel != nullptr;
    for (int32_t e = 0; e < n_members; ++e) {
        // the checks and folds of cmx_sb2006_warm_rain_tendencies_* / cmx_sb2006_column_tendencies_sedimentation_*, in their order
        int velk = !vel ? VEL_NONE : sbv ? VEL_SB : chen_vel_kind<FT>(vel[e].chen2022);
        if (limited && !sb_limiters_ok(wr[e])) return CMX_ERR_BAD_ARG;
        if (velk == VEL_SB && !sb_rain_vel_ok(vel[e], limited)) return CMX_ERR_BAD_ARG;
        const uint32_t intpow = sb_integer_exponents(wr[e]);
        if (e == 0) { d.vel_kind = (uint32_t)velk; d.integer_exponents = intpow; }
        else if (d.vel_kind != (uint32_t)velk || d.integer_exponents != intpow) return CMX_ERR_UNSUPPORTED;      // one instantiation per table
        SbEnsBlock<FT> b;
        std::memset(&b, 0, sizeof b);
        b.c = make_sb_consts<FT>(wr[e], tps[e], vel ? vel + e : (const VL *)nullptr, (double)Math<FT>::eps_1m());
        if (cloud_vel) b.cv = make_cloud_vel_consts<FT>(wr[e].seifert_beheng.pdf_c, cloud_vel[e]);
        b.Lv = (FT)tps[e].LH_v0 / (FT)tps[e].cp_d;      // the expressions of make_implicit_average_args (cmx_jacobian.hpp)
        b.Ls = (FT)tps[e].LH_s0 / (FT)tps[e].cp_d;
        unsigned char *dst = static_cast<unsigned char *>(table) + (size_t)e * stride;
        std::memset(dst, 0, stride);
        std::memcpy(dst, &b, sizeof b);
    }
    *desc = d;
    return CMX_OK;
}

// ---- the ensemble entry ----------------------------------------------------------------------------------------------------------------------
template <typename FT>
static int32_t tendencies_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n, const FT *rho,
                                         const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai, const FT *n_rai, FT *dq_lcl,
                                         FT *dn_lcl, FT *dq_rai, FT *dn_rai, FT *vt_n, FT *vt_m, void *stream) {
    if (!desc || !table) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_SB2006, (uint32_t)sizeof(FT), (uint32_t)ens_stride<SbEnsBlock<FT>>())) return st;
    if (desc->vel_kind > (uint32_t)VEL_CHEN_GEN || desc->integer_exponents > 1u) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if (!rho || !T || !q_tot || !q_lcl || !n_lcl || !q_rai || !n_rai || !dq_lcl || !dn_lcl || !dq_rai || !dn_rai) return CMX_ERR_BAD_ARG;
    const bool want_vel = vt_n || vt_m;
    if (want_vel && desc->vel_kind == (uint32_t)VEL_NONE) return CMX_ERR_BAD_ARG;      // the table was packed without fall-speed parameters
    const int velk = want_vel ? (int)desc->vel_kind : VEL_NONE;      // as the single entry: no fall-speed output, no fall-speed instantiation
    const bool limited = desc->flags & CMX_SB2006_LIMITED, intpow = desc->integer_exponents != 0, shared = ens_flags & CMX_ENSEMBLE_SHARED_STATE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;         // Float64: one point per lane, as in the single entry
    const void *ins[] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, *outs[] = {dq_lcl, dn_lcl, dq_rai, dn_rai, vt_n, vt_m};
    const int64_t in_stride = shared ? 0 : n;
    const EnsPlan plan = ens_plan<FT, VEC>(ins, 7, outs, 6, n, in_stride, n_members);
    const SbIn<FT> in{rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai};
    const SbOut<FT> out{dq_lcl, dn_lcl, dq_rai, dn_rai, vt_n, vt_m};
    bool known = true;
    ens_for_each_part<VEC>(plan, n, [&](auto vec_tag, int32_t part, int64_t nvec_max) {
        constexpr int V = decltype(vec_tag)::value;
        const EnsArgs ea{static_cast<const unsigned char *>(table), in_stride, desc->stride, (uint32_t)VEC, plan.mis0, part};
        const dim3 grid((unsigned)tile_grid(nvec_max, kTendBS), (unsigned)n_members);
        known &= dispatch([&](auto L, auto K, auto I, auto NT) {
            launch_grid(sb2006_tendencies_ensemble_kernel<FT, decltype(L)::value, decltype(K)::value, V, kTendBS, decltype(NT)::value, decltype(I)::value>, grid,
                        dim3(kTendBS), 0, s, ea, in, out, n);
        }, flag(limited), one_of<VEL_NONE, VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(velk), flag(intpow), flag(!shared));
    });
    if (!known) return CMX_ERR_BAD_ARG;      // unreachable: the kinds were checked above
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_sb2006_ensemble_table_stride_f32(void) { return cmx::ens_stride<cmx::SbEnsBlock<float>>(); }
int32_t cmx_sb2006_ensemble_table_stride_f64(void) { return cmx::ens_stride<cmx::SbEnsBlock<double>>(); }

int32_t cmx_sb2006_ensemble_pack_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                     const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int32_t n_members, void *table, int64_t table_bytes,
                                     cmx_ensemble_desc *desc) {
    return cmx::sb_pack_entry<float>(warm_rain, tps, vel, cloud_vel, flags, n_members, table, table_bytes, desc);
}
int32_t cmx_sb2006_ensemble_pack_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                     const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int32_t n_members, void *table, int64_t table_bytes,
                                     cmx_ensemble_desc *desc) {
    return cmx::sb_pack_entry<double>(warm_rain, tps, vel, cloud_vel, flags, n_members, table, table_bytes, desc);
}

int32_t cmx_sb2006_warm_rain_tendencies_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                     int64_t n_points, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                                     const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt,
                                                     float *dq_rai_dt, float *dn_rai_dt, float *vt_rai_n, float *vt_rai_m, void *stream) {
    return cmx::tendencies_ensemble_entry<float>(desc, table, n_members, ens_flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl_dt, dn_lcl_dt,
                                                 dq_rai_dt, dn_rai_dt, vt_rai_n, vt_rai_m, stream);
}
int32_t cmx_sb2006_warm_rain_tendencies_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                     int64_t n_points, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                                     const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt,
                                                     double *dq_rai_dt, double *dn_rai_dt, double *vt_rai_n, double *vt_rai_m, void *stream) {
    return cmx::tendencies_ensemble_entry<double>(desc, table, n_members, ens_flags, n_points, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl_dt, dn_lcl_dt,
                                                  dq_rai_dt, dn_rai_dt, vt_rai_n, vt_rai_m, stream);
}

}  // extern "C"
