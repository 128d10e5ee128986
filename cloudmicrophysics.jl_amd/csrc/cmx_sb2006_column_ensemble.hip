// cmx_sb2006_column_ensemble.hip — include/cmx.h §(29): the ensemble form of the fused SB2006 column step (cmx_sb2006_column.hip).  One launch, member
// blockIdx.y; the pack lives in cmx_sb2006_ensemble.hip, the kernel shape in cmx_ensemble.hpp.
//
// Member boundaries are hard boundaries for the halo.  The kernel body sees ONE member: its SbColIO holds the member's own column bases and io.n = the
// member's n_col·n_lev, so "the point after the tile" of the member's last workgroup is index io.n — which the body never reads (it takes a zero
// inflow there, as the single entry does at the end of its arrays).  Member e + 1's first point is not loaded, let alone multiplied by zero.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cmx_ensemble.hpp"
#include "cmx_sb2006_column_kernel.hpp"
#include "cmx_sb2006_ensemble.hpp"

namespace cmx {

// launch bounds and waves per SIMD: those of sb2006_column_kernel
template <typename FT, bool LIMITED, int VEL, bool CLOUD, int VEC, int BS, bool NT_IN, bool INTPOW>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(sizeof(FT) == 4 ? CMX_COL_F32_WAVES : CMX_COL_F64_WAVES)))
void sb2006_column_ensemble_kernel(const EnsArgs ea, const SbColIO<FT> io0, const int64_t n_col) {
    const uint32_t e = blockIdx.y;
    int64_t first, count;
    ens_member_range(ea.part, ea.vec, ea.mis0, io0.n, e, first, count);
    const int64_t nvec = count / VEC;
    if ((int64_t)blockIdx.x * (BS - 1) >= nvec) return;      // (the whole workgroup: a member whose part is shorter than the longest one)
    KernArg<SbEnsBlock<FT>> &blk = ens_block<SbEnsBlock<FT>>(ea, e);
    CloudVelConsts<FT> cv;
    cv.pre_c = blk.cv.pre_c; cv.rho_w = blk.cv.rho_w; cv.K23 = blk.cv.K23; cv.K53 = blk.cv.K53;
    const int64_t oi = (int64_t)e * ea.in_stride, oo = (int64_t)e * io0.n;
    SbColIO<FT> io = io0;
    io.rho += oi; io.T += oi; io.q_tot += oi; io.q_lcl += oi; io.n_lcl += oi; io.q_rai += oi; io.n_rai += oi;
    io.dq_lcl += oo; io.dn_lcl += oo; io.dq_rai += oo; io.dn_rai += oo;
    if (io.precip) io.precip += (int64_t)e * n_col;
    SbConsts<FT> cl{};
    if constexpr (sizeof(FT) == 4) cl = ens_load(blk.c);
#define CMX_SB_COL_CONSTS(ALSO) ens_consts<FT, ALSO>(blk.c, cl)
#define CMX_SB_COL_NT_IN NT_IN
#include "cmx_sb2006_column_body.inc"
#undef CMX_SB_COL_CONSTS
#undef CMX_SB_COL_NT_IN
}

template <typename FT>
static int32_t column_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n_col, int32_t n_lev,
                                     const FT *inv_dz, const FT *rho, const FT *T, const FT *q_tot, const FT *q_lcl, const FT *n_lcl, const FT *q_rai,
                                     const FT *n_rai, FT *dq_lcl, FT *dn_lcl, FT *dq_rai, FT *dn_rai, FT *precip, void *stream) {
    if (!desc || !table || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;      // a member's n_col·n_lev must fit what one launch of the single entry takes
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_SB2006, (uint32_t)sizeof(FT), (uint32_t)ens_stride<SbEnsBlock<FT>>())) return st;
    if (desc->vel_kind > (uint32_t)VEL_CHEN_GEN || desc->integer_exponents > 1u || desc->cloud_vel > 1u) return CMX_ERR_BAD_ARG;
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !rho || !T || !q_tot || !q_lcl || !n_lcl || !q_rai || !n_rai || !dq_lcl || !dn_lcl || !dq_rai || !dn_rai) return CMX_ERR_BAD_ARG;
    if (desc->vel_kind == (uint32_t)VEL_NONE) return CMX_ERR_BAD_ARG;      // the column step needs the fall-speed parameters the table was packed without
    const bool limited = desc->flags & CMX_SB2006_LIMITED, intpow = desc->integer_exponents != 0, cloud = desc->cloud_vel != 0;
    const bool shared = ens_flags & CMX_ENSEMBLE_SHARED_STATE;
    const SbColIO<FT> io{rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl, dn_lcl, dq_rai, dn_rai, inv_dz, precip, n, n_lev, 1.0 / (double)n_lev, make_fastdiv((uint32_t)n_lev)};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;         // Float64: one point per lane, as in the single entry
    const void *ins[] = {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, *outs[] = {dq_lcl, dn_lcl, dq_rai, dn_rai};
    const int64_t in_stride = shared ? 0 : n;
    const EnsPlan plan = ens_plan<FT, VEC>(ins, 7, outs, 4, n, in_stride, n_members);
    bool known = true;
    ens_for_each_part<VEC>(plan, n, [&](auto vec_tag, int32_t part, int64_t nvec_max) {
        constexpr int V = decltype(vec_tag)::value;
        const EnsArgs ea{static_cast<const unsigned char *>(table), in_stride, desc->stride, (uint32_t)VEC, plan.mis0, part};
        const dim3 grid((unsigned)((nvec_max + (kColBS - 1) - 1) / (kColBS - 1)), (unsigned)n_members);      // tiles overlap by one lane (sb2006_column_kernel)
        known &= dispatch([&](auto L, auto K, auto C, auto I, auto NT) {
            launch_grid(sb2006_column_ensemble_kernel<FT, decltype(L)::value, decltype(K)::value, decltype(C)::value, V, kColBS, decltype(NT)::value, decltype(I)::value>,
                        grid, dim3(kColBS), 0, s, ea, io, n_col);
        }, flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>((int)desc->vel_kind), flag(cloud), flag(intpow), flag(!shared));
    });
    if (!known) return CMX_ERR_BAD_ARG;      // unreachable: the kinds were checked above
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_sb2006_column_tendencies_sedimentation_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                                int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho, const float *T,
                                                                const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai,
                                                                const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt,
                                                                float *dn_rai_dt, float *precip_flux, void *stream) {
    return cmx::column_ensemble_entry<float>(desc, table, n_members, ens_flags, n_col, n_lev, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl_dt,
                                             dn_lcl_dt, dq_rai_dt, dn_rai_dt, precip_flux, stream);
}
int32_t cmx_sb2006_column_tendencies_sedimentation_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                                int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho, const double *T,
                                                                const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                                                const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt,
                                                                double *dn_rai_dt, double *precip_flux, void *stream) {
    return cmx::column_ensemble_entry<double>(desc, table, n_members, ens_flags, n_col, n_lev, inv_dz, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, dq_lcl_dt,
                                              dn_lcl_dt, dq_rai_dt, dn_rai_dt, precip_flux, stream);
}

}  // extern "C"
