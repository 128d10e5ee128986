// cmx_mp1m_ensemble.hip — include/cmx.h §(29) for the 1-moment scheme: the host-side pack of a parameter ensemble into a constants table, and the
// ensemble form of the Instantaneous tendencies (the column step: cmx_mp1m_column_ensemble.hip).  cmx_ensemble.hpp has the kernel shape.
//
// A member's block is the column kernel's constants struct, Mp1mColKernArgs (cmx_mp1m_column_kernel.hpp): the tendency constants first, where the
// pointwise kernel reads them; then the LinearizedAverage step constants, of which the table holds only what depends on the member (L_v/c_p, L_s/c_p —
// q_min, Δt and nsub are arguments of the call, shared by all members); then the fall-speed constants (zeros in a table packed without them).
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "cmx_ensemble.hpp"
#include "cmx_mp1m_column_kernel.hpp"

namespace cmx {

// Member blockIdx.y's points of one part of the alignment split, tiled by blockIdx.x: the body of mp1m_tendencies_kernel on the member's slice of the
// columns, with the member's block of the table as constants.  Launch bounds: those of mp1m_tendencies_kernel.
template <typename FT, int VEC, uint32_t FLAGS, bool NT_IN>
__global__ __launch_bounds__(kBlock1m<FT>) void mp1m_tendencies_ensemble_kernel(const EnsArgs ea, const Mp1mIn<FT> in0, const Mp1mOut<FT> out0, const int64_t n) {
    const uint32_t e = blockIdx.y;
    int64_t lo, count;
    ens_member_range(ea.part, ea.vec, ea.mis0, n, e, lo, count);
    const int64_t nvec = count / VEC;
    if ((int64_t)blockIdx.x * kBlock1m<FT> >= nvec) return;      // (the whole workgroup: a member whose part is shorter than the longest one)
    KernArg<Mp1mColKernArgs<FT>> &blk = ens_block<Mp1mColKernArgs<FT>>(ea, e);
    const int64_t oi = (int64_t)e * ea.in_stride + lo, oo = (int64_t)e * n + lo;
    const Mp1mIn<FT> in{in0.rho + oi, in0.T + oi, in0.q_tot + oi, in0.q_lcl + oi, in0.q_icl + oi, in0.q_rai + oi, in0.q_sno + oi};
    const Mp1mOut<FT> out{out0.dq_lcl + oo, out0.dq_icl + oo, out0.dq_rai + oo, out0.dq_sno + oo};
    Mp1mConsts<FT> cl{};
    if constexpr (sizeof(FT) == 4 && !(VEC == 4 || FLAGS == kRuntimeFlags)) cl = ens_load(blk.k.c);      // (the one instantiation whose body asks for by-value constants)
#define CMX_MP1M_TEND_CONSTS(ALSO) ens_consts<FT, ALSO>(blk.k.c, cl)
#define CMX_MP1M_TEND_NT_IN NT_IN
#include "cmx_mp1m_tend_body.inc"
#undef CMX_MP1M_TEND_CONSTS
#undef CMX_MP1M_TEND_NT_IN
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------------------
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t mp1m_pack_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, int32_t n_members,
                               void *table, int64_t table_bytes, cmx_ensemble_desc *desc) {
    constexpr int32_t stride = ens_stride<Mp1mColKernArgs<FT>>();
    if (!mp || !tps || !table || !desc || n_members < 1) return CMX_ERR_BAD_ARG;
    const int n_sed = (stokes != nullptr) + (chen_rain != nullptr) + (chen_ice != nullptr);
    if (n_sed != 0 && n_sed != 3) return CMX_ERR_BAD_ARG;            // the fall-speed parameters: all three or none
    // the flag checks of cmx_mp1m_column_tendencies_sedimentation_*, in its order
    const uint32_t shape_bits = flags & (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE);
    if (shape_bits == (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE)) return CMX_ERR_BAD_ARG;
    if (const int32_t st = check_flags_1m(flags & ~shape_bits)) return st;
    if (shape_bits) return CMX_ERR_UNSUPPORTED;                      // the unshaped step only
    if (table_bytes < (int64_t)n_members * stride) return CMX_ERR_BAD_ARG;
    cmx_ensemble_desc d{};
    d.magic = CMX_ENSEMBLE_MAGIC; d.scheme = CMX_ENSEMBLE_SCHEME_MP1M; d.float_type = (uint32_t)sizeof(FT); d.flags = flags;
    d.n_members = n_members; d.stride = (uint32_t)stride; d.sedimentation = n_sed == 3;
    for (int32_t e = 0; e < n_members; ++e) {
        Mp1mColKernArgs<FT> b;
        std::memset(&b, 0, sizeof b);
        // the folds of cmx_mp1m_tendencies_* / cmx_mp1m_column_tendencies_sedimentation_*
        b.k.c = make_mp1m_consts<FT>(mp[e], tps[e], flags, (double)Math<FT>::eps_1m());
        const Mp1mLinArgs<FT> la = make_mp1m_lin_args<FT>(FT(0), FT(1), 1, (FT)tps[e].LH_v0, (FT)tps[e].LH_s0, (FT)tps[e].cp_d);
        b.k.a.Lv_over_cp = la.Lv_over_cp;
        b.k.a.Ls_over_cp = la.Ls_over_cp;
        bool general = false;
        if (n_sed == 3) {
            b.vc = make_vel1m_consts<FT>(mp[e], chen_rain + e, &general);
            add_sedimentation_consts<FT>(b.vc, mp[e], stokes + e, chen_ice + e);
        }
        const uint32_t runtime = !(flags == CMX_1M_DEFAULT_OPTIONS && mp1m_default_exponents(b.k.c));      // the choice of flags_1m (cmx_mp1m.hpp)
        if (e == 0) { d.runtime_flags = runtime; d.general_gamma = general; }
        else if (d.runtime_flags != runtime || d.general_gamma != (uint32_t)general) return CMX_ERR_UNSUPPORTED;      // one instantiation per table
        unsigned char *dst = static_cast<unsigned char *>(table) + (size_t)e * stride;
        std::memset(dst, 0, stride);
        std::memcpy(dst, &b, sizeof b);
    }
    *desc = d;
    return CMX_OK;
}

// ---- the ensemble entry ----------------------------------------------------------------------------------------------------------------------
template <typename FT>
static int32_t tendencies_1m_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n, const FT *rho,
                                            const FT *T, const FT *q_tot, const FT *q_lcl, const FT *q_icl, const FT *q_rai, const FT *q_sno, FT *dq_lcl,
                                            FT *dq_icl, FT *dq_rai, FT *dq_sno, void *stream) {
    if (!desc || !table) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_MP1M, (uint32_t)sizeof(FT), (uint32_t)ens_stride<Mp1mColKernArgs<FT>>())) return st;
    if (check_flags_1m(desc->flags) || desc->runtime_flags > 1u) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if (!rho || !T || !q_tot || !q_lcl || !q_icl || !q_rai || !q_sno || !dq_lcl || !dq_icl || !dq_rai || !dq_sno) return CMX_ERR_BAD_ARG;
    const bool shared = ens_flags & CMX_ENSEMBLE_SHARED_STATE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;         // Float64: one point per lane, as in the single entry
    const void *ins[] = {rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno}, *outs[] = {dq_lcl, dq_icl, dq_rai, dq_sno};
    const int64_t in_stride = shared ? 0 : n;
    const EnsPlan plan = ens_plan<FT, VEC>(ins, 7, outs, 4, n, in_stride, n_members);
    const Mp1mIn<FT> in{rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno};
    const Mp1mOut<FT> out{dq_lcl, dq_icl, dq_rai, dq_sno};
    ens_for_each_part<VEC>(plan, n, [&](auto vec_tag, int32_t part, int64_t nvec_max) {
        constexpr int V = decltype(vec_tag)::value;
        const EnsArgs ea{static_cast<const unsigned char *>(table), in_stride, desc->stride, (uint32_t)VEC, plan.mis0, part};
        const dim3 grid((unsigned)tile_grid(nvec_max, kBlock1m<FT>), (unsigned)n_members);
        dispatch([&](auto FL, auto NT) {
            launch_grid(mp1m_tendencies_ensemble_kernel<FT, V, decltype(FL)::value, decltype(NT)::value>, grid, dim3(kBlock1m<FT>), 0, s, ea, in, out, n);
        }, one_of<kDefaultFlags, kRuntimeFlags>(desc->runtime_flags ? kRuntimeFlags : kDefaultFlags), flag(!shared));
    });
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_mp1m_ensemble_table_stride_f32(void) { return cmx::ens_stride<cmx::Mp1mColKernArgs<float>>(); }
int32_t cmx_mp1m_ensemble_table_stride_f64(void) { return cmx::ens_stride<cmx::Mp1mColKernArgs<double>>(); }

int32_t cmx_mp1m_ensemble_pack_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                   const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int32_t n_members,
                                   void *table, int64_t table_bytes, cmx_ensemble_desc *desc) {
    return cmx::mp1m_pack_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, n_members, table, table_bytes, desc);
}
int32_t cmx_mp1m_ensemble_pack_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                   const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int32_t n_members,
                                   void *table, int64_t table_bytes, cmx_ensemble_desc *desc) {
    return cmx::mp1m_pack_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, n_members, table, table_bytes, desc);
}

int32_t cmx_mp1m_tendencies_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n_points,
                                         const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai,
                                         const float *q_sno, float *dq_lcl_dt, float *dq_icl_dt, float *dq_rai_dt, float *dq_sno_dt, void *stream) {
    return cmx::tendencies_1m_ensemble_entry<float>(desc, table, n_members, ens_flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dq_lcl_dt, dq_icl_dt,
                                                    dq_rai_dt, dq_sno_dt, stream);
}
int32_t cmx_mp1m_tendencies_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n_points,
                                         const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *q_icl,
                                         const double *q_rai, const double *q_sno, double *dq_lcl_dt, double *dq_icl_dt, double *dq_rai_dt,
                                         double *dq_sno_dt, void *stream) {
    return cmx::tendencies_1m_ensemble_entry<double>(desc, table, n_members, ens_flags, n_points, rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno, dq_lcl_dt, dq_icl_dt,
                                                     dq_rai_dt, dq_sno_dt, stream);
}

}  // extern "C"
