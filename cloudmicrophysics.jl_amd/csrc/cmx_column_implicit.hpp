// cmx_column_implicit.hpp — what the two implicit column translation units share (cmx_column_implicit_average.hip: include/cmx.h §(20);
// cmx_column_implicit_step.hip: §(21)): the flux side of each scheme, the one kernel-argument struct and the entry layer.  The kernels, their IO structs and
// launches and the extern "C" functions stay in the two files.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_mp1m_jacobian.hpp"
#include "cmx_mp1m_vel.hpp"
#include "cmx_sb2006_jacobian.hpp"
#include "cmx_sb2006_sed.hpp"

namespace cmx {

// ---- the flux side of a scheme: its constants (kernel argument KA: the tendency constants FIRST, where the scheme's eval reads them through front_consts),
// 1/ρ as the scheme's column entry forms it, and the fluxes F — for §(21) also the fall speeds w — of the four species of one raw point in the order of the
// outputs.  The flux options — rain velocity scheme, cloud sedimentation, run-time Γ — are wave-uniform run-time branches (with_options) around the existing
// flux functions' instantiations: the same inline code on the same operands, the same bits.  §(20) calls the F-only functions and §(21) the (F, w) ones (the
// operations of the F-only functions on the same operands); neither is formed from the other.
// `dep`: the value the constants wait for (consts_after).  `ka` is the kernel's by-value argument (KA) or, in the ensemble form of §(21) (include/cmx.h §(29)),
// the constant-address-space reference to a member's block of the table, which has the members a flux function reads under the same names ----------------------
// The cloud fall-speed constants as the plain reference sed_fluxes_of_point takes: the by-value kernel argument's member itself, or a copy of the table
// block's member, loaded with scalar loads where it is used (`after`: the member behind consts_after).
template <typename FT, typename TA> __device__ __forceinline__ const CloudVelConsts<FT> &plain_consts(const CloudVelConsts<FT> &direct, const TA &) { return direct; }
#if !defined(CMX_HOST_BUILD)
template <typename FT> __device__ __forceinline__ CloudVelConsts<FT> plain_consts(KernArg<CloudVelConsts<FT>> &, KernArg<CloudVelConsts<FT>> &after) {
    CloudVelConsts<FT> v;
    __builtin_memcpy(&v, &after, sizeof v);
    return v;
}
#endif
template <typename FT, bool LIMITED> struct SbFlux {
    struct KA { SbConsts<FT> c; CloudVelConsts<FT> cv; };
    static constexpr int precip(int p) { return p == 0 ? CMX_SB2006_JAC_DQ_RAI_DT : -1; }      // the species of io.precip[p], −1: none
    // sb2006_point: ρ^(-1/2) of the clamped ρ, squared
    static __device__ __forceinline__ FT inv_rho(FT rho) {
        const FT rs_rho = Math<FT>::rsqrt(max0(rho));
        return rs_rho * rs_rho;
    }
    // without cloud sedimentation q_lcl and n_lcl do not fall: their outputs are the averages themselves
    static __device__ __forceinline__ bool falls(int q, const int32_t (&opt)[2]) { return q >= CMX_SB2006_JAC_DQ_RAI_DT || opt[1] != 0; }
    // opt (velocity kind, cloud sedimentation) → g(<VEL>, <CLOUD>)
    template <typename G> static __device__ __forceinline__ void with_options(const int32_t (&opt)[2], G &&g) {
        const auto cloud = [&](auto vel) __attribute__((always_inline)) {
            if (opt[1]) g(vel, std::true_type{});
            else g(vel, std::false_type{});
        };
        if (opt[0] == VEL_SB) cloud(std::integral_constant<int, VEL_SB>{});
        else if (opt[0] == VEL_CHEN) cloud(std::integral_constant<int, VEL_CHEN>{});
        else cloud(std::integral_constant<int, VEL_CHEN_GEN>{});
    }
    static __device__ __forceinline__ void put(const SedFlux<FT> &f, FT (&F)[4]) {
        F[CMX_SB2006_JAC_DQ_LCL_DT] = f.q_lcl;
        F[CMX_SB2006_JAC_DN_LCL_DT] = f.n_lcl;
        F[CMX_SB2006_JAC_DQ_RAI_DT] = f.q_rai;
        F[CMX_SB2006_JAC_DN_RAI_DT] = f.n_rai;
    }
    // s: q_lcl, n_lcl, q_rai, n_rai
    template <typename KAT> static __device__ __forceinline__ void fluxes(const KAT &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4]) {
        const auto &kd = consts_after(front_consts<FT, true>(ka), dep);
        const auto &c = kd.c;
        decltype(auto) cv = plain_consts(ka.cv, kd.cv);
        with_options(opt, [&](auto vel, auto cloud) __attribute__((always_inline)) {
            put(sed_fluxes_of_point<FT, LIMITED, decltype(vel)::value, decltype(cloud)::value>(c, cv, rho, s[0], s[1], s[2], s[3]), F);
        });
    }
    template <typename KAT>
    static __device__ __forceinline__ void fluxes(const KAT &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4], FT (&w)[4]) {
        const auto &kd = consts_after(front_consts<FT, true>(ka), dep);
        const auto &c = kd.c;
        decltype(auto) cv = plain_consts(ka.cv, kd.cv);
        with_options(opt, [&](auto vel, auto cloud) __attribute__((always_inline)) {
            const SedFluxW<FT> f = sed_fluxes_w_of_point<FT, LIMITED, decltype(vel)::value, decltype(cloud)::value>(c, cv, rho, s[0], s[1], s[2], s[3]);
            put(f.F, F);
            put(f.w, w);
        });
    }
};

template <typename FT> struct Mp1mFlux {
    struct KA { Mp1mConsts<FT> c; Vel1mConsts<FT> vc; };
    static constexpr int precip(int p) { return p == 0 ? CMX_MP1M_JAC_DQ_RAI_DT : CMX_MP1M_JAC_DQ_SNO_DT; }
    static __device__ __forceinline__ FT inv_rho(FT rho) { return Math<FT>::rcp(max0(rho)); }
    static __device__ __forceinline__ bool falls(int, const int32_t (&)[2]) { return true; }
    // opt (run-time Γ, —) → g(<GENERAL_GAMMA>)
    template <typename G> static __device__ __forceinline__ void with_options(const int32_t (&opt)[2], G &&g) {
        if (opt[0]) g(std::true_type{});
        else g(std::false_type{});
    }
    // s: q_lcl, q_icl, q_rai, q_sno
    template <typename KAT> static __device__ __forceinline__ void fluxes(const KAT &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4]) {
        const auto &vc = consts_after(front_consts<FT, true>(ka), dep).vc;
        SedFlux4<FT> f;
        with_options(opt, [&](auto general) __attribute__((always_inline)) { f = mp1m_sed_fluxes<FT, decltype(general)::value>(vc, rho, s[0], s[1], s[2], s[3]); });
#pragma unroll
        for (int q = 0; q < 4; ++q) F[q] = f.f[q];
    }
    template <typename KAT>
    static __device__ __forceinline__ void fluxes(const KAT &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4], FT (&w)[4]) {
        const auto &vc = consts_after(front_consts<FT, true>(ka), dep).vc;
        SedFluxW4<FT> f;
        with_options(opt, [&](auto general) __attribute__((always_inline)) { f = mp1m_sed_fluxes_w<FT, decltype(general)::value>(vc, rho, s[0], s[1], s[2], s[3]); });
#pragma unroll
        for (int q = 0; q < 4; ++q) { F[q] = f.f[q]; w[q] = f.w[q]; }
    }
};

// The ONE kernel argument: the constants first (the scheme's eval and the flux functions read them at offset 0 of the kernel-argument segment), then the
// average entry's arguments, then the kernel's own IO struct (the column geometry, the flux options).  One struct, so that everything the lane needs only
// AFTER the substeps — the output pointers, the geometry, the flux options — can be read through the kernel-argument pointer at that point (consts_after)
// instead of waiting in SGPRs, and from there in VGPR lanes, across the point function: the Float64 instantiations have no register to spare.
template <typename S, typename FX, typename FT, int K, typename IO> struct ImplicitColumnArgs {
    typename FX::KA ka;
    ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> a;
    IO io;
};

// ---- the entry layer: the checks, the constants and the average entry's arguments, once for §(20) and §(21).  `launch(scheme, flux side, ka, a, opt0, opt1)`
// is the translation unit's: it builds the kernel's IO struct (opt0, opt1: its flux options), launches and returns the status ---------------------------------
// Statuses: those of cmx_sb2006_column_tendencies_sedimentation_* in its order, up to and including the columns and the limiter / fall-speed tables; then
// Δt, nsub and the step flags as the average entries check them.
template <typename FT, typename WR, typename TH, typename VL, typename ST, typename L>
inline int32_t sb2006_implicit_column_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                            int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const (&in)[7], FT *const (&out)[4], L &&launch) {
    if (!wr || !tps || !vel || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(CMX_SB2006_LIMITED | CMX_VEL_SB2006 | CMX_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_VEL_SB2006, chv = flags & CMX_VEL_CHEN2022;
    if (sbv == chv) return CMX_ERR_BAD_ARG;                      // exactly one rain fall-speed scheme
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    if (n_col == 0) return CMX_OK;
    if (!inv_dz) return CMX_ERR_BAD_ARG;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    for (FT *p : out)
        if (!p) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    if (sbv && !sb_rain_vel_ok(*vel, limited)) return CMX_ERR_BAD_ARG;      // the not-limited SB2006 fall speed needs aR < bR
    if (!implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    ImplicitAverageArgs<FT, kImplicitAvgK<FT>, CMX_SB2006_JAC_NOUT, CMX_SB2006_JAC_NWRT> a;
    make_implicit_average_args(a, in, SbJac<false, false>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, &out[0]);
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel->chen2022);   // fitted Γ(b(ρ)+1) or the general instantiation (cmx_math.hpp ChenGamma)
    // the constants of the column entry: those of the average entries (with_sb2006_jac) plus the fall-speed members, which no tendency reads
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, vel, (double)Math<FT>::eps_1m());
    CloudVelConsts<FT> cv{};
    if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr->seifert_beheng.pdf_c, *cloud_vel);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L_, auto I) -> int32_t {
        using FX = SbFlux<FT, decltype(L_)::value>;
        return launch(SbJac<decltype(L_)::value, decltype(I)::value>{}, FX{}, typename FX::KA{c, cv}, a, velk, (int32_t)(cloud_vel != nullptr));
    }, flag(limited), flag(sb_integer_exponents(*wr)));
}

// Statuses: those of cmx_mp1m_column_tendencies_sedimentation_* in its order, up to and including the columns (a single snow-shape bit, which that entry
// accepts, is CMX_ERR_UNSUPPORTED where that entry decodes the shape); then Δt, nsub and the step flags as the average entries check them.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI, typename L>
inline int32_t mp1m_implicit_column_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, double dt, int32_t nsub,
                                          uint32_t step_flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *out, L &&launch) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    const uint32_t shape_bits = flags & (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE);
    if (shape_bits == (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE)) return CMX_ERR_BAD_ARG;
    if (shape_bits) return CMX_ERR_UNSUPPORTED;
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    if (n_col == 0) return CMX_OK;
    if (!inv_dz || !in || !out) return CMX_ERR_BAD_ARG;
    for (int j = 0; j < 7; ++j)
        if (!in[j]) return CMX_ERR_BAD_ARG;
    for (int j = 0; j < 4; ++j)
        if (!out[j]) return CMX_ERR_BAD_ARG;
    if (!implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    const FT *const cols[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
    ImplicitAverageArgs<FT, kImplicitAvgK<FT>, CMX_MP1M_JAC_NOUT, CMX_MP1M_JAC_NWRT> a;
    make_implicit_average_args(a, cols, Mp1mJac<kDefaultFlags>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, out);
    bool general = false;
    Vel1mConsts<FT> vc = make_vel1m_consts<FT>(*mp, chen_rain, &general);
    add_sedimentation_consts<FT>(vc, *mp, stokes, chen_ice);
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto scheme) -> int32_t {
        using FX = Mp1mFlux<FT>;
        return launch(scheme, FX{}, typename FX::KA{c, vc}, a, (int32_t)general, 0);
    });
}

}  // namespace cmx
