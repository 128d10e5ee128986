// cmx_column_implicit_step_ensemble.hip — include/cmx.h §(29): the ensemble form of the implicit column steps of §(21) (cmx_column_implicit_step.hip).
// One launch, member blockIdx.y, blockIdx.x tiling that member's columns exactly as the single kernel tiles its columns: a workgroup owns cols_per_wg whole
// columns of ONE member, a member's last workgroup fewer.  The recurrence lives inside a workgroup, so nothing can cross a member.  The packs live in
// cmx_sb2006_ensemble.hip and cmx_mp1m_ensemble.hip, the kernel-side view of the table in cmx_ensemble.hpp, the arithmetic in
// cmx_column_implicit_step_body.inc — the single kernel's own text: same operations, same operands, same bits.
//
// Where a member's values come from.  Its constants: its block of the table through the constant-address-space reference — the tendencies under the rule of
// ens_consts (Float64 and the run-time-flags 1-moment instantiation read the block phase by phase, the other Float32 instantiations get a by-value copy held
// in SGPRs, which is what the single kernel's by-value argument is; the reference to the block is formed where each eval reads it, cmx_ensemble.hpp
// EnsFrontConsts, as the single kernel forms its kernel-argument pointer there), the flux side phase by phase in both float types, as front_consts<FT, true>
// does in the single kernel.  Lv and Ls of the substeps: the block.  h, 1/h, 1/Δt, nsub, the step flags, Δt and the geometry: the kernel argument, shared.  Its columns:
// the shared pointers plus e·in_stride (inputs), e·n (outputs) and e·n_col (surface fluxes).  None of these offsets is formed before it is used: the input
// offset at the loads, the output offsets after the substeps, through the kernel-argument pointer behind consts_after — the Float64 instantiations run at
// one wave per SIMD with no register to spare, and a 64-bit offset held across the point function is two of them.
//
// One point per lane with scalar accesses: there is no alignment split (ENS_ALL only), any alignment of the columns is accepted.
// The non-temporal hint of the input loads is a WAVE-UNIFORM BRANCH on in_stride (0: a shared state, which the other members' workgroups read again), not a
// template flag: 12 kernels per float type instead of 24 of the library's most expensive ones to compile, and the branch costs no register (HISTORY.md).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "cmx_column_implicit_step_kernel.hpp"
#include "cmx_ensemble.hpp"
#include "cmx_mp1m_column_kernel.hpp"
#include "cmx_sb2006_ensemble.hpp"

namespace cmx {

// A member's block as the step reads it, per scheme (the flux side FX names the scheme)
template <typename FX> struct EnsStepBlock;
template <typename FT, bool LIMITED> struct EnsStepBlock<SbFlux<FT, LIMITED>> {
    using Block = SbEnsBlock<FT>;
    using Consts = SbConsts<FT>;
    template <typename S> static constexpr bool ALSO = false;      // scheme_consts<FT> in SbJac::eval
    static constexpr uint32_t CONSTS_AT = offsetof(Block, c);
    static __device__ __forceinline__ KernArg<Consts> &consts(KernArg<Block> &b) { return b.c; }
    static __device__ __forceinline__ FT Lv(KernArg<Block> &b) { return b.Lv; }
    static __device__ __forceinline__ FT Ls(KernArg<Block> &b) { return b.Ls; }
};
template <typename FT> struct EnsStepBlock<Mp1mFlux<FT>> {
    using Block = Mp1mColKernArgs<FT>;
    using Consts = Mp1mConsts<FT>;
    template <typename S> static constexpr bool ALSO = std::is_same_v<S, Mp1mJac<kRuntimeFlags>>;      // scheme_consts<FT, FLAGS == kRuntimeFlags> in Mp1mJac::eval
    static constexpr uint32_t CONSTS_AT = offsetof(Block, k) + offsetof(Mp1mLinKernArgs<FT>, c);
    static __device__ __forceinline__ KernArg<Consts> &consts(KernArg<Block> &b) { return b.k.c; }
    static __device__ __forceinline__ FT Lv(KernArg<Block> &b) { return b.k.a.Lv_over_cp; }
    static __device__ __forceinline__ FT Ls(KernArg<Block> &b) { return b.k.a.Ls_over_cp; }
};

// The ONE kernel argument, so that .a and .io can be read through the kernel-argument pointer after the substeps (cmx_column_implicit.hpp
// ImplicitColumnArgs, without the constants).  a.in / a.avg / io.precip hold member 0's pointers, a.Lv and a.Ls are not read.
template <typename S, typename FT, int K> struct ImplicitStepEnsArgs {
    EnsArgs ea;
    ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> a;
    ImplicitStepIO<FT> io;
};

// The ImplicitAverageArgs of one member as the body reads them: the kernel argument's own members by reference (a copy of the struct would put its index
// table into private memory) and the member's two latent-heat ratios.
template <typename FT, int NOUT, int NWRT> struct ImplicitAverageMemberArgs {
    const FT *const (&in)[NWRT + 1];
    const int32_t (&wrt)[NOUT];
    const int32_t &nsub;
    const uint32_t &step_flags;
    const FT &h, &inv_h, &inv_dt;
    FT Lv, Ls;
};

// launch bounds and waves per SIMD: those of implicit_sedimentation_step_kernel
template <typename S, typename FX, typename FT, int K, int BS>
__global__ __launch_bounds__(BS, sizeof(FT) == 4 ? 4 : 1) void implicit_sedimentation_step_ensemble_kernel(const ImplicitStepEnsArgs<S, FT, K> k0) {
    using EB = EnsStepBlock<FX>;
    constexpr bool ALSO = EB::template ALSO<S>;
    KernArg<typename EB::Block> &blk = ens_block<typename EB::Block>(k0.ea, blockIdx.y);
    // the tendency constants of the substeps: read in the block where each eval uses them (cmx_ensemble.hpp EnsFrontConsts), or the by-value copy
    const EnsFrontConsts<typename EB::Consts, EB::CONSTS_AT> ct{};
    typename EB::Consts cl{};
    if constexpr (sizeof(FT) == 4 && !ALSO) cl = ens_load(EB::consts(blk));
    const auto &tend_consts = [&]() -> decltype(auto) {
        if constexpr (sizeof(FT) == 8 || ALSO) return (ct);
        else return (cl);
    }();
    const ImplicitAverageMemberArgs<FT, S::NOUT, S::NWRT> am{k0.a.in, k0.a.wrt, k0.a.nsub, k0.a.step_flags, k0.a.h, k0.a.inv_h, k0.a.inv_dt, EB::Lv(blk), EB::Ls(blk)};
#define CMX_ISTEP_TEND_CONSTS tend_consts
#define CMX_ISTEP_FLUX_CONSTS blk
#define CMX_ISTEP_AVG_ARGS am
#define CMX_ISTEP_IO0 k0.io
#define CMX_ISTEP_ARGS_AFTER(dep) consts_after(front_consts<FT, true>(k0), dep)
#define CMX_ISTEP_IN_INDEX(i) ((i) + (int64_t)blockIdx.y * k0.ea.in_stride)
#define CMX_ISTEP_COL_ORIGIN(io) ((int64_t)blockIdx.y * (io).n_col)
#define CMX_ISTEP_NT_IN (k0.ea.in_stride != 0)
#include "cmx_column_implicit_step_body.inc"
#undef CMX_ISTEP_TEND_CONSTS
#undef CMX_ISTEP_FLUX_CONSTS
#undef CMX_ISTEP_AVG_ARGS
#undef CMX_ISTEP_IO0
#undef CMX_ISTEP_ARGS_AFTER
#undef CMX_ISTEP_IN_INDEX
#undef CMX_ISTEP_COL_ORIGIN
#undef CMX_ISTEP_NT_IN
}

// ---- host side -----------------------------------------------------------------------------------------------------
// What the two entries share after their own checks of the descriptor: the statuses 4–6 of include/cmx.h §(29), the kernel argument, the launch.
// `with_scheme(f)` calls f(scheme, flux side) for the instantiation the descriptor records and returns false for an unknown one.
template <typename FT, typename W>
static int32_t step_ensemble_launch(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, bool has_fall_speeds, double dt,
                                    int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const (&in)[7],
                                    FT *const (&out)[4], FT *precip0, FT *precip1, int32_t opt0, int32_t opt1, void *stream, W &&with_scheme) {
    if (n_col == 0) return CMX_OK;
    if (!inv_dz) return CMX_ERR_BAD_ARG;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    for (FT *p : out)
        if (!p) return CMX_ERR_BAD_ARG;
    if (!has_fall_speeds) return CMX_ERR_BAD_ARG;      // the step needs the fall-speed parameters the table was packed without
    if (!implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    const int64_t n = n_col * (int64_t)n_lev;
    const bool shared = ens_flags & CMX_ENSEMBLE_SHARED_STATE;
    const EnsArgs ea{static_cast<const unsigned char *>(table), shared ? (int64_t)0 : n, desc->stride, 1u, 0u, (int32_t)ENS_ALL};
    const ImplicitStepIO<FT> io = make_io<FT>(inv_dz, precip0, precip1, n_col, n_lev, opt0, opt1, dt);
    // grid.x as the single entry's (cmx_column_implicit_step.hip step_grid), grid.y ≤ kEnsMaxMembers (ens_check)
    const dim3 grid((unsigned)tile_grid(io.n_col, io.cols_per_wg), (unsigned)n_members);
    const bool known = with_scheme([&](auto scheme, auto fx) {
        using S = decltype(scheme);
        constexpr int K = kImplicitAvgK<FT>;
        ImplicitStepEnsArgs<S, FT, K> k{};
        k.ea = ea;
        // (Lv, Ls: zeros here — per member, from the table)
        make_implicit_average_args(k.a, in, S::SPECIES0, dt, nsub, step_flags, FT(0), FT(0), FT(1), &out[0]);
        k.io = io;
        launch_grid(implicit_sedimentation_step_ensemble_kernel<S, decltype(fx), FT, K, kImplStepBS>, grid, dim3(kImplStepBS), 0,
                    reinterpret_cast<hipStream_t>(stream), k);
    });
    if (!known) return CMX_ERR_BAD_ARG;      // unreachable: the entries check the kinds
    return launched();
}

template <typename FT>
static int32_t sb2006_step_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt, int32_t nsub,
                                          uint32_t step_flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const (&in)[7], FT *const (&out)[4],
                                          FT *precip, void *stream) {
    if (!desc || !table) return CMX_ERR_BAD_ARG;
    if (n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;      // a member's n_col·n_lev must fit what one launch of the single entry takes
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_SB2006, (uint32_t)sizeof(FT), (uint32_t)ens_stride<SbEnsBlock<FT>>())) return st;
    if (desc->vel_kind > (uint32_t)VEL_CHEN_GEN || desc->integer_exponents > 1u || desc->cloud_vel > 1u) return CMX_ERR_BAD_ARG;
    const bool limited = desc->flags & CMX_SB2006_LIMITED, intpow = desc->integer_exponents != 0;
    return step_ensemble_launch<FT>(desc, table, n_members, ens_flags, desc->vel_kind != (uint32_t)VEL_NONE, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                    precip, nullptr, (int32_t)desc->vel_kind, (int32_t)(desc->cloud_vel != 0), stream, [&](auto &&f) {
        // the instantiations of sb2006_implicit_column_entry (cmx_column_implicit.hpp)
        return dispatch([&](auto L, auto I) { f(SbJac<decltype(L)::value, decltype(I)::value>{}, SbFlux<FT, decltype(L)::value>{}); }, flag(limited), flag(intpow));
    });
}

template <typename FT>
static int32_t mp1m_step_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt, int32_t nsub,
                                        uint32_t step_flags, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *out, FT *precip_rai,
                                        FT *precip_sno, void *stream) {
    if (!desc || !table) return CMX_ERR_BAD_ARG;
    if (n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;      // a member's n_col·n_lev must fit what one launch of the single entry takes
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_MP1M, (uint32_t)sizeof(FT), (uint32_t)ens_stride<Mp1mColKernArgs<FT>>())) return st;
    if (check_flags_1m(desc->flags) || desc->runtime_flags > 1u || desc->general_gamma > 1u) return CMX_ERR_BAD_ARG;
    if (n_col == 0) return CMX_OK;
    if (!in || !out) return CMX_ERR_BAD_ARG;
    const FT *const cols[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
    FT *const outs[4] = {out[0], out[1], out[2], out[3]};
    return step_ensemble_launch<FT>(desc, table, n_members, ens_flags, desc->sedimentation != 0, dt, nsub, step_flags, n_col, n_lev, inv_dz, cols, outs, precip_rai,
                                    precip_sno, (int32_t)(desc->general_gamma != 0), 0, stream, [&](auto &&f) {
        // the instantiations of mp1m_implicit_column_entry (with_mp1m_jac: flags_1m's choice, which the pack recorded)
        return dispatch([&](auto FL) { f(Mp1mJac<decltype(FL)::value>{}, Mp1mFlux<FT>{}); },
                        one_of<kDefaultFlags, kRuntimeFlags>(desc->runtime_flags ? kRuntimeFlags : kDefaultFlags));
    });
}

}  // namespace cmx

extern "C" {

int32_t cmx_sb2006_column_implicit_step_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                     int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai,
                                                     const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
                                                     float *precip_flux, void *stream) {
    return cmx::sb2006_step_ensemble_entry<float>(desc, table, n_members, ens_flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                  {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt}, precip_flux, stream);
}
int32_t cmx_sb2006_column_implicit_step_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                     int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                                     const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                     double *precip_flux, void *stream) {
    return cmx::sb2006_step_ensemble_entry<double>(desc, table, n_members, ens_flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                   {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt}, precip_flux, stream);
}
int32_t cmx_mp1m_column_implicit_step_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                   int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *const *in,
                                                   float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::mp1m_step_ensemble_entry<float>(desc, table, n_members, ens_flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}
int32_t cmx_mp1m_column_implicit_step_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                   int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *const *in,
                                                   double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::mp1m_step_ensemble_entry<double>(desc, table, n_members, ens_flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}

}  // extern "C"
