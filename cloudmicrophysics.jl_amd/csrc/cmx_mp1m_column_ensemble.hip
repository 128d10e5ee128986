// cmx_mp1m_column_ensemble.hip — include/cmx.h §(29): the ensemble form of the unshaped 1-moment column step (cmx_mp1m_column.hip).  One launch, member
// blockIdx.y; the pack lives in cmx_mp1m_ensemble.hip, the kernel shape in cmx_ensemble.hpp.
//
// Member boundaries are hard boundaries for the halo, as in cmx_sb2006_column_ensemble.hip: the kernel body sees ONE member — its Mp1mColIO holds the
// member's own column bases and io.n = the member's n_col·n_lev, so the point after the member's last tile is index io.n, which the body never reads.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cmx_ensemble.hpp"
#include "cmx_mp1m_column_kernel.hpp"

namespace cmx {

// lin0: the LinearizedAverage step constants every member shares (q_min, Δt, nsub and what follows from them); L_v/c_p and L_s/c_p come from the member's
// block.  Launch bounds: those of mp1m_column_kernel.
template <typename FT, uint32_t FLAGS, bool LIN, bool GENERAL_GAMMA, int VEC, int BS, bool NT_IN>
__global__ __launch_bounds__(BS) void mp1m_column_ensemble_kernel(const EnsArgs ea, const Mp1mColIO<FT> io0, const Mp1mLinArgs<FT> lin0, const int64_t n_col) {
    constexpr bool SHAPED = false;
    const uint32_t e = blockIdx.y;
    int64_t first, count;
    ens_member_range(ea.part, ea.vec, ea.mis0, io0.n, e, first, count);
    const int64_t nvec = count / VEC;
    if ((int64_t)blockIdx.x * (BS - 1) >= nvec) return;      // (the whole workgroup: a member whose part is shorter than the longest one)
    KernArg<Mp1mColKernArgs<FT>> &blk = ens_block<Mp1mColKernArgs<FT>>(ea, e);
    Mp1mLinArgs<FT> lin = lin0;
    if constexpr (LIN) { lin.Lv_over_cp = blk.k.a.Lv_over_cp; lin.Ls_over_cp = blk.k.a.Ls_over_cp; }
    const int64_t oi = (int64_t)e * ea.in_stride, oo = (int64_t)e * io0.n;
    Mp1mColIO<FT> io = io0;
#pragma unroll
    for (int j = 0; j < 7; ++j) io.in[j] += oi;
#pragma unroll
    for (int j = 0; j < 4; ++j) io.out[j] += oo;
    if (io.precip_rai) io.precip_rai += (int64_t)e * n_col;
    if (io.precip_sno) io.precip_sno += (int64_t)e * n_col;
#define CMX_MP1M_COL_CONSTS blk
#define CMX_MP1M_COL_NSUB lin0.nsub
#define CMX_MP1M_COL_LIN_ARGS(k, dep) (lin)
#define CMX_MP1M_COL_NT_IN NT_IN
#include "cmx_mp1m_column_body.inc"
#undef CMX_MP1M_COL_CONSTS
#undef CMX_MP1M_COL_NSUB
#undef CMX_MP1M_COL_LIN_ARGS
#undef CMX_MP1M_COL_NT_IN
}

template <typename FT>
static int32_t column_1m_ensemble_entry(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, FT q_min, FT dt, int32_t nsub,
                                        int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *out, FT *precip_rai, FT *precip_sno,
                                        void *stream) {
    if (!desc || !table || n_col < 0 || n_lev < 1 || nsub < 0) return CMX_ERR_BAD_ARG;
    const bool lin = nsub > 0;
    if (lin && (!(dt > FT(0)) || !(q_min >= FT(0)))) return CMX_ERR_BAD_ARG;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;      // a member's n_col·n_lev must fit what one launch of the single entry takes
    if (const int32_t st = ens_check(desc, n_members, ens_flags, CMX_ENSEMBLE_SCHEME_MP1M, (uint32_t)sizeof(FT), (uint32_t)ens_stride<Mp1mColKernArgs<FT>>())) return st;
    if (check_flags_1m(desc->flags) || desc->runtime_flags > 1u || desc->general_gamma > 1u) return CMX_ERR_BAD_ARG;
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !in || !out) return CMX_ERR_BAD_ARG;
    if (!desc->sedimentation) return CMX_ERR_BAD_ARG;                // the column step needs the fall-speed parameters the table was packed without
    Mp1mLinArgs<FT> la{};
    if (lin) la = make_mp1m_lin_args<FT>(q_min, dt, nsub, FT(0), FT(1), FT(1));      // (the two latent-heat ratios: per member, from the table)
    Mp1mColIO<FT> io{};
    const void *ins[7], *outs[4];
    for (int j = 0; j < 7; ++j) { if (!in[j]) return CMX_ERR_BAD_ARG; io.in[j] = in[j]; ins[j] = in[j]; }
    for (int j = 0; j < 4; ++j) { if (!out[j]) return CMX_ERR_BAD_ARG; io.out[j] = out[j]; outs[j] = out[j]; }
    io.inv_dz = inv_dz; io.precip_rai = precip_rai; io.precip_sno = precip_sno; io.n = n; io.n_lev = n_lev; io.inv_n_lev = 1.0 / (double)n_lev; io.lev_div = make_fastdiv((uint32_t)n_lev);
    const bool shared = ens_flags & CMX_ENSEMBLE_SHARED_STATE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    constexpr int VEC = sizeof(FT) == 8 ? 1 : Math<FT>::VEC;         // Float64: one point per lane, as in the single entry
    const int64_t in_stride = shared ? 0 : n;
    const EnsPlan plan = ens_plan<FT, VEC>(ins, 7, outs, 4, n, in_stride, n_members);
    ens_for_each_part<VEC>(plan, n, [&](auto vec_tag, int32_t part, int64_t nvec_max) {
        constexpr int V = decltype(vec_tag)::value;
        const EnsArgs ea{static_cast<const unsigned char *>(table), in_stride, desc->stride, (uint32_t)VEC, plan.mis0, part};
        const dim3 grid(column_1m_grid(nvec_max).x, (unsigned)n_members);
        dispatch([&](auto FL, auto LN, auto GG, auto NT) {
            launch_grid(mp1m_column_ensemble_kernel<FT, decltype(FL)::value, decltype(LN)::value, decltype(GG)::value, V, kColBS1m, decltype(NT)::value>, grid,
                        dim3(kColBS1m), 0, s, ea, io, la, n_col);
        }, one_of<kDefaultFlags, kRuntimeFlags>(desc->runtime_flags ? kRuntimeFlags : kDefaultFlags), flag(lin), flag(desc->general_gamma != 0), flag(!shared));
    });
    return launched();
}

}  // namespace cmx

extern "C" {

int32_t cmx_mp1m_column_tendencies_sedimentation_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                              float q_min, float dt, int32_t nsub, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                              const float *const *in, float *const *out, float *precip_rai, float *precip_sno,
                                                              void *stream) {
    return cmx::column_1m_ensemble_entry<float>(desc, table, n_members, ens_flags, q_min, dt, nsub, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}
int32_t cmx_mp1m_column_tendencies_sedimentation_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                              double q_min, double dt, int32_t nsub, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                              const double *const *in, double *const *out, double *precip_rai, double *precip_sno,
                                                              void *stream) {
    return cmx::column_1m_ensemble_entry<double>(desc, table, n_members, ens_flags, q_min, dt, nsub, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}

}  // extern "C"
