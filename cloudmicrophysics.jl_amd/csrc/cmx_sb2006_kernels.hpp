// cmx_sb2006_kernels.hpp — the fused SB2006 warm-rain device kernels (templates), shared by the C-ABI
// translation unit (cmx_sb2006_kernels.hip) and the roofline probe (tools/sb2006_probe.hip).
//
// Kernel shape: pointwise map over structure-of-arrays state columns, HBM-bound.
// One lane owns VEC consecutive points (VEC·sizeof(FT) = 16 B), so each of the 7 input columns is
// read with one global_load_dwordx4 per lane (1 KiB per wave-instruction, fully coalesced) and each
// of the 4–6 output columns written with one global_store_dwordx4; loads and stores carry the
// non-temporal hint (every byte is touched exactly once).  128-thread workgroups (kTendBS), one short-lived workgroup per
// tile (non-persistent, see below).  No LDS, no MFMA: there is no data reuse and no contraction on this path.
#pragma once
#include <hip/hip_runtime.h>

#include "cmx_launch.hpp"
#include "cmx_layout.hpp"
#include "cmx_sb2006.hpp"

namespace cmx {

template <typename FT> struct SbIn { const FT *rho, *T, *q_tot, *q_lcl, *n_lcl, *q_rai, *n_rai; };
template <typename FT> struct SbOut { FT *dq_lcl, *dn_lcl, *dq_rai, *dn_rai, *vt_n, *vt_m; };
template <typename FT> struct SbProcOut { FT *col[CMX_SB2006_NPROC]; };

// bulk_microphysics_tendencies(::Microphysics2Moment, …) over columns — BMT:820-854 + :707-782
//
// Launch shape: NON-persistent — workgroup b owns C consecutive tiles of BS lanes × VEC points, issues all of
// its 7·C vector loads up front, computes, stores, retires.  Measured on MI355X (tools/sb2006_probe, 1e8 f32
// points, 13 concurrent HBM streams): a grid-stride loop over CUs×k resident workgroups keeps every wave of the
// chip in the same load→compute→store phase and sustains only ≈59 % of the 8 TB/s peak, the same bytes moved by
// short-lived workgroups ≈70–73 % (new waves start loading while older ones store; profiles/r01_probe.txt).
// Float64 is VALU-bound (≈ 800 dependent instructions per point at 4 waves per SIMD).  A software-pipelined shape for it — a workgroup
// walking 4 or 8 tiles in a loop, tile t+1's loads issued before tile t is computed, the table copy paid once — was measured in round
// 2 and rejected: the loop carries the prefetched columns and hoisted invariants, 167–198 VGPRs against 125, 2–3 waves per SIMD
// instead of 4, 3.50 ms against 3.06 (tools/valu_probe: a dependent v_fma_f64 issues every 11 cycles; what hides that is waves).
// A scheduling fence between the points of a lane did not pay either (round 2: 0.89 vs 0.86 ms).
// CMX_SB_WAVES (A/B switch, default 1 = no request): waves per SIMD the register allocator is asked to keep for the instantiations without a Chen-2022
// velocity (they sit at 124–136 VGPRs, on either side of the 128-register step between four and three waves; the Chen variants need 200+ and are left alone)
#ifndef CMX_SB_WAVES
#define CMX_SB_WAVES 1
#endif
template <typename FT, bool LIMITED, int VEL, int VEC, int BS = kBlock, int C = 1, bool NT = true, bool INTPOW = false>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu((VEL <= VEL_SB && VEC * (int)sizeof(FT) <= 16 && C == 1) ? CMX_SB_WAVES : 1)))
void sb2006_tendencies_kernel(const SbConsts<FT> c, const SbIn<FT> in,
                                                               const SbOut<FT> out, const int64_t nvec) {
#define CMX_SB_TEND_CONSTS front_consts<FT>(c)
#define CMX_SB_TEND_NT_IN NT
#include "cmx_sb2006_tend_body.inc"
#undef CMX_SB_TEND_CONSTS
#undef CMX_SB_TEND_NT_IN
}

#ifndef CMX_TEND_BS
#define CMX_TEND_BS 128
#endif
constexpr int kTendBS = CMX_TEND_BS;   // lanes per workgroup of the fused tendency kernel (tuning: -DCMX_TEND_BS=64|256|512).  Measured with the
                                       // 263-instruction point function, 1e8 f32 points, three runs on one box: 128 → 0.883–0.885 ms, 64 → 0.887–0.902,
                                       // 512 → 0.894–0.923, 256 → 0.915–0.962 (256 was the optimum of the 350-instruction version)

// ---- host-model layouts: the VEL_NONE tendencies as a policy of the generic adapter kernel (cmx_layout.hpp) ---
template <typename FT, bool LIMITED, bool INTPOW = false> struct Sb2006LayoutPolicy {
    static constexpr int NIN = 7, NOUT = 4, NAOS = 8;       // rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai → dq_lcl, dn_lcl, dq_rai, dn_rai (+4 zero fields)
    using Consts = SbConsts<FT>;
    static constexpr bool PACKABLE = true;      // point() also takes the packed pair type (cmx_layout.hpp evaluates two points per call then)
    template <typename C, typename VT> static __device__ __forceinline__ void point(const C &c, const VT (&x)[NIN], VT (&y)[NOUT]) {
        using M = Math<VT>;
        const VT r_ = max0(x[0]), qt = max0(x[2]), ql = max0(x[3]);
        const VT nl = max0(x[4]), qr = max0(x[5]), nr = max0(x[6]);
        const SbRates<VT> p = sb2006_point<VT, LIMITED, VEL_NONE, false, INTPOW>(c, r_, x[1], qt, ql, qr, r_ * nl, r_ * nr, nl, nr);
        y[0] = (p.cond + p.au_dq_lcl) + p.ac_dq_lcl;
        y[1] = M::fma(p.lsc_plus_au + p.ac_dN_lcl, p.inv_rho, p.na_lcl);
        y[2] = (p.evq + p.au_dq_rai) + p.ac_dq_rai;
        y[3] = M::fma(((p.evN + p.au_dN_rai) + p.rsc) + p.rbr, p.inv_rho, p.na_rai);
        const VT poison = nan_mask(x[0], x[2], x[3], x[4], x[5], x[6], x[1]) ? M::nan() : VT(0);
        y[0] += poison; y[1] += poison; y[2] += poison; y[3] += poison;
    }
};

// SB2006_2M_kernel (test/gpu_tests.jl:220-235): the individual process rates, N per m³, no clamping
template <typename FT, bool LIMITED, int VEL>
__global__ __launch_bounds__(kBlock) void sb2006_process_kernel(const SbConsts<FT> c, const FT *__restrict__ q_tot,
                                                                const FT *__restrict__ q_lcl, const FT *__restrict__ q_rai,
                                                                const FT *__restrict__ N_lcl, const FT *__restrict__ N_rai,
                                                                const FT *__restrict__ rho, const FT *__restrict__ T,
                                                                const SbProcOut<FT> out, const int64_t n) {
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (no-op for Float32)
    using M = Math<FT>;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const FT r_ = rho[i];
        const FT inv_r = M::rcp(r_);
        const SbRates<FT> p = sb2006_point<FT, LIMITED, VEL>(front_consts<FT>(c), r_, T[i], q_tot[i], q_lcl[i], q_rai[i], N_lcl[i],
                                                             N_rai[i], N_lcl[i] * inv_r, N_rai[i] * inv_r);
        // NaN in → NaN out (cmx_math.hpp any_nan): the max(x, ϵ) floors of the process functions would hide it
        const FT poison = any_nan(q_tot[i], q_lcl[i], q_rai[i], N_lcl[i], N_rai[i], r_, T[i]) ? M::nan() : FT(0);
#define CMX_PUT(colid, v) if (out.col[colid]) out.col[colid][i] = (v) + poison
        CMX_PUT(CMX_SB_ACNV_DQ_LCL, p.au_dq_lcl);
        CMX_PUT(CMX_SB_ACNV_DN_LCL, p.au_dN_lcl);
        CMX_PUT(CMX_SB_ACNV_DQ_RAI, p.au_dq_rai);
        CMX_PUT(CMX_SB_ACNV_DN_RAI, p.au_dN_rai);
        CMX_PUT(CMX_SB_LCL_SELFCOL, p.lsc);
        CMX_PUT(CMX_SB_ACCR_DQ_LCL, p.ac_dq_lcl);
        CMX_PUT(CMX_SB_ACCR_DN_LCL, p.ac_dN_lcl);
        CMX_PUT(CMX_SB_ACCR_DQ_RAI, p.ac_dq_rai);
        CMX_PUT(CMX_SB_RAI_SELFCOL, p.rsc);
        CMX_PUT(CMX_SB_RAI_BREAKUP, p.rbr);
        CMX_PUT(CMX_SB_RAI_VEL_N, p.vt_n);
        CMX_PUT(CMX_SB_RAI_VEL_M, p.vt_m);
        CMX_PUT(CMX_SB_EVAP_DN_RAI, p.evN);
        CMX_PUT(CMX_SB_EVAP_DQ_RAI, p.evq);
        CMX_PUT(CMX_SB_NUMADJ_RAI, p.na_rai);
        CMX_PUT(CMX_SB_NUMADJ_LCL, p.na_lcl);
        CMX_PUT(CMX_SB_CONDEVAP, p.cond);
        // ∂rain_evaporation_∂N_rai_∂q_rai — CM2:844-855: the evaporation tendencies over N_rai / q_rai above ϵ, 0 otherwise
        CMX_PUT(CMX_SB_DEVAP_DN_RAI, N_rai[i] > M::eps() ? p.evN * M::rcp(N_rai[i]) : FT(0));
        CMX_PUT(CMX_SB_DEVAP_DQ_RAI, q_rai[i] > M::eps() ? p.evq * M::rcp(q_rai[i]) : FT(0));
#undef CMX_PUT
    }
}

}  // namespace cmx
