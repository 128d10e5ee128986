// cmx_mp1m_column_kernel.hpp — what the two forms of the 1-moment column step share besides the kernel body (cmx_mp1m_column_body.inc): the IO struct, the
// constants as one kernel argument, the lanes per workgroup and the grid.  cmx_mp1m_column.hip has the story.
#pragma once
#include "cmx_launch.hpp"
#include "cmx_mp1m.hpp"
#include "cmx_mp1m_vel.hpp"

namespace cmx {

template <typename FT> struct Mp1mColIO {
    const FT *in[7];       // rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno
    FT *out[4];            // dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip_rai, *precip_sno;   // n_col values each or nullptr: the surface fluxes F_0 of rain and snow
    int64_t n;             // n_col · n_lev
    int32_t n_lev;
    double inv_n_lev;
    FastDivU32 lev_div;    // division by n_lev for flat indices below 2³² (cmx_launch.hpp fastdiv)
};

// All constants (≈ 170 values: tendencies, LinearizedAverage step, fall speeds) travel as ONE by-value kernel argument, the first, and BOTH
// float types read them through the kernel-argument pointer (front_consts<FT, true>): as plain by-value arguments they overflow the
// SGPR file and were parked in VGPR lanes — 34 v_readlane / v_writelane per Float32 point and 143 VGPRs in the first version.
template <typename FT> struct Mp1mColKernArgs { Mp1mLinKernArgs<FT> k; Vel1mConsts<FT> vc; };
// … of the step with a snow shape (CMX_1M_SED_SNOW_*): the fall-speed constants with the shaped snow terms (cmx_mp1m_vel.hpp Vel1mShapeConsts)
template <typename FT> struct Mp1mColShapeKernArgs { Mp1mLinKernArgs<FT> k; Vel1mShapeConsts<FT> vc; };

// lanes per workgroup: 256 (same-box A/B, round 4, ms per 1e8 points: Float32 64 lanes 1.156, 128 lanes 1.140, 256 lanes 1.120; Float64 4.74 / 4.63 / 4.55;
// profiles/r04_ab_sessions.txt, session 18 — as for the SB2006 column kernel, a longer tile halves the share of the overlap lane)
#ifndef CMX_COLUMN1M_BS
#define CMX_COLUMN1M_BS 256
#endif
constexpr int kColBS1m = CMX_COLUMN1M_BS;

// the grid of one range of nvec lanes: tiles overlap by one lane
static dim3 column_1m_grid(int64_t nvec) { return dim3((unsigned)((nvec + (kColBS1m - 1) - 1) / (kColBS1m - 1))); }

}  // namespace cmx
