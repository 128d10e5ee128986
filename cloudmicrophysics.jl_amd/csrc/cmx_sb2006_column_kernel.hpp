// cmx_sb2006_column_kernel.hpp — what the two forms of the fused SB2006 column step share besides the kernel body (cmx_sb2006_column_body.inc): the IO
// struct, the waves-per-SIMD requests and the lanes per workgroup.  cmx_sb2006_column.hip has the story.
#pragma once
#include "cmx_launch.hpp"
#include "cmx_sb2006.hpp"
#include "cmx_sb2006_sed.hpp"

namespace cmx {

template <typename FT> struct SbColIO {
    const FT *rho, *T, *q_tot, *q_lcl, *n_lcl, *q_rai, *n_rai;
    FT *dq_lcl, *dn_lcl, *dq_rai, *dn_rai;
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip;            // n_col values or nullptr
    int64_t n;             // n_col · n_lev
    int32_t n_lev;
    double inv_n_lev;
    FastDivU32 lev_div;    // division by n_lev for flat indices below 2³² (cmx_launch.hpp fastdiv)
};

// waves per SIMD the Float32 instantiation is compiled for: 5 (96 VGPRs) for the one-point form of rounds 2–4; the packed form holds two points' intermediates in
// register pairs and spills at 96 (2–25 VGPRs to scratch in the SB2006 / Chen instantiations): 4 (128 VGPRs)
#ifndef CMX_COL_F32_WAVES
#define CMX_COL_F32_WAVES 4
#endif
#ifndef CMX_COL_F64_WAVES
#define CMX_COL_F64_WAVES 2      // A/B switch: waves per SIMD the Float64 instantiation is compiled for
#endif

// lanes per workgroup: 256 (same-box A/B, round 4, ms per 1e8 points: Float32 64 lanes 0.884, 128 lanes 0.852, 256 lanes 0.834; Float64 2.97 / 2.72 / 2.65 —
// a longer tile halves the share of the overlap lane and of the halo traffic; profiles/r04_ab_sessions.txt, session 17)
#ifndef CMX_COLUMN_BS
#define CMX_COLUMN_BS 256
#endif
constexpr int kColBS = CMX_COLUMN_BS;

}  // namespace cmx
