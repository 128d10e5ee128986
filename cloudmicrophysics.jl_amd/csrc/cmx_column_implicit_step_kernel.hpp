// cmx_column_implicit_step_kernel.hpp — what the implicit column step (cmx_column_implicit_step.hip, include/cmx.h §(21)) and its ensemble form
// (cmx_column_implicit_step_ensemble.hip, §(29)) share besides the kernel body (cmx_column_implicit_step_body.inc): the tuning numbers, the kernel's IO
// struct and how the host fills it.
#pragma once
#include "cmx_column_implicit.hpp"

namespace cmx {

#ifndef CMX_IMPLICIT_STEP_BS
#define CMX_IMPLICIT_STEP_BS 256
#endif
#ifndef CMX_IMPLICIT_STEP_CHUNKS
#define CMX_IMPLICIT_STEP_CHUNKS 4      // a workgroup owns about this many chunks of points (whole columns; one column if it is longer)
#endif
constexpr int kImplStepBS = CMX_IMPLICIT_STEP_BS;

template <typename FT> struct ImplicitStepIO {
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip[2];         // n_col values each or nullptr: the surface fluxes G_0 of the species FX::precip(0), FX::precip(1)
    int64_t n_col;
    int32_t n_lev;
    int32_t cols_per_wg;   // cols_per_wg · n_lev < 2³¹
    int32_t opt[2];        // the flux options of the scheme (velocity kind, cloud sedimentation; run-time Γ)
    FT dt;                 // FT(Δt)
    FastDivU32 lev_div;    // division by n_lev (cmx_launch.hpp fastdiv)
};

// whole columns per workgroup: about CMX_IMPLICIT_STEP_CHUNKS chunks of points, at least one column
static int32_t columns_per_workgroup(int32_t n_lev) {
    const int32_t m = CMX_IMPLICIT_STEP_CHUNKS * kImplStepBS / n_lev;
    return m < 1 ? 1 : m;
}

template <typename FT>
static ImplicitStepIO<FT> make_io(const FT *inv_dz, FT *precip0, FT *precip1, int64_t n_col, int32_t n_lev, int32_t opt0, int32_t opt1, double dt) {
    ImplicitStepIO<FT> io{};
    io.inv_dz = inv_dz;
    io.precip[0] = precip0;
    io.precip[1] = precip1;
    io.n_col = n_col;
    io.n_lev = n_lev;
    io.cols_per_wg = columns_per_workgroup(n_lev);
    io.opt[0] = opt0;
    io.opt[1] = opt1;
    io.dt = (FT)dt;
    io.lev_div = make_fastdiv((uint32_t)n_lev);
    return io;
}

}  // namespace cmx
