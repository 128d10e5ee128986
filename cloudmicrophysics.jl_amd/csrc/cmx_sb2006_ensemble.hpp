// cmx_sb2006_ensemble.hpp — one member's block of an SB2006 ensemble table (include/cmx.h §(29)): the constants of the warm-rain tendencies first, where
// the pointwise kernel reads them, then the cloud fall-speed constants of the column steps, then the two latent-heat ratios of the implicit column step's
// substeps (cmx_jacobian.hpp ImplicitAverageArgs: per member, because the thermodynamics parameters are).  Plain FT members only: no padding, and a block is
// a function of its member's parameters alone.
#pragma once
#include "cmx_sb2006.hpp"

namespace cmx {

template <typename FT> struct SbEnsBlock {
    SbConsts<FT> c;
    CloudVelConsts<FT> cv;      // zeros when the table was packed without cloud_vel
    FT Lv, Ls;                  // LH_v0/cp_d, LH_s0/cp_d as make_implicit_average_args forms them
};
static_assert(sizeof(SbEnsBlock<float>) == sizeof(SbConsts<float>) + 6 * sizeof(float) && sizeof(SbEnsBlock<double>) == sizeof(SbConsts<double>) + 6 * sizeof(double),
              "SbEnsBlock: no padding holes");

}  // namespace cmx
