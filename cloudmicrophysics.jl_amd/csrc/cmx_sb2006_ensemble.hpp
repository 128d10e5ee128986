// cmx_sb2006_ensemble.hpp — one member's block of an SB2006 ensemble table (include/cmx.h §(29)): the constants of the warm-rain tendencies first, where
// the pointwise kernel reads them, then the cloud fall-speed constants of the column step.  Plain FT members only: no padding, and a block is a
// function of its member's parameters alone.
#pragma once
#include "cmx_sb2006.hpp"

namespace cmx {

template <typename FT> struct SbEnsBlock {
    SbConsts<FT> c;
    CloudVelConsts<FT> cv;      // zeros when the table was packed without cloud_vel
};

}  // namespace cmx
