// precip_susceptibility_host.cpp — TEST INFRASTRUCTURE, like nucleation_host.cpp: the point function of csrc/cmx_precip_susceptibility.hpp (SB2006
// precipitation susceptibilities) with its host folding (make_susceptibility_consts) compiled by g++ for the HOST (CMX_HOST_BUILD: libm stand-ins for
// the hardware transcendental instructions), so that the algebra, the gates and the NaN contract are checked in the CPU suite
// (tests/test_precip_susceptibility_host.py).  Not part of libcmx.so; the -m gpu suite checks the device bits.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../include/cmx.h"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_precip_susceptibility.hpp"

namespace {
using namespace cmx;
// out = the six columns in the order of the C ABI (any may be NULL); a NULL struct skips its process
template <typename FT, typename AC, typename AR>
void run(const AC *acnv, const AR *accr, int64_t n, const FT *q_lcl, const FT *q_rai, const FT *rho, const FT *N_lcl, FT *const *out) {
    const SuscConsts<FT> c = make_susceptibility_consts<FT>(acnv, accr);
    for (int64_t i = 0; i < n; ++i) {
        const Susceptibilities<FT> s = precip_susceptibility_point<FT>(c, acnv != nullptr, accr != nullptr, q_lcl[i], q_rai[i], rho[i], N_lcl[i]);
        const FT v[6] = {s.au_q_lcl, s.au_q_rai, s.au_N_lcl, s.ac_q_lcl, s.ac_q_rai, s.ac_N_lcl};
        for (int k = 0; k < 6; ++k)
            if (out[k]) out[k][i] = v[k];
    }
}
}  // namespace

extern "C" {
void precip_susceptibility_f32(const cmx_acnv_sb2006_f32 *acnv, const cmx_accr_sb2006_f32 *accr, int64_t n, const float *q_lcl, const float *q_rai,
                               const float *rho, const float *N_lcl, float *const *out) {
    run<float>(acnv, accr, n, q_lcl, q_rai, rho, N_lcl, out);
}
void precip_susceptibility_f64(const cmx_acnv_sb2006_f64 *acnv, const cmx_accr_sb2006_f64 *accr, int64_t n, const double *q_lcl, const double *q_rai,
                               const double *rho, const double *N_lcl, double *const *out) {
    run<double>(acnv, accr, n, q_lcl, q_rai, rho, N_lcl, out);
}
}
