// nucleation_host.cpp — TEST INFRASTRUCTURE, like point_host.cpp: the point functions of csrc/cmx_nucleation.hpp (aerosol nucleation rates and the P3
// ice-nucleation counts) with their host folding (make_nucleation_consts, make_p3_nucleation_consts) compiled by g++ for the HOST (CMX_HOST_BUILD:
// libm stand-ins for the hardware transcendental instructions), so that the algebra and the special values are checked in the CPU suite
// (tests/test_nucleation_host.py).  Not part of libcmx.so; the -m gpu suite checks the device bits.
#define CMX_HOST_BUILD 1
#include <cstdint>

#include "../../include/cmx.h"
#include "../../cloudmicrophysics.jl_amd/csrc/cmx_nucleation.hpp"

namespace {
using namespace cmx;
// out = binary, ternary, organic, mixed (any may be NULL; the inputs the requested outputs read must not be)
template <typename FT, typename HP, typename OP, typename MP>
void rates(const HP *hp, const OP *op, const MP *mp, int64_t n, const FT *const *in, FT *const *out) {
    const NucConsts<FT> c = make_nucleation_consts<FT>(hp, op, mp);
    using M = Math<FT>;
    for (int64_t i = 0; i < n; ++i) {
        const FT h = in[0] ? in[0][i] : FT(0), a = in[1] ? in[1][i] : FT(0), ion = in[2] ? in[2][i] : FT(0), mt = in[3] ? in[3][i] : FT(0);
        const FT o3 = in[4] ? in[4][i] : FT(0), oh = in[5] ? in[5][i] : FT(0), T = in[6][i], cs = in[7] ? in[7][i] : FT(1);
        FT b, t;
        if (out[0] || out[1]) {
            h2so4_rates<FT>(c, h, a, ion, T, b, t);
            if (out[0]) out[0][i] = b;
            if (out[1]) out[1][i] = t;
        }
        const FT rT = M::rcp(T), rcs = M::rcp(cs);
        if (out[2]) out[2][i] = organic_rate<FT>(c, ion, mt, o3, oh, rT, rcs);
        if (out[3]) out[3][i] = mixed_rate<FT>(c, h, mt, oh, rT, rcs);
    }
}
template <typename FT, typename OP, typename MP>
void prescribed(const OP *op, const MP *mp, int64_t n, const FT *ion, const FT *hom, const FT *h, const FT *bio, FT *organic, FT *mixed) {
    const NucConsts<FT> c = make_nucleation_consts<FT>(static_cast<const cmx_h2so4_nucleation_f64 *>(nullptr), op, mp);
    for (int64_t i = 0; i < n; ++i) {
        if (organic) organic[i] = organic_from_hom<FT>(c, ion[i], hom[i]);
        if (mixed) mixed[i] = mixed_from_bio<FT>(c, h[i], bio[i]);
    }
}
template <typename FT>
void apparent(int64_t n, const FT *od, const FT *nr, const FT *gr, const FT *cs, const FT *csi, const FT *id, FT *J) {
    for (int64_t i = 0; i < n; ++i) J[i] = apparent_rate<FT>(od[i], nr[i], gr[i], cs[i], csi[i], id ? id[i] : FT(1.7));
}
template <typename FT, typename IP>
void p3(const IP *ip, int64_t n, const FT *T, const FT *Nl, const FT *Vl, const FT *dt, FT *N_dep, FT *N_het) {
    const P3NucConsts<FT> c = make_p3_nucleation_consts<FT>(*ip);
    for (int64_t i = 0; i < n; ++i) {
        if (N_dep) N_dep[i] = p3_deposition_N_i<FT>(c, T[i]);
        if (N_het) N_het[i] = p3_het_N_i<FT>(c, T[i], Nl[i], Vl[i], dt[i]);
    }
}
}  // namespace

extern "C" {
void nuc_rates_f32(const cmx_h2so4_nucleation_f32 *hp, const cmx_organic_nucleation_f32 *op, const cmx_mixed_nucleation_f32 *mp, int64_t n,
                   const float *const *in, float *const *out) {
    rates<float>(hp, op, mp, n, in, out);
}
void nuc_rates_f64(const cmx_h2so4_nucleation_f64 *hp, const cmx_organic_nucleation_f64 *op, const cmx_mixed_nucleation_f64 *mp, int64_t n,
                   const double *const *in, double *const *out) {
    rates<double>(hp, op, mp, n, in, out);
}
void nuc_prescribed_f32(const cmx_organic_nucleation_f32 *op, const cmx_mixed_nucleation_f32 *mp, int64_t n, const float *ion, const float *hom,
                        const float *h, const float *bio, float *organic, float *mixed) {
    prescribed<float>(op, mp, n, ion, hom, h, bio, organic, mixed);
}
void nuc_prescribed_f64(const cmx_organic_nucleation_f64 *op, const cmx_mixed_nucleation_f64 *mp, int64_t n, const double *ion, const double *hom,
                        const double *h, const double *bio, double *organic, double *mixed) {
    prescribed<double>(op, mp, n, ion, hom, h, bio, organic, mixed);
}
void nuc_apparent_f32(int64_t n, const float *od, const float *nr, const float *gr, const float *cs, const float *csi, const float *id, float *J) {
    apparent<float>(n, od, nr, gr, cs, csi, id, J);
}
void nuc_apparent_f64(int64_t n, const double *od, const double *nr, const double *gr, const double *cs, const double *csi, const double *id, double *J) {
    apparent<double>(n, od, nr, gr, cs, csi, id, J);
}
void nuc_p3_f32(const cmx_morrison_milbrandt2014_f32 *ip, int64_t n, const float *T, const float *Nl, const float *Vl, const float *dt, float *N_dep,
                float *N_het) {
    p3<float>(ip, n, T, Nl, Vl, dt, N_dep, N_het);
}
void nuc_p3_f64(const cmx_morrison_milbrandt2014_f64 *ip, int64_t n, const double *T, const double *Nl, const double *Vl, const double *dt, double *N_dep,
                double *N_het) {
    p3<double>(ip, n, T, Nl, Vl, dt, N_dep, N_het);
}
}
