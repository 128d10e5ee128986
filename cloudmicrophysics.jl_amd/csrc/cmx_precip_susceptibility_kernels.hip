// cmx_precip_susceptibility_kernels.hip — SB2006 precipitation susceptibilities (PrecipitationSusceptibility.jl) over columns for gfx950; C-ABI entry
// points cmx_sb2006_precip_susceptibility_* (include/cmx.h §(12)).  The point function is in cmx_precip_susceptibility.hpp.  A streaming kernel: VEC
// points per lane with 16-byte non-temporal accesses in the body of the alignment split (cmx_split.hpp), one point per lane in its head and tail — the
// same instructions per point, so the result does not depend on the split.  4 columns in, up to 6 out; which outputs are written, and which of the two
// processes is evaluated, is decided at run time from the NULL pointers (uniform branches), so there is one instantiation per float type and vector
// width.  A translation unit of its own: no existing kernel's code changes.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_math.hpp"
#include "cmx_precip_susceptibility.hpp"

namespace cmx {

template <typename FT> struct SuscIO {
    const FT *q_lcl, *q_rai, *rho, *N_lcl;
    FT *au_q_lcl, *au_q_rai, *au_N_lcl, *ac_q_lcl, *ac_q_rai, *ac_N_lcl;
};

template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void precip_susceptibility_kernel(const SuscConsts<FT> c_in, const SuscIO<FT> io, const int64_t nvec) {
    const auto &c = front_consts<FT>(c_in);     // Float64: the constants are read from the kernel-argument segment at their use
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool au = io.au_q_lcl || io.au_q_rai || io.au_N_lcl, ac = io.ac_q_lcl || io.ac_q_rai || io.ac_N_lcl;
    FT ql[VEC], qr[VEC], rho[VEC], N[VEC];
    if (i < nvec) {
        load_col<FT, VEC>(io.q_lcl, i, ql);
        load_col<FT, VEC>(io.q_rai, i, qr);
        load_col<FT, VEC>(io.rho, i, rho);
        load_col<FT, VEC>(io.N_lcl, i, N);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= nvec) return;
    FT o[6][VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const Susceptibilities<FT> s = precip_susceptibility_point<FT>(c, au, ac, ql[k], qr[k], rho[k], N[k]);
        o[0][k] = s.au_q_lcl; o[1][k] = s.au_q_rai; o[2][k] = s.au_N_lcl;
        o[3][k] = s.ac_q_lcl; o[4][k] = s.ac_q_rai; o[5][k] = s.ac_N_lcl;
    }
    if (io.au_q_lcl) store_col<FT, VEC>(io.au_q_lcl, i, o[0]);
    if (io.au_q_rai) store_col<FT, VEC>(io.au_q_rai, i, o[1]);
    if (io.au_N_lcl) store_col<FT, VEC>(io.au_N_lcl, i, o[2]);
    if (io.ac_q_lcl) store_col<FT, VEC>(io.ac_q_lcl, i, o[3]);
    if (io.ac_q_rai) store_col<FT, VEC>(io.ac_q_rai, i, o[4]);
    if (io.ac_N_lcl) store_col<FT, VEC>(io.ac_N_lcl, i, o[5]);
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <typename FT, typename AC, typename AR>
static int32_t precip_susceptibility_entry(const AC *acnv, const AR *accr, int64_t n, const FT *q_lcl, const FT *q_rai, const FT *rho, const FT *N_lcl,
                                           FT *au_q_lcl, FT *au_q_rai, FT *au_N_lcl, FT *ac_q_lcl, FT *ac_q_rai, FT *ac_N_lcl, void *stream) {
    CMX_TRY_COUNT_LIMIT(n);
    const bool au = au_q_lcl || au_q_rai || au_N_lcl, ac = ac_q_lcl || ac_q_rai || ac_N_lcl;
    if (!au && !ac) return CMX_ERR_BAD_ARG;
    if ((au && !acnv) || (ac && !accr)) return CMX_ERR_BAD_ARG;      // a NULL struct skips its process: its outputs must be NULL
    if (n == 0) return CMX_OK;
    if (!q_lcl || !q_rai || !rho || !N_lcl) return CMX_ERR_BAD_ARG;
    const SuscConsts<FT> c = make_susceptibility_consts<FT>(au ? acnv : nullptr, ac ? accr : nullptr);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const void *ptrs[] = {q_lcl, q_rai, rho, N_lcl, au_q_lcl, au_q_rai, au_N_lcl, ac_q_lcl, ac_q_rai, ac_N_lcl};
    for_each_range<FT, Math<FT>::VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {      // alignment split: cmx_split.hpp
        constexpr int V = decltype(vec_tag)::value;
        const SuscIO<FT> io{q_lcl + lo, q_rai + lo, rho + lo, N_lcl + lo, shift(au_q_lcl, lo), shift(au_q_rai, lo), shift(au_N_lcl, lo),
                            shift(ac_q_lcl, lo), shift(ac_q_rai, lo), shift(ac_N_lcl, lo)};
        const int64_t nv = count / V;
        launch<kBlock>(precip_susceptibility_kernel<FT, V>, nv, s, c, io, nv);
    });
    return launched();
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_precip_susceptibility_f32(const cmx_acnv_sb2006_f32 *acnv, const cmx_accr_sb2006_f32 *accr, int64_t n_points, const float *q_lcl,
                                             const float *q_rai, const float *rho, const float *N_lcl, float *acnv_d_ln_q_lcl, float *acnv_d_ln_q_rai,
                                             float *acnv_d_ln_N_lcl, float *accr_d_ln_q_lcl, float *accr_d_ln_q_rai, float *accr_d_ln_N_lcl, void *stream) {
    return cmx::precip_susceptibility_entry<float>(acnv, accr, n_points, q_lcl, q_rai, rho, N_lcl, acnv_d_ln_q_lcl, acnv_d_ln_q_rai, acnv_d_ln_N_lcl,
                                                   accr_d_ln_q_lcl, accr_d_ln_q_rai, accr_d_ln_N_lcl, stream);
}
int32_t cmx_sb2006_precip_susceptibility_f64(const cmx_acnv_sb2006_f64 *acnv, const cmx_accr_sb2006_f64 *accr, int64_t n_points, const double *q_lcl,
                                             const double *q_rai, const double *rho, const double *N_lcl, double *acnv_d_ln_q_lcl, double *acnv_d_ln_q_rai,
                                             double *acnv_d_ln_N_lcl, double *accr_d_ln_q_lcl, double *accr_d_ln_q_rai, double *accr_d_ln_N_lcl,
                                             void *stream) {
    return cmx::precip_susceptibility_entry<double>(acnv, accr, n_points, q_lcl, q_rai, rho, N_lcl, acnv_d_ln_q_lcl, acnv_d_ln_q_rai, acnv_d_ln_N_lcl,
                                                    accr_d_ln_q_lcl, accr_d_ln_q_rai, accr_d_ln_N_lcl, stream);
}
}
