// cmx_nucleation_kernels.hip — aerosol nucleation rates (Nucleation.jl) and the P3 ice-nucleation counts over columns for gfx950; C-ABI entry points
// cmx_aerosol_nucleation_rates_*, cmx_nucleation_rates_prescribed_*, cmx_apparent_nucleation_rate_*, cmx_p3_ice_nucleation_counts_* (include/cmx.h §(11)).
// The point functions are in cmx_nucleation.hpp.  Streaming kernels: VEC points per lane with 16-byte non-temporal accesses in the body of the alignment
// split (cmx_split.hpp), one point per lane in its head and tail — the same instructions per point, so the result does not depend on the split.  A
// column that no requested output reads is not loaded.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_math.hpp"
#include "cmx_nucleation.hpp"

namespace cmx {

template <typename FT> struct NucIO {
    const FT *h2so4, *nh3, *ion, *mt, *o3, *oh, *T, *cs;
    FT *binary, *ternary, *organic, *mixed;
};

// the fused pass: up to 8 columns in, 4 out (48 B/point in f32)
template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void aerosol_nucleation_kernel(const NucConsts<FT> c_in, const NucIO<FT> io, const int64_t nvec) {
    const auto &c = front_consts<FT>(c_in);     // Float64: the constants are read from the kernel-argument segment at their use
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool wb = io.binary, wt = io.ternary, wo = io.organic, wm = io.mixed, wh = wb || wt, wom = wo || wm;
    FT h[VEC], a[VEC], ion[VEC], mt[VEC], o3[VEC], oh[VEC], T[VEC], cs[VEC];
    if (i < nvec) {
        load_col<FT, VEC>(io.T, i, T);
        if (wh || wm) load_col<FT, VEC>(io.h2so4, i, h);
        if (wh) load_col<FT, VEC>(io.nh3, i, a);
        if (wh || wo) load_col<FT, VEC>(io.ion, i, ion);
        if (wom) {
            load_col<FT, VEC>(io.mt, i, mt);
            load_col<FT, VEC>(io.oh, i, oh);
            load_col<FT, VEC>(io.cs, i, cs);
        }
        if (wo) load_col<FT, VEC>(io.o3, i, o3);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= nvec) return;
    FT ob[VEC], ot[VEC], oo[VEC], om[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        ob[k] = ot[k] = oo[k] = om[k] = FT(0);
        if (wh) h2so4_rates<FT>(c, h[k], a[k], ion[k], T[k], ob[k], ot[k]);
        if (wom) {
            const FT rT = Math<FT>::rcp(T[k]), rcs = Math<FT>::rcp(cs[k]);     // shared by the organic and the mixed rate
            if (wo) oo[k] = organic_rate<FT>(c, ion[k], mt[k], o3[k], oh[k], rT, rcs);
            if (wm) om[k] = mixed_rate<FT>(c, h[k], mt[k], oh[k], rT, rcs);
        }
    }
    if (wb) store_col<FT, VEC>(io.binary, i, ob);
    if (wt) store_col<FT, VEC>(io.ternary, i, ot);
    if (wo) store_col<FT, VEC>(io.organic, i, oo);
    if (wm) store_col<FT, VEC>(io.mixed, i, om);
}

template <typename FT> struct NucPrescribedIO { const FT *ion, *hom, *h2so4, *bio; FT *organic, *mixed; };

template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void nucleation_prescribed_kernel(const NucConsts<FT> c_in, const NucPrescribedIO<FT> io, const int64_t nvec) {
    const auto &c = front_consts<FT>(c_in);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool wo = io.organic, wm = io.mixed;
    FT ion[VEC], hom[VEC], h[VEC], bio[VEC];
    if (i < nvec) {
        if (wo) {
            load_col<FT, VEC>(io.ion, i, ion);
            load_col<FT, VEC>(io.hom, i, hom);
        }
        if (wm) {
            load_col<FT, VEC>(io.h2so4, i, h);
            load_col<FT, VEC>(io.bio, i, bio);
        }
    }
    Math<FT>::prepare();
    if (i >= nvec) return;
    FT oo[VEC], om[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        oo[k] = wo ? organic_from_hom<FT>(c, ion[k], hom[k]) : FT(0);
        om[k] = wm ? mixed_from_bio<FT>(c, h[k], bio[k]) : FT(0);
    }
    if (wo) store_col<FT, VEC>(io.organic, i, oo);
    if (wm) store_col<FT, VEC>(io.mixed, i, om);
}

template <typename FT> struct ApparentIO { const FT *od, *nr, *gr, *cs, *csi, *id; FT *J; };

template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void apparent_nucleation_kernel(const ApparentIO<FT> io, const FT id_default, const int64_t nvec) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    FT od[VEC], nr[VEC], gr[VEC], cs[VEC], csi[VEC], id[VEC];
    if (i < nvec) {
        load_col<FT, VEC>(io.od, i, od);
        load_col<FT, VEC>(io.nr, i, nr);
        load_col<FT, VEC>(io.gr, i, gr);
        load_col<FT, VEC>(io.cs, i, cs);
        load_col<FT, VEC>(io.csi, i, csi);
        if (io.id) load_col<FT, VEC>(io.id, i, id);
    }
    Math<FT>::prepare();
    if (i >= nvec) return;
    FT J[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) J[k] = apparent_rate<FT>(od[k], nr[k], gr[k], cs[k], csi[k], io.id ? id[k] : id_default);
    store_col<FT, VEC>(io.J, i, J);
}

template <typename FT> struct P3NucIO { const FT *T, *Nl, *Vl, *dt; FT *N_dep, *N_het; };

template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void p3_ice_nucleation_counts_kernel(const P3NucConsts<FT> c, const P3NucIO<FT> io, const int64_t nvec) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool wd = io.N_dep, wh = io.N_het;
    FT T[VEC], Nl[VEC], Vl[VEC], dt[VEC];
    if (i < nvec) {
        load_col<FT, VEC>(io.T, i, T);
        if (wh) {
            load_col<FT, VEC>(io.Nl, i, Nl);
            load_col<FT, VEC>(io.Vl, i, Vl);
            load_col<FT, VEC>(io.dt, i, dt);
        }
    }
    Math<FT>::prepare();
    if (i >= nvec) return;
    FT nd[VEC], nh[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        nd[k] = wd ? p3_deposition_N_i<FT>(c, T[k]) : FT(0);
        nh[k] = wh ? p3_het_N_i<FT>(c, T[k], Nl[k], Vl[k], dt[k]) : FT(0);
    }
    if (wd) store_col<FT, VEC>(io.N_dep, i, nd);
    if (wh) store_col<FT, VEC>(io.N_het, i, nh);
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <typename FT, typename HP, typename OP, typename MP>
static int32_t aerosol_nucleation_entry(const HP *hp, const OP *op, const MP *mp, int64_t n, const FT *h2so4, const FT *nh3, const FT *ion, const FT *mt,
                                        const FT *o3, const FT *oh, const FT *T, const FT *cs, FT *binary, FT *ternary, FT *organic, FT *mixed, void *stream) {
    CMX_TRY_COUNT_LIMIT(n);
    const bool wh = binary || ternary;
    if (!wh && !organic && !mixed) return CMX_ERR_BAD_ARG;
    if ((wh && !hp) || (organic && !op) || (mixed && !mp)) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if (!T) return CMX_ERR_BAD_ARG;
    if (wh && (!h2so4 || !nh3 || !ion)) return CMX_ERR_BAD_ARG;
    if (organic && (!ion || !mt || !o3 || !oh || !cs)) return CMX_ERR_BAD_ARG;
    if (mixed && (!h2so4 || !mt || !oh || !cs)) return CMX_ERR_BAD_ARG;
    const NucConsts<FT> c = make_nucleation_consts<FT>(wh ? hp : nullptr, organic ? op : nullptr, mixed ? mp : nullptr);
    // the columns no requested output reads are not passed on: they neither count in the split nor are loaded
    const FT *h_ = (wh || mixed) ? h2so4 : nullptr, *a_ = wh ? nh3 : nullptr, *ion_ = (wh || organic) ? ion : nullptr;
    const FT *mt_ = (organic || mixed) ? mt : nullptr, *o3_ = organic ? o3 : nullptr, *oh_ = (organic || mixed) ? oh : nullptr;
    const FT *cs_ = (organic || mixed) ? cs : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const void *ptrs[] = {h_, a_, ion_, mt_, o3_, oh_, T, cs_, binary, ternary, organic, mixed};
    for_each_range<FT, Math<FT>::VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {      // alignment split: cmx_split.hpp
        constexpr int V = decltype(vec_tag)::value;
        const NucIO<FT> io{shift(h_, lo), shift(a_, lo), shift(ion_, lo), shift(mt_, lo), shift(o3_, lo), shift(oh_, lo), T + lo, shift(cs_, lo),
                           shift(binary, lo), shift(ternary, lo), shift(organic, lo), shift(mixed, lo)};
        const int64_t nv = count / V;
        launch<kBlock>(aerosol_nucleation_kernel<FT, V>, nv, s, c, io, nv);
    });
    return launched();
}

template <typename FT, typename OP, typename MP>
static int32_t nucleation_prescribed_entry(const OP *op, const MP *mp, int64_t n, const FT *ion, const FT *hom, const FT *h2so4, const FT *bio, FT *organic,
                                           FT *mixed, void *stream) {
    CMX_TRY_COUNT_LIMIT(n);
    if (!organic && !mixed) return CMX_ERR_BAD_ARG;
    if ((organic && !op) || (mixed && !mp)) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if ((organic && (!ion || !hom)) || (mixed && (!h2so4 || !bio))) return CMX_ERR_BAD_ARG;
    const NucConsts<FT> c = make_nucleation_consts<FT>(static_cast<const cmx_h2so4_nucleation_f64 *>(nullptr), organic ? op : nullptr, mixed ? mp : nullptr);
    const FT *ion_ = organic ? ion : nullptr, *hom_ = organic ? hom : nullptr, *h_ = mixed ? h2so4 : nullptr, *bio_ = mixed ? bio : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const void *ptrs[] = {ion_, hom_, h_, bio_, organic, mixed};
    for_each_range<FT, Math<FT>::VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
        constexpr int V = decltype(vec_tag)::value;
        const NucPrescribedIO<FT> io{shift(ion_, lo), shift(hom_, lo), shift(h_, lo), shift(bio_, lo), shift(organic, lo), shift(mixed, lo)};
        const int64_t nv = count / V;
        launch<kBlock>(nucleation_prescribed_kernel<FT, V>, nv, s, c, io, nv);
    });
    return launched();
}

template <typename FT>
static int32_t apparent_nucleation_entry(int64_t n, const FT *od, const FT *nr, const FT *gr, const FT *cs, const FT *csi, const FT *id, FT *J, void *stream) {
    CMX_TRY_COUNT_LIMIT(n);
    if (!J) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if (!od || !nr || !gr || !cs || !csi) return CMX_ERR_BAD_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const void *ptrs[] = {od, nr, gr, cs, csi, id, J};
    for_each_range<FT, Math<FT>::VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
        constexpr int V = decltype(vec_tag)::value;
        const ApparentIO<FT> io{od + lo, nr + lo, gr + lo, cs + lo, csi + lo, shift(id, lo), J + lo};
        const int64_t nv = count / V;
        launch<kBlock>(apparent_nucleation_kernel<FT, V>, nv, s, io, FT(1.7), nv);
    });
    return launched();
}

template <typename FT, typename IP>
static int32_t p3_ice_nucleation_counts_entry(const IP *ip, int64_t n, const FT *T, const FT *Nl, const FT *Vl, const FT *dt, FT *N_dep, FT *N_het,
                                              void *stream) {
    if (!ip) return CMX_ERR_BAD_ARG;
    CMX_TRY_COUNT_LIMIT(n);
    if (!N_dep && !N_het) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    if (!T || (N_het && (!Nl || !Vl || !dt))) return CMX_ERR_BAD_ARG;
    const P3NucConsts<FT> c = make_p3_nucleation_consts<FT>(*ip);
    const FT *Nl_ = N_het ? Nl : nullptr, *Vl_ = N_het ? Vl : nullptr, *dt_ = N_het ? dt : nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const void *ptrs[] = {T, Nl_, Vl_, dt_, N_dep, N_het};
    for_each_range<FT, Math<FT>::VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
        constexpr int V = decltype(vec_tag)::value;
        const P3NucIO<FT> io{T + lo, shift(Nl_, lo), shift(Vl_, lo), shift(dt_, lo), shift(N_dep, lo), shift(N_het, lo)};
        const int64_t nv = count / V;
        launch<kBlock>(p3_ice_nucleation_counts_kernel<FT, V>, nv, s, c, io, nv);
    });
    return launched();
}

}  // namespace cmx

extern "C" {
int32_t cmx_aerosol_nucleation_rates_f32(const cmx_h2so4_nucleation_f32 *h2so4p, const cmx_organic_nucleation_f32 *orgp, const cmx_mixed_nucleation_f32 *mixp,
                                         int64_t n, const float *h2so4, const float *nh3, const float *negative_ion, const float *monoterpene, const float *O3,
                                         const float *OH, const float *T, const float *condensation_sink, float *binary, float *ternary, float *organic,
                                         float *mixed, void *stream) {
    return cmx::aerosol_nucleation_entry<float>(h2so4p, orgp, mixp, n, h2so4, nh3, negative_ion, monoterpene, O3, OH, T, condensation_sink, binary, ternary,
                                                organic, mixed, stream);
}
int32_t cmx_aerosol_nucleation_rates_f64(const cmx_h2so4_nucleation_f64 *h2so4p, const cmx_organic_nucleation_f64 *orgp, const cmx_mixed_nucleation_f64 *mixp,
                                         int64_t n, const double *h2so4, const double *nh3, const double *negative_ion, const double *monoterpene,
                                         const double *O3, const double *OH, const double *T, const double *condensation_sink, double *binary, double *ternary,
                                         double *organic, double *mixed, void *stream) {
    return cmx::aerosol_nucleation_entry<double>(h2so4p, orgp, mixp, n, h2so4, nh3, negative_ion, monoterpene, O3, OH, T, condensation_sink, binary, ternary,
                                                 organic, mixed, stream);
}
int32_t cmx_nucleation_rates_prescribed_f32(const cmx_organic_nucleation_f32 *orgp, const cmx_mixed_nucleation_f32 *mixp, int64_t n, const float *negative_ion,
                                            const float *HOM, const float *h2so4, const float *bioOxOrg, float *organic, float *mixed, void *stream) {
    return cmx::nucleation_prescribed_entry<float>(orgp, mixp, n, negative_ion, HOM, h2so4, bioOxOrg, organic, mixed, stream);
}
int32_t cmx_nucleation_rates_prescribed_f64(const cmx_organic_nucleation_f64 *orgp, const cmx_mixed_nucleation_f64 *mixp, int64_t n, const double *negative_ion,
                                            const double *HOM, const double *h2so4, const double *bioOxOrg, double *organic, double *mixed, void *stream) {
    return cmx::nucleation_prescribed_entry<double>(orgp, mixp, n, negative_ion, HOM, h2so4, bioOxOrg, organic, mixed, stream);
}
int32_t cmx_apparent_nucleation_rate_f32(int64_t n, const float *output_diam, const float *nucleation_rate, const float *condensation_growth_rate,
                                         const float *coag_sink, const float *coag_sink_input_diam, const float *input_diam, float *J_x, void *stream) {
    return cmx::apparent_nucleation_entry<float>(n, output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam, J_x,
                                                 stream);
}
int32_t cmx_apparent_nucleation_rate_f64(int64_t n, const double *output_diam, const double *nucleation_rate, const double *condensation_growth_rate,
                                         const double *coag_sink, const double *coag_sink_input_diam, const double *input_diam, double *J_x, void *stream) {
    return cmx::apparent_nucleation_entry<double>(n, output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam, J_x,
                                                  stream);
}
int32_t cmx_p3_ice_nucleation_counts_f32(const cmx_morrison_milbrandt2014_f32 *ip, int64_t n, const float *T, const float *N_l, const float *V_l,
                                         const float *dt, float *N_dep, float *N_het, void *stream) {
    return cmx::p3_ice_nucleation_counts_entry<float>(ip, n, T, N_l, V_l, dt, N_dep, N_het, stream);
}
int32_t cmx_p3_ice_nucleation_counts_f64(const cmx_morrison_milbrandt2014_f64 *ip, int64_t n, const double *T, const double *N_l, const double *V_l,
                                         const double *dt, double *N_dep, double *N_het, void *stream) {
    return cmx::p3_ice_nucleation_counts_entry<double>(ip, n, T, N_l, V_l, dt, N_dep, N_het, stream);
}
}
