// cmx_mp2m_p3_column.hip — the 2M + P3 COLUMN step: what a mixed-phase host model evaluates once per time step, as one call.
//
//   (1) log λ, v_n, v_m = cmx_p3_shape_terminal_velocities_* on (ρ q_ice, ρ n_ice, ρ q_rim, ρ b_rim)        include/cmx.h §(7)
//   (2) tend            = cmx_microphysics_2m_p3_tendencies_* with that log λ                                 include/cmx.h §(9)
//   (3) w_r = CM2.rain_terminal_velocity, w_c = CM2.cloud_terminal_velocity (optional), and the host model's first-order upwind
//       ("right-biased") flux divergence of the eight falling species — the formula of cmx_sb2006_column.hip:
//           F_k = ρ_k χ_k w_k,   ∂χ_k/∂t += (F_{k+1} − F_k) · inv_dz[k] / ρ_k,   F_{n_lev} = 0
//       χ = q_rai (w_m), n_rai (w_n), q_ice, q_rim, b_rim (v_ice_m), n_ice (v_ice_n) and — with cloud_vel — q_lcl, n_lcl.
//
// (1) and (2) are the library's own entries, called as they are (the same launches, hence the same bits): this translation unit holds no P3
// code and is compiled like every pointwise file (-ffp-contract=off, no contraction bracket).  The library allocates nothing, so the hand-off
// between the launches goes through the caller's columns: log λ, v_n, v_m are outputs of the entry, and the four volumetric products (1) reads
// are parked in the last four TENDENCY columns, which (2) overwrites afterwards (every tendency column is written by (2) before (3) reads it).
// (3) is new: one kernel, lanes along the flat index i = col·n_lev + k with 16-byte accesses, the flux of the cell above handed across lanes
// through an LDS halo exactly as in sb2006_column_kernel, the point after a launch's last tile evaluated by the same flux function from the
// raw columns — results, NaN propagation included, do not depend on where tile or launch boundaries fall.
// The entry layer — the checks in their order, steps (1) and (2), the constants of (3) — the species enum and the flux function of a raw point are
// cmx_mp2m_p3_column.hpp's, shared with the implicit step of include/cmx.h §(24) (cmx_mp2m_p3_column_implicit.hip); here are the products kernel and its
// launch, the kernel of step (3), its IO struct and launches, and the extern "C" functions.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cmx_mp2m_p3_column.hpp"

namespace cmx {

// ---- the four volumetric products of step (1) ---------------------------------------------------------------------------------
template <typename FT, int VEC>
__global__ __launch_bounds__(kBlock) void p3col_products_kernel(const FT *__restrict__ rho, const FT *__restrict__ q_ice, const FT *__restrict__ n_ice,
                                                                const FT *__restrict__ q_rim, const FT *__restrict__ b_rim, FT *__restrict__ rho_q,
                                                                FT *__restrict__ rho_n, FT *__restrict__ rho_x3, FT *__restrict__ rho_x4, const int64_t nvec) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nvec) return;
    FT r[VEC], a[VEC], b[VEC], c[VEC], d[VEC];
    load_col<FT, VEC, false>(rho, v, r);        // (ρ and the ice columns are read again by the launches that follow: no non-temporal hint)
    load_col<FT, VEC, false>(q_ice, v, a);
    load_col<FT, VEC, false>(n_ice, v, b);
    load_col<FT, VEC, false>(q_rim, v, c);
    load_col<FT, VEC, false>(b_rim, v, d);
#pragma unroll
    for (int k = 0; k < VEC; ++k) { a[k] = r[k] * a[k]; b[k] = r[k] * b[k]; c[k] = r[k] * c[k]; d[k] = r[k] * d[k]; }
    store_col<FT, VEC, false>(rho_q, v, a);
    store_col<FT, VEC, false>(rho_n, v, b);
    store_col<FT, VEC, false>(rho_x3, v, c);
    store_col<FT, VEC, false>(rho_x4, v, d);
}

// ---- step (3) -------------------------------------------------------------------------------------------------------------------
// species: the enum of cmx_mp2m_p3_column.hpp, in the order of the tendency columns
template <typename FT> struct P3SedIO {
    const FT *rho, *q_lcl, *n_lcl, *q_rai, *n_rai, *q_ice, *n_ice, *q_rim, *b_rim, *v_n, *v_m;
    FT *tend[SP_N];        // read-modify-written
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip_rai, *precip_ice;      // n_col values each, or nullptr
    int64_t n;             // n_col · n_lev
    int32_t n_lev;
    double inv_n_lev;
    FastDivU32 lev_div;    // division by n_lev for flat indices below 2³² (cmx_launch.hpp fastdiv)
};

// The fluxes of a raw point: p3col_fluxes_of_point (cmx_mp2m_p3_column.hpp, shared with the implicit step of §(24)).  The fall speeds it hands out as well
// are not used here.
// lanes per workgroup and the tile geometry are those of sb2006_column_kernel (256 lanes, tiles that overlap by one lane: CMX_COLUMN_BS there)
#ifndef CMX_P3COL_BS
#define CMX_P3COL_BS 256
#endif
constexpr int kP3ColBS = CMX_P3COL_BS;

template <typename FT, bool LIMITED, int VEL, bool CLOUD, int VEC, int BS>
__global__ __launch_bounds__(BS) void mp2m_p3_sedimentation_kernel(const SbConsts<FT> c, const CloudVelConsts<FT> cv, const P3SedIO<FT> io,
                                                                   const int64_t first, const int64_t nvec) {
    using M = Math<FT>;
    constexpr int S0 = CLOUD ? SP_QLCL : SP_QRAI;      // first sedimenting species: without cloud_vel the two cloud columns are not touched
    // fluxes of every lane's FIRST point, + slot BS for the point that follows the launch's last tile
    __shared__ __align__(16) FT halo[BS + 1][SP_N];
    // workgroup b owns the vectors [b(BS−1), (b+1)(BS−1)); its lane BS−1 evaluates the first vector of the next tile like any other lane and
    // only supplies the flux that vector's first point sends down to lane BS−2 (sb2006_column_kernel)
    const int64_t tile0 = (int64_t)blockIdx.x * (BS - 1);
    const int64_t v = tile0 + threadIdx.x;
    const bool active = v < nvec;
    const int64_t nvalid = nvec - tile0 < BS ? nvec - tile0 : BS;       // active lanes of this tile (≥ 1)
    const bool owner = threadIdx.x < BS - 1;
    const int64_t i0 = first + v * VEC;                                 // flat index of the lane's first point

    FT rho[VEC], q_lcl[VEC], n_lcl[VEC], q_rai[VEC], n_rai[VEC], q_ice[VEC], n_ice[VEC], q_rim[VEC], b_rim[VEC], v_n[VEC], v_m[VEC];
    if (active) {
        load_col<FT, VEC, true>(io.rho + first, v, rho);
        load_col<FT, VEC, true>(io.q_rai + first, v, q_rai);
        load_col<FT, VEC, true>(io.n_rai + first, v, n_rai);
        load_col<FT, VEC, true>(io.q_ice + first, v, q_ice);
        load_col<FT, VEC, true>(io.n_ice + first, v, n_ice);
        load_col<FT, VEC, true>(io.q_rim + first, v, q_rim);
        load_col<FT, VEC, true>(io.b_rim + first, v, b_rim);
        load_col<FT, VEC, true>(io.v_n + first, v, v_n);
        load_col<FT, VEC, true>(io.v_m + first, v, v_m);
        if constexpr (CLOUD) {
            load_col<FT, VEC, true>(io.q_lcl + first, v, q_lcl);
            load_col<FT, VEC, true>(io.n_lcl + first, v, n_lcl);
        }
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (nvalid < BS && threadIdx.x == BS - 1) {        // last workgroup of the launch only (lane BS−1 has no vector there)
        const int64_t e = first + (tile0 + nvalid) * VEC;
        FT f[SP_N], w[SP_N];
#pragma unroll
        for (int q = 0; q < SP_N; ++q) f[q] = FT(0);
        if (e < io.n) {
            FT ql = FT(0), nl = FT(0);
            if constexpr (CLOUD) { ql = io.q_lcl[e]; nl = io.n_lcl[e]; }
            p3col_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(front_consts<FT>(c), cv, io.rho[e], ql, nl, io.q_rai[e], io.n_rai[e], io.q_ice[e], io.n_ice[e],
                                                           io.q_rim[e], io.b_rim[e], io.v_n[e], io.v_m[e], f, w);
        }
#pragma unroll
        for (int q = 0; q < SP_N; ++q) halo[BS][q] = f[q];
    }
    FT F[VEC][SP_N], g[VEC];      // the flux each point sends down, and 1/(ρ_k Δz_k)
    int64_t col = 0;
    int32_t lev = 0;
    if (active) {
        // level of the lane's first point: i0 = col·n_lev + k
        if (io.n < ((int64_t)1 << 32)) {             // wave-uniform: one v_mul_hi_u32
            const uint32_t c32 = fastdiv((uint32_t)i0, io.lev_div);
            col = c32;
            lev = (int32_t)((uint32_t)i0 - c32 * (uint32_t)io.n_lev);
        } else {                                     // one double multiply + fix-up per lane; exact below 2^53
            col = (int64_t)((double)i0 * io.inv_n_lev);
            int64_t k64 = i0 - col * io.n_lev;
            if (k64 < 0) { --col; k64 += io.n_lev; }
            if (k64 >= io.n_lev) { ++col; k64 -= io.n_lev; }
            lev = (int32_t)k64;
        }
        int32_t lv = lev;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            FT ql = FT(0), nl = FT(0), w[SP_N];
            if constexpr (CLOUD) { ql = q_lcl[k]; nl = n_lcl[k]; }
            p3col_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(front_consts<FT>(c), cv, rho[k], ql, nl, q_rai[k], n_rai[k], q_ice[k], n_ice[k], q_rim[k],
                                                           b_rim[k], v_n[k], v_m[k], F[k], w);
            g[k] = io.inv_dz[lv] * M::rcp(max0(rho[k]));
            if (++lv == io.n_lev) lv = 0;
        }
#pragma unroll
        for (int q = 0; q < SP_N; ++q) halo[threadIdx.x][q] = F[0][q];
    }
    __syncthreads();
    if (!active || !owner) return;
    const int up = (threadIdx.x + 1 < nvalid) ? threadIdx.x + 1 : BS;
    FT above[SP_N];
#pragma unroll
    for (int q = 0; q < SP_N; ++q) above[q] = halo[up][q];
    // one tendency column at a time: load, subtract the outflow through the lower face, add the inflow through the upper face (nothing
    // enters through the model top), store
    bool top[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        top[k] = lev == io.n_lev - 1;
        if (lev == 0) {      // the surface fluxes of the column
            if (io.precip_rai) io.precip_rai[col] = F[k][SP_QRAI];
            if (io.precip_ice) io.precip_ice[col] = F[k][SP_QICE];
        }
        if (++lev == io.n_lev) { lev = 0; ++col; }
    }
#pragma unroll
    for (int q = S0; q < SP_N; ++q) {
        FT t[VEC];
        load_col<FT, VEC, true>(io.tend[q] + first, v, t);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const FT upf = (k + 1 < VEC) ? F[k + 1 < VEC ? k + 1 : 0][q] : above[q];
            const FT A = M::fma(-F[k][q], g[k], t[k]);
            t[k] = top[k] ? A : M::fma(upf, g[k], A);
        }
        store_col<FT, VEC, true>(io.tend[q] + first, v, t);
    }
}

template <typename FT, int VEC>
static bool launch_p3_sedimentation(bool limited, int vel, bool cloud, const SbConsts<FT> &c, const CloudVelConsts<FT> &cv, const P3SedIO<FT> &io, int64_t first,
                                    int64_t nvec, hipStream_t s) {
    if (nvec <= 0) return true;
    const dim3 grid((unsigned)((nvec + (kP3ColBS - 1) - 1) / (kP3ColBS - 1))), block(kP3ColBS);      // tiles overlap by one lane
    return dispatch([&](auto L, auto K, auto C) {
        launch_grid(mp2m_p3_sedimentation_kernel<FT, decltype(L)::value, decltype(K)::value, decltype(C)::value, VEC, kP3ColBS>, grid, block, 0, s, c, cv, io, first, nvec);
    }, flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(vel), flag(cloud));
}

// step (1)'s products, for both column entries (declared in cmx_mp2m_p3_column.hpp)
template <typename FT> int32_t p3col_launch_products(const FT *const *in, FT *const *tend, int64_t n, hipStream_t s) {
    constexpr int VEC = Math<FT>::VEC;
    const void *ptrs[] = {in[IN_RHO], in[IN_QICE], in[IN_NICE], in[IN_QRIM], in[IN_BRIM], tend[SP_QICE], tend[SP_NICE], tend[SP_QRIM], tend[SP_BRIM]};
    for_each_range<FT, VEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
        constexpr int V = decltype(vec_tag)::value;
        launch<kBlock>(p3col_products_kernel<FT, V>, count / V, s, in[IN_RHO] + lo, in[IN_QICE] + lo, in[IN_NICE] + lo, in[IN_QRIM] + lo, in[IN_BRIM] + lo,
                       tend[SP_QICE] + lo, tend[SP_NICE] + lo, tend[SP_QRIM] + lo, tend[SP_BRIM] + lo, count / V);
    });
    return launched();
}
template int32_t p3col_launch_products<float>(const float *const *, float *const *, int64_t, hipStream_t);
template int32_t p3col_launch_products<double>(const double *const *, double *const *, int64_t, hipStream_t);

// the callable of the entry layer (cmx_mp2m_p3_column.hpp): the IO struct and the launches of step (3)
template <typename FT, typename ST>
static auto explicit_sedimentation(const ST *cloud_vel, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *tend, FT *v_n, FT *v_m,
                                   FT *precip_rai, FT *precip_ice, void *stream) {
    return [=](bool limited, int velk, const SbConsts<FT> &c, const CloudVelConsts<FT> &cv) -> int32_t {
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int64_t n = n_col * (int64_t)n_lev;
        P3SedIO<FT> io{};
        io.rho = in[IN_RHO]; io.q_lcl = in[IN_QLCL]; io.n_lcl = in[IN_NLCL]; io.q_rai = in[IN_QRAI]; io.n_rai = in[IN_NRAI];
        io.q_ice = in[IN_QICE]; io.n_ice = in[IN_NICE]; io.q_rim = in[IN_QRIM]; io.b_rim = in[IN_BRIM]; io.v_n = v_n; io.v_m = v_m;
        for (int q = 0; q < SP_N; ++q) io.tend[q] = tend[q];
        io.inv_dz = inv_dz; io.precip_rai = precip_rai; io.precip_ice = precip_ice;
        io.n = n; io.n_lev = n_lev; io.inv_n_lev = 1.0 / (double)n_lev; io.lev_div = make_fastdiv((uint32_t)n_lev);
        const bool cloud = cloud_vel != nullptr;
        // scalar head, vector body, scalar tail (cmx_split.hpp); the halo point of each range is read from the full columns, so the launches compose exactly
        const void *ptrs[] = {io.rho, io.q_lcl, io.n_lcl, io.q_rai, io.n_rai, io.q_ice, io.n_ice, io.q_rim, io.b_rim, io.v_n, io.v_m,
                              tend[0], tend[1], tend[2], tend[3], tend[4], tend[5], tend[6], tend[7]};
        // Float64: one point per lane, as in sb2006_column_kernel — two points hold two fall-speed evaluations' table reads and take 198–272 VGPRs
        // (one wave per SIMD) where one point takes 67–153
        constexpr int VEC = Math<FT>::VEC, SVEC = sizeof(FT) == 8 ? 1 : VEC;
        bool known = true;
        for_each_range<FT, SVEC>(ptrs, n, [&](auto vec_tag, int64_t lo, int64_t count) {
            constexpr int V = decltype(vec_tag)::value;
            known &= launch_p3_sedimentation<FT, V>(limited, velk, cloud, c, cv, io, lo, count / V, s);
        });
        if (!known) return CMX_ERR_BAD_ARG;      // unreachable: velk is VEL_SB or what chen_vel_kind gives
        return launched();
    };
}

}  // namespace cmx

extern "C" {

int32_t cmx_mp2m_p3_column_tendencies_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                                        const cmx_rain_vel_f32 *rain_vel, const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags,
                                                        int32_t brent_iters, float p, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                        const float *const *in, float *const *tendencies, float *log_lambda, float *v_ice_n,
                                                        float *v_ice_m, float *precip_rai, float *precip_ice, void *stream) {
    return cmx::p3_column_entry<float>(warm_rain, ice, tps, rain_vel, cloud_vel, flags, brent_iters, p, n_col, n_lev, inv_dz, in, tendencies, log_lambda,
                                       v_ice_n, v_ice_m, true, stream,
                                       cmx::explicit_sedimentation<float>(cloud_vel, n_col, n_lev, inv_dz, in, tendencies, v_ice_n, v_ice_m, precip_rai,
                                                                          precip_ice, stream));
}
int32_t cmx_mp2m_p3_column_tendencies_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                                        const cmx_rain_vel_f64 *rain_vel, const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags,
                                                        int32_t brent_iters, double p, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                        const double *const *in, double *const *tendencies, double *log_lambda, double *v_ice_n,
                                                        double *v_ice_m, double *precip_rai, double *precip_ice, void *stream) {
    return cmx::p3_column_entry<double>(warm_rain, ice, tps, rain_vel, cloud_vel, flags, brent_iters, p, n_col, n_lev, inv_dz, in, tendencies, log_lambda,
                                        v_ice_n, v_ice_m, true, stream,
                                        cmx::explicit_sedimentation<double>(cloud_vel, n_col, n_lev, inv_dz, in, tendencies, v_ice_n, v_ice_m, precip_rai,
                                                                            precip_ice, stream));
}

}  // extern "C"
