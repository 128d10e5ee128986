// cmx_mp2m_p3_column_implicit.hip — the 2M + P3 column step with backward-Euler upwind sedimentation, stable at any Courant number Δt·w/Δz: C-ABI entry
// points cmx_mp2m_p3_column_implicit_sedimentation_* (include/cmx.h §(24)).  Steps (1) and (2) of (9b) — products → shape and fall speeds → the eight
// tendencies — are the same launches through the same entry layer (cmx_mp2m_p3_column.hpp), hence the same bits; ONE kernel, here, replaces step (3).  Per
// column and falling species, with a the tendency step (2) left in the column, F and w the flux and the fall speed of p3col_fluxes_of_point and
// g = inv_dz[k]·rcp(ρ⁺) as the (9b) kernel forms it,
//     τ = Δt·w   c = τ·inv_dz[k]   β = τ·ρ⁺   r = 1/(1 + c)   A = c·r   B = fma(β, a, F)·r
//     G_k = top ? B_k : fma(A_k, G_{k+1}, B_k)                     from the column top downward
//     out_k = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k))·r_k     surface outputs: G_0 of q_rai and q_ice
// r is a TRUE division (exactly 1 at c = 0); the fall speeds are those of the initial state.  Compiled like every pointwise file (-ffp-contract=off, no
// contraction bracket): every product and sum not written as fma above is an operation of its own.
//
// Kernel shape: that of implicit_sedimentation_step_kernel (cmx_column_implicit_step.hip).  A workgroup OWNS a contiguous range of whole columns
// (cols_per_wg of them, a host-side tuning number that no result depends on) and walks it in chunks of BS flat points from the highest index to the lowest.
// Per chunk
//   1. parallel — one point per lane: the eleven columns the fluxes read, (F, w), then per falling species the tendency a from its column; the lane stores
//      A and B to LDS at once and keeps fma(−F, g, a), r and g.  Barrier.
//   2. serial — one lane per (column segment inside the chunk, species) runs G = fma(A, G_up, B) down its segment and writes G OVER B: with eight species
//      (six without cloud_vel) where the sibling has four, A and B/G take 32 KiB (24 KiB) in Float64 instead of 48 KiB for three arrays, next to the 4 KiB of
//      exp2 / log2 tables of Math<double>::prepare(): four (five) workgroups share a CU's 160 KiB where three arrays allow three — as many waves per SIMD as
//      the SB2006-velocity instantiations' registers allow (105–117 VGPRs with cloud_vel: 4; 78 without: 6; Chen-2022: 141–253 VGPRs, 3 or 2 waves either
//      way).  A segment that starts below a column top takes G_up from the carry of the chunk before (two slots used in turn: the lane that writes the next
//      carry never races the lane that reads this one).  Barrier.
//   3. parallel — every lane reads G_{k+1} and stores `out` over the tendency; the lane at level 0 stores G_0.  Barrier: the next chunk's phase 1 writes B where
//      this phase read G.
// Limited PSD, velocity kind and cloud sedimentation are template arguments, as in (9b): 2 × 3 × 2 instantiations per float type.
#include <limits>

#include "cmx_mp2m_p3_column.hpp"

namespace cmx {

constexpr int kP3ImplBS = 256;         // lanes per workgroup = points per chunk, as in the sibling
constexpr int kP3ImplChunks = 4;       // a workgroup owns about this many chunks of points (whole columns; one column if it is longer), as in the sibling

template <typename FT> struct P3ImplicitIO {
    const FT *rho, *q_lcl, *n_lcl, *q_rai, *n_rai, *q_ice, *n_ice, *q_rim, *b_rim, *v_n, *v_m;
    FT *tend[SP_N];        // a on entry, out on return
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip_rai, *precip_ice;      // n_col values each, or nullptr: G_0 of q_rai and q_ice
    int64_t n_col;
    int32_t n_lev;
    int32_t cols_per_wg;   // cols_per_wg · n_lev < 2³¹
    FT dt;                 // FT(Δt)
    FastDivU32 lev_div;    // division by n_lev (cmx_launch.hpp fastdiv)
};

template <typename FT, bool LIMITED, int VEL, bool CLOUD, int BS>
__global__ __launch_bounds__(BS) void mp2m_p3_implicit_sedimentation_kernel(const SbConsts<FT> c, const CloudVelConsts<FT> cv, const P3ImplicitIO<FT> io) {
    using M = Math<FT>;
    constexpr int S0 = CLOUD ? SP_QLCL : SP_QRAI;      // first sedimenting species: without cloud_vel the two cloud columns are not touched
    constexpr int NS = SP_N - S0;
    __shared__ __align__(16) FT As[BS][NS], Gs[BS][NS];      // A, and B → G, of every point of the chunk
    __shared__ FT carry[2][NS];                              // G of the point above the chunk, per species; the slots alternate from chunk to chunk
    // the workgroup's range of whole columns: P points from flat index `base`
    const int64_t col0 = (int64_t)blockIdx.x * io.cols_per_wg;
    const int64_t left = io.n_col - col0;
    const uint32_t P = (uint32_t)(left < io.cols_per_wg ? left : (int64_t)io.cols_per_wg) * (uint32_t)io.n_lev;
    const int64_t base = col0 * io.n_lev;
    const uint32_t n_lev = (uint32_t)io.n_lev;
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    uint32_t par = 0;
#pragma unroll 1
    for (uint32_t cs = (P - 1) / BS * BS;; cs -= BS) {      // chunks [cs, cs + BS) ∩ [0, P) of the range, the highest first
        const uint32_t rel = cs + threadIdx.x;
        const bool active = rel < P;
        const int64_t i = base + rel;
        FT hq[NS], rr[NS], g = FT(0);
        uint32_t lev = 0, relcol = 0;
        bool top = false;
        if (active) {
            const FT rho = __builtin_nontemporal_load(io.rho + i);
            const FT q_rai = __builtin_nontemporal_load(io.q_rai + i), n_rai = __builtin_nontemporal_load(io.n_rai + i);
            const FT q_ice = __builtin_nontemporal_load(io.q_ice + i), n_ice = __builtin_nontemporal_load(io.n_ice + i);
            const FT q_rim = __builtin_nontemporal_load(io.q_rim + i), b_rim = __builtin_nontemporal_load(io.b_rim + i);
            const FT v_n = __builtin_nontemporal_load(io.v_n + i), v_m = __builtin_nontemporal_load(io.v_m + i);
            FT q_lcl = FT(0), n_lcl = FT(0);
            if constexpr (CLOUD) {
                q_lcl = __builtin_nontemporal_load(io.q_lcl + i);
                n_lcl = __builtin_nontemporal_load(io.n_lcl + i);
            }
            FT F[SP_N], w[SP_N];
            p3col_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(front_consts<FT>(c), cv, rho, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, v_n, v_m, F, w);
            relcol = fastdiv(rel, io.lev_div);
            lev = rel - relcol * n_lev;
            top = lev == n_lev - 1;                       // nothing enters through the model top
            const FT idz = io.inv_dz[lev];
            const FT rp = max0(rho);
            g = idz * M::rcp(rp);                         // 1/(ρ_k Δz_k), as mp2m_p3_sedimentation_kernel forms it
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const FT a = __builtin_nontemporal_load(io.tend[S0 + q] + i);
                const FT tau = io.dt * w[S0 + q];
                const FT cn = tau * idz, beta = tau * rp;
                const FT r = FT(1) / (FT(1) + cn);        // a true division: exactly 1 at c = 0
                As[threadIdx.x][q] = cn * r;
                Gs[threadIdx.x][q] = M::fma(beta, a, F[S0 + q]) * r;
                rr[q] = r;
                hq[q] = M::fma(-F[S0 + q], g, a);
            }
        }
        __syncthreads();
        {   // ---- the chains of the chunk: lane → (segment = the part of one column inside the chunk, species)
            const uint32_t ce = cs + BS < P ? cs + BS : P;
            const uint32_t colA = fastdiv(cs, io.lev_div), nseg = fastdiv(ce - 1, io.lev_div) - colA + 1;
            for (uint32_t sl = threadIdx.x; sl < nseg * NS; sl += BS) {
                const uint32_t q = sl % NS, col = colA + sl / NS;
                const uint32_t cb = col * n_lev, ct = cb + n_lev;       // the column: [cb, ct) of the range
                const uint32_t lo = cb > cs ? cb : cs, hi = ct < ce ? ct : ce;
                const bool from_top = hi == ct;
                uint32_t p = hi - 1 - cs;
                const FT Gup = carry[par][q];
                FT G = from_top ? Gs[p][q] : M::fma(As[p][q], Gup, Gs[p][q]);      // a select: nothing crosses a column top
                Gs[p][q] = G;
#pragma unroll 4
                for (uint32_t m = hi - lo - 1; m > 0; --m) {
                    --p;
                    G = M::fma(As[p][q], G, Gs[p][q]);
                    Gs[p][q] = G;
                }
                if (lo > cb) carry[par ^ 1][q] = G;       // the column goes on in the next chunk
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                FT up = FT(0);
                if (!top) up = threadIdx.x == BS - 1 ? carry[par][q] : Gs[threadIdx.x + 1 < BS ? threadIdx.x + 1 : 0][q];
                __builtin_nontemporal_store(M::fma(up, g, hq[q]) * rr[q], io.tend[S0 + q] + i);
            }
            if (lev == 0) {                               // the flux that leaves the column during the step
                const int64_t col = col0 + relcol;
                if (io.precip_rai) io.precip_rai[col] = Gs[threadIdx.x][SP_QRAI - S0];
                if (io.precip_ice) io.precip_ice[col] = Gs[threadIdx.x][SP_QICE - S0];
            }
        }
        if (cs == 0) break;
        par ^= 1;
        __syncthreads();      // G of this chunk has been read: the next chunk's B may take its place
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// the callable of the entry layer (cmx_mp2m_p3_column.hpp): the IO struct and the launch
template <typename FT, typename ST>
static auto implicit_sedimentation(const ST *cloud_vel, double dt, int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *tend, FT *v_n,
                                   FT *v_m, FT *precip_rai, FT *precip_ice, void *stream) {
    return [=](bool limited, int velk, const SbConsts<FT> &c, const CloudVelConsts<FT> &cv) -> int32_t {
        P3ImplicitIO<FT> io{};
        io.rho = in[IN_RHO]; io.q_lcl = in[IN_QLCL]; io.n_lcl = in[IN_NLCL]; io.q_rai = in[IN_QRAI]; io.n_rai = in[IN_NRAI];
        io.q_ice = in[IN_QICE]; io.n_ice = in[IN_NICE]; io.q_rim = in[IN_QRIM]; io.b_rim = in[IN_BRIM]; io.v_n = v_n; io.v_m = v_m;
        for (int q = 0; q < SP_N; ++q) io.tend[q] = tend[q];
        io.inv_dz = inv_dz; io.precip_rai = precip_rai; io.precip_ice = precip_ice;
        io.n_col = n_col; io.n_lev = n_lev;
        // whole columns per workgroup: about kP3ImplChunks chunks of points, at least one column
        const int32_t m = kP3ImplChunks * kP3ImplBS / n_lev;
        io.cols_per_wg = m < 1 ? 1 : m;
        io.dt = (FT)dt;
        io.lev_div = make_fastdiv((uint32_t)n_lev);
        // (n_col·n_lev ≤ 4·(2^31 − 8) and more than 512 points per full workgroup keep the grid inside HIP's 2^31 − 1)
        const dim3 grid((unsigned)tile_grid(n_col, io.cols_per_wg)), block(kP3ImplBS);
        const bool known = dispatch([&](auto L, auto K, auto C) {
            launch_grid(mp2m_p3_implicit_sedimentation_kernel<FT, decltype(L)::value, decltype(K)::value, decltype(C)::value, kP3ImplBS>, grid, block, 0,
                        reinterpret_cast<hipStream_t>(stream), c, cv, io);
        }, flag(limited), one_of<VEL_SB, VEL_CHEN, VEL_CHEN_GEN>(velk), flag(cloud_vel != nullptr));
        if (!known) return CMX_ERR_BAD_ARG;      // unreachable: velk is VEL_SB or what chen_vel_kind gives
        return launched();
    };
}

// dt: finite and ≥ 0, and finite as FT — judged in double, before any conversion: a double above the largest FT has no defined conversion to FT.  (The doubles
// within half an ulp above the largest Float32, which would round down to it, are refused with the rest.)
template <typename FT> static bool implicit_dt_ok(double dt) { return dt >= 0.0 && dt <= (double)std::numeric_limits<FT>::max(); }

}  // namespace cmx

extern "C" {

int32_t cmx_mp2m_p3_column_implicit_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                                      const cmx_rain_vel_f32 *rain_vel, const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags,
                                                      int32_t brent_iters, float p, double dt, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                      const float *const *in, float *const *tendencies, float *log_lambda, float *v_ice_n, float *v_ice_m,
                                                      float *precip_rai, float *precip_ice, void *stream) {
    return cmx::p3_column_entry<float>(warm_rain, ice, tps, rain_vel, cloud_vel, flags, brent_iters, p, n_col, n_lev, inv_dz, in, tendencies, log_lambda,
                                       v_ice_n, v_ice_m, cmx::implicit_dt_ok<float>(dt), stream,
                                       cmx::implicit_sedimentation<float>(cloud_vel, dt, n_col, n_lev, inv_dz, in, tendencies, v_ice_n, v_ice_m, precip_rai,
                                                                          precip_ice, stream));
}
int32_t cmx_mp2m_p3_column_implicit_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                                      const cmx_rain_vel_f64 *rain_vel, const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags,
                                                      int32_t brent_iters, double p, double dt, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                      const double *const *in, double *const *tendencies, double *log_lambda, double *v_ice_n,
                                                      double *v_ice_m, double *precip_rai, double *precip_ice, void *stream) {
    return cmx::p3_column_entry<double>(warm_rain, ice, tps, rain_vel, cloud_vel, flags, brent_iters, p, n_col, n_lev, inv_dz, in, tendencies, log_lambda,
                                        v_ice_n, v_ice_m, cmx::implicit_dt_ok<double>(dt), stream,
                                        cmx::implicit_sedimentation<double>(cloud_vel, dt, n_col, n_lev, inv_dz, in, tendencies, v_ice_n, v_ice_m, precip_rai,
                                                                            precip_ice, stream));
}

}  // extern "C"
