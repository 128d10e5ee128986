// cmx_column_implicit_step.hip — the column steps with the sub-stepped implicit average as tendency operator AND backward-Euler upwind sedimentation, stable
// and positive at any Courant number: C-ABI entry points cmx_sb2006_column_implicit_step_* and cmx_mp1m_column_implicit_step_* (include/cmx.h §(21)).  Per
// point the average a_j of §(19) and the fluxes F_j, g of §(20), bit for bit as in cmx_column_implicit_average.hip; then per species, with the fall speed w the
// flux function multiplied into F,
//     τ = Δt·w   c = τ·inv_dz[k]   β = τ·ρ⁺   r = 1/(1 + c)   A = c·r   B = fma(β, a, F)·r
//     G_k = top ? B_k : fma(A_k, G_{k+1}, B_k)                     from the column top downward
//     out_k = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k))·r_k     surface output: G_0
// r is a TRUE division (exactly 1 at c = 0); the fall speeds are those of the initial state.
//
// Kernel shape: the recurrence runs down a column, so a workgroup OWNS a contiguous range of whole columns (cols_per_wg of them, a host-side tuning number
// that no result depends on) and no workgroup ever waits for another.  It walks its range in chunks of BS flat points from the highest index to the lowest.
// Per chunk
//   1. parallel — one point per lane, as in cmx_column_implicit_average.hip: the substeps (implicit_average_substeps, cmx_jacobian.hpp: the loop
//      of the average entry itself), then the (F, w) flux function of the scheme (sed_fluxes_w_of_point, mp1m_sed_fluxes_w: the operations of the
//      flux-only functions on the same operands).  The lane forms A and B, stores them to LDS at once and keeps fma(−F, g, a), g and r: the Float64 instantiations have no register to
//      spare.  Barrier.
//   2. serial — one lane per (column segment inside the chunk, species) runs G = fma(A, G_up, B) down its segment: one dependent fma per level, the A and B
//      reads do not depend on the chain.  A segment that starts below a column top takes G_up from the carry of the chunk before (LDS, two slots used in
//      turn so that the lane that writes the next carry never races the lane that reads this one); a column longer than a chunk is simply several chunks.
//      Being sequential by definition is what makes the result independent of tiling.  Barrier.
//   3. parallel — every lane reads G_{k+1} and stores `out`; the lane at level 0 stores G_0.
// The flux options are wave-uniform run-time branches, the tendency options template arguments through the average entries' own dispatch, as in the sibling:
// 8 + 4 kernels.  The outputs must not alias the inputs (the entries keep the rule of §(20)).
// The flux side of each scheme, the kernel-argument struct and the entry layer — so the statuses of the §(20) entries, in their order — are
// cmx_column_implicit.hpp's, shared with the sibling; here are the kernel, its IO struct, its launch and the extern "C" functions.
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

// Float32: compiled for four waves per SIMD, where cmx_column_implicit_average.hip runs (without the request 130–134 registers, three waves: 1-moment 0.82 → 0.76 ms,
// SB2006 0.69 → 0.66 ms per 1e7 points at nsub = 1; no vector register spills, no scratch instruction).  Float64 sits at one wave per SIMD either way.
template <typename S, typename FX, typename FT, int K, int BS>
__global__ __launch_bounds__(BS, sizeof(FT) == 4 ? 4 : 1) void implicit_sedimentation_step_kernel(const ImplicitColumnArgs<S, FX, FT, K, ImplicitStepIO<FT>> k0) {
    using M = Math<FT>;
    constexpr int N = S::NOUT, S0 = 1 + S::SPECIES0;
    static_assert(N == 4 && S0 + N == S::NWRT + 1, "implicit_sedimentation_step_kernel: four species, the last four inputs of the point");
    __shared__ __align__(16) FT As[BS][N], Bs[BS][N], Gs[BS][N];      // A, B and G of every point of the chunk
    __shared__ FT carry[2][N];                                        // G of the point above the chunk, per species; the slots alternate from chunk to chunk
    const auto &a = k0.a;
    // the workgroup's range of whole columns: P points from flat index `base`
    const int64_t col0 = (int64_t)blockIdx.x * k0.io.cols_per_wg;
    const int64_t left = k0.io.n_col - col0;
    const uint32_t P = (uint32_t)(left < k0.io.cols_per_wg ? left : (int64_t)k0.io.cols_per_wg) * (uint32_t)k0.io.n_lev;
    const int64_t base = col0 * k0.io.n_lev;
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    uint32_t par = 0;
#pragma unroll 1
    for (uint32_t cs = (P - 1) / BS * BS;; cs -= BS) {      // chunks [cs, cs + BS) ∩ [0, P) of the range, the highest first
        const uint32_t rel = cs + threadIdx.x;
        const bool active = rel < P;
        const int64_t i = base + rel;
        FT hq[N], rr[N], g = FT(0);
        uint32_t lev = 0, relcol = 0;
        bool top = false;
        if (active) {
            FT x[S::NWRT + 1], s0[N], avg[N], F[N], w[N];
#pragma unroll
            for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
#pragma unroll
            for (int q = 0; q < N; ++q) s0[q] = x[S0 + q];
            implicit_average_substeps<S, FT, K>(k0.ka.c, a, x, avg);
            // ---- fluxes and fall speeds of the INITIAL state
            {
                const auto &kq = consts_after(front_consts<FT, true>(k0), avg[N - 1]);
                const int32_t opt[2] = {kq.io.opt[0], kq.io.opt[1]};
                FX::fluxes(k0.ka, avg[N - 1], opt, x[0], s0, F, w);
            }
            const auto &kp = consts_after(front_consts<FT, true>(k0), F[N - 1]);
            const auto &io = kp.io;
            const FastDivU32 dv{io.lev_div.magic, io.lev_div.sh1, io.lev_div.sh2, io.lev_div.d};
            relcol = fastdiv(rel, dv);
            lev = rel - relcol * (uint32_t)io.n_lev;
            top = lev == (uint32_t)io.n_lev - 1;          // nothing enters through the model top
            const FT idz = io.inv_dz[lev];
            const FT rp = max0(x[0]);
            g = idz * FX::inv_rho(x[0]);                  // 1/(ρ_k Δz_k)
            const int32_t opt[2] = {io.opt[0], io.opt[1]};
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const FT tau = io.dt * w[q];
                const FT c = tau * idz, beta = tau * rp;
                const FT r = FT(1) / (FT(1) + c);         // a true division: exactly 1 at c = 0
                As[threadIdx.x][q] = c * r;
                Bs[threadIdx.x][q] = M::fma(beta, avg[q], F[q]) * r;
                rr[q] = r;
                hq[q] = FX::falls(q, opt) ? M::fma(-F[q], g, avg[q]) : avg[q];
            }
        }
        __syncthreads();
        {   // ---- the chains of the chunk: lane → (segment = the part of one column inside the chunk, species)
            const auto &io = consts_after(front_consts<FT, true>(k0), g).io;
            const uint32_t n_lev = (uint32_t)io.n_lev;
            const uint32_t ce = cs + BS < P ? cs + BS : P;
            const FastDivU32 dv{io.lev_div.magic, io.lev_div.sh1, io.lev_div.sh2, io.lev_div.d};
            const uint32_t colA = fastdiv(cs, dv), nseg = fastdiv(ce - 1, dv) - colA + 1;
            for (uint32_t sl = threadIdx.x; sl < nseg * N; sl += BS) {
                const uint32_t q = sl % N, col = colA + sl / N;
                const uint32_t cb = col * n_lev, ct = cb + n_lev;       // the column: [cb, ct) of the range
                const uint32_t lo = cb > cs ? cb : cs, hi = ct < ce ? ct : ce;
                const bool from_top = hi == ct;
                uint32_t p = hi - 1 - cs;
                const FT Gup = carry[par][q];
                FT G = from_top ? Bs[p][q] : M::fma(As[p][q], Gup, Bs[p][q]);      // a select: nothing crosses a column top
                Gs[p][q] = G;
#pragma unroll 4
                for (uint32_t m = hi - lo - 1; m > 0; --m) {
                    --p;
                    G = M::fma(As[p][q], G, Bs[p][q]);
                    Gs[p][q] = G;
                }
                if (lo > cb) carry[par ^ 1][q] = G;       // the column goes on in the next chunk
            }
        }
        __syncthreads();
        if (active) {
            const auto &kp = consts_after(front_consts<FT, true>(k0), g);
            const auto &io = kp.io;
            const int32_t opt[2] = {io.opt[0], io.opt[1]};
#pragma unroll
            for (int q = 0; q < N; ++q) {
                FT up = FT(0);
                if (!top) up = threadIdx.x == BS - 1 ? carry[par][q] : Gs[threadIdx.x + 1 < BS ? threadIdx.x + 1 : 0][q];
                const FT o = M::fma(up, g, hq[q]) * rr[q];
                kp.a.avg[q][i] = FX::falls(q, opt) ? o : hq[q];
            }
            if (lev == 0) {                               // the flux that leaves the column during the step
                const int64_t col = col0 + relcol;
                if constexpr (FX::precip(0) >= 0)
                    if (io.precip[0]) io.precip[0][col] = Gs[threadIdx.x][FX::precip(0)];
                if constexpr (FX::precip(1) >= 0)
                    if (io.precip[1]) io.precip[1][col] = Gs[threadIdx.x][FX::precip(1)];
            }
        }
        par ^= 1;
        if (cs == 0) break;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
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
// (n_col ≤ kMaxPoints / n_lev and at least 16 points per workgroup — n_lev ≥ 16, or ≥ 512 columns of fewer levels — keep the grid inside HIP's 2^31 − 1)
template <typename FT> static dim3 step_grid(const ImplicitStepIO<FT> &io) { return dim3((unsigned)tile_grid(io.n_col, io.cols_per_wg)); }

// the callable of the entry layer (cmx_column_implicit.hpp): the IO struct and the launch
template <typename FT> static auto step_launch(const FT *inv_dz, FT *precip0, FT *precip1, int64_t n_col, int32_t n_lev, double dt, void *stream) {
    return [=](auto scheme, auto fx, const auto &ka, const auto &a, int32_t opt0, int32_t opt1) -> int32_t {
        constexpr int K = kImplicitAvgK<FT>;
        const ImplicitColumnArgs<decltype(scheme), decltype(fx), FT, K, ImplicitStepIO<FT>> k{ka, a, make_io<FT>(inv_dz, precip0, precip1, n_col, n_lev, opt0, opt1, dt)};
        launch_grid(implicit_sedimentation_step_kernel<decltype(scheme), decltype(fx), FT, K, kImplStepBS>, step_grid(k.io), dim3(kImplStepBS), 0,
                    reinterpret_cast<hipStream_t>(stream), k);
        return launched();
    };
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_column_implicit_step_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                            const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const float *inv_dz, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                            const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt,
                                            float *dn_rai_dt, float *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<float>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                    {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                    cmx::step_launch<float>(inv_dz, precip_flux, nullptr, n_col, n_lev, dt, stream));
}
int32_t cmx_sb2006_column_implicit_step_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                            const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const double *inv_dz, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                            const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt,
                                            double *dq_rai_dt, double *dn_rai_dt, double *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<double>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                     {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                     cmx::step_launch<double>(inv_dz, precip_flux, nullptr, n_col, n_lev, dt, stream));
}
int32_t cmx_mp1m_column_implicit_step_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                          const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *const *in,
                                          float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                  cmx::step_launch<float>(inv_dz, precip_rai, precip_sno, n_col, n_lev, dt, stream));
}
int32_t cmx_mp1m_column_implicit_step_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                          const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *const *in,
                                          double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                   cmx::step_launch<double>(inv_dz, precip_rai, precip_sno, n_col, n_lev, dt, stream));
}
}
