// cmx_column_implicit_average.hip — the column steps with the sub-stepped implicit average as tendency operator: per point the average tendency of
// include/cmx.h §(19) (cmx_jacobian.hpp implicit_average_substeps) and, in the same pass, the first-order upwind sedimentation of the existing column steps
// (cmx_sb2006_column.hip, cmx_mp1m_column.hip) evaluated at the INITIAL state; C-ABI entry points cmx_sb2006_column_implicit_average_sedimentation_* and
// cmx_mp1m_column_implicit_average_sedimentation_* (include/cmx.h §(20)).  One kernel family for both schemes and both float types:
//     out_j[k] = fma(top ? 0 : F_j[k+1], g, fma(−F_j[k], g, a_j)),   g = inv_dz[k] / ρ_k
// with a_j the average of §(19) bit for bit and F, g the fluxes and 1/(ρ Δz) of the scheme's column entry bit for bit.
//
// Kernel shape: ONE point per lane in both float types.  The average is bound by VALU issue (hundreds of instructions per pass, nsub·4/K passes),
// so the 16-byte accesses, the alignment split and the f32x2 pairing of the streaming column kernels buy nothing here; any alignment and any n go through one
// launch.  A lane
//   1. reads its seven values and runs the substeps, the averages left in registers: the loop of implicit_average_substeps (cmx_jacobian.hpp), of which this
//      kernel keeps a copy because the call was measured slower here (the comment at the loop has the numbers);
//   2. AFTER the loop evaluates the flux-only function of the scheme (sed_fluxes_of_point, cmx_sb2006_sed.hpp; mp1m_sed_fluxes, cmx_mp1m_vel.hpp) from ρ and
//      the initial species, which the loop keeps in registers anyway: nothing of the fluxes is live across the point function.  The flux constants are read
//      through the kernel-argument segment at this point (front_consts, consts_after), in both float types;
//   3. passes its fluxes to the lane below through LDS (halo[BS][4], one barrier).  The point after the tile is another workgroup's: tiles overlap by one lane,
//      and the workgroup's last lane holds that point, evaluates its fluxes — and only its fluxes, from the raw columns — and stores nothing.  It is never
//      run through the substeps: the lane idles while its wave runs them.  Every flux comes from one function of (ρ, species) alone, so results do not
//      depend on where tile boundaries fall.
// The flux options — rain velocity scheme, cloud sedimentation, run-time Γ — are wave-uniform run-time branches around the existing flux functions'
// instantiations (the same inline code on the same operands: the same bits); the tendency options are template arguments through the average entries' own
// dispatch (the flags of with_sb2006_jac, with_mp1m_jac).  8 + 4 kernels.  The outputs must not alias the inputs: lane BS − 1 reads the next tile's first point.
// The flux side of each scheme, the kernel-argument struct and the entry layer (checks, constants) are cmx_column_implicit.hpp's, shared with
// cmx_column_implicit_step.hip; here are the kernel, its IO struct, its launch and the extern "C" functions.
#include "cmx_column_implicit.hpp"

namespace cmx {

#ifndef CMX_IMPLICIT_COLUMN_BS
#define CMX_IMPLICIT_COLUMN_BS 256
#endif
constexpr int kImplColBS = CMX_IMPLICIT_COLUMN_BS;

template <typename FT> struct ImplicitColIO {
    const FT *inv_dz;      // n_lev values 1/Δz_k
    FT *precip[2];         // n_col values each or nullptr: the surface fluxes F_0 of the species FX::precip(0), FX::precip(1)
    int64_t n;             // n_col · n_lev
    int32_t n_lev;
    int32_t opt[2];        // the flux options of the scheme (SbFlux: velocity kind, cloud sedimentation; Mp1mFlux: run-time Γ)
    double inv_n_lev;
    FastDivU32 lev_div;    // division by n_lev for flat indices below 2³² (cmx_launch.hpp fastdiv)
};

// S: the scheme of the average entries (SbJac<…>, Mp1mJac<…>); FX: its flux side.
template <typename S, typename FX, typename FT, int K, int BS>
__global__ __launch_bounds__(BS) void implicit_average_column_kernel(const ImplicitColumnArgs<S, FX, FT, K, ImplicitColIO<FT>> k0) {
    using M = Math<FT>;
    constexpr int N = S::NOUT, S0 = 1 + S::SPECIES0;
    static_assert(N == 4 && S0 + N == S::NWRT + 1, "implicit_average_column_kernel: four species, the last four inputs of the point");
    // Tiles OVERLAP by one lane, as in the streaming column kernels: workgroup b owns the points [b(BS − 1), (b + 1)(BS − 1)); its lane BS − 1 holds the first
    // point of the next tile, skips the substeps and only supplies the fluxes that point sends down to lane BS − 2.  Every wave then evaluates the flux
    // function exactly once.  (First form: tiles of BS points and a second trip of the tile's last lane through the flux code for the point after the tile —
    // at the one wave per SIMD of the Float64 instantiations the whole workgroup waited at the barrier for that second trip: DESIGN.md §9 has both times.)
    constexpr int OWN = BS - 1;
    __shared__ __align__(16) FT halo[BS][N];      // the fluxes of every lane's point
    const auto &a = k0.a;
    const int64_t i = (int64_t)blockIdx.x * OWN + threadIdx.x;
    const bool active = i < k0.io.n;
    FT x[S::NWRT + 1];
    if (active) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    FT avg[N] = {}, F[N];
    if (active) {
        FT s0[N];
#pragma unroll
        for (int q = 0; q < N; ++q) s0[q] = x[S0 + q];
        if (threadIdx.x < OWN) {
            // ---- the substeps: implicit_average_substeps (cmx_jacobian.hpp) operation for operation.  The one copy of that loop, kept because it was
            // measured: with the call in its place this kernel compiles to the same instructions on permuted registers (same VGPR / SGPR / spill counts)
            // and runs slower at 1e7 points — Float64 SB2006 3.890 → 3.947 ms, 1-moment 4.784 → 4.849 ms at nsub = 4 against a spread of 0.010 / 0.012 ms;
            // with s0 handed to the core the same.  The same code at another address runs as before, so it is not placement (HISTORY.md has the table).
            // tests/test_column_implicit_average_gpu.py holds this copy to the average entry in every bit.
            const bool limit = a.step_flags & CMX_STEP_NONNEGATIVE;
#pragma unroll 1
            for (int32_t sub = 0; sub < a.nsub; ++sub) {
                FT r[N], d[N];
                implicit_solve<S, FT, K>(k0.ka.c, a.wrt, a.h, x, r);
                const auto poison = S::poison(x);
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const FT s = x[S0 + q];
                    FT sn = s + S::out(r[q], poison) * a.h;
                    if (limit) {
                        const FT lo = s < FT(0) ? s : FT(0);
                        sn = sn < lo ? lo : sn;
                    }
                    d[q] = (sn - s) * a.inv_h;
                    x[S0 + q] = sn;
                }
                if constexpr (S::TEMP >= 0) x[1 + S::TEMP] = x[1 + S::TEMP] + S::heating(a.Lv, a.Ls, d) * a.h;
            }
#pragma unroll
            for (int q = 0; q < N; ++q) avg[q] = (x[S0 + q] - s0[q]) * a.inv_dt;
        }
        // ---- the fluxes of the INITIAL state of the lane's point, from ρ and the species the loop kept
        const auto &kp = consts_after(front_consts<FT, true>(k0), avg[N - 1]);
        const int32_t opt[2] = {kp.io.opt[0], kp.io.opt[1]};
        FX::fluxes(k0.ka, avg[N - 1], opt, x[0], s0, F);
#pragma unroll
        for (int q = 0; q < N; ++q) halo[threadIdx.x][q] = F[q];
    }
    __syncthreads();
    if (!active || threadIdx.x >= OWN) return;
    const auto &kp = consts_after(front_consts<FT, true>(k0), F[N - 1]);
    const auto &io = kp.io;
    // i = col·n_lev + lev
    int64_t col;
    int32_t lev;
    if (io.n < ((int64_t)1 << 32)) {             // wave-uniform: one v_mul_hi_u32 (cmx_launch.hpp fastdiv)
        const FastDivU32 dv{io.lev_div.magic, io.lev_div.sh1, io.lev_div.sh2, io.lev_div.d};
        const uint32_t c32 = fastdiv((uint32_t)i, dv);
        col = c32;
        lev = (int32_t)((uint32_t)i - c32 * (uint32_t)io.n_lev);
    } else {                                     // one double multiply + fix-up per lane; exact below 2^53
        col = (int64_t)((double)i * io.inv_n_lev);
        int64_t k64 = i - col * io.n_lev;
        if (k64 < 0) { --col; k64 += io.n_lev; }
        if (k64 >= io.n_lev) { ++col; k64 -= io.n_lev; }
        lev = (int32_t)k64;
    }
    const bool top = lev == io.n_lev - 1;        // nothing enters through the model top
    const FT g = io.inv_dz[lev] * FX::inv_rho(x[0]);      // 1/(ρ_k Δz_k)
    const int32_t opt[2] = {io.opt[0], io.opt[1]};
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const FT up = halo[threadIdx.x + 1][q];  // (the last point of the call is a top: the select drops what its lane read)
        const FT o = M::fma(top ? FT(0) : up, g, M::fma(-F[q], g, avg[q]));
        kp.a.avg[q][i] = FX::falls(q, opt) ? o : avg[q];
    }
    if (lev == 0) {                              // surface precipitation fluxes of the column
        if constexpr (FX::precip(0) >= 0)
            if (io.precip[0]) io.precip[0][col] = F[FX::precip(0)];
        if constexpr (FX::precip(1) >= 0)
            if (io.precip[1]) io.precip[1][col] = F[FX::precip(1)];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// the grid of n points: tiles overlap by one lane (n ≤ kMaxPoints keeps it inside HIP's 2^31 − 1 workgroups)
static dim3 column_grid(int64_t n) { return dim3((unsigned)tile_grid(n, kImplColBS - 1)); }

template <typename FT> static ImplicitColIO<FT> make_io(const FT *inv_dz, FT *precip0, FT *precip1, int64_t n, int32_t n_lev, int32_t opt0, int32_t opt1) {
    ImplicitColIO<FT> io{};
    io.inv_dz = inv_dz;
    io.precip[0] = precip0;
    io.precip[1] = precip1;
    io.n = n;
    io.n_lev = n_lev;
    io.opt[0] = opt0;
    io.opt[1] = opt1;
    io.inv_n_lev = 1.0 / (double)n_lev;
    io.lev_div = make_fastdiv((uint32_t)n_lev);
    return io;
}

// the callable of the entry layer (cmx_column_implicit.hpp): the IO struct and the launch
template <typename FT> static auto column_launch(const FT *inv_dz, FT *precip0, FT *precip1, int64_t n_col, int32_t n_lev, void *stream) {
    return [=](auto scheme, auto fx, const auto &ka, const auto &a, int32_t opt0, int32_t opt1) -> int32_t {
        constexpr int K = kImplicitAvgK<FT>;
        const int64_t n = n_col * (int64_t)n_lev;
        const ImplicitColumnArgs<decltype(scheme), decltype(fx), FT, K, ImplicitColIO<FT>> k{ka, a, make_io<FT>(inv_dz, precip0, precip1, n, n_lev, opt0, opt1)};
        launch_grid(implicit_average_column_kernel<decltype(scheme), decltype(fx), FT, K, kImplColBS>, column_grid(n), dim3(kImplColBS), 0,
                    reinterpret_cast<hipStream_t>(stream), k);
        return launched();
    };
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_column_implicit_average_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                                             const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev,
                                                             const float *inv_dz, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                                             const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
                                                             float *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<float>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                    {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                    cmx::column_launch<float>(inv_dz, precip_flux, nullptr, n_col, n_lev, stream));
}
int32_t cmx_sb2006_column_implicit_average_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                                             const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev,
                                                             const double *inv_dz, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                                             const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                             double *precip_flux, void *stream) {
    return cmx::sb2006_implicit_column_entry<double>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz,
                                                     {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai}, {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt},
                                                     cmx::column_launch<double>(inv_dz, precip_flux, nullptr, n_col, n_lev, stream));
}
int32_t cmx_mp1m_column_implicit_average_sedimentation_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                                           const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                           const float *const *in, float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                cmx::column_launch<float>(inv_dz, precip_rai, precip_sno, n_col, n_lev, stream));
}
int32_t cmx_mp1m_column_implicit_average_sedimentation_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                                           const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                           const double *const *in, double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::mp1m_implicit_column_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out,
                                                 cmx::column_launch<double>(inv_dz, precip_rai, precip_sno, n_col, n_lev, stream));
}
}
