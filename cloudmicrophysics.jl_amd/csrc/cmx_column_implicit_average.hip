// cmx_column_implicit_average.hip — the column steps with the sub-stepped implicit average as tendency operator: per point the average tendency of
// include/cmx.h §(19) (cmx_jacobian.hpp implicit_average_point) and, in the same pass, the first-order upwind sedimentation of the existing column steps
// (cmx_sb2006_column.hip, cmx_mp1m_column.hip) evaluated at the INITIAL state; C-ABI entry points cmx_sb2006_column_implicit_average_sedimentation_* and
// cmx_mp1m_column_implicit_average_sedimentation_* (include/cmx.h §(20)).  One kernel family for both schemes and both float types:
//     out_j[k] = fma(top ? 0 : F_j[k+1], g, fma(−F_j[k], g, a_j)),   g = inv_dz[k] / ρ_k
// with a_j the average of §(19) bit for bit and F, g the fluxes and 1/(ρ Δz) of the scheme's column entry bit for bit.
//
// Kernel shape: ONE point per lane in both float types.  The average is bound by VALU issue (hundreds of instructions per pass, nsub·4/K passes),
// so the 16-byte accesses, the alignment split and the f32x2 pairing of the streaming column kernels buy nothing here; any alignment and any n go through one
// launch.  A lane
//   1. reads its seven values and runs the substeps — the loop of implicit_average_point, written a second time below because the averages are needed in
//      registers and not in memory (implicit_average_point and the kernels that call it are untouched and keep their code);
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
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_mp1m_jacobian.hpp"
#include "cmx_mp1m_vel.hpp"
#include "cmx_sb2006_jacobian.hpp"
#include "cmx_sb2006_sed.hpp"

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

// ---- the flux side of a scheme: its constants (kernel argument KA: the tendency constants FIRST, where the scheme's eval reads them through front_consts),
// 1/ρ as the scheme's column entry forms it, and the fluxes of the four species of one raw point in the order of the outputs -------------------------------
template <typename FT, bool LIMITED> struct SbFlux {
    struct KA { SbConsts<FT> c; CloudVelConsts<FT> cv; };
    static constexpr int precip(int p) { return p == 0 ? CMX_SB2006_JAC_DQ_RAI_DT : -1; }      // the species of io.precip[p], −1: none
    // sb2006_point: ρ^(-1/2) of the clamped ρ, squared
    static __device__ __forceinline__ FT inv_rho(FT rho) {
        const FT rs_rho = Math<FT>::rsqrt(max0(rho));
        return rs_rho * rs_rho;
    }
    // without cloud sedimentation q_lcl and n_lcl do not fall: their outputs are the averages themselves
    static __device__ __forceinline__ bool falls(int q, const int32_t (&opt)[2]) { return q >= CMX_SB2006_JAC_DQ_RAI_DT || opt[1] != 0; }
    template <int VEL, bool CLOUD, typename C>
    static __device__ __forceinline__ void one(const C &c, const CloudVelConsts<FT> &cv, FT rho, const FT (&s)[4], FT (&F)[4]) {
        const SedFlux<FT> f = sed_fluxes_of_point<FT, LIMITED, VEL, CLOUD>(c, cv, rho, s[0], s[1], s[2], s[3]);
        F[CMX_SB2006_JAC_DQ_LCL_DT] = f.q_lcl;
        F[CMX_SB2006_JAC_DN_LCL_DT] = f.n_lcl;
        F[CMX_SB2006_JAC_DQ_RAI_DT] = f.q_rai;
        F[CMX_SB2006_JAC_DN_RAI_DT] = f.n_rai;
    }
    // s: q_lcl, n_lcl, q_rai, n_rai.  `dep`: the value the constants wait for (consts_after)
    static __device__ __forceinline__ void fluxes(const KA &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4]) {
        const auto &c = consts_after(front_consts<FT, true>(ka), dep).c;
        if (opt[0] == VEL_SB) {
            if (opt[1]) one<VEL_SB, true>(c, ka.cv, rho, s, F);
            else one<VEL_SB, false>(c, ka.cv, rho, s, F);
        } else if (opt[0] == VEL_CHEN) {
            if (opt[1]) one<VEL_CHEN, true>(c, ka.cv, rho, s, F);
            else one<VEL_CHEN, false>(c, ka.cv, rho, s, F);
        } else {
            if (opt[1]) one<VEL_CHEN_GEN, true>(c, ka.cv, rho, s, F);
            else one<VEL_CHEN_GEN, false>(c, ka.cv, rho, s, F);
        }
    }
};

template <typename FT> struct Mp1mFlux {
    struct KA { Mp1mConsts<FT> c; Vel1mConsts<FT> vc; };
    static constexpr int precip(int p) { return p == 0 ? CMX_MP1M_JAC_DQ_RAI_DT : CMX_MP1M_JAC_DQ_SNO_DT; }
    static __device__ __forceinline__ FT inv_rho(FT rho) { return Math<FT>::rcp(max0(rho)); }
    static __device__ __forceinline__ bool falls(int, const int32_t (&)[2]) { return true; }
    // s: q_lcl, q_icl, q_rai, q_sno
    static __device__ __forceinline__ void fluxes(const KA &ka, FT dep, const int32_t (&opt)[2], FT rho, const FT (&s)[4], FT (&F)[4]) {
        const auto &vc = consts_after(front_consts<FT, true>(ka), dep).vc;
        SedFlux4<FT> f;
        if (opt[0]) f = mp1m_sed_fluxes<FT, true>(vc, rho, s[0], s[1], s[2], s[3]);
        else f = mp1m_sed_fluxes<FT, false>(vc, rho, s[0], s[1], s[2], s[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) F[q] = f.f[q];
    }
};

// The ONE kernel argument: the constants first (the scheme's eval and the flux functions read them at offset 0 of the kernel-argument segment), then the
// average entry's arguments and the column geometry.  One struct, so that everything the lane needs only AFTER the substeps — the output pointers, the
// geometry, the flux options — can be read through the kernel-argument pointer at that point (consts_after) instead
// of waiting in SGPRs, and from there in VGPR lanes, across the point function: the Float64 instantiations have no register to spare.
template <typename S, typename FX, typename FT, int K> struct ImplicitColArgs {
    typename FX::KA ka;
    ImplicitAverageArgs<FT, K, S::NOUT, S::NWRT> a;
    ImplicitColIO<FT> io;
};

// S: the scheme of the average entries (SbJac<…>, Mp1mJac<…>); FX: its flux side.
template <typename S, typename FX, typename FT, int K, int BS>
__global__ __launch_bounds__(BS) void implicit_average_column_kernel(const ImplicitColArgs<S, FX, FT, K> k0) {
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
            // ---- the substeps: implicit_average_point (cmx_jacobian.hpp) operation for operation, the averages kept in registers instead of stored.  A
            // second copy on purpose: as a value-returning core called from both, the existing kernel would have to be shown to keep its code in every instantiation
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

// Statuses: those of cmx_sb2006_column_tendencies_sedimentation_* in its order, up to and including the columns and the limiter / fall-speed tables; then
// Δt, nsub and the step flags as the average entries check them.
template <typename FT, typename WR, typename TH, typename VL, typename ST>
static int32_t sb2006_entry(const WR *wr, const TH *tps, const VL *vel, const ST *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                            int32_t n_lev, const FT *inv_dz, const FT *const (&in)[7], FT *const (&out)[4], FT *precip, void *stream) {
    if (!wr || !tps || !vel || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(CMX_SB2006_LIMITED | CMX_VEL_SB2006 | CMX_VEL_CHEN2022)) return CMX_ERR_BAD_ARG;
    const bool sbv = flags & CMX_VEL_SB2006, chv = flags & CMX_VEL_CHEN2022;
    if (sbv == chv) return CMX_ERR_BAD_ARG;                      // exactly one rain fall-speed scheme
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz) return CMX_ERR_BAD_ARG;
    for (const FT *p : in)
        if (!p) return CMX_ERR_BAD_ARG;
    for (FT *p : out)
        if (!p) return CMX_ERR_BAD_ARG;
    const bool limited = flags & CMX_SB2006_LIMITED;
    if (limited && !sb_limiters_ok(*wr)) return CMX_ERR_BAD_ARG;      // clamp_ordered needs ordered limiter pairs
    if (sbv && !sb_rain_vel_ok(*vel, limited)) return CMX_ERR_BAD_ARG;      // the not-limited SB2006 fall speed needs aR < bR
    if (!implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    constexpr int K = kImplicitAvgK<FT>;
    ImplicitAverageArgs<FT, K, CMX_SB2006_JAC_NOUT, CMX_SB2006_JAC_NWRT> a;
    make_implicit_average_args(a, in, SbJac<false, false>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, &out[0]);
    const int velk = sbv ? VEL_SB : chen_vel_kind<FT>(vel->chen2022);   // fitted Γ(b(ρ)+1) or the general instantiation (cmx_math.hpp ChenGamma)
    const ImplicitColIO<FT> io = make_io<FT>(inv_dz, precip, nullptr, n, n_lev, velk, cloud_vel != nullptr);
    // the constants of the column entry: those of the average entries (with_sb2006_jac) plus the fall-speed members, which no tendency reads
    const SbConsts<FT> c = make_sb_consts<FT>(*wr, *tps, vel, (double)Math<FT>::eps_1m());
    CloudVelConsts<FT> cv{};
    if (cloud_vel) cv = make_cloud_vel_consts<FT>(wr->seifert_beheng.pdf_c, *cloud_vel);
    return dispatch_or((int32_t)CMX_ERR_BAD_ARG, [&](auto L, auto I) -> int32_t {
        using S = SbJac<decltype(L)::value, decltype(I)::value>;
        using FX = SbFlux<FT, decltype(L)::value>;
        const ImplicitColArgs<S, FX, FT, K> k{{c, cv}, a, io};
        launch_grid(implicit_average_column_kernel<S, FX, FT, K, kImplColBS>, column_grid(n), dim3(kImplColBS), 0, reinterpret_cast<hipStream_t>(stream), k);
        return launched();
    }, flag(limited), flag(sb_integer_exponents(*wr)));
}

// Statuses: those of cmx_mp1m_column_tendencies_sedimentation_* in its order, up to and including the columns (a single snow-shape bit, which that entry
// accepts, is CMX_ERR_UNSUPPORTED where that entry decodes the shape); then Δt, nsub and the step flags as the average entries check them.
template <typename FT, typename MP, typename TH, typename ST, typename CH, typename CI>
static int32_t mp1m_entry(const MP *mp, const TH *tps, const ST *stokes, const CH *chen_rain, const CI *chen_ice, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                          int64_t n_col, int32_t n_lev, const FT *inv_dz, const FT *const *in, FT *const *out, FT *precip_rai, FT *precip_sno,
                          void *stream) {
    if (!mp || !tps || !stokes || !chen_rain || !chen_ice || n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    const uint32_t shape_bits = flags & (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE);
    if (shape_bits == (CMX_1M_SED_SNOW_OBLATE | CMX_1M_SED_SNOW_PROLATE)) return CMX_ERR_BAD_ARG;
    if (shape_bits) return CMX_ERR_UNSUPPORTED;
    if (const int32_t st = check_flags_1m(flags)) return st;
    if (n_col > kMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;  // n_col·n_lev must fit one launch (cmx_launch.hpp)
    const int64_t n = n_col * (int64_t)n_lev;
    if (n == 0) return CMX_OK;
    if (!inv_dz || !in || !out) return CMX_ERR_BAD_ARG;
    for (int j = 0; j < 7; ++j)
        if (!in[j]) return CMX_ERR_BAD_ARG;
    for (int j = 0; j < 4; ++j)
        if (!out[j]) return CMX_ERR_BAD_ARG;
    if (!implicit_average_step_ok<FT>(dt, nsub, step_flags)) return CMX_ERR_BAD_ARG;
    constexpr int K = kImplicitAvgK<FT>;
    const FT *const cols[7] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6]};
    ImplicitAverageArgs<FT, K, CMX_MP1M_JAC_NOUT, CMX_MP1M_JAC_NWRT> a;
    make_implicit_average_args(a, cols, Mp1mJac<kDefaultFlags>::SPECIES0, dt, nsub, step_flags, (FT)tps->LH_v0, (FT)tps->LH_s0, (FT)tps->cp_d, out);
    bool general = false;
    Vel1mConsts<FT> vc = make_vel1m_consts<FT>(*mp, chen_rain, &general);
    add_sedimentation_consts<FT>(vc, *mp, stokes, chen_ice);
    const ImplicitColIO<FT> io = make_io<FT>(inv_dz, precip_rai, precip_sno, n, n_lev, general, 0);
    return with_mp1m_jac<FT>(*mp, *tps, flags, [&](const Mp1mConsts<FT> &c, auto scheme) -> int32_t {
        using S = decltype(scheme);
        const ImplicitColArgs<S, Mp1mFlux<FT>, FT, K> k{{c, vc}, a, io};
        launch_grid(implicit_average_column_kernel<S, Mp1mFlux<FT>, FT, K, kImplColBS>, column_grid(n), dim3(kImplColBS), 0, reinterpret_cast<hipStream_t>(stream), k);
        return launched();
    });
}

}  // namespace cmx

extern "C" {
int32_t cmx_sb2006_column_implicit_average_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                                             const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev,
                                                             const float *inv_dz, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                                             const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
                                                             float *precip_flux, void *stream) {
    return cmx::sb2006_entry<float>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai},
                                    {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt}, precip_flux, stream);
}
int32_t cmx_sb2006_column_implicit_average_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                                             const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev,
                                                             const double *inv_dz, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                                             const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                             double *precip_flux, void *stream) {
    return cmx::sb2006_entry<double>(warm_rain, tps, vel, cloud_vel, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, {rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai},
                                     {dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt}, precip_flux, stream);
}
int32_t cmx_mp1m_column_implicit_average_sedimentation_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                                           const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                           const float *const *in, float *const *out, float *precip_rai, float *precip_sno, void *stream) {
    return cmx::mp1m_entry<float>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}
int32_t cmx_mp1m_column_implicit_average_sedimentation_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                                           const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                           const double *const *in, double *const *out, double *precip_rai, double *precip_sno, void *stream) {
    return cmx::mp1m_entry<double>(mp, tps, stokes, chen_rain, chen_ice, flags, dt, nsub, step_flags, n_col, n_lev, inv_dz, in, out, precip_rai, precip_sno, stream);
}
}
