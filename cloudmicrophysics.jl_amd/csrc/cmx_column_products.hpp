// cmx_column_products.hpp — what the derivative entries of the column steps with sedimentation share, whatever the scheme and whatever is differentiated
// (include/cmx.h §(25)–(28): cmx_sb2006_column_products.hip, cmx_sb2006_column_param.hip, cmx_mp1m_column_products.hip, cmx_mp1m_column_param.hip, and their
// host mirrors tests/native/column_*_host.cpp): what a point keeps between its evaluation and its stores, the ONE status ladder of the entries, and — device
// build only — the three kernel shells with their launches.  A scheme and operation enters a shell as a policy struct `B` (the four .hip files have them):
//     B::S         the scheme (NWRT differentiated inputs next to ρ)         B::FT   the float type
//     B::Consts    the constants, ONE by-value struct and the FIRST kernel argument: the Float64 point functions read it through front_consts() at offset 0
//                  of the kernel-argument segment (cmx_math.hpp), so the scheme's own constants are its first member
//     halo shell   B::Args, B::Point (what a point keeps: ColumnPoint, or the scheme's own struct of one tangent) with B::Fd(p, k, s), the tangent in slot k
//                  of flux s; B::NT tangents per point, B::TANGENTS (the caller's tangent columns a.tan are loaded), B::eval(c, x, t, inv_dz, p) and
//                  B::store(a, p, upv, upd, top, surface, i, col)
//     point shell  B::VjpArgs<K> and B::vjp_point<K>(c, a, x, i, col, lev)
//     chunk shell  B::GradArgs, B::NT directions per evaluation and B::grad_point(c, a, x, i, col, lev, acc)
// No HIP outside the CMX_HOST_BUILD guard.
#pragma once
#include <cstdint>

#include "../../include/cmx.h"

namespace cmx {

constexpr int kColumnInputs = 7;      // ρ and the six differentiated inputs of either scheme

// What a point keeps between its evaluation and its stores: A = sum − (own flux)·g, value and NT tangents (final but for the inflow), the four fluxes it sends
// down, g
template <typename FT, int NT> struct ColumnPoint {
    FT Av[4], Ad[NT][4];
    FT Fv[4], Fd[NT][4];
    FT g;
};

// ---- the status ladder --------------------------------------------------------------------------------------------------------------------------------
// n_col·n_lev must fit one launch: kMaxPoints of cmx_launch.hpp, which the host build cannot include
constexpr int64_t kColumnMaxPoints = 16ll * 0x7fffffffll;

// the direction table of a parameter-derivative entry
struct ColumnDirs {
    int32_t ndir;
    const void *table;
};

// column_entry_status: "every check passed, set up and launch" — not a CMX status (those are ≤ 0)
constexpr int32_t kColumnEntryRun = 1;

// The statuses every column-derivative entry shares, after the NULL checks of the scheme's parameter structs and in this order: the counts; the flags
// (`flags_status`, the scheme's own function of them); the limit on n_col·n_lev; no point at all (CMX_OK — but the gradient entry writes grad, so it goes on
// and is checked like any other call except for the columns, which it does not read); the columns; the direction table (`dirs`, NULL: the entry has none);
// grad and workspace, the last two of `outs`, for the gradient entry; at least one output for the others; no output is an input — a lane reads its
// neighbours' state and cotangents.  `in` (kColumnInputs columns) and `inv_dz` may be NULL when there is no point, and NULL members are not compared.
template <typename FT>
inline int32_t column_entry_status(int64_t n_col, int32_t n_lev, int32_t flags_status, const FT *inv_dz, const FT *const *in, const ColumnDirs *dirs,
                                   const void *const *given, int ngiven, void *const *outs, int nouts, bool gradient) {
    if (n_col < 0 || n_lev < 1) return CMX_ERR_BAD_ARG;
    if (flags_status) return flags_status;
    if (n_col > kColumnMaxPoints / n_lev) return CMX_ERR_UNSUPPORTED;
    if (n_col == 0 && !gradient) return CMX_OK;
    if (n_col > 0) {
        if (!inv_dz || !in) return CMX_ERR_BAD_ARG;
        for (int j = 0; j < kColumnInputs; ++j)
            if (!in[j]) return CMX_ERR_BAD_ARG;
    }
    if (dirs && (dirs->ndir < 1 || dirs->ndir > CMX_PARAM_MAX_DIRS || !dirs->table)) return CMX_ERR_BAD_ARG;
    if (gradient && (!outs[nouts - 2] || !outs[nouts - 1])) return CMX_ERR_BAD_ARG;
    bool any = gradient;
    for (int o = 0; o < nouts; ++o) {
        if (!outs[o]) continue;
        any = true;
        if (outs[o] == (const void *)inv_dz) return CMX_ERR_BAD_ARG;
        for (int j = 0; in && j < kColumnInputs; ++j)
            if (outs[o] == (const void *)in[j]) return CMX_ERR_BAD_ARG;
        for (int g = 0; g < ngiven; ++g)
            if (outs[o] == given[g]) return CMX_ERR_BAD_ARG;
    }
    return any ? kColumnEntryRun : (int32_t)CMX_ERR_BAD_ARG;
}

}  // namespace cmx

#if !defined(CMX_HOST_BUILD)
#include "cmx_column_geom.hpp"
#include "cmx_jacobian.hpp"
#include "cmx_launch.hpp"

namespace cmx {

static_assert(kColumnMaxPoints == kMaxPoints, "one limit on the points of a launch");

// Lanes per workgroup of the halo and point shells: a tuning number (-DCMX_COLPROD_BS=…).  The chunk shell's is the reduction's: stage 2
// (param_vjp_finish_kernel) gives each of its lanes four partials.
#ifndef CMX_COLPROD_BS
#define CMX_COLPROD_BS 256
#endif
constexpr int kColProdBS = CMX_COLPROD_BS;
constexpr int kColGradBS = CMX_PARAM_VJP_PARTIALS / 4;

// stage 2 of the reduction: param_vjp_finish_kernel, launched by its one instantiation (cmx_sb2006_param.hip)
void launch_param_vjp_finish(int32_t ndir, const double *workspace, double *grad, hipStream_t stream);

// ---- the halo shell: forward mode over the column -----------------------------------------------------------------------------------------------------
// Tiled like the primal column kernels: lanes run along the flat index i = col·n_lev + k, workgroup b owns the points [b(BS−1), (b+1)(BS−1)), its lane BS−1
// evaluates the first point of the next tile like any other lane and only supplies what that point sends down.  The LDS halo carries the value F and the NT
// tangents Ḟ of every lane's four fluxes: [0 … 3] F, [4(1 + k) … 4(1 + k) + 3] Ḟ of slot k.  Every lane runs the same evaluation, so a result does not
// depend on where a tile boundary falls, bit for bit.  One point per lane in BOTH float types: 4- / 8-byte accesses, so any alignment and any n go through
// ONE launch, and the launch's last point is the top of the last column — no point follows the last tile, and no flux-only evaluation of one is needed.
// No lane leaves before the two barriers (the one inside Math::prepare, the halo's): inactive lanes and the non-owner lane skip work instead.
template <typename B, int BS>
__global__ __launch_bounds__(BS) void column_halo_kernel(const typename B::Consts c, const typename B::Args a, const ColGeom geom) {
    using S = typename B::S;
    using FT = typename B::FT;
    constexpr int NT = B::NT;
    __shared__ __align__(16) FT halo[BS][4 * (1 + NT)];
    const int64_t i = (int64_t)blockIdx.x * (BS - 1) + threadIdx.x;
    const bool active = i < a.n;
    const bool owner = threadIdx.x < BS - 1;      // lane BS−1 never stores: its point belongs to the next workgroup
    FT x[S::NWRT + 1], t[S::NWRT];
    if (active) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
        if constexpr (B::TANGENTS) {
#pragma unroll
            for (int j = 0; j < S::NWRT; ++j) t[j] = a.tan[j] ? __builtin_nontemporal_load(a.tan[j] + i) : FT(0);
        }
    }
    Math<FT>::prepare();   // Float64: exp2 / log2 tables → LDS while the loads fly (every lane of the workgroup reaches the barrier inside); no-op for Float32
    int64_t col = 0;
    int32_t lev = 0;
    typename B::Point p;
    if (active) {
        column_level(geom, i, col, lev);
        B::eval(c, x, t, a.inv_dz[lev], p);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            halo[threadIdx.x][s] = p.Fv[s];
#pragma unroll
            for (int k = 0; k < NT; ++k) halo[threadIdx.x][4 * (1 + k) + s] = B::Fd(p, k, s);
        }
    }
    __syncthreads();
    if (!active || !owner) return;
    const bool top = lev == a.n_lev - 1;
    // the cell above is the next lane's point (an owner's next lane exists in its workgroup; it is active unless this point is the launch's last, a top)
    FT upv[4] = {FT(0), FT(0), FT(0), FT(0)}, upd[NT][4];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int s = 0; s < 4; ++s) upd[k][s] = FT(0);
    if (!top) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            upv[s] = halo[threadIdx.x + 1][s];
#pragma unroll
            for (int k = 0; k < NT; ++k) upd[k][s] = halo[threadIdx.x + 1][4 * (1 + k) + s];
        }
    }
    B::store(a, p, upv, upd, top, lev == 0, i, col);
}

// tiles overlap by one lane
template <typename B> inline void launch_column_halo(const typename B::Consts &c, const typename B::Args &a, hipStream_t stream) {
    launch_grid(column_halo_kernel<B, kColProdBS>, dim3((unsigned)tile_grid(a.n, kColProdBS - 1)), dim3(kColProdBS), 0, stream, c, a, make_col_geom(a.n, a.n_lev));
}

// ---- the point shell: Jᵀḡ -----------------------------------------------------------------------------------------------------------------------------
// Pointwise, no LDS and no barrier beyond the Float64 math tables: what a point needs of its neighbours — ρ and the cotangents of the point below for λ, the
// state of the point above for a requested primal output — its body reads raw.
template <typename B, int K, int BS>
__global__ __launch_bounds__(BS) void column_point_kernel(const typename B::Consts c, const typename B::template VjpArgs<K> a, const ColGeom geom) {
    using S = typename B::S;
    using FT = typename B::FT;
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    FT x[S::NWRT + 1];
    if (i < a.n) {
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
    }
    Math<FT>::prepare();
    if (i >= a.n) return;
    int64_t col;
    int32_t lev;
    column_level(geom, i, col, lev);
    B::template vjp_point<K>(c, a, x, i, col, lev);
}

template <typename B, int K> inline void launch_column_point(const typename B::Consts &c, const typename B::template VjpArgs<K> &a, hipStream_t stream) {
    launch<kColProdBS>(column_point_kernel<B, K, kColProdBS>, a.n, stream, c, a, make_col_geom(a.n, a.n_lev));
}

// ---- the chunk shell: stage 1 of a parameter gradient ---------------------------------------------------------------------------------------------------
// param_vjp_kernel (cmx_jacobian.hpp) with the point's place in its column: workgroup b owns the chunk [b·chunk, (b + 1)·chunk), lane t its points t, t + BS, …
// in index order, then param_vjp_reduce — deterministic, no atomics, no allocation.
template <typename B, int BS>
__global__ __launch_bounds__(BS) void column_param_vjp_kernel(const typename B::Consts c, const typename B::GradArgs a, const ColGeom geom, const int64_t chunk,
                                                              const int32_t nlive, double *__restrict__ ws) {
    using S = typename B::S;
    using FT = typename B::FT;
    constexpr int KP = B::NT;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < a.n ? lo + chunk : a.n;
    Math<FT>::prepare();
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int64_t i = lo + threadIdx.x; i < hi; i += BS) {
        FT x[S::NWRT + 1];
#pragma unroll
        for (int j = 0; j < S::NWRT + 1; ++j) x[j] = __builtin_nontemporal_load(a.in[j] + i);
        int64_t col;
        int32_t lev;
        column_level(geom, i, col, lev);
        B::grad_point(c, a, x, i, col, lev, acc);
    }
    param_vjp_reduce<KP, BS>(acc, nlive, ws);
}

// the launch of the directions d0 … d0 + NT − 1 of ndir: their partial sums go to their rows of the workspace
template <typename B>
inline void launch_column_param_vjp(const typename B::Consts &c, const typename B::GradArgs &a, int d0, int32_t ndir, double *workspace, hipStream_t stream) {
    const int32_t nlive = ndir - d0 < B::NT ? ndir - d0 : B::NT;
    launch_grid(column_param_vjp_kernel<B, kColGradBS>, dim3(CMX_PARAM_VJP_PARTIALS), dim3(kColGradBS), 0, stream, c, a, make_col_geom(a.n, a.n_lev),
                param_vjp_chunk(a.n, kColGradBS), nlive, workspace + (int64_t)d0 * CMX_PARAM_VJP_PARTIALS);
}

}  // namespace cmx
#endif
