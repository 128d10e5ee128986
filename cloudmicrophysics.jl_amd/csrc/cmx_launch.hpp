// cmx_launch.hpp — launch geometry, vector column access and error plumbing shared by the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include <cstdint>
#include <cstdlib>

#include "../../include/cmx.h"
#include "cmx_dispatch.hpp"
#include "cmx_split.hpp"

namespace cmx {

// --- error plumbing ------------------------------------------------------------------------
void set_hip_error(hipError_t e, const char *where);   // cmx_common.hip
#define CMX_HIP_TRY(expr)                                 \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) {                           \
            ::cmx::set_hip_error(e_, #expr);              \
            return CMX_ERR_HIP;                           \
        }                                                 \
    } while (0)

// The epilogue of every entry that launched: `return launched();` reports a failed launch as CMX_ERR_HIP (where-text for cmx_last_hip_error()).
inline int32_t launched() {
    CMX_HIP_TRY(hipGetLastError());
    return CMX_OK;
}

// --- geometry ------------------------------------------------------------------------------
// MI355X: 256 CUs in 8 XCDs.  The streaming kernels are NON-persistent: one short-lived workgroup per tile
// (256 lanes; 128 for the SB2006 sweep), one lane owns 16 bytes of every column, so the grid is ≫ 256 workgroups and
// workgroup b lands on XCD b % 8 — consecutive workgroups stream consecutive tiles and each XCD L2 sees a disjoint,
// dense address set.  (A grid-stride loop over CUs × k resident workgroups was measured slower with 13 concurrent
// streams, DESIGN.md §4: every wave of the chip sits in the same load → compute → store phase.)
// Who sizes which grid: launch() below sizes the one-lane-per-item grids of the point kernels and the layout adapters with
// tile_grid; `grid_for` (capped, grid-stride) sizes sb2006_process_kernel only.  A geometry of their own have the column-sum
// reduction (fixed 2-D grid, cmx_common.hip), the column kernels (tiles that overlap by one lane, cmx_*_column.hip) and the P3
// collision kernels (collision_geometry with dynamic LDS, cmx_p3_collisions.hip).
// Who picks which instantiation: the entry, with dispatch() (cmx_dispatch.hpp) — run-time flags and modes become the kernel's template arguments
// inside one generic lambda whose body is the launch; for_each_range below adds the vector width of each range.
constexpr int kBlock = 256;

struct DeviceInfo { int cus; int blocks_per_cu; };
DeviceInfo device_info();                                // cmx_common.hip (cached per device)

inline int grid_for(int64_t work_items, int items_per_block = kBlock) {
    const DeviceInfo di = device_info();
    const int64_t need = (work_items + items_per_block - 1) / items_per_block;
    const int64_t cap = (int64_t)di.cus * di.blocks_per_cu;
    const int64_t g = need < cap ? need : cap;
    return (int)(g < 1 ? 1 : g);
}

// Upper bound on the points / states of ONE call, checked by every entry point (CMX_ERR_UNSUPPORTED above it): the streaming kernels give a
// workgroup at least 16 points, so n ≤ 16·(2^31 − 1) ≈ 3.4e10 keeps their grids inside HIP's 2^31 − 1 workgroups; at ≥ 12 B per point that is
// beyond the 288 GB of HBM anyway.  The P3 collision kernels have SMALLER tiles (Float32: 64-lane workgroups = 8 states at 8 lanes per state, 4 at
// 16) and check their own rounded-up tile count (collision_geometry, cmx_p3_collisions.hip): CMX_ERR_UNSUPPORTED above 8·(2^31 − 8) resp. 4·(…) states.
constexpr int64_t kMaxPoints = 16ll * 0x7fffffffll;

// The point-count rule of the entry points: n < 0 → CMX_ERR_BAD_ARG, n > kMaxPoints → CMX_ERR_UNSUPPORTED (one launch cannot express the
// grid), n == 0 → CMX_OK.  An entry that validates more arguments before it returns for n == 0 uses CMX_TRY_COUNT_LIMIT and tests n == 0 itself.
inline int32_t count_limit_status(int64_t n) { return n < 0 ? CMX_ERR_BAD_ARG : n > kMaxPoints ? CMX_ERR_UNSUPPORTED : CMX_OK; }
#define CMX_TRY_COUNT_LIMIT(n)                                                    \
    do {                                                                          \
        if (const int32_t st_ = ::cmx::count_limit_status(n)) return st_;         \
    } while (0)
#define CMX_TRY_COUNT(n)                                                          \
    do {                                                                          \
        CMX_TRY_COUNT_LIMIT(n);                                                   \
        if ((n) == 0) return CMX_OK;                                              \
    } while (0)

// Steps of ONE launch of the parcel-run kernel (cmx_parcel_kernels.hip); cmx_parcel_run_* splits a longer integration into consecutive launches on
// the caller's stream, which is exact: the nine state values pass through memory between launches as they are.  Every other kernel here finishes in
// milliseconds whatever its arguments; this one loops n_steps times per lane, and a launch that runs for seconds holds the device against everything
// else queued on it.  256 steps, from the timing of tools/time_parcel.py on an MI355X (1e6 parcels, 600 steps, median of 5): one 256-step launch takes
// 1.4 ms (Float32, every option off), 1.9 ms (Float32, ABIFM + Condensation + Deposition), 3.4 ms and 5.0 ms (Float64, the same two), i.e. 5.3 / 7.4 /
// 13.2 / 19.6 ps per parcel-step, linear in the parcels; the listing (626 / 1539 static VALU instructions with every option's branch counted,
// tools/isa_cost.py) had put it at 4 / 11 ms.  The split costs one read and write of the state per launch, 0.03–0.06 ms of the above.
constexpr int kParcelMaxStepsPerLaunch = CMX_PARCEL_MAX_STEPS_PER_LAUNCH;

// Workgroups for `lanes` lanes at `bs` each.  launch() passes at most kMaxPoints lanes (the count rule) at bs ≥ 16, which stays within HIP's
// 2^31 − 1 workgroups in x.
inline int64_t tile_grid(int64_t lanes, int64_t bs) { return (lanes + bs - 1) / bs; }

// Every launch goes through these two.  The arguments must have exactly the kernel's parameter types (after decay): no conversion happens
// at the launch, and a kernel whose Float64 instantiation reads its constants through front_consts() (cmx_math.hpp) from the start of the
// kernel-argument segment cannot be called with the constants struct anywhere but first.
// launch_grid: a geometry of the caller's own (kernel<<<grid, block, lds, stream>>>(args...)).
template <typename... P, typename... A>
inline void launch_grid(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &...args) {
    static_assert(sizeof...(P) == sizeof...(A) && (std::is_same_v<std::remove_cv_t<P>, std::decay_t<A>> && ...),
                  "launch arguments must have the kernel's parameter types");
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}
// launch<BS>: one lane per item, kernel<<<tile_grid(lanes, BS), BS, 0, stream>>>(args...).
template <int BS, typename... P, typename... A>
inline void launch(void (*kernel)(P...), int64_t lanes, hipStream_t stream, const A &...args) {
    static_assert(BS >= 16, "kMaxPoints assumes at least 16 lanes per workgroup");
    launch_grid(kernel, dim3((unsigned)tile_grid(lanes, BS)), dim3(BS), 0, stream, args...);
}

// The two heaviest Float64 kernels (SB2006, 1-moment) run one point per lane (8-byte loads) instead of two (16-byte): they are
// VALU-bound, not HBM-bound, and the two-points-per-lane variants spend VALU instructions on SGPR-spill traffic for the 2-SGPR
// Float64 constants (SB2006: 1307 vs 1048 instructions per point in round 1; 1-moment 4.60 → 4.36 ms per 1e8 points in a same-box
// A/B, round 2).  The lighter ones keep two points per lane (same A/B: ARG 3.25 vs 3.50 ms, ice nucleation 0.73 vs 0.88 with one).

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// --- alignment split of the streaming entry points ------------------------------------------------------------------
// Calls f(std::integral_constant<int, V>{}, lo, count) for each non-empty range of split_aligned (cmx_split.hpp, where the rule is
// explained): the scalar head (V = 1), the vector body (V = VEC) and the scalar tail (V = 1).  f offsets its IO by lo, picks the
// instantiation and launches count / V lanes.
template <typename FT, int VEC, typename F>
inline void for_each_range(const void *const *cols, int ncols, int64_t n, F &&f) {
    const Split r = split_aligned(cols, ncols, n, sizeof(FT), VEC);
    if (r.head > 0) f(std::integral_constant<int, 1>{}, (int64_t)0, r.head);
    if (r.body > 0) f(std::integral_constant<int, VEC>{}, r.head, r.body);
    if (r.tail > 0) f(std::integral_constant<int, 1>{}, r.head + r.body, r.tail);
}
template <typename FT, int VEC, size_t N, typename F>
inline void for_each_range(const void *const (&cols)[N], int64_t n, F &&f) {
    for_each_range<FT, VEC>(cols, (int)N, n, f);
}

// An optional (NULL-able) column offset by lo points: the column of range [lo, lo + count) of for_each_range.
template <typename T> inline T *shift(T *p, int64_t lo) { return p ? p + lo : p; }

// --- vector column access --------------------------------------------------------------------
template <typename FT, int VEC> struct VecT;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));
template <> struct VecT<float, 4> { using type = f32x4_t; };    // global_load_dwordx4: 16 B / lane
template <> struct VecT<float, 1> { using type = float; };
template <> struct VecT<double, 2> { using type = f64x2_t; };   // 16 B / lane as well
template <> struct VecT<double, 1> { using type = double; };

// NT = non-temporal hint: every byte of a state column is touched exactly once per sweep.
template <typename FT, int VEC, bool NT = true>
__device__ __forceinline__ void load_col(const FT *__restrict__ p, int64_t i, FT (&x)[VEC]) {
    using V = typename VecT<FT, VEC>::type;
    V v;
    if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const V *>(p) + i);
    else v = reinterpret_cast<const V *>(p)[i];
    const FT *e = reinterpret_cast<const FT *>(&v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) x[k] = e[k];
}
template <typename FT, int VEC, bool NT = true>
__device__ __forceinline__ void store_col(FT *__restrict__ p, int64_t i, const FT (&x)[VEC]) {
    using V = typename VecT<FT, VEC>::type;
    V v;
    FT *e = reinterpret_cast<FT *>(&v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) e[k] = x[k];
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<V *>(p) + i);
    else reinterpret_cast<V *>(p)[i] = v;
}

// Workgroup-base addressing (round 6): `wg` = the column's address at the workgroup's first vector — a UNIFORM pointer the compiler keeps in an SGPR pair —
// plus the lane's own vector index as a 32-bit offset: one `global_load … v_off, s[base:base+1]` per access with ONE offset VGPR shared by every column,
// where `p + i` with a 64-bit per-lane index costs an address pair per column (the per-element ARG kernel streams 4 + 5·NM columns: 16 VGPRs per mode).
template <typename FT, int VEC, bool NT = true>
__device__ __forceinline__ void load_col_wg(const FT *__restrict__ wg, uint32_t lane, FT (&x)[VEC]) {
    using V = typename VecT<FT, VEC>::type;
    const char *a = reinterpret_cast<const char *>(wg) + (uint32_t)(lane * (uint32_t)sizeof(V));
    V v;
    if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const V *>(a));
    else v = *reinterpret_cast<const V *>(a);
    const FT *e = reinterpret_cast<const FT *>(&v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) x[k] = e[k];
}
template <typename FT, int VEC, bool NT = true>
__device__ __forceinline__ void store_col_wg(FT *__restrict__ wg, uint32_t lane, const FT (&x)[VEC]) {
    using V = typename VecT<FT, VEC>::type;
    char *a = reinterpret_cast<char *>(wg) + (uint32_t)(lane * (uint32_t)sizeof(V));
    V v;
    FT *e = reinterpret_cast<FT *>(&v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) e[k] = x[k];
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<V *>(a));
    else *reinterpret_cast<V *>(a) = v;
}

// --- division of a 32-bit index by a run-time constant (Granlund & Montgomery 1994; Hacker's Delight §10-9) ---------------------
// The layout and column kernels turn a flat element index into (run, offset) or (column, level).  As a 64-bit quotient through
// doubles that is ≈ 40 VALU instructions per lane (conversions, a Float64 multiply, a 64-bit multiply-subtract, two fix-ups) — in the
// Float32 kernels, which are VALU-bound, 3–8 % of the lane's work (round 4: PMC counts).  For indices below 2³² (every launch up
// to 4.29e9 elements; the kernels keep the 64-bit path for larger ones) the quotient is exact with one v_mul_hi_u32:
//     t = mulhi(n, magic);   q = (t + ((n − t) >> sh1)) >> sh2;      magic = ⌊2³²(2^s − d)/d⌋ + 1,  s = ⌈log2 d⌉, sh1 = min(s, 1), sh2 = max(s − 1, 0)
struct FastDivU32 { uint32_t magic, sh1, sh2, d; };
inline FastDivU32 make_fastdiv(uint32_t d) {          // d ≥ 1
    uint32_t s = 0;
    while (s < 32 && ((uint64_t)1 << s) < d) ++s;      // s = ⌈log2 d⌉
    FastDivU32 f;
    f.magic = (uint32_t)((((uint64_t)1 << 32) * ((((uint64_t)1) << s) - d)) / d + 1);
    f.sh1 = s < 1 ? s : 1;
    f.sh2 = s > 0 ? s - 1 : 0;
    f.d = d;
    return f;
}
__host__ __device__ __forceinline__ uint32_t fastdiv(uint32_t n, const FastDivU32 &f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = __umulhi(n, f.magic);
#else
    const uint32_t t = (uint32_t)(((uint64_t)n * f.magic) >> 32);
#endif
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// Byte offset of the LAST parameter of a kernel inside its kernel-argument segment, derived from the kernel's own signature (the
// one-launch 2M + P3 kernel found its EXTRA argument with offsetof() on a hand-copied mirror struct that nothing tied to the parameter list).
// The AMDGPU kernarg ABI lays explicit arguments out in declaration order, each at the next multiple of its ABI alignment — the same rule as a
// C struct of those members — so the fold below follows a reordered, added or removed parameter by itself; `Last` must be the type the caller
// expects there, or it does not compile.
template <typename Last, typename F> struct kernarg_last;
template <typename Last, typename... A> struct kernarg_last<Last, void (*)(A...)> {
    static_assert(sizeof...(A) > 0, "a kernel without parameters has no last argument");
    static_assert(std::is_same_v<std::remove_cv_t<std::tuple_element_t<sizeof...(A) - 1, std::tuple<A...>>>, std::remove_cv_t<Last>>,
                  "the kernel's last parameter is not the type read through the kernel-argument segment");
    static constexpr size_t offset() {
        constexpr size_t sz[] = {sizeof(A)...}, al[] = {alignof(A)...};
        size_t off = 0;
        for (size_t i = 0; i < sizeof...(A); ++i) {
            off = (off + al[i] - 1) / al[i] * al[i];
            if (i + 1 < sizeof...(A)) off += sz[i];
        }
        return off;
    }
};
// use: kernarg_offset_of_last<EXTRA, decltype(&kernel<...>)>() — the kernel is named in an unevaluated operand only
template <typename Last, typename F> constexpr size_t kernarg_offset_of_last() { return kernarg_last<Last, F>::offset(); }

}  // namespace cmx
