// cmx_ensemble.hpp — what the parameter-ensemble entries (include/cmx.h §(29)) share: the descriptor checks, the per-member alignment split and the
// kernel-side view of the constants table.
//
// Kernel shape.  The grid is two-dimensional: blockIdx.y is the member, blockIdx.x tiles that member's points, no workgroup spans two members.  Member
// e's constants are one block of a table in device memory, read through a constant-address-space reference
//     *(KernArg<Block> *)(table + blockIdx.y · stride)
// whose address is a kernel argument plus a blockIdx expression — provably wave-uniform, so the loads are scalar loads (s_load through the scalar
// data cache: E blocks of 0.4–1.7 KiB, shared by every workgroup of a member) and consts_after (cmx_math.hpp) works on it exactly as on the
// kernel-argument pointer of the single entries.  The arithmetic is the single kernels' own text (the *_body.inc files): same operations, same operands,
// same bits.
//
// Alignment.  Member e's columns start e·n points after member 0's, so unless n is a multiple of the vector width every member has its own
// misalignment.  The split of cmx_split.hpp is applied PER MEMBER inside the kernel: the entry launches up to three parts — scalar heads (one
// workgroup per member), vector bodies, scalar tails — and each workgroup derives its member's range of that part from (mis0 + e·n) mod vec.  When the
// columns of a call do not share one offset modulo 16 bytes (or, with a shared state, when n is not a multiple of the vector width: the inputs then
// keep their offset from member to member while the outputs move), everything runs one point per lane (ENS_ALL).  Every instantiation computes the
// identical instruction sequence per point, so the choice does not change any result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cmx_launch.hpp"
#include "cmx_math.hpp"

namespace cmx {

constexpr int32_t kEnsMaxMembers = 65535;      // gridDim.y

enum : int32_t { ENS_ALL = 0, ENS_HEAD = 1, ENS_BODY = 2, ENS_TAIL = 3 };

// first kernel argument of every ensemble kernel
struct EnsArgs {
    const unsigned char *table;   // device: n_members blocks, `stride` bytes apart
    int64_t in_stride;            // points from one member's input columns to the next: n (member-major) or 0 (shared state)
    uint32_t stride;
    uint32_t vec;                 // points per lane of the vector body (a power of two)
    uint32_t mis0;                // offset of member 0's columns from a vector boundary, in points
    int32_t part;                 // ENS_*
};

// the range [lo, lo + count) of `part` inside member e's n points
__host__ __device__ inline void ens_member_range(int32_t part, uint32_t vec, uint32_t mis0, int64_t n, uint32_t e, int64_t &lo, int64_t &count) {
    if (part == ENS_ALL) { lo = 0; count = n; return; }
    const uint32_t mis = (uint32_t)(((uint64_t)mis0 + (uint64_t)e * (uint64_t)n) & (uint64_t)(vec - 1));
    int64_t head = mis ? (int64_t)(vec - mis) : 0;
    if (head > n) head = n;
    const int64_t body = (n - head) / vec * vec;
    if (part == ENS_HEAD) { lo = 0; count = head; }
    else if (part == ENS_BODY) { lo = head; count = body; }
    else { lo = head + body; count = n - head - body; }
}

// member e's block of the table
template <typename BLOCK> __device__ __forceinline__ KernArg<BLOCK> &ens_block(const EnsArgs &ea, uint32_t e) {
    return *(KernArg<BLOCK> *)(ea.table + (uint64_t)e * ea.stride);
}

// The constants an included kernel body reads where the single kernel says front_consts<FT, ALSO>(c) (cmx_math.hpp), with the same rule: Float64, or ALSO,
// reads the table through the constant-address-space reference, phase by phase; otherwise the body gets a by-value copy of the member's constants, loaded
// once with scalar loads and held in SGPRs — what the by-value kernel argument of the single kernel is.
template <typename T> __device__ __forceinline__ T ens_load(KernArg<T> &src) {
    T dst;
    __builtin_memcpy(&dst, &src, sizeof(T));
    return dst;
}
template <typename FT, bool ALSO, typename T> __device__ __forceinline__ decltype(auto) ens_consts(KernArg<T> &tab, const T &local) {
    if constexpr (sizeof(FT) == 8 || ALSO) return (tab);
    else return (local);
}

// The constants of a scheme's eval (cmx_jacobian.hpp: S::eval reads them through scheme_consts → front_consts) in an ensemble kernel: a tag in place of the
// constants, and the overload of front_consts that forms the reference to member blockIdx.y's block — OFFSET bytes into it — WHERE THE EVAL READS IT, from
// the EnsArgs at the front of the kernel-argument segment.  That is the single kernels' form (a fresh kernel-argument pointer per eval).  One reference
// formed at the top of the kernel and handed down to every eval compiles to the same loads but moved 14–22 Float64 values into spill registers in the
// implicit column step (428 → 456, 408 → 452, 498 → 512 VGPRs + 20 spilled, HISTORY.md): the Float64 instantiations there have no register to spare.
template <typename CT, uint32_t OFFSET> struct EnsFrontConsts {};
template <typename FT, bool ALSO = false, typename CT, uint32_t OFFSET> __device__ __forceinline__ KernArg<CT> &front_consts(const EnsFrontConsts<CT, OFFSET> &) {
    KernArg<EnsArgs> &ea = *(KernArg<EnsArgs> *)__builtin_amdgcn_kernarg_segment_ptr();
    return *(KernArg<CT> *)(ea.table + ((uint64_t)blockIdx.y * ea.stride + OFFSET));
}

template <typename BLOCK> constexpr int32_t ens_stride() { return (int32_t)((sizeof(BLOCK) + 15) / 16 * 16); }

// The ensemble arguments of an entry, checked after its counts (include/cmx.h §(29) for the order): 0, or the status to return.
inline int32_t ens_check(const cmx_ensemble_desc *desc, int32_t n_members, uint32_t ens_flags, uint32_t scheme, uint32_t float_type, uint32_t stride) {
    if (desc->magic != CMX_ENSEMBLE_MAGIC || desc->scheme != scheme || desc->float_type != float_type) return CMX_ERR_BAD_ARG;
    if (n_members < 1 || n_members != desc->n_members || desc->stride != stride) return CMX_ERR_BAD_ARG;
    if (ens_flags & ~(uint32_t)CMX_ENSEMBLE_SHARED_STATE) return CMX_ERR_BAD_ARG;
    if (n_members > kEnsMaxMembers) return CMX_ERR_UNSUPPORTED;
    return CMX_OK;
}

// How the n points of every member are split into launches.
struct EnsPlan { bool vector; uint32_t mis0; bool any_head, any_tail; };

// in / out: the call's columns (NULL: an absent optional one).  Inputs move in_stride points from member to member, outputs n.
template <typename FT, int VEC>
inline EnsPlan ens_plan(const void *const *in, int n_in, const void *const *out, int n_out, int64_t n, int64_t in_stride, int32_t n_members) {
    EnsPlan p{false, 0, false, false};
    if (VEC == 1) return p;
    const uintptr_t A = (uintptr_t)VEC * sizeof(FT);
    bool have = false;
    uintptr_t mis = 0;
    for (int k = 0; k < n_in + n_out; ++k) {
        const void *c = k < n_in ? in[k] : out[k - n_in];
        if (!c) continue;
        const uintptr_t m = reinterpret_cast<uintptr_t>(c) % A;
        if (have ? m != mis : m % sizeof(FT) != 0) return p;
        mis = m;
        have = true;
    }
    if (n_members > 1 && (in_stride - n) % VEC != 0) return p;      // inputs and outputs drift apart from member to member
    p.vector = true;
    p.mis0 = (uint32_t)(mis / sizeof(FT));
    for (int32_t e = 0; e < n_members && e < VEC; ++e) {             // (mis0 + e·n) mod VEC has period ≤ VEC in e
        int64_t lo, count;
        ens_member_range(ENS_HEAD, VEC, p.mis0, n, (uint32_t)e, lo, count);
        p.any_head |= count > 0;
        ens_member_range(ENS_TAIL, VEC, p.mis0, n, (uint32_t)e, lo, count);
        p.any_tail |= count > 0;
    }
    return p;
}

// Calls f(std::integral_constant<int, V>{}, part, nvec_max) for every launch of the plan: V points per lane, nvec_max = the largest number of lanes a
// member can have in that part (what sizes grid.x; a member with fewer leaves its last workgroups idle).
template <int VEC, typename F> inline void ens_for_each_part(const EnsPlan &p, int64_t n, F &&f) {
    if (!p.vector) { f(std::integral_constant<int, 1>{}, (int32_t)ENS_ALL, n); return; }
    if (p.any_head) f(std::integral_constant<int, 1>{}, (int32_t)ENS_HEAD, (int64_t)(VEC - 1));
    if (n / VEC > 0) f(std::integral_constant<int, VEC>{}, (int32_t)ENS_BODY, n / VEC);
    if (p.any_tail) f(std::integral_constant<int, 1>{}, (int32_t)ENS_TAIL, (int64_t)(VEC - 1));
}

}  // namespace cmx
