// cmx_parcel_kernels.hip — the adiabatic parcel model over an ensemble of parcels for gfx950; C-ABI entry points cmx_parcel_tendencies_* and
// cmx_parcel_run_* (include/cmx.h §(13)).  The point functions are in cmx_parcel.hpp.
//
// One parcel per lane in both kernels.  The tendencies kernel is a pointwise map (10 columns in, up to 15 out); the run kernel keeps the nine state
// values, w and the six coefficients of its parcel in registers and executes the forward-Euler recurrence inside the kernel: nothing is re-read from
// memory between steps, and a step is several hundred VALU instructions, so the kernel is bound by VALU issue, not by HBM — which is why it does not
// use the 16-byte vector path and its alignment split (cmx_split.hpp): with one 4- or 8-byte value per lane and column the accesses are coalesced at
// any alignment, and the result cannot depend on it.  Options are wave-uniform branches on the flags word (a kernel argument, i.e. an SGPR).  The
// constants come from the kernel-argument segment (front_consts); Float64 evaluates its functions from the LDS tables that prepare() fills.
// Trajectory records are written with non-temporal stores, layout [record][variable][parcel]: every store instruction of a wave is one contiguous run.
#include <hip/hip_runtime.h>

#include "../../include/cmx.h"
#include "cmx_launch.hpp"
#include "cmx_math.hpp"
#include "cmx_parcel.hpp"

namespace cmx {

template <typename FT> struct ParcelIn {
    const FT *Y[CMX_PARCEL_NSTATE];
    const FT *w;
    const FT *coef[CMX_PARCEL_NCOEF];      // NULL: the struct's value (ParcelConsts::coef)
};
template <typename FT> struct ParcelTendOut {
    FT *dY[CMX_PARCEL_NSTATE];
    FT *proc[CMX_PARCEL_NPROC];
};
template <typename FT> struct ParcelRunOut {
    FT *Y[CMX_PARCEL_NSTATE];
    FT *traj;                              // NULL: no trajectory
};

// loads the parcel of lane i; returns "one of its inputs is a NaN"
template <typename FT, typename C>
__device__ __forceinline__ bool parcel_load(const C &c, const ParcelIn<FT> &in, const int64_t i, FT (&Y)[CMX_PARCEL_NSTATE], FT &w, FT (&k)[CMX_PARCEL_NCOEF]) {
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) Y[j] = __builtin_nontemporal_load(in.Y[j] + i);
    w = __builtin_nontemporal_load(in.w + i);
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NCOEF; ++j) k[j] = in.coef[j] ? __builtin_nontemporal_load(in.coef[j] + i) : c.coef[j];      // wave-uniform
    return parcel_inputs_nan<FT>(Y, w, k);
}

template <typename FT>
__global__ __launch_bounds__(kBlock) void parcel_tendencies_kernel(const ParcelConsts<FT> c_in, const ParcelIn<FT> in, const ParcelTendOut<FT> out,
                                                                   const uint32_t flags, const int64_t n) {
    const auto &c = front_consts<FT, true>(c_in);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (sizeof(FT) == 8) lean::erfc_tab_fill();   // published by the barrier inside prepare()
    Math<FT>::prepare();                                    // Float64: exp2 / log2 tables → LDS (every lane of the workgroup reaches the barrier inside); no-op for Float32
    if (i >= n) return;
    FT Y[CMX_PARCEL_NSTATE], w, k[CMX_PARCEL_NCOEF], dY[CMX_PARCEL_NSTATE], proc[CMX_PARCEL_NPROC];
    const bool bad = parcel_load<FT>(c, in, i, Y, w, k);
    parcel_rhs<FT>(c, flags, Y, w, k, dY, proc);
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j)
        if (out.dY[j]) __builtin_nontemporal_store(bad ? Math<FT>::nan() : dY[j], out.dY[j] + i);
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NPROC; ++j)
        if (out.proc[j]) __builtin_nontemporal_store(bad ? Math<FT>::nan() : proc[j], out.proc[j] + i);
}

// Steps step0 + 1 … step0 + n_steps of the integration (step0 = the steps earlier launches of the same call have done).  Record r of the trajectory
// is the state after r·save_every steps; `until_save` counts down to the next one, a scalar.
template <typename FT> __device__ __forceinline__ void parcel_store_record(FT *traj, int64_t record, int64_t n, int64_t i, const FT (&Y)[CMX_PARCEL_NSTATE]) {
    FT *rec = traj + record * CMX_PARCEL_NSTATE * n + i;
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) __builtin_nontemporal_store(Y[j], rec + (int64_t)j * n);
}

template <typename FT>
__global__ __launch_bounds__(kBlock) void parcel_run_kernel(const ParcelConsts<FT> c_in, const ParcelIn<FT> in, const ParcelRunOut<FT> out,
                                                            const uint32_t flags, const int64_t n, const int32_t n_steps, const int64_t step0,
                                                            const int32_t save_every) {
    const auto &c = front_consts<FT, true>(c_in);
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (sizeof(FT) == 8) lean::erfc_tab_fill();
    Math<FT>::prepare();
    if (i >= n) return;
    FT Y[CMX_PARCEL_NSTATE], w, k[CMX_PARCEL_NCOEF];
    const bool bad = parcel_load<FT>(c, in, i, Y, w, k);
    if (bad) {      // the whole parcel is NaN from here on: every later value is computed from these nine
#pragma unroll
        for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) Y[j] = Math<FT>::nan();
    }
    const bool save = out.traj && save_every > 0;           // wave-uniform
    if (save && step0 == 0) parcel_store_record<FT>(out.traj, 0, n, i, Y);
    int64_t record = save ? step0 / save_every : 0;
    int32_t until_save = save ? save_every - (int32_t)(step0 % save_every) : 0;
    for (int32_t s = 0; s < n_steps; ++s) {
        parcel_step<FT>(c, flags, Y, w, k);
        if (save && --until_save == 0) {
            until_save = save_every;
            parcel_store_record<FT>(out.traj, ++record, n, i, Y);
        }
    }
#pragma unroll
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) __builtin_nontemporal_store(Y[j], out.Y[j] + i);
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The coefficient columns of a scheme that is off are dropped here, so that the kernel neither loads them nor lets a NaN in them poison a parcel.
template <typename FT> static bool parcel_fill_inputs(ParcelIn<FT> &in, uint32_t flags, const FT *const *state, const FT *w, const FT *const *coef) {
    if (!state || !w) return false;
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) {
        if (!state[j]) return false;
        in.Y[j] = state[j];
    }
    in.w = w;
    const bool on[3] = {(flags & CMX_PARCEL_DEP_MASK) == CMX_PARCEL_DEP_ABDINM, (flags & CMX_PARCEL_HET_MASK) == CMX_PARCEL_HET_ABIFM,
                        (flags & CMX_PARCEL_HOM_MASK) == CMX_PARCEL_HOM_ABHOM};
    for (int j = 0; j < CMX_PARCEL_NCOEF; ++j) in.coef[j] = (coef && on[j / 2]) ? coef[j] : nullptr;
    return true;
}

template <typename FT, typename PP> static int32_t parcel_common_checks(const PP *pp, uint32_t flags, int64_t n) {
    if (!pp) return CMX_ERR_BAD_ARG;
    if (const int32_t st = parcel_flags_status(flags)) return st;
    CMX_TRY_COUNT_LIMIT(n);
    return CMX_OK;
}

template <typename FT, typename PP>
static int32_t parcel_tendencies_entry(const PP *pp, uint32_t flags, int64_t n, const FT *const *state, const FT *w, const FT *const *coef,
                                       FT *const *tend, FT *const *proc, void *stream) {
    if (const int32_t st = parcel_common_checks<FT>(pp, flags, n)) return st;
    if (n == 0) return CMX_OK;
    ParcelIn<FT> in{};
    ParcelTendOut<FT> out{};
    if (!parcel_fill_inputs<FT>(in, flags, state, w, coef)) return CMX_ERR_BAD_ARG;
    bool any = false;
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) any |= (out.dY[j] = tend ? tend[j] : nullptr) != nullptr;
    for (int j = 0; j < CMX_PARCEL_NPROC; ++j) any |= (out.proc[j] = proc ? proc[j] : nullptr) != nullptr;
    if (!any) return CMX_ERR_BAD_ARG;
    const ParcelConsts<FT> c = make_parcel_consts<FT>(*pp, flags);
    launch<kBlock>(parcel_tendencies_kernel<FT>, n, reinterpret_cast<hipStream_t>(stream), c, in, out, flags, n);
    return launched();
}

template <typename FT, typename PP>
static int32_t parcel_run_entry(const PP *pp, uint32_t flags, int64_t n, int64_t n_steps, int64_t save_every, const FT *const *state, const FT *w,
                                const FT *const *coef, FT *const *state_out, FT *traj, void *stream) {
    if (const int32_t st = parcel_common_checks<FT>(pp, flags, n)) return st;
    if (n_steps < 0 || save_every < 0 || save_every > 0x7fffffffll) return CMX_ERR_BAD_ARG;
    if (n == 0) return CMX_OK;
    ParcelIn<FT> in{};
    ParcelRunOut<FT> out{};
    if (!parcel_fill_inputs<FT>(in, flags, state, w, coef) || !state_out) return CMX_ERR_BAD_ARG;
    for (int j = 0; j < CMX_PARCEL_NSTATE; ++j)
        if (!(out.Y[j] = state_out[j])) return CMX_ERR_BAD_ARG;
    out.traj = save_every > 0 ? traj : nullptr;
    const ParcelConsts<FT> c = make_parcel_consts<FT>(*pp, flags);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // launches of at most kParcelMaxStepsPerLaunch steps (cmx_launch.hpp); the second and later ones continue from state_out.  n_steps = 0 still
    // runs one launch: it copies the state and writes record 0.
    int64_t done = 0;
    do {
        const int64_t left = n_steps - done;
        const int32_t now = (int32_t)(left < kParcelMaxStepsPerLaunch ? left : kParcelMaxStepsPerLaunch);
        launch<kBlock>(parcel_run_kernel<FT>, n, s, c, in, out, flags, n, now, done, (int32_t)save_every);
        done += now;
        for (int j = 0; j < CMX_PARCEL_NSTATE; ++j) in.Y[j] = out.Y[j];
    } while (done < n_steps);
    return launched();
}

}  // namespace cmx

extern "C" {
int32_t cmx_parcel_tendencies_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n_parcels, const float *const *state, const float *w,
                                  const float *const *coefficients, float *const *tendencies, float *const *process_rates, void *stream) {
    return cmx::parcel_tendencies_entry<float>(pp, flags, n_parcels, state, w, coefficients, tendencies, process_rates, stream);
}
int32_t cmx_parcel_tendencies_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n_parcels, const double *const *state, const double *w,
                                  const double *const *coefficients, double *const *tendencies, double *const *process_rates, void *stream) {
    return cmx::parcel_tendencies_entry<double>(pp, flags, n_parcels, state, w, coefficients, tendencies, process_rates, stream);
}
int32_t cmx_parcel_run_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n_parcels, int64_t n_steps, int64_t save_every,
                           const float *const *state, const float *w, const float *const *coefficients, float *const *state_out, float *trajectory,
                           void *stream) {
    return cmx::parcel_run_entry<float>(pp, flags, n_parcels, n_steps, save_every, state, w, coefficients, state_out, trajectory, stream);
}
int32_t cmx_parcel_run_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n_parcels, int64_t n_steps, int64_t save_every,
                           const double *const *state, const double *w, const double *const *coefficients, double *const *state_out, double *trajectory,
                           void *stream) {
    return cmx::parcel_run_entry<double>(pp, flags, n_parcels, n_steps, save_every, state, w, coefficients, state_out, trajectory, stream);
}
}
