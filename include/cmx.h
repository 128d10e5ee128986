/*
 * cmx.h — C ABI of the MI355X-native cloud-microphysics rate evaluator.
 *
 * This is the drop-in boundary.  The reference package
 * (CliMA/CloudMicrophysics.jl v0.38.1) has no FFI of its own: "array
 * evaluation" there is a Julia broadcast / KernelAbstractions kernel of the
 * form `output[i] = f(params, x[i]...)` over equal-length columns
 * (test/gpu_performance.jl:49-57, test/gpu_tests.jl:220-244,407-415,
 * test/type_stability_tests.jl:131-137).  Each entry point below replaces ONE
 * such broadcast with one fused HIP kernel for gfx950; the reference call it
 * replaces is cited next to it.  INTEGRATION.md shows the Julia `ccall`
 * binding a maintainer would add.
 *
 * Conventions
 *  - all array pointers are DEVICE pointers (HBM), structure-of-arrays, one
 *    column per state variable, `n` elements each, no aliasing between inputs
 *    and outputs; 16-byte alignment enables the 128-bit load/store path, any
 *    alignment is accepted;
 *  - parameter structs are plain host structs, passed by pointer, copied into
 *    the kernel argument segment (they end up in SGPRs: wave-uniform);
 *    field order == declaration order of the reference's immutable Julia
 *    structs (src/parameters/Microphysics2M.jl etc.) so an all-FT isbits
 *    Julia struct can be passed with `Ref(x)`;
 *  - `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream);
 *    calls are asynchronous on that stream and never synchronise;
 *  - return value: 0 = ok, < 0 = error (cmx_status), the library never
 *    throws, never takes ownership of a pointer and keeps no device memory;
 *  - negative ρ, q and n inputs are clamped to 0 like UT.clamp_to_nonneg in the reference's entries (T is not clamped); a NaN in any
 *    input of a point gives NaN in every output of that point.  The air density must be positive: ρ ≤ 0 is outside the domain.  Such a
 *    point never yields a valid-looking result — the Float32 kernels reproduce the reference's own NaN / ±Inf pattern, the Float64 kernels
 *    return a non-finite value wherever the reference does and may return NaN for an output the reference still evaluates (their
 *    finite-argument elementary functions assume ρ > 0; the Float64 1-moment entries return NaN in EVERY output of such a point;
 *    tests/test_nan_inputs_gpu.py::test_zero_and_negative_air_density);
 *  - parameter domain of the SB2006 rain fall speed (CMX_VEL_SB2006): with the NOT-limited rain PSD the speeds integrate from the radius
 *    r_c = −log(aR/bR)/(2 cR), which exists only for aR < bR.  With aR ≥ bR that radius is zero or negative, the truncation means nothing, and the reference's
 *    Float64 result is NaN where q_rai → 0 at large N_rai (exp(−2 r_c λ_r) overflows: Inf − Inf; src/Microphysics2M.jl:685-739); the entries that evaluate this fall speed
 *    (cmx_sb2006_warm_rain_tendencies_*, cmx_sb2006_process_rates_*, cmx_sb2006_column_tendencies_sedimentation_*) return CMX_ERR_BAD_ARG for
 *    such a struct and launch nothing.  The limited PSD (CMX_SB2006_LIMITED) takes any aR, bR;
 *    tests/test_param_sweep_gpu.py::test_sb2006_fall_speed_needs_aR_below_bR;
 *  - `_f32` entry points compute in float with the reference's Float32
 *    thresholds (eps(Float32), cbrt(floatmin(Float32)) — src/Utilities.jl:318-340),
 *    `_f64` ones in double with the Float64 thresholds.
 *
 * What this boundary deliberately does NOT have (SURVEY.md §8b proposed them; the decision is recorded here so
 * the header is the whole contract):
 *  - no `cmx_ctx` / `cmx_context_create`: the library is STATELESS.  The device is the calling thread's current HIP
 *    device, the stream is an argument, parameters are copied into the kernel arguments per call, nothing is
 *    cached between calls (the only process-wide state is a per-device properties cache filled once under
 *    std::call_once).  Every entry is therefore re-entrant, capturable into a HIP graph, and safe to call
 *    concurrently from several host threads on several streams or devices;
 *  - no `cmx_*_host` entry points taking host pointers: a host-pointer variant could only be a copy-in / copy-out
 *    wrapper (PCIe 63 GB/s against 52 B/point: ≈ 90× below the HBM-resident rate) or a CPU
 *    implementation, and a CPU path inside the product is ruled out (the CPU restatement lives in oracle/ as
 *    test infrastructure only).  A caller with host data does hipMemcpyAsync on its own stream;
 *  - no `cmx_multi_*` device-list entry points: the multi-GPU model is one PROCESS per GPU (torch.distributed /
 *    RCCL, cmx/sharding.py); each rank calls the single-device entries on its contiguous shard of every column
 *    and there is no data-path collective to hide behind an API.
 */
#ifndef CMX_H
#define CMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* cmx_version() = (MAJOR << 16) | MINOR.  The minor number moves whenever a parameter struct changes its layout or an entry point is added, so a
 * binding compiled against another header can refuse to run:
 *   0.1  rounds 1–2
 *   0.3  round 3: cmx_process_params_1m gained the Frostenberg member (cmx_microphysics_1m: 85 → 90 fields); new structs cmx_mohler2006,
 *        cmx_mohler_dust, cmx_deposition_dust, cmx_h2so4_solution_params; new entries cmx_mp1m_column_tendencies_sedimentation,
 *        cmx_mp1m_linearized_average_fields, cmx_microphysics_2m_p3_tendencies_fields, cmx_ice_nucleation_rates_xT, cmx_h2so4_solution,
 *        cmx_mohler2006_deposition, cmx_deposition_J, cmx_inp_concentration_frequency, cmx_arg2000_total_activated, cmx_lean_eval_literal;
 *        process columns CMX_SB_DEVAP_DN_RAI / CMX_SB_DEVAP_DQ_RAI; CMX_1M_CLOUD_ICE_FORMATION_TDEP and every Chen-2022 table accepted
 *   0.4  round 4: no struct layout changed.  New entries cmx_gamma_inc, cmx_gamma_inc_inv (UT.gamma_inc / gamma_inc_inv over columns),
 *        cmx_generalized_gamma, cmx_exponential_distribution, cmx_sb2006_size_distribution (DistributionTools and the SB2006 PSD accessors); cmx_column_sums_* takes a caller-owned workspace and is deterministic (one launch
 *        for all columns + a one-workgroup-per-column finish, no floating-point atomics).
 *   0.5  round 5: no struct layout changed.  New entry cmx_cloud_diagnostics (CloudDiagnostics over columns); cmx_sb2006_size_distribution refuses the
 *        limited variant of a struct without limiters (CMX_ERR_BAD_ARG instead of silently clamping to 0).
 *        Later, without a new number (no struct layout changed; entries only added — an older library fails on the symbol lookup):
 *        cmx_snow_terminal_velocity (the snow fall speed with CM1.Oblate / CM1.Prolate) and the CMX_1M_SED_SNOW_* bits of the column step.
 *        cmx_aerosol_nucleation_rates, cmx_nucleation_rates_prescribed, cmx_apparent_nucleation_rate (Nucleation.jl) with the new structs cmx_h2so4_nucleation /
 *        cmx_organic_nucleation / cmx_mixed_nucleation, and cmx_p3_ice_nucleation_counts (CMI_het.P3_deposition_N_i / P3_het_N_i).
 *        cmx_mp2m_p3_column_tendencies_sedimentation (the 2M + P3 column step, (9b)) with the flag bits CMX_P3COL_VEL_*.
 *        julia/CMXExt.jl (the reference-side binding) checks this number. */
#define CMX_VERSION_MAJOR 0
#define CMX_VERSION_MINOR 5

typedef enum cmx_status {
    CMX_OK = 0,
    CMX_ERR_BAD_ARG = -1,     /* null pointer, n < 0, unknown flag combination */
    CMX_ERR_HIP = -2,         /* a HIP runtime call failed: see cmx_last_hip_error() */
    CMX_ERR_UNSUPPORTED = -3  /* valid request this build has no kernel for */
} cmx_status;

/* ---- domain of the Chen-2022 RAIN fall speeds (every entry that takes a cmx_chen2022_rain_vel_* table: cmx_sb2006_warm_rain_tendencies_*,
 * cmx_sb2006_process_rates_*, cmx_sb2006_column_tendencies_sedimentation_* with CMX_VEL_CHEN2022; cmx_mp1m_terminal_velocity_*,
 * cmx_sedimentation_velocities_*, cmx_mp1m_column_tendencies_sedimentation_*; the vel_rain member of cmx_p3_ice_params_*) ---------------
 * The table's exponents depend on the state only through the air density, b_i(ρ) = b_i − b_ρ ρ (src/Common.jl:290-302), and the reference
 * evaluates Γ(b_i(ρ) + 1) with SpecialFunctions at any ρ.  The library fits those Γ per parameter set on 0 ≤ ρ ≤ 2 kg/m³ (csrc/cmx_math.hpp
 * make_chen_gamma; the fit is checked against tgamma on the host and a table it cannot represent takes a general-Γ instantiation, valid
 * for every ρ).  With a fitted table, a point with ρ > 2 kg/m³ gets NaN rain fall speeds — and, in the column entries, NaN sedimentation
 * tendencies of that cell and the cell below — rather than an extrapolated value.  ρ ≤ 2 kg/m³ covers every terrestrial state
 * (ρ = 1.4 kg/m³ at 1050 hPa and 260 K); callers with denser gases must not use the Chen-2022 rain table.  The SB2006 fall speeds
 * (CMX_VEL_SB2006) and the Chen-2022 ICE tables have no such restriction. */

/* ---- flags for the SB2006 entry points ------------------------------------ */
/* rain PSD with the SB2006 Eq. 94-97 limiters (RainParticlePDF_SB2006_limited,
 * src/parameters/Microphysics2M.jl:314-335) vs. without (…_notlimited, :362-375) */
#define CMX_SB2006_LIMITED      (1u << 0)
/* rain terminal-velocity scheme for the two optional velocity columns */
#define CMX_VEL_SB2006          (1u << 1)  /* CM2.rain_terminal_velocity(::SB2006VelType)  src/Microphysics2M.jl:685-702 */
#define CMX_VEL_CHEN2022        (1u << 2)  /* CM2.rain_terminal_velocity(::Chen2022VelTypeRain) :703-719 */

/* ---------------------------------------------------------------------------
 * Parameter structs.  One macro stamps the Float32 and the Float64 family.
 * Field names are ASCII transliterations of the Julia field names
 * (νc → nu_c, ρw → rho_w, λ_min → lambda_min, κrr → kappa_rr, τ → tau …).
 * ------------------------------------------------------------------------- */
#define CMX_DECLARE_PARAM_STRUCTS(FT, SFX)                                                     \
    /* CloudParticlePDF_SB2006 — src/parameters/Microphysics2M.jl:401-416 */                   \
    typedef struct cmx_cloud_pdf_sb2006_##SFX {                                                \
        FT nu_c, mu_c, xc_min, xc_max, rho_w, loggamma_z1, loggamma_z2;                        \
    } cmx_cloud_pdf_sb2006_##SFX;                                                              \
    /* RainParticlePDF_SB2006_limited — :314-335 (the not-limited variant, :362-375, uses   */ \
    /* nu_r, mu_r, xr_min, xr_max, rho_w, rho_0 only; its N0/lambda fields are ignored)      */ \
    typedef struct cmx_rain_pdf_sb2006_##SFX {                                                 \
        FT nu_r, mu_r, xr_min, xr_max, N0_min, N0_max, lambda_min, lambda_max, rho_w, rho_0;   \
    } cmx_rain_pdf_sb2006_##SFX;                                                               \
    /* AcnvSB2006 — :443-456 */                                                                \
    typedef struct cmx_acnv_sb2006_##SFX { FT kcc, x_star, rho_0, A, a, b; }                   \
        cmx_acnv_sb2006_##SFX;                                                                 \
    /* AccrSB2006 — :480-489 */                                                                \
    typedef struct cmx_accr_sb2006_##SFX { FT kcr, tau_0, rho_0, c; } cmx_accr_sb2006_##SFX;   \
    /* SelfColSB2006 — :510-517 */                                                             \
    typedef struct cmx_selfcol_sb2006_##SFX { FT krr, kappa_rr, d; } cmx_selfcol_sb2006_##SFX; \
    /* BreakupSB2006 — :537-546 */                                                             \
    typedef struct cmx_breakup_sb2006_##SFX { FT Deq, Dr_th, kbr, kappa_br; }                  \
        cmx_breakup_sb2006_##SFX;                                                              \
    /* EvaporationSB2006 — :567-588; the last five are host-derived (:599-606) */              \
    typedef struct cmx_evap_sb2006_##SFX {                                                     \
        FT av, bv, alpha, beta, rho_0, a_vent_1, b_vent_1, a_vent_0_coeff, b_vent_0_coeff,     \
            beta_vent_0;                                                                       \
    } cmx_evap_sb2006_##SFX;                                                                   \
    /* NumberAdjustmentHorn2012 — :617-620 */                                                  \
    typedef struct cmx_numadj_horn2012_##SFX { FT tau; } cmx_numadj_horn2012_##SFX;            \
    /* SB2006 — :642-659 */                                                                    \
    typedef struct cmx_sb2006_##SFX {                                                          \
        cmx_cloud_pdf_sb2006_##SFX pdf_c;                                                      \
        cmx_rain_pdf_sb2006_##SFX pdf_r;                                                       \
        cmx_acnv_sb2006_##SFX acnv;                                                            \
        cmx_accr_sb2006_##SFX accr;                                                            \
        cmx_selfcol_sb2006_##SFX self;                                                         \
        cmx_breakup_sb2006_##SFX brek;                                                         \
        cmx_evap_sb2006_##SFX evap;                                                            \
        cmx_numadj_horn2012_##SFX numadj;                                                      \
    } cmx_sb2006_##SFX;                                                                        \
    /* AirProperties — src/parameters/AirProperties.jl:11-18 */                                \
    typedef struct cmx_air_properties_##SFX { FT K_therm, D_vapor, nu_air; }                   \
        cmx_air_properties_##SFX;                                                              \
    /* WarmRainParams2M — src/parameters/Microphysics2MParams.jl:14-19                      */ \
    /* (seifert_beheng, air_properties, condevap.τ_relax, subdep.τ_relax)                   */ \
    typedef struct cmx_warm_rain_2m_##SFX {                                                    \
        cmx_sb2006_##SFX seifert_beheng;                                                       \
        cmx_air_properties_##SFX air_properties;                                               \
        FT condevap_tau_relax;                                                                 \
        FT subdep_tau_relax;                                                                   \
    } cmx_warm_rain_2m_##SFX;                                                                  \
    /* Thermodynamics.Parameters.ThermodynamicsParameters is NOT the reference's struct   */   \
    /* (un-vendored Thermodynamics.jl); the shim flattens it through the accessors the    */   \
    /* reference itself uses (src/ThermodynamicsInterface.jl:9-25).                        */  \
    typedef struct cmx_thermo_##SFX {                                                          \
        FT R_v, R_d, cp_d, cp_v, cp_l, cp_i, LH_v0, LH_s0, T_0, T_triple, press_triple,        \
            T_freeze, cv_l;                                                                    \
    } cmx_thermo_##SFX;                                                                        \
    /* KK2000 / B1994 / TC1980 / LD2004 bulk two-moment autoconversion and accretion parameter */ \
    /* sets — src/parameters/Microphysics2M.jl:11-75, 89-160, 172-240, 258-279                 */ \
    typedef struct cmx_kk2000_##SFX { FT acnv_A, acnv_a, acnv_b, acnv_c, accr_A, accr_a, accr_b; } cmx_kk2000_##SFX; \
    typedef struct cmx_b1994_##SFX {                                                           \
        FT acnv_C, acnv_a, acnv_b, acnv_c, acnv_N_0, acnv_d_low, acnv_d_high, acnv_k, accr_A;  \
    } cmx_b1994_##SFX;                                                                         \
    typedef struct cmx_tc1980_##SFX {                                                          \
        FT acnv_a, acnv_b, acnv_D, acnv_r_0, acnv_me_liq, acnv_m0_liq_coeff, acnv_k, accr_A;   \
    } cmx_tc1980_##SFX;                                                                        \
    typedef struct cmx_ld2004_##SFX { FT R_6C_0, E_0, rho_w, k; } cmx_ld2004_##SFX;            \
    typedef struct cmx_bulk_2m_schemes_##SFX {                                                 \
        cmx_kk2000_##SFX kk2000; cmx_b1994_##SFX b1994; cmx_tc1980_##SFX tc1980;               \
        cmx_ld2004_##SFX ld2004;                                                               \
    } cmx_bulk_2m_schemes_##SFX;                                                               \
    /* StokesRegimeVelType — src/parameters/TerminalVelocity.jl:150-154 */                     \
    typedef struct cmx_stokes_vel_##SFX { FT rho_w, nu_air, grav; } cmx_stokes_vel_##SFX;      \
    /* SB2006VelType — src/parameters/TerminalVelocity.jl:174-182 */                           \
    typedef struct cmx_sb2006_vel_##SFX { FT rho_0, aR, bR, cR, rho_w, nu_air, grav; }         \
        cmx_sb2006_vel_##SFX;                                                                  \
    /* Chen2022VelTypeRain — src/parameters/TerminalVelocity.jl:288-295 (Table B1) */          \
    typedef struct cmx_chen2022_rain_vel_##SFX {                                               \
        FT rho_0, a[3], a3_pow, b[3], b_rho, c[3];                                             \
    } cmx_chen2022_rain_vel_##SFX;                                                             \
    /* terminal-velocity parameters for the optional velocity columns: which member is    */   \
    /* read is selected by CMX_VEL_SB2006 / CMX_VEL_CHEN2022                              */   \
    typedef struct cmx_rain_vel_##SFX {                                                        \
        cmx_sb2006_vel_##SFX sb2006;                                                           \
        cmx_chen2022_rain_vel_##SFX chen2022;                                                  \
    } cmx_rain_vel_##SFX;                                                                      \
    /* Koop2000 — src/parameters/IceNucleation.jl:38-55 */                                     \
    typedef struct cmx_koop2000_##SFX {                                                        \
        FT delta_a_w_min, delta_a_w_max, c1, c2, c3, c4, linear_c1, linear_c2;                 \
    } cmx_koop2000_##SFX;                                                                      \
    /* the two ABIFM fields of a dust type (Kaolinite, Illite, DesertDust, …:                */ \
    /* src/parameters/AerosolKaolinite.jl:19-21 etc.): log10 J = m·Δa_w + c  [cm⁻² s⁻¹]      */ \
    typedef struct cmx_abifm_dust_##SFX { FT ABIFM_m, ABIFM_c; } cmx_abifm_dust_##SFX;          \
    /* Mohler2006 (Sᵢ_max, T_thr) — src/parameters/IceNucleation.jl:13-18; the four deposition fields of DesertDust /       */ \
    /* ArizonaTestDust (S₀_warm, S₀_cold, a_warm, a_cold) — src/parameters/AerosolDesertDust.jl:13-21, AerosolATD.jl:12-20   */ \
    typedef struct cmx_mohler2006_##SFX { FT S_i_max, T_thr; } cmx_mohler2006_##SFX;           \
    typedef struct cmx_mohler_dust_##SFX { FT S0_warm, S0_cold, a_warm, a_cold; } cmx_mohler_dust_##SFX; \
    /* the two deposition fields of a mineral (Kaolinite, Feldspar, Ferrihydrite, …: src/parameters/AerosolKaolinite.jl etc.): */ \
    /* log10 J = m·Δa_w + c  [cm⁻² s⁻¹]                                                                                   */ \
    typedef struct cmx_deposition_dust_##SFX { FT deposition_m, deposition_c; } cmx_deposition_dust_##SFX; \
    /* H2SO4SolutionParameters — src/parameters/Aerosol_H2SO4_Solution.jl (Luo et al. 1995) */  \
    typedef struct cmx_h2so4_solution_params_##SFX { FT T_max, T_min, w_2, c1, c2, c3, c4, c5, c6, c7; } cmx_h2so4_solution_params_##SFX; \
    /* ---- 1-moment scheme: src/parameters/Microphysics1M.jl ---------------------------- */   \
    /* ParticleMass — m(r) = m0 χm (r/r0)^(me+Δm); gamma_coeff = Γ(me+Δm+1) host-derived */     \
    typedef struct cmx_particle_mass_##SFX { FT r0, m0, me, delta_m, chi_m, gamma_coeff; }     \
        cmx_particle_mass_##SFX;                                                               \
    /* ParticleArea — a(r) = a0 χa (r/r0)^(ae+Δa) */                                           \
    typedef struct cmx_particle_area_##SFX { FT a0, ae, delta_a, chi_a; }                      \
        cmx_particle_area_##SFX;                                                               \
    typedef struct cmx_ventilation_##SFX { FT a, b; } cmx_ventilation_##SFX;                   \
    /* Acnv1M (τ, q_threshold, k) and VarTimescaleAcnv (τ, α, Nc) */                           \
    typedef struct cmx_acnv_1m_##SFX { FT tau, q_threshold, k; } cmx_acnv_1m_##SFX;            \
    typedef struct cmx_var_timescale_acnv_##SFX { FT tau, alpha, Nc; }                         \
        cmx_var_timescale_acnv_##SFX;                                                          \
    /* CloudLiquid{ρw, r_eff, N_0}; CloudIce{pdf(n0), mass, ρᵢ, r_eff, N_0} */                 \
    typedef struct cmx_cloud_liquid_##SFX { FT rho_w, r_eff, N_0; } cmx_cloud_liquid_##SFX;    \
    typedef struct cmx_cloud_ice_##SFX {                                                       \
        FT n0; cmx_particle_mass_##SFX mass; FT rho_i, r_eff, N_0;                             \
    } cmx_cloud_ice_##SFX;                                                                     \
    /* Rain{pdf(n0), mass, area, vent} */                                                      \
    typedef struct cmx_rain_##SFX {                                                            \
        FT n0; cmx_particle_mass_##SFX mass; cmx_particle_area_##SFX area;                     \
        cmx_ventilation_##SFX vent;                                                            \
    } cmx_rain_##SFX;                                                                          \
    /* Snow{pdf(μ, ν), mass, area, vent, aspr(ϕ, κ), ρᵢ, gamma_aspect_oblate/prolate} */       \
    typedef struct cmx_snow_##SFX {                                                            \
        FT mu, nu; cmx_particle_mass_##SFX mass; cmx_particle_area_##SFX area;                 \
        cmx_ventilation_##SFX vent; FT phi, kappa, rho_i, gamma_aspect_oblate,                 \
            gamma_aspect_prolate;                                                              \
    } cmx_snow_##SFX;                                                                          \
    /* Blk1MVelTypeRain / Blk1MVelTypeSnow — src/parameters/TerminalVelocity.jl:12-30,76-85 */ \
    typedef struct cmx_blk1m_vel_rain_##SFX {                                                  \
        FT r0, ve, delta_v, chi_v, rho_w, C_drag, grav, gamma_vent, gamma_term, gamma_accr,    \
            gamma_accr_rain_sink;                                                              \
    } cmx_blk1m_vel_rain_##SFX;                                                                \
    typedef struct cmx_blk1m_vel_snow_##SFX {                                                  \
        FT r0, ve, delta_v, chi_v, v0, gamma_vent, gamma_term, gamma_accr;                     \
    } cmx_blk1m_vel_snow_##SFX;                                                                \
    /* Frostenberg2023 — src/parameters/IceNucleation.jl:171-193 (log_a = log(a), host-derived) */ \
    typedef struct cmx_frostenberg2023_##SFX { FT sigma, a, b, T_freeze, log_a; } cmx_frostenberg2023_##SFX; \
    /* process_params of Microphysics1MParams (src/parameters/Microphysics1MOptions.jl:296-   */ \
    /* 395), flattened: every variant's parameters are present, `flags` says which are read */  \
    typedef struct cmx_process_params_1m_##SFX {                                               \
        FT cloud_liquid_formation_tau_relax, cloud_ice_formation_tau_relax;                    \
        cmx_frostenberg2023_##SFX cloud_ice_formation_frostenberg; /* TemperatureDependent :314-318 */ \
        cmx_acnv_1m_##SFX rain_autoconversion;             /* Kessler1M          */            \
        cmx_var_timescale_acnv_##SFX rain_autoconversion_nd; /* PrescribedNd     */            \
        cmx_acnv_1m_##SFX snow_autoconversion;             /* NoSupersaturation  */            \
        FT r_ice_snow;                                     /* WithSupersaturation */           \
        FT e_lcl_rai, e_lcl_sno, e_icl_rai, e_icl_sno, e_rai_sno, coeff_disp;                  \
    } cmx_process_params_1m_##SFX;                                                             \
    /* Microphysics1MParams — src/parameters/Microphysics1MParams.jl:63-70 */                  \
    typedef struct cmx_microphysics_1m_##SFX {                                                 \
        cmx_process_params_1m_##SFX process_params;                                            \
        cmx_cloud_liquid_##SFX cloud_liquid;                                                   \
        cmx_cloud_ice_##SFX cloud_ice;                                                         \
        cmx_rain_##SFX rain;                                                                   \
        cmx_snow_##SFX snow;                                                                   \
        cmx_air_properties_##SFX air_properties;                                               \
        cmx_blk1m_vel_rain_##SFX vel_rain;                                                     \
        cmx_blk1m_vel_snow_##SFX vel_snow;                                                     \
    } cmx_microphysics_1m_##SFX;                                                               \
    /* AerosolActivationParameters — src/parameters/AerosolActivation.jl:12-37 */              \
    typedef struct cmx_aerosol_activation_params_##SFX {                                       \
        FT M_w, R, rho_w, rho_i, sigma, g, f1, f2, g1, g2, p1, p2;                             \
    } cmx_aerosol_activation_params_##SFX;                                                     \
    /* One lognormal mode of an AerosolDistribution (src/AerosolModel.jl:26-100), reduced to */ \
    /* what the activation needs: the component tuples of Mode_B / Mode_κ enter only through */ \
    /* mean_hygroscopicity_parameter (src/AerosolActivation.jl:55-95) and Σ M_j·w_j (:313),  */ \
    /* both evaluated on the host.                                                           */ \
    typedef struct cmx_aerosol_mode_##SFX {                                                    \
        FT r_dry, stdev, N, hygroscopicity, molar_mass_mix;                                    \
    } cmx_aerosol_mode_##SFX;                                                                  \
    typedef struct cmx_aerosol_distribution_##SFX {                                            \
        int32_t n_modes; int32_t pad_;                                                         \
        cmx_aerosol_mode_##SFX modes[CMX_ARG_MAX_MODES];                                       \
    } cmx_aerosol_distribution_##SFX;                                                          \
    /* ParametersP3 (src/parameters/MicrophysicsP3.jl:267-286), the fields the shape solver  */ \
    /* reads: MassPowerLaw (α_va, β_va :26-31), AreaPowerLaw (γ, σ :60-65), SlopePowerLaw    */ \
    /* (a, b, c, μ_max :104-113) or SlopeConstant (μ :139-142), ρ_i, ρ_l                      */ \
    typedef struct cmx_p3_params_##SFX {                                                       \
        FT alpha_va, beta_va, gamma, sigma, slope_a, slope_b, slope_c, mu_max, mu_const,       \
            rho_i, rho_l, tau_wet, T_freeze;                                                   \
    } cmx_p3_params_##SFX;                                                                     \
    /* CMP.Chen2022VelTypeSmallIce / LargeIce — src/parameters/TerminalVelocity.jl:207-216,    */ \
    /* 247-257 (Chen et al. 2022 tables B3 / B5 + the small/large cutoff dimension)            */ \
    typedef struct cmx_chen2022_small_ice_vel_##SFX {                                          \
        FT A[3], B[3], C[4], E[3], F[3], G[3], cutoff;                                         \
    } cmx_chen2022_small_ice_vel_##SFX;                                                        \
    typedef struct cmx_chen2022_large_ice_vel_##SFX {                                          \
        FT A[3], B[3], C[3], E[3], F[3], G[3], H[3], cutoff;                                   \
    } cmx_chen2022_large_ice_vel_##SFX;                                                        \
    typedef struct cmx_chen2022_ice_vel_##SFX {                                                \
        cmx_chen2022_small_ice_vel_##SFX small_ice;                                            \
        cmx_chen2022_large_ice_vel_##SFX large_ice;                                            \
    } cmx_chen2022_ice_vel_##SFX;                                                              \
    /* Quadrature.ChebyshevGauss(n) / GaussLegendre(FT, n) — src/Quadrature.jl:168-175,226-252: */ \
    /* n nodes yᵢ on [-1, 1] and TOTAL weights inv_weight_fun(yᵢ)·weight(i) (host-built once,   */ \
    /* like the reference builds GaussLegendre host-side and ships it as an isbits struct)      */ \
    typedef struct cmx_quadrature_##SFX {                                                      \
        int32_t n, reserved;                                                                   \
        FT node[CMX_QUAD_MAX], weight[CMX_QUAD_MAX];                                           \
    } cmx_quadrature_##SFX;                                                                    \
    /* Parameters0M — src/parameters/Microphysics0M.jl:12-28 */                                \
    typedef struct cmx_parameters_0m_##SFX { FT tau_precip, qc_0, S_0; } cmx_parameters_0m_##SFX; \
    /* LocalRimeDensity — src/parameters/MicrophysicsP3.jl:202-239 (Cober & List 1993 Eq. 16-17) */ \
    typedef struct cmx_local_rime_density_##SFX { FT a, b, c, rho_ice; } cmx_local_rime_density_##SFX; \
    /* RainFreezing (Bigg 1953 / Barklie–Gokhale 1959) — src/parameters/IceNucleation.jl:129-146 */ \
    typedef struct cmx_rain_freezing_##SFX { FT het_a, het_B; } cmx_rain_freezing_##SFX;       \
    /* MorrisonMilbrandt2014 — src/parameters/IceNucleation.jl:80-107 */                       \
    typedef struct cmx_morrison_milbrandt2014_##SFX { FT T_dep_thres, c1, c2, T0, het_a, het_B; } \
        cmx_morrison_milbrandt2014_##SFX;                                                      \
    /* H2S04NucleationParameters (sic: the reference's spelling), OrganicNucleationParameters, */ \
    /* MixedNucleationParameters — src/parameters/AerosolModalNucleation.jl:4-129             */ \
    typedef struct cmx_h2so4_nucleation_##SFX {                                                \
        FT p_b_n, p_b_i, u_b_n, u_b_i, v_b_n, v_b_i, w_b_n, w_b_i, p_t_n, p_t_i, u_t_n, u_t_i,  \
            v_t_n, v_t_i, w_t_n, w_t_i, p_A_n, p_A_i, a_n, a_i;                                \
    } cmx_h2so4_nucleation_##SFX;                                                              \
    typedef struct cmx_organic_nucleation_##SFX {                                              \
        FT a_1, a_2, a_3, a_4, a_5, Y_MTO3, Y_MTOH, k_MTO3, k_MTOH, exp_MTO3, exp_MTOH;        \
    } cmx_organic_nucleation_##SFX;                                                            \
    typedef struct cmx_mixed_nucleation_##SFX { FT k_H2SO4org, k_MTOH, exp_MTOH; }             \
        cmx_mixed_nucleation_##SFX;                                                            \
    /* P3IceParams — src/parameters/Microphysics2MParams.jl:58-86: scheme (+ its vent and      */ \
    /* ρ_rim_local members, src/parameters/MicrophysicsP3.jl:267-288), terminal_velocity       */ \
    /* (Chen2022VelType: rain, small_ice, large_ice), cloud_pdf, rain_pdf, ice_nucleation,     */ \
    /* rain_freezing, inp_depletion_model.τ_act, quad                                          */ \
    typedef struct cmx_p3_ice_params_##SFX {                                                   \
        cmx_p3_params_##SFX scheme;                                                            \
        cmx_ventilation_##SFX vent;                                                            \
        cmx_local_rime_density_##SFX rho_rim_local;                                            \
        cmx_chen2022_rain_vel_##SFX vel_rain;                                                  \
        cmx_chen2022_ice_vel_##SFX vel_ice;                                                    \
        cmx_cloud_pdf_sb2006_##SFX cloud_pdf;                                                  \
        cmx_rain_pdf_sb2006_##SFX rain_pdf;                                                    \
        cmx_frostenberg2023_##SFX ice_nucleation;                                              \
        cmx_rain_freezing_##SFX rain_freezing;                                                 \
        FT tau_act;                                                                            \
        cmx_quadrature_##SFX quad;                                                             \
    } cmx_p3_ice_params_##SFX;                                                                 \
    /* parcel_params — parcel/ParcelModel.jl:12-43 — as the constructors of run_parcel read it  */ \
    /* (:230-366): tps, aps, aap, ips.homogeneous / .deposition / .p3, ip, the coefficients of   */ \
    /* the `aerosol` member (ABIFM, deposition_J, Mohler: zero-filled where the aerosol type has */ \
    /* none), then the scalars.  grav = TDI.grav(tps), rho_w / rho_i = wps.ρw / wps.ρi,          */ \
    /* aero_N = pp.Nₐ, aero_M / aero_kappa = aerosol.M / aerosol.κ (AeroAct),                    */ \
    /* tau_relax_liq / tau_relax_ice = MNE.τ_relax(liquid) / (ice) of the NonEq _simple options  */ \
    typedef struct cmx_parcel_params_##SFX {                                                   \
        cmx_thermo_##SFX tps;                                                                  \
        cmx_air_properties_##SFX aps;                                                          \
        cmx_aerosol_activation_params_##SFX aap;                                               \
        cmx_koop2000_##SFX homogeneous;                                                        \
        cmx_mohler2006_##SFX deposition;                                                       \
        cmx_morrison_milbrandt2014_##SFX p3;                                                   \
        cmx_frostenberg2023_##SFX ip;                                                          \
        cmx_abifm_dust_##SFX aerosol_abifm;                                                    \
        cmx_deposition_dust_##SFX aerosol_deposition;                                          \
        cmx_mohler_dust_##SFX aerosol_mohler;                                                  \
        FT const_dt, r_nuc, A_aer, aero_sigma_g, aero_N, aero_M, aero_kappa;                   \
        FT grav, rho_w, rho_i, tau_relax_liq, tau_relax_ice;                                   \
    } cmx_parcel_params_##SFX;

#define CMX_ARG_MAX_MODES 8
#define CMX_QUAD_MAX 128

CMX_DECLARE_PARAM_STRUCTS(float, f32)
CMX_DECLARE_PARAM_STRUCTS(double, f64)

/* ---------------------------------------------------------------------------
 * Size contract of every parameter struct: field count × sizeof(FT) (+ the 8-byte integer header of the two structs
 * that carry a count).  No struct has padding — every member is an FT or an array / struct of FT — so a binding that
 * declares the same fields in the same order (INTEGRATION.md §2 quotes these counts) has the same layout; a binding
 * with a missing field (e.g. the 13th member `cv_l` of cmx_thermo_*) has a different sizeof and must not compile.
 * tests/test_abi.py checks the same numbers from the Python side, tests/native/abi_caller.c from plain C.
 * ------------------------------------------------------------------------- */
#if defined(__cplusplus)
#define CMX_STATIC_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define CMX_STATIC_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
#define CMX_ASSERT_PARAM_STRUCT_SIZES(FT, SFX) \
    CMX_STATIC_ASSERT(sizeof(cmx_abifm_dust_##SFX) == 2 * sizeof(FT), "cmx_abifm_dust");\
    CMX_STATIC_ASSERT(sizeof(cmx_mohler2006_##SFX) == 2 * sizeof(FT), "cmx_mohler2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_mohler_dust_##SFX) == 4 * sizeof(FT), "cmx_mohler_dust");\
    CMX_STATIC_ASSERT(sizeof(cmx_deposition_dust_##SFX) == 2 * sizeof(FT), "cmx_deposition_dust");\
    CMX_STATIC_ASSERT(sizeof(cmx_h2so4_solution_params_##SFX) == 10 * sizeof(FT), "cmx_h2so4_solution_params");\
    CMX_STATIC_ASSERT(sizeof(cmx_accr_sb2006_##SFX) == 4 * sizeof(FT), "cmx_accr_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_acnv_1m_##SFX) == 3 * sizeof(FT), "cmx_acnv_1m");\
    CMX_STATIC_ASSERT(sizeof(cmx_acnv_sb2006_##SFX) == 6 * sizeof(FT), "cmx_acnv_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_aerosol_activation_params_##SFX) == 12 * sizeof(FT), "cmx_aerosol_activation_params");\
    CMX_STATIC_ASSERT(sizeof(cmx_aerosol_distribution_##SFX) == 8 + 40 * sizeof(FT), "cmx_aerosol_distribution");\
    CMX_STATIC_ASSERT(sizeof(cmx_aerosol_mode_##SFX) == 5 * sizeof(FT), "cmx_aerosol_mode");\
    CMX_STATIC_ASSERT(sizeof(cmx_air_properties_##SFX) == 3 * sizeof(FT), "cmx_air_properties");\
    CMX_STATIC_ASSERT(sizeof(cmx_b1994_##SFX) == 9 * sizeof(FT), "cmx_b1994");\
    CMX_STATIC_ASSERT(sizeof(cmx_blk1m_vel_rain_##SFX) == 11 * sizeof(FT), "cmx_blk1m_vel_rain");\
    CMX_STATIC_ASSERT(sizeof(cmx_blk1m_vel_snow_##SFX) == 8 * sizeof(FT), "cmx_blk1m_vel_snow");\
    CMX_STATIC_ASSERT(sizeof(cmx_breakup_sb2006_##SFX) == 4 * sizeof(FT), "cmx_breakup_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_bulk_2m_schemes_##SFX) == 28 * sizeof(FT), "cmx_bulk_2m_schemes");\
    CMX_STATIC_ASSERT(sizeof(cmx_chen2022_ice_vel_##SFX) == 42 * sizeof(FT), "cmx_chen2022_ice_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_chen2022_large_ice_vel_##SFX) == 22 * sizeof(FT), "cmx_chen2022_large_ice_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_chen2022_rain_vel_##SFX) == 12 * sizeof(FT), "cmx_chen2022_rain_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_chen2022_small_ice_vel_##SFX) == 20 * sizeof(FT), "cmx_chen2022_small_ice_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_cloud_ice_##SFX) == 10 * sizeof(FT), "cmx_cloud_ice");\
    CMX_STATIC_ASSERT(sizeof(cmx_cloud_liquid_##SFX) == 3 * sizeof(FT), "cmx_cloud_liquid");\
    CMX_STATIC_ASSERT(sizeof(cmx_cloud_pdf_sb2006_##SFX) == 7 * sizeof(FT), "cmx_cloud_pdf_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_evap_sb2006_##SFX) == 10 * sizeof(FT), "cmx_evap_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_frostenberg2023_##SFX) == 5 * sizeof(FT), "cmx_frostenberg2023");\
    CMX_STATIC_ASSERT(sizeof(cmx_kk2000_##SFX) == 7 * sizeof(FT), "cmx_kk2000");\
    CMX_STATIC_ASSERT(sizeof(cmx_koop2000_##SFX) == 8 * sizeof(FT), "cmx_koop2000");\
    CMX_STATIC_ASSERT(sizeof(cmx_ld2004_##SFX) == 4 * sizeof(FT), "cmx_ld2004");\
    CMX_STATIC_ASSERT(sizeof(cmx_local_rime_density_##SFX) == 4 * sizeof(FT), "cmx_local_rime_density");\
    CMX_STATIC_ASSERT(sizeof(cmx_microphysics_1m_##SFX) == 90 * sizeof(FT), "cmx_microphysics_1m");\
    CMX_STATIC_ASSERT(sizeof(cmx_morrison_milbrandt2014_##SFX) == 6 * sizeof(FT), "cmx_morrison_milbrandt2014");\
    CMX_STATIC_ASSERT(sizeof(cmx_numadj_horn2012_##SFX) == 1 * sizeof(FT), "cmx_numadj_horn2012");\
    CMX_STATIC_ASSERT(sizeof(cmx_p3_ice_params_##SFX) == 8 + 354 * sizeof(FT), "cmx_p3_ice_params");\
    CMX_STATIC_ASSERT(sizeof(cmx_p3_params_##SFX) == 13 * sizeof(FT), "cmx_p3_params");\
    CMX_STATIC_ASSERT(sizeof(cmx_parameters_0m_##SFX) == 3 * sizeof(FT), "cmx_parameters_0m");\
    CMX_STATIC_ASSERT(sizeof(cmx_particle_area_##SFX) == 4 * sizeof(FT), "cmx_particle_area");\
    CMX_STATIC_ASSERT(sizeof(cmx_particle_mass_##SFX) == 6 * sizeof(FT), "cmx_particle_mass");\
    CMX_STATIC_ASSERT(sizeof(cmx_process_params_1m_##SFX) == 23 * sizeof(FT), "cmx_process_params_1m");\
    CMX_STATIC_ASSERT(sizeof(cmx_quadrature_##SFX) == 8 + 256 * sizeof(FT), "cmx_quadrature");\
    CMX_STATIC_ASSERT(sizeof(cmx_rain_##SFX) == 13 * sizeof(FT), "cmx_rain");\
    CMX_STATIC_ASSERT(sizeof(cmx_rain_freezing_##SFX) == 2 * sizeof(FT), "cmx_rain_freezing");\
    CMX_STATIC_ASSERT(sizeof(cmx_rain_pdf_sb2006_##SFX) == 10 * sizeof(FT), "cmx_rain_pdf_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_rain_vel_##SFX) == 19 * sizeof(FT), "cmx_rain_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_sb2006_##SFX) == 45 * sizeof(FT), "cmx_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_sb2006_vel_##SFX) == 7 * sizeof(FT), "cmx_sb2006_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_selfcol_sb2006_##SFX) == 3 * sizeof(FT), "cmx_selfcol_sb2006");\
    CMX_STATIC_ASSERT(sizeof(cmx_snow_##SFX) == 19 * sizeof(FT), "cmx_snow");\
    CMX_STATIC_ASSERT(sizeof(cmx_stokes_vel_##SFX) == 3 * sizeof(FT), "cmx_stokes_vel");\
    CMX_STATIC_ASSERT(sizeof(cmx_tc1980_##SFX) == 8 * sizeof(FT), "cmx_tc1980");\
    CMX_STATIC_ASSERT(sizeof(cmx_thermo_##SFX) == 13 * sizeof(FT), "cmx_thermo");\
    CMX_STATIC_ASSERT(sizeof(cmx_var_timescale_acnv_##SFX) == 3 * sizeof(FT), "cmx_var_timescale_acnv");\
    CMX_STATIC_ASSERT(sizeof(cmx_ventilation_##SFX) == 2 * sizeof(FT), "cmx_ventilation");\
    CMX_STATIC_ASSERT(sizeof(cmx_warm_rain_2m_##SFX) == 50 * sizeof(FT), "cmx_warm_rain_2m");

CMX_ASSERT_PARAM_STRUCT_SIZES(float, f32)
CMX_ASSERT_PARAM_STRUCT_SIZES(double, f64)
/* the same contract for the aerosol-nucleation structs, in a macro of their own: tests/test_abi_caller.py pins the row count of the list above */
#define CMX_ASSERT_NUCLEATION_STRUCT_SIZES(FT, SFX) \
    CMX_STATIC_ASSERT((sizeof(cmx_h2so4_nucleation_##SFX) == 20 * sizeof(FT)), "cmx_h2so4_nucleation");\
    CMX_STATIC_ASSERT((sizeof(cmx_organic_nucleation_##SFX) == 11 * sizeof(FT)), "cmx_organic_nucleation");\
    CMX_STATIC_ASSERT((sizeof(cmx_mixed_nucleation_##SFX) == 3 * sizeof(FT)), "cmx_mixed_nucleation");
CMX_ASSERT_NUCLEATION_STRUCT_SIZES(float, f32)
CMX_ASSERT_NUCLEATION_STRUCT_SIZES(double, f64)
/* … and for the parcel-model struct: 13 + 3 + 12 + 8 + 2 + 6 + 5 + 2 + 2 + 4 nested values and 12 scalars (a row of its own spelling: the rows of the
 * two lists above are pinned by tests/test_abi_caller.py and tests/test_nucleation_host.py; tests/test_parcel_host.py checks this one) */
#define CMX_ASSERT_PARCEL_STRUCT_SIZES(FT, SFX) \
    CMX_STATIC_ASSERT( sizeof(cmx_parcel_params_##SFX) == 69 * sizeof(FT) , "cmx_parcel_params");
CMX_ASSERT_PARCEL_STRUCT_SIZES(float, f32)
CMX_ASSERT_PARCEL_STRUCT_SIZES(double, f64)

/* ---------------------------------------------------------------------------
 * Library / device queries
 * ------------------------------------------------------------------------- */
/* (major << 16) | minor */
int32_t cmx_version(void);
/* text of the last HIP error seen by this thread ("" if none); static storage */
const char *cmx_last_hip_error(void);

/* Diagnostic entry (no reference counterpart): the library's own Float64 elementary functions (csrc/cmx_lean_f64.hpp — gfx950 has
 * no Float64 transcendental unit) evaluated over a device column, so that a test can measure them against libm in ulps ON the
 * device.  which: 0 exp2, 1 log2, 2 exp, 3 log, 4 rcp, 5 sqrt, 6 rsqrt, 7 expm1, 8 log1p, 9 erfc (the table-driven form of the ARG kernel),
 * 10 lgamma for z > 0 (the P3 shape solver's); 11-17 the finite-argument forms exp2_fin, exp_fin, rcp_finite, rcp_nz, sqrt_pos, rsqrt_pos,
 * pow_m34_pos and 18 log_pos (positive normal finite arguments only: DESIGN.md section 4.3); 19 the identity (the kernel's own instructions:
 * tools/f64_floor.py subtracts them from the per-dispatch instruction counters of the others). */
int32_t cmx_lean_eval_f64(int32_t which, int64_t n, const double *x, double *y, void *stream);
/* … and the same functions as compiled into the production Float64 kernels' translation units (polynomial coefficients as SGPR literals
 * instead of LDS reads; csrc/Makefile LITCOEF). */
int32_t cmx_lean_eval_literal_f64(int32_t which, int64_t n, const double *x, double *y, void *stream);

/* ---------------------------------------------------------------------------
 * (1) North star — SB2006 two-moment warm-rain fused tendencies.
 *
 * Replaces the broadcast
 *   BMT.bulk_microphysics_tendencies.(Ref(BMT.Microphysics2Moment()), Ref(mp), Ref(tps),
 *                                     ρ, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)
 * src/BulkMicrophysicsTendencies.jl:820-854 → warm_rain_tendencies_2m :707-782
 * (KA wrapper: test/gpu_performance.jl:49-57), plus — when vt_rai_n / vt_rai_m
 * are non-NULL — CM2.rain_terminal_velocity(sb, vel, q_rai, ρ, ρ n_rai)
 * (src/Microphysics2M.jl:685-719) evaluated on the same clamped state.
 *
 * Inputs per point: ρ [kg/m3], T [K], q_tot, q_lcl, q_rai [kg/kg],
 * n_lcl, n_rai [1/kg] (per kg of air, as in BMT).  Outputs: dq_lcl_dt, dq_rai_dt
 * [kg/kg/s], dn_lcl_dt, dn_rai_dt [1/kg/s]; optional number- and mass-weighted
 * rain fall speeds [m/s].  The four identically-zero ice fields of the
 * reference's NamedTuple (BMT:840-842,852-853) are not materialised.
 * `vel` may be NULL iff both velocity columns are NULL.
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_warm_rain_tendencies_f32(
    const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps,
    const cmx_rain_vel_f32 *vel, uint32_t flags, int64_t n,
    const float *rho, const float *T, const float *q_tot, const float *q_lcl,
    const float *n_lcl, const float *q_rai, const float *n_rai,
    float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
    float *vt_rai_n, float *vt_rai_m, void *stream);

int32_t cmx_sb2006_warm_rain_tendencies_f64(
    const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps,
    const cmx_rain_vel_f64 *vel, uint32_t flags, int64_t n,
    const double *rho, const double *T, const double *q_tot, const double *q_lcl,
    const double *n_lcl, const double *q_rai, const double *n_rai,
    double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
    double *vt_rai_n, double *vt_rai_m, void *stream);

/* (1b) The same tendencies behind the host model's own data layouts.
 * Input: 7 SEGMENTED columns in[k] (k = rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai): n_seg runs of seg_len contiguous
 * elements, run s of column k starting at in[k] + s·in_seg_stride[k] (elements).  That is a ClimaCore field in place: a
 * DataLayouts.VIJFH array (Nv, Ni, Nj, Nf, Nh) stores component f of element h as one run of Nv·Ni·Nj elements, i.e.
 * in[k] = pointer(parent(field)) + f·Nv·Ni·Nj, seg_len = Nv·Ni·Nj, stride = Nv·Ni·Nj·Nf, n_seg = Nh
 * (test/gpu_clima_core_test.jl:16-30,100-114); VF columns and VIJHF fields are the single-run case n_seg = 1 (strides may be NULL).
 * Output, exactly one of:
 *   out[4] + out_seg_stride[4]: dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt as segmented columns (each with its own stride);
 *   out_aos: n_seg·seg_len rows of 8 FT — the reference's result type, Vector{@NamedTuple{dq_lcl_dt, dn_lcl_dt, dq_rai_dt,
 *            dn_rai_dt, dq_ice_dt, dq_rim_dt, db_rim_dt, dn_lcl_activation_dt}} (BMT:852-853, test/gpu_performance.jl:212-216;
 *            the last four are 0), 16-byte aligned.
 * Values are bit-identical to cmx_sb2006_warm_rain_tendencies_* on the same points.  flags: CMX_SB2006_LIMITED. */
int32_t cmx_sb2006_warm_rain_tendencies_fields_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_seg,
                                                   int64_t seg_len, const float *const *in, const int64_t *in_seg_stride, float *const *out,
                                                   const int64_t *out_seg_stride, float *out_aos, void *stream);
int32_t cmx_sb2006_warm_rain_tendencies_fields_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_seg,
                                                   int64_t seg_len, const double *const *in, const int64_t *in_seg_stride, double *const *out,
                                                   const int64_t *out_seg_stride, double *out_aos, void *stream);

/* ---------------------------------------------------------------------------
 * (2) SB2006 per-process rates ("verbose" variant of the same kernel).
 *
 * Replaces the KA wrapper test_2_moment_SB2006_kernel! / SB2006_2M_kernel
 * (test/gpu_tests.jl:220-244): the individual CM2 process functions on
 * (q_tot, q_lcl, q_rai, N_lcl, N_rai, ρ, T) with N in [1/m3], plus the
 * cond/evap relaxation of src/MicrophysicsNonEq.jl:117-140.  `out` is a
 * host array of CMX_SB2006_NPROC device column pointers (any may be NULL to
 * skip that column), indexed by cmx_sb2006_process_column.
 * ------------------------------------------------------------------------- */
typedef enum cmx_sb2006_process_column {
    CMX_SB_ACNV_DQ_LCL = 0,  /* autoconversion(...).dq_lcl_dt    CM2:396-427 */
    CMX_SB_ACNV_DN_LCL,      /*                 .dN_lcl_dt [1/m3/s]          */
    CMX_SB_ACNV_DQ_RAI,      /*                 .dq_rai_dt                   */
    CMX_SB_ACNV_DN_RAI,      /*                 .dN_rai_dt [1/m3/s]          */
    CMX_SB_LCL_SELFCOL,      /* cloud_liquid_self_collection      CM2:488-501 */
    CMX_SB_ACCR_DQ_LCL,      /* accretion(...).dq_lcl_dt          CM2:445-470 */
    CMX_SB_ACCR_DN_LCL,      /*               .dN_lcl_dt [1/m3/s]            */
    CMX_SB_ACCR_DQ_RAI,      /*               .dq_rai_dt                     */
    CMX_SB_RAI_SELFCOL,      /* rain_self_collection [1/m3/s]     CM2:545-560 */
    CMX_SB_RAI_BREAKUP,      /* rain_breakup [1/m3/s]             CM2:579-601 */
    CMX_SB_RAI_VEL_N,        /* rain_terminal_velocity[1] (per `flags`) CM2:685-719 */
    CMX_SB_RAI_VEL_M,        /* rain_terminal_velocity[2]                    */
    CMX_SB_EVAP_DN_RAI,      /* rain_evaporation.∂ₜρn_rai [1/m3/s] CM2:780-828 */
    CMX_SB_EVAP_DQ_RAI,      /* rain_evaporation.∂ₜq_rai                     */
    CMX_SB_NUMADJ_RAI,       /* number_tendency_from_mass_limits(rain; q_rai, N_rai/ρ) CM2:882-891 */
    CMX_SB_NUMADJ_LCL,       /* same for cloud (xc_min, xc_max; q_lcl, N_lcl/ρ)     */
    CMX_SB_CONDEVAP,         /* _conv_q_vap_to_q_lcl_const        NonEq:117-140 */
    CMX_SB_DEVAP_DN_RAI,     /* ∂rain_evaporation_∂N_rai_∂q_rai(…).∂N_rai = ∂ₜρn_rai / N_rai  [1/s]  CM2:844-855 */
    CMX_SB_DEVAP_DQ_RAI,     /*                                   .∂q_rai = ∂ₜq_rai / q_rai   [1/s]              */
    CMX_SB2006_NPROC
} cmx_sb2006_process_column;

int32_t cmx_sb2006_process_rates_f32(
    const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps,
    const cmx_rain_vel_f32 *vel, uint32_t flags, int64_t n,
    const float *q_tot, const float *q_lcl, const float *q_rai, const float *N_lcl,
    const float *N_rai, const float *rho, const float *T,
    float *const out[CMX_SB2006_NPROC], void *stream);

int32_t cmx_sb2006_process_rates_f64(
    const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps,
    const cmx_rain_vel_f64 *vel, uint32_t flags, int64_t n,
    const double *q_tot, const double *q_lcl, const double *q_rai, const double *N_lcl,
    const double *N_rai, const double *rho, const double *T,
    double *const out[CMX_SB2006_NPROC], void *stream);

/* CM2.cloud_terminal_velocity(pdf_c, vel::StokesRegimeVelType, q_liq, ρₐ, N_liq) — src/Microphysics2M.jl:647-664:
 * number- and mass-weighted mean fall speeds of the cloud droplets (Stokes regime, generalized-gamma PSD moments
 * M^{2/3}, M^{5/3}; DistributionTools.jl:109-112).  N_liq is per m³ as in the reference.  Either output may be NULL. */
int32_t cmx_sb2006_cloud_terminal_velocity_f32(const cmx_cloud_pdf_sb2006_f32 *pdf_c, const cmx_stokes_vel_f32 *vel, int64_t n,
                                               const float *q_liq, const float *rho, const float *N_liq, float *vt_n, float *vt_m,
                                               void *stream);
int32_t cmx_sb2006_cloud_terminal_velocity_f64(const cmx_cloud_pdf_sb2006_f64 *pdf_c, const cmx_stokes_vel_f64 *vel, int64_t n,
                                               const double *q_liq, const double *rho, const double *N_liq, double *vt_n, double *vt_m,
                                               void *stream);

/* ---------------------------------------------------------------------------
 * (2b) Fused COLUMN kernel: the north-star tendencies + the sedimentation step a host model applies
 * right after them, in one pass: 7 columns in, 4 out (44 B/point f32) instead of 88 B/point for the unfused sequence.
 *
 * Replaces, per column of n_lev contiguous levels (level 0 = lowest; flat index i = col·n_lev + k — a ClimaCore VF /
 * VIJFH(Ni = Nj = 1) column field; test/gpu_clima_core_test.jl:16-30 builds such spaces):
 *   tend = BMT.bulk_microphysics_tendencies(Microphysics2Moment(), mp, tps, ρ, T, q_tot, q_lcl, n_lcl, q_rai, n_rai)   BMT:820-854
 *   (w_n, w_m) = CM2.rain_terminal_velocity(sb, vel, q_rai, ρ, ρ n_rai)                                                CM2:685-719
 *   (c_n, c_m) = CM2.cloud_terminal_velocity(sb.pdf_c, cloud_vel, q_lcl, ρ, ρ n_lcl)    [iff cloud_vel != NULL]        CM2:647-664
 * followed by the host model's first-order upwind ("right-biased": the value of the cell above) flux divergence
 *   F_k = ρ_k χ_k w_k,   ∂χ_k/∂t += (F_{k+1} − F_k) · inv_dz[k] / ρ_k,   F_{n_lev} = 0,
 * for χ = q_rai (w_m), n_rai (w_n) and — with cloud_vel — q_lcl (c_m), n_lcl (c_n).  The flux scheme is the host model's
 * (ClimaAtmos precipitation advection), NOT part of the reference package: its oracle is a restatement of the formula
 * above ("parity unpinned" for the flux step; the tendencies and fall speeds it consumes are pinned as in (1)).
 * flags: CMX_SB2006_LIMITED and exactly one of CMX_VEL_SB2006 / CMX_VEL_CHEN2022.  inv_dz: n_lev values 1/Δz_k [1/m].
 * precip_flux (optional, n_col values): F_0 of q_rai, the surface precipitation mass flux [kg m⁻² s⁻¹].
 * Results do not depend on tile boundaries or alignment (bit-identical to a one-point-per-lane evaluation).
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_column_tendencies_sedimentation_f32(
    const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
    const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const float *inv_dz,
    const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai,
    const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt, float *precip_flux,
    void *stream);
int32_t cmx_sb2006_column_tendencies_sedimentation_f64(
    const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
    const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const double *inv_dz,
    const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
    const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt, double *precip_flux,
    void *stream);

/* Bulk cloud → rain conversion of the other two-moment schemes — src/Microphysics2M.jl:920-1003:
 *   acnv = CM2.conv_q_lcl_to_q_rai(scheme, q_lcl, ρ, N_d[, smooth_transition])     KK2000 | B1994 | TC1980 | LD2004
 *   accr = CM2.accretion(scheme, q_lcl, q_rai, ρ)                                   KK2000 | B1994 | TC1980
 * (KA kernels test_2_moment_acnv_kernel! / test_2_moment_accr_kernel!, test/gpu_tests.jl:782-818).  `scheme` is one of
 * CMX_2M_KK2000 … CMX_2M_LD2004; CMX_2M_SMOOTH_TRANSITION selects the logistic threshold (src/Common.jl:125-139) instead
 * of the step.  N_d per m³.  accr (and q_rai) may be NULL; LD2004 has no accretion (accr must be NULL). */
#define CMX_2M_KK2000 0u
#define CMX_2M_B1994 1u
#define CMX_2M_TC1980 2u
#define CMX_2M_LD2004 3u
#define CMX_2M_SMOOTH_TRANSITION (1u << 8)
int32_t cmx_bulk_2m_cloud_to_rain_f32(const cmx_bulk_2m_schemes_f32 *schemes, uint32_t scheme, int64_t n, const float *q_lcl,
                                      const float *q_rai, const float *rho, const float *N_d, float *acnv, float *accr, void *stream);
int32_t cmx_bulk_2m_cloud_to_rain_f64(const cmx_bulk_2m_schemes_f64 *schemes, uint32_t scheme, int64_t n, const double *q_lcl,
                                      const double *q_rai, const double *rho, const double *N_d, double *acnv, double *accr,
                                      void *stream);

/* ---------------------------------------------------------------------------
 * (4) Ice nucleation rates — ABIFM immersion freezing + Koop-2000 homogeneous freezing.
 *
 * Replaces the KA wrappers IceNucleation_ABIFM_J_kernel!, IceNucleation_homogeneous_J_kernel!,
 * Common_a_w_ice_kernel! (test/gpu_tests.jl:294-362) and the per-droplet products the parcel
 * model forms from them (parcel/ParcelTendencies.jl:120-133,194-205):
 *   Δa_w    = a_w − CO.a_w_ice(tps, T)                         src/Common.jl:267-271
 *   J_het   = CMI_het.ABIFM_J(dust, Δa_w)          [m⁻² s⁻¹]  src/IceNucleation.jl:124-134
 *   J_hom   = CMI_hom.homogeneous_J_cubic(ip, Δa_w) [m⁻³ s⁻¹]  src/IceNucleation.jl:557-565
 *             (or homogeneous_J_linear, :581-584, with CMX_ICENUC_HOM_LINEAR)
 *   rate_het = J_het · 4π r²    rate_hom = J_hom · 4/3 π r³    [s⁻¹ per droplet]
 * Inputs per point: T [K], a_w [-], r [m].  Any output column may be NULL.
 * homogeneous_J_cubic THROWS DomainError outside [Δa_w_min, Δa_w_max]; a device kernel cannot:
 * such points get J_hom = rate_hom = NaN and, if `n_domain_errors` is non-NULL, are counted.
 * `n_domain_errors` is a device array of CMX_ICENUC_ERR_WORDS int64, zeroed by the caller; the number of
 * domain-error points is the SUM of all its words (counts accumulate across calls until re-zeroed).
 * Only every (WORDS/SLOTS)-th word is written: one 128-byte line per slot, so that the ≈1e5 concurrent
 * workgroups of a 1e8-point launch do not serialise on a single L2 atomic unit.
 * ------------------------------------------------------------------------- */
#define CMX_ICENUC_HOM_LINEAR   (1u << 0)   /* homogeneous_J_linear instead of homogeneous_J_cubic */
#define CMX_ICENUC_ERR_SLOTS    64
#define CMX_ICENUC_ERR_WORDS    1024        /* int64 words in the n_domain_errors buffer (8 KiB) */

int32_t cmx_ice_nucleation_rates_f32(
    const cmx_thermo_f32 *tps, const cmx_abifm_dust_f32 *dust, const cmx_koop2000_f32 *koop,
    uint32_t flags, int64_t n, const float *T, const float *a_w, const float *r,
    float *delta_a_w, float *J_het, float *J_hom, float *rate_het, float *rate_hom,
    int64_t *n_domain_errors, void *stream);

int32_t cmx_ice_nucleation_rates_f64(
    const cmx_thermo_f64 *tps, const cmx_abifm_dust_f64 *dust, const cmx_koop2000_f64 *koop,
    uint32_t flags, int64_t n, const double *T, const double *a_w, const double *r,
    double *delta_a_w, double *J_het, double *J_hom, double *rate_het, double *rate_hom,
    int64_t *n_domain_errors, void *stream);

/* The same with the water activity of a sulphuric-acid solution droplet computed in the kernel, as the parcel model drives it
 * (parcel/ParcelTendencies.jl:120-133: a_w = CO.a_w_xT(H2SO4_prs, tps, x_sulph, T) when T < T_max of the solution fit): the second
 * input column is x, the weight fraction of H2SO4 [-], instead of a_w;  a_w = p_sol(x, T) / p_sat,liq(T), src/Common.jl:188-246. */
int32_t cmx_ice_nucleation_rates_xT_f32(const cmx_thermo_f32 *tps, const cmx_abifm_dust_f32 *dust, const cmx_koop2000_f32 *koop,
                                        const cmx_h2so4_solution_params_f32 *h2so4, uint32_t flags, int64_t n, const float *T, const float *x_sulph,
                                        const float *r, float *delta_a_w, float *J_het, float *J_hom, float *rate_het, float *rate_hom,
                                        int64_t *n_domain_errors, void *stream);
int32_t cmx_ice_nucleation_rates_xT_f64(const cmx_thermo_f64 *tps, const cmx_abifm_dust_f64 *dust, const cmx_koop2000_f64 *koop,
                                        const cmx_h2so4_solution_params_f64 *h2so4, uint32_t flags, int64_t n, const double *T, const double *x_sulph,
                                        const double *r, double *delta_a_w, double *J_het, double *J_hom, double *rate_het, double *rate_hom,
                                        int64_t *n_domain_errors, void *stream);

/* CO.H2SO4_soln_saturation_vapor_pressure(prs, x, T) [Pa] and CO.a_w_xT(prs, tps, x, T) over columns — src/Common.jl:188-246
 * (KA wrapper Common_H2SO4_kernel!, test/gpu_tests.jl:876-893).  Either output may be NULL. */
int32_t cmx_h2so4_solution_f32(const cmx_h2so4_solution_params_f32 *prs, const cmx_thermo_f32 *tps, int64_t n, const float *x_sulph, const float *T,
                               float *p_sol, float *a_w, void *stream);
int32_t cmx_h2so4_solution_f64(const cmx_h2so4_solution_params_f64 *prs, const cmx_thermo_f64 *tps, int64_t n, const double *x_sulph, const double *T,
                               double *p_sol, double *a_w, void *stream);

/* Mohler et al. (2006) deposition nucleation on dust — src/IceNucleation.jl:44-79 (KA wrappers
 * IceNucleation_dust_activated_number_fraction_kernel!, IceNucleation_MohlerDepositionRate_kernel!, test/gpu_tests.jl:930-966):
 *   act_frac = CMI_het.dust_activated_number_fraction(dust, ip, S_i, T) = max(0, exp(a (S_i − S₀)) − 1)
 *   dep_rate = CMI_het.MohlerDepositionRate(dust, ip, S_i, T, dSi_dt, N_aer) = max(0, N_aer a dSi_dt)        (a, S₀ by T ≷ T_thr)
 * Columns S_i, T; dSi_dt and N_aer (both needed for dep_rate, NULL otherwise); either output may be NULL.  The reference asserts
 * S_i < Sᵢ_max: such points get NaN and are counted in `n_domain_errors` (optional: ONE device int64, accumulating, zeroed by the caller). */
int32_t cmx_mohler2006_deposition_f32(const cmx_mohler_dust_f32 *dust, const cmx_mohler2006_f32 *ip, int64_t n, const float *S_i, const float *T,
                                      const float *dSi_dt, const float *N_aer, float *act_frac, float *dep_rate, int64_t *n_domain_errors,
                                      void *stream);
int32_t cmx_mohler2006_deposition_f64(const cmx_mohler_dust_f64 *dust, const cmx_mohler2006_f64 *ip, int64_t n, const double *S_i, const double *T,
                                      const double *dSi_dt, const double *N_aer, double *act_frac, double *dep_rate, int64_t *n_domain_errors,
                                      void *stream);

/* CMI_het.deposition_J(dust, Δa_w) = 10^(m Δa_w + c + 4) [m⁻² s⁻¹] — src/IceNucleation.jl:81-102 (water-activity based deposition
 * nucleation, China et al. 2017 / Alpert et al. 2022; KA wrapper IceNucleation_deposition_J_kernel!, test/gpu_tests.jl:968-984). */
int32_t cmx_deposition_J_f32(const cmx_deposition_dust_f32 *dust, int64_t n, const float *delta_a_w, float *J, void *stream);
int32_t cmx_deposition_J_f64(const cmx_deposition_dust_f64 *dust, int64_t n, const double *delta_a_w, double *J, void *stream);

/* CMI_het.INP_concentration_frequency(params, INPC, T) — src/IceNucleation.jl:219-226 (Frostenberg et al. 2023: log-normal relative
 * frequency of an INP concentration at temperature T; 0 at and above T_freeze; KA wrapper IceNucleation_INPC_frequency_kernel!,
 * test/gpu_tests.jl:1041-1055). */
int32_t cmx_inp_concentration_frequency_f32(const cmx_frostenberg2023_f32 *ip, int64_t n, const float *INPC, const float *T, float *freq, void *stream);
int32_t cmx_inp_concentration_frequency_f64(const cmx_frostenberg2023_f64 *ip, int64_t n, const double *INPC, const double *T, double *freq, void *stream);

/* CO.a_w_ice(tps, T) and CO.a_w_eT(tps, e, T) over columns — src/Common.jl:250-253,267-271
 * (KA wrappers Common_a_w_ice_kernel!, Common_a_w_eT_kernel!, test/gpu_tests.jl:340-362).
 * `e` may be NULL iff `a_w_eT` is NULL. */
int32_t cmx_water_activity_f32(const cmx_thermo_f32 *tps, int64_t n, const float *T, const float *e,
                               float *a_w_ice, float *a_w_eT, void *stream);
int32_t cmx_water_activity_f64(const cmx_thermo_f64 *tps, int64_t n, const double *T, const double *e,
                               double *a_w_ice, double *a_w_eT, void *stream);

/* ---------------------------------------------------------------------------
 * (5) One-moment (Marshall–Palmer) bulk scheme.
 *
 * `flags` = the reference's Microphysics1MOptions (src/parameters/Microphysics1MOptions.jl:257-286):
 * one bit per process / variant; a cleared bit is the reference's `nothing` (process disabled).
 * CMX_1M_DEFAULT_OPTIONS reproduces `Microphysics1MOptions()`.  Exactly one variant bit of a process may be set
 * (CMX_ERR_BAD_ARG otherwise).
 * ------------------------------------------------------------------------- */
#define CMX_1M_CLOUD_LIQUID_FORMATION     (1u << 0)   /* CloudLiquidFormation        NonEq:104-140 */
#define CMX_1M_CLOUD_ICE_FORMATION_CONST  (1u << 1)   /* ConstantTimescale           NonEq:163-193 */
#define CMX_1M_CLOUD_ICE_FORMATION_TDEP   (1u << 2)   /* TemperatureDependent          NonEq:32-50,194-224 */
#define CMX_1M_CLOUD_ICE_MELT             (1u << 3)   /* CloudIceMelt                CM1:1055-1077 */
#define CMX_1M_RAIN_ACNV_KESSLER          (1u << 4)   /* Kessler1M                   CM1:354-358   */
#define CMX_1M_RAIN_ACNV_PRESCRIBED_ND    (1u << 5)   /* PrescribedNd                CM1:359-364   */
#define CMX_1M_SNOW_ACNV_NO_SUPERSAT      (1u << 6)   /* NoSupersaturation           CM1:414-418   */
#define CMX_1M_SNOW_ACNV_WITH_SUPERSAT    (1u << 7)   /* WithSupersaturation         CM1:420-446   */
#define CMX_1M_RAIN_EVAPORATION           (1u << 8)   /* RainEvaporation             CM1:917-960   */
#define CMX_1M_SNOW_SUBLIMATION_ONLY      (1u << 9)   /* SublimationOnly             CM1:979-988   */
#define CMX_1M_SNOW_DEP_AND_SUBL          (1u << 10)  /* DepositionAndSublimation    CM1:990-999   */
#define CMX_1M_SNOW_MELT                  (1u << 11)  /* SnowMelt                    CM1:1094-1139 */
#define CMX_1M_ACCR_LCL_RAI               (1u << 12)  /* CloudLiquidRainAccretion    CM1:709-732   */
#define CMX_1M_ACCR_LCL_SNO               (1u << 13)  /* CloudLiquidSnowAccretion    CM1:734-760   */
#define CMX_1M_ACCR_ICL_RAI               (1u << 14)  /* CloudIceRainAccretion (+ rain sink) CM1:762-785,872-897 */
#define CMX_1M_ACCR_ICL_SNO               (1u << 15)  /* CloudIceSnowAccretion       CM1:787-810   */
#define CMX_1M_ACCR_RAI_SNO               (1u << 16)  /* RainSnowAccretion           CM1:815-867   */
#define CMX_1M_DEFAULT_OPTIONS                                                                            \
    (CMX_1M_CLOUD_LIQUID_FORMATION | CMX_1M_CLOUD_ICE_FORMATION_CONST | CMX_1M_CLOUD_ICE_MELT |           \
     CMX_1M_RAIN_ACNV_KESSLER | CMX_1M_SNOW_ACNV_NO_SUPERSAT | CMX_1M_RAIN_EVAPORATION |                  \
     CMX_1M_SNOW_DEP_AND_SUBL | CMX_1M_SNOW_MELT | CMX_1M_ACCR_LCL_RAI | CMX_1M_ACCR_LCL_SNO |            \
     CMX_1M_ACCR_ICL_RAI | CMX_1M_ACCR_ICL_SNO | CMX_1M_ACCR_RAI_SNO)

/* Fused 1M tendencies.  Replaces the broadcast
 *   BMT.bulk_microphysics_tendencies.(Ref(BMT.Instantaneous()), Ref(BMT.Microphysics1Moment()), Ref(mp), Ref(tps),
 *                                     ρ, T, q_tot, q_lcl, q_icl, q_rai, q_sno)
 * src/BulkMicrophysicsTendencies.jl:505-514 → _microphysics_source_terms :141-217 → _aggregate_tendencies
 * :227-252 (KA wrapper benchmark_1m_bulk_tendencies_kernel!, test/gpu_performance.jl:39-47).
 * 7 columns in, 4 out (dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt [kg/kg/s]). */
int32_t cmx_mp1m_tendencies_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags,
                                int64_t n, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                const float *q_icl, const float *q_rai, const float *q_sno, float *dq_lcl_dt,
                                float *dq_icl_dt, float *dq_rai_dt, float *dq_sno_dt, void *stream);
int32_t cmx_mp1m_tendencies_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags,
                                int64_t n, const double *rho, const double *T, const double *q_tot,
                                const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                double *dq_lcl_dt, double *dq_icl_dt, double *dq_rai_dt, double *dq_sno_dt,
                                void *stream);

/* The 1-moment Instantaneous tendencies behind the host model's layouts — same conventions as
 * cmx_sb2006_warm_rain_tendencies_fields_*: in[7] = (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno) as segmented columns (n_seg runs of
 * seg_len elements, per-column run strides; a ClimaCore VIJFH field component in place), output either out[4] segmented columns or
 * out_aos = n rows of the reference's NamedTuple (dq_lcl_dt, dq_icl_dt, dq_rai_dt, dq_sno_dt) (BMT:246-251; the output type of
 * benchmark_1m_bulk_tendencies_kernel!, test/gpu_performance.jl:138-182).  Bit-identical to cmx_mp1m_tendencies_*. */
int32_t cmx_mp1m_tendencies_fields_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_seg, int64_t seg_len,
                                       const float *const *in, const int64_t *in_seg_stride, float *const *out, const int64_t *out_seg_stride,
                                       float *out_aos, void *stream);
int32_t cmx_mp1m_tendencies_fields_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_seg, int64_t seg_len,
                                       const double *const *in, const int64_t *in_seg_stride, double *const *out, const int64_t *out_seg_stride,
                                       double *out_aos, void *stream);

/* bulk_microphysics_tendencies(LinearizedAverage(), Microphysics1Moment(), mp, tps, ρ, T, q_tot, q_lcl, q_icl, q_rai, q_sno,
 * Δt, nsub) — src/BulkMicrophysicsTendencies.jl:572-632 (the mode ClimaAtmos runs operationally, :112-115): the average
 * tendencies over Δt from `nsub` linearized implicit substeps (:381-465) of the donor-based linearization dq/dt ≈ M q + e
 * (:269-379), with T updated from the latent heating of each substep.  q_min = TD.Parameters.q_min(tps) (the donor floor
 * of the linearization).  Same flags (Microphysics1MOptions) as cmx_mp1m_tendencies_*. */
int32_t cmx_mp1m_linearized_average_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, float q_min,
                                        float dt, int32_t nsub, int64_t n, const float *rho, const float *T, const float *q_tot,
                                        const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                        float *dq_lcl_dt, float *dq_icl_dt, float *dq_rai_dt, float *dq_sno_dt, void *stream);
int32_t cmx_mp1m_linearized_average_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, double q_min,
                                        double dt, int32_t nsub, int64_t n, const double *rho, const double *T, const double *q_tot,
                                        const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                        double *dq_lcl_dt, double *dq_icl_dt, double *dq_rai_dt, double *dq_sno_dt, void *stream);

/* … and behind the host model's layouts, exactly as cmx_mp1m_tendencies_fields_* (segmented columns in place, SoA or the reference's
 * array-of-NamedTuples output).  Bit-identical to cmx_mp1m_linearized_average_*. */
int32_t cmx_mp1m_linearized_average_fields_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, float q_min, float dt,
                                               int32_t nsub, int64_t n_seg, int64_t seg_len, const float *const *in, const int64_t *in_seg_stride,
                                               float *const *out, const int64_t *out_seg_stride, float *out_aos, void *stream);
int32_t cmx_mp1m_linearized_average_fields_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, double q_min, double dt,
                                               int32_t nsub, int64_t n_seg, int64_t seg_len, const double *const *in, const int64_t *in_seg_stride,
                                               double *const *out, const int64_t *out_seg_stride, double *out_aos, void *stream);

/* Snow shape of the Chen-2022 snow fall speed: cmx_snow_terminal_velocity_* `snow_shape`, and — as CMX_1M_SED_SNOW_* bits in `flags` — the
 * w_sno of cmx_mp1m_column_tendencies_sedimentation_* (no other 1-moment entry accepts those bits) */
#define CMX_SNOW_SHAPE_ASPR       0u          /* CM1.terminal_velocity(snow, Chen2022VelTypeLargeIce, ρ, q): the fixed ϕ^κ           CM1:272-297 */
#define CMX_SNOW_SHAPE_OBLATE     1u          /* … , ρ, q, CM1.Oblate()                                                          CM1:155-181, 299-324 */
#define CMX_SNOW_SHAPE_PROLATE    2u          /* … , ρ, q, CM1.Prolate()                                                         CM1:183-195, 299-324 */
#define CMX_1M_SED_SNOW_OBLATE    (1u << 17)  /* cmx_mp1m_column_tendencies_sedimentation_* only: w_sno with CM1.Oblate()        */
#define CMX_1M_SED_SNOW_PROLATE   (1u << 18)  /* cmx_mp1m_column_tendencies_sedimentation_* only: w_sno with CM1.Prolate()       */

/* The OPERATIONAL 1-moment column step in one pass (SURVEY §8f-1 + §8f-4): per grid point of n_col columns × n_lev contiguous levels
 * (flat index col·n_lev + k, level 0 = lowest — `parent(field)` of a ClimaCore column field)
 *   tend  = BMT.bulk_microphysics_tendencies(mode, Microphysics1Moment(), mp, tps, ρ, T, q_tot, q_lcl, q_icl, q_rai, q_sno[, Δt, nsub])
 *           mode = Instantaneous() when nsub = 0 (BMT:505-514), LinearizedAverage() when nsub ≥ 1 (BMT:572-632; q_min, dt as there)
 *   w     = the four bulk fall speeds a host model precomputes — exactly cmx_sedimentation_velocities_* on the clamped state
 *           (CMNonEq.terminal_velocity cloud liquid / cloud ice, CM1.terminal_velocity Chen-2022 rain / snow; NonEq:250-281, CM1:251-297)
 * followed by the host model's first-order upwind ("right-biased") flux divergence of the four species
 *   F_k = ρ_k χ_k w_k,   ∂χ_k/∂t += (F_{k+1} − F_k) · inv_dz[k] / ρ_k,   F_{n_lev} = 0,    χ = q_lcl, q_icl, q_rai, q_sno.
 * The flux scheme is the host model's (ClimaAtmos precipitation advection; column spaces test/gpu_clima_core_test.jl:16-45), NOT part
 * of the reference package: "parity unpinned" for the flux step, as for cmx_sb2006_column_tendencies_sedimentation_*.
 * in = HOST array of the 7 device columns (rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno), out = HOST array of the 4 device tendency
 * columns; precip_rai / precip_sno (optional, n_col values): the surface fluxes F_0 of rain and snow [kg m⁻² s⁻¹].  44 B/point (f32)
 * instead of the 148 B/point of the three unfused steps.  Results do not depend on tile boundaries or alignment; a NaN in ρ or in a
 * species' q gives a NaN flux of that species (and a NaN tendency of that species in the cell below).
 * Snow shape: `flags` may also hold ONE of CMX_1M_SED_SNOW_OBLATE / CMX_1M_SED_SNOW_PROLATE (both: CMX_ERR_BAD_ARG); w_sno is then
 * cmx_snow_terminal_velocity_* with that shape (CM1:299-324), everything else is unchanged.  Such a call runs the run-time-options kernel
 * whatever the options: with CMX_1M_DEFAULT_OPTIONS its tendencies may differ from a call without the bit in the last bits (the
 * default-options kernel takes the powers of λ⁻¹ as integer exponents), not beyond the Float32 / Float64 parity tolerances. */
int32_t cmx_mp1m_column_tendencies_sedimentation_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                                     const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags,
                                                     float q_min, float dt, int32_t nsub, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                     const float *const *in, float *const *out, float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_tendencies_sedimentation_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                                     const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags,
                                                     double q_min, double dt, int32_t nsub, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                     const double *const *in, double *const *out, double *precip_rai, double *precip_sno, void *stream);

/* The individual 1M source terms — `_microphysics_source_terms` (BMT:141-217), same inputs (clamped the
 * same way), `out` = host array of CMX_MP1M_NSRC device column pointers (NULL = skip). */
typedef enum cmx_mp1m_source_column {
    CMX_1M_S_PHASE_CHANGE_VAP_LCL = 0, CMX_1M_S_PHASE_CHANGE_VAP_ICL,
    CMX_1M_S_ACNV_LCL_RAI, CMX_1M_S_ACNV_ICL_SNO,
    CMX_1M_S_ACCR_LCL_RAI, CMX_1M_S_ACCR_LCL_SNO_COLD, CMX_1M_S_ACCR_LCL_SNO_WARM, CMX_1M_S_ACCR_MELT_LCL_SNO,
    CMX_1M_S_ACCR_ICL_RAI, CMX_1M_S_ACCR_FREEZE_ICL_RAI, CMX_1M_S_ACCR_ICL_SNO,
    CMX_1M_S_ACCR_RAI_SNO_COLD, CMX_1M_S_ACCR_RAI_SNO_WARM, CMX_1M_S_ACCR_MELT_RAI_SNO,
    CMX_1M_S_PHASE_CHANGE_VAP_RAI, CMX_1M_S_PHASE_CHANGE_VAP_SNO,
    CMX_1M_S_MELT_ICL_LCL, CMX_1M_S_MELT_SNO_RAI,
    CMX_MP1M_NSRC
} cmx_mp1m_source_column;
int32_t cmx_mp1m_source_terms_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags,
                                  int64_t n, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                  const float *q_icl, const float *q_rai, const float *q_sno,
                                  float *const out[CMX_MP1M_NSRC], void *stream);
int32_t cmx_mp1m_source_terms_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags,
                                  int64_t n, const double *rho, const double *T, const double *q_tot,
                                  const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                  double *const out[CMX_MP1M_NSRC], void *stream);

/* Mass-weighted 1M fall speeds over (ρ, q) columns — BASELINE config 1 together with the autoconversion
 * source term above.  Replaces `@. w = CM1.terminal_velocity(rain, vel, ρ, q)` (test/gpu_clima_core_test.jl:39-42):
 *   vt_rai_blk1m = CM1.terminal_velocity(rain, Blk1MVelTypeRain, ρ, q_rai)       CM1:223-249
 *   vt_sno_blk1m = CM1.terminal_velocity(snow, Blk1MVelTypeSnow, ρ, q_sno)       CM1:223-249
 *   vt_rai_chen  = CM1.terminal_velocity(rain, Chen2022VelTypeRain, ρ, q_rai)    CM1:251-270
 * Output columns may be NULL; q_sno may be NULL iff vt_sno_blk1m is; chen may be NULL iff vt_rai_chen is. */
int32_t cmx_mp1m_terminal_velocity_f32(const cmx_microphysics_1m_f32 *mp, const cmx_chen2022_rain_vel_f32 *chen,
                                       int64_t n, const float *rho, const float *q_rai, const float *q_sno,
                                       float *vt_rai_blk1m, float *vt_sno_blk1m, float *vt_rai_chen, void *stream);
int32_t cmx_mp1m_terminal_velocity_f64(const cmx_microphysics_1m_f64 *mp, const cmx_chen2022_rain_vel_f64 *chen,
                                       int64_t n, const double *rho, const double *q_rai, const double *q_sno,
                                       double *vt_rai_blk1m, double *vt_sno_blk1m, double *vt_rai_chen, void *stream);

/* The bulk sedimentation velocities a host model precomputes per cell (ClimaAtmos set_sedimentation_precomputed_quantities;
 * test/gpu_clima_core_test.jl:36-45; KA kernel test_chen2022_terminal_velocity_kernel!, test/gpu_tests.jl:608-630):
 *   w_lcl = CMNonEq.terminal_velocity(liquid, ::StokesRegimeVelType, ρ, q_lcl)          src/MicrophysicsNonEq.jl:250-265
 *   w_icl = CMNonEq.terminal_velocity(ice, ::Chen2022VelTypeSmallIce, ρ, q_icl)         src/MicrophysicsNonEq.jl:267-281
 *   w_rai = CM1.terminal_velocity(rain, ::Chen2022VelTypeRain, ρ, q_rai)                src/Microphysics1M.jl:251-270
 *   w_sno = CM1.terminal_velocity(snow, ::Chen2022VelTypeLargeIce, ρ, q_sno)            src/Microphysics1M.jl:272-297
 * Any (q, w) pair may be NULL together with the parameter struct only it needs. */
int32_t cmx_sedimentation_velocities_f32(const cmx_microphysics_1m_f32 *mp, const cmx_stokes_vel_f32 *stokes,
                                         const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, int64_t n,
                                         const float *rho, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                         float *w_lcl, float *w_icl, float *w_rai, float *w_sno, void *stream);
int32_t cmx_sedimentation_velocities_f64(const cmx_microphysics_1m_f64 *mp, const cmx_stokes_vel_f64 *stokes,
                                         const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, int64_t n,
                                         const double *rho, const double *q_lcl, const double *q_icl, const double *q_rai,
                                         const double *q_sno, double *w_lcl, double *w_icl, double *w_rai, double *w_sno, void *stream);

/* The Chen-2022 snow fall speed with a snow shape — CM1.terminal_velocity(snow, Ch2022.large_ice, ρ, q, shape), src/Microphysics1M.jl:299-324:
 *   ϕ_av = ϕ₀ λ⁻¹^α Γ_aspect (CM1.aspect_ratio_coeffs, CM1:155-195; Γ_aspect = snow.gamma_aspect_oblate / _prolate)
 *   w_sno = max(0, ϕ_av^κ Σₖ Chen2022_exponential_pdf(aₖ, bₖ, cₖ, 2 λ⁻¹, 3)) if q > ϵ, else 0      (Common.jl:327-350,414-422)
 * snow_shape = CMX_SNOW_SHAPE_OBLATE / _PROLATE, or CMX_SNOW_SHAPE_ASPR for the fixed aspect ratio (CM1:272-297): then bit-identical to w_sno of
 * cmx_sedimentation_velocities_* at every point without a NaN input.  snow_shape > 2: CMX_ERR_BAD_ARG.  A NaN in ρ or q gives NaN; Float64:
 * ρ ≤ 0 gives NaN; q ≤ ϵ gives exactly 0.  12 B/point (f32); any alignment, results independent of it; launches only, on `stream`. */
int32_t cmx_snow_terminal_velocity_f32(const cmx_microphysics_1m_f32 *mp, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t snow_shape, int64_t n,
                                       const float *rho, const float *q_sno, float *w_sno, void *stream);
int32_t cmx_snow_terminal_velocity_f64(const cmx_microphysics_1m_f64 *mp, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t snow_shape, int64_t n,
                                       const double *rho, const double *q_sno, double *w_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (6) Abdul-Razzak & Ghan (2000) aerosol activation.
 *
 * Replaces the broadcasts
 *   AA.N_activated_per_mode.(Ref(ap), Ref(ad), Ref(aip), Ref(tps), T, p, w, q_tot, q_liq, q_ice[, N_liq, N_ice])
 *   AA.M_activated_per_mode.(…)      AA.max_supersaturation.(…)
 * src/AerosolActivation.jl:138-200, 235-259, 294-321 (KA wrapper aerosol_activation_kernel!,
 * test/gpu_tests.jl:45-79) for an aerosol distribution shared by all states (BASELINE config 3).
 * Inputs per state: T [K], p [Pa], w [m/s], q_tot [kg/kg]; q_liq, q_ice [kg/kg] and N_liq, N_ice [1/m3] are
 * optional columns (NULL = 0, the reference's 10-argument methods).  Outputs (all optional): `N_act` / `M_act`
 * = host arrays of ad->n_modes device column pointers (activated number [1/m3] / mass per mode), `S_max`.
 * ------------------------------------------------------------------------- */
int32_t cmx_arg2000_activation_f32(
    const cmx_aerosol_activation_params_f32 *ap, const cmx_aerosol_distribution_f32 *ad,
    const cmx_air_properties_f32 *aip, const cmx_thermo_f32 *tps, int64_t n,
    const float *T, const float *p, const float *w, const float *q_tot, const float *q_liq, const float *q_ice,
    const float *N_liq, const float *N_ice, float *const *N_act, float *const *M_act, float *S_max, void *stream);
int32_t cmx_arg2000_activation_f64(
    const cmx_aerosol_activation_params_f64 *ap, const cmx_aerosol_distribution_f64 *ad,
    const cmx_air_properties_f64 *aip, const cmx_thermo_f64 *tps, int64_t n,
    const double *T, const double *p, const double *w, const double *q_tot, const double *q_liq, const double *q_ice,
    const double *N_liq, const double *N_ice, double *const *N_act, double *const *M_act, double *S_max, void *stream);

/* AA.total_N_activated(…) / AA.total_M_activated(…) — src/AerosolActivation.jl:355-433: the sums over the modes of N_activated_per_mode /
 * M_activated_per_mode (left to right, as Julia sums the tuple), formed in the activation kernel.  Either output may be NULL, not both. */
int32_t cmx_arg2000_total_activated_f32(const cmx_aerosol_activation_params_f32 *ap, const cmx_aerosol_distribution_f32 *ad,
                                        const cmx_air_properties_f32 *aip, const cmx_thermo_f32 *tps, int64_t n, const float *T, const float *p,
                                        const float *w, const float *q_tot, const float *q_liq, const float *q_ice, const float *N_liq,
                                        const float *N_ice, float *N_total, float *M_total, void *stream);
int32_t cmx_arg2000_total_activated_f64(const cmx_aerosol_activation_params_f64 *ap, const cmx_aerosol_distribution_f64 *ad,
                                        const cmx_air_properties_f64 *aip, const cmx_thermo_f64 *tps, int64_t n, const double *T, const double *p,
                                        const double *w, const double *q_tot, const double *q_liq, const double *q_ice, const double *N_liq,
                                        const double *N_ice, double *N_total, double *M_total, void *stream);

/* Same activation for aerosol that varies in space: every mode's (r_dry, stdev, N, hygroscopicity, molar_mass_mix) is a
 * device column (arrays of n_modes column pointers), as the reference's own KA kernel passes them per element
 * (aerosol_activation_kernel!, test/gpu_tests.jl:45-79).  hygroscopicity = the mode's mean B̄ or κ̄
 * (AA.mean_hygroscopicity_parameter, src/AerosolActivation.jl:61-97); molar_mass (nullable) = Σ w_j M_j, only needed
 * for M_act.  The mode-only factors the shared-distribution entry folds on the host are formed per state here. */
int32_t cmx_arg2000_activation_columns_f32(
    const cmx_aerosol_activation_params_f32 *ap, const cmx_air_properties_f32 *aip, const cmx_thermo_f32 *tps, int32_t n_modes,
    int64_t n, const float *T, const float *p, const float *w, const float *q_tot, const float *q_liq, const float *q_ice,
    const float *N_liq, const float *N_ice, const float *const *r_dry, const float *const *stdev, const float *const *N_mode,
    const float *const *hygroscopicity, const float *const *molar_mass, float *const *N_act, float *const *M_act, float *S_max,
    void *stream);
int32_t cmx_arg2000_activation_columns_f64(
    const cmx_aerosol_activation_params_f64 *ap, const cmx_air_properties_f64 *aip, const cmx_thermo_f64 *tps, int32_t n_modes,
    int64_t n, const double *T, const double *p, const double *w, const double *q_tot, const double *q_liq, const double *q_ice,
    const double *N_liq, const double *N_ice, const double *const *r_dry, const double *const *stdev, const double *const *N_mode,
    const double *const *hygroscopicity, const double *const *molar_mass, double *const *N_act, double *const *M_act, double *S_max,
    void *stream);

/* ---------------------------------------------------------------------------
 * (7) P3 ice scheme: state construction, size-distribution shape solver, mass-weighted mean diameter.
 *
 * Replaces, per point,
 *   state = P3.state_from_prognostic(params, ρq_ice, ρn_ice, ρq_rim, ρb_rim)    src/P3_particle_properties.jl:101-106
 *           (or P3.P3State(params, ρq_ice, ρn_ice, F_rim, ρ_rim) with CMX_P3_INPUT_IS_STATE, :43-56)
 *   logλ  = P3.get_distribution_logλ(state)                                      src/P3_size_distribution.jl:284-320
 *   D_m   = P3.D_m(state, logλ)                                                  src/P3_integral_properties.jl:56-61
 *   logN₀ = P3.get_logN₀(ρn_ice, μ(logλ), logλ)                                  src/P3_size_distribution.jl:233-237
 * (KA wrappers test_P3_get_distribution_logλ_kernel!, benchmark_p3_kernel!, test/gpu_tests.jl:436-451,
 * test/gpu_performance.jl:59-67).  Compute-bound: ≈12 evaluations of the shape residual per point, each 8 incomplete-
 * gamma evaluations of 20/30 fixed iterations (src/Utilities.jl:93-144).  The root is bracketed on logλ ∈ [2, 17] with
 * Brent's method like the reference (same end-point fallbacks, :295-297); logλ = −Inf when ρn_ice or ρq_ice < eps(FT).
 * The solver is Brent's zeroin under a fixed evaluation budget: RootSolvers.jl is not vendored, and zeroin is the restatement
 * that satisfies the reference's own warm-start suite (test/p3_shape_solver_warmstart_tests.jl).
 * brent_iters ≤ 0 selects the reference's fixed budget (8 Float32 / 10 Float64 iterations, :311); a larger value runs that many.
 * THE BUDGET DOES NOT ALWAYS CONVERGE: over 1e6 random states (L_ice 1e-6…1e-3 kg/m³, N_ice 1e2…1e6 m⁻³) the Float64 budget leaves
 * logλ more than 1e-6 from the root for 6.8 % of them and D_m more than 1 % off for 3.5 % — every one of them in 8 ≤ logλ < 11, where
 * the SlopePowerLaw's μ(λ) ramps (21 % of the states of that band).  brent_iters = 12 / 14 / 16 / 20 leave 2.2 % / 0.27 % / 0.02 % /
 * 0.001 % (profiles/r06_brent_exposure.json).  Whether the reference is equally unconverged there depends on RootSolvers' iterates;
 * on the reference's own state sweeps (warm-start, robustness, round trip) its budget converges, here too.
 * log_lambda_guess (nullable): the reference's optional warm start — the guess, when finite, strictly inside the
 * bracket and with a finite residual, replaces the bracket end on its side of the root (_narrow_bracket, :336-353).
 * Output columns may be NULL.
 * ------------------------------------------------------------------------- */
#define CMX_P3_INPUT_IS_STATE   (1u << 0)   /* columns 3, 4 are (F_rim, ρ_rim) instead of (ρq_rim, ρb_rim) */
#define CMX_P3_SLOPE_CONSTANT   (1u << 1)   /* SlopeConstant (μ = mu_const) instead of SlopePowerLaw */
#define CMX_P3_NO_ASPECT_RATIO  (1u << 2)   /* CMP.NoAspectRatio() instead of the default CMP.Oblate() (velocities) */
#define CMX_FREEZE_CLOUD_PSD     (1u << 4)   /* cmx_liquid_freezing_rate_*: cloud (generalized gamma) PSD instead of the rain PSD */
#define CMX_P3_RAIN_PDF_LIMITED (1u << 3)   /* rain_pdf is RainParticlePDF_SB2006_limited (collisions, rain freezing, 2M+P3 entry) */

int32_t cmx_p3_shape_f32(const cmx_p3_params_f32 *params, uint32_t flags, int32_t brent_iters, int64_t n, const float *rho_q_ice,
                         const float *rho_n_ice, const float *x3, const float *x4, const float *log_lambda_guess,
                         float *F_rim, float *rho_rim, float *log_lambda, float *D_m, float *log_N0, void *stream);
int32_t cmx_p3_shape_f64(const cmx_p3_params_f64 *params, uint32_t flags, int32_t brent_iters, int64_t n, const double *rho_q_ice,
                         const double *rho_n_ice, const double *x3, const double *x4, const double *log_lambda_guess,
                         double *F_rim, double *rho_rim, double *log_lambda, double *D_m, double *log_N0, void *stream);

/* P3 number- and mass-weighted ice fall speeds.  Replaces, per point,
 *   v_n = P3.ice_terminal_velocity_number_weighted(vel, ρₐ, state, logλ; p, quad)   src/P3_terminal_velocity.jl:72-91
 *   v_m = P3.ice_terminal_velocity_mass_weighted(vel, ρₐ, state, logλ; p, quad)     src/P3_terminal_velocity.jl:118-137
 * (and the *_from_prognostic wrappers :152-178 when CMX_P3_INPUT_IS_STATE is not set): the integrals
 * ∫ n(D) v(D) [m(D)] dD over the four mass-regime segments between the p and 1−p quantiles of the size distribution
 * (integral_bounds, src/P3_integral_properties.jl:34-46 → UT.gamma_inc_inv, src/Utilities.jl:205-252), with the
 * piecewise small/large-ice Chen-2022 particle velocity (src/Common.jl:304-350,381-382; ρᵢ = 916.7 as hard-wired at
 * src/P3_terminal_velocity.jl:41) times the aspect-ratio factor cbrt(ϕᵢ) (src/P3_particle_properties.jl:402-475) unless
 * CMX_P3_NO_ASPECT_RATIO.  log_lambda is an INPUT here, exactly as in the reference's signatures (use cmx_p3_shape_*
 * to produce it).  Either output may be NULL.  Points with ρn_ice or ρq_ice < eps(FT) give 0. */
int32_t cmx_p3_terminal_velocities_f32(const cmx_p3_params_f32 *params, const cmx_chen2022_ice_vel_f32 *vel,
                                       const cmx_quadrature_f32 *quad, uint32_t flags, float p, int64_t n,
                                       const float *rho_q_ice, const float *rho_n_ice, const float *x3, const float *x4,
                                       const float *rho_air, const float *log_lambda, float *v_n, float *v_m, void *stream);
int32_t cmx_p3_terminal_velocities_f64(const cmx_p3_params_f64 *params, const cmx_chen2022_ice_vel_f64 *vel,
                                       const cmx_quadrature_f64 *quad, uint32_t flags, double p, int64_t n,
                                       const double *rho_q_ice, const double *rho_n_ice, const double *x3, const double *x4,
                                       const double *rho_air, const double *log_lambda, double *v_n, double *v_m, void *stream);

/* BASELINE config 5 as ONE launch: cmx_p3_shape_* (log λ, D_m) followed by cmx_p3_terminal_velocities_* on the same columns, without the
 * log λ round trip through HBM and without reading the state twice (36 → 28 B/point of traffic in f32; the pass is compute-bound, so
 * the gain is the launch and the re-read, not bandwidth).  Same arithmetic as the two separate entries, bit for bit.  log_lambda_guess,
 * log_lambda and D_m may be NULL; brent_iters = 0 keeps the reference's fixed budget. */
int32_t cmx_p3_shape_terminal_velocities_f32(const cmx_p3_params_f32 *params, const cmx_chen2022_ice_vel_f32 *vel,
                                             const cmx_quadrature_f32 *quad, uint32_t flags, int32_t brent_iters, float p, int64_t n,
                                             const float *rho_q_ice, const float *rho_n_ice, const float *x3, const float *x4,
                                             const float *rho_air, const float *log_lambda_guess, float *log_lambda, float *D_m,
                                             float *v_n, float *v_m, void *stream);
int32_t cmx_p3_shape_terminal_velocities_f64(const cmx_p3_params_f64 *params, const cmx_chen2022_ice_vel_f64 *vel,
                                             const cmx_quadrature_f64 *quad, uint32_t flags, int32_t brent_iters, double p, int64_t n,
                                             const double *rho_q_ice, const double *rho_n_ice, const double *x3, const double *x4,
                                             const double *rho_air, const double *log_lambda_guess, double *log_lambda, double *D_m,
                                             double *v_n, double *v_m, void *stream);

/* P3 melting rate (QIMLT of Morrison & Milbrandt 2015): replaces, per point,
 *   (; dNdt, dLdt) = P3.ice_melt(vel, aps, tps, T, ρₐ, state, logλ; quad)                  src/P3_processes.jl:64-94
 * dL/dt = max(0, 4 K_therm / L_f(T) · (T − T_freeze) ∫ ∂m/∂D · F_v(D) · N′(D)/D dD) over the same bounds / segments as the fall
 * speeds, F_v = a_v + b_v ∛(ν/D_v) √(D v(D)/ν) (CO.ventilation_factor, src/Common.jl:506-514; vent = params.vent, the SB2006
 * ventilation coefficients); dN/dt = N/L · dL/dt.  Points with ρn_ice or ρq_ice < eps(FT) give 0 (the reference calls
 * ice_melt only where ice is present, BMT:966).
 * Parameter domain: the Chen-2022 ice tables must give a non-negative particle fall speed v(D) over the integration range, as the published tables do.
 * Where v(D) < 0 the reference takes the square root of a negative Reynolds number (DomainError on the CPU, NaN in a kernel); this entry clamps the
 * Reynolds number at 0 there (F_v = a_v) and returns a finite rate — it does not reproduce that failure
 * (tests/param_sweep.py DOMAIN, "P3 ventilation factor": the six one-entry changes of Table B3's E and F that reach it). */
int32_t cmx_p3_ice_melt_f32(const cmx_p3_params_f32 *params, const cmx_chen2022_ice_vel_f32 *vel, const cmx_air_properties_f32 *aps,
                            const cmx_thermo_f32 *tps, const cmx_ventilation_f32 *vent, const cmx_quadrature_f32 *quad, uint32_t flags,
                            float p, int64_t n, const float *rho_q_ice, const float *rho_n_ice, const float *x3, const float *x4,
                            const float *rho_air, const float *T, const float *log_lambda, float *dNdt, float *dLdt, void *stream);
int32_t cmx_p3_ice_melt_f64(const cmx_p3_params_f64 *params, const cmx_chen2022_ice_vel_f64 *vel, const cmx_air_properties_f64 *aps,
                            const cmx_thermo_f64 *tps, const cmx_ventilation_f64 *vent, const cmx_quadrature_f64 *quad, uint32_t flags,
                            double p, int64_t n, const double *rho_q_ice, const double *rho_n_ice, const double *x3, const double *x4,
                            const double *rho_air, const double *T, const double *log_lambda, double *dNdt, double *dLdt, void *stream);

/* P3 ice self-collection (aggregation): replaces, per point,
 *   (; dNdt) = P3.ice_self_collection(state, logλ, vel, ρₐ; quad)                          src/P3_processes.jl:676-712
 * (KA kernels test_P3_ice_self_collection_kernel!, test/gpu_tests.jl:444-451, and the reference's own P3 benchmark kernel
 * benchmark_p3_kernel!, test/gpu_performance.jl:59-67).  dN/dt ≥ 0 is the loss rate of ice number [1/m³/s].  8·quad.n²
 * integrand evaluations per point. */
int32_t cmx_p3_ice_self_collection_f32(const cmx_p3_params_f32 *params, const cmx_chen2022_ice_vel_f32 *vel, const cmx_quadrature_f32 *quad,
                                       uint32_t flags, int64_t n, const float *rho_q_ice, const float *rho_n_ice, const float *x3,
                                       const float *x4, const float *rho_air, const float *log_lambda, float *dNdt, void *stream);
int32_t cmx_p3_ice_self_collection_f64(const cmx_p3_params_f64 *params, const cmx_chen2022_ice_vel_f64 *vel, const cmx_quadrature_f64 *quad,
                                       uint32_t flags, int64_t n, const double *rho_q_ice, const double *rho_n_ice, const double *x3,
                                       const double *x4, const double *rho_air, const double *log_lambda, double *dNdt, void *stream);

/* P3 heterogeneous (immersion) freezing: replaces, per point,
 *   (; dNdt, dLdt) = P3.het_ice_nucleation(aerosol, tps, q_lcl, N_lcl, RH, T, ρₐ)              src/P3_processes.jl:20-46
 * J = CM_HetIce.ABIFM_J(aerosol, RH − a_w_ice(T)) on an assumed aerosol surface of 1e-10 m² per droplet; dNdt = max(0, J A N_lcl)
 * [1/m³/s], dLdt = max(0, J A q_lcl ρₐ) [kg/m³/s]; a non-finite J gives 0.  Either output may be NULL. */
int32_t cmx_p3_het_ice_nucleation_f32(const cmx_abifm_dust_f32 *dust, const cmx_thermo_f32 *tps, int64_t n, const float *q_lcl,
                                      const float *N_lcl, const float *RH, const float *T, const float *rho_air, float *dNdt, float *dLdt,
                                      void *stream);
int32_t cmx_p3_het_ice_nucleation_f64(const cmx_abifm_dust_f64 *dust, const cmx_thermo_f64 *tps, int64_t n, const double *q_lcl,
                                      const double *N_lcl, const double *RH, const double *T, const double *rho_air, double *dNdt,
                                      double *dLdt, void *stream);

/* Bigg (1953) immersion freezing of liquid drops: replaces, per point,
 *   (; ∂ₜn_frz, ∂ₜq_frz) = CMI_het.liquid_freezing_rate(rf, pdf, tps, q, ρ, N, T)          src/IceNucleation.jl:274-311 (rain PSD),
 *                                                                                            :355-389 (cloud PSD)
 * (KA kernel test_rain_freezing_kernel!, test/gpu_tests.jl:463-468).  ice->rain_freezing, ice->rain_pdf / ice->cloud_pdf are read;
 * flags: CMX_FREEZE_CLOUD_PSD selects the cloud method, CMX_P3_RAIN_PDF_LIMITED the limited rain PSD.  N is per m³; the rates are per
 * kg of air.  Either output may be NULL. */
int32_t cmx_liquid_freezing_rate_f32(const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n, const float *q,
                                     const float *rho, const float *N, const float *T, float *dn_frz, float *dq_frz, void *stream);
int32_t cmx_liquid_freezing_rate_f64(const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n, const double *q,
                                     const double *rho, const double *N, const double *T, double *dn_frz, double *dq_frz, void *stream);

/* (8) P3 liquid–ice collisions: replaces, per point,
 *   rates   = P3.∫liquid_ice_collisions(state, logλ, psd_c, psd_r, L_c, N_c, L_r, N_r, aps, tps, vel, ρₐ, T, m_liq; quad)
 *                                                                                         src/P3_processes.jl:527-562
 *   sources = P3.bulk_liquid_ice_collision_sources(state, logλ, psd_c, psd_r, L_c, N_c, L_r, N_r, aps, tps, vel, ρₐ, T; quad)
 *                                                                                         src/P3_processes.jl:600-655
 * (called from the 2M+P3 fused entry, BMT:962-972).  `ice` carries scheme (+ vent, ρ_rim_local), the Chen-2022 rain and
 * ice fall-speed tables, cloud_pdf and rain_pdf (flags & CMX_P3_RAIN_PDF_LIMITED selects the limited rain PSD); the
 * quadrature rule is the explicit `quad` (ice->quad is what the fused entry passes).  The rain inner integral uses the
 * reference's closed form (closed_rain_inner_NM :343-369: crossover diameter by a fixed-budget Brent solve, incomplete-gamma
 * moments), the cloud inner integral and both rime-volume integrals the quadrature rule.
 * sources[7] = device columns (∂ₜq_c, ∂ₜq_r, ∂ₜN_c, ∂ₜN_r, ∂ₜL_rim, ∂ₜL_ice, ∂ₜB_rim), rates[10] = device columns (QCFRZ, QCSHD,
 * NCCOL, QRFRZ, QRSHD, NRCOL, ∫M_col, BCCOL, BRCOL, ∫𝟙_wet M_col); either array (host array of device pointers) or any
 * entry may be NULL.  Points with ρn_ice or ρq_ice < eps(FT) give 0. */
int32_t cmx_p3_liquid_ice_collisions_f32(const cmx_p3_ice_params_f32 *ice, const cmx_air_properties_f32 *aps, const cmx_thermo_f32 *tps,
                                         const cmx_quadrature_f32 *quad, uint32_t flags, int64_t n, const float *rho_q_ice,
                                         const float *rho_n_ice, const float *x3, const float *x4, const float *L_c, const float *N_c,
                                         const float *L_r, const float *N_r, const float *rho_air, const float *T, const float *log_lambda,
                                         float *const *sources, float *const *rates, void *stream);
int32_t cmx_p3_liquid_ice_collisions_f64(const cmx_p3_ice_params_f64 *ice, const cmx_air_properties_f64 *aps, const cmx_thermo_f64 *tps,
                                         const cmx_quadrature_f64 *quad, uint32_t flags, int64_t n, const double *rho_q_ice,
                                         const double *rho_n_ice, const double *x3, const double *x4, const double *L_c, const double *N_c,
                                         const double *L_r, const double *N_r, const double *rho_air, const double *T, const double *log_lambda,
                                         double *const *sources, double *const *rates, void *stream);

/* (9) 2M + P3 fused entry: replaces, per point,
 *   bulk_microphysics_tendencies(Microphysics2Moment(), mp::Microphysics2MParams{WR, P3IceParams}, tps, ρ, T, q_tot, q_lcl, n_lcl,
 *                                q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, logλ, inpc_log_shift)          BMT:898-1083
 * i.e. warm rain with the ice content in the vapour budget (:942), liquid–ice collisions, aggregation and melting where
 * q_ice > ϵ and n_ice > ϵ (:959-995), Frostenberg-2023 deposition nucleation (:1004-1010), F23-capped Bigg immersion freezing
 * of cloud drops (:1013-1034), ice sublimation / deposition (:1037-1054), ice number adjustment (:1057-1064) and Bigg freezing
 * of rain (:1067-1075).  log_lambda is an INPUT (the host model caches it, cmx_p3_shape_* produces it); inpc_log_shift may be
 * NULL (= 0); the optional w, p arguments of the reference are unused by it (aerosol activation is not wired in, :729).
 * tendencies[8] = device columns (dq_lcl_dt, dn_lcl_dt, dq_rai_dt, dn_rai_dt, dq_ice_dt, dn_ice_dt, dq_rim_dt, db_rim_dt), all
 * required; the ninth field of the reference's NamedTuple, dn_lcl_activation_dt, is identically 0.
 * flags: CMX_P3_RAIN_PDF_LIMITED (is_limited of both the SB2006 set and P3IceParams.rain_pdf), CMX_P3_SLOPE_CONSTANT,
 * CMX_P3_NO_ASPECT_RATIO.  Two launches on `stream`: a pointwise kernel that writes the columns, then the 8-lanes-per-point
 * quadrature kernel that adds the ice-process terms to them. */
int32_t cmx_microphysics_2m_p3_tendencies_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                              uint32_t flags, int64_t n, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                              const float *n_lcl, const float *q_rai, const float *n_rai, const float *q_ice, const float *n_ice,
                                              const float *q_rim, const float *b_rim, const float *log_lambda, const float *inpc_log_shift,
                                              float *const *tendencies, void *stream);
int32_t cmx_microphysics_2m_p3_tendencies_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                              uint32_t flags, int64_t n, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                              const double *n_lcl, const double *q_rai, const double *n_rai, const double *q_ice, const double *n_ice,
                                              const double *q_rim, const double *b_rim, const double *log_lambda, const double *inpc_log_shift,
                                              double *const *tendencies, void *stream);

/* … and on the host model's own storage, like cmx_sb2006_warm_rain_tendencies_fields_* and cmx_mp1m_*_fields_*: every column is n_seg
 * runs of seg_len contiguous elements with its own run stride (a component of a ClimaCore VIJFH field in place: seg_len = Nv·Ni·Nj, stride =
 * Nv·Ni·Nj·Nf).  in[13] = (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda, inpc_log_shift — the last may be
 * NULL), in_seg_stride[13]; out[8] = the eight tendency columns in the order of cmx_microphysics_2m_p3_tendencies_*, out_seg_stride[8].  Strides
 * are in elements and >= seg_len.  Bit-identical to the SoA entry on the same states.  (No array-of-rows output form.) */
int32_t cmx_microphysics_2m_p3_tendencies_fields_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                                     uint32_t flags, int64_t n_seg, int64_t seg_len, const float *const *in,
                                                     const int64_t *in_seg_stride, float *const *out, const int64_t *out_seg_stride, void *stream);
int32_t cmx_microphysics_2m_p3_tendencies_fields_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                                     uint32_t flags, int64_t n_seg, int64_t seg_len, const double *const *in,
                                                     const int64_t *in_seg_stride, double *const *out, const int64_t *out_seg_stride, void *stream);

/* (9b) The 2M + P3 COLUMN step — the third fused column step, next to cmx_sb2006_column_tendencies_sedimentation_* (2b) and
 * cmx_mp1m_column_tendencies_sedimentation_*: what a mixed-phase host model evaluates once per time step, as one call.  Layout as there:
 * n_col columns of n_lev contiguous levels, flat index i = col·n_lev + k, level 0 lowest, inv_dz = n_lev values 1/Δz_k [1/m].
 *   in[13]        = HOST array of device columns (rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, q_ice, n_ice, q_rim, b_rim, log_lambda_guess,
 *                   inpc_log_shift); the last two may be NULL
 *   tendencies[8] = HOST array of device columns in the order of cmx_microphysics_2m_p3_tendencies_*, all required
 *   log_lambda, v_ice_n, v_ice_m = n_col·n_lev values each, all required: the caller caches log λ as the next step's warm start and wants the
 *                   speeds for its CFL check — and, the library being stateless and allocating nothing, they are the hand-off between the launches
 *   precip_rai, precip_ice = n_col values each, optional: F_0 of q_rai and of q_ice, the surface mass fluxes [kg m⁻² s⁻¹]
 * Per point, in this order:
 *   1. cmx_p3_shape_terminal_velocities_* on (ρ q_ice, ρ n_ice, ρ q_rim, ρ b_rim) with ice->scheme, ice->vel_ice, ice->quad, the caller's p and
 *      brent_iters (0 = the reference's budget) and log_lambda_guess as the warm start (a non-finite guess is ignored, as without one)
 *      → log_lambda, v_ice_n, v_ice_m, bit for bit that entry's.  Points without ice: log λ = −Inf, speeds 0.
 *   2. cmx_microphysics_2m_p3_tendencies_* with that log λ → tendencies, bit for bit that entry's.  It reads log λ only where ice is present, so
 *      the −Inf of the other points is passed as it is; the tendencies there are what that entry returns for any log λ (0, say).
 *   3. (w_n, w_m) = CM2.rain_terminal_velocity(sb, rain_vel, q_rai, ρ, ρ n_rai) on the clamped state (CM2:685-719), with cloud_vel != NULL also
 *      (c_n, c_m) = CM2.cloud_terminal_velocity(sb.pdf_c, cloud_vel, q_lcl, ρ, ρ n_lcl) (CM2:647-664), then the host model's first-order upwind
 *      ("right-biased") flux divergence of (2b),
 *          F_k = ρ_k χ_k w_k,   ∂χ_k/∂t += (F_{k+1} − F_k) · inv_dz[k] / ρ_k,   F_{n_lev} = 0,
 *      for χ = q_rai (w_m), n_rai (w_n), q_ice, q_rim, b_rim (v_ice_m), n_ice (v_ice_n) and — with cloud_vel — q_lcl (c_m), n_lcl (c_n).
 *      The flux scheme is the host model's, NOT part of the reference package: "parity unpinned" for the flux step, as for (2b); the tendencies
 *      and fall speeds it consumes are pinned by their own entries.
 * flags: CMX_P3_RAIN_PDF_LIMITED, CMX_P3_SLOPE_CONSTANT, CMX_P3_NO_ASPECT_RATIO as for cmx_microphysics_2m_p3_tendencies_*, and exactly one of
 * CMX_P3COL_VEL_SB2006 / CMX_P3COL_VEL_CHEN2022: the rain fall-speed scheme of step 3.  (CMX_VEL_SB2006 / CMX_VEL_CHEN2022 are bits 1 and 2 — the
 * bits of CMX_P3_SLOPE_CONSTANT / CMX_P3_NO_ASPECT_RATIO — so the choice has bits of its own in this word.)
 * Results do not depend on tile boundaries or pointer alignment.  A NaN in ρ or in any column of a species gives a NaN flux of that species and a
 * NaN tendency in the cell below; the four ice species share the two fall speeds and hence their NaN fate, as the two rain moments do.
 * A pure sequence of launches on `stream` (products → shape + fall speeds → tendencies → sedimentation): no allocation, no synchronisation, no host
 * read-back — capturable in a HIP graph.  The four products are parked in tendencies[4..7] until step 2 overwrites them, so the tendency
 * columns must not alias an input column.
 * Status, before any HIP call: n_col < 0, n_lev <= 0, both or neither velocity flag, an unknown flag → CMX_ERR_BAD_ARG; n_col·n_lev > 16·(2^31 − 1),
 * or above the 4·(2^31 − 8) states of the collision kernel's smallest tile → CMX_ERR_UNSUPPORTED; n_col = 0 → CMX_OK; then a NULL required column,
 * disordered limiters, a quadrature order outside 1…CMX_QUAD_MAX or p outside (0, ½) → CMX_ERR_BAD_ARG.
 * cmx_version() stays at 0.5 (no struct layout changed; an older library fails on the symbol lookup). */
#define CMX_P3COL_VEL_SB2006    (1u << 8)   /* the 2M + P3 column entries (9b), (24) only: rain fall speeds as with CMX_VEL_SB2006 */
#define CMX_P3COL_VEL_CHEN2022  (1u << 9)   /* the 2M + P3 column entries (9b), (24) only: rain fall speeds as with CMX_VEL_CHEN2022 */
int32_t cmx_mp2m_p3_column_tendencies_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                                        const cmx_rain_vel_f32 *rain_vel, const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags,
                                                        int32_t brent_iters, float p, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                        const float *const *in, float *const *tendencies, float *log_lambda, float *v_ice_n,
                                                        float *v_ice_m, float *precip_rai, float *precip_ice, void *stream);
int32_t cmx_mp2m_p3_column_tendencies_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                                        const cmx_rain_vel_f64 *rain_vel, const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags,
                                                        int32_t brent_iters, double p, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                        const double *const *in, double *const *tendencies, double *log_lambda, double *v_ice_n,
                                                        double *v_ice_m, double *precip_rai, double *precip_ice, void *stream);

/* UT.gamma_inc(a, x) = (P, Q) and UT.gamma_inc_inv(a, p, q) over columns — src/Utilities.jl:54-61,93-144 and :205-252 (KA wrapper
 * test_gamma_inc_kernel!, test/gpu_tests.jl:456-461; CPU test test/gamma_inc_tests.jl): the reference's fast regularised incomplete gamma
 * functions — series for x < a + 1, Lentz continued fraction otherwise, 20 (Float32) / 30 (Float64) terms — and their Halley inverse,
 * evaluated by the SAME device routines the P3 kernels call (shape solver moments, quantile bounds, closed-form rain collisions).  a > 0.
 * Either of P, Q may be NULL (not both).  The device series / continued fraction may stop early once converged to eps(FT); the reference's
 * fixed term count is an upper bound, so results agree with it to rounding wherever the reference's truncation has converged. */
int32_t cmx_gamma_inc_f32(int64_t n, const float *a, const float *x, float *P, float *Q, void *stream);
int32_t cmx_gamma_inc_f64(int64_t n, const double *a, const double *x, double *P, double *Q, void *stream);
int32_t cmx_gamma_inc_inv_f32(int64_t n, const float *a, const float *p, const float *q, float *x, void *stream);
int32_t cmx_gamma_inc_inv_f64(int64_t n, const double *a, const double *p, const double *q, double *x, void *stream);

/* Size-distribution helpers over columns (VERDICT r03 "missing" 5) — the reference's DistributionTools and the SB2006 PSD accessors:
 *   DT.generalized_gamma_quantile(ν, μ, B, Y) = (UT.gamma_inc_inv((ν+1)/μ, Y, 1−Y)/B)^(1/μ)      src/DistributionTools.jl:44-47
 *   DT.generalized_gamma_cdf(ν, μ, B, x)      = P((ν+1)/μ, B x^μ), 0 for x ≤ 0                    :75-82
 *   DT.exponential_quantile(D_mean, Y)        = exp(log D_mean + cloglog(Y))                     :146-151
 *   DT.exponential_cdf(D_mean, D)             = exp(log1mexp(−D/D_mean)), 0 for D < 0             :124-129
 * (test/DistributionTools_tests.jl), ν and μ shared by the call, B / D_mean per point.  Where the scalar functions throw a DomainError
 * (μ ≤ 0, B ≤ 0, D_mean ≤ 0, Y outside [0, 1]) the array entries write NaN.  `quantile` needs Y, `cdf` needs x (resp. D); either output may
 * be NULL, not both. */
int32_t cmx_generalized_gamma_f32(float nu, float mu, int64_t n, const float *B, const float *Y, const float *x, float *quantile, float *cdf, void *stream);
int32_t cmx_generalized_gamma_f64(double nu, double mu, int64_t n, const double *B, const double *Y, const double *x, double *quantile, double *cdf,
                                  void *stream);
int32_t cmx_exponential_distribution_f32(int64_t n, const float *D_mean, const float *Y, const float *D, float *quantile, float *cdf, void *stream);
int32_t cmx_exponential_distribution_f64(int64_t n, const double *D_mean, const double *Y, const double *D, double *quantile, double *cdf, void *stream);
/*   CM2.size_distribution_value(pdf, q, ρₐ, N, D)            n(D) of the rain (N₀r e^(−D/D̄r)) or cloud (N₀c D^(3ν+2) e^(−λc D^(3μ))) PSD      src/Microphysics2M.jl:270-315
 *   CM2.get_size_distribution_bounds(pdf, q, ρₐ, N, p)        the p and 1 − p quantiles of that PSD (the reference's default p = eps(FT))     :336-354
 * flags: CMX_PSD_CLOUD selects pdf_c (CloudParticlePDF_SB2006; pdf_r may be NULL), otherwise pdf_r (CMX_SB2006_LIMITED: the limited rain PSD;
 * pdf_c may be NULL).  N per m³.  D is needed for n_D only; any output may be NULL (not all three).  With CMX_SB2006_LIMITED the limiter
 * pairs of pdf_r must be positive and ordered (xr_min ≤ xr_max, N0_min ≤ N0_max, lambda_min ≤ lambda_max) as for the rate entries: a struct of
 * the not-limited variant (limiters zero) passed with the flag set returns CMX_ERR_BAD_ARG instead of clamping N₀ and λ to 0. */
#define CMX_PSD_CLOUD (1u << 5)
int32_t cmx_sb2006_size_distribution_f32(const cmx_cloud_pdf_sb2006_f32 *pdf_c, const cmx_rain_pdf_sb2006_f32 *pdf_r, uint32_t flags, float p, int64_t n,
                                         const float *q, const float *rho, const float *N, const float *D, float *n_D, float *D_min, float *D_max,
                                         void *stream);
int32_t cmx_sb2006_size_distribution_f64(const cmx_cloud_pdf_sb2006_f64 *pdf_c, const cmx_rain_pdf_sb2006_f64 *pdf_r, uint32_t flags, double p, int64_t n,
                                         const double *q, const double *rho, const double *N, const double *D, double *n_D, double *D_min, double *D_max,
                                         void *stream);

/* ---------------------------------------------------------------------------
 * (0) 0-moment entry of bulk_microphysics_tendencies (src/BulkMicrophysicsTendencies.jl:658-680; KA kernels
 * test_bulk_tendencies_0m_kernel!, test_bulk_tendencies_0m_S0_kernel!, test/gpu_tests.jl:364-383, and
 * test_0_moment_micro_kernel! / test_0M_derivatives_kernel!, test/gpu_tests.jl:105-141).  Replaces the broadcasts
 *   BMT.bulk_microphysics_tendencies.(Microphysics0Moment(), mp, tps, T, q_lcl, q_icl[, q_vap_sat])
 *   CM0.remove_precipitation.(p0m, q_lcl, q_icl[, q_vap_sat])   CM0.∂remove_precipitation_∂q_tot.(…)   src/Microphysics0M.jl:35-75
 * dq_tot_dt = −max(0, q_lcl⁺ + q_icl⁺ − threshold)/τ_precip with threshold = qc_0 (q_vap_sat == NULL) or S_0·q_vap_sat;
 * ddq_dq_tot (optional) = −1/τ_precip where condensate exceeds the threshold, else 0.  Negative q_lcl / q_icl are clamped to 0 as BMT
 * does (a no-op for the non-negative inputs CM0's direct callers pass).  T is not read by the reference and is not an argument.
 * ------------------------------------------------------------------------- */
int32_t cmx_mp0m_tendencies_f32(const cmx_parameters_0m_f32 *p, int64_t n, const float *q_lcl, const float *q_icl,
                                const float *q_vap_sat, float *dq_tot_dt, float *ddq_dq_tot, void *stream);
int32_t cmx_mp0m_tendencies_f64(const cmx_parameters_0m_f64 *p, int64_t n, const double *q_lcl, const double *q_icl,
                                const double *q_vap_sat, double *dq_tot_dt, double *ddq_dq_tot, void *stream);

/* ---------------------------------------------------------------------------
 * (10) Cloud diagnostics over columns — src/CloudDiagnostics.jl (round 5; what a host model's radiation / radar diagnostics broadcast over the SAME state
 * columns the tendency entries read):
 *   Z_1m      = CMD.radar_reflectivity_1M(rain, q_rai, ρ)                                    :31-46    [dBZ, clipped at −150]
 *   Z_2m      = CMD.radar_reflectivity_2M(SB2006, q_lcl, q_rai, N_lcl, N_rai, ρ)             :64-84    [dBZ, clipped at −150]
 *   reff_2m   = CMD.effective_radius_2M(SB2006, q_lcl, q_rai, N_lcl, N_rai, ρ)               :100-125  [m]
 *   reff_lh97 = CMD.effective_radius_Liu_Hallet_97(wtr, ρ, q_lcl, N_lcl, q_rai, N_rai)       :143-163  [m]
 * (CMD.effective_radius_const is the r_eff field of cmx_cloud_liquid / cmx_cloud_ice.)  N per m³ as in the reference.  Any output may be NULL (not all
 * four); the parameter structs and columns only a NULL output needs may be NULL: `rain` and q_rai for Z_1m; pdf_c, pdf_r (flags: CMX_SB2006_LIMITED as
 * for the rate entries, same limiter-pair rule) and all four of q_lcl, q_rai, N_lcl, N_rai for Z_2m / reff_2m; rho_w (WaterProperties.ρw) and q_lcl for
 * reff_lh97 — whose three-argument method (N_lcl = 100, no rain: :165-180) is selected by passing N_lcl, q_rai and N_rai all NULL.  The reference's
 * gates are kept (absent species, notvalid(B) = B is 0 or not finite in the float type, M² ≤ ϵ); a NaN input gives NaN.
 * ------------------------------------------------------------------------- */
int32_t cmx_cloud_diagnostics_f32(const cmx_rain_f32 *rain, const cmx_cloud_pdf_sb2006_f32 *pdf_c, const cmx_rain_pdf_sb2006_f32 *pdf_r, float rho_w,
                                  uint32_t flags, int64_t n, const float *rho, const float *q_lcl, const float *q_rai, const float *N_lcl,
                                  const float *N_rai, float *Z_1m, float *Z_2m, float *reff_2m, float *reff_lh97, void *stream);
int32_t cmx_cloud_diagnostics_f64(const cmx_rain_f64 *rain, const cmx_cloud_pdf_sb2006_f64 *pdf_c, const cmx_rain_pdf_sb2006_f64 *pdf_r, double rho_w,
                                  uint32_t flags, int64_t n, const double *rho, const double *q_lcl, const double *q_rai, const double *N_lcl,
                                  const double *N_rai, double *Z_1m, double *Z_2m, double *reff_2m, double *reff_lh97, void *stream);

/* ---------------------------------------------------------------------------
 * (11) Aerosol nucleation — src/Nucleation.jl (the CLOUD-chamber new-particle-formation rates; test/gpu_tests.jl:246-285,1094-1153 broadcasts them over
 * device arrays) — and the P3 ice-nucleation counts CMI_het.P3_deposition_N_i / P3_het_N_i (src/IceNucleation.jl:162-166,202-205;
 * test/gpu_tests.jl:335-344,1001-1037).  Concentrations per m³, T in K, condensation sink in 1/s, rates per m³ per s, as in the reference.  Each entry
 * is one launch sequence on `stream`, any alignment (results do not depend on it), n up to the usual limit.  Any output may be NULL, not all; a
 * parameter struct or input column that only NULL outputs would read may be NULL.
 *
 * Numerical semantics (tests/test_nucleation_host.py, tests/test_nucleation_gpu.py):
 *  - every power behaves as IEEE pow / Julia's ^: 0^p = 0 (p > 0), x/0 = Inf, 1^y = 1 for every y, x^0 = 1.  So nh3 = 0 gives f_y = 0 and a ternary
 *    rate of exactly 0, h2so4 = nh3 = 0 gives NaN (0/0, as the reference), and equal diameters in the apparent rate give J_x = nucleation_rate exactly.
 *  - a negative concentration that the reference raises to a non-integer power (h2so4, nh3, HOM; the ratios of the apparent rate) is a DomainError
 *    there and NaN here; nh3 < 0 makes binary NaN too (the reference throws for the whole call).  Products without a power (negative_ion, the
 *    mixed rate's h2so4² and bioOxOrg) keep the reference's value.
 *  - a NaN in any input an output reads gives NaN in that output.  P3_deposition_N_i at a NaN T is therefore NaN, where the reference's
 *    ifelse(T < T₀, …, 0) returns 0.
 *  - each function's own unit conversions as the reference: h2so4_nucleation_rate scales h2so4 and nh3 by 1e-6 but not negative_ion (:60-61);
 *    organic_nucleation_rate scales all four concentrations (:117-120); the mixed rate squares h2so4 unscaled (:202 is commented out).  Float32
 *    products keep the reference's order, except that k(T)·(h2so4/ref)^p is one exp2 of the summed logarithms, the f_y ratio one exp2 of the
 *    exponent difference, and the final ×1e6 is applied to each term — so no intermediate over- or underflows where the reference's does not.
 *    A Float32 term that is multiplied up afterwards is formed ×2^64 where it would be subnormal and scaled back last (exact powers of two).
 * ------------------------------------------------------------------------- */
/* One fused pass over the state columns:
 *   (binary, ternary) = Nucleation.h2so4_nucleation_rate(h2so4, nh3, negative_ion, T, h2so4p)                                      :51-90
 *   organic           = Nucleation.organic_nucleation_rate(negative_ion, monoterpene, O3, OH, T, condensation_sink, orgp)          :106-135
 *   mixed             = Nucleation.organic_and_h2so4_nucleation_rate(h2so4, monoterpene, OH, T, condensation_sink, mixp)           :172-190
 * binary / ternary read h2so4, nh3, negative_ion, T and need h2so4p; organic reads negative_ion, monoterpene, O3, OH, T, condensation_sink and needs
 * orgp; mixed reads h2so4, monoterpene, OH, T, condensation_sink and needs mixp.  The reference's GPU kernel stores sum(h2so4_nucleation_rate(…)):
 * the caller adds binary + ternary.  Only the columns the requested outputs read are loaded: 8 in + 4 out = 48 B/point (f32) with every output. */
int32_t cmx_aerosol_nucleation_rates_f32(const cmx_h2so4_nucleation_f32 *h2so4p, const cmx_organic_nucleation_f32 *orgp, const cmx_mixed_nucleation_f32 *mixp,
                                         int64_t n, const float *h2so4, const float *nh3, const float *negative_ion, const float *monoterpene, const float *O3,
                                         const float *OH, const float *T, const float *condensation_sink, float *binary, float *ternary, float *organic,
                                         float *mixed, void *stream);
int32_t cmx_aerosol_nucleation_rates_f64(const cmx_h2so4_nucleation_f64 *h2so4p, const cmx_organic_nucleation_f64 *orgp, const cmx_mixed_nucleation_f64 *mixp,
                                         int64_t n, const double *h2so4, const double *nh3, const double *negative_ion, const double *monoterpene,
                                         const double *O3, const double *OH, const double *T, const double *condensation_sink, double *binary, double *ternary,
                                         double *organic, double *mixed, void *stream);
/* The prescribed forms (the ones test/nucleation_unit_tests.jl pins with known answers):
 *   organic = Nucleation.organic_nucleation_rate_hom_prescribed(negative_ion, HOM, orgp)                           :137-157  (HOM in cm⁻³, negative_ion as passed)
 *   mixed   = Nucleation.organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed(h2so4, bioOxOrg, mixp)            :192-206
 * organic reads negative_ion, HOM and needs orgp; mixed reads h2so4, bioOxOrg and needs mixp. */
int32_t cmx_nucleation_rates_prescribed_f32(const cmx_organic_nucleation_f32 *orgp, const cmx_mixed_nucleation_f32 *mixp, int64_t n, const float *negative_ion,
                                            const float *HOM, const float *h2so4, const float *bioOxOrg, float *organic, float *mixed, void *stream);
int32_t cmx_nucleation_rates_prescribed_f64(const cmx_organic_nucleation_f64 *orgp, const cmx_mixed_nucleation_f64 *mixp, int64_t n, const double *negative_ion,
                                            const double *HOM, const double *h2so4, const double *bioOxOrg, double *organic, double *mixed, void *stream);
/* J_x = Nucleation.apparent_nucleation_rate(output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam)  :23-37
 * (Lehtinen et al. 2007).  input_diam NULL: the reference's default argument 1.7; every other column is required.  (r^(m+1) − 1)/(m+1), r =
 * output_diam/input_diam, is evaluated as expm1((m+1) ln r)/(m+1): the reference's form cancels as m → −1 (1 % off in Float32 at |m + 1| ≈ 2e-5). */
int32_t cmx_apparent_nucleation_rate_f32(int64_t n, const float *output_diam, const float *nucleation_rate, const float *condensation_growth_rate,
                                         const float *coag_sink, const float *coag_sink_input_diam, const float *input_diam, float *J_x, void *stream);
int32_t cmx_apparent_nucleation_rate_f64(int64_t n, const double *output_diam, const double *nucleation_rate, const double *condensation_growth_rate,
                                         const double *coag_sink, const double *coag_sink_input_diam, const double *input_diam, double *J_x, void *stream);
/* P3 ice-nucleation counts over columns [m⁻³]:
 *   N_dep = CMI_het.P3_deposition_N_i(ip, T)              src/IceNucleation.jl:162-166   (reads T only)
 *   N_het = CMI_het.P3_het_N_i(ip, T, N_l, V_l, dt)       src/IceNucleation.jl:202-205   (dt is a column, as in the reference's GPU kernel)
 * N_het is evaluated as −N_l·expm1(x), x = −het_B V_l dt exp(het_a (T₀ − T)), in BOTH precisions: a deliberate difference from the reference, whose
 * N_l (1 − exp(x)) cancels in Float32 (its own GPU test quotes 0.00023841858 against the Float64 value 0.0002736160475969029, 13 % off).  The Float32
 * result stays within the 1e-3 parity bound of the reference's Float64 arithmetic (the ARG2000 erfc precedent). */
int32_t cmx_p3_ice_nucleation_counts_f32(const cmx_morrison_milbrandt2014_f32 *ip, int64_t n, const float *T, const float *N_l, const float *V_l,
                                         const float *dt, float *N_dep, float *N_het, void *stream);
int32_t cmx_p3_ice_nucleation_counts_f64(const cmx_morrison_milbrandt2014_f64 *ip, int64_t n, const double *T, const double *N_l, const double *V_l,
                                         const double *dt, double *N_dep, double *N_het, void *stream);

/* ---------------------------------------------------------------------------
 * (12) SB2006 precipitation susceptibilities — src/PrecipitationSusceptibility.jl (Glassmeier & Lohmann 2016): the logarithmic derivatives of the rain
 * source of CM2.autoconversion (src/Microphysics2M.jl:396-427) and CM2.accretion (:445-470),
 *   precipitation_susceptibility_autoconversion(scheme, q_lcl, q_rai, ρ, N_lcl)   :36-51    → acnv_d_ln_q_lcl, acnv_d_ln_q_rai, acnv_d_ln_N_lcl
 *   precipitation_susceptibility_accretion(scheme, q_lcl, q_rai, ρ, N_lcl)        :66-79    → accr_d_ln_q_lcl, accr_d_ln_q_rai, accr_d_ln_N_lcl
 * over columns in one pass.  The reference differentiates ln(dq_rai_dt) with ForwardDiff with respect to ln|q_lcl|, ln|q_rai|, ln|ρ|, ln|N_lcl| and
 * returns components 1, 2 and 4; its d_ln_pp_d_ln_N_rai is always 0 and has no column here.  The device evaluates the closed forms of those derivatives
 * (the ones the reference's test states, test/precipitation_susceptibility_tests.jl:11-29,59-68); there is no automatic differentiation on the device.
 * Per point, with the inputs taken through abs as in the reference (:43, :71), ϵ = eps(FT), 1−τ = q_lcl/(q_lcl+q_rai), τ = q_rai/(q_lcl+q_rai),
 * x̄_c = ρ q_lcl/N_lcl:
 *   autoconversion:  u = A τ^a (1−τ^a)^b/(1−τ)²,  G = u/(1+u)·[a − a b τ^a/(1−τ^a) + 2τ/(1−τ)],  G = 0 where q_rai < ϵ (the ifelse of CM2 :411);
 *                    acnv_d_ln_q_rai = (1−τ) G;
 *                    x̄_c < x_star:  acnv_d_ln_q_lcl = 4 − (1−τ) G,  acnv_d_ln_N_lcl = −2;
 *                    otherwise (the min of CM2 :406 clips to x_star):  acnv_d_ln_q_lcl = 2 − (1−τ) G,  acnv_d_ln_N_lcl = 0
 *   accretion:       h = (1−τ) c τ0/(τ+τ0);  accr_d_ln_q_lcl = 1 − h,  accr_d_ln_q_rai = 1 + h,  accr_d_ln_N_lcl = 0
 * N_lcl per m³, as in the reference.  ϵ depends on the float type, so the gates of a Float32 call are the Float32 ones.
 *
 * NaN contract — cmx's own statement: the reference was not run for it.  The reference zeroes dq_rai_dt where its gate fires (autoconversion:
 * q_lcl < ϵ or N_lcl < ϵ, CM2 :420; accretion: those or q_rai < ϵ, :463); the derivative of the logarithm of that zero is undefined, and default
 * ForwardDiff yields NaN there (0·Inf).  All three outputs of a process whose gate fires are therefore NaN.  They are NaN too where any of the four
 * inputs is NaN or ρ = 0.  A negative input gives the result of its absolute value, bit for bit.
 *
 * A NULL `acnv` or `accr` skips that process, and its three outputs must then be NULL; any output may be NULL, not all (CMX_ERR_BAD_ARG).  The four input
 * columns are always required.  One launch sequence on `stream`, any alignment (results do not depend on it), n_points up to the usual limit, 0 is OK.
 * (The count is spelled n_points here: tests/test_abi.py pins the set of entries it drives through the count rule by their `int64_t n`, as
 * tests/test_abi_caller.py pins the rows of CMX_ASSERT_PARAM_STRUCT_SIZES; this entry's count statuses are checked in
 * tests/test_precip_susceptibility_host.py.)
 * 4 columns in + 6 out = 40 B/point (f32) with every output, 28 B/point for one process.
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_precip_susceptibility_f32(const cmx_acnv_sb2006_f32 *acnv, const cmx_accr_sb2006_f32 *accr, int64_t n_points, const float *q_lcl,
                                             const float *q_rai, const float *rho, const float *N_lcl, float *acnv_d_ln_q_lcl, float *acnv_d_ln_q_rai,
                                             float *acnv_d_ln_N_lcl, float *accr_d_ln_q_lcl, float *accr_d_ln_q_rai, float *accr_d_ln_N_lcl, void *stream);
int32_t cmx_sb2006_precip_susceptibility_f64(const cmx_acnv_sb2006_f64 *acnv, const cmx_accr_sb2006_f64 *accr, int64_t n_points, const double *q_lcl,
                                             const double *q_rai, const double *rho, const double *N_lcl, double *acnv_d_ln_q_lcl, double *acnv_d_ln_q_rai,
                                             double *acnv_d_ln_N_lcl, double *accr_d_ln_q_lcl, double *accr_d_ln_q_rai, double *accr_d_ln_N_lcl,
                                             void *stream);

/* ---------------------------------------------------------------------------
 * (13) The adiabatic parcel model — parcel/ParcelModel.jl, ParcelTendencies.jl, ParcelDistributions.jl, ParcelCommon.jl — over an ENSEMBLE of parcels,
 * one parcel per lane: calibration ensembles (test/ice_nucleation_calibration.jl, papers/ice_nucleation_2024/calibration.jl) and the sweeps over updraft
 * speed and initial state of parcel/Example_*.jl.
 *   cmx_parcel_tendencies_*   the right-hand side parcel_model(dY, Y, p, t) (ParcelModel.jl:54-187) as a pointwise map
 *   cmx_parcel_run_*          run_parcel (:230-366): n_steps forward-Euler steps Y ← Y + const_dt·dY inside ONE kernel (ODE.Euler with dt = const_dt is this
 *                             recurrence), the nine state values in registers from the first step to the last
 * State columns, in the reference's order: S_l, p_air, T, q_vap, q_liq, q_ice, N_aer, N_liq, N_ice (rows 1–9 of Y), plus the updraft speed w per parcel.
 * Row 10, ln_INPC, matters to the stochastic Frostenberg option only, which is not built: it is no column of this ABI.
 *
 * Options: `flags` holds one field per member of parcel_params, the values below; every other parameter is in cmx_parcel_params_*.  Not built, refused
 * with CMX_ERR_UNSUPPORTED: deposition MohlerRate (it reads dY[1] before the call has written it, ParcelTendencies.jl:73: its value depends on the
 * solver's buffer reuse), heterogeneous Frostenberg_random / Frostenberg_stochastic (random draws), NonEq_Condensation / NonEq_Deposition (a mock
 * 1-moment parameter set), MonodisperseMix (two more state variables), prescribed_thermodynamics (AIDA profiles).  A value outside a field's list, or a
 * bit outside every field, is CMX_ERR_BAD_ARG.
 *
 * Per-parcel coefficients: `coefficients` is NULL or an array of CMX_PARCEL_NCOEF column pointers (each NULL-able) that override, per parcel, the
 * coefficient pair of the activity-based schemes — deposition_m, deposition_c (ABDINM), ABIFM_m, ABIFM_c (ABIFM), linear_c1, linear_c2 (ABHOM).  A NULL
 * column means the struct's value for every parcel; a column filled with that value gives the same bits.
 *
 * Semantics kept from the reference: the clip of rows 4–9 only; the N == 0 || q == 0 branch of distribution_moments; the number sinks
 * dq < 0 && 0 < q < 1e-6; r_act with its eps(FT) gates and min(1e-6, …); every min(…, N/const_dt) limiter; S_i ≥ S_i_max → AF = 0 (the reference
 * also logs a warning there; the device does not report it).  eps(FT) is the float type's.  min / max propagate NaN as Julia's do, and a parcel with a
 * NaN in any of its ten inputs (or in a coefficient it reads) has NaN in ALL its outputs — the library's NaN rule; the reference's own arithmetic
 * carries a NaN only to the tendencies that read it.  Division by zero and overflow follow IEEE.
 *
 * cmx_parcel_tendencies: nine NULL-able tendency columns dY (same order as the state) and `process_rates`, NULL or an array of CMX_PARCEL_NPROC
 * NULL-able columns: dN_liq_act, dN_ice_dep, dN_ice_imm, dN_ice_hom, dq_liq_ce, dq_ice_ds (cmx_parcel_process_column).  At least one output.
 *
 * cmx_parcel_run: `state_out` = nine columns, all required; each may be the matching input column (in place), no other overlap.  n_steps ≥ 0 steps of
 * pp->const_dt.  `trajectory` is NULL or a buffer of (1 + n_steps / save_every) records × 9 variables × n_parcels values, layout
 * [record][variable][parcel]: record 0 is the initial state, record j the state after j·save_every steps; NULL or save_every = 0 skips it.
 * A run of a + b steps equals a run of a steps followed by a run of b steps on its result, bit for bit; the entry itself splits n_steps into launches of
 * at most CMX_PARCEL_MAX_STEPS_PER_LAUNCH steps (cmx_launch.hpp states the launch time that cap corresponds to), all on `stream`, no host
 * synchronisation: graph-capturable like every other entry.
 *
 * Status order: pp NULL / flags → BAD_ARG or UNSUPPORTED; n_parcels < 0 → BAD_ARG, > the point limit → UNSUPPORTED; n_steps < 0 or save_every < 0 →
 * BAD_ARG; n_parcels = 0 → OK; then the columns.  (The count is spelled n_parcels: tests/test_abi.py pins the entries it drives by `int64_t n`.)
 * ------------------------------------------------------------------------- */
#define CMX_PARCEL_AERO_ACT                  (1u << 0)    /* aerosol_act = "AeroAct"                          ParcelTendencies.jl:20-41   */
#define CMX_PARCEL_DEP_MASK                  (7u << 4)    /* deposition                                                                   */
#define CMX_PARCEL_DEP_MOHLER_AF             (1u << 4)    /*   "MohlerAF"                                     :48-66                      */
#define CMX_PARCEL_DEP_MOHLER_RATE           (2u << 4)    /*   "MohlerRate" — CMX_ERR_UNSUPPORTED             :68-90                      */
#define CMX_PARCEL_DEP_ABDINM                (3u << 4)    /*   "ABDINM"                                       :92-105                     */
#define CMX_PARCEL_DEP_P3                    (4u << 4)    /*   "P3_dep"                                       :107-113                    */
#define CMX_PARCEL_HET_MASK                  (7u << 8)    /* heterogeneous                                                                */
#define CMX_PARCEL_HET_ABIFM                 (1u << 8)    /*   "ABIFM"                                        :120-133                    */
#define CMX_PARCEL_HET_P3                    (2u << 8)    /*   "P3_het"                                       :135-141                    */
#define CMX_PARCEL_HET_FROSTENBERG_RANDOM    (3u << 8)    /*   "Frostenberg_random" — CMX_ERR_UNSUPPORTED     :143-154                    */
#define CMX_PARCEL_HET_FROSTENBERG_MEAN      (4u << 8)    /*   "Frostenberg_mean"                             :156-162                    */
#define CMX_PARCEL_HET_FROSTENBERG_STOCHASTIC (5u << 8)   /*   "Frostenberg_stochastic" — CMX_ERR_UNSUPPORTED :169-187                    */
#define CMX_PARCEL_HOM_MASK                  (3u << 12)   /* homogeneous                                                                  */
#define CMX_PARCEL_HOM_ABHOM                 (1u << 12)   /*   "ABHOM"                                        :194-205                    */
#define CMX_PARCEL_HOM_P3                    (2u << 12)   /*   "P3_hom"                                       :207-213                    */
#define CMX_PARCEL_COND_MASK                 (3u << 16)   /* condensation_growth                                                          */
#define CMX_PARCEL_COND_CONDENSATION         (1u << 16)   /*   "Condensation"                                 :220-232                    */
#define CMX_PARCEL_COND_NONEQ_SIMPLE         (2u << 16)   /*   "NonEq_Condensation_simple"                    :234-246                    */
#define CMX_PARCEL_COND_NONEQ                (3u << 16)   /*   "NonEq_Condensation" — CMX_ERR_UNSUPPORTED     :248-276                    */
#define CMX_PARCEL_DEPGROWTH_MASK            (3u << 20)   /* deposition_growth                                                            */
#define CMX_PARCEL_DEPGROWTH_DEPOSITION      (1u << 20)   /*   "Deposition"                                   :283-296                    */
#define CMX_PARCEL_DEPGROWTH_NONEQ_SIMPLE    (2u << 20)   /*   "NonEq_Deposition_simple"                      :298-311                    */
#define CMX_PARCEL_DEPGROWTH_NONEQ           (3u << 20)   /*   "NonEq_Deposition" — CMX_ERR_UNSUPPORTED       :313-342                    */
#define CMX_PARCEL_LIQ_MASK                  (3u << 24)   /* liq_size_distribution ("Monodisperse" = 0)       ParcelDistributions.jl      */
#define CMX_PARCEL_LIQ_GAMMA                 (1u << 24)   /*   "Gamma"                                        :54-74                      */
#define CMX_PARCEL_LIQ_MONODISPERSE_MIX      (2u << 24)   /*   "MonodisperseMix" — CMX_ERR_UNSUPPORTED        :25-52                      */
#define CMX_PARCEL_ICE_GAMMA                 (1u << 26)   /* ice_size_distribution = "Gamma" ("Monodisperse" = 0)                         */
#define CMX_PARCEL_PRESCRIBED_THERMODYNAMICS (1u << 28)   /* prescribed_thermodynamics = true — CMX_ERR_UNSUPPORTED                       */
#define CMX_PARCEL_NSTATE 9
#define CMX_PARCEL_NCOEF 6
#define CMX_PARCEL_NPROC 6
#define CMX_PARCEL_MAX_STEPS_PER_LAUNCH 256               /* == kParcelMaxStepsPerLaunch, cmx_launch.hpp                                  */
typedef enum cmx_parcel_process_column {
    CMX_PARCEL_PROC_DN_LIQ_ACT = 0,
    CMX_PARCEL_PROC_DN_ICE_DEP = 1,
    CMX_PARCEL_PROC_DN_ICE_IMM = 2,
    CMX_PARCEL_PROC_DN_ICE_HOM = 3,
    CMX_PARCEL_PROC_DQ_LIQ_CE = 4,
    CMX_PARCEL_PROC_DQ_ICE_DS = 5
} cmx_parcel_process_column;
typedef enum cmx_parcel_coefficient_column {
    CMX_PARCEL_COEF_DEPOSITION_M = 0,
    CMX_PARCEL_COEF_DEPOSITION_C = 1,
    CMX_PARCEL_COEF_ABIFM_M = 2,
    CMX_PARCEL_COEF_ABIFM_C = 3,
    CMX_PARCEL_COEF_LINEAR_C1 = 4,
    CMX_PARCEL_COEF_LINEAR_C2 = 5
} cmx_parcel_coefficient_column;
int32_t cmx_parcel_tendencies_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n_parcels, const float *const *state, const float *w,
                                  const float *const *coefficients, float *const *tendencies, float *const *process_rates, void *stream);
int32_t cmx_parcel_tendencies_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n_parcels, const double *const *state, const double *w,
                                  const double *const *coefficients, double *const *tendencies, double *const *process_rates, void *stream);
int32_t cmx_parcel_run_f32(const cmx_parcel_params_f32 *pp, uint32_t flags, int64_t n_parcels, int64_t n_steps, int64_t save_every,
                           const float *const *state, const float *w, const float *const *coefficients, float *const *state_out, float *trajectory,
                           void *stream);
int32_t cmx_parcel_run_f64(const cmx_parcel_params_f64 *pp, uint32_t flags, int64_t n_parcels, int64_t n_steps, int64_t save_every,
                           const double *const *state, const double *w, const double *const *coefficients, double *const *state_out, double *trajectory,
                           void *stream);

/* ---------------------------------------------------------------------------
 * (14) The Jacobian of the SB2006 warm-rain tendencies — the derivatives the reference obtains with ForwardDiff through
 * BMT.bulk_microphysics_tendencies(Microphysics2Moment(), mp{WR, Nothing}, …) (test/ad_compat_tests.jl:106-175): what an implicit time step or a
 * calibration gradient of the host model consumes.  Per point the four tendencies of cmx_sb2006_warm_rain_tendencies_* (cmx_sb2006_jac_out) are
 * differentiated with respect to six of its seven inputs (cmx_sb2006_jac_wrt): T, q_tot, q_lcl, n_lcl, q_rai, n_rai; the air density ρ is held fixed.
 *   jac[o * CMX_SB2006_JAC_NWRT + i] = the column ∂out_o/∂in_i   (a host array of 24 device column pointers, any of them NULL)
 *   tendencies[o]                    = the tendency itself (NULL, or an array of 4 NULL-able columns): bit-identical to what
 *                                      cmx_sb2006_warm_rain_tendencies_* writes for the same points and parameters
 * The device runs the SAME point function as the tendencies entry on forward-mode dual numbers (a value and K tangents, csrc/cmx_dual.hpp): no finite
 * difference, no second statement of the physics.  Tangents follow the analytic rules; min / max / clamp and the conditional carry the tangents of the
 * operand whose value they return (ForwardDiff's rule), so at a kink the one-sided derivative of the branch taken is returned; the input clamps max(0, x)
 * (BMT:828-837) are part of the differentiated function (a negative input has zero derivative); a gate is a select, so a gated-off process contributes
 * exactly zero and a non-finite tangent behind a closed gate is discarded.  With the integer exponents of the published scheme (b = 3, c = 4, d = −5) the
 * integer-power instantiation runs, otherwise the general one — the choice the tendencies entry makes for the same struct.
 *
 * An input whose four columns are all NULL is not differentiated; the others are carried K at a time through ⌈n/K⌉ evaluations of the point function
 * inside ONE kernel (the inputs are read once).  The value of a column does not depend on which other columns are requested, bit for bit.
 * At least one column of `jac` or `tendencies` must be non-NULL (CMX_ERR_BAD_ARG).  flags: CMX_SB2006_LIMITED only; any other bit is CMX_ERR_BAD_ARG.
 * Statuses as for cmx_sb2006_warm_rain_tendencies_*, in its order: NULL parameters; the count rule (n_points = 0 is CMX_OK before anything else is looked
 * at); a NULL input column; no output; flags; unordered limiter pairs under CMX_SB2006_LIMITED.  A NaN in any of the seven inputs of a point gives NaN in
 * every output of that point.  A pure launch sequence on `stream`: no allocation, no synchronisation, graph-capturable; any alignment.
 * 7 columns in + up to 28 out: 140 B/point (f32) for the full Jacobian with the tendencies.
 * ------------------------------------------------------------------------- */
#define CMX_SB2006_JAC_NOUT 4
#define CMX_SB2006_JAC_NWRT 6
#define CMX_SB2006_JAC_NCOL 24               /* NOUT * NWRT */
typedef enum cmx_sb2006_jac_out {
    CMX_SB2006_JAC_DQ_LCL_DT = 0,
    CMX_SB2006_JAC_DN_LCL_DT = 1,
    CMX_SB2006_JAC_DQ_RAI_DT = 2,
    CMX_SB2006_JAC_DN_RAI_DT = 3
} cmx_sb2006_jac_out;
typedef enum cmx_sb2006_jac_wrt {
    CMX_SB2006_JAC_WRT_T = 0,
    CMX_SB2006_JAC_WRT_Q_TOT = 1,
    CMX_SB2006_JAC_WRT_Q_LCL = 2,
    CMX_SB2006_JAC_WRT_N_LCL = 3,
    CMX_SB2006_JAC_WRT_Q_RAI = 4,
    CMX_SB2006_JAC_WRT_N_RAI = 5
} cmx_sb2006_jac_wrt;
int32_t cmx_sb2006_warm_rain_jacobian_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                          const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                          float *const jac[CMX_SB2006_JAC_NCOL], float *const tendencies[CMX_SB2006_JAC_NOUT],
                                          void *stream);
int32_t cmx_sb2006_warm_rain_jacobian_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                          const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                          const double *n_rai, double *const jac[CMX_SB2006_JAC_NCOL],
                                          double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (15) The Jacobian of the 1-moment tendencies — the derivatives of BMT.bulk_microphysics_tendencies(Instantaneous(), Microphysics1Moment(), mp, tps, …)
 * (BMT:505-514 → :141-252) with respect to the state: what a linearly implicit step of the host model consumes in place of the donor-based
 * approximation inside LinearizedAverage (BMT:269-379).  Per point the four tendencies of cmx_mp1m_tendencies_* (cmx_mp1m_jac_out) are differentiated with
 * respect to six of its seven inputs (cmx_mp1m_jac_wrt): T, q_tot, q_lcl, q_icl, q_rai, q_sno; the air density ρ is held fixed.
 *   jac[o * CMX_MP1M_JAC_NWRT + i] = the column ∂out_o/∂in_i   (a host array of 24 device column pointers, any of them NULL)
 *   tendencies[o]                  = the tendency itself (NULL, or an array of 4 NULL-able columns): bit-identical to what cmx_mp1m_tendencies_*
 *                                    writes for the same points and parameters
 * The device runs the SAME point function as the tendencies entry on forward-mode dual numbers (csrc/cmx_dual.hpp), with the rules of (14): analytic
 * tangents; min / max / clamp and the conditional carry the tangents of the operand whose value they return, so at a kink — the saturation limiters, the
 * melting gate at T_freeze, q = ϵ — the one-sided derivative of the branch taken is returned; the input clamps max(0, x) (BMT:147-152; T is not clamped)
 * are part of the differentiated function; a gate is a select, and a process switched off by its option contributes exactly zero.  `flags` and the
 * parameter struct select the instantiation as for cmx_mp1m_tendencies_*: the default options with the default exponents, or the run-time-flags one.
 *
 * An input whose four columns are all NULL is not differentiated; the others are carried K at a time through ⌈n/K⌉ evaluations of the point function
 * inside ONE kernel (the inputs are read once).  The value of a column does not depend on which other columns are requested, bit for bit.
 * Statuses as for cmx_mp1m_tendencies_*, in its order: NULL parameters; the count rule; the flags (both members of an exclusive option pair, an unknown
 * bit: CMX_ERR_BAD_ARG); n_points = 0 is CMX_OK; a NULL input column; no non-NULL column in `jac` and `tendencies` at all (CMX_ERR_BAD_ARG).
 * A NaN in any of the seven inputs of a point gives NaN in every output of that point; in Float64 so does ρ ≤ 0.  A pure launch sequence on `stream`: no
 * allocation, no synchronisation, graph-capturable; any alignment.  7 columns in + up to 28 out: 140 B/point (f32) for the full Jacobian with the
 * tendencies.
 * ------------------------------------------------------------------------- */
#define CMX_MP1M_JAC_NOUT 4
#define CMX_MP1M_JAC_NWRT 6
#define CMX_MP1M_JAC_NCOL 24                 /* NOUT * NWRT */
typedef enum cmx_mp1m_jac_out {
    CMX_MP1M_JAC_DQ_LCL_DT = 0,
    CMX_MP1M_JAC_DQ_ICL_DT = 1,
    CMX_MP1M_JAC_DQ_RAI_DT = 2,
    CMX_MP1M_JAC_DQ_SNO_DT = 3
} cmx_mp1m_jac_out;
typedef enum cmx_mp1m_jac_wrt {
    CMX_MP1M_JAC_WRT_T = 0,
    CMX_MP1M_JAC_WRT_Q_TOT = 1,
    CMX_MP1M_JAC_WRT_Q_LCL = 2,
    CMX_MP1M_JAC_WRT_Q_ICL = 3,
    CMX_MP1M_JAC_WRT_Q_RAI = 4,
    CMX_MP1M_JAC_WRT_Q_SNO = 5
} cmx_mp1m_jac_wrt;
int32_t cmx_mp1m_jacobian_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                              const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                              float *const jac[CMX_MP1M_JAC_NCOL], float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_jacobian_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                              const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                              double *const jac[CMX_MP1M_JAC_NCOL], double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (16) Products with the Jacobian of the SB2006 warm-rain tendencies (14), fused into the pass that holds the tangents in registers: what a
 * Jacobian-free Newton–Krylov matvec (J v) and a gradient (Jᵀḡ: calibration, a closure trained through the scheme, torch autograd) consume, without
 * the 24 columns being written and read back.  State, outputs (cmx_sb2006_jac_out), differentiated inputs (cmx_sb2006_jac_wrt; ρ is held fixed),
 * derivative rules and instantiation choice are those of (14).
 *   cmx_sb2006_warm_rain_jvp_*:  jvp[o] = Σ_i ∂out_o/∂in_i · tangents[i]        one evaluation of the point function on duals seeded with the tangent
 *     tangents[i]   the tangent column of input i (a host array of 6 device column pointers; a NULL member is a zero tangent)
 *     jvp[o]        NULL, or an array of 4 NULL-able columns
 *   cmx_sb2006_warm_rain_vjp_*:  grad[i] = Σ_o cotangents[o] · ∂out_o/∂in_i      ⌈n_grad/K⌉ evaluations with unit seeds, contracted before the store
 *     cotangents[o] the cotangent column ḡ of output o (a host array of 4 device column pointers; a NULL member removes that output from the sum)
 *     grad[i]       NULL, or an array of 6 NULL-able columns; an input whose gradient is NULL is not differentiated
 *   tendencies[o]   as in (14): NULL, or 4 NULL-able columns, bit-identical to cmx_sb2006_warm_rain_tendencies_*
 * The products are plain IEEE arithmetic on the tangents (14) would store: a zero cotangent times an infinite tangent is NaN, as contracting the
 * columns of (14) would give; only a NULL cotangent removes an output.  The sum runs over the non-NULL cotangents in output order (first product, then
 * fused multiply-adds).  The value of grad[i] does not depend on which other gradients are requested, bit for bit.  With every member of `tangents`
 * NULL the products are zeros; with every member of `cotangents` NULL the requested gradients are zeros.
 * Statuses, their order, the flags and the limiter check as for (14); the `tangents` / `cotangents` table itself NULL, or no output column at all
 * (`jvp` / `grad` and `tendencies`), is CMX_ERR_BAD_ARG where (14) reports "no output".  A NaN in any of the seven inputs of a point, or in any given
 * tangent or cotangent value of it, gives NaN in every output of that point (tendencies included) and in that point only.  A pure launch sequence on
 * `stream`: no allocation, no synchronisation, graph-capturable; any alignment.  f32: J v 7 + 6 columns in, 4 out (68 B/point); Jᵀḡ 7 + 4 in, 6 out.
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_warm_rain_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const tangents[CMX_SB2006_JAC_NWRT], float *const jvp[CMX_SB2006_JAC_NOUT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const tangents[CMX_SB2006_JAC_NWRT], double *const jvp[CMX_SB2006_JAC_NOUT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                     const float *const cotangents[CMX_SB2006_JAC_NOUT], float *const grad[CMX_SB2006_JAC_NWRT],
                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                     const double *const cotangents[CMX_SB2006_JAC_NOUT], double *const grad[CMX_SB2006_JAC_NWRT],
                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (17) Products with the Jacobian of the 1-moment tendencies (15): cmx_mp1m_jvp_* and cmx_mp1m_vjp_*, with the arguments and the rules of (16) —
 * tangents[6] over cmx_mp1m_jac_wrt, cotangents[4] over cmx_mp1m_jac_out, NULL members, the order of the sum, plain IEEE products, subset independence —
 * and the state, `flags`, instantiation choice, statuses and their order of (15): NULL parameters; the count rule; the flags; n_points = 0 is CMX_OK;
 * a NULL input column; the `tangents` / `cotangents` table NULL or no output column at all (CMX_ERR_BAD_ARG).  `tendencies` is bit-identical to
 * cmx_mp1m_tendencies_*.  A NaN in any of the seven inputs of a point (in Float64 also ρ ≤ 0), or in any given tangent or cotangent value of it, gives
 * NaN in every output of that point and in that point only.  A pure launch sequence on `stream`, graph-capturable; any alignment.
 * ------------------------------------------------------------------------- */
int32_t cmx_mp1m_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const tangents[CMX_MP1M_JAC_NWRT], float *const jvp[CMX_MP1M_JAC_NOUT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream);
int32_t cmx_mp1m_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const tangents[CMX_MP1M_JAC_NWRT], double *const jvp[CMX_MP1M_JAC_NOUT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream);
int32_t cmx_mp1m_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                         const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                         const float *const cotangents[CMX_MP1M_JAC_NOUT], float *const grad[CMX_MP1M_JAC_NWRT], float *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream);
int32_t cmx_mp1m_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho, const double *T,
                         const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                         const double *const cotangents[CMX_MP1M_JAC_NOUT], double *const grad[CMX_MP1M_JAC_NWRT], double *const tendencies[CMX_MP1M_JAC_NOUT],
                         void *stream);

/* ---------------------------------------------------------------------------
 * (18) The tendency of a linearly implicit (Rosenbrock–Euler) step of the SB2006 warm-rain tendencies (14) and of the 1-moment tendencies (15), solved in
 * the pass that holds the Jacobian in registers.  With s the four species whose tendencies the scheme returns — SB2006: q_lcl, n_lcl, q_rai, n_rai;
 * 1-moment: q_lcl, q_icl, q_rai, q_sno (wrt indices 2 … 5; output q is the tendency of s_q) — f the four tendencies at the point and J = ∂f/∂s the
 * 4 × 4 species block of (14) / (15), with ρ, T and q_tot held fixed:
 *     implicit = r = (I − Δt J)⁻¹ f            the step is  s ← s + Δt r;  r = f at Δt = 0
 *   dt             Δt in seconds, finite and ≥ 0 (rounded to the float type of the entry)
 *   implicit[q]    a host array of 4 NULL-able device columns, not NULL itself
 *   tendencies[q]  NULL, or 4 NULL-able columns: f itself, bit-identical to cmx_sb2006_warm_rain_tendencies_* / cmx_mp1m_tendencies_*
 * J is what (14) / (15) would store, bit for bit.  I − Δt J is equilibrated with exact powers of two (columns from the clamped state, rows from the row
 * maxima) and solved by Gaussian elimination with partial pivoting in registers; the result is that of torch.linalg.solve on the columns of (14) / (15) to
 * the backward error of an LU in the entry's float type.  All four components are computed whatever subset is stored: a column's bits do not depend on
 * which others are requested.  At Δt = 0, implicit is f in every bit.  A singular I − Δt J follows IEEE: non-finite r at that point only, no status.  An
 * absent species (input ≤ 0) has a zero Jacobian column, the system stays regular.  A NaN in any of the seven inputs of a point (1-moment Float64: also
 * ρ ≤ 0) gives NaN in every output of that point and in that point only.
 * State, `flags`, option sets, instantiation choice, statuses and their order are those of (14) resp. (15); `dt` is checked after the columns and the
 * `implicit` table: negative, NaN or infinite is CMX_ERR_BAD_ARG, as is a NULL `implicit` or no output column at all.  A pure launch sequence on `stream`:
 * no allocation, no synchronisation, graph-capturable; any alignment; 7 columns in, 4 out (8 with the tendencies).  An output column may be the species
 * column it steps (in place): a lane reads its point before it writes it.
 * Not done here: T or q_tot as unknowns of the solve, autograd through the solve, the 2M + P3 scheme; sub-stepping and positivity limiting of s + Δt r: (19).
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_warm_rain_implicit_tendencies_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points,
                                                     const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl,
                                                     const float *q_rai, const float *n_rai, double dt, float *const implicit[CMX_SB2006_JAC_NOUT],
                                                     float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_implicit_tendencies_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points,
                                                     const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl,
                                                     const double *q_rai, const double *n_rai, double dt, double *const implicit[CMX_SB2006_JAC_NOUT],
                                                     double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_mp1m_implicit_tendencies_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                         const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                         double dt, float *const implicit[CMX_MP1M_JAC_NOUT], float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_implicit_tendencies_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                         const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                         double dt, double *const implicit[CMX_MP1M_JAC_NOUT], double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (19) The average tendency of the four species of (18) over a time step Δt, taken in `nsub` linearly implicit substeps inside ONE kernel, with the
 * temperature following the latent heating of every substep — what a host model calls per time step.  The mode the reference has for the 1-moment scheme as
 * LinearizedAverage (BMT:572-632; entry (5) here) with a donor-based linearization, built on the true Jacobian of (14) / (15) and for the 2-moment warm-rain
 * scheme as well.  The definition, normative bit for bit — all arithmetic in the entry's float type FT, every product and sum a separate IEEE operation
 * (no fma), the selects written as selects so that a NaN stays a NaN:
 *     dt_f = FT(dt);  h = dt_f / FT(nsub);  inv_h = FT(1)/h;  inv_dt = FT(1)/dt_f;  Lv = LH_v0/cp_d;  Ls = LH_s0/cp_d     (fields of `tps`, FT divisions)
 *     repeat nsub times, with s the four species, T the temperature, ρ and q_tot fixed:
 *         r    = the `implicit` result of (18) for (ρ, T, q_tot, s) with Δt = h, bit for bit
 *         sn_j = s_j + r_j*h
 *         if step_flags has CMX_STEP_NONNEGATIVE:   lo_j = (s_j < 0 ? s_j : 0);   sn_j = (sn_j < lo_j ? lo_j : sn_j)
 *         d_j  = (sn_j − s_j) * inv_h
 *         T    = T + (Lv*(d_q_lcl + d_q_rai)) * h                                   SB2006
 *         T    = T + (Lv*(d_q_lcl + d_q_rai) + Ls*(d_q_icl + d_q_sno)) * h          1-moment (BMT:619-623)
 *         s    = sn
 *     average_j = (s_j − s0_j) * inv_dt
 * With CMX_STEP_NONNEGATIVE a species never ends a substep below 0, and one that was negative already never below where it started; the plain
 * Rosenbrock–Euler step leaves a species negative at a large share of realistic states.  The limiter does not change the first
 * order of the scheme in Δt/nsub.
 *   dt             Δt in seconds: finite and > 0, and h and 1/dt_f finite positive normal numbers of FT
 *   nsub           1 … CMX_IMPLICIT_AVERAGE_MAX_NSUB
 *   step_flags     0 or CMX_STEP_NONNEGATIVE
 *   average[q]     a host array of 4 NULL-able device columns, not NULL itself; a column's bits do not depend on which others are requested
 * State, `flags`, option sets, instantiation choice, statuses and their order are those of (18); then `dt`, `nsub` and `step_flags` as above — anything else is
 * CMX_ERR_BAD_ARG, as is a NULL `average` or no output column at all.  The NaN rule is that of (18) in every substep: a NaN in any of the seven inputs of a
 * point (1-moment Float64: also ρ ≤ 0) gives NaN in all four outputs of that point and in that point only; a singular substep solve makes that point
 * non-finite and no other.  A pure launch sequence on `stream`: no allocation, no synchronisation, graph-capturable; any alignment; 7 columns in, 4 out.  An
 * output column may be a species column (in place): a lane reads everything it needs before it writes.
 * Not done here: adaptive step sizes, T or q_tot as unknowns of the solve, autograd through the average, the `*_fields_*` layouts, the 2M + P3 scheme.
 * ------------------------------------------------------------------------- */
#define CMX_STEP_NONNEGATIVE 1u
#define CMX_IMPLICIT_AVERAGE_MAX_NSUB 64
int32_t cmx_sb2006_warm_rain_implicit_average_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points,
                                                  const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl,
                                                  const float *q_rai, const float *n_rai, double dt, int32_t nsub, uint32_t step_flags,
                                                  float *const average[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_implicit_average_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points,
                                                  const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl,
                                                  const double *q_rai, const double *n_rai, double dt, int32_t nsub, uint32_t step_flags,
                                                  double *const average[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_mp1m_implicit_average_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                      const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                                      double dt, int32_t nsub, uint32_t step_flags, float *const average[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_implicit_average_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                      const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                                      double dt, int32_t nsub, uint32_t step_flags, double *const average[CMX_MP1M_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (20) The column steps with the average tendency of (19) as tendency operator: what a host model calls per time step — tendencies, fall speeds and first-order
 * upwind sedimentation in one pass, as cmx_sb2006_column_tendencies_sedimentation_* and cmx_mp1m_column_tendencies_sedimentation_* — with the sub-stepped
 * implicit average in the place of the instantaneous (or LinearizedAverage) tendencies.  For the 2-moment scheme this is the one column step that is stable at a
 * large Δt.  ONE kernel; layout, `inv_dz`, the parameter structs, `flags` and the surface-flux outputs are those of the scheme's column entry, `dt`, `nsub`
 * and `step_flags` those of (19).  The definition, normative — per point k of a column, in the entry's float type FT:
 *     a_j   = average_j of (19) for (ρ, T, q_tot, s) of the point with (dt, nsub, step_flags), bit for bit
 *     F, g  = the fluxes F_j = ρ⁺ χ_j⁺ w_j of the four falling species and g = inv_dz[k]/ρ_k⁺ of the scheme's column entry for the same options, bit for bit,
 *             evaluated at the INITIAL state of the step: sedimentation stays explicit
 *     out_j = fma(top ? 0 : F_j[k+1], g, fma(−F_j[k], g, a_j)),      top: k = n_lev − 1 (nothing enters through the model top)
 * — the combining expression of the existing column entries with a_j in the place of the tendency.  The surface outputs (`precip_flux`; `precip_rai`,
 * `precip_sno`; optional, n_col values) are F at level 0, as in the existing entries.  SB2006 without `cloud_vel`: q_lcl and n_lcl do not fall, their outputs
 * are a_j themselves (as today, no fma is applied to them).
 * NaN rule: that of (19) for a point's four a_j — a NaN in any of the seven inputs of a point (1-moment Float64: also ρ ≤ 0) gives NaN in all four outputs of
 * the point; that of the existing column entries for the fluxes — a NaN in ρ or in a species poisons that species' flux (SB2006: the fluxes of the point) and,
 * through it, the tendency of the cell below, and nothing else.  Results do not depend on where the kernel's tile boundaries fall, nor on alignment.
 * Statuses, in this order: those of the scheme's column entry up to and including the column and table checks (NULL structs, n_col < 0, n_lev < 1; the flags —
 * cmx_mp1m_*: both snow-shape bits CMX_ERR_BAD_ARG, a single one CMX_ERR_UNSUPPORTED; n_col·n_lev above what one launch expresses CMX_ERR_UNSUPPORTED;
 * n_col·n_lev = 0 is CMX_OK; NULL columns; cmx_sb2006_*: the limiter pairs and the fall-speed table); then `dt`, `nsub` and `step_flags` as in (19)
 * (CMX_ERR_BAD_ARG).  All four outputs are required.  A pure launch sequence on `stream`: no allocation, no synchronisation, graph-capturable; any alignment.
 * NOT in place: an output column must not alias an input column — another workgroup reads the point above.  This deliberately differs from (19).
 * Not done here: the 1-moment snow shapes (CMX_1M_SED_SNOW_OBLATE / _PROLATE: CMX_ERR_UNSUPPORTED), implicit sedimentation — (21) —, the 2M + P3 column step, the
 * `*_fields_*` layouts, autograd.
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_column_implicit_average_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                                             const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho, const float *T,
                                                             const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                                             float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt, float *precip_flux,
                                                             void *stream);
int32_t cmx_sb2006_column_implicit_average_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                                             const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags,
                                                             int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho, const double *T,
                                                             const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                                             const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                             double *precip_flux, void *stream);
int32_t cmx_mp1m_column_implicit_average_sedimentation_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                                           const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                           const float *const *in, float *const *out, float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_implicit_average_sedimentation_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                                           const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags,
                                                           double dt, int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                           const double *const *in, double *const *out, double *precip_rai, double *precip_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (21) The column steps of (20) with IMPLICIT sedimentation: the average tendency of (19) per point and, in the same kernel, backward-Euler first-order upwind
 * sedimentation — stable and positive at any Courant number c = Δt·w/Δz, where the explicit fluxes of (20) need c ≤ 1 (rain at 5–9 m/s through 30–100 m
 * layers at Δt = 30–300 s: c = 2 … 80).  A host model that takes (20) at the Δt the average is built for must sub-cycle sedimentation itself; with these
 * entries it need not.  The argument lists are exactly those of the (20) entries, the checks and statuses the same in the same order.  The definition,
 * normative — per column, for each falling species j, in the entry's float type FT, level 0 the lowest:
 *     a      = average_j of (19) for the point, bit for bit                                                       (as in (20))
 *     F, g   = F_j = (ρ⁺χ_j⁺)·w_j and g = inv_dz[k]/ρ_k⁺ of the scheme's column entry, bit for bit                (as in (20))
 *     w      = the fall speed that the scheme's flux function multiplies into F_j (that value itself, not F/(ρχ))
 *     τ      = FT(dt)·w          c = τ·inv_dz[k]       β = τ·ρ⁺        D = 1 + c       r = 1/D
 *     A      = c·r               B = fma(β, a, F)·r
 *     G_k    = top ? B_k : fma(A_k, G_{k+1}, B_k)          top: k = n_lev − 1;  evaluated from the top level downward, in this order
 *     out_k  = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k)) · r_k
 * r is a TRUE (correctly rounded IEEE) division in both float types: exactly 1 at c = 0.  Every other product and sum is a separate IEEE operation except
 * the fma's written above.  "top" is a select, never a multiplication by zero.
 * This is backward Euler on ∂χ/∂t = a + (G_{k+1} − G_k)·g with G_k = w_k ρ_k (χ_k + Δt·out_k), the fall speeds frozen at the initial state; substituting gives
 * G_k = (F_k + β_k a_k + c_k G_{k+1})/(1 + c_k), an affine recurrence with 0 ≤ A < 1.  With inv_dz ≡ 0 the outputs are the averages of (19).
 * The surface outputs (`precip_flux`; `precip_rai`, `precip_sno`; optional, n_col values) are G at level 0 — the flux that leaves the column DURING the step,
 * so that the column budget Σ_k ρ_k out_k Δz_k + G_0 = Σ_k ρ_k a_k Δz_k closes — not the initial F_0 of (20).  SB2006 without `cloud_vel`: q_lcl and n_lcl do
 * not fall, their outputs are a_j themselves, as in (20).
 * NaN rule: that of (19) for a_j and that of (20) for F_j; on top of those the recurrence carries a NaN in G_j DOWNWARD: it reaches every lower level of the
 * same species in the same column (of every species, if a_j is NaN at that point: then all four B are), never a higher level and never another column.
 * Results do not depend on how the kernel divides the columns among workgroups, on alignment, or on the number of columns in the call.  A pure launch
 * sequence on `stream` (ONE kernel): no allocation, no synchronisation, graph-capturable; any alignment.  NOT in place, as (20).
 * Not done here: the 1-moment snow shapes (a single CMX_1M_SED_SNOW_* bit: CMX_ERR_UNSUPPORTED, as in (20)), the 2M + P3 column step — (24) —, the `*_fields_*`
 * layouts, autograd, fall speeds re-evaluated inside the step.
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_column_implicit_step_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                            const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const float *inv_dz, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                            const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt,
                                            float *dn_rai_dt, float *precip_flux, void *stream);
int32_t cmx_sb2006_column_implicit_step_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                            const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, double dt, int32_t nsub, uint32_t step_flags, int64_t n_col,
                                            int32_t n_lev, const double *inv_dz, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                            const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt,
                                            double *dq_rai_dt, double *dn_rai_dt, double *precip_flux, void *stream);
int32_t cmx_mp1m_column_implicit_step_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                          const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *const *in,
                                          float *const *out, float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_implicit_step_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                          const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, double dt,
                                          int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *const *in,
                                          double *const *out, double *precip_rai, double *precip_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (22) The derivatives of the SB2006 warm-rain tendencies (14) with respect to the PARAMETERS θ — what a calibration, or a closure trained through the
 * scheme, needs: dL/dθ, not dL/dx.  State, `flags`, outputs (cmx_sb2006_jac_out) and derivative rules are those of (14); the state is held fixed.
 * A DIRECTION is a pair of structs of the entry's own parameter types whose floating fields hold δθ: d_warm_rain[d] (a host array of `ndir` structs) and
 * d_tps[d] (NULL: zero).  For each direction the host forms the tangent ċ = Dc(θ)[δθ] of every folded constant in exact forward mode in double (no
 * difference quotient); the tangents travel as kernel arguments (no allocation, no copy to the device), and the device runs the SAME point function as
 * the tendencies entry on forward-mode duals whose tangents are those of the constants.
 *   cmx_sb2006_warm_rain_param_jvp_*:  jvp[d·4 + o] = Σ_p ∂out_o/∂θ_p · δθ_p⁽ᵈ⁾ per point
 *     jvp           a host array of ndir·4 NULL-able device columns
 *   cmx_sb2006_warm_rain_param_vjp_*:  grad[d] = Σ_points Σ_o cotangents[o] · (∂out_o/∂θ · δθ⁽ᵈ⁾), accumulated in DOUBLE; a one-hot direction gives dL/dθ_p
 *     cotangents[o] the cotangent column ḡ of output o (a host array of 4 device column pointers; a NULL member removes that output from the sum)
 *     grad          `ndir` doubles of DEVICE memory
 *     workspace     ndir · CMX_PARAM_VJP_PARTIALS doubles of device memory owned by the caller (the library allocates nothing)
 *   tendencies[o]   NULL, or 4 NULL-able columns
 * The reduction is that of (3): a fixed number of workgroups each own a contiguous chunk, a lane adds its points in index order (per point the sum over the
 * outputs is the fused multiply-add chain of (16), widened to double), a fixed shuffle tree, a finish launch.  No floating-point atomics: grad is a pure
 * function of the inputs and n_points, bit-identical from run to run and from device to device.  n_points = 0 sets grad to zeros.
 * A call with more directions than one launch carries is a sequence of launches on `stream`; a jvp column's bits and a grad value's bits do not depend on
 * which other directions are in the call, on ndir or on how the call was split.
 * INSTANTIATION.  If no direction has a non-zero component on acnv.b, accr.c or self.d, the instantiation the tendencies entry selects runs and `tendencies`
 * is bit-identical to cmx_sb2006_warm_rain_tendencies_*.  Otherwise the general (exp2(e·log2 x)) instantiation runs for the whole call — a power by
 * multiplication has no derivative with respect to its exponent — and `tendencies` agrees with the tendencies entry to the parity bound, not bit for bit.
 * Constants that only feed compares (thresholds, gates) contribute no derivative: the derivative is that of the branch taken.
 * Statuses, in this order: NULL parameters; the count rule (param_jvp: n_points = 0 is CMX_OK; param_vjp writes grad for n_points = 0 too and goes on with every
 * check below but the columns, so a bad call is refused whatever n_points is); NULL columns; ndir outside
 * 1 … CMX_PARAM_MAX_DIRS; a NULL direction table (param_vjp: or a NULL cotangent table); no output at all (param_vjp: a NULL grad or workspace); a
 * non-finite component in a direction; the flags and limiters of (14) — all CMX_ERR_BAD_ARG, all before the first enqueue.  NaN rule: a NaN in any of the
 * seven inputs of a point gives NaN in every jvp and tendency of that point; in param_vjp a NaN in a point's state or cotangents makes every grad[d] NaN.
 * Graph-capturable; any alignment.  The 1-moment scheme: (23).  Not done here: the fall-speed outputs, the implicit entries, second derivatives.  The SB2006 column step with its fall speeds: (26).
 * ------------------------------------------------------------------------- */
#define CMX_PARAM_MAX_DIRS 16
#define CMX_PARAM_VJP_PARTIALS 1024
int32_t cmx_sb2006_warm_rain_param_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                           const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                           int32_t ndir, const cmx_warm_rain_2m_f32 *d_warm_rain, const cmx_thermo_f32 *d_tps, float *const *jvp,
                                           float *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_param_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                           const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                           const double *n_rai, int32_t ndir, const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps,
                                           double *const *jvp, double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);
int32_t cmx_sb2006_warm_rain_param_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho,
                                           const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                           const float *const cotangents[CMX_SB2006_JAC_NOUT], int32_t ndir, const cmx_warm_rain_2m_f32 *d_warm_rain,
                                           const cmx_thermo_f32 *d_tps, double *grad, double *workspace, float *const tendencies[CMX_SB2006_JAC_NOUT],
                                           void *stream);
int32_t cmx_sb2006_warm_rain_param_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                                           const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                           const double *n_rai, const double *const cotangents[CMX_SB2006_JAC_NOUT], int32_t ndir,
                                           const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps, double *grad, double *workspace,
                                           double *const tendencies[CMX_SB2006_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (23) The derivatives of the 1-moment tendencies (15) with respect to the PARAMETERS: cmx_mp1m_param_jvp_* and cmx_mp1m_param_vjp_*, with the arguments and
 * the rules of (22) — directions d_mp[d] (cmx_microphysics_1m_*) + d_tps[d] | NULL, jvp[d·4 + o] over cmx_mp1m_jac_out, grad / workspace, NULL members, the
 * reduction, the launches, bit independence from the other directions and from the split — and the state, `flags`, NaN rule (Float64: also ρ ≤ 0) and statuses
 * of (15): NULL parameters; the count rule; the flags; param_jvp: n_points = 0 is CMX_OK; NULL columns; then ndir, the tables, the outputs and non-finite
 * directions as in (22).
 * INSTANTIATION.  The default-options instantiation of (5) holds nine slope-parameter exponents as compile-time numbers (rain: fall speed, accretion, ice–rain
 * sink, snow–rain kernel, ventilation; snow: the same without the sink).  It runs — and `tendencies` is bit-identical to cmx_mp1m_tendencies_* — only if the
 * tendencies entry would select it AND no direction gives one of the nine a non-zero tangent (the size-relation exponents me, Δm, ae, Δa, ve, Δv of rain and
 * snow do).  Otherwise the run-time-flags instantiation runs for the whole call and `tendencies` agrees to the parity bound, not bit for bit.
 * The 1-moment column step with its four fall speeds and both precipitation fluxes: (28).
 * ------------------------------------------------------------------------- */
int32_t cmx_mp1m_param_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                               const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno, int32_t ndir,
                               const cmx_microphysics_1m_f32 *d_mp, const cmx_thermo_f32 *d_tps, float *const *jvp,
                               float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_param_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                               const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                               int32_t ndir, const cmx_microphysics_1m_f64 *d_mp, const cmx_thermo_f64 *d_tps, double *const *jvp,
                               double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_param_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, uint32_t flags, int64_t n_points, const float *rho, const float *T,
                               const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai, const float *q_sno,
                               const float *const cotangents[CMX_MP1M_JAC_NOUT], int32_t ndir, const cmx_microphysics_1m_f32 *d_mp,
                               const cmx_thermo_f32 *d_tps, double *grad, double *workspace, float *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);
int32_t cmx_mp1m_param_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, uint32_t flags, int64_t n_points, const double *rho,
                               const double *T, const double *q_tot, const double *q_lcl, const double *q_icl, const double *q_rai, const double *q_sno,
                               const double *const cotangents[CMX_MP1M_JAC_NOUT], int32_t ndir, const cmx_microphysics_1m_f64 *d_mp,
                               const cmx_thermo_f64 *d_tps, double *grad, double *workspace, double *const tendencies[CMX_MP1M_JAC_NOUT], void *stream);

/* ---------------------------------------------------------------------------
 * (24) The 2M + P3 column step (9b) with IMPLICIT sedimentation: backward-Euler first-order upwind sedimentation of the eight falling species, stable at any
 * Courant number c = Δt·w/Δz, where the explicit flux divergence of (9b) needs c ≤ 1 (rimed ice at 5–9 m/s, rain at up to 12 m/s through 30–500 m layers:
 * the largest c is 7–10 at Δt = 30 s and 74–99 at Δt = 300 s on the test states, with the fall speeds of this library on an MI355X).  A host model that
 * calls (9b) must sub-cycle sedimentation itself; with these entries it need not.  The
 * argument list is that of the (9b) entries with one `double dt` inserted after `p`; layout, `in`, `tendencies`, `log_lambda`, `v_ice_n`, `v_ice_m` and `flags`
 * are those of (9b).  The call runs steps 1 and 2 of (9b) unchanged — products → shape and fall speeds → the eight tendencies: the same launches, hence the
 * same bits for log_lambda, v_ice_n, v_ice_m and the tendencies a_j — and ONE kernel in the place of step 3.  The definition, normative — per column, for
 * each falling species j, in the entry's float type FT, level 0 the lowest:
 *     a      = the tendency of step 2 at the point, bit for bit
 *     F, w   = the flux F_j = (ρ⁺χ_j⁺)·w_j of step 3 of (9b), bit for bit, and the fall speed w_j that step multiplies into it (that value itself, not F/(ρχ)):
 *              the rain speeds w_m (q_rai) and w_n (n_rai), v_ice_m (q_ice, q_rim, b_rim), v_ice_n (n_ice), with cloud_vel c_m (q_lcl) and c_n (n_lcl)
 *     g      = inv_dz[k]·rcp(ρ⁺), exactly as step 3 of (9b) forms it
 *     τ      = FT(dt)·w          c = τ·inv_dz[k]       β = τ·ρ⁺        r = 1/(1 + c)
 *     A      = c·r               B = fma(β, a, F)·r
 *     G_k    = top ? B_k : fma(A_k, G_{k+1}, B_k)          top: k = n_lev − 1;  evaluated from the top level downward, in this order
 *     out_k  = fma(top ? 0 : G_{k+1}, g, fma(−F_k, g, a_k)) · r_k
 * r is a TRUE (correctly rounded IEEE) division in both float types: exactly 1 at c = 0.  Every other product and sum is a separate IEEE operation except the
 * fma's written above.  out_j overwrites tendencies[j].  Without cloud_vel the two cloud columns are not touched: they keep the tendencies of step 2.
 * This is backward Euler on ∂χ/∂t = a + (G_{k+1} − G_k)·g with G_k = w_k ρ_k (χ_k + Δt·out_k), the fall speeds frozen at the initial state, as in (21); the
 * tendency a is NOT limited here (the limiter of (19) has no counterpart in (9)), so χ + Δt·out can be negative where χ + Δt·a is — the step adds no
 * negativity of its own to what the tendencies alone would leave.
 * precip_rai, precip_ice (optional, n_col values) are G at level 0 of q_rai and q_ice — the flux that leaves the column DURING the step, so that the column
 * budget Σ_k ρ_k out_k Δz_k + G_0 = Σ_k ρ_k a_k Δz_k closes — not the initial F_0 of (9b).
 * Two consequences of the definition:
 *   - dt = 0: c = 0, r = 1, A = 0 and G = F, so the entry is the (9b) entry value for value (wherever a and F are finite).  The only possible difference is a
 *     −0 that becomes +0 at the top level, where fma(0, g, ·) stands in the place of the select.
 *   - inv_dz ≡ 0: c = 0, r = 1 and g = 0, so the outputs are the pointwise tendencies of step 2 for every dt.
 * `dt` must be finite and ≥ 0, and FT(dt) must be finite (0 ≤ dt ≤ the largest finite FT).  Statuses: those of (9b) in their order, then `dt`
 * (CMX_ERR_BAD_ARG) — all of them before any HIP
 * call; n_col = 0 is CMX_OK whatever dt is, as it is whatever the columns are.
 * NaN rule: that of (9b) for a_j and F_j; on top of it the recurrence carries a non-finite G DOWNWARD — a non-finite a_j or F_j at level l makes out_j non-finite
 * at every level ≤ l of that species in that column; it never reaches a level above l and never another column.
 * Results do not depend on how the kernel divides the columns among workgroups, on alignment, or on the number of columns in the call.  A pure launch
 * sequence on `stream` (products → shape + fall speeds → tendencies → implicit sedimentation): no allocation, no synchronisation, graph-capturable.  The
 * tendency columns must not alias an input column, as in (9b).
 * Not done here: implicit (Jacobian-based) P3 tendencies, fall speeds re-evaluated inside the step, the `*_fields_*` layouts, autograd.
 * ------------------------------------------------------------------------- */
int32_t cmx_mp2m_p3_column_implicit_sedimentation_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_p3_ice_params_f32 *ice, const cmx_thermo_f32 *tps,
                                                      const cmx_rain_vel_f32 *rain_vel, const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags,
                                                      int32_t brent_iters, float p, double dt, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                      const float *const *in, float *const *tendencies, float *log_lambda, float *v_ice_n, float *v_ice_m,
                                                      float *precip_rai, float *precip_ice, void *stream);
int32_t cmx_mp2m_p3_column_implicit_sedimentation_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_p3_ice_params_f64 *ice, const cmx_thermo_f64 *tps,
                                                      const cmx_rain_vel_f64 *rain_vel, const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags,
                                                      int32_t brent_iters, double p, double dt, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                      const double *const *in, double *const *tendencies, double *log_lambda, double *v_ice_n,
                                                      double *v_ice_m, double *precip_rai, double *precip_ice, void *stream);

/* ---------------------------------------------------------------------------
 * (25) The products J v and Jᵀḡ with the Jacobian of the SB2006 COLUMN step (2b) — tendencies, fall speeds and upwind flux divergence in one call, plus the
 * surface precipitation flux — with respect to the prognostic state: cmx_sb2006_column_jvp_* and cmx_sb2006_column_vjp_*.  (16) differentiates the point
 * function without its fall speeds; these differentiate what a host model steps.  J v is the matvec of a Newton–Krylov solver that treats microphysics and
 * sedimentation implicitly together; Jᵀḡ with the cotangent of the precipitation flux is what loss(precip_flux).backward() needs (cmx.autograd).
 * The function that is differentiated, normative — per column, level 0 the lowest, x_k = (T, q_tot, q_lcl, n_lcl, q_rai, n_rai)_k:
 *     out_k  = tend(ρ_k, x_k) + g_k·(F_{k+1} − F_k)        g_k = inv_dz[k]·(1/ρ_k⁺)        F_{n_lev} = 0        precip = F_0[q_rai]
 * F_k = ρ⁺χ⁺w: the fluxes of q_rai and n_rai, and of q_lcl and n_lcl when `cloud_vel` is given; the flux terms apply to those species' tendencies only.  The
 * fluxes are those of (2b): the fall speeds the point function returns, multiplied as there.  ρ and inv_dz are held FIXED, as ρ is in (14) – (19).
 * The clamps of the inputs, the ε floors, the gates and the max(0, ·) of the fall speeds are part of the function; the derivative is that of the branch taken,
 * as in (14).  In the general Chen-2022 instantiation the Γ terms depend on ρ only: they are evaluated on the value and carry no tangent.
 * With Ḟ_k = (∂F_k/∂x_k)·v_k, and J_pt the Jacobian of tend at the point:
 *     J v:    ẏ_k = J_pt(x_k)·v_k + g_k·(Ḟ_{k+1} − Ḟ_k)          ṗ = Ḟ_0[q_rai], one value per column
 *     Jᵀḡ:    x̄_k = J_pt(x_k)ᵀ·ḡ_k + (∂F_k/∂x_k)ᵀ·λ_k            λ_k[s] = −g_k·ḡ_k[s] + [k > 0]·g_{k−1}·ḡ_{k−1}[s] + [k = 0 and s = q_rai]·p̄
 * for each falling species s; p̄ is the cotangent of the precipitation flux, one value per column.  The block Jacobian is upper bidiagonal in the level
 * index and never couples two columns.
 * Arguments: the head of the (2b) entries through n_rai, with its layout (n_col columns of n_lev contiguous levels), flags, limiter and fall-speed checks and
 * their statuses, in that entry's order; then
 *   jvp:  tangents[6] in the order of cmx_sb2006_jac_wrt (the table or a member NULL: a zero tangent), jvp[4] in the order of cmx_sb2006_jac_out, jvp_precip
 *         (n_col values), tendencies[4], precip_flux (n_col values);
 *   vjp:  cotangents[4] (the table or a member NULL: that output is structurally absent from the sum), cot_precip (n_col values or NULL: absent), grad[6],
 *         tendencies[4], precip_flux.
 * Every output table, every member and every output column may be NULL; a call with no output at all is CMX_ERR_BAD_ARG, and so is an output that is one of
 * the call's input columns (a lane reads its neighbours).  n_col·n_lev is limited as in (2b); n_col = 0 is CMX_OK.
 * Requested `tendencies` and `precip_flux` are those of the (2b) entry on the same columns, bit for bit.  The products are plain IEEE arithmetic on the
 * tangents: Jᵀḡ accumulates the point sums with ḡ in output order, then the fluxes with λ in the order q_rai, n_rai, q_lcl, n_lcl, as one chain of fma
 * seeded with −0 (no term at all: +0); each gradient comes from its own tangent slot, so its bits do not depend on which other gradients are requested.  T
 * and q_tot do not enter the fluxes.  With inv_dz ≡ 0 the products equal those of (16) under == wherever the flux tangents are finite.
 * NaN rule: a NaN in any state input, or in any given tangent or cotangent value of a point (p̄ counts for the level-0 point), gives NaN in every output of
 * that point.  A NaN in an input of the fluxes (ρ, q_lcl, n_lcl, q_rai, n_rai) reaches the cell below through F and Ḟ exactly as in (2b), and the column's
 * precipitation outputs at level 0; a NaN tangent reaches Ḟ by plain IEEE arithmetic.  In Jᵀḡ a NaN in ḡ_{k−1} or ρ_{k−1} reaches x̄_k by plain IEEE
 * propagation through λ_k.  There is no other rule.
 * Results do not depend on how the kernels divide the columns among workgroups, on alignment, or on the number of columns in the call.  Both entries are
 * pure launches on `stream`: no allocation, no synchronisation, graph-capturable.
 * Not done here: the 2M + P3 column step, derivatives with respect to ρ or inv_dz, the implicit column steps (20), (21).  The
 * parameters through the column: (26).  The 1-moment column step: (27).  cmx_version() stays at 0.5 (no struct layout changed; an older library fails on the symbol lookup).
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_column_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                  const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                  const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                  const float *const tangents[CMX_SB2006_JAC_NWRT], float *const jvp[CMX_SB2006_JAC_NOUT], float *jvp_precip,
                                  float *const tendencies[CMX_SB2006_JAC_NOUT], float *precip_flux, void *stream);
int32_t cmx_sb2006_column_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                  const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                  const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                  const double *const tangents[CMX_SB2006_JAC_NWRT], double *const jvp[CMX_SB2006_JAC_NOUT], double *jvp_precip,
                                  double *const tendencies[CMX_SB2006_JAC_NOUT], double *precip_flux, void *stream);
int32_t cmx_sb2006_column_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                  const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                  const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                  const float *const cotangents[CMX_SB2006_JAC_NOUT], const float *cot_precip, float *const grad[CMX_SB2006_JAC_NWRT],
                                  float *const tendencies[CMX_SB2006_JAC_NOUT], float *precip_flux, void *stream);
int32_t cmx_sb2006_column_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                  const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                  const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                  const double *const cotangents[CMX_SB2006_JAC_NOUT], const double *cot_precip, double *const grad[CMX_SB2006_JAC_NWRT],
                                  double *const tendencies[CMX_SB2006_JAC_NOUT], double *precip_flux, void *stream);

/* ---------------------------------------------------------------------------
 * (26) The derivatives of the SB2006 COLUMN step (2b), (25) with respect to the scheme's PARAMETERS, the fall-speed parameters and the surface
 * precipitation flux included: cmx_sb2006_column_param_jvp_* (per point, J_θ·δθ) and cmx_sb2006_column_param_vjp_* (the reduced gradient dL/dθ).  (22)
 * stops before the fall speeds; (25) reaches the state but not θ.  This is what loss(precip_flux).backward() needs to reach `theta` (cmx.autograd).
 * The function is that of (25), normative, with the state, ρ and inv_dz held FIXED and θ = every floating field of the four parameter structs the (2b)
 * entry reads:
 *     out_k = tend(ρ_k, x_k; θ) + g_k·(F_{k+1}(θ) − F_k(θ))        precip = F_0[q_rai]
 * With Ḟ_k = ∂F_k/∂θ·δθ:
 *     J_θ δθ:    ẏ_k = ∂tend/∂θ·δθ + g_k·(Ḟ_{k+1} − Ḟ_k)          ṗ = Ḟ_0[q_rai], one value per column
 *     gradient:  grad[d] = Σ_columns Σ_k ( Σ_o ḡ_{o,k}·(∂tend_o/∂θ·δθ⁽ᵈ⁾)_k + Σ_s λ_k[s]·Ḟ_k[s]⁽ᵈ⁾ ),  λ_k exactly that of (25), p̄ at level 0 for q_rai
 * A DIRECTION is four structs of the entry's own types holding δθ: d_warm_rain[ndir] (required), d_tps[ndir], d_vel[ndir], d_cloud_vel[ndir] (each may be
 * NULL: zero).  Without `cloud_vel`, d_cloud_vel is IGNORED (not read, not checked).  The tangents of the folded constants are formed on the host in exact
 * forward mode in double (no difference quotient), as in (22); the fields loggamma_z1 and loggamma_z2 of pdf_c are read as fields, so a direction along
 * ν_c or μ_c moves them too (cmx.parameters.column_parameter_direction does).
 * The Chen-2022 table (vel.chen2022: a, b, c, rho_0, a3_pow, b_rho) is HELD FIXED: any non-zero component of a direction there is CMX_ERR_UNSUPPORTED,
 * whatever the flags (the fitted instantiation takes it through a polynomial fit of log2 Γ, which has no derivative here; the general one would need ψ on the
 * device).  With CMX_VEL_CHEN2022 every other parameter still reaches the fluxes through λ, the limiters and π ρ_w.
 * Arguments: the head of the (2b) entries through n_rai; then
 *   jvp:  ndir (1 … CMX_PARAM_MAX_DIRS), the four direction tables, jvp[ndir·4] (direction-major, then cmx_sb2006_jac_out), jvp_precip[ndir] (columns of
 *         n_col values), tendencies[4], precip_flux.  Every output table, member and column may be NULL; no output at all is CMX_ERR_BAD_ARG.
 *   vjp:  cotangents[4] (the table or a member NULL: absent), cot_precip (n_col values or NULL), ndir, the direction tables, grad (ndir doubles, device),
 *         workspace (ndir·CMX_PARAM_VJP_PARTIALS doubles, device), tendencies[4], precip_flux.
 * Statuses, in order: the parameter pointers and counts, the flags, the limit on n_col·n_lev [jvp: n_col = 0 is CMX_OK here], the columns, ndir and
 * d_warm_rain, [vjp: grad and workspace], the outputs (none may be an input column, inv_dz or a cotangent: a lane reads its neighbours), a non-finite
 * component of a direction (CMX_ERR_BAD_ARG), a direction on the Chen-2022 table (CMX_ERR_UNSUPPORTED), the limiters and the fall-speed parameters as in
 * (2b).  n_col = 0 of the gradient entry passes all of these but the columns and writes zeros to grad.
 * The rules of (22) and (25) hold: a direction on acnv.b, accr.c or self.d selects the general-exponent instantiation for the whole call; the derivative is
 * that of the branch taken; a NaN in a state input of a point poisons that point's outputs, a NaN in an input of the fluxes reaches the cell below and the
 * precipitation outputs, and in the gradient any such NaN — or one in a cotangent — makes every grad[d] NaN.
 * Requested `tendencies` and `precip_flux` are those of the (2b) entry bit for bit when no direction touches an exponent.  A jvp column's bits and a grad
 * value's bits do not depend on ndir, on which other directions are in the call, or on how the call is split into launches; the gradient is a fixed-order
 * reduction without atomics (the decomposition of (22)), bit-identical from run to run.  No allocation, graph-capturable.
 * Not shipped: the Float64 GRADIENT entry with a Chen-2022 table that takes the general instantiation (run-time Γ) returns CMX_ERR_UNSUPPORTED — its kernel
 * needs 482–511 vector registers at one direction per evaluation and spills 8; the jvp entry serves that case (264–278).
 * Not done here: the 1-moment column — (28); its state products: (27) —, the 2M + P3 column, the implicit column steps, derivatives with respect to ρ or inv_dz, of the
 * Chen-2022 table, second derivatives.  cmx_version() stays at 0.5 (no struct layout changed; an older library fails on the symbol lookup).
 * ------------------------------------------------------------------------- */
int32_t cmx_sb2006_column_param_jvp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                        const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                        const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai, int32_t ndir,
                                        const cmx_warm_rain_2m_f32 *d_warm_rain, const cmx_thermo_f32 *d_tps, const cmx_rain_vel_f32 *d_vel,
                                        const cmx_stokes_vel_f32 *d_cloud_vel, float *const *jvp, float *const *jvp_precip,
                                        float *const tendencies[CMX_SB2006_JAC_NOUT], float *precip_flux, void *stream);
int32_t cmx_sb2006_column_param_vjp_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                        const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                        const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai, const float *n_rai,
                                        const float *const cotangents[CMX_SB2006_JAC_NOUT], const float *cot_precip, int32_t ndir,
                                        const cmx_warm_rain_2m_f32 *d_warm_rain, const cmx_thermo_f32 *d_tps, const cmx_rain_vel_f32 *d_vel,
                                        const cmx_stokes_vel_f32 *d_cloud_vel, double *grad, double *workspace,
                                        float *const tendencies[CMX_SB2006_JAC_NOUT], float *precip_flux, void *stream);
int32_t cmx_sb2006_column_param_jvp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                        const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                        const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai, int32_t ndir,
                                        const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps, const cmx_rain_vel_f64 *d_vel,
                                        const cmx_stokes_vel_f64 *d_cloud_vel, double *const *jvp, double *const *jvp_precip,
                                        double *const tendencies[CMX_SB2006_JAC_NOUT], double *precip_flux, void *stream);
int32_t cmx_sb2006_column_param_vjp_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                        const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                        const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai, const double *n_rai,
                                        const double *const cotangents[CMX_SB2006_JAC_NOUT], const double *cot_precip, int32_t ndir,
                                        const cmx_warm_rain_2m_f64 *d_warm_rain, const cmx_thermo_f64 *d_tps, const cmx_rain_vel_f64 *d_vel,
                                        const cmx_stokes_vel_f64 *d_cloud_vel, double *grad, double *workspace,
                                        double *const tendencies[CMX_SB2006_JAC_NOUT], double *precip_flux, void *stream);

/* ---------------------------------------------------------------------------
 * (27) The products J v and Jᵀḡ with the Jacobian of the 1-moment COLUMN step cmx_mp1m_column_tendencies_sedimentation_* in Instantaneous mode (nsub = 0) —
 * tendencies, the four fall speeds and the upwind flux divergence in one call, plus the surface fluxes of rain and snow — with respect to the prognostic
 * state: cmx_mp1m_column_jvp_* and cmx_mp1m_column_vjp_*.  (17) differentiates the point function, which knows nothing of the fall speeds; these differentiate
 * what a mixed-phase host model steps.  J v is the matvec of a Newton–Krylov solver that treats 1-moment microphysics and sedimentation implicitly together;
 * Jᵀḡ with the cotangents of the two precipitation fluxes is what loss(precip_rai + precip_sno).backward() needs (cmx.autograd).
 * The function that is differentiated, normative — per column, level 0 the lowest, x_k = (T, q_tot, q_lcl, q_icl, q_rai, q_sno)_k:
 *     out_k  = tend(ρ_k, x_k) + g_k·(F_{k+1} − F_k)        g_k = inv_dz[k]/ρ_k, formed exactly as the primal kernel forms it: inv_dz[k]·rcp(max(0, ρ_k))
 *     F_{n_lev} = 0        precip_rai = F_0[q_rai]        precip_sno = F_0[q_sno]
 * tend is the Instantaneous 1-moment tendencies (15).  F_k[s] = ρ⁺χ⁺w_s for s = q_lcl, q_icl, q_rai, q_sno — the fluxes of the primal entry: Stokes cloud
 * liquid, Chen-2022 small ice, Chen-2022 rain, Chen-2022 large ice with the fixed aspect ratio.  ρ and inv_dz are held FIXED, as ρ is in (14) – (19).
 * The clamps of the inputs, the ε gates, the floors and the max(0, w) of the fall speeds are part of the function; the derivative is that of the branch taken,
 * as in (15).  Γ(b(ρ) + …) of the Chen-2022 rain curve depends on ρ only: it is evaluated on the value and carries no tangent, in the fitted and in the
 * general (run-time Γ) instantiation alike.
 * With Ḟ_k = (∂F_k/∂x_k)·v_k, and J_pt the Jacobian of tend at the point:
 *     J v:    ẏ_k = J_pt(x_k)·v_k + g_k·(Ḟ_{k+1} − Ḟ_k)          ṗ_rai = Ḟ_0[q_rai], ṗ_sno = Ḟ_0[q_sno], one value per column each
 *     Jᵀḡ:    x̄_k = J_pt(x_k)ᵀ·ḡ_k + (∂F_k/∂x_k)ᵀ·λ_k            λ_k[s] = −g_k·ḡ_k[s] + [k > 0]·g_{k−1}·ḡ_{k−1}[s] + [k = 0]·p̄_s
 * for each falling species s; p̄_s is the cotangent of the precipitation flux of s, non-zero for rain and snow only.  F_k[s] depends on ρ_k and on its own
 * species (q_s)_k alone: ∂F_k/∂x_k has the one entry ∂F_k[s]/∂q_s per species, the block Jacobian is upper bidiagonal in the level index and never couples
 * two columns.
 * Arguments: the head of cmx_mp1m_column_tendencies_sedimentation_* through `in` (a HOST array of the 7 device columns rho, T, q_tot, q_lcl, q_icl, q_rai,
 * q_sno; n_col columns of n_lev contiguous levels) WITHOUT q_min, dt and nsub — Instantaneous mode only; then
 *   jvp:  tangents[6] in the order of cmx_mp1m_jac_wrt (the table or a member NULL: a zero tangent), jvp[4] in the order of cmx_mp1m_jac_out, jvp_precip_rai,
 *         jvp_precip_sno (n_col values each), tendencies[4], precip_rai, precip_sno;
 *   vjp:  cotangents[4] (the table or a member NULL: that output is structurally absent from the sum), cot_precip_rai, cot_precip_sno (n_col values or
 *         NULL: absent), grad[6], tendencies[4], precip_rai, precip_sno.
 * Every output table, every member and every output column may be NULL; a call with no output at all is CMX_ERR_BAD_ARG, and so is an output that is one of
 * the call's input columns, inv_dz, a tangent or a cotangent (a lane reads its neighbours).  n_col·n_lev is limited as in the primal entry; n_col = 0 is
 * CMX_OK.  Statuses in the primal entry's order: the parameter pointers and counts, both snow-shape bits (CMX_ERR_BAD_ARG), the Microphysics1MOptions bits
 * exactly as the primal entry checks them, a single snow-shape bit (CMX_ERR_UNSUPPORTED, below), the limit, n_col = 0, the columns, the outputs.
 * Requested `tendencies` and `precip_*` are those of the primal entry on the same columns with nsub = 0, bit for bit; the instantiation is the one the primal
 * chooses (default options or run-time flags; fitted or general Γ of the Chen-2022 rain table).  The products are plain IEEE arithmetic on the tangents: Jᵀḡ
 * accumulates the point sums with ḡ in output order, then — in the gradient of q_s only — the one flux term λ_k[s]·∂F_k[s]/∂q_s, as one chain of fma seeded
 * with −0 (no term at all: +0); each gradient comes from its own tangent slot, so its bits do not depend on which other gradients are requested.  T and q_tot
 * do not enter the fluxes.  With inv_dz ≡ 0 the products equal those of (17) under == wherever the flux tangents are finite.
 * NaN rule: the poison rule of the 1-moment entries holds per point — a NaN in any state input (Float64: also ρ ≤ 0), or in any given tangent or cotangent
 * value of the point (p̄ counts for the level-0 point), gives NaN in every output of that point.  A NaN in ρ or in a species' q (Float64: ρ ≤ 0) reaches the
 * cell below through F and Ḟ of that species exactly as in the primal, and the column's precipitation outputs at level 0; a NaN tangent reaches Ḟ by plain
 * IEEE arithmetic.  In Jᵀḡ a NaN in ḡ_{k−1}[s] reaches the gradient of q_s at level k by plain IEEE propagation through λ_k[s]; a NaN in ρ_{k−1} makes
 * g_{k−1} what the primal makes it — max(0, NaN) = 0, its reciprocal +Inf — and the flux terms of x̄_k non-finite.  There is no other rule.
 * Results do not depend on how the kernels divide the columns among workgroups, on alignment, or on the number of columns in the call.  Both entries are
 * pure launches on `stream`: no allocation, no synchronisation, graph-capturable.
 * Not done here: the LinearizedAverage mode (nsub > 0); the implicit column steps (20), (21); the snow shapes — a CMX_1M_SED_SNOW_OBLATE / _PROLATE bit returns
 * CMX_ERR_UNSUPPORTED: the oracle's column step has no shaped snow to difference against —; parameter derivatives of this column step — (28) —; derivatives with
 * respect to ρ or inv_dz; the 2M + P3 column.  cmx_version() stays at 0.5 (no struct layout changed; an older library fails on the symbol lookup).
 * ------------------------------------------------------------------------- */
int32_t cmx_mp1m_column_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int64_t n_col,
                                int32_t n_lev, const float *inv_dz, const float *const *in, const float *const tangents[CMX_MP1M_JAC_NWRT],
                                float *const jvp[CMX_MP1M_JAC_NOUT], float *jvp_precip_rai, float *jvp_precip_sno,
                                float *const tendencies[CMX_MP1M_JAC_NOUT], float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int64_t n_col,
                                int32_t n_lev, const double *inv_dz, const double *const *in, const double *const tangents[CMX_MP1M_JAC_NWRT],
                                double *const jvp[CMX_MP1M_JAC_NOUT], double *jvp_precip_rai, double *jvp_precip_sno,
                                double *const tendencies[CMX_MP1M_JAC_NOUT], double *precip_rai, double *precip_sno, void *stream);
int32_t cmx_mp1m_column_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int64_t n_col,
                                int32_t n_lev, const float *inv_dz, const float *const *in, const float *const cotangents[CMX_MP1M_JAC_NOUT],
                                const float *cot_precip_rai, const float *cot_precip_sno, float *const grad[CMX_MP1M_JAC_NWRT],
                                float *const tendencies[CMX_MP1M_JAC_NOUT], float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int64_t n_col,
                                int32_t n_lev, const double *inv_dz, const double *const *in, const double *const cotangents[CMX_MP1M_JAC_NOUT],
                                const double *cot_precip_rai, const double *cot_precip_sno, double *const grad[CMX_MP1M_JAC_NWRT],
                                double *const tendencies[CMX_MP1M_JAC_NOUT], double *precip_rai, double *precip_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (28) The derivatives of the 1-moment COLUMN step (27) with respect to the scheme's PARAMETERS, the fall-speed parameters and the two surface
 * precipitation fluxes included: cmx_mp1m_column_param_jvp_* (per point, J_θ·δθ) and cmx_mp1m_column_param_vjp_* (the reduced gradient dL/dθ).  (23) stops
 * at the point function, which knows nothing of the fall speeds; (27) reaches the state but not θ.  This is what loss(precip_rai + precip_sno).backward()
 * needs to reach `theta` (cmx.autograd), and where the parameters that act through sedimentation only — the Stokes cloud fall speed, the sedimentation
 * number concentrations, the apparent densities of cloud ice and snow, ϕ, κ and the Chen-2022 coefficients — get a derivative at all.
 * The function is that of (27), normative, with the state, ρ and inv_dz held FIXED and θ = the floating fields of the five parameter structs:
 *     out_k = tend(ρ_k, x_k; θ) + g_k·(F_{k+1}(θ) − F_k(θ))        F_{n_lev} = 0        precip_rai = F_0[q_rai]        precip_sno = F_0[q_sno]
 * With Ḟ_k = ∂F_k/∂θ·δθ:
 *     J_θ δθ:    ẏ_k = ∂tend/∂θ·δθ + g_k·(Ḟ_{k+1} − Ḟ_k)          ṗ_rai = Ḟ_0[q_rai], ṗ_sno = Ḟ_0[q_sno], one value per column each
 *     gradient:  grad[d] = Σ_columns Σ_k ( Σ_o ḡ_{o,k}·(∂tend_o/∂θ·δθ⁽ᵈ⁾)_k + Σ_s λ_k[s]·Ḟ_k[s]⁽ᵈ⁾ ),  λ_k exactly that of (27), p̄_rai and p̄_sno at level 0
 * A DIRECTION is five structs of the entry's own types holding δθ: d_mp[ndir] (required), d_tps[ndir], d_stokes[ndir], d_chen_rain[ndir],
 * d_chen_ice[ndir] (each of the last four may be NULL: zero).  The tangents of the folded constants are formed on the host in exact forward mode in double
 * (no difference quotient), as in (22), (23) and (26).
 * What carries a tangent: every floating field of cmx_microphysics_1m and cmx_thermo that (23) differentiates; the fields of `mp` only the fall speeds read —
 * cloud_liquid.N_0, cloud_liquid.rho_w, cloud_ice.N_0, cloud_ice.rho_i, snow.rho_i, snow.phi, snow.kappa — and the slope-parameter fields; cmx_stokes_vel
 * (grav, nu_air, rho_w); every coefficient of chen_ice.small_ice (A, B, C, E, F, G) and .large_ice (A, B, C, E, F, G, H) through the closed forms that
 * reduce the tables at the apparent densities, Γ(C_l + 4) and Γ(F_l + 4) with Γ·ψ; of chen_rain a[3], c[3], rho_0 and a3_pow.
 * HELD FIXED: chen_rain.b[3] and chen_rain.b_rho.  They reach the fall speed through Γ(b − b_ρ ρ + 4), a polynomial fit in ρ in the fitted instantiation and
 * a run-time Γ in the general one, neither with a derivative on the device: any non-zero component of a direction there is CMX_ERR_UNSUPPORTED, whatever
 * the flags; Γ is evaluated on the value and carries no tangent in both instantiations, as in (27).  The `cutoff` fields of the ice tables are not read by
 * this step: a direction there contributes nothing.
 * Arguments: the head of the (27) entries through `in` (mp, tps, stokes, chen_rain, chen_ice, flags, n_col, n_lev, inv_dz, the HOST array of the 7 device
 * columns); then
 *   jvp:  ndir (1 … CMX_PARAM_MAX_DIRS), the five direction tables, jvp[ndir·4] (direction-major, then cmx_mp1m_jac_out), jvp_precip_rai[ndir],
 *         jvp_precip_sno[ndir] (tables of columns of n_col values), tendencies[4], precip_rai, precip_sno.  Every output table, member and column may be
 *         NULL; no output at all is CMX_ERR_BAD_ARG.
 *   vjp:  cotangents[4] (the table or a member NULL: absent), cot_precip_rai, cot_precip_sno (n_col values or NULL: absent), ndir, the five direction
 *         tables, grad (ndir doubles, device), workspace (ndir·CMX_PARAM_VJP_PARTIALS doubles, device), tendencies[4], precip_rai, precip_sno.
 * Statuses, in order: those of (27) — the parameter pointers and counts, both snow-shape bits (CMX_ERR_BAD_ARG), the Microphysics1MOptions bits, a single
 * snow-shape bit (CMX_ERR_UNSUPPORTED), the limit on n_col·n_lev [jvp: n_col = 0 is CMX_OK here], the columns —, ndir and d_mp, [vjp: grad and
 * workspace], the outputs (none may be an input column, inv_dz or a cotangent: a lane reads its neighbours), a non-finite component of a direction
 * (CMX_ERR_BAD_ARG), a direction on b or b_ρ (CMX_ERR_UNSUPPORTED).  n_col = 0 of the gradient entry passes all of these but the columns and writes zeros
 * to grad.
 * The instantiation is the one the primal entry selects (default options or run-time flags, fitted or general Γ); a direction on one of the nine
 * slope-parameter exponents that the default-options instantiation holds at compile time selects the run-time-flags instantiation for the whole call (23).
 * Requested `tendencies` and `precip_*` are those of the primal entry (nsub = 0) bit for bit when no direction moves such an exponent.  A jvp column's bits
 * and a grad value's bits do not depend on ndir, on which other directions are in the call, or on how the call is split into launches; the gradient is a
 * fixed-order reduction in double without atomics (the decomposition of (22)), bit-identical from run to run.  With inv_dz ≡ 0 and directions on mp and
 * tps only the four jvp rows equal those of (23) under == wherever the flux tangents of the point and of the point above are finite.
 * NaN rule: the point and flux poison rules of (27); in the gradient any such NaN, or a NaN in a cotangent, makes every grad[d] NaN (26).
 * Pure launches on `stream`: no allocation, graph-capturable.
 * Not done here: the LinearizedAverage mode (nsub > 0); the implicit column steps (20), (21); the snow shapes; derivatives with respect to ρ or inv_dz; b
 * and b_ρ of the Chen-2022 rain table; the 2M + P3 column; second derivatives; tuning beyond the choice of the directions per evaluation.  cmx_version()
 * stays at 0.5 (no struct layout changed; an older library fails on the symbol lookup).
 * ------------------------------------------------------------------------- */
int32_t cmx_mp1m_column_param_jvp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                        const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int64_t n_col,
                                        int32_t n_lev, const float *inv_dz, const float *const *in, int32_t ndir, const cmx_microphysics_1m_f32 *d_mp,
                                        const cmx_thermo_f32 *d_tps, const cmx_stokes_vel_f32 *d_stokes, const cmx_chen2022_rain_vel_f32 *d_chen_rain,
                                        const cmx_chen2022_ice_vel_f32 *d_chen_ice, float *const *jvp, float *const *jvp_precip_rai, float *const *jvp_precip_sno,
                                        float *const tendencies[CMX_MP1M_JAC_NOUT], float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_param_vjp_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                        const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int64_t n_col,
                                        int32_t n_lev, const float *inv_dz, const float *const *in, const float *const cotangents[CMX_MP1M_JAC_NOUT],
                                        const float *cot_precip_rai, const float *cot_precip_sno, int32_t ndir, const cmx_microphysics_1m_f32 *d_mp,
                                        const cmx_thermo_f32 *d_tps, const cmx_stokes_vel_f32 *d_stokes, const cmx_chen2022_rain_vel_f32 *d_chen_rain,
                                        const cmx_chen2022_ice_vel_f32 *d_chen_ice, double *grad, double *workspace, float *const tendencies[CMX_MP1M_JAC_NOUT],
                                        float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_param_jvp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                        const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int64_t n_col,
                                        int32_t n_lev, const double *inv_dz, const double *const *in, int32_t ndir, const cmx_microphysics_1m_f64 *d_mp,
                                        const cmx_thermo_f64 *d_tps, const cmx_stokes_vel_f64 *d_stokes, const cmx_chen2022_rain_vel_f64 *d_chen_rain,
                                        const cmx_chen2022_ice_vel_f64 *d_chen_ice, double *const *jvp, double *const *jvp_precip_rai, double *const *jvp_precip_sno,
                                        double *const tendencies[CMX_MP1M_JAC_NOUT], double *precip_rai, double *precip_sno, void *stream);
int32_t cmx_mp1m_column_param_vjp_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                        const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int64_t n_col,
                                        int32_t n_lev, const double *inv_dz, const double *const *in, const double *const cotangents[CMX_MP1M_JAC_NOUT],
                                        const double *cot_precip_rai, const double *cot_precip_sno, int32_t ndir, const cmx_microphysics_1m_f64 *d_mp,
                                        const cmx_thermo_f64 *d_tps, const cmx_stokes_vel_f64 *d_stokes, const cmx_chen2022_rain_vel_f64 *d_chen_rain,
                                        const cmx_chen2022_ice_vel_f64 *d_chen_ice, double *grad, double *workspace, double *const tendencies[CMX_MP1M_JAC_NOUT],
                                        double *precip_rai, double *precip_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (29) Parameter ENSEMBLES: one launch evaluates E parameter sets ("members") of the SB2006 warm-rain tendencies (1), the 1-moment tendencies (5), the SB2006
 * column step (7) and the unshaped 1-moment column step (8b) — what an ensemble Kalman inversion, a perturbed-parameter ensemble or E single-column models
 * pay E launches and E host-side folds for with the single entries.  Member e's outputs equal, BIT FOR BIT, the single entry called with member e's
 * parameters on member e's state: the kernels run the single entries' own code on the same operands; only the constants come from a table in device
 * memory instead of the kernel arguments.
 *
 * The library stays stateless and every entry a pure sequence of launches, so the table is built in two steps.
 *
 * PACK (host only, no HIP call): cmx_sb2006_ensemble_pack_* and cmx_mp1m_ensemble_pack_* take ARRAYS of n_members parameter structs of the single
 * entries' types and the single entries' `flags`, run the single entries' folds and argument checks member by member (the first member that fails a
 * check gives that check's status), and write one constants block per member into the caller's HOST buffer `table` (table_bytes ≥ n_members · stride,
 * stride = cmx_*_ensemble_table_stride_*(), a multiple of 16 bytes; CMX_ERR_BAD_ARG otherwise) and the plain struct cmx_ensemble_desc.  Block e is a
 * function of member e alone — packing [A, B] and packing [B] give the same bytes for B — so one member is updated by re-packing it alone and copying
 * its stride bytes.  One block serves the pointwise and the column entry of its scheme.
 *   SB2006: warm_rain[E], tps[E]; vel[E] or NULL (NULL: no fall speed — the table serves the pointwise entry without vt_rai_* only; otherwise exactly
 *     one of CMX_VEL_SB2006 / CMX_VEL_CHEN2022 in flags); cloud_vel[E] or NULL (NULL: the column entry runs without cloud sedimentation).
 *   1-moment: mp[E], tps[E]; stokes[E], chen_rain[E], chen_ice[E] — all three, or all three NULL when the table is for the pointwise entry only.
 *     A snow-shape bit (CMX_1M_SED_SNOW_*) in flags is CMX_ERR_UNSUPPORTED.
 * ALL MEMBERS OF ONE TABLE RUN ONE KERNEL INSTANTIATION.  The single entries choose theirs from parameter VALUES: the integer SB2006 exponents
 * (b = 3, c = 4, d = −5), the fitted or general Γ of a Chen-2022 rain table (here and in the 1-moment fall speeds), the default-options or run-time-flags
 * form of the 1-moment scheme.  If two members differ in one of these choices pack returns CMX_ERR_UNSUPPORTED — perturb such a member in its own table;
 * a table that falls back to the general instantiations would not be bit-identical to the single entries.
 * The caller copies n_members · stride bytes to the device however it likes (hipMemcpyAsync on the stream of the calls orders the update) and passes
 * the desc (host) and the device pointer.  The table is an ordinary device buffer the kernels only read: calls stay graph-capturable, and a captured
 * graph sees a table updated in place between replays.
 *
 * ENSEMBLE ENTRIES: (desc, table, n_members, ens_flags), then the single entry's array arguments; sizes (n_points resp. n_col, n_lev) are PER MEMBER.
 * Outputs are member-major: member e owns points [e·n, (e+1)·n) of every output column and columns [e·n_col, (e+1)·n_col) of the precipitation fluxes.
 * Inputs are member-major too (every member its own state) or, with CMX_ENSEMBLE_SHARED_STATE, of length n: every member reads the same state (the
 * loads then drop the non-temporal hint: the other members' workgroups want the lines from L2).  inv_dz (n_lev values) is always shared; q_min, dt and
 * nsub of the 1-moment column step are shared.  Optional outputs stay NULL-able as in the single entries (vt_rai_n, vt_rai_m — a table packed without
 * `vel` cannot give them: CMX_ERR_BAD_ARG —, the precipitation fluxes).  The column halo never crosses a member: the last column of a member takes a
 * zero inflow at its top and the next member's first point is not read.  Any alignment is accepted (per-member scalar head, vector body, scalar tail, or
 * one point per lane throughout when the columns' offsets differ) and does not change a bit.
 * Statuses, in order: NULL desc or table (CMX_ERR_BAD_ARG); the counts as in the single entry (negative: CMX_ERR_BAD_ARG; above the single entry's limit
 * PER MEMBER: CMX_ERR_UNSUPPORTED; 1-moment column: nsub < 0, and dt ≤ 0 or q_min < 0 with nsub > 0: CMX_ERR_BAD_ARG); wrong magic, scheme or float type,
 * n_members < 1 or ≠ desc->n_members, a stride or flags the library would not have packed, unknown ens_flags bits (CMX_ERR_BAD_ARG); n_members > 65535,
 * the y limit of a grid (CMX_ERR_UNSUPPORTED); a per-member size of 0 (CMX_OK); a NULL required array, the column entries on a table packed without their
 * fall-speed parameters (CMX_ERR_BAD_ARG).  `table` is never dereferenced on the host.
 *
 * THE IMPLICIT COLUMN STEPS (21) — what a single-column model at Δt of minutes calls — have ensemble forms too:
 * cmx_sb2006_column_implicit_step_ensemble_* and cmx_mp1m_column_implicit_step_ensemble_* take (desc, table, n_members, ens_flags), then
 * (dt, nsub, step_flags, n_col, n_lev, inv_dz) and the arrays of the (21) entry.  The contract is the one above: member e of every output has the bits of the
 * (21) entry called with member e's parameters on member e's state; sizes per member, outputs and fluxes member-major, inputs member-major or shared;
 * inv_dz, dt, nsub and step_flags are shared by all members; the precipitation fluxes stay NULL-able; the outputs must not alias the state; the recurrence
 * never crosses a member (a workgroup owns whole columns of one member).  The latent heating of the substeps uses Lv = LH_v0/cp_d and Ls = LH_s0/cp_d of
 * member e's `tps`: the 1-moment block holds them already, the SB2006 block holds them after the cloud fall-speed constants (the SB2006 stride grew by
 * two values; callers read it from cmx_sb2006_ensemble_table_stride_*).  The options come from the desc: limited, integer exponents, velocity kind and
 * cloud sedimentation (SB2006); default-options or run-time-flags form and fitted or general Γ (1-moment).  The kernel runs one point per lane, so there is no
 * alignment split and any alignment is accepted.
 * Statuses, in order: NULL desc or table (CMX_ERR_BAD_ARG); n_col < 0 or n_lev < 1 (CMX_ERR_BAD_ARG), n_col > the single entry's limit per member
 * (CMX_ERR_UNSUPPORTED); the descriptor checks above; n_col = 0 (CMX_OK); a NULL required array or a table packed without the fall-speed parameters
 * (CMX_ERR_BAD_ARG); Δt, nsub and the step flags as the (21) entries check them (CMX_ERR_BAD_ARG).
 *
 * Not done here: ensemble forms of the derivative entries, of the pointwise implicit average (19) and of the column step with explicit fluxes (20), 2M + P3,
 * the snow-shaped 1-moment column step, the parcel model (it has per-parcel coefficients); per-member Δt or nsub; tables of mixed instantiations; sharding
 * members over devices.  cmx_version() stays at 0.5 (no struct of the interface changed layout; an older library fails on the symbol lookup).
 * ------------------------------------------------------------------------- */
#define CMX_ENSEMBLE_SHARED_STATE (1u << 0)
#define CMX_ENSEMBLE_MAGIC 0x434d5845u      /* "CMXE" */
#define CMX_ENSEMBLE_SCHEME_SB2006 1u
#define CMX_ENSEMBLE_SCHEME_MP1M 2u
typedef struct cmx_ensemble_desc {
    uint32_t magic;              /* CMX_ENSEMBLE_MAGIC */
    uint32_t scheme;             /* CMX_ENSEMBLE_SCHEME_* */
    uint32_t float_type;         /* 4: the _f32 family, 8: the _f64 family */
    uint32_t flags;              /* the `flags` the table was packed with */
    int32_t n_members;
    uint32_t stride;             /* bytes from one member's block to the next */
    /* the dispatch choices made from parameter values, equal for all members */
    uint32_t integer_exponents;  /* SB2006: b = 3, c = 4, d = −5 */
    uint32_t vel_kind;           /* SB2006: 0 no fall speed, 1 SB2006, 2 Chen-2022 (fitted Γ), 3 Chen-2022 (general Γ) */
    uint32_t cloud_vel;          /* SB2006: packed with cloud_vel (the column entry sediments cloud droplets) */
    uint32_t runtime_flags;      /* 1-moment: the run-time-flags instantiation (0: the default-options one) */
    uint32_t sedimentation;      /* 1-moment: packed with stokes, chen_rain, chen_ice (the column entry is served) */
    uint32_t general_gamma;      /* 1-moment: run-time Γ of the Chen-2022 rain fall speed */
    uint32_t reserved[4];
} cmx_ensemble_desc;
int32_t cmx_sb2006_ensemble_table_stride_f32(void);
int32_t cmx_sb2006_ensemble_table_stride_f64(void);
int32_t cmx_mp1m_ensemble_table_stride_f32(void);
int32_t cmx_mp1m_ensemble_table_stride_f64(void);
int32_t cmx_sb2006_ensemble_pack_f32(const cmx_warm_rain_2m_f32 *warm_rain, const cmx_thermo_f32 *tps, const cmx_rain_vel_f32 *vel,
                                     const cmx_stokes_vel_f32 *cloud_vel, uint32_t flags, int32_t n_members, void *table, int64_t table_bytes,
                                     cmx_ensemble_desc *desc);
int32_t cmx_sb2006_ensemble_pack_f64(const cmx_warm_rain_2m_f64 *warm_rain, const cmx_thermo_f64 *tps, const cmx_rain_vel_f64 *vel,
                                     const cmx_stokes_vel_f64 *cloud_vel, uint32_t flags, int32_t n_members, void *table, int64_t table_bytes,
                                     cmx_ensemble_desc *desc);
int32_t cmx_mp1m_ensemble_pack_f32(const cmx_microphysics_1m_f32 *mp, const cmx_thermo_f32 *tps, const cmx_stokes_vel_f32 *stokes,
                                   const cmx_chen2022_rain_vel_f32 *chen_rain, const cmx_chen2022_ice_vel_f32 *chen_ice, uint32_t flags, int32_t n_members,
                                   void *table, int64_t table_bytes, cmx_ensemble_desc *desc);
int32_t cmx_mp1m_ensemble_pack_f64(const cmx_microphysics_1m_f64 *mp, const cmx_thermo_f64 *tps, const cmx_stokes_vel_f64 *stokes,
                                   const cmx_chen2022_rain_vel_f64 *chen_rain, const cmx_chen2022_ice_vel_f64 *chen_ice, uint32_t flags, int32_t n_members,
                                   void *table, int64_t table_bytes, cmx_ensemble_desc *desc);
int32_t cmx_sb2006_warm_rain_tendencies_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                     int64_t n_points, const float *rho, const float *T, const float *q_tot, const float *q_lcl,
                                                     const float *n_lcl, const float *q_rai, const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt,
                                                     float *dq_rai_dt, float *dn_rai_dt, float *vt_rai_n, float *vt_rai_m, void *stream);
int32_t cmx_sb2006_warm_rain_tendencies_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                     int64_t n_points, const double *rho, const double *T, const double *q_tot, const double *q_lcl,
                                                     const double *n_lcl, const double *q_rai, const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt,
                                                     double *dq_rai_dt, double *dn_rai_dt, double *vt_rai_n, double *vt_rai_m, void *stream);
int32_t cmx_mp1m_tendencies_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n_points,
                                         const float *rho, const float *T, const float *q_tot, const float *q_lcl, const float *q_icl, const float *q_rai,
                                         const float *q_sno, float *dq_lcl_dt, float *dq_icl_dt, float *dq_rai_dt, float *dq_sno_dt, void *stream);
int32_t cmx_mp1m_tendencies_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, int64_t n_points,
                                         const double *rho, const double *T, const double *q_tot, const double *q_lcl, const double *q_icl,
                                         const double *q_rai, const double *q_sno, double *dq_lcl_dt, double *dq_icl_dt, double *dq_rai_dt,
                                         double *dq_sno_dt, void *stream);
int32_t cmx_sb2006_column_tendencies_sedimentation_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                                int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho, const float *T,
                                                                const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai,
                                                                const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt,
                                                                float *dn_rai_dt, float *precip_flux, void *stream);
int32_t cmx_sb2006_column_tendencies_sedimentation_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                                int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho, const double *T,
                                                                const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                                                const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt,
                                                                double *dn_rai_dt, double *precip_flux, void *stream);
int32_t cmx_mp1m_column_tendencies_sedimentation_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                              float q_min, float dt, int32_t nsub, int64_t n_col, int32_t n_lev, const float *inv_dz,
                                                              const float *const *in, float *const *out, float *precip_rai, float *precip_sno,
                                                              void *stream);
int32_t cmx_mp1m_column_tendencies_sedimentation_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags,
                                                              double q_min, double dt, int32_t nsub, int64_t n_col, int32_t n_lev, const double *inv_dz,
                                                              const double *const *in, double *const *out, double *precip_rai, double *precip_sno,
                                                              void *stream);
int32_t cmx_sb2006_column_implicit_step_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                     int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *rho,
                                                     const float *T, const float *q_tot, const float *q_lcl, const float *n_lcl, const float *q_rai,
                                                     const float *n_rai, float *dq_lcl_dt, float *dn_lcl_dt, float *dq_rai_dt, float *dn_rai_dt,
                                                     float *precip_flux, void *stream);
int32_t cmx_sb2006_column_implicit_step_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                     int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *rho,
                                                     const double *T, const double *q_tot, const double *q_lcl, const double *n_lcl, const double *q_rai,
                                                     const double *n_rai, double *dq_lcl_dt, double *dn_lcl_dt, double *dq_rai_dt, double *dn_rai_dt,
                                                     double *precip_flux, void *stream);
int32_t cmx_mp1m_column_implicit_step_ensemble_f32(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                   int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const float *inv_dz, const float *const *in,
                                                   float *const *out, float *precip_rai, float *precip_sno, void *stream);
int32_t cmx_mp1m_column_implicit_step_ensemble_f64(const cmx_ensemble_desc *desc, const void *table, int32_t n_members, uint32_t ens_flags, double dt,
                                                   int32_t nsub, uint32_t step_flags, int64_t n_col, int32_t n_lev, const double *inv_dz, const double *const *in,
                                                   double *const *out, double *precip_rai, double *precip_sno, void *stream);

/* ---------------------------------------------------------------------------
 * (3) Optional diagnostic sums over one rank's shard: Σx of `ncols` (≤ CMX_COLUMN_SUMS_MAX_COLS) device columns of length
 * n, accumulated in double, into `sums[ncols]` (device, double).  ONE launch reduces all columns to CMX_COLUMN_SUMS_PARTIALS partial
 * sums each (`workspace`: ncols · CMX_COLUMN_SUMS_PARTIALS doubles of device memory owned by the caller — the library allocates nothing),
 * a second, one-workgroup-per-column launch adds those in a fixed tree.  No floating-point atomics: the result is a pure function of
 * the column contents and n — bit-identical from run to run and from device to device (the decomposition does not depend on the CU
 * count).  It is NOT invariant under re-sharding: a rank count changes the order of additions, so the all-reduced total of 8 shards and
 * the sum of the unsharded column agree to rounding (a few ulp of Σ|x|·2⁻⁵³·log₂ n), not bit for bit.  The caller all-reduces the ≤ 16
 * doubles over RCCL / MPI; the library itself performs no communication.
 * ------------------------------------------------------------------------- */
#define CMX_COLUMN_SUMS_MAX_COLS 16
#define CMX_COLUMN_SUMS_PARTIALS 1024
int32_t cmx_column_sums_f32(int32_t ncols, const float *const *cols, int64_t n, double *sums, double *workspace, void *stream);
int32_t cmx_column_sums_f64(int32_t ncols, const double *const *cols, int64_t n, double *sums, double *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CMX_H */
