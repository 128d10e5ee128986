"""Shared machinery of the parameter sweeps (tests/test_param_sweep_host.py on the CPU, tests/test_param_sweep_gpu.py on the device).

Every other parity test runs the kernels at the ClimaParams defaults.  Between a parameter struct and what a kernel reads sits host code that
folds constants (make_sb_consts, make_mp1m_consts, …), fits polynomials per parameter set (make_chen_gamma / make_chen_log) and picks fast
instantiations from a handful of fields (sb_integer_exponents, mp1m_default_exponents, b_is_3, chen_vel_kind).  The sweep changes ONE parameter
at a time and compares the entry with the oracle evaluated with the same override, so a folded constant that ignores its field, or a fast
instantiation keyed on too few fields, fails by name.

* RecordingDict       the names a family's constructors read — nothing is hand-listed, a parameter added later is swept automatically;
* perturbations()     scalars × 1.25 and × 0.8 (the range of tests/test_point_host.py's perturbed sets), a default of 0 shifted by ZERO_STEP,
                      tuples one element at a time; DOMAIN says which perturbations are skipped to stay inside a scheme's domain;
* liveness()          on the ORACLE ALONE: at how many states the reference moves by more than 10·RTOL — a case that cannot see its parameter
                      proves nothing, so the host test demands ≥ MIN_LIVE states for every parameter in its best entry, or a row in INERT;
* Sweep.check()       parity.scaled_err + parity.plain_stats at parity.RTOL / CTOL with the DEFAULT knobs (family "parameter sweep": the
                      FAMILY_KNOBS were set from default-parameter runs); failures are collected and raised once, with the whole list.
"""
import warnings
from collections import namedtuple

import numpy as np

import parity
from cmx import parameters as P

NPT = {"f32": np.float32, "f64": np.float64}
FAMILY = "parameter sweep"
MIN_LIVE = 50                     # states at which the reference must move for a perturbation to count as seen (condition on the inputs)
LIVE_FACTOR = 10.0                # … by more than 10·RTOL[ft] in the normalised metric of parity.scaled_err
N_POINTWISE = 4099                # four 1024-point Float32 workgroup tiles + a 3-point scalar tail, odd
UP, DOWN = 1.25, 0.8


class RecordingDict(P.ParamDict):
    """A ParamDict that remembers which names were asked for (every constructor of cmx.parameters takes one wherever it takes FT)."""

    def __init__(self, FT, override=None):
        super().__init__(FT, override)
        self.names = []

    def __getitem__(self, k):
        if k not in self.names:
            self.names.append(k)
        return super().__getitem__(k)


def names_read(build, ft="f64"):
    td = RecordingDict(ft)
    build(td)
    return list(td.names)


# additive step of a parameter (or tuple element) whose default is 0 — a scale factor would do nothing
ZERO_STEP = {
    "Chen2022_table_B1_ci": 0.05,                           # c₁ = 0 [1/mm]: the first term gains an exponential cut-off
    "P3_constant_slope_parameterization_value": 0.5,        # μ of the constant slope law
    "mam3_nucleation_w_b_i_ion_induced": 0.05,
}
DEFAULT_ZERO_STEP = 0.1                                     # the δ exponents of the 1-moment size relations (*_delm, *_dela, *_delv)

Perturbation = namedtuple("Perturbation", ["name", "index", "label", "override"])
Perturbation.key = property(lambda p: p.name + ("" if p.index is None else f"[{p.index}]") + " " + p.label)

# Which perturbations leave a scheme's domain.  (name, label or None for both, context or None for every entry, reason) — a perturbation
# that matches is skipped in that context; the other direction, or another context, still sweeps the parameter.
Rule = namedtuple("Rule", ["name", "label", "context", "reason"])
DOMAIN = [
    Rule("SB2006_raindrops_terminal_velocity_coeff_aR", "x1.25", "not-limited SB2006 fall speed",
         "aR·1.25 = 12.06 ≥ bR = 10.3: the not-limited fall speed integrates from r_c = −log(aR/bR)/(2cR) and needs aR < bR "
         "(include/cmx.h Conventions; the entries return CMX_ERR_BAD_ARG); swept with the limited PSD and as ×0.8"),
    Rule("SB2006_raindrops_terminal_velocity_coeff_bR", "x0.8", "not-limited SB2006 fall speed",
         "bR·0.8 = 8.24 ≤ aR = 9.65: as above; swept with the limited PSD and as ×1.25"),
    Rule("latent_heat_vaporization_at_reference", "x1.25", None,
         "LH_v0·1.25 = 3.13e6 > LH_s0 = 2.83e6: the latent heat of fusion LH_s0 − LH_v0 turns negative (melting would release ice); swept as ×0.8"),
    Rule("latent_heat_sublimation_at_reference", "x0.8", None, "LH_s0·0.8 = 2.27e6 < LH_v0 = 2.50e6: as above; swept as ×1.25"),
    Rule("Koop2000_J_hom_coeff4", "x1.25", None,
         "log10 J_hom = c1 + c2 Δ − c3 Δ² + c4 Δ³ grows by 0.25·29180·Δ³ ≈ +287 at the upper edge of the Δa_w window: J_hom [1/m³/s] leaves the Float64 range "
         "(the reference's own value is Inf there); swept as ×0.8"),
    *[Rule(f"mam3_nucleation_{k}_t_n_neutral", "x0.8", "Float32",
           "k_t_n = exp(u − exp(v (T/1000 − w))) with u = 182: at 0.8 v or 0.8 w the inner exponential drops from ≈ 200 to ≈ 70 and k_t_n ≈ e^113 overflows Float32 — "
           "the reference's own Float32 arithmetic is Inf or NaN at EVERY state (AerosolNucleation._ternary_literal_f32; checked by the host test); swept in "
           "Float64 and as ×1.25") for k in ("v", "w")],
    *[Rule(f"Chen2022_table_B3_{k}", label, "P3 ventilation factor",
           "the small-ice fall speed E_s D^… − F_s e^{−G_s D}… turns negative at small D: the reference's ventilation factor takes √ of a negative Reynolds number "
           "(src/Common.jl:511-512: DomainError; the oracle restates it as NaN), the device clamps it at 0 (include/cmx.h at cmx_p3_ice_melt); the other direction, "
           "and the fall-speed and self-collection entries in both directions, sweep the entry")
      for k, label in (("Es[0]", "x1.25"), ("Es[1]", "x1.25"), ("Es[2]", "x0.8"), ("Fs[0]", "x0.8"), ("Fs[1]", "x0.8"), ("Fs[2]", "x1.25"))],
]
# The ordered pairs of the schemes stay ordered under × 1.25 / × 0.8 of one member (checked by test_domain_pairs_stay_ordered):
ORDERED_PAIRS = [
    ("SB2006_raindrops_min_mass", "SB2006_raindrops_max_mass"),
    ("SB2006_raindrops_size_distribution_coeff_N0_min", "SB2006_raindrops_size_distribution_coeff_N0_max"),
    ("SB2006_raindrops_size_distribution_coeff_lambda_min", "SB2006_raindrops_size_distribution_coeff_lambda_max"),
    ("SB2006_raindrops_breakup_mean_diameter_threshold", "SB2006_raindrops_equilibrium_mean_diameter"),
    ("SB2006_cloud_droplets_min_mass", "SB2006_raindrops_min_mass"),
    ("Koop2000_min_delta_aw", "Koop2000_max_delta_aw"),
    ("p_over_sulphuric_acid_solution_T_min", "p_over_sulphuric_acid_solution_T_max"),
]

# Parameters that a constructor reads but no formula of the family evaluates (checked against the reference's source, not this code).
# (family → name → one line).  A parameter that is inert in one entry but live in another entry of its family needs no row.
_NO_WARM_RAIN = "no warm-rain formula reads it (the thermodynamics struct is shared with the ice-phase schemes); live in the 1-moment family"
INERT = {
    "SB2006": {
        "SB2006_rain_distribution_coeff_nu": "νr of the rain PDF struct: read by CloudDiagnostics only (src/CloudDiagnostics.jl:67,103), swept there; no process rate reads it",
        "SB2006_rain_distribution_coeff_mu": "μr of the rain PDF struct: as νr",
        "sublimation_deposition_timescale": "subdep_tau_relax of WarmRainParams2M: read by the 2M + P3 method only (ice deposition), which the sweep leaves out; live in the 1-moment family",
        "gas_constant_dry_air": "R_d: no formula of the replaced subsystems reads it except ARG2000's q_vs (swept there)",
        "isobaric_specific_heat_ice": _NO_WARM_RAIN, "latent_heat_sublimation_at_reference": _NO_WARM_RAIN, "temperature_water_freeze": _NO_WARM_RAIN,
        "isochoric_specific_heat_liquid": _NO_WARM_RAIN,
    },
    "1-moment": {
        "liquid_cloud_effective_radius": "r_eff of CloudLiquid: only CloudDiagnostics.effective_radius_const returns it (src/CloudDiagnostics.jl:181), no kernel",
        "ice_cloud_effective_radius": "r_eff of CloudIce: as above (src/CloudDiagnostics.jl:184)",
        "Frostenberg2023_standard_deviation": "σ: read by INP_concentration_frequency only, which the sweep leaves out (its own test allows 10·RTOL: tests/test_row_g.py) — σ is swept NOWHERE; "
                                              "the TemperatureDependent timescale of this family uses INP_concentration_mean, which does not read it",
        "gas_constant_dry_air": "R_d: no formula of the replaced subsystems reads it except ARG2000's q_vs (swept there)",
        "Chen2022_ice_cutoff": "small / large ice cut-off diameter: read by the P3 particle fall speed only (src/P3_terminal_velocity.jl:19,40); the bulk 1-moment speeds take "
                               "small_ice for cloud ice and large_ice for snow without it",
    },
    "cloud diagnostics": {
        "rain_drop_length_scale": "r₀ of the rain mass relation cancels in λ⁻¹ for Δm = 0 (m₀ ∝ r₀^me); radar_reflectivity_1M reads (pdf, mass) only (src/CloudDiagnostics.jl:29-43)",
        **{f"rain_cross_section_size_relation_coefficient_{k}": "area relation of CMP.Rain: radar_reflectivity_1M reads (pdf, mass) only" for k in ("ae", "dela", "chia")},
        "rain_ventilation_coefficient_a": "ventilation of CMP.Rain: radar_reflectivity_1M reads (pdf, mass) only",
        "rain_ventilation_coefficient_b": "ventilation of CMP.Rain: radar_reflectivity_1M reads (pdf, mass) only",
        "SB2006_cloud_droplets_min_mass": "xc_min of the cloud PDF: the diagnostics read (νc, μc, ρw) and (νr, μr, ρw) + the limiters (src/CloudDiagnostics.jl:66-67,102-103); swept in SB2006",
        "SB2006_reference_air_density": "ρ₀ of the rain PDF: as above; swept in SB2006",
    },
    "ice nucleation": {
        **{k: "the water activities read the two saturation vapour pressures only (src/Common.jl:250-271): cp_v, cp_l, cp_i, LH_v0, LH_s0, T_0, T_triple, p_triple, R_v"
           for k in ("gas_constant_dry_air", "isobaric_specific_heat_dry_air", "temperature_water_freeze", "isochoric_specific_heat_liquid")},
        "p_over_sulphuric_acid_solution_T_max": "destructured by H2SO4_soln_saturation_vapor_pressure and never evaluated (src/Common.jl:188-212)",
        "p_over_sulphuric_acid_solution_T_min": "destructured by H2SO4_soln_saturation_vapor_pressure and never evaluated (src/Common.jl:188-212)",
    },
    "ARG2000": {
        **{k: "read by the ice-sink (12-argument) method only (src/AerosolActivation.jl:138-200), which the sweep leaves to tests/test_arg2000_gpu.py::test_liquid_and_ice_sinks "
              "at the defaults: its S_max needs that test's own conditioning of αw − K_ice(ξ − 1)"
           for k in ("density_ice_water", "isobaric_specific_heat_ice", "latent_heat_sublimation_at_reference")},
        "temperature_water_freeze": "no ARG2000 formula reads it", "isochoric_specific_heat_liquid": "no ARG2000 formula reads it",
        "kinematic_viscosity_of_air": "ν_air of AirProperties: ARG2000 reads K_therm and D_vapor only, through CO.G_func_liquid (src/AerosolActivation.jl:160)",
    },
    "0-moment": {},
    "aerosol nucleation": {},
    "P3": {
        "P3_constant_slope_parameterization_value": "μ of the constant slope law: the entries are swept with the default power law (slope_law = 'powerlaw')",
        "density_liquid_water": "ρ_l of ParametersP3: read by the liquid-ice collision sources only (left out, see tests/test_param_sweep_gpu.py)",
        "P3_wet_growth_timescale": "τ_wet of ParametersP3: read by the collision sources only (left out)",
        **{k: "ice_melt reads TDI.Lf(tps, T) = LH_s(T) − LH_v(T) and T_freeze only (src/P3_processes.jl:64-94): LH_v0, LH_s0, cp_l, cp_i, T_0"
           for k in ("gas_constant_vapor", "gas_constant_dry_air", "isobaric_specific_heat_dry_air", "isobaric_specific_heat_vapor", "temperature_triple_point",
                     "pressure_triple_point", "isochoric_specific_heat_liquid")},
    },
}
# Parameters whose whole effect on a family stays below 10·RTOL[f32] = 1 % over the swept states: Float32 cannot be asked to see them (its liveness count
# is below MIN_LIVE by construction); the Float64 count, with its 1e-5 threshold, is asserted as for every other parameter.
WEAK_F32 = {
    "P3": {"Chen2022_table_B5_Gl": "G of the large-ice fall speed (Table B5): over L = 1e-7…3e-2 kg/m³, N = 0.1…1e7 1/m³ (down to the solver's lower bracket log λ = 2) "
                                   "a 25 % change moves the P3 integrals by at most 0.93 % (self-collection; fall speeds 0.67 %, melt 0.30 %) — no P3 state reaches "
                                   "1 %, asserted by test_weak_f32_rows_cannot_reach_the_threshold; live in Float32 in the 1-moment fall speeds"},
}


def perturbations(names, context=(), only=None, base=None):
    """The (name, element, direction) cases of `names`, minus those DOMAIN excludes in `context`.  `base`: overrides that the entry holds
    fixed at non-default values (each case is base + one change).  Returns (cases, skipped)."""
    cases, skipped = [], []
    base = base or {}
    for name in names:
        if only is not None and name not in only:
            continue
        v = base.get(name, P.DEFAULT_PARAMETERS[name])
        elems = [None] if isinstance(v, float) else list(range(len(v)))
        for i in elems:
            x = v if i is None else v[i]
            if x == 0:
                step = ZERO_STEP.get(name, DEFAULT_ZERO_STEP)
                moves = [(f"+{step:g}", x + step)]
            else:
                moves = [("x1.25", x * UP), ("x0.8", x * DOWN)]
            for label, y in moves:
                ov = {**base, name: y if i is None else tuple(y if j == i else e for j, e in enumerate(v))}
                p = Perturbation(name, i, label, ov)
                rule = next((r for r in DOMAIN if r.name in (name, f"{name}[{i}]") and r.label in (None, label) and (r.context is None or r.context in context)), None)
                (skipped if rule else cases).append(p)
    return cases, skipped


def rounded(cols, ft):
    """The state columns as the float type rounds them, and those values in double for the oracle."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    return x, [c.astype(np.float64) for c in x]


def _moved(a, b, scale, ft):
    e = parity.scaled_err(b, a, scale, parity.FLOOR[ft], parity.CEIL[ft], parity.CTOL[ft] / parity.RTOL[ft])
    fa, fb = np.isfinite(np.asarray(a, dtype=np.float64)), np.isfinite(np.asarray(b, dtype=np.float64))
    # a value that becomes, or stops being, the NaN of a domain error (Koop's Δa_w window, S_i,max) has moved too
    return (fa & fb & (np.nan_to_num(e, nan=0.0) > LIVE_FACTOR * parity.RTOL[ft])) | (fa != fb)


def liveness(ref_default, ref_perturbed, scale, ft, names=None):
    """Number of compared states at which the reference ALONE moves by more than 10·RTOL[ft] (normalised as parity.scaled_err does, with
    the default run's operand scale) in at least one output, or turns from a finite value into the NaN of a domain error or back."""
    moved = None
    keeps = ref_perturbed.get("keep", {})
    for k in (names or [k for k in ref_default if k not in ("scale", "near_branch", "sources", "keep")]):
        m = _moved(ref_default[k], ref_perturbed[k], None if scale is None else scale.get(k), ft)
        if k in keeps:
            m &= keeps[k]
        moved = m if moved is None else (moved | m)
    near = ref_perturbed.get("near_branch")
    if near is not None:
        moved &= ~near
    return int(moved.sum())


class Sweep:
    """Collects the comparisons of one (entry, float type): check() never raises, finish() writes ONE summary row and raises once."""

    def __init__(self, entry, ft):
        self.entry, self.ft = entry, ft
        self.failures, self.n_cases = [], 0
        self.min_frac, self.worst_wc, self.worst = 1.0, 0.0, (-1.0, None)
        self.min_kept = (1.0, "")                        # smallest fraction of the states a comparison kept (per-output masks included), and where
        self.live = {}                                   # perturbation key → liveness count

    def check(self, got, ref, what, names):
        ft, rtol = self.ft, parity.RTOL[self.ft]
        near = ref.get("near_branch")
        keep = ~near if near is not None else slice(None)
        self.n_cases += 1
        keep_all, keeps = keep, ref.get("keep", {})
        for k in names:
            keep = keeps.get(k, keep_all)
            kept = 1.0 if isinstance(keep, slice) else float(np.mean(keep))
            if kept < self.min_kept[0]:
                self.min_kept = (kept, f"{what} {k}")
            sc = ref.get("scale", {}).get(k)
            e = np.nan_to_num(parity.scaled_err(got[k], ref[k], sc, parity.FLOOR[ft], parity.CEIL[ft], parity.CTOL[ft] / rtol), nan=np.inf)
            worst = float(np.max(e[keep])) if e[keep].size else 0.0
            ps = parity.plain_stats(got[k], ref[k], sc, rtol, parity.FLOOR[ft], parity.CEIL[ft], keep, parity.WELLCOND[ft])
            self.min_frac, self.worst_wc = min(self.min_frac, ps["frac_within"]), max(self.worst_wc, ps["worst_wellcond"])
            if worst > self.worst[0]:
                self.worst = (worst, (what, k, np.array(got[k], dtype=np.float64), np.array(ref[k], dtype=np.float64),
                                      None if sc is None else np.array(sc, dtype=np.float64), None if isinstance(keep, slice) else keep))
            why = []
            if not worst <= rtol:
                i = int(np.argmax(e if isinstance(keep, slice) else np.where(keep, e, 0)))
                why.append(f"normalised error {worst:.3e} > {rtol:g} at i={i}: got {np.asarray(got[k])[i]!r} ref {ref[k][i]!r}")
            if ps["frac_within"] < parity.MIN_FRAC_WITHIN[ft]:
                why.append(f"only {ps['frac_within']:.6f} of {ps['n']} points within the plain bound (required {parity.MIN_FRAC_WITHIN[ft]})")
            if ps["worst_wellcond"] > rtol:
                why.append(f"well-conditioned point with plain relative error {ps['worst_wellcond']:.3e} > {rtol:g}")
            if why:
                self.failures.append(f"{self.entry} {ft} | {what} | {k}: " + "; ".join(why))
        if near is not None and near.size and not (near.mean() < 1e-4 or near.sum() <= 2):
            self.failures.append(f"{self.entry} {ft} | {what}: implausibly many near-branch points ({int(near.sum())} of {near.size})")

    def fail(self, what, why):
        self.failures.append(f"{self.entry} {self.ft} | {what}: {why}")

    def finish(self):
        if self.worst[1] is not None:
            what, k, g, r, sc, keep = self.worst[1]
            parity.record(f"parameter sweep, {self.entry}: {self.n_cases} comparisons; shown: the worst one ({what})", self.ft, {k: g}, {k: r},
                          family=FAMILY, pinned_by="oracle evaluated with the same one-parameter override", scale=None if sc is None else {k: sc},
                          keep=keep, names=[k],
                          note=f"over all {self.n_cases} comparisons: min fraction inside the plain bound {self.min_frac:.6f}, "
                               f"worst well-conditioned plain error {self.worst_wc:.3e}, smallest kept fraction {self.min_kept[0]:.4f} ({self.min_kept[1]}), "
                               f"{len(self.failures)} failures")
        print(f"\n[parameter sweep] {self.entry} {self.ft}: {self.n_cases} comparisons, worst normalised error {self.worst[0]:.3e}, "
              f"min fraction inside the plain bound {self.min_frac:.6f}, worst well-conditioned error {self.worst_wc:.3e}, "
              f"smallest kept fraction {self.min_kept[0]:.4f} ({self.min_kept[1]})")
        assert not self.failures, f"{len(self.failures)} failing (entry, parameter, direction):\n" + "\n".join(self.failures)


# =====================================================================================================================================
# entries: how a family's structs are built from a ParamDict, which states it is run on, and its oracle twin
# =====================================================================================================================================
def _t(ft):
    import torch
    return {"f32": torch.float32, "f64": torch.float64}[ft]


def _rng_block(rng, m, lo, hi):
    return 10 ** rng.uniform(np.log10(lo), np.log10(hi), m)


_STATE_CACHE = {}


def sb2006_states(ft):
    """4099 random warm-rain states + directed blocks for the parameters the random ones barely see (measured by liveness on the oracle):
    Φ_ac (q_rai/q_lcl log-uniform 1e-7…1), the x̄_r / N₀ / λ limiters (x̄_r across both clamps), Dr_th / Deq (mean diameters on both sides),
    xc_min (tiny x̄_c) and ρ up to 1.9 kg/m³ for the Chen-2022 table."""
    if ("sb", ft) in _STATE_CACHE:
        return _STATE_CACHE[("sb", ft)]
    from cmx import synthetic
    base = [c.numpy().astype(np.float64) for c in synthetic.sb2006_state(N_POINTWISE, dtype=_t("f64"), seed=5)]
    rng = np.random.default_rng(11)
    blocks = []

    def block(m, q_lcl, n_lcl, q_rai, n_rai, rho=None):
        i = rng.integers(0, N_POINTWISE, m)
        r, T = (base[0][i] if rho is None else rho), base[1][i]
        q_vap = np.maximum(base[2][i] - np.maximum(base[3][i], 0) - np.maximum(base[5][i], 0), 0)
        blocks.append([r, T, q_vap + q_lcl + q_rai, q_lcl, n_lcl, q_rai, n_rai])

    m = 96
    ql = _rng_block(rng, m, 1e-4, 2e-3)                                      # Φ_ac(τ), τ = q_rai/(q_lcl + q_rai)
    qr = ql * _rng_block(rng, m, 1e-7, 1.0)
    block(m, ql, _rng_block(rng, m, 1e7, 1e9), qr, qr / _rng_block(rng, m, 1e-9, 1e-7))
    qr = _rng_block(rng, 2 * m, 1e-6, 2e-3)                                  # x̄_r = q_rai/n_rai from 1e-13 to 1e-3 kg: every limiter on both sides
    block(2 * m, _rng_block(rng, 2 * m, 1e-6, 1e-3), _rng_block(rng, 2 * m, 1e7, 1e9), qr, qr / _rng_block(rng, 2 * m, 1e-13, 1e-3))
    qr = _rng_block(rng, m, 1e-4, 5e-3)                                      # large mean drops: λ_r below λ_min = 1e3 1/m
    block(m, _rng_block(rng, m, 1e-6, 1e-3), _rng_block(rng, m, 1e7, 1e9), qr, qr / _rng_block(rng, m, 1e-6, 3e-5))
    D = rng.uniform(0.15e-3, 1.6e-3, m)                                      # mean diameters around Dr_th = 0.35 mm and Deq = 0.9 mm
    qr = _rng_block(rng, m, 1e-5, 2e-3)
    block(m, _rng_block(rng, m, 1e-6, 1e-3), _rng_block(rng, m, 1e7, 1e9), qr, qr / (np.pi * 1000.0 * D ** 3 / 6.0))
    ql = _rng_block(rng, m, 1e-7, 1e-4)                                      # x̄_c = q_lcl/n_lcl around xc_min = 4.2e-15 kg
    block(m, ql, ql / _rng_block(rng, m, 1e-16, 1e-13), _rng_block(rng, m, 1e-7, 1e-4), _rng_block(rng, m, 1e2, 1e5))
    qr = _rng_block(rng, m + 2, 1e-6, 3e-3)                                  # the Chen-2022 table over its whole fitted density range
    block(m + 2, _rng_block(rng, m + 2, 1e-6, 1e-3), _rng_block(rng, m + 2, 1e7, 1e9), qr, qr / _rng_block(rng, m + 2, 1e-10, 1e-6),
          rho=rng.uniform(0.3, 1.9, m + 2))
    cols = [np.concatenate([b] + [blk[k] for blk in blocks]) for k, b in enumerate(base)]
    assert cols[0].size % 2 == 1
    _STATE_CACHE[("sb", ft)] = rounded(cols, ft)
    return _STATE_CACHE[("sb", ft)]


def mp1m_states(ft):
    """4099 random 1-moment states + directed blocks: q_lcl / q_icl on both sides of the autoconversion thresholds (5e-4, 1e-6), warm and
    cold, with and without precipitation."""
    if ("1m", ft) in _STATE_CACHE:
        return _STATE_CACHE[("1m", ft)]
    from cmx import synthetic
    base = [c.numpy().astype(np.float64) for c in synthetic.mp1m_state(N_POINTWISE, dtype=_t("f64"), seed=5)]
    rng = np.random.default_rng(12)
    m = 256
    i = rng.integers(0, N_POINTWISE, m)
    q_vap = np.maximum(base[2][i] - sum(np.maximum(base[k][i], 0) for k in (3, 4, 5, 6)), 0)
    ql = _rng_block(rng, m, 1e-4, 2.5e-3)
    qi = _rng_block(rng, m, 1e-7, 2e-5)
    qr = np.where(rng.random(m) < 0.5, _rng_block(rng, m, 1e-6, 2e-3), 0.0)
    qs = np.where(rng.random(m) < 0.5, _rng_block(rng, m, 1e-6, 2e-3), 0.0)
    blk = [base[0][i], base[1][i], q_vap + ql + qi + qr + qs, ql, qi, qr, qs]
    m2 = 256                                                                  # warm snow with liquid: the melt / accretion-melt terms (cv_l, T − T_freeze)
    i = rng.integers(0, N_POINTWISE, m2)
    w = [_rng_block(rng, m2, 1e-6, 1e-3), np.zeros(m2), _rng_block(rng, m2, 1e-6, 2e-3), _rng_block(rng, m2, 1e-6, 2e-3)]
    blk2 = [base[0][i], 273.15 + rng.uniform(0.5, 15.0, m2), 8e-3 + sum(w), *w]
    cols = [np.concatenate([b, blk[k], blk2[k]]) for k, b in enumerate(base)]
    assert cols[0].size % 2 == 1
    _STATE_CACHE[("1m", ft)] = rounded(cols, ft)
    return _STATE_CACHE[("1m", ft)]


def mp1m_linearized_state(n, seed=11):
    """(ρ, T, q_tot, q_lcl, q_icl, q_rai, q_sno) of the LinearizedAverage parity tests (tests/test_mp1m_linearized.py, tests/test_point_host.py)"""
    rng = np.random.default_rng(seed)
    rho, T = rng.uniform(0.3, 1.3, n), rng.uniform(235, 300, n)
    q = lambda: np.where(rng.random(n) < 0.25, 0.0, 10 ** rng.uniform(-7, -2.7, n))  # noqa: E731
    q_lcl, q_icl, q_rai, q_sno = q(), q(), q(), q()
    q_tot = q_lcl + q_icl + q_rai + q_sno + 10 ** rng.uniform(-5, -1.8, n)
    return rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno


def cloud_diagnostics_state(n, seed):
    """(ρ, q_lcl, q_rai, N_lcl, N_rai) of the cloud-diagnostics parity test (tests/test_cloud_diagnostics.py)"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.3, 1.3, n)
    present = lambda p: rng.random(n) < p  # noqa: E731
    q_lcl = np.where(present(0.8), 10 ** rng.uniform(-8, -2.5, n), 0.0)
    q_rai = np.where(present(0.8), 10 ** rng.uniform(-9, -2.5, n), 0.0)
    N_lcl = np.where(present(0.9), 10 ** rng.uniform(5, 9.5, n), 0.0)
    N_rai = np.where(present(0.9), 10 ** rng.uniform(0, 6.5, n), 0.0)
    # tiny values around the gates (eps(FT) and far below), as in the reference's "small numbers" case
    k = n // 20
    q_lcl[:k] = 10 ** rng.uniform(-30, -6, k); N_lcl[:k] = 10 ** rng.uniform(-15, 3, k)
    q_rai[k:2 * k] = 10 ** rng.uniform(-30, -6, k); N_rai[k:2 * k] = 10 ** rng.uniform(-20, 1, k)
    return rho, q_lcl, q_rai, N_lcl, N_rai


def nucleation_state(n, seed):
    """Physical ranges — T 190–320 K; concentrations log-uniform over the CLOUD-chamber ranges and beyond (per m³): h2so4 1e8–1e16, nh3 1e8–1e18,
    negative ions 1e6–1e10, monoterpenes 1e12–1e18, O3 1e16–1e19, OH 1e9–1e14; condensation sink 1e-5–1e-1 s⁻¹."""
    g = np.random.default_rng(seed)
    lu = lambda lo, hi: 10.0 ** g.uniform(lo, hi, n)  # noqa: E731
    return {"h2so4": lu(8, 16), "nh3": lu(8, 18), "negative_ion": lu(6, 10), "monoterpene": lu(12, 18), "O3": lu(16, 19), "OH": lu(9, 14),
            "temp": g.uniform(190, 320, n), "condensation_sink": lu(-5, -1)}


SB_NAMES = ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "vt_rai_n", "vt_rai_m"]
M1_NAMES = ["dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt"]
# the option sets of tests/test_point_host.py::OPTION_SETS (restated here: importing that module would build its fixtures' libraries)
OPTION_SETS = {
    "default": {},
    "alt": dict(snow_autoconversion=P.WithSupersaturation(), snow_deposition_sublimation=P.SublimationOnly(), rain_autoconversion=P.PrescribedNd()),
    "sparse": dict(rain_snow_accretion=None, cloud_ice_melt=None, cloud_liquid_snow_accretion=None, snow_melt=None),
    "tdep": dict(cloud_ice_formation=P.TemperatureDependent()),
}


class Entry:
    """One swept entry point (in one configuration).  params(td) builds its structs from a ParamDict; ref() is the oracle with the same structs
    in double; gpu() the caller-visible Python wrapper; host() the CPU build of the device point function, where one exists."""
    family = entry = ""
    context = ()
    names = ()
    host = None
    base = None            # overrides held fixed at non-default values (a parameter that is inert at the defaults, e.g. α of (N_c/1e8)^α)
    ref_uses_got = False   # the P3 integrals: the reference is evaluated at the log λ the device solved for (ref(…, got))
    skip_dead = False      # entries that read many structs: a perturbation the oracle does not see at all (liveness 0) is not launched

    def __str__(self):
        return self.entry

    def passed(self, p):
        """the structs / numbers of params(td) that the entry hands to the kernel, where that is less than everything params() builds"""
        return None

    def read(self):
        """The names this entry's constructors read.  Where passed() is given, only those whose perturbation changes a byte of what is passed: a
        constructor such as Microphysics1MParams reads ninety names to build the one member (`rain`) that cloud_diagnostics takes."""
        names = names_read(lambda td: self.params(td))
        if self.passed(self.params(P.ParamDict("f64", self.base))) is None:
            return names
        blob = lambda ov: b"".join(bytes(memoryview(x)) if hasattr(x, "_fields_") else np.float64(x).tobytes()  # noqa: E731
                                   for x in self.passed(self.params(P.ParamDict("f64", ov))))
        ref = blob(self.base)
        return [n for n in names if any(blob(c.override) != ref for c in perturbations([n], (), None, self.base)[0])]


class SbTendencies(Entry):
    family, names = "SB2006", SB_NAMES

    def __init__(self, limited, vel):
        from cmx import _abi
        self.limited, self.vel = limited, vel
        self.flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | (_abi.CMX_VEL_CHEN2022 if vel == "chen" else _abi.CMX_VEL_SB2006)
        self.entry = f"bulk_microphysics_tendencies 2M ({'limited' if limited else 'not limited'}, {vel} velocity)"
        self.context = () if limited or vel == "chen" else ("not-limited SB2006 fall speed",)

    states = staticmethod(sb2006_states)

    def params(self, td):
        return dict(wr=P.WarmRainParams2M(td, self.limited), tps=P.ThermodynamicsParameters(td), vel=P.rain_vel_params(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        return ob.sb2006_warm_rain_tendencies(_abi.F64, p["wr"].c, p["tps"], p["vel"], self.flags, *x64, float32_gates=(ft == "f32"), nthreads=8,
                                              branch_margin=1e-5 if ft == "f32" else 1e-11)

    def gpu(self, p, xt):
        import cmx
        r = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), p["wr"], p["tps"], *xt, vel_params=p["vel"],
                                             vel=cmx.Chen2022VelTypeRain if self.vel == "chen" else cmx.SB2006VelType)
        return {k: v.cpu().numpy() for k, v in r._asdict().items()}

    def host(self, lib, p, x, ft):
        import ctypes as C
        rc, y = host_call(lib, "host_sb2006", ft, (C.byref(p["wr"].c), C.byref(p["tps"]), C.byref(p["vel"]), C.c_uint32(self.flags), C.c_int(0)), x, 6)
        return rc, dict(zip(SB_NAMES, y))


class Mp1mTendencies(Entry):
    family, names = "1-moment", M1_NAMES

    def __init__(self, optset):
        self.optset = optset
        self.entry = f"bulk_microphysics_tendencies_1m Instantaneous ({optset} options)"

    states = staticmethod(mp1m_states)

    def params(self, td):
        return dict(mp=P.Microphysics1MParams(td, **OPTION_SETS[self.optset]), tps=P.ThermodynamicsParameters(td), T_freeze=td["temperature_water_freeze"])

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = ob.mp1m(_abi.F64, p["mp"].c, p["tps"], p["mp"].flags, *x64, float32_gates=(ft == "f32"), nthreads=8)
        r["near_branch"] = np.abs(x64[1] - p["T_freeze"]) < (1e-4 if ft == "f32" else 1e-11)      # the warm / cold routing (BMT:171)
        return r

    def gpu(self, p, xt):
        import cmx
        r = cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), p["mp"], p["tps"], *xt)
        return {k: v.cpu().numpy() for k, v in r._asdict().items()}

    def host(self, lib, p, x, ft):
        import ctypes as C
        rc, y = host_call(lib, "host_mp1m_tendencies", ft, (C.byref(p["mp"].c), C.byref(p["tps"]), C.c_uint32(p["mp"].flags)), x, 4)
        return rc, dict(zip(M1_NAMES, y))


def _raw(kind):
    """the unrounded state columns of sb2006_states / mp1m_states (Float64 rounding is the identity)"""
    return (sb2006_states if kind == "sb" else mp1m_states)("f64")[1]


def _np_out(r, names):
    return {k: getattr(r, k).reshape(-1).cpu().numpy() for k in names}


def _copy(struct):
    return type(struct).from_buffer_copy(struct)


class SbProcessRates(Entry):
    """sb2006_process_rates: every process in its own column — a parameter moves its own column wholesale."""
    family = "SB2006"

    def __init__(self, limited):
        from cmx import _abi
        self.limited = limited
        self.flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006
        self.entry = f"sb2006_process_rates ({'limited' if limited else 'not limited'})"
        self.context = () if limited else ("not-limited SB2006 fall speed",)
        self.names = list(_abi.SB2006_PROCESS_COLUMNS)

    def states(self, ft):
        rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai = [np.maximum(c, 0) if k != 1 else c for k, c in enumerate(_raw("sb"))]
        return rounded([q_tot, q_lcl, q_rai, rho * n_lcl, rho * n_rai, rho, T], ft)

    params = SbTendencies.params

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        q_tot, q_lcl, q_rai, N_lcl, N_rai, rho, T = x64
        r = ob.sb2006_process_rates(_abi.F64, p["wr"].c, p["tps"], p["vel"], self.flags, *x64, float32_gates=(ft == "f32"))
        fused = ob.sb2006_warm_rain_tendencies(_abi.F64, p["wr"].c, p["tps"], p["vel"], self.flags, rho, T, q_tot, q_lcl, N_lcl / rho, q_rai, N_rai / rho,
                                               float32_gates=(ft == "f32"), nthreads=8, branch_margin=1e-5 if ft == "f32" else 1e-11)
        tps = p["tps"]
        dcp = tps.cp_v - tps.cp_l
        p_sat = tps.press_triple * (T / tps.T_triple) ** (dcp / tps.R_v) * np.exp((tps.LH_v0 - dcp * tps.T_0) / tps.R_v * (1 / tps.T_triple - 1 / T))
        S = np.maximum(0, q_tot - q_lcl - q_rai) * rho * tps.R_v * T / p_sat - 1
        far = np.abs(S) > 0.02                                     # the columns ∝ S = q_v/q_sat − 1 are compared away from its zero
        tau = p["wr"].c.seifert_beheng.numadj.tau
        r["keep"] = {**{k: far for k in ("evap_dN_rai_dt", "evap_dq_rai_dt", "condevap", "devap_dN_rai", "devap_dq_rai")}, "rain_breakup": ~fused["near_branch"]}
        r["scale"] = {"rain_vel_n": fused["scale"]["vt_rai_n"], "rain_vel_m": fused["scale"]["vt_rai_m"],
                      "numadj_rai": 2 * np.abs(N_rai / rho) / tau, "numadj_lcl": 2 * np.abs(N_lcl / rho) / tau}   # (n_target − n)/τ cancels when the clamp is inactive
        return r

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.sb2006_process_rates(p["wr"], p["tps"], *xt, vel=cmx.SB2006VelType, vel_params=p["vel"]), self.names)


class SbCloudVelocity(Entry):
    family, entry, names = "SB2006", "cloud_terminal_velocity", ["vt_n", "vt_m"]

    def states(self, ft):
        rho, _, _, q_lcl, n_lcl = _raw("sb")[:5]
        return rounded([q_lcl, rho, rho * n_lcl], ft)

    def params(self, td):
        return dict(pdf=P.CloudParticlePDF_SB2006(td), vel=P.StokesRegimeVelType(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        return dict(zip(self.names, ob.sb2006_cloud_terminal_velocity(_abi.F64, p["pdf"], p["vel"], *x64, float32_gates=(ft == "f32"))))

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.cloud_terminal_velocity(p["pdf"], p["vel"], *xt), self.names)


COLUMN_SHAPE = (37, 111)          # 4107 points: columns that straddle the workgroup tiles, an odd number of levels


def _inv_dz(n_lev):
    return 1.0 / (30.0 + 470.0 * np.random.default_rng(3).random(n_lev))


class SbColumn(Entry):
    family, names, skip_dead = "SB2006", ["dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt"], True

    def __init__(self, limited, vel):
        SbTendencies.__init__(self, limited, vel)
        self.entry = f"column_tendencies_sedimentation {COLUMN_SHAPE} with cloud_vel ({'limited' if limited else 'not limited'}, {vel} velocity)"

    def states(self, ft):
        n = COLUMN_SHAPE[0] * COLUMN_SHAPE[1]
        return rounded([c[:n] for c in _raw("sb")], ft)

    def params(self, td):
        return dict(SbTendencies.params(self, td), stokes=P.StokesRegimeVelType(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        return ob.sb2006_column_tendencies_sedimentation(_abi.F64, p["wr"].c, p["tps"], p["vel"], p["stokes"], self.flags, _inv_dz(COLUMN_SHAPE[1]),
                                                         *[c.reshape(COLUMN_SHAPE) for c in x64], float32_gates=(ft == "f32"), nthreads=8,
                                                         branch_margin=1e-5 if ft == "f32" else 1e-11)

    def gpu(self, p, xt):
        import cmx
        import torch
        dz = torch.from_numpy(_inv_dz(COLUMN_SHAPE[1])).to(xt[0].dtype).to(xt[0].device)
        r = cmx.column_tendencies_sedimentation(p["wr"], p["tps"], dz, *[c.view(COLUMN_SHAPE) for c in xt], vel_params=p["vel"], cloud_vel=p["stokes"],
                                                vel=cmx.Chen2022VelTypeRain if self.vel == "chen" else cmx.SB2006VelType)
        return _np_out(r, self.names)


class Bulk2M(Entry):
    """bulk_2m_cloud_to_rain with the smooth transition (so that the steepness k is live)."""
    family = "SB2006"

    def __init__(self, scheme):
        self.scheme = scheme
        self.entry = f"bulk_2m_cloud_to_rain {scheme}"
        self.names = ["acnv"] if scheme == "LD2004" else ["acnv", "accr"]

    def states(self, ft):
        rng = np.random.default_rng(21)
        n = N_POINTWISE
        q = lambda lo, hi: np.where(rng.random(n) < 0.1, 0.0, _rng_block(rng, n, lo, hi))  # noqa: E731
        return rounded([q(1e-7, 3e-3), q(1e-7, 3e-3), rng.uniform(0.3, 1.3, n), _rng_block(rng, n, 1e7, 1e9)], ft)   # q_lcl, q_rai, ρ, N_d

    def params(self, td):
        return dict(sch=P.Bulk2MSchemes(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        from cmx.bulk_tendencies import _SCHEMES_2M
        q_lcl, q_rai, rho, N_d = x64
        acnv, accr = ob.bulk_2m_cloud_to_rain(_abi.F64, p["sch"], _SCHEMES_2M[self.scheme] | _abi.CMX_2M_SMOOTH_TRANSITION, q_lcl, q_rai, rho, N_d,
                                              float32_gates=(ft == "f32"))
        return {"acnv": acnv, "accr": accr}

    def gpu(self, p, xt):
        import cmx
        q_lcl, q_rai, rho, N_d = xt
        r = cmx.bulk_2m_cloud_to_rain(p["sch"], self.scheme, q_lcl, rho, N_d, None if self.scheme == "LD2004" else q_rai, smooth_transition=True)
        return _np_out(r, self.names)


class PrecipSusceptibility(Entry):
    """precipitation_susceptibilities: b_is_3 (the default b) with non-default A, a, x_star; and the general form with b perturbed.  Reference:
    tests/precip_susceptibility_ref.py, which takes the structs.  Operand scale of the sums const − S_r and 1 ∓ h: |const| + |term|."""
    family, entry = "SB2006", "precipitation_susceptibilities"
    names = [f"{proc}_{f}" for proc in ("acnv", "accr") for f in ("d_ln_q_lcl", "d_ln_q_rai", "d_ln_N_lcl")]

    def states(self, ft):
        import precip_susceptibility_ref as R
        return rounded(R.random_states(N_POINTWISE, seed=4), ft)

    def params(self, td):
        return dict(sb=P.SB2006(td))

    def passed(self, p):
        return [p["sb"].acnv, p["sb"].accr]

    def ref(self, p, x64, ft):
        import precip_susceptibility_ref as R
        au, ac = R.autoconversion(p["sb"].acnv, *x64, R.EPS[ft]), R.accretion(p["sb"].accr, *x64, R.EPS[ft])
        r = {**{f"acnv_{k}": v for k, v in au.items()}, **{f"accr_{k}": v for k, v in ac.items()}}
        S_r, h = np.abs(np.nan_to_num(au["d_ln_q_rai"])), np.abs(np.nan_to_num(ac["d_ln_q_rai"] - 1))
        r["scale"] = {"acnv_d_ln_q_lcl": 4 + S_r, "acnv_d_ln_q_rai": S_r, "accr_d_ln_q_lcl": 1 + h, "accr_d_ln_q_rai": 1 + h}
        clip = ~R.near_clip(p["sb"].acnv, x64[0], x64[2], x64[3])       # |x̄_c/x_star − 1| < 1e-5: either branch of the min of CM2:406
        r["keep"] = {k: clip for k in self.names if k.startswith("acnv")}
        return r

    def gpu(self, p, xt):
        import cmx
        r = cmx.precipitation_susceptibilities(p["sb"], *xt)
        out = {}
        for proc, rr in (("acnv", r.autoconversion), ("accr", r.accretion)):
            for f in ("d_ln_q_lcl", "d_ln_q_rai", "d_ln_N_lcl"):
                out[f"{proc}_{f}"] = getattr(rr, "d_ln_pp_" + f).cpu().numpy()
        return out


# ---- 1-moment ------------------------------------------------------------------------------------------------------------------------
_CANCEL_1M = {"S_phase_change_vap_lcl": "dq_lcl_dt", "S_phase_change_vap_icl": "dq_icl_dt", "S_phase_change_vap_rai": "dq_rai_dt",
              "S_phase_change_vap_sno": "dq_sno_dt", "S_melt_icl_lcl": "dq_icl_dt", "S_melt_sno_rai": "dq_sno_dt", "S_accr_melt_lcl_sno": "dq_sno_dt",
              "S_accr_melt_rai_sno": "dq_sno_dt", "S_acnv_icl_sno": "dq_icl_dt", "S_acnv_lcl_rai": "dq_lcl_dt"}


class Mp1mSources(Mp1mTendencies):
    """microphysics_source_terms_1m: the 18 source terms; the vapour / melt / threshold terms carry the operand scale of the tendency they enter
    (tests/test_mp1m_gpu.py::test_tendencies_and_sources_match_oracle)."""

    def __init__(self, optset, base=None):
        from cmx import _abi
        self.optset, self.base = optset, base
        self.entry = f"microphysics_source_terms_1m ({optset} options{'' if not base else ', base ' + ', '.join(f'{k} = {v:g}' for k, v in base.items())})"
        self.names = list(_abi.MP1M_SOURCE_COLUMNS)

    def ref(self, p, x64, ft):
        r = Mp1mTendencies.ref(self, p, x64, ft)
        out = dict(r["sources"])
        out["scale"] = {k: r["scale"][t] for k, t in _CANCEL_1M.items()}
        out["near_branch"] = r["near_branch"]
        return out

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.microphysics_source_terms_1m(p["mp"], p["tps"], *xt), self.names)

    def host(self, lib, p, x, ft):
        import ctypes as C
        rc, y = host_call(lib, "host_mp1m_sources", ft, (C.byref(p["mp"].c), C.byref(p["tps"]), C.c_uint32(p["mp"].flags)), x, len(self.names))
        return rc, dict(zip(self.names, y))


class Mp1mLinearized(Mp1mTendencies):
    """LinearizedAverage (Δt = 20 s, 2 substeps) with the tolerance of tests/test_mp1m_linearized.py::check_linearized_parity: operand scale = Σ of the
    Instantaneous scales + the rounding floor 8 eps (q + |r| Δt)/Δt of the difference quotient; the Float32 plain bound on the points where it is attainable."""
    DT, NSUB = 20.0, 2

    def __init__(self):
        self.optset = "default"
        self.entry = f"bulk_microphysics_tendencies_1m LinearizedAverage (dt = {self.DT:g}, nsub = {self.NSUB})"

    def states(self, ft):
        return rounded(mp1m_linearized_state(N_POINTWISE, seed=21), ft)      # the states that entry's own parity test draws (its plain bound is stated for them)

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        q_min = P.DEFAULT_PARAMETERS["specific_humidity_minimum"]
        r = ob.mp1m_linearized_average(_abi.F64, p["mp"].c, p["tps"], p["mp"].flags, q_min, self.DT, self.NSUB, *x64, float32_gates=(ft == "f32"), nthreads=8)
        inst = ob.mp1m(_abi.F64, p["mp"].c, p["tps"], p["mp"].flags, *x64, float32_gates=(ft == "f32"), nthreads=8, want_sources=False)
        scale = sum(inst["scale"].values())
        eps = {"f64": 2.2e-16, "f32": 1.2e-7}[ft]
        near = np.abs(x64[1] - p["T_freeze"]) < (1e-3 if ft == "f32" else 1e-9)
        r["scale"], r["keep"] = {}, {}
        for k, q0 in zip(M1_NAMES, x64[3:]):
            r["scale"][k] = scale + 8 * eps * (np.maximum(q0, 0) + np.abs(r[k]) * self.DT) / self.DT / parity.CTOL[ft]
            r["keep"][k] = ~near & ((2 * eps * np.maximum(q0, 0) / self.DT <= parity.RTOL[ft] * np.abs(r[k])) | (ft == "f64"))
        return r

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.bulk_microphysics_tendencies_1m(cmx.LinearizedAverage(), cmx.Microphysics1Moment(), p["mp"], p["tps"], *xt, self.DT, self.NSUB), M1_NAMES)

    def host(self, lib, p, x, ft):
        import ctypes as C
        ct = {"f32": C.c_float, "f64": C.c_double}[ft]
        head = (C.byref(p["mp"].c), C.byref(p["tps"]), C.c_uint32(p["mp"].flags), ct(P.DEFAULT_PARAMETERS["specific_humidity_minimum"]), ct(self.DT), C.c_int32(self.NSUB))
        rc, y = host_call(lib, "host_mp1m_linearized", ft, head, x, 4)
        return rc, dict(zip(M1_NAMES, y))


def vel_states(ft):
    """(ρ, q_lcl, q_icl, q_rai, q_sno) for the fall-speed entries: ρ over 0.3…1.9 kg/m³ (the whole fitted range of the Chen-2022 rain table)."""
    rng = np.random.default_rng(3)
    n = N_POINTWISE
    return rounded([rng.uniform(0.3, 1.9, n)] + [np.where(rng.random(n) < 0.2, 0.0, _rng_block(rng, n, 1e-8, 10 ** -2.0)) for _ in range(4)], ft)


def _chen_rain_magnitudes(cr):
    """the Chen-2022 rain speed is a sum of three terms of both signs (a₂ < 0): operand scale = the same sum with |aᵢ|, as the 2-moment oracle reports it"""
    pos = _copy(cr)
    for i in range(3):
        pos.a[i] = abs(cr.a[i])
    return pos


def _chen_ice_positive_part(ci):
    """the Chen-2022 ice curves are differences of two terms that cancel near the zero crossing: conditioning scale = the positive term alone"""
    pos = _copy(ci)
    pos.small_ice.F[0] = -1e30
    pos.large_ice.E[0], pos.large_ice.E[1], pos.large_ice.E[2] = 0.0, 0.0, 0.0
    return pos


class Sedimentation(Entry):
    family, entry, names, skip_dead = "1-moment", "sedimentation_velocities", ["w_lcl", "w_icl", "w_rai", "w_sno"], True
    states = staticmethod(vel_states)

    def params(self, td):
        return dict(mp=P.Microphysics1MParams(td), stokes=P.StokesRegimeVelType(td), cr=P.Chen2022VelTypeRain(td), ci=P.Chen2022VelTypeIce(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = ob.sedimentation_velocities(_abi.F64, p["mp"].c, p["stokes"], p["cr"], p["ci"], *x64, float32_gates=(ft == "f32"))
        pos = ob.sedimentation_velocities(_abi.F64, p["mp"].c, p["stokes"], _chen_rain_magnitudes(p["cr"]), _chen_ice_positive_part(p["ci"]), *x64,
                                          float32_gates=(ft == "f32"))
        r["scale"] = {"w_icl": pos["w_icl"], "w_rai": pos["w_rai"], "w_sno": pos["w_sno"]}
        return r

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.sedimentation_velocities(p["mp"], p["stokes"], p["cr"], p["ci"], *xt), self.names)

    def host(self, lib, p, x, ft):
        import ctypes as C
        rc, y = host_call(lib, "host_sedimentation", ft, (C.byref(p["mp"].c), C.byref(p["stokes"]), C.byref(p["cr"]), C.byref(p["ci"]), C.c_int(-1)), x, 4)
        return rc, dict(zip(self.names, y))


class TerminalVelocity1M(Entry):
    family, entry, names, skip_dead = "1-moment", "terminal_velocity_1m", ["vt_rai_blk1m", "vt_sno_blk1m", "vt_rai_chen"], True

    def states(self, ft):
        x, x64 = vel_states(ft)
        return [x[0], x[3], x[4]], [x64[0], x64[3], x64[4]]

    def params(self, td):
        return dict(mp=P.Microphysics1MParams(td), cr=P.Chen2022VelTypeRain(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = ob.mp1m_terminal_velocity(_abi.F64, p["mp"].c, p["cr"], *x64, float32_gates=(ft == "f32"))
        r["scale"] = {"vt_rai_chen": ob.mp1m_terminal_velocity(_abi.F64, p["mp"].c, _chen_rain_magnitudes(p["cr"]), *x64, float32_gates=(ft == "f32"))["vt_rai_chen"]}
        return r

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.terminal_velocity_1m(p["mp"], *xt, chen=p["cr"]), self.names)


class SnowVelocity(Entry):
    """snow_terminal_velocity with the fixed aspect ratio, CM1.Oblate and CM1.Prolate, against tests/snow_shape_ref.py (which takes the structs).  The two
    large-ice terms may cancel: operand scale = the first term alone, as for w_sno of sedimentation_velocities."""
    family, names, skip_dead = "1-moment", ["w_sno"], True

    def __init__(self, shape):
        self.shape, self.entry = shape, f"snow_terminal_velocity ({shape or 'fixed aspect ratio'})"

    def states(self, ft):
        x, x64 = vel_states(ft)
        return [x[0], x[4]], [x64[0], x64[4]]

    def params(self, td):
        return dict(mp=P.Microphysics1MParams(td), ci=P.Chen2022VelTypeIce(td))

    def passed(self, p):
        return [p["mp"].c.snow, p["ci"].large_ice]

    def ref(self, p, x64, ft):
        import snow_shape_ref as R
        sh = {None: None, "Oblate": R.Oblate(), "Prolate": R.Prolate()}[self.shape]
        return {"w_sno": R.snow_velocity(p["mp"].c, p["ci"], *x64, sh, ft=ft),
                "scale": {"w_sno": R.snow_velocity(p["mp"].c, _chen_ice_positive_part(p["ci"]), *x64, sh, ft=ft)}}

    def gpu(self, p, xt):
        import cmx
        sh = {None: None, "Oblate": cmx.Oblate(), "Prolate": cmx.Prolate()}[self.shape]
        return {"w_sno": cmx.snow_terminal_velocity(p["mp"], p["ci"], *xt, sh).cpu().numpy()}


class Mp1mColumn(Entry):
    family, names, skip_dead = "1-moment", M1_NAMES, True
    entry = f"column_tendencies_sedimentation_1m {COLUMN_SHAPE} Instantaneous"

    def states(self, ft):
        n = COLUMN_SHAPE[0] * COLUMN_SHAPE[1]
        return rounded([c[:n] for c in _raw("1m")], ft)

    def params(self, td):
        return dict(Sedimentation.params(self, td), tps=P.ThermodynamicsParameters(td), T_freeze=td["temperature_water_freeze"])

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = ob.mp1m_column_tendencies_sedimentation(_abi.F64, p["mp"].c, p["tps"], p["stokes"], p["cr"], p["ci"], p["mp"].flags, _inv_dz(COLUMN_SHAPE[1]),
                                                    *[c.reshape(COLUMN_SHAPE) for c in x64], chen_ice_scale=_chen_ice_positive_part(p["ci"]),
                                                    float32_gates=(ft == "f32"), nthreads=8)
        r["near_branch"] = np.abs(x64[1] - p["T_freeze"]) < (1e-3 if ft == "f32" else 1e-9)      # as tests/test_mp1m_column.py (the fluxes do not read T)
        return r

    def gpu(self, p, xt):
        import cmx
        import torch
        dz = torch.from_numpy(_inv_dz(COLUMN_SHAPE[1])).to(xt[0].dtype).to(xt[0].device)
        r = cmx.column_tendencies_sedimentation_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), p["mp"], p["tps"], p["stokes"], p["cr"], p["ci"], dz,
                                                   *[c.view(COLUMN_SHAPE) for c in xt])
        return _np_out(r, self.names)


# ---- 0-moment, cloud diagnostics -----------------------------------------------------------------------------------------------------
class Mp0m(Entry):
    """bulk_microphysics_tendencies_0m, both threshold forms (q_c,0 and S_0·q_vap_sat) + the derivative.  −max(0, q_l + q_i − threshold)/τ cancels
    at the threshold: operand scale (q_l + q_i + threshold)/τ."""
    family, names = "0-moment", ["dq_tot_dt", "dq_tot_dt_sat", "d_dq_tot"]
    entry = "bulk_microphysics_tendencies_0m / remove_precipitation"

    def states(self, ft):
        rng = np.random.default_rng(31)
        n = N_POINTWISE
        q = lambda: np.where(rng.random(n) < 0.1, 0.0, _rng_block(rng, n, 1e-7, 1e-3))  # noqa: E731
        return rounded([q(), q(), _rng_block(rng, n, 1e-5, 2e-2)], ft)        # q_lcl, q_icl, q_vap_sat: both sides of 5e-6 and of 0.02 q_vap_sat

    def params(self, td):
        return dict(mp=P.Microphysics0MParams(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        ql, qi, qvs = x64
        p0 = p["mp"].precip
        a, da = ob.mp0m_tendencies(_abi.F64, p0, ql, qi)
        b, _ = ob.mp0m_tendencies(_abi.F64, p0, ql, qi, qvs)
        qc = np.maximum(ql, 0) + np.maximum(qi, 0)
        thr_edge = np.abs(qc - p0.qc_0) < (1e-6 if ft == "f32" else 1e-14) * p0.qc_0           # the step of the derivative at the threshold
        return {"dq_tot_dt": a, "dq_tot_dt_sat": b, "d_dq_tot": da, "keep": {"d_dq_tot": ~thr_edge},
                "scale": {"dq_tot_dt": (qc + p0.qc_0) / p0.tau_precip, "dq_tot_dt_sat": (qc + p0.S_0 * qvs) / p0.tau_precip}}

    def gpu(self, p, xt):
        import cmx
        ql, qi, qvs = xt
        return {"dq_tot_dt": cmx.bulk_microphysics_tendencies_0m(cmx.Microphysics0Moment(), p["mp"], None, ql, ql, qi).cpu().numpy(),
                "dq_tot_dt_sat": cmx.remove_precipitation(p["mp"].precip, ql, qi, qvs).cpu().numpy(),
                "d_dq_tot": cmx.d_remove_precipitation_d_q_tot(p["mp"].precip, ql, qi).cpu().numpy()}


class CloudDiagnostics(Entry):
    """cloud_diagnostics: radar reflectivities (compared as the linear factor 10^(Z/10): a relative bound on a dB value would be a bound on its offset)
    and effective radii (above 1e-12 m, below which q ρ/N underflows Float32 — tests/test_cloud_diagnostics.py)."""
    family, names = "cloud diagnostics", ["Z_1m", "Z_2m", "reff_2m", "reff_lh97"]

    def __init__(self, limited):
        self.limited = limited
        self.entry = f"cloud_diagnostics ({'limited' if limited else 'not limited'})"

    def states(self, ft):
        return rounded(cloud_diagnostics_state(N_POINTWISE, 11), ft)                     # ρ, q_lcl, q_rai, N_lcl, N_rai

    def params(self, td):
        return dict(rain=P.Microphysics1MParams(td).c.rain, sb=P.SB2006(td, self.limited), rho_w=P.WaterProperties(td).rho_w)

    def passed(self, p):
        return [p["rain"], p["sb"].pdf_c, p["sb"].pdf_r, p["rho_w"]]

    @staticmethod
    def _lin(r):
        return {k: (10.0 ** (np.asarray(v, dtype=np.float64) / 10.0) if k.startswith("Z") else np.asarray(v, dtype=np.float64)) for k, v in r.items()}

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = self._lin(ob.cloud_diagnostics(_abi.F64, *x64, rain=p["rain"], pdf_c=p["sb"].pdf_c, pdf_r=p["sb"].pdf_r, rho_w=p["rho_w"], limited=self.limited,
                                           float32_gates=(ft == "f32")))
        r["keep"] = {k: r[k] >= 1e-12 for k in ("reff_2m", "reff_lh97")}
        return r

    def gpu(self, p, xt):
        from cmx import cloud_diagnostics as CD
        rho, q_lcl, q_rai, N_lcl, N_rai = xt
        r = CD.cloud_diagnostics(p["rain"], p["sb"], p["rho_w"], rho, q_lcl, q_rai, N_lcl, N_rai)
        return self._lin({k: getattr(r, k).cpu().numpy() for k in self.names})


# ---- ice nucleation ------------------------------------------------------------------------------------------------------------------
ICENUC_NAMES = ["delta_a_w", "J_het", "J_hom", "rate_het", "rate_hom"]


class IceNucleationRates(Entry):
    family, names = "ice nucleation", ICENUC_NAMES

    def __init__(self, dust, linear):
        self.dust, self.linear = dust, linear
        self.entry = f"ice_nucleation_rates (ABIFM {dust}, Koop {'linear' if linear else 'cubic'})"

    def states(self, ft):
        from cmx import synthetic
        return rounded([c.numpy() for c in synthetic.ice_nucleation_state(N_POINTWISE, dtype=_t("f64"), seed=42)], ft)

    def params(self, td):
        return dict(tps=P.ThermodynamicsParameters(td), dust=getattr(P, self.dust)(td), koop=P.Koop2000(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = ob.ice_nucleation_rates(_abi.F64, p["tps"], p["dust"], p["koop"], _abi.CMX_ICENUC_HOM_LINEAR if self.linear else 0, *x64)
        r.pop("n_domain_errors")
        tol = 1e-6 if ft == "f32" else 1e-13                       # within rounding of the Koop Δa_w window edges: the domain-error branch may flip
        edge = (np.abs(r["delta_a_w"] - p["koop"].delta_a_w_min) < tol) | (np.abs(r["delta_a_w"] - p["koop"].delta_a_w_max) < tol)
        r["scale"] = {"delta_a_w": np.ones_like(r["delta_a_w"])}    # Δa_w = a_w − a_w_ice: two O(1) terms
        r["keep"] = {"J_hom": ~edge, "rate_hom": ~edge}
        return r

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.ice_nucleation_rates(p["tps"], p["dust"], p["koop"], *xt, want=tuple(ICENUC_NAMES), linear=self.linear), ICENUC_NAMES)


class WaterActivity(Entry):
    family, entry, names = "ice nucleation", "a_w_ice / a_w_eT", ["a_w_ice", "a_w_eT"]

    def states(self, ft):
        rng = np.random.default_rng(41)
        return rounded([rng.uniform(190.0, 273.0, N_POINTWISE), _rng_block(rng, N_POINTWISE, 0.05, 600.0)], ft)      # T, e [Pa]

    def params(self, td):
        return dict(tps=P.ThermodynamicsParameters(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        return dict(zip(self.names, ob.water_activity(_abi.F64, p["tps"], x64[0], x64[1])))

    def gpu(self, p, xt):
        import cmx
        return {"a_w_ice": cmx.a_w_ice(p["tps"], xt[0]).cpu().numpy(), "a_w_eT": cmx.a_w_eT(p["tps"], xt[1], xt[0]).cpu().numpy()}


class DepositionJ(Entry):
    family, names = "ice nucleation", ["J"]

    def __init__(self, mineral):
        self.mineral, self.entry = mineral, f"deposition_J ({mineral})"

    def states(self, ft):
        return rounded([np.random.default_rng(43).uniform(0.0, 0.32, N_POINTWISE)], ft)

    def params(self, td):
        return dict(dust=P.DepositionDust(td, self.mineral))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        return {"J": ob.deposition_J(_abi.F64, p["dust"], x64[0])}

    def gpu(self, p, xt):
        import cmx
        return {"J": cmx.deposition_J(p["dust"], xt[0]).cpu().numpy()}


class MohlerDeposition(Entry):
    """mohler2006_deposition: exp(a ΔS) − 1 cancels for small a ΔS — operand scale 1 + |f| (tests/test_row_g.py)."""
    family, names = "ice nucleation", ["act_frac", "dep_rate"]

    def __init__(self, dust):
        self.dust, self.entry = dust, f"mohler2006_deposition ({dust})"

    def states(self, ft):
        rng = np.random.default_rng(44)
        n = N_POINTWISE
        return rounded([rng.uniform(1.0, 1.45, n), rng.uniform(200.0, 260.0, n), rng.uniform(-0.1, 0.1, n), _rng_block(rng, n, 10.0, 1e5)], ft)

    def params(self, td):
        return dict(dust=getattr(P, self.dust)(td), ip=P.Mohler2006(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        f, r = ob.mohler2006_deposition(_abi.F64, p["dust"], p["ip"], *x64)
        S_i, T = x64[0], x64[1]
        tol = 1e-6 if ft == "f32" else 1e-13                       # within rounding of S_i,max (the assert) and of T_thr (warm / cold coefficients)
        edge = (np.abs(S_i - p["ip"].S_i_max) < tol * S_i) | (np.abs(T - p["ip"].T_thr) < tol * T)
        return {"act_frac": f, "dep_rate": r, "scale": {"act_frac": 1 + np.abs(np.nan_to_num(f))}, "near_branch": edge}

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.mohler2006_deposition(p["dust"], p["ip"], *xt), self.names)


class H2SO4Solution(Entry):
    family, entry, names = "ice nucleation", "h2so4_solution", ["p_sol", "a_w_xT"]

    def states(self, ft):
        rng = np.random.default_rng(45)
        return rounded([rng.uniform(0.0, 0.4, N_POINTWISE), rng.uniform(185.0, 235.0, N_POINTWISE)], ft)     # the validity range of the fit

    def params(self, td):
        return dict(prs=P.H2SO4SolutionParameters(td), tps=P.ThermodynamicsParameters(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        r = dict(zip(self.names, ob.h2so4_solution(_abi.F64, p["prs"], p["tps"], *x64)))
        T, tol = x64[1], 1e-6 if ft == "f32" else 1e-13
        r["near_branch"] = (np.abs(T - p["prs"].T_min) < tol * T) | (np.abs(T - p["prs"].T_max) < tol * T)
        return r

    def gpu(self, p, xt):
        import cmx
        return dict(zip(self.names, [t.cpu().numpy() for t in cmx.h2so4_solution(p["prs"], p["tps"], *xt)]))


# ---- ARG2000 -------------------------------------------------------------------------------------------------------------------------
class ArgActivation(Entry):
    """aerosol_activation (mode descriptors) and aerosol_activation_columns: S_max and the activated mass per mode (M ½ erfc, on the operand scale M).
    The activated NUMBER is left to tests/test_arg2000_gpu.py: the reference forms it as N ½ (1 − erf u), which cancels, and that test states its own
    erfc-form bound; every ARG2000 parameter reaches it only through S_max and u, which these outputs carry."""
    family, NM = "ARG2000", 3

    def __init__(self, columns):
        self.columns = columns
        self.entry = "aerosol_activation_columns" if columns else "aerosol_activation"
        self.names = ["S_max"] + [f"M_act[{k}]" for k in range(self.NM)]

    def _ad(self):
        from cmx import synthetic
        from cmx.aerosol import AerosolDistribution
        m = synthetic.arg_config3_distribution().modes
        return AerosolDistribution([m[0], m[2], m[3]])

    def states(self, ft):
        from cmx import _abi, synthetic
        cols = [c.numpy() for c in synthetic.arg_state(N_POINTWISE, dtype=_t("f64"), seed=7)]
        # + 256 cold states (215…235 K): cp_v reaches S_max through (T/T_triple)^(Δcp/R_v), which is within 1 % of its default above 250 K
        rng, td = np.random.default_rng(47), P.DEFAULT_PARAMETERS
        T, pr = rng.uniform(215.0, 235.0, 256), rng.uniform(2e4, 5e4, 256)
        dcp, Rv = td["isobaric_specific_heat_vapor"] - td["isobaric_specific_heat_liquid"], td["gas_constant_vapor"]
        Ttr, T0 = td["temperature_triple_point"], td["thermodynamics_temperature_reference"]
        p_vs = td["pressure_triple_point"] * (T / Ttr) ** (dcp / Rv) * np.exp((td["latent_heat_vaporization_at_reference"] - dcp * T0) / Rv * (1 / Ttr - 1 / T))
        q_vs = 1.0 / (1.0 - Rv / td["gas_constant_dry_air"] * (p_vs - pr) / p_vs)
        cold = [T, pr, _rng_block(rng, 256, 0.01, 10.0), q_vs * rng.uniform(0.98, 1.0, 256)]
        cols = [np.concatenate([c, d]) for c, d in zip(cols, cold)]
        n = cols[0].size
        if self.columns:                                             # the aerosol itself varies in space: five columns per mode
            rng = np.random.default_rng(46)
            adc = self._ad().c_struct(P.AerosolActivationParameters("f64"), _abi.F64)
            for k in range(self.NM):
                m = adc.modes[k]
                for v, j in ((m.r_dry, 0.2), (m.stdev, 0.05), (m.N, 0.5), (m.hygroscopicity, 0.2), (m.molar_mass_mix, 0.0)):
                    cols.append(v * (1 + j * rng.uniform(-1, 1, n)))
        return rounded(cols, ft)

    def params(self, td):
        return dict(ap=P.AerosolActivationParameters(td), aip=P.AirProperties(td), tps=P.ThermodynamicsParameters(td))

    def ref(self, p, x64, ft):
        import oracle_binding as ob
        from cmx import _abi
        if self.columns:
            modes = [x64[4 + 5 * k: 9 + 5 * k] for k in range(self.NM)]
            r = ob.arg2000_activation_columns(_abi.F64, p["ap"], p["aip"], p["tps"], *x64[:4], modes, want_M=True, float32_gates=(ft == "f32"), nthreads=8)
            mm = [m[4] for m in modes]
        else:
            adc = self._ad().c_struct(p["ap"], _abi.F64)
            r = ob.arg2000_activation(_abi.F64, p["ap"], adc, p["aip"], p["tps"], *x64, float32_gates=(ft == "f32"), nthreads=8)
            mm = [np.full(x64[0].shape, adc.modes[k].molar_mass_mix) for k in range(self.NM)]
        out = {"S_max": r["S_max"], "scale": {}}
        for k in range(self.NM):
            out[f"M_act[{k}]"], out["scale"][f"M_act[{k}]"] = r["M_act"][k], mm[k]
        return out

    def gpu(self, p, xt):
        import cmx
        if self.columns:
            modes = [cmx.ModeColumns(*xt[4 + 5 * k: 9 + 5 * k]) for k in range(self.NM)]
            r = cmx.aerosol_activation_columns(p["ap"], modes, p["aip"], p["tps"], *xt[:4], want=("M_act", "S_max"))
        else:
            r = cmx.aerosol_activation(p["ap"], self._ad(), p["aip"], p["tps"], *xt, want=("M_act", "S_max"))
        return {"S_max": r.S_max.cpu().numpy(), **{f"M_act[{k}]": r.M_act[k].cpu().numpy() for k in range(self.NM)}}


# ---- P3 ------------------------------------------------------------------------------------------------------------------------------
N_P3 = 515            # the quadrature-heavy entries: 8 Float32 wavefronts + 3 points


def p3_states(ft):
    """(L_ice, N_ice, F_rim, ρ_rim, ρ_a, T) as P3State(params, L, N, F_rim, ρ_rim) takes them; T on both sides of T_freeze for the melt"""
    from cmx import synthetic
    st = synthetic.p3_state(N_P3, dtype=_t("f64"), seed=77)
    L, N, q_rim, b_rim = [c.numpy() for c in st]
    F = np.where(L > 0, q_rim / np.maximum(L, 1e-300), 0.0)
    rr = np.where(b_rim > 0, q_rim / np.maximum(b_rim, 1e-300), 400.0)
    rng = np.random.default_rng(61)
    return rounded([L, N, F, rr, synthetic.p3_air_density(N_P3, dtype=_t("f64")).numpy(), rng.uniform(268.0, 300.0, N_P3)], ft)


class P3Entry(Entry):
    """The P3 integrals at the log λ of the CONVERGED device shape solve (p3_shape, brent_iters = 40, with the same perturbed parameters), as their own parity
    tests do: the oracle evaluates the integral at that very log λ, so the unconverged-iterate question of ADVICE.md stays out.  For the liveness count (no
    device) the oracle's own converged solve (80 iterations) stands in."""
    family, skip_dead, ref_uses_got = "P3", True, True
    QUAD = 12
    states = staticmethod(p3_states)

    def params(self, td):
        return dict(p3=P.ParametersP3(td), vel=P.Chen2022VelTypeIce(td), aps=P.AirProperties(td), tps=P.ThermodynamicsParameters(td),
                    vent=P.VentilationFactorP3(td), quad=P.GaussLegendre(td, self.QUAD))

    def _ll(self, p, x64, ft, got):
        import oracle_binding as ob
        from cmx import _abi
        if got is not None:
            return np.asarray(got["_log_lambda"], dtype=np.float64)
        return ob.p3_shape(_abi.F64, p["p3"].c, _abi.CMX_P3_INPUT_IS_STATE | p["p3"].flags, *x64[:4], float32_gates=(ft == "f32"), maxiters=80, nthreads=8)["log_lambda"]

    def _dev_ll(self, p, xt):
        import cmx
        return cmx.p3_shape(p["p3"], *xt[:4], from_state=True, want=("log_lambda",), brent_iters=40).log_lambda


class P3Shape(P3Entry):
    """p3_shape(brent_iters = 40): log λ and D_m against the oracle's converged solve (80 iterations) with the same perturbed struct.
    The residual log(L/N)(log λ) has a multi-root band (8 ≤ log λ < 11): a state whose device log λ differs from the oracle's is set aside only if the
    ORACLE's residual at the device's log λ, with the perturbed struct, vanishes (≤ 1e-6 / 2e-3, the bound of tests/test_p3_gpu.py::
    test_random_state_parity_converged) — another genuine root — and such states stay within the cap on exclusions; any other disagreement fails.
    D_m inherits the root's error, |d ln D_m/d log λ| ≈ 1 with δ log λ ≤ RTOL·|log λ|: operand scale |D_m|·|log λ|·RTOL/CTOL."""
    entry, names = "p3_shape (brent_iters = 40)", ["log_lambda", "D_m"]

    def passed(self, p):
        return [p["p3"].c]

    def ref(self, p, x64, ft, got=None):
        import oracle_binding as ob
        from cmx import _abi
        flags = _abi.CMX_P3_INPUT_IS_STATE | p["p3"].flags
        r = ob.p3_shape(_abi.F64, p["p3"].c, flags, *x64[:4], float32_gates=(ft == "f32"), maxiters=80, nthreads=8)
        ll = r["log_lambda"]
        out = {"log_lambda": ll, "D_m": r["D_m"], "scale": {"D_m": np.abs(r["D_m"]) * np.abs(np.nan_to_num(ll, neginf=0.0)) * parity.RTOL[ft] / parity.CTOL[ft]}}
        other = np.zeros(ll.shape, dtype=bool)
        if got is not None:
            g = np.asarray(got["log_lambda"], dtype=np.float64)
            fin = np.isfinite(ll) & np.isfinite(g)
            for i in np.flatnonzero(fin & (np.abs(g - ll) > parity.RTOL[ft] * np.abs(ll))):
                res = ob.p3_logLdivN(_abi.F64, p["p3"].c, p["p3"].flags, x64[2][i], x64[3][i], g[i]) - (np.log(x64[0][i]) - np.log(x64[1][i]))
                other[i] = abs(res) <= (1e-6 if ft == "f64" else 2e-3)
        out["near_branch"] = other
        return out

    def gpu(self, p, xt):
        import cmx
        r = cmx.p3_shape(p["p3"], *xt[:4], from_state=True, want=("log_lambda", "D_m"), brent_iters=40)
        return {"log_lambda": r.log_lambda.cpu().numpy(), "D_m": r.D_m.cpu().numpy()}


class P3Velocities(P3Entry):
    entry, names = "p3_terminal_velocities", ["v_n", "v_m"]

    def passed(self, p):
        return [p["p3"].c, p["vel"]]

    def ref(self, p, x64, ft, got=None):
        import oracle_binding as ob
        from cmx import _abi
        v = ob.p3_terminal_velocities(_abi.F64, p["p3"].c, p["vel"], p["quad"], _abi.CMX_P3_INPUT_IS_STATE | p["p3"].flags, *x64[:5], self._ll(p, x64, ft, got),
                                      float32_gates=(ft == "f32"), nthreads=8)
        return dict(zip(self.names, v))

    def gpu(self, p, xt):
        import cmx
        ll = self._dev_ll(p, xt)
        v = cmx.p3_terminal_velocities(p["p3"], p["vel"], xt[4], *xt[:4], ll, from_state=True, quad=p["quad"])
        return {"v_n": v.v_n.cpu().numpy(), "v_m": v.v_m.cpu().numpy(), "_log_lambda": ll.cpu().numpy()}


class P3SelfCollection(P3Entry):
    entry, names = "p3_ice_self_collection", ["dNdt"]
    passed = P3Velocities.passed

    def ref(self, p, x64, ft, got=None):
        import oracle_binding as ob
        from cmx import _abi
        return {"dNdt": ob.p3_ice_self_collection(_abi.F64, p["p3"].c, p["vel"], p["quad"], _abi.CMX_P3_INPUT_IS_STATE | p["p3"].flags, *x64[:5],
                                                  self._ll(p, x64, ft, got), float32_gates=(ft == "f32"), nthreads=8)}

    def gpu(self, p, xt):
        import cmx
        ll = self._dev_ll(p, xt)
        return {"dNdt": cmx.p3_ice_self_collection(p["p3"], p["vel"], xt[4], *xt[:4], ll, from_state=True, quad=p["quad"]).cpu().numpy(), "_log_lambda": ll.cpu().numpy()}


class P3Melt(P3Entry):
    """p3_ice_melt ∝ T − T_freeze: operand scale = the rate at |T − T_freeze| = T_freeze (tests/test_p3_gpu.py::test_ice_melt)."""
    entry, names, context = "p3_ice_melt", ["dNdt", "dLdt"], ("P3 ventilation factor",)

    def passed(self, p):
        return [p["p3"].c, p["vel"], p["aps"], p["tps"], p["vent"]]

    def ref(self, p, x64, ft, got=None):
        import oracle_binding as ob
        from cmx import _abi
        dN, dL = ob.p3_ice_melt(_abi.F64, p["p3"].c, p["vel"], p["aps"], p["tps"], p["vent"], p["quad"], _abi.CMX_P3_INPUT_IS_STATE | p["p3"].flags, *x64[:4], x64[4],
                                x64[5], self._ll(p, x64, ft, got), float32_gates=(ft == "f32"), nthreads=8)
        Tf = p["p3"].c.T_freeze
        dT = np.maximum(np.abs(x64[5] - Tf), 1e-30)
        return {"dNdt": dN, "dLdt": dL, "scale": {"dNdt": np.abs(dN) * Tf / dT, "dLdt": np.abs(dL) * Tf / dT},
                "near_branch": np.abs(x64[5] - Tf) < (1e-4 if ft == "f32" else 1e-11)}

    def gpu(self, p, xt):
        import cmx
        ll = self._dev_ll(p, xt)
        r = cmx.p3_ice_melt(p["p3"], p["vel"], p["aps"], p["tps"], p["vent"], xt[5], xt[4], *xt[:4], ll, from_state=True, quad=p["quad"])
        return {"dNdt": r.dNdt.cpu().numpy(), "dLdt": r.dLdt.cpu().numpy(), "_log_lambda": ll.cpu().numpy()}


# ---- aerosol nucleation ----------------------------------------------------------------------------------------------------------------
class AerosolNucleation(Entry):
    """nucleation_rates (the fused pass) against tests/nucleation_ref.py, which takes the parameter structs as they are built from the dict."""
    family, entry, names = "aerosol nucleation", "nucleation_rates", ["binary", "ternary", "organic", "mixed"]
    COLS = ("h2so4", "nh3", "negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink")

    def states(self, ft):
        s, d = nucleation_state(N_POINTWISE, 17), nucleation_state(384, 18)
        # + 384 states with few or no negative ions: the ion count enters per m³ (Nucleation.jl:60-61), so the ion-induced terms bury the neutral ternary one
        # (p_t_n, p_A_n, a_n) at every chamber concentration — the reference's own known answers set negative_ion = 0
        rng = np.random.default_rng(19)
        d["negative_ion"] = np.where(rng.random(384) < 0.25, 0.0, _rng_block(rng, 384, 1e-3, 1e3))
        return rounded([np.concatenate([s[k], d[k]]) for k in self.COLS], ft)

    def params(self, td):
        return dict(hp=P.H2S04NucleationParameters(td), op=P.OrganicNucleationParameters(td), mp=P.MixedNucleationParameters(td))

    def ref(self, p, x64, ft):
        import nucleation_ref as R
        x = dict(zip(self.COLS, x64))
        with np.errstate(all="ignore"):
            b, t = R.h2so4_nucleation_rate(x["h2so4"], x["nh3"], x["negative_ion"], x["temp"], p["hp"])
            r = {"binary": b, "ternary": t,
                 "organic": R.organic_nucleation_rate(x["negative_ion"], x["monoterpene"], x["O3"], x["OH"], x["temp"], x["condensation_sink"], p["op"]),
                 "mixed": R.organic_and_h2so4_nucleation_rate(x["h2so4"], x["monoterpene"], x["OH"], x["temp"], x["condensation_sink"], p["mp"])}
        if ft == "f32":
            r["near_branch"] = self.ref_f32_range(p, x64, r)
        return r

    @staticmethod
    def _ternary_literal_f32(hp, h, a, ion, T):
        """Nucleation.jl:51-90 term by term in Float32, as the reference's own Float32 method evaluates it (k, f_y and the power are separate factors there)"""
        f = np.float32
        g = lambda n: f(getattr(hp, n))  # noqa: E731
        h, a, ion, T = (np.asarray(c, dtype=f) for c in (h, a, ion, T))
        with np.errstate(all="ignore"):
            h, a, ref = h * f(1e-6), a * f(1e-6), f(1e6)
            k = lambda u, v, w: np.exp(g(u) - np.exp(g(v) * (T / f(1000) - g(w))))  # noqa: E731
            fy = lambda pt, pA, ay: (a / ref) / (g(ay) + np.power(h / ref, g(pt)) / np.power(a / ref, g(pA)))  # noqa: E731
            t = (k("u_t_n", "v_t_n", "w_t_n") * fy("p_t_n", "p_A_n", "a_n") * np.power(h / ref, g("p_t_n"))
                 + k("u_t_i", "v_t_i", "w_t_i") * fy("p_t_i", "p_A_i", "a_i") * np.power(h / ref, g("p_t_i")) * ion)
            return (t * f(1e6)).astype(np.float64)

    def ref_f32_range(self, p, x64, r):
        """Float32 only: states at which the reference's OWN Float32 arithmetic leaves the float type's range in a factor (k_t_n = exp(u − exp(…)) balances two
        exponents near 200) — it returns 0 or a non-finite value where the Float64 value is representable.  Set aside like a branch point, under the same cap."""
        x = dict(zip(self.COLS, x64))
        lit = self._ternary_literal_f32(p["hp"], x["h2so4"], x["nh3"], x["negative_ion"], x["temp"])
        t = r["ternary"]
        # (values the metric can see: its floor hides differences below RTOL·FLOOR, its ceiling accepts an infinity above CEIL)
        return (np.abs(t) > parity.RTOL["f32"] * parity.FLOOR["f32"]) & (np.abs(t) < parity.CEIL["f32"]) & (~np.isfinite(lit) | (lit == 0))

    def gpu(self, p, xt):
        import cmx
        return _np_out(cmx.nucleation_rates(p["hp"], p["op"], p["mp"], **dict(zip(self.COLS, xt))), self.names)


# ---- the CPU builds of the device point functions (tests/native/point_host.cpp) -----------------------------------------------------
def host_call(lib, name, ft, head, cols, nout):
    import ctypes as C
    ct = {"f32": C.c_float, "f64": C.c_double}[ft]
    ptrs = lambda arrs: (C.POINTER(ct) * len(arrs))(*[a.ctypes.data_as(C.POINTER(ct)) for a in arrs])  # noqa: E731
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    y = [np.full_like(x[0], np.nan) for _ in range(nout)]
    fn = getattr(lib, f"{name}_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(x[0].size), ptrs(x), ptrs(y))
    return rc, y


def run_sweep(entry, ft, runner, sweep=None, only=None, base_live=None):
    """The loop both suites share: for every perturbation of the names `entry` reads, the oracle with the override against `runner(params, x)`
    → dict of outputs (None: liveness only).  Returns (Sweep, {perturbation key: liveness}, skipped perturbations)."""
    warnings.simplefilter("ignore", P.UnpinnedParameterWarning)      # the sweep overrides one name at a time; the others stay defaults on purpose
    sweep = sweep or Sweep(entry, ft)
    x, x64 = entry.states(ft)
    names = entry.read()
    cases, skipped = perturbations(names, tuple(entry.context) + (("Float32",) if ft == "f32" else ()), only, entry.base)
    ref0 = entry.ref(entry.params(P.ParamDict("f64", entry.base)), x64, ft)
    live = {}
    if runner is not None:
        got = runner(entry.params(P.ParamDict(ft, entry.base)), x)
        if got is not None:
            sweep.check(got, entry.ref(entry.params(P.ParamDict("f64", entry.base)), x64, ft, got) if entry.ref_uses_got else ref0, "defaults", entry.names)
    for c in cases:
        try:
            ref = entry.ref(entry.params(P.ParamDict("f64", c.override)), x64, ft)
        except Exception as e:                                                       # a constructor that refuses the value: a DOMAIN row is missing
            sweep.fail(c.key, f"the parameter structs could not be built: {e!r}")
            continue
        live[c.key] = liveness(ref0, ref, ref0.get("scale"), ft, entry.names)
        if runner is None or (entry.skip_dead and live[c.key] == 0):
            continue
        try:
            got = runner(entry.params(P.ParamDict(ft, c.override)), x)
        except Exception as e:
            sweep.fail(c.key, f"the entry refused the parameter set: {e!r}")
            continue
        if got is not None:
            if entry.ref_uses_got:
                ref = entry.ref(entry.params(P.ParamDict("f64", c.override)), x64, ft, got)
            sweep.check(got, ref, c.key, entry.names)
    sweep.live.update(live)
    return sweep, live, skipped


def all_entries():
    """Every swept entry, in the order the suites run them."""
    sb = [SbTendencies(lim, vel) for lim in (True, False) for vel in ("sb", "chen")]
    sb += [SbProcessRates(True), SbProcessRates(False), SbCloudVelocity(), SbColumn(True, "sb"), SbColumn(False, "chen")]
    sb += [Bulk2M(s) for s in ("KK2000", "B1994", "TC1980", "LD2004")] + [PrecipSusceptibility()]
    m1 = [Mp1mTendencies(o) for o in OPTION_SETS] + [Mp1mLinearized()]
    # two parameters are inert AT the defaults and live next to them: α of (N_c/1e8)^α, and r₀ of the cloud-ice mass relation (cancels for Δm = 0)
    m1 += [Mp1mSources("default"), Mp1mSources("alt", {"prescribed_cloud_droplet_number_concentration": 2e8}), Mp1mSources("sparse"),
           Mp1mSources("tdep", {"cloud_ice_mass_size_relation_coefficient_delm": 0.3})]
    m1 += [Sedimentation(), TerminalVelocity1M(), SnowVelocity(None), SnowVelocity("Oblate"), SnowVelocity("Prolate"), Mp1mColumn()]
    rest = [Mp0m(), CloudDiagnostics(True), CloudDiagnostics(False)]
    rest += [IceNucleationRates("Kaolinite", False), IceNucleationRates("Illite", True), WaterActivity(), H2SO4Solution()]
    rest += [DepositionJ(m) for m in ("Kaolinite", "Feldspar", "Ferrihydrite")] + [MohlerDeposition("DesertDust"), MohlerDeposition("ArizonaTestDust")]
    rest += [ArgActivation(False), ArgActivation(True)]
    rest += [P3Shape(), P3Velocities(), P3SelfCollection(), P3Melt(), AerosolNucleation()]
    return sb + m1 + rest


def run_cases(entry, ft, runner, cases, sweep=None, x=None):
    """`cases` = [(label, override)]: the oracle with each override against runner(params, x) on entry.states(ft) (or the given (x, x64))."""
    warnings.simplefilter("ignore", P.UnpinnedParameterWarning)
    sweep = sweep or Sweep(entry, ft)
    x, x64 = x or entry.states(ft)
    for label, ov in cases:
        ref = entry.ref(entry.params(P.ParamDict("f64", ov)), x64, ft)
        got = runner(entry.params(P.ParamDict(ft, ov)), x, label)
        sweep.check(got, ref, label, entry.names)
    return sweep


# ---- the Chen-2022 fit boundary --------------------------------------------------------------------------------------------------------
# make_chen_gamma / make_chen_log fit polynomials in ρ per parameter set and hand the set to the general (run-time Γ) instantiation when the fit misses its
# accuracy or a pole of Γ comes within the guard b₃ + 1 − 2 b_ρ > 0.05.  Two walks from the published table towards that boundary, 12 geometric steps each:
CHEN_STEPS = 12


def chen_boundary_cases():
    d = P.DEFAULT_PARAMETERS
    b, brho = d["Chen2022_table_B1_bi"], d["Chen2022_table_B1_b_rho_coeff"]
    cases = [("defaults", {})]
    for k in range(1, CHEN_STEPS + 1):
        v = brho * (0.6 / brho) ** (k / CHEN_STEPS)
        cases.append((f"b_rho = {v:.6g}", {"Chen2022_table_B1_b_rho_coeff": v}))
    g0 = b[2] + 1 - 2 * brho                                           # the smallest Γ argument of the third term over 0 ≤ ρ ≤ 2
    for k in range(1, CHEN_STEPS + 1):
        g = g0 * (0.05 / g0) ** (k / CHEN_STEPS)
        cases.append((f"b[2] = {g - 1 + 2 * brho:.6g} (b3 + 1 - 2 b_rho = {g:.4g})", {"Chen2022_table_B1_bi": (b[0], b[1], g - 1 + 2 * brho)}))
    return cases


def chen_density_probe(entry, ft):
    """64 states with rain at ρ = 2.5 kg/m³, outside the fitted Γ (ρ ≤ 2): a fitted instantiation must return NaN fall speeds there, the general one finite ones.
    Returns (columns, name of the rain fall-speed output)."""
    x = [np.array(c[:64], copy=True) for c in entry.states(ft)[0]]
    x[0][:] = 2.5
    if isinstance(entry, SbTendencies):
        x[5][:], x[6][:] = 1e-3, 1e4
        return x, "vt_rai_m"
    x[3][:] = 1e-3
    return x, "w_rai"


def chen_host_is_general(entry, rc):
    """what the host harness's return code says about the Chen-2022 instantiation: bit 1 of host_sb2006, the value of host_sedimentation"""
    return bool(rc & 2) if isinstance(entry, SbTendencies) else bool(rc)


# ---- aR ≥ bR ---------------------------------------------------------------------------------------------------------------------------
def aR_states(ft):
    """q_rai = 0 with N_rai > ϵ (λ_r → ∞: where the reference's exp(−2 r_c λ_r) overflows for aR ≥ bR), the converse, and ordinary rain."""
    rng = np.random.default_rng(51)
    m = 109
    base = [c[:3 * m] for c in _raw("sb")]
    q_rai = np.concatenate([np.zeros(m), _rng_block(rng, m, 1e-7, 2e-3), np.maximum(base[5][2 * m:], 0)])
    n_rai = np.concatenate([_rng_block(rng, m, 1e2, 1e8), np.zeros(m), np.maximum(base[6][2 * m:], 0)])
    q_vap = np.maximum(base[2] - np.maximum(base[3], 0) - np.maximum(base[5], 0), 0)
    return rounded([base[0], base[1], q_vap + np.maximum(base[3], 0) + q_rai, base[3], base[4], q_rai, n_rai], ft)


def aR_override(factor):
    return {"SB2006_raindrops_terminal_velocity_coeff_aR": P.DEFAULT_PARAMETERS["SB2006_raindrops_terminal_velocity_coeff_bR"] * factor}
