"""Parameters, reference and error measure shared by tests/test_param_derivatives_host.py and tests/test_param_derivatives_gpu.py: the derivatives of the SB2006 warm-rain tendencies with respect to the scheme's PARAMETERS (include/cmx.h §22).

REFERENCE.  Central differences of the Float64 ORACLE with respect to one ClimaParams name at a time: θ_p ± h with h = 1e-6·|θ_p| (and 4h), both parameter
structs rebuilt by the constructors of cmx.parameters from the overridden dictionary — so a name that feeds several fields, or derived ones, moves all of
them — the quotient formed with the realised θ⁺ − θ⁻, held as logarithmic sensitivities S_op = ∂out_o/∂θ_p·θ_p (the tendency's units, whatever the
parameter's).  The code under test returns S directly: its direction for name p is `parameter_direction(params, {p: θ_p})`.

MEASURE.  Per state and row, e_op = |S_op − S^ref_op| / s_o with s_o = max_p max(|S_op|, |S^ref_op|) over the tested parameters; a row with s_o = 0 must be
exactly zero.  A state is kept only if the references at h and 4h agree within jacobian_cases.AGREE (2e-6) in that measure; at most
jacobian_cases.MAX_SET_ASIDE (1 %) of a set may be set aside (asserted where the reference is built).  Bounds: jacobian_cases.BOUND (Float64 1e-5, Float32
1e-3).  A parameter whose reference is identically zero at h and 4h on a set is DEAD there: the code under test must return exactly 0 for it.  A live
parameter whose largest share |S^ref_op|/s_o stays below LOW_SHARE (0.02) on a set is poorly resolved by the row measure; for it the Float64 result is also
held in the column's own scale, max_i |S − S^ref| ≤ 1e-5·max_i |S^ref| per row (`assert_low_share_columns` prints which ones).

SETS.  `interior`: the 4096 interior states of tests/jacobian_cases.py (all four species present, away from the gates), on which the number-adjustment
limiters do not bind and the mean rain-drop mass stays inside its limits.  `limiters`: a small second set that drives them — droplets and drops with mean
masses below x_min and above x_max, so that SB2006_cloud_droplets_min_mass, SB2006_raindrops_max_mass and the adjustment timescale act.
"""
import functools

import numpy as np

import jacobian_cases as jc
from cmx import _abi
from cmx import parameters as P

OUT = _abi.SB2006_JAC_OUT
BOUND, AGREE, MAX_SET_ASIDE = jc.BOUND, jc.AGREE, jc.MAX_SET_ASIDE
LOW_SHARE = 0.02

# every name of the direction table except the thermodynamic constants that the warm-rain tendencies do not read
NAMES = tuple(k for k in P.WARM_RAIN_2M_DIRECTION_FIELDS
              if k not in ("gas_constant_dry_air", "isobaric_specific_heat_ice", "latent_heat_sublimation_at_reference", "temperature_water_freeze",
                           "isochoric_specific_heat_liquid"))
EXPONENTS = ("SB2006_autoconversion_correcting_function_coeff_b", "SB2006_accretion_correcting_function_coeff_c", "SB2006_raindrops_self-collection_coeff_d")


def overrides(perturbed):
    return jc.perturbed_overrides() if perturbed else {}


def theta(perturbed, names=NAMES):
    ov = overrides(perturbed)
    return np.array([ov.get(k, P.DEFAULT_PARAMETERS[k]) for k in names], dtype=np.float64)


def params(ft, limited, ov):
    """(WarmRainParams2M, thermodynamics struct) of the float type from one overridden dictionary."""
    td = P.create_toml_dict(ft, ov)
    return P.WarmRainParams2M(td, limited), P.ThermodynamicsParameters(td)


def directions(ft, limited, perturbed, names=NAMES):
    """(wr, tps, d_wr[len(names)], d_tps[len(names)]): direction p is θ_p along name p, so that a jvp column is the logarithmic sensitivity S_·p."""
    wr, tps = params(ft, limited, overrides(perturbed))
    th = theta(perturbed, names)
    pairs = [P.parameter_direction(wr, {k: float(t)}) for k, t in zip(names, th)]
    d_wr = (type(wr.c) * len(names))(*[a for a, _ in pairs])
    d_tps = (type(tps) * len(names))(*[b for _, b in pairs])
    return wr, tps, d_wr, d_tps


def limiter_states(n=512, seed=11):
    """Droplets and drops outside the mass limits of the number adjustment: x̄_c = q_lcl/n_lcl from 1e-16 to 1e-8 kg (limits 4.2e-15, 2.6e-10), x̄_r = q_rai/n_rai
    from 1e-11 to 1e-4 kg (limits 2.6e-10, 5e-6); the rest as the interior set."""
    import oracle_binding as oracle
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.6, 1.2, n)
    T = rng.uniform(275.0, 300.0, n)
    q_lcl = 10.0 ** rng.uniform(-5.0, -2.7, n)
    q_rai = 10.0 ** rng.uniform(-6.0, -2.7, n)
    n_lcl = q_lcl / 10.0 ** rng.uniform(-16.0, -8.0, n)
    n_rai = q_rai / 10.0 ** rng.uniform(-11.0, -4.0, n)
    q_tot = q_lcl + q_rai + jc.q_sat(oracle, T, rho) * rng.uniform(0.5, 1.05, n)
    return [rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai]


def states(which):
    import oracle_binding as oracle
    return jc.interior_states(oracle) if which == "interior" else limiter_states()


def _oracle(limited, ov, cols):
    import oracle_binding as oracle
    wr, tps = params("f64", limited, ov)
    flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006
    r = oracle.sb2006_warm_rain_tendencies(_abi.F64, wr.c, tps, P.rain_vel_params("f64"), flags, *cols, nthreads=8, want_scale=False)
    return np.stack([r[k] for k in OUT])


def fd_sensitivities(limited, perturbed, cols, names, step):
    """[4, len(names), n]: S^ref by central differences of the oracle with h = step·|θ_p|."""
    base = overrides(perturbed)
    S = np.empty((len(OUT), len(names), cols[0].size))
    for p, (k, t) in enumerate(zip(names, theta(perturbed, names))):
        h = step * abs(t)
        tp, tm = t + h, t - h
        S[:, p] = (_oracle(limited, {**base, k: tp}, cols) - _oracle(limited, {**base, k: tm}, cols)) / (tp - tm) * t
    return S


def row_error(S, S_ref):
    """[4, P, n]: e_op = |S_op − S^ref_op| / s_o, s_o = max_p max(|S_op|, |S^ref_op|); 0 where a row with s_o = 0 is exactly zero in both, Inf where it is not
    or an entry is not finite."""
    S, S_ref = np.asarray(S, dtype=np.float64), np.asarray(S_ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.maximum(np.abs(S).max(axis=1), np.abs(S_ref).max(axis=1))[:, None, :]
        e = np.where(s > 0, np.abs(S - S_ref) / s, np.where((S == 0) & (S_ref == 0), 0.0, np.inf))
    return np.where(np.isfinite(e), e, np.inf)


@functools.lru_cache(maxsize=None)
def _reference(limited, perturbed, which):
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in states(which)]
    S1, S4 = fd_sensitivities(limited, perturbed, cols, NAMES, 1e-6), fd_sensitivities(limited, perturbed, cols, NAMES, 4e-6)
    disagree = row_error(S1, S4).max(axis=(0, 1))
    kept = disagree <= AGREE
    dead = np.array([not S1[:, p].any() and not S4[:, p].any() for p in range(len(NAMES))])
    for a in (*cols, S1, kept, dead):
        a.setflags(write=False)
    return cols, S1, kept, dead, float(disagree[kept].max())


def reference(limited, perturbed=False, which="interior"):
    """(cols, S^ref [4, P, n], kept [n], dead [P], worst h-vs-4h disagreement among the kept) of a set, computed once and shared read-only; asserts the 1 % cap."""
    ref = _reference(bool(limited), bool(perturbed), which)
    kept = ref[2]
    assert (~kept).sum() <= MAX_SET_ASIDE * kept.size, (which, limited, perturbed, int((~kept).sum()), kept.size)
    return ref


def shares(S_ref, kept):
    """[P]: the largest share |S^ref_op|/s_o a parameter reaches in any row at any kept state."""
    A = np.abs(S_ref)[:, :, kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nan_to_num(A / A.max(axis=1, keepdims=True)).max(axis=(0, 2))


def assert_parity(ft, S, limited, perturbed, which, what):
    """Every (row, parameter) of every kept state inside BOUND[ft]; every dead parameter exactly zero at EVERY state; Float64: the low-share columns also in
    their own scale.  Prints and returns the worst error per parameter."""
    cols, S_ref, kept, dead, worst_fd = reference(limited, perturbed, which)
    S = np.asarray(S, dtype=np.float64)
    e = row_error(S, S_ref)[:, :, kept].max(axis=(0, 2))
    print(f"{what} {ft} limited={limited} perturbed={perturbed} {which}: kept {int(kept.sum())}/{kept.size}, h-vs-4h {worst_fd:.3g}, worst {e.max():.3g} "
          f"({NAMES[int(e.argmax())]}), dead: {[NAMES[p] for p in np.nonzero(dead)[0]]}")
    for p in np.nonzero(dead)[0]:
        assert not S[:, p].any(), (what, which, NAMES[p], "dead in the reference, not exactly zero")
    for p in np.nonzero(~(e < BOUND[ft]))[0]:
        raise AssertionError((what, which, NAMES[p], float(e[p])))
    if ft == "f64":
        assert_low_share_columns(S, S_ref, kept, dead, what)
    return e


def assert_low_share_columns(S, S_ref, kept, dead, what, report=True):
    """The live parameters whose largest row share is below LOW_SHARE, in the column's own scale per row: max_i |S − S^ref| ≤ 1e-5·max_i |S^ref|."""
    sh = shares(S_ref, kept)
    low = [p for p in range(len(NAMES)) if not dead[p] and sh[p] < LOW_SHARE]
    for p in low:
        d = np.abs(S[:, p][:, kept] - S_ref[:, p][:, kept]).max(axis=1)
        scale = np.abs(S_ref[:, p][:, kept]).max(axis=1)
        if report:
            print(f"  {what}: low share {sh[p]:.2g} {NAMES[p]}: column-scale error {np.max(d / np.where(scale > 0, scale, 1.0)):.3g}")
        assert (d <= 1e-5 * scale).all(), (what, NAMES[p], d, scale)
    return low
