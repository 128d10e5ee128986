"""Parameters, reference and error measure of the derivatives of the 1-moment tendencies with respect to the scheme's PARAMETERS (include/cmx.h §23), shared by
tests/test_param_1m_host.py and tests/test_param_1m_gpu.py: the 1-moment twin of tests/param_cases.py, whose measure (`row_error`, `shares`), bounds and
1 % cap it uses unchanged.

REFERENCE.  Central differences of the Float64 ORACLE (oracle_binding.mp1m) with respect to one ClimaParams name at a time, θ_p ± h with h = 1e-6·|θ_p| (and
4h), both structs rebuilt by the constructors from the overridden dictionary, held as logarithmic sensitivities S_op = ∂out_o/∂θ_p·θ_p.  NAMES: every name of
`parameters.MICROPHYSICS_1M_DIRECTION_NAMES` whose value is not zero in the case's dictionary (a zero θ has no logarithmic sensitivity and no step 1e-6·|θ|:
the three Δ exponents that default to 0 are covered where the "exponents" dictionary of tests/jacobian_1m_cases.py gives them a value).

CASES: "default" (the compile-time instantiation unless a direction moves one of its nine exponents), "alt" (the four alternative options of
jacobian_1m_cases.ALT_OPTIONS: the run-time-flags instantiation), "exponents" (general exponents).  SETS: "cold" and "warm" of jacobian_1m_cases.states (4096
states each), and "limiters": 512 states with traces of rain and snow (10⁻¹² … 10⁻⁷ kg/kg), where the floors of the slope parameters λ⁻¹ ≥ r0·10⁻⁵ and the
evaporation / sublimation limiters bind, so that the length scales act through the floors.  Cloud liquid and cloud ice keep the range of the other sets: a
first draw with cloud ice as a trace too put the snow row at the size of the cloud-ice autoconversion of q_icl ≪ q_threshold, the logistic integral
log((1 − e⁻ᵏ) + e⁻ᵏ eʸ) at y → 0, whose Float32 absolute error is eps·x0/k whatever x is (csrc/cmx_mp1m.hpp logistic_rate): there the Float32 host build
showed 1.1e-3 in the row measure for threshold_smooth_transition_steepness (Float64 passed).  That is the conditioning of the Float32 primal at a state the set
is not about, not a limiter; the cloud species were moved back instead of the bound.
"""
import functools

import numpy as np

import jacobian_1m_cases as j1
import param_cases as pc
from cmx import _abi
from cmx import parameters as P

OUT = _abi.MP1M_JAC_OUT
BOUND, AGREE, MAX_SET_ASIDE, LOW_SHARE = pc.BOUND, pc.AGREE, pc.MAX_SET_ASIDE, pc.LOW_SHARE
CASES = ("default", "alt", "exponents")
SETS = ("cold", "warm", "limiters")
# the size-relation exponents of rain and snow: a direction on one of them selects the run-time-flags instantiation
EXPONENT_NAMES = tuple(k for k in P.MICROPHYSICS_1M_DIRECTION_NAMES if k.startswith(("rain_", "snow_")) and "size_relation_coefficient" in k
                       and not k.endswith(("chim", "chia", "chiv")))


def overrides(case):
    return dict(j1.EXPONENT_OVERRIDES) if case == "exponents" else {}


def options(case):
    return j1.ALT_OPTIONS if case == "alt" else {}


def names(case):
    ov = overrides(case)
    return tuple(k for k in P.MICROPHYSICS_1M_DIRECTION_NAMES if ov.get(k, P.DEFAULT_PARAMETERS[k]) != 0)


def theta(case, nm=None):
    ov = overrides(case)
    return np.array([ov.get(k, P.DEFAULT_PARAMETERS[k]) for k in (names(case) if nm is None else nm)], dtype=np.float64)


def params(ft, case, ov=None):
    td = P.create_toml_dict(ft, overrides(case) if ov is None else ov)
    return P.Microphysics1MParams(td, **options(case)), P.ThermodynamicsParameters(td)


def pairs(mp, case, nm):
    """Direction p = θ_p along nm[p]: a jvp column is the logarithmic sensitivity S_·p."""
    return [P.parameter_direction(mp, {k: float(t)}) for k, t in zip(nm, theta(case, nm))]


def limiter_states(n=512, seed=13):
    import oracle_binding as oracle
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.4, 1.2, n)
    T = np.where(rng.uniform(size=n) < 0.5, rng.uniform(235.0, 272.65, n), rng.uniform(273.65, 300.0, n))
    q_lcl, q_icl = 10.0 ** rng.uniform(-6.0, -3.0, n), 10.0 ** rng.uniform(-6.0, -3.0, n)
    q_rai, q_sno = 10.0 ** rng.uniform(-12.0, -7.0, n), 10.0 ** rng.uniform(-12.0, -7.0, n)
    q_tot = (q_lcl + q_icl + q_rai + q_sno) + j1.q_sat_liquid(oracle, T, rho) * rng.uniform(0.5, 1.05, n)
    return [rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno]


def states(which):
    import oracle_binding as oracle
    return limiter_states() if which == "limiters" else j1.states(oracle, which)


def _oracle(case, ov, cols):
    import oracle_binding as oracle
    mp, tps = params("f64", case, ov)
    r = oracle.mp1m(_abi.F64, mp.c, tps, mp.flags, *cols, nthreads=8, want_sources=False)
    return np.stack([r[k] for k in OUT])


def fd_sensitivities(case, cols, nm, step):
    base = overrides(case)
    S = np.empty((len(OUT), len(nm), cols[0].size))
    for p, (k, t) in enumerate(zip(nm, theta(case, nm))):
        h = step * abs(t)
        tp, tm = t + h, t - h
        S[:, p] = (_oracle(case, {**base, k: tp}, cols) - _oracle(case, {**base, k: tm}, cols)) / (tp - tm) * t
    return S


@functools.lru_cache(maxsize=None)
def _reference(case, which):
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in states(which)]
    nm = names(case)
    S1, S4 = fd_sensitivities(case, cols, nm, 1e-6), fd_sensitivities(case, cols, nm, 4e-6)
    disagree = pc.row_error(S1, S4).max(axis=(0, 1))
    kept = disagree <= AGREE
    dead = np.array([not S1[:, p].any() and not S4[:, p].any() for p in range(len(nm))])
    # [4, P]: the column is RESOLVED in its own scale — the references at h and 4h agree within AGREE of the column's largest entry over the kept states.  A
    # column that is not (central differences of a quantity that cancels analytically: rounding noise of the oracle, 1e-10 of the row) has no derivative to
    # compare with in that scale; the row measure still holds for it
    top = np.abs(S1)[:, :, kept].max(axis=2)
    resolved = (top > 0) & (np.abs(S1 - S4)[:, :, kept].max(axis=2) <= AGREE * top)
    for a in (*cols, S1, kept, dead, resolved):
        a.setflags(write=False)
    return cols, S1, kept, dead, float(disagree[kept].max()), resolved


def reference(case, which):
    """(cols, S^ref [4, P, n], kept [n], dead [P], worst h-vs-4h disagreement among the kept, resolved [4, P]); asserts the 1 % cap."""
    ref = _reference(case, which)
    kept = ref[2]
    assert (~kept).sum() <= MAX_SET_ASIDE * kept.size, (case, which, int((~kept).sum()), kept.size)
    return ref


def assert_parity(ft, S, case, which, what):
    """Every (row, parameter) of every kept state inside BOUND[ft]; every dead parameter exactly zero at every state; Float64: the live parameters whose
    largest row share is below LOW_SHARE also in the column's own scale, max_i |S − S^ref| ≤ 1e-5·max_i |S^ref| per row (printed)."""
    cols, S_ref, kept, dead, worst_fd, resolved = reference(case, which)
    nm = names(case)
    S = np.asarray(S, dtype=np.float64)
    e = pc.row_error(S, S_ref)[:, :, kept].max(axis=(0, 2))
    print(f"{what} {ft} {case} {which}: kept {int(kept.sum())}/{kept.size}, h-vs-4h {worst_fd:.3g}, worst {e.max():.3g} ({nm[int(e.argmax())]}), "
          f"{int(dead.sum())} dead of {len(nm)}")
    for p in np.nonzero(dead)[0]:
        assert not S[:, p].any(), (what, case, which, nm[p], "dead in the reference, not exactly zero")
    for p in np.nonzero(~(e < BOUND[ft]))[0]:
        raise AssertionError((what, case, which, nm[p], float(e[p])))
    if ft == "f64":
        assert_low_share_columns(S, S_ref, kept, dead, resolved, nm, what)
    return e


def assert_low_share_columns(S, S_ref, kept, dead, resolved, nm, what, report=True):
    """The live parameters whose largest row share is below LOW_SHARE, in the column's own scale, for every row the reference resolves in that scale
    (`_reference`); prints which ones and which rows are not resolved."""
    sh = pc.shares(S_ref, kept)
    low = [p for p in range(len(nm)) if not dead[p] and sh[p] < LOW_SHARE]
    for p in low:
        d = np.abs(S[:, p][:, kept] - S_ref[:, p][:, kept]).max(axis=1)
        scale = np.abs(S_ref[:, p][:, kept]).max(axis=1)
        rows = resolved[:, p] & (scale > 0)
        if report:
            print(f"  {what}: low share {sh[p]:.2g} {nm[p]}: column-scale error {np.max(np.where(rows, d / np.where(scale > 0, scale, 1.0), 0.0)):.3g}"
                  + (f", rows the reference does not resolve: {[OUT[o] for o in np.nonzero(~rows & (scale > 0))[0]]}" if (~rows & (scale > 0)).any() else ""))
        assert (d[rows] <= 1e-5 * scale[rows]).all(), (what, nm[p], d, scale, rows)
    return low
