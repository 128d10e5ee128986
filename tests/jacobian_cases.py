"""States, reference and error measure shared by tests/test_sb2006_jacobian_host.py and tests/test_sb2006_jacobian_gpu.py.

The reference Jacobian is the method of the reference's own test (test/ad_compat_tests.jl:143-165): central differences of the Float64 ORACLE
tendencies (oracle_binding.sb2006_warm_rain_tendencies, _abi.F64) with step h = 1e-6·|x_j|, the quotient formed with the realised x⁺ − x⁻, compared
row by row in the scale s_i = max_j max(|J_ij|, |J^fd_ij|); a row with s_i = 0 must be exactly zero.  A state is KEPT only if the references at h and
at 4h agree within 2e-6 in that measure: a state that sits on a kink of the tendency function (a min / max / clamp changing sides inside the stencil)
has no derivative to compare with.  At most 1 % of a set may be set aside (asserted where the set is built).

Float32 is compared with the SAME Float64 reference at the project's Float32 bound 1e-3 in the same per-row measure: all four rows with the default
parameter sets, three rows with the perturbed set.  The one exception is dn_rai_dt with the perturbed parameter set, which cannot meet it (2.2e-3 at one
state of 4096 in the host build, 2.3e-3 on the device; HISTORY.md has the decomposition): there ∂dn_rai_dt/∂q_rai is evaporation (−5.6e5) against
autoconversion (+5.8e5) leaving 7e3, and the evaporation rate is LINEAR in the supersaturation S = q_vap/q_sat − 1 with q_vap = q_tot − q_lcl − q_rai,
two cancelling differences.  That row is held, entry by entry, to 1e-3·s_i + ε_i·|E_ij| (`float32_bound`), both factors taken from the ORACLE, not from
the code under test:
  * E_ij = the evaporation share of the reference Jacobian, central differences of the oracle's evaporation rate (`evaporation_share`);
  * ε_i = the Float32-against-Float64 spread of that row's evaporation primal (`evaporation_spread_f32`).  The oracle evaluates evap_dN_rai_dt in Float32
    and in Float64 arithmetic on the whole interior set; its relative spread follows c·u/|S_i| (u = 2⁻²⁴: an absolute rounding error of S + 1 ≈ 1
    divided by |S|), and ε_i = c·u/|S_i| with c the LARGEST constant measured on the set, c = max_k spread_k·|S_k|/u (38 here).  The spread of a single
    state is one sample of rounding and no bound — the oracle's own is 1.5e-5 at the state in question where this library's Float32 primal shows 2.9e-5 —
    which is why the set's worst constant is used with the 1/|S| law; a first-order worst-case analysis of S + 1 = q_vap·ρ·R_v·T/p_sat(T) in Float32
    (rounded inputs, the roundings of log2 p_sat amplified by L/(R_v T) ≈ 18) gives c ≤ 158, so the measured constant is the tighter of the two.

THE SECOND MEASURE.  The six inputs carry different units (K, kg/kg, 1/kg): a ∂/∂q entry is about 4f/q with q ≈ 1e-4, a ∂/∂n entry about 2f/n with n ≈ 1e8, a
∂/∂T entry about 0.06f, so s_i is set by the q columns and the other three sit far below any bound in the per-row measure — median |J^ref_ij|/s_i on the
interior set: T 7e-6 … 3e-5, n_lcl 5e-16 … 3e-12, n_rai 9e-9 … 2e-8; the whole n_lcl column scaled by 1.1, zeroed or negated passes it in both float types.
`assert_parity` therefore asserts, next to it and with nothing of it removed, the input-scaled measure (`input_scaled_error`)
  e_ij = |J_ij − J^ref_ij|·|x_j| / s'_i,   s'_i = max_j max(|J_ij|, |J^ref_ij|)·|x_j|,
x the Float64 state columns of the reference: the row's sensitivity to a RELATIVE perturbation of each input, dimensionless.  A row with s'_i = 0 must be
exactly zero, a non-finite entry gives Inf.  Same bounds (Float64 1e-5, Float32 1e-3), every (row, column), NO exception row — dn_rai_dt with the perturbed
set, which needs `float32_bound` in the per-row measure, is at 5.3e-6 in this one.  A state is kept only if h and 4h agree within 2e-6 in BOTH measures
(`disagreement`); the 1 % cap applies to the union (0 of 4096 set aside in all three cases; worst disagreement in the new measure 2.0e-8).
That both measures can fail is tested in tests/test_sb2006_jacobian_host.py: each input column scaled by 1.1 (0.091 in the new measure), zeroed or negated
is rejected, and `assert_resolution` requires from the reference alone that every structurally non-zero entry reaches 1 % of its row in one of the two
measures at some kept state (smallest shares on the interior set: dq_lcl_dt × n_lcl 0.02 … 0.03, dq_rai_dt × n_rai 0.02 … 0.04, every other ≥ 0.57).

Worst input-scaled value per row over the three cases and both sets (column and case of the worst in brackets), host build | device (MI355X):
  Float64   dq_lcl_dt 1.5e-10 | 1.5e-10 (T, perturbed)   dn_lcl_dt 4.2e-9 | 4.2e-9 (q_rai)   dq_rai_dt 1.6e-8 | 1.6e-8 (q_rai)   dn_rai_dt 2.3e-8 | 2.3e-8 (q_rai)
  Float32   dq_lcl_dt 1.6e-6 | 1.8e-6 (T)   dn_lcl_dt 2.2e-6 | 1.9e-6 (n_lcl | q_rai, perturbed)   dq_rai_dt 2.3e-6 | 2.8e-6 (T)   dn_rai_dt 5.2e-6 | 5.3e-6 (q_rai, perturbed)
The Float32 T column, taken through the hardware's exp2 / log2 on the device and through libm in the host build: ≤ 2.7e-6 | ≤ 2.9e-6 in every row.
"""
import functools

import numpy as np

from cmx import _abi
from cmx import parameters as P

WRT = _abi.SB2006_JAC_WRT          # T, q_tot, q_lcl, n_lcl, q_rai, n_rai = columns 1 … 6 of the state
OUT = _abi.SB2006_JAC_OUT
BOUND = {"f64": 1e-5, "f32": 1e-3}         # f64: the reference's own bound (ad_compat_tests.jl:163); f32: the project's Float32 bound
AGREE = 2e-6
MAX_SET_ASIDE = 0.01

# the reference's "warm rain" regime (ad_compat_tests.jl:121-122), the KAT state of tests/test_abi_caller.py:135 and the boundary state of
# ad_compat_tests.jl:170-174 (zero rain with cloud present); order rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai
WARM_RAIN = (1.05, 288.0, 0.015, 4e-4, 8e7, 2.1e-3, 5e4)
KAT = (1.2, 290.0, 7e-3, 2e-3, 1e8 / 1.2, 5e-4, 1e7 / 1.2)
BOUNDARY = (0.45, 233.0, 0.003, 1e-6, 1e6, 0.0, 0.0)


def q_sat(oracle, T, rho):
    tps = P.ThermodynamicsParameters("f64")
    p = np.array([oracle.psat_liquid(_abi.F64, tps, float(t)) for t in T])
    return p / (rho * tps.R_v * T)


def interior_states(oracle, n=4096, seed=7):
    """All four species present, away from the gates (the issue's recipe, drawn in this order)."""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.6, 1.2, n)
    T = rng.uniform(275.0, 300.0, n)
    q_lcl = 10.0 ** rng.uniform(-5.0, -2.7, n)
    q_rai = 10.0 ** rng.uniform(-6.0, -2.7, n)
    n_lcl = q_lcl / 10.0 ** rng.uniform(-12.2, -10.0, n)
    n_rai = q_rai / 10.0 ** rng.uniform(-9.5, -6.2, n)
    q_tot = q_lcl + q_rai + q_sat(oracle, T, rho) * rng.uniform(0.5, 1.05, n)
    return [rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai]


def points(*states):
    """Single states → columns."""
    return [np.array(c, dtype=np.float64) for c in zip(*states)]


def warm_rain_params(ft, limited, overrides=None):
    return P.WarmRainParams2M(P.create_toml_dict(ft, overrides), limited) if overrides else P.WarmRainParams2M(ft, limited)


def perturbed_overrides(seed=1):
    """Every SB2006 / air / relaxation parameter scaled by a random factor in [0.8, 1.25], as tests/test_point_host.py:265-277 builds it: the three
    "integer" exponents become general ones, so the exp2(e·log2 x) instantiation runs."""
    rng = np.random.default_rng(seed)
    names = [k for k in P.DEFAULT_PARAMETERS if k.startswith("SB2006_") and "distribution_coeff_nu" not in k and "distribution_coeff_mu" not in k]
    names += ["condensation_evaporation_timescale", "thermal_conductivity_of_air", "diffusivity_of_water_vapor", "kinematic_viscosity_of_air"]
    names = [k for k in names if k in P.DEFAULT_PARAMETERS and isinstance(P.DEFAULT_PARAMETERS[k], float)]
    return {k: P.DEFAULT_PARAMETERS[k] * rng.uniform(0.8, 1.25) for k in names}


def oracle_tendencies(oracle, wr64, limited, cols):
    flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006
    r = oracle.sb2006_warm_rain_tendencies(_abi.F64, wr64.c, P.ThermodynamicsParameters("f64"), P.rain_vel_params("f64"), flags,
                                           *[np.ascontiguousarray(c, dtype=np.float64) for c in cols], nthreads=8, want_scale=False)
    return np.stack([r[k] for k in OUT])


def fd_jacobian(tendencies, cols, step=1e-6):
    """[n_out, n_wrt, n]: central differences of tendencies(cols) → [n_out, n] (the ORACLE's, Float64) with h = step·|x_j|, divided by the realised
    x⁺ − x⁻; cols[0] = ρ is not differentiated."""
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    J = None
    for j in range(len(cols) - 1):
        x = cols[j + 1]
        h = step * np.abs(x)
        xp, xm = x + h, x - h
        fp, fm = tendencies(cols[:j + 1] + [xp] + cols[j + 2:]), tendencies(cols[:j + 1] + [xm] + cols[j + 2:])
        J = np.empty((fp.shape[0], len(cols) - 1, x.size)) if J is None else J
        J[:, j] = (fp - fm) / (xp - xm)
    return J


def evaporation_share(oracle, wr64, limited, cols, step=1e-6):
    """[4, 6, n]: the part of the reference Jacobian that comes from rain evaporation (CM2:780-828) — central differences of the oracle's
    evap_dq_rai_dt (row dq_rai_dt) and evap_dN_rai_dt/ρ (row dn_rai_dt); the cloud rows have none."""
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006

    def ev(c):
        rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai = c
        r = oracle.sb2006_process_rates(_abi.F64, wr64.c, P.ThermodynamicsParameters("f64"), P.rain_vel_params("f64"), flags,
                                        *[np.ascontiguousarray(a) for a in (q_tot, q_lcl, q_rai, rho * n_lcl, rho * n_rai, rho, T)])
        return np.stack([r["evap_dq_rai_dt"], r["evap_dN_rai_dt"] / rho])
    E = np.zeros((4, 6, cols[0].size))
    for j in range(6):
        x = cols[j + 1]
        h = step * np.abs(x)
        xp, xm = x + h, x - h
        E[2:, j] = (ev(cols[:j + 1] + [xp] + cols[j + 2:]) - ev(cols[:j + 1] + [xm] + cols[j + 2:])) / (xp - xm)
    return E


def supersaturation(oracle, cols):
    rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai = [np.asarray(c, dtype=np.float64) for c in cols]
    return (q_tot - q_lcl - q_rai) / q_sat(oracle, T, rho) - 1.0


@functools.lru_cache(maxsize=None)
def evaporation_spread_constant(limited, perturbed):
    """c = max over the interior set of (relative Float32-against-Float64 spread of the oracle's evap_dN_rai_dt)·|S|/u, u = 2⁻²⁴ (module docstring)."""
    import oracle_binding as oracle
    ov = perturbed_overrides() if perturbed else None
    rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai = cols = interior_states(oracle)
    flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006
    ev = {}
    for fam in (_abi.F64, _abi.F32):          # the ARITHMETIC; the gates are the Float64 ones in both, as for the reference Jacobian
        r = oracle.sb2006_process_rates(fam, warm_rain_params(fam.sfx, limited, ov).c, P.ThermodynamicsParameters(fam.sfx), P.rain_vel_params(fam.sfx), flags,
                                        q_tot, q_lcl, q_rai, rho * n_lcl, rho * n_rai, rho, T, float32_gates=False)
        ev[fam.sfx] = r["evap_dN_rai_dt"].astype(np.float64)
    on = ev["f64"] != 0
    assert on.sum() > 0.5 * on.size                      # evaporation acts on most of the set (S < 0)
    spread = np.abs(ev["f32"] - ev["f64"])[on] / np.abs(ev["f64"][on])
    return float((spread * np.abs(supersaturation(oracle, cols))[on]).max() / 2.0 ** -24)


def evaporation_spread_f32(oracle, limited, perturbed, cols):
    """ε_i = c·u/|S_i| per state (module docstring)."""
    with np.errstate(divide="ignore"):
        return evaporation_spread_constant(bool(limited), bool(perturbed)) * 2.0 ** -24 / np.abs(supersaturation(oracle, cols))


def float32_bound(J, J_ref, E, eps_S):
    """[4, 6, n]: the Float32 entry bound of |J_ij − J^ref_ij| for the row that cannot meet the plain one (module docstring): 1e-3·s_i + ε_i·|E_ij|."""
    s = np.maximum(np.abs(np.asarray(J, dtype=np.float64)).max(axis=1), np.abs(J_ref).max(axis=1))
    return BOUND["f32"] * s[:, None, :] + eps_S[None, None, :] * np.abs(E)


def scaled_error(J, J_ref):
    """[4, n]: max_j |J_ij − J^ref_ij| / s_i with s_i = max_j max(|J_ij|, |J^ref_ij|) per state; a row with s_i = 0 is exactly zero in both: error 0.
    A non-finite entry gives Inf."""
    J, J_ref = np.asarray(J, dtype=np.float64), np.asarray(J_ref, dtype=np.float64)
    s = np.maximum(np.abs(J).max(axis=1), np.abs(J_ref).max(axis=1))
    d = np.abs(J - J_ref).max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(s > 0, d / s, 0.0)
    return np.where(np.isfinite(e), e, np.inf)


def input_scaled_error(J, J_ref, x):
    """[4, 6, n]: e_ij = |J_ij − J^ref_ij|·|x_j| / s'_i with s'_i = max_j max(|J_ij|, |J^ref_ij|)·|x_j| per state, x the six Float64 state columns of the
    REFERENCE.  A row with s'_i = 0 must be exactly zero in both: error 0 if it is, Inf if not.  A non-finite entry gives Inf."""
    J, J_ref = np.asarray(J, dtype=np.float64), np.asarray(J_ref, dtype=np.float64)
    w = np.abs(np.stack([np.asarray(c, dtype=np.float64) for c in x]))[None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.maximum((np.abs(J) * w).max(axis=1), (np.abs(J_ref) * w).max(axis=1))[:, None, :]
        e = np.where(s > 0, np.abs(J - J_ref) * w / s, np.where((J == 0) & (J_ref == 0), 0.0, np.inf))
    return np.where(np.isfinite(e), e, np.inf)


def worst_cells(J, J_ref, x, kept):
    """[4, 6]: the worst input-scaled error per (row, column) over the kept states."""
    return input_scaled_error(J, J_ref, x)[:, :, kept].max(axis=2)


def disagreement(J1, J4, x):
    """[n]: the larger of the two measures between two references, per state."""
    return np.maximum(scaled_error(J1, J4).max(axis=0), input_scaled_error(J1, J4, x).max(axis=(0, 1)))


def entry_shares(J_ref, x, kept):
    """[4, 6]: from the reference alone, the largest share an entry reaches at any kept state in either measure — |J^ref_ij|/s_i or |J^ref_ij x_j|/s'_i.
    An error of relative size r in entry (i, j) shows as r·share at that state, so BOUND/share is the relative error of that entry that the set resolves."""
    A = np.abs(np.asarray(J_ref, dtype=np.float64))[:, :, kept]
    B = A * np.abs(np.stack([np.asarray(c, dtype=np.float64) for c in x]))[None][:, :, kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = A / A.max(axis=1, keepdims=True), B / B.max(axis=1, keepdims=True)
    return np.fmax(np.nan_to_num(a).max(axis=2), np.nan_to_num(b).max(axis=2))


MIN_SHARE = 0.01


def assert_resolution(J_ref, x, kept, out, wrt, what):
    """Every structurally non-zero entry of the reference Jacobian (non-zero at any kept state of the set) reaches a share of at least MIN_SHARE of its row
    in one of the two measures at some kept state: an error of 0.1 % of that entry then misses the Float64 bound and one of 10 % the Float32 bound.  Prints
    the resolved relative error BOUND/share per entry and returns the shares."""
    share = entry_shares(J_ref, x, kept)
    nonzero = (np.asarray(J_ref)[:, :, kept] != 0).any(axis=2)
    print(f"{what}: relative error of an entry that misses the bound (f64 {BOUND['f64']:g} / f32 {BOUND['f32']:g} over its share), kept {int(kept.sum())}/{kept.size}")
    for i, row in enumerate(out):
        print(f"  {row}: " + ", ".join(f"{c} " + (f"{BOUND['f64'] / share[i, j]:.1e}/{BOUND['f32'] / share[i, j]:.1e} (share {share[i, j]:.2g})" if nonzero[i, j] else "zero")
                                       for j, c in enumerate(wrt)))
    low = [(out[i], wrt[j], float(share[i, j])) for i in range(len(out)) for j in range(len(wrt)) if nonzero[i, j] and not share[i, j] >= MIN_SHARE]
    assert not low, (what, low)
    return share, nonzero


def cells_line(cells, out, wrt):
    return "; ".join(f"{row}: " + " ".join(f"{c} {cells[i, j]:.2g}" for j, c in enumerate(wrt)) for i, row in enumerate(out))


def fd_reference(tendencies, cols):
    """(J_fd at h, kept, worst h-vs-4h disagreement in either measure) of the states `cols`: a state is kept if the references at h and 4h agree within AGREE."""
    J1, J4 = fd_jacobian(tendencies, cols), fd_jacobian(tendencies, cols, step=4e-6)
    disagree = disagreement(J1, J4, cols[1:])
    return J1, disagree <= AGREE, float(disagree.max())


def checked(ref, *what):
    """The first four members (cols, J_fd, kept, worst disagreement) of a cached reference, shared read-only; asserts the 1 % condition."""
    cols, J, kept, worst = ref[:4]
    assert (~kept).sum() <= MAX_SET_ASIDE * kept.size, (*what, int((~kept).sum()), kept.size, worst)
    return cols, J, kept, worst


@functools.lru_cache(maxsize=None)
def _reference(limited, perturbed, which):
    import oracle_binding as oracle
    oracle.lib()
    ov = perturbed_overrides() if perturbed else None
    wr64 = warm_rain_params("f64", limited, ov)
    cols = interior_states(oracle) if which == "interior" else points(WARM_RAIN, KAT)
    J1, kept, worst = fd_reference(lambda c: oracle_tendencies(oracle, wr64, limited, c), cols)
    E, eps_S = evaporation_share(oracle, wr64, limited, cols), evaporation_spread_f32(oracle, limited, perturbed, cols)
    for a in (*cols, J1, kept, E, eps_S):
        a.setflags(write=False)
    return cols, J1, kept, worst, E, eps_S


def reference(limited, perturbed=False, which="interior"):
    """(cols, J_fd, kept, worst h-vs-4h disagreement in either measure) of a set, computed once and shared read-only; asserts the 1 % condition."""
    return checked(_reference(bool(limited), bool(perturbed), which))


# the one (float type, parameter set, row) that cannot meet the plain Float32 bound and is held to `float32_bound` instead
ENTRY_BOUND_ROWS = {("f32", True): ("dn_rai_dt",)}


def assert_parity(ft, J, limited, perturbed, which, what, report=True):
    """The parity assertion of both test files, in BOTH measures.  Row measure: every row of every kept state inside BOUND[ft] — Float64 1e-5, Float32
    1e-3 — except dn_rai_dt in Float32 with the perturbed parameter set, every entry of which is inside `float32_bound`.  Input-scaled measure: every
    (row, column) of every kept state inside the same BOUND[ft], no exception.  Prints (report=True) and returns the worst scaled error per row, the largest
    fraction of the entry bound that was used and the worst input-scaled error per (row, column)."""
    cols, J_ref, kept, worst_fd, E, eps_S = ref = _reference(bool(limited), bool(perturbed), which)
    checked(ref)
    rows = worst_rows(J, J_ref, kept, OUT)
    cells = worst_cells(J, J_ref, cols[1:], kept)
    J = np.asarray(J, dtype=np.float64)
    by_entry = ENTRY_BOUND_ROWS.get((ft, bool(perturbed)), ())
    used = 0.0
    for name in by_entry:
        i = OUT.index(name)
        with np.errstate(invalid="ignore"):
            frac = (np.abs(J - J_ref) / float32_bound(J, J_ref, E, eps_S))[i]
        frac = np.where(np.isnan(frac), np.where(J[i] == J_ref[i], 0.0, np.inf), frac)[:, kept]
        used = max(used, float(frac.max()))
    if report:
        print(f"{what} {ft} limited={limited} perturbed={perturbed} {which}: kept {int(kept.sum())}/{kept.size}, h-vs-4h {worst_fd:.3g}, worst rows "
              + ", ".join(f"{k} {v:.3g}" for k, v in rows.items())
              + (f"; {', '.join(by_entry)} uses {used:.3g} of its entry bound (c = {evaporation_spread_constant(bool(limited), bool(perturbed)):.3g})" if by_entry else "")
              + f"\n  input-scaled, worst {cells.max():.3g} — " + cells_line(cells, OUT, WRT))
    for name, v in rows.items():
        if name not in by_entry:
            assert v < BOUND[ft], (what, which, name, v)
    assert used < 1.0, (what, which, used)
    for i, j in zip(*np.nonzero(~(cells < BOUND[ft]))):
        raise AssertionError((what, which, "input-scaled", OUT[i], WRT[j], float(cells[i, j])))
    return rows, used, cells


def worst_rows(J, J_ref, kept, out):
    """Worst scaled error per output row over the kept states: {row name: value}; out: the row names."""
    e = scaled_error(J, J_ref)[:, kept]
    return {name: float(e[i].max()) for i, name in enumerate(out)}
