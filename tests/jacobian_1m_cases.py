"""States, reference and error measure shared by tests/test_mp1m_jacobian_host.py and tests/test_mp1m_jacobian_gpu.py.

The reference Jacobian is the method of tests/jacobian_cases.py (the reference's own, test/ad_compat_tests.jl:143-165): central differences of the Float64
ORACLE tendencies (oracle_binding.mp1m, _abi.F64, want_sources=False) with step h = 1e-6·|x_j|, the quotient formed with the realised x⁺ − x⁻, compared row
by row in the scale s_i = max_j max(|J_ij|, |J^fd_ij|).  A state is KEPT only if the references at h and at 4h agree within 2e-6 in that measure: a state
that sits on a kink of the tendency function (the saturation limiters, a min / max changing sides inside the stencil) has no derivative to compare with.  At
most 1 % of a set may be set aside (asserted where the set is built).

Sets: "cold" (T ∈ (235, 272.65)) and "warm" (T ∈ (273.65, 300)), 4096 states each with all four species present and T at least 0.5 K away from T_freeze,
and "points", the two single states the repository pins for the 1-moment scheme.  Parameter cases: "default" (the compile-time instantiation), "alt" (the
four alternative options: the run-time-flags instantiation) and "exponents" (default options, five size-relation parameters overridden: the run-time-flags
instantiation with general exponents).

Bounds: Float64 1e-5, the reference's own Jacobian bound (ad_compat_tests.jl:163); Float32 against the SAME Float64 reference at the project's Float32 bound
1e-3, every row.

Both bounds are asserted in two measures (tests/jacobian_cases.py, "THE SECOND MEASURE"): the per-row one above and the input-scaled one,
e_ij = |J_ij − J^ref_ij|·|x_j| / s'_i with s'_i = max_j max(|J_ij|, |J^ref_ij|)·|x_j| and x the reference's Float64 state columns, every (row, column), no
exception.  The per-row scale is set by the q columns: the largest share of a T entry at any kept state is 2.3e-3, so the whole T column scaled by 1.1 shows
as 7e-5 … 2.3e-4 there and passes Float32 — a T-derivative wrong by 40 % would; in the input-scaled measure it shows as 0.091.  A state is kept only if h and
4h agree within 2e-6 in both measures; the cap of 1 % applies to the union (set aside of 4096: default 3 cold / 2 warm, alt 5 / 2, exponents 3 / 2).  That both
measures can fail is tested in tests/test_mp1m_jacobian_host.py: every input column scaled by 1.1, zeroed or negated is rejected on every (case, set), and
every one of the 24 entries reaches 1 % of its row in one of the measures on the cold and on the warm set (smallest share 0.03: dq_sno_dt × (q_tot, q_lcl),
warm; 0.21 … 0.26 for dq_sno_dt × q_lcl and dq_rai_dt × q_tot, cold; every other ≥ 0.47).

Worst input-scaled value per row over the three cases and three sets (column, case and set of the worst in brackets), host build | device (MI355X):
  Float64   dq_lcl_dt 2.9e-10 | 2.9e-10 (q_lcl, alt cold)   dq_icl_dt 9.7e-8 | 9.7e-8 (T, alt cold)   dq_rai_dt 1.5e-9 | 1.5e-9 (T, default warm)   dq_sno_dt 7.9e-10 | 7.9e-10 (q_rai, default cold)
  Float32   dq_lcl_dt 2.2e-6 | 2.6e-6 (T, default cold)   dq_icl_dt 5.0e-4 | 4.9e-4 (T, alt cold)   dq_rai_dt 6.0e-5 | 4.6e-5 (T, alt | default warm)   dq_sno_dt 6.6e-6 | 6.0e-6 (q_rai, alt cold)
dq_icl_dt × T with the alternative options on the cold set is the one entry within a factor 2 of the Float32 bound, in the host build and on the device alike
— 13 of 4091 kept states lie above 6e-5, all at T = 252.4 … 255.1 K, where ∂dq_icl_dt/∂T changes sign with these options and the entry is the small
difference of terms of opposite sign (relative error of the entry itself 7e-3 at the worst state).  It meets the plain 1e-3 and is held to it like every
other entry.  No entry has a bound of its own.
"""
import functools

import numpy as np

from cmx import _abi
from cmx import parameters as P
from jacobian_cases import (AGREE, BOUND, MAX_SET_ASIDE, assert_resolution, cells_line, checked, fd_reference, points, worst_cells,  # noqa: F401
                            worst_rows)

WRT = _abi.MP1M_JAC_WRT            # T, q_tot, q_lcl, q_icl, q_rai, q_sno = columns 1 … 6 of the state
OUT = _abi.MP1M_JAC_OUT
N_STATES = 4096
T_RANGE = {"cold": (235.0, 272.65), "warm": (273.65, 300.0)}

# order rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno: the state of the plain-C caller (tests/test_abi_caller.py:152) and the reference suite's warm
# all-species state (test/bulk_tendencies_tests.jl:919-977, tests/test_mp1m_linearized.py:52-56)
CALLER = (1.2, 268.0, 6e-3, 5e-4, 5e-4, 5e-4, 5e-4)
SUITE_WARM = (1.2, 273.15 + 5.0, 0.012, 5e-4, 2e-4, 3e-4, 3e-4)

ALT_OPTIONS = dict(cloud_ice_formation=P.TemperatureDependent(), rain_autoconversion=P.PrescribedNd(), snow_autoconversion=P.WithSupersaturation(),
                   snow_deposition_sublimation=P.SublimationOnly())
EXPONENT_OVERRIDES = {"rain_terminal_velocity_size_relation_coefficient_ve": 0.47, "snow_terminal_velocity_size_relation_coefficient": 0.27,
                      "rain_terminal_velocity_size_relation_coefficient_delv": 0.1, "snow_mass_size_relation_coefficient_delm": 0.05,
                      "snow_flake_size_distribution_coefficient_nu": 0.6}
CASES = ("default", "alt", "exponents")
SETS = ("cold", "warm", "points")


def params(ft, case):
    """Microphysics1MParams of a parameter case."""
    opts = ALT_OPTIONS if case == "alt" else {}
    return P.Microphysics1MParams(P.create_toml_dict(ft, EXPONENT_OVERRIDES) if case == "exponents" else ft, **opts)


def q_sat_liquid(oracle, T, rho):
    tps = P.ThermodynamicsParameters("f64")
    p = np.array([oracle.psat_liquid(_abi.F64, tps, float(t)) for t in T])
    return p / (rho * tps.R_v * T)


def states(oracle, which, n=N_STATES, seed=11):
    """All four species present, T at least 0.5 K from T_freeze (the issue's recipe, drawn in this order)."""
    lo, hi = T_RANGE[which]
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.4, 1.2, n)
    T = rng.uniform(lo, hi, n)
    q_lcl, q_icl = 10.0 ** rng.uniform(-6.0, -3.0, n), 10.0 ** rng.uniform(-6.0, -3.0, n)
    q_rai, q_sno = 10.0 ** rng.uniform(-6.0, -2.7, n), 10.0 ** rng.uniform(-6.0, -2.7, n)
    q_tot = (q_lcl + q_icl + q_rai + q_sno) + q_sat_liquid(oracle, T, rho) * rng.uniform(0.5, 1.05, n)
    return [rho, T, q_tot, q_lcl, q_icl, q_rai, q_sno]


def oracle_tendencies(oracle, mp64, cols):
    r = oracle.mp1m(_abi.F64, mp64.c, P.ThermodynamicsParameters("f64"), mp64.flags, *[np.ascontiguousarray(c, dtype=np.float64) for c in cols],
                    nthreads=8, want_sources=False)
    return np.stack([r[k] for k in OUT])


@functools.lru_cache(maxsize=None)
def _reference(case, which):
    import oracle_binding as oracle
    oracle.lib()
    mp64 = params("f64", case)
    cols = points(CALLER, SUITE_WARM) if which == "points" else states(oracle, which)
    J1, kept, worst = fd_reference(lambda c: oracle_tendencies(oracle, mp64, c), cols)
    for a in (*cols, J1, kept):
        a.setflags(write=False)
    return cols, J1, kept, worst


def reference(case, which):
    """(cols, J_fd, kept, worst h-vs-4h disagreement) of a set, computed once and shared read-only; asserts the 1 % condition."""
    return checked(_reference(case, which), case, which)


def assert_parity(ft, J, case, which, what, report=True):
    """The parity assertion of both test files, in BOTH measures: every row of every kept state inside BOUND[ft] in the per-row measure, and every
    (row, column) of every kept state inside the same BOUND[ft] in the input-scaled one.  Prints (report=True) and returns the worst scaled error per row
    and the worst input-scaled error per (row, column)."""
    cols, J_ref, kept, worst_fd = reference(case, which)
    assert np.isfinite(np.asarray(J)[:, :, kept]).all(), (what, case, which)          # (a NaN would leave the row scale undefined, not large)
    rows = worst_rows(J, J_ref, kept, OUT)
    cells = worst_cells(J, J_ref, cols[1:], kept)
    if report:
        print(f"{what} {ft} {case} {which}: kept {int(kept.sum())}/{kept.size}, h-vs-4h {worst_fd:.3g}, worst rows " + ", ".join(f"{k} {v:.3g}" for k, v in rows.items())
              + f"\n  input-scaled, worst {cells.max():.3g} — " + cells_line(cells, OUT, WRT))
    for name, v in rows.items():
        assert v < BOUND[ft], (what, case, which, name, v)
    for i, j in zip(*np.nonzero(~(cells < BOUND[ft]))):
        raise AssertionError((what, case, which, "input-scaled", OUT[i], WRT[j], float(cells[i, j])))
    return rows, cells
