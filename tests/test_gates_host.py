"""The gates at and around their thresholds (tests/gate_cases.py), CPU side:

  * the conditions the catalogue sets for itself, on the reference alone: open side far from zero and closed side exactly zero, the side at the exact
    threshold, the caps on the share of a computed-gate ladder inside its margin, both Float32 references for T_freeze, the oracle's ϵ;
  * the checker can fail: the reference, recomputed with a moved threshold (raw gates: one rung, which at the exact value is `<` for `≤`; computed gates:
    twice the margin) or with one in-margin value replaced (NaN, the mean of the two branches), is rejected;
  * the host build of the device point functions (tests/native/point_host.cpp: the SB2006 fused outputs, the 1-moment tendencies and sources;
    precip_susceptibility_host.cpp) through the same ladders.  The per-process SB2006 columns and cmx_bulk_2m_cloud_to_rain have no host entry: they
    are checked on the device only (tests/test_gates_gpu.py)."""
import ctypes as C
import dataclasses
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gate_cases as G
import parity
from cmx import _abi
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
CT = {"f32": C.c_float, "f64": C.c_double}
FTS = ["f32", "f64"]


def _all_cases(oracle, ft):
    return [(c, None) for c in G.raw_cases(ft)] + list(G.computed_cases(oracle, ft))


# ---- the catalogue, on the reference alone --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", FTS)
def test_oracle_epsilon_is_the_float_of_the_float_type(oracle, ft):
    """ϵ = cbrt(floatmin(FT)) correctly rounded (Float32: 2⁻⁴² exactly; Float64: the double whose cube is nearest 2⁻¹⁰²²) and eps(FT)"""
    th = oracle.thresholds(_abi.F64, ft == "f32")
    assert th.eps_1m == G.EPS_1M[ft] and th.eps_m == th.eps_n == th.eps_ft == G.EPS[ft]
    assert G.EPS_1M["f32"] == 2.0 ** -42
    from fractions import Fraction
    x, c = G.EPS_1M["f64"], Fraction(1, 2 ** 1022)
    err = lambda v: abs(Fraction(v) ** 3 - c)  # noqa: E731
    assert err(x) < err(np.nextafter(x, 1.0)) and err(x) < err(np.nextafter(x, 0.0))


@pytest.mark.parametrize("ft", FTS)
def test_raw_catalogue_conditions(oracle, ft):
    """every raw ladder, on the reference: it passes its own checker; the watched columns are exactly 0 on the closed side and above parity.FLOOR on
    the open side; the side at the exact threshold is the catalogue's"""
    rows = []
    for case in G.raw_cases(ft):
        ref = G.reference(oracle, case)
        v = case.values()
        assert v.size == 17 and v[case.half] == G.NPT[ft](case.center), case.name
        assert all(v[i + 1] == np.nextafter(v[i], G.NPT[ft](np.inf)) for i in range(v.size - 1)), case.name      # consecutive values of FT
        side = G.check(case, ref["out"], ref)
        if case.watch:
            lo, hi = G.open_magnitude(case, ref)
            assert hi == 0.0 and lo > 1e3 * parity.FLOOR[ft], (case.name, lo, hi)
            assert side == ("open" if case.open_at_exact else "closed"), (case.name, side)
            rows.append(f"{case.name}: {case.predicate}: {side} at the threshold, open side >= {lo:.2e}")
    print(f"\n[gates, raw catalogue on the reference] {ft}:\n  " + "\n  ".join(rows))


def test_both_float32_references_for_t_freeze(oracle):
    """T = float32(273.15) and its two neighbours.  The oracle with the double 273.15 as T_freeze calls the exact value cold; with T_freeze set to the
    float the Float32 kernel holds it gives cold / warm / warm, the Float32 reference's answer."""
    case = next(c for c in G.raw_cases("f32") if c.name == "mp1m.T.is_warm.default")
    assert case.center == 273.149993896484375
    i = slice(case.half - 1, case.half + 2)
    warm = lambda ref: list(ref["out"]["S_accr_lcl_sno_warm"][i] != 0)  # noqa: E731
    cold = lambda ref: list(ref["out"]["S_accr_lcl_sno_cold"][i] != 0)  # noqa: E731
    plain = G.reference(oracle, case, round_t_freeze=False)
    assert warm(plain) == [False, False, True] and cold(plain) == [True, True, False]
    rounded = G.reference(oracle, case)
    assert warm(rounded) == [False, True, True] and cold(rounded) == [True, False, False]
    for pair in ("rai_sno", "lcl_sno"):                  # the warm / cold accretion pairs flip together
        w, c = rounded["out"][f"S_accr_{pair}_warm"][i], rounded["out"][f"S_accr_{pair}_cold"][i]
        assert list(w != 0) == [False, True, True] and list(c != 0) == [True, False, False], pair
    assert list(rounded["out"]["S_accr_melt_lcl_sno"][i] != 0) == [False, False, True]        # ∝ T − T_freeze: 0 at the exact value
    # the deposition limit (T > T_freeze) and the ice autoconversion (T < T_freeze) at the same three values
    dep = G.reference(oracle, next(c for c in G.raw_cases("f32") if c.name == "mp1m.T.deposition_limit.default"))
    assert list(dep["out"]["S_phase_change_vap_icl"][i] > 0) == [True, True, False]
    acnv = G.reference(oracle, next(c for c in G.raw_cases("f32") if c.name == "mp1m.T.ice_acnv.supersat"))
    assert list(acnv["out"]["S_acnv_icl_sno"][i] != 0) == [True, False, False]


@pytest.mark.parametrize("ft", FTS)
def test_computed_ladders_meet_their_caps(oracle, ft):
    """on the reference alone: ≤ 25 % of a ladder inside its margin, ≥ 64 rungs outside on each side, Float32 ladders of consecutive floats, the Float64
    stride the smallest power of two that meets the cap; the two ends of the ladder on the two branches"""
    rows = []
    for case, thr in G.computed_cases(oracle, ft):
        ref = G.reference(oracle, case, threshold=thr)
        m0, m1, t = G._segments(case, ref)
        frac = float(np.mean(ref["near"]))
        assert case.n == 4097 and frac <= G.MAX_INSIDE and m0 >= G.MIN_OUTSIDE and case.n - 1 - m1 >= G.MIN_OUTSIDE, (case.name, frac, m0, m1)
        assert abs(t - case.half) <= 1, (case.name, t)                      # the bisected threshold, rounded to FT, is the centre
        if ft == "f32":
            assert case.stride == 1
        elif case.stride > 1:
            assert G.inside_fraction(oracle, dataclasses.replace(case, stride=case.stride // 2), thr) > G.MAX_INSIDE, case.name
        assert G.check(case, ref["out"], ref) is None
        ind = ref["out"].get(G.INDICATOR[case.gate])
        if case.gate == "breakup" and ind is not None:
            rsc = ref["out"]["rain_self_collection"]
            assert np.all(ind[:t] == 0) and np.all(ind[t:] > 0.4 * np.abs(rsc[t:])), case.name       # 0 → 0.45·|rain_self_collection|
        if case.gate == "clip":
            assert np.all(ind[:t] == -2) and np.all(ind[t:] == 0), case.name
        if case.gate == "evap_number":
            # the gate is invisible: its open side is below FLOOR (Float32 gate) or −0 (Float64 gate) — see tests/gate_cases.py
            assert np.all(np.signbit(ind[:t])) and not np.any(np.signbit(ind[t:])) and np.max(np.abs(ind)) < parity.FLOOR[ft], case.name
        rows.append(f"{case.name}: threshold {case.var} = {thr!r}, stride {case.stride} ulp, {frac:.3f} inside the margin (rungs {m0 - case.half:+d} … {m1 - case.half:+d})")
    print(f"\n[gates, computed ladders on the reference] {ft}:\n  " + "\n  ".join(rows))


def test_breakup_thresholds_are_where_the_oracle_puts_them(oracle):
    thr = {c.name: t for c, t in G.computed_cases(oracle, "f64")}
    assert thr["sb2006.limited.process.breakup"] == pytest.approx(8.648027e-5, rel=1e-6)
    assert thr["sb2006.notlimited.process.breakup"] == pytest.approx(2.244930e-4, rel=1e-6)


# ---- the checker can fail -------------------------------------------------------------------------------------------------------------------

def _rejected(case, got, ref):
    try:
        G.check(case, got, ref)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("ft", FTS)
def test_checker_rejects_a_raw_threshold_moved_by_one_rung(oracle, ft):
    """the reference recomputed one rung up and one rung down, for every raw gate: one of the two flips the exact value (`<` for `≤`, `>` for `≥`),
    the other its neighbour"""
    run = G.oracle_run(oracle)
    for case in G.raw_cases(ft):
        ref = G.reference(oracle, case)
        for shift in (+1, -1):
            assert _rejected(case, run(case, case.columns(shift)), ref), (case.name, shift)
        flipped = run(case, case.columns(-1 if case.open_at_exact == case.open_above else +1))       # closes (opens) the exact value only
        if case.watch:
            assert G.exact_side(case, flipped) == ("closed" if case.open_at_exact else "open"), case.name


@pytest.mark.parametrize("ft", FTS)
def test_checker_rejects_computed_gate_mutations(oracle, ft):
    for case, thr in G.computed_cases(oracle, ft):
        ref = G.reference(oracle, case, threshold=thr)
        m0, m1, t = G._segments(case, ref)
        good = {k: v.copy() for k, v in ref["out"].items()}
        col = "dn_rai_dt" if case.family == "sb_fused" else G.INDICATOR[case.gate]
        for i in (m0, t - 1, t, m1):                                        # one in-margin value replaced by NaN
            bad = {k: v.copy() for k, v in good.items()}
            bad[col][i] = np.nan
            assert _rejected(case, bad, ref), (case.name, "nan", i)
        if case.gate == "evap_number":
            continue      # invisible gate (both sides are zero for the float type): there is no output a moved threshold or a mean could change
        width = m1 - m0 + 1                                                 # the margin is ± its half-width: twice the margin = its full width in rungs
        run = G.oracle_run(oracle, threshold=thr)
        for shift in (+width, -width):
            assert _rejected(case, run(case, case.columns(shift)), ref), (case.name, "moved by twice the margin", shift)
        for i in (m0, t - 1, t, m1):                                        # one in-margin value replaced by the mean of the two branch values
            bad = {k: v.copy() for k, v in good.items()}
            bad[col][i] = 0.5 * (good[col][t - 1] + good[col][t])
            assert _rejected(case, bad, ref), (case.name, "mean", i)


# ---- the host build of the point functions --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_libs():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    libs = {}
    for name, src in (("gates_point", "point_host.cpp"), ("gates_susc", "precip_susceptibility_host.cpp")):
        so = out / f"lib{name}_host.so"
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(REPO / "tests" / "native" / src)], check=True)
        libs[name] = C.CDLL(str(so))
    return libs


def _ptrs(arrs, ft):
    return (C.POINTER(CT[ft]) * len(arrs))(*[a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None for a in arrs])


def host_run(libs):
    """the `run` callable of the host build; families without a host entry → None"""
    def run(case, cols):
        ft = case.ft
        x = [np.ascontiguousarray(cols[k], dtype=G.NPT[ft]) for k in G.COLUMNS[case.family]]
        n = x[0].size
        new = lambda m: [np.full(n, -7.0, dtype=G.NPT[ft]) for _ in range(m)]  # noqa: E731
        if case.family == "sb_fused":
            wr, tps, vel = P.WarmRainParams2M(ft, case.limited), P.ThermodynamicsParameters(ft), P.rain_vel_params(ft)
            flags = (_abi.CMX_SB2006_LIMITED if case.limited else 0) | _abi.CMX_VEL_SB2006
            y = new(6)
            fn = getattr(libs["gates_point"], f"host_sb2006_{ft}")
            fn.restype = C.c_int32
            fn(C.byref(wr.c), C.byref(tps), C.byref(vel), C.c_uint32(flags), C.c_int(0), C.c_int64(n), _ptrs(x, ft), _ptrs(y, ft))
            return dict(zip(parity.OUT_NAMES, y))
        if case.family == "mp1m":
            mp, tps = P.Microphysics1MParams(ft, **G.MP1M_OPTIONS[case.optset]), P.ThermodynamicsParameters(ft)
            tend, src = new(4), new(_abi.CMX_MP1M_NSRC)
            for name, y in (("host_mp1m_tendencies", tend), ("host_mp1m_sources", src)):
                fn = getattr(libs["gates_point"], f"{name}_{ft}")
                fn.restype = C.c_int32
                fn(C.byref(mp.c), C.byref(tps), C.c_uint32(mp.flags), C.c_int64(n), _ptrs(x, ft), _ptrs(y, ft))
            return {**dict(zip(G.TENDENCIES_1M, tend)), **dict(zip(_abi.MP1M_SOURCE_COLUMNS, src))}
        if case.family == "susc":
            sb = P.SB2006(ft)
            y = new(6)
            pp = lambda a: a.ctypes.data_as(C.POINTER(CT[ft]))  # noqa: E731
            getattr(libs["gates_susc"], f"precip_susceptibility_{ft}")(C.byref(sb.acnv), C.byref(sb.accr), C.c_int64(n), *[pp(a) for a in x], _ptrs(y, ft))
            return dict(zip(G.SUSC_OUTS, y))
        return None
    return run


@pytest.mark.parametrize("ft", FTS)
def test_host_build_takes_the_reference_side_at_every_gate(oracle, host_libs, ft):
    run = host_run(host_libs)
    rows, ran = [], 0
    for case, thr in _all_cases(oracle, ft):
        got = run(case, case.columns())
        if got is None:
            continue
        ran += 1
        ref = G.reference(oracle, case, threshold=thr)
        res = G.check(case, got, ref)
        if case.computed:
            rows.append(f"{case.name}: side differs from the reference's at rungs {res}")
        elif case.watch:
            assert res == ("open" if case.open_at_exact else "closed"), (case.name, res)
            rows.append(f"{case.name}: {res} at the threshold")
    assert ran == 19              # 8 fused SB2006 + 8 one-moment raw ladders, 2 fused breakup ladders, the clip
    print(f"\n[gates, host build] {ft}:\n  " + "\n  ".join(rows))
