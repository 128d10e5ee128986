"""Aerosol nucleation rates (src/Nucleation.jl) and the P3 ice-nucleation counts (CMI_het.P3_deposition_N_i / P3_het_N_i), CPU side:

  * the float64 restatement tests/nucleation_ref.py against the 24 known answers of test/nucleation_unit_tests.jl with the Python defaults, and its P3
    pair against the oracle;
  * the device point functions and their host folding (csrc/cmx_nucleation.hpp) compiled by g++ (tests/native/nucleation_host.cpp) against the
    restatement on random sweeps with zeros, negatives, NaN, ±Inf, subnormal intermediates and the 1^Inf case of the apparent rate;
  * the C layout of the three new parameter structs against their ctypes mirrors, the argument checks of the C ABI that need no GPU, and the warning
    of the unpinned defaults."""
import ctypes as C
import json
import subprocess
import warnings
from pathlib import Path

import numpy as np
import pytest

import nucleation_ref as R
from cmx import _abi, _lib
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
KATS = json.loads((REPO / "tests" / "golden" / "nucleation_kats.json").read_text())
P3_KATS = json.loads((REPO / "tests" / "golden" / "p3_kats.json").read_text())["het_ice_nucleation"]
NPT = {"f32": np.float32, "f64": np.float64}
CT = {"f32": C.c_float, "f64": C.c_double}
RTOL = {"f32": 1e-3, "f64": 1e-6}
FLOOR = {"f32": 1e-30, "f64": 1e-290}
CEIL = {"f32": 1e30, "f64": 1e300}
COLS = ("h2so4", "nh3", "negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink")
OUTS = ("binary", "ternary", "organic", "mixed")


def params(ft):
    """the three nucleation structs with the Python defaults (their unpinned-default warnings silenced here; test_unpinned_defaults_warn checks them)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", P.UnpinnedParameterWarning)
        return P.H2S04NucleationParameters(ft), P.OrganicNucleationParameters(ft), P.MixedNucleationParameters(ft)


from param_sweep import nucleation_state as random_states  # noqa: E402  (shared with the parameter sweep)


def special_states(seed=3, ft="f64"):
    """every input at 0, negative, NaN, ±Inf, subnormal-producing and ordinary values, in random combinations.  (The largest finite special is 1e20
    in Float32: an h2so4 of 1e30 m⁻³ overflows (h2so4/ref)^p_t in Float32 — in the reference's own Float32 arithmetic too — and 0·Inf is NaN there.)"""
    base = random_states(4000, seed)
    g = np.random.default_rng(seed + 1)
    specials = np.array([0.0, -0.0, -1e10, -1.0, np.nan, np.inf, -np.inf, 1e-40, 1e-300, 1e-20, 1.0, 1e30 if ft == "f64" else 1e20])
    for k in base:
        m = g.random(base[k].size) < 0.15
        base[k][m] = g.choice(specials, int(m.sum()))
    return base


def reference(s, hp, op, mp):
    b, t = R.h2so4_nucleation_rate(s["h2so4"], s["nh3"], s["negative_ion"], s["temp"], hp)
    o = R.organic_nucleation_rate(s["negative_ion"], s["monoterpene"], s["O3"], s["OH"], s["temp"], s["condensation_sink"], op)
    m = R.organic_and_h2so4_nucleation_rate(s["h2so4"], s["monoterpene"], s["OH"], s["temp"], s["condensation_sink"], mp)
    return {"binary": b, "ternary": t, "organic": o, "mixed": m}


def compare(got, ref, ft, what, rtol=None, overflow_nan_ok=False, floor=None):
    """NaN exactly where the reference is NaN; beyond the float type's range an infinity of the right sign (or the overflowing value); below floatmin
    anything of magnitude ≤ FLOOR; elsewhere the relative bound.  Returns the worst relative error.  overflow_nan_ok: where the float64 value lies
    beyond the float type's range, two overflowing terms of opposite sign may also give NaN (Inf − Inf, as in the reference's own arithmetic in
    that float type)."""
    rtol = RTOL[ft] if rtol is None else rtol
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    gn, rn = np.isnan(got), np.isnan(ref)
    if overflow_nan_ok:
        rn = rn | (gn & (np.abs(ref) > CEIL[ft]))
    assert (gn == rn).all(), (what, ft, np.flatnonzero(gn != rn)[:5], got[gn != rn][:5], ref[gn != rn][:5])
    ok = ~rn
    big = ok & (np.abs(ref) > CEIL[ft])
    assert ((np.sign(got[big]) == np.sign(ref[big])) & (np.abs(got[big]) > CEIL[ft] / 10)).all(), what
    k = ok & ~big
    err = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), FLOOR[ft] if floor is None else floor)
    worst = float(err.max()) if err.size else 0.0
    assert worst <= rtol, (what, ft, worst, got[k][np.argmax(err)], ref[k][np.argmax(err)])
    return worst


# ---- the restatement against the reference's known answers ---------------------------------------------------------------------------

def test_restatement_reproduces_the_h2so4_known_answers():
    k = KATS["h2so4_unit"]
    hp, _, _ = params("f64")
    for c, r in zip(k["h2so4_c"], k["rates"]):
        b, t = R.h2so4_nucleation_rate(c * 1e6, k["nh3"], k["negative_ion"], k["temp"], hp)
        assert float(t) == 0.0                                   # nh3 = 0: f_y = 0 exactly
        assert float(b + t) * 1e-6 == pytest.approx(r, rel=k["rtol"])


def test_restatement_reproduces_the_organic_known_answers():
    k = KATS["organic_unit"]
    _, op, _ = params("f64")
    for c, r in zip(k["hom_c"], k["rates"]):
        assert float(R.organic_nucleation_rate_hom_prescribed(k["negative_ion"], c, op)) * 1e-6 == pytest.approx(r, rel=k["rtol"])


def test_restatement_reproduces_the_mixed_known_answers():
    k = KATS["mixed_unit"]
    _, _, mp = params("f64")
    for c, r in zip(k["bioOxOrg"], k["rates"]):
        assert float(R.organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed(k["h2so4"], c, mp)) * 1e6 == pytest.approx(r, rel=k["rtol"])


def test_there_are_24_known_answers():
    assert len(KATS["h2so4_unit"]["rates"]) + len(KATS["organic_unit"]["rates"]) + len(KATS["mixed_unit"]["rates"]) == 24


def test_restatement_passes_the_reference_gpu_checks():
    hp, op, mp = params("f64")
    g = KATS["gpu_modal"]
    h = g["h2so4"]
    assert float(sum(R.h2so4_nucleation_rate(h["h2so4"], h["nh3"], h["negative_ion"], h["temp"], hp))) > 0
    o = g["organic"]
    assert float(R.organic_nucleation_rate(o["negative_ion"], o["monoterpene"], o["O3"], o["OH"], o["temp"], o["condensation_sink"], op)) > 0
    m = g["mixed"]
    assert float(R.organic_and_h2so4_nucleation_rate(m["h2so4"], m["monoterpene"], m["OH"], m["temp"], m["condensation_sink"], mp)) > 0
    a = g["apparent"]
    J = R.apparent_nucleation_rate(a["output_diam"], a["nucleation_rate"], a["condensation_growth_rate"], a["coag_sink"], a["coag_sink_input_diam"],
                                   a["input_diam"])
    assert float(J) == KATS["apparent_derived"]["J_x"]


def test_restatement_p3_pair_matches_the_known_answers_and_the_oracle(oracle):
    ip = P.MorrisonMilbrandt2014("f64")
    k = P3_KATS
    assert float(R.p3_deposition_N_i(ip, k["P3_deposition_N_i"]["T"])) == pytest.approx(k["P3_deposition_N_i"]["expected"], rel=1e-9)
    h = k["P3_het_N_i"]
    assert float(R.p3_het_N_i(ip, h["T"], h["N_l"], h["V_l"], h["dt"])) == pytest.approx(h["expected_f64"], rel=1e-9)
    # the reference's own Float32 arithmetic reproduces its quoted Float32 value (the cancellation the library avoids)
    assert float(R.p3_het_N_i_reference_form(ip, h["T"], h["N_l"], h["V_l"], h["dt"], np.float32)) == pytest.approx(h["expected_f32"], rel=1e-6)
    g = np.random.default_rng(5)
    T = np.concatenate([g.uniform(190, 320, 300), [ip.T_dep_thres, ip.T0, np.nextafter(ip.T0, 0), np.nextafter(ip.T0, 400)]])
    Nl, Vl, dt = 10 ** g.uniform(6, 9, T.size), 10 ** g.uniform(-18, -12, T.size), g.uniform(1, 300, T.size)
    for i in range(T.size):
        assert R.p3_deposition_N_i(ip, T[i]) == pytest.approx(oracle.P3_deposition_N_i(_abi.F64, ip, T[i]), rel=1e-13, abs=0)
        x = abs(float(ip.het_B) * Vl[i] * dt[i] * np.exp(float(ip.het_a) * (float(ip.T0) - T[i])))
        if x >= 1e-6:                                  # below that the oracle's own 1 − exp loses Float64 digits
            assert R.p3_het_N_i(ip, T[i], Nl[i], Vl[i], dt[i]) == pytest.approx(oracle.P3_het_N_i(_abi.F64, ip, T[i], Nl[i], Vl[i], dt[i]), rel=1e-9)
    assert oracle.P3_deposition_N_i(_abi.F64, ip, np.nan) == 0.0                    # the reference's ifelse; the library returns NaN
    assert np.isnan(R.p3_deposition_N_i(ip, np.nan)) and R.p3_deposition_N_i(ip, np.nan, nan_rule=False) == 0.0


# ---- the point functions and their host folding --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libnucleation_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(REPO / "tests" / "native" / "nucleation_host.cpp")], check=True)
    return C.CDLL(str(so))


def _pp(a, ft):
    return a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None


def host_rates(host, ft, s, want=OUTS):
    hp, op, mp = params(ft)
    x = {k: np.ascontiguousarray(s[k], dtype=NPT[ft]) for k in COLS}
    out = {k: (np.full(x["temp"].size, -7.0, dtype=NPT[ft]) if k in want else None) for k in OUTS}
    ins = (C.POINTER(CT[ft]) * 8)(*[_pp(x[k], ft) for k in COLS])
    outs = (C.POINTER(CT[ft]) * 4)(*[_pp(out[k], ft) for k in OUTS])
    getattr(host, f"nuc_rates_{ft}")(C.byref(hp), C.byref(op), C.byref(mp), C.c_int64(x["temp"].size), ins, outs)
    return x, out


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_functions_match_the_restatement(host, ft):
    x, got = host_rates(host, ft, random_states(200_000, 7))
    ref = reference({k: v.astype(np.float64) for k, v in x.items()}, *params("f64"))
    for k in OUTS:
        worst = compare(got[k], ref[k], ft, k)
        print(f"\n[nucleation host] {k} {ft}: worst relative error {worst:.3e}")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_functions_special_values(host, ft):
    """0, negatives, NaN, ±Inf, subnormal intermediates: the same NaN pattern as the restatement (IEEE pow, DomainError → NaN), the same values elsewhere.
    Float32 results whose float64 value lies below floatmin(Float32) only need to be tiny."""
    x, got = host_rates(host, ft, special_states(ft=ft))
    ref = reference({k: v.astype(np.float64) for k, v in x.items()}, *params("f64"))
    # Float32: an infinite input or one above 1e19 (h2so4² overflows), a temperature of 1e10 K or of 1 K, or an input below floatmin(Float32) makes an intermediate of the reference's own
    # Float32 arithmetic overflow or underflow (k_t_n = exp(u_t_n) and exp(444/T) are Inf, MT·1e-6 is 0, ±Inf ions multiply an underflowed 0):
    # those points are excluded in Float32 and counted; every other point must match, NaN pattern included
    keep = np.ones(x["temp"].size, bool)
    if ft == "f32":
        keep = (np.abs(x["temp"]) < 1e4) & (np.abs(x["temp"]) > 50)
        for v in x.values():
            keep &= (np.abs(v) < 1e19) & ~((v != 0) & (np.abs(v) < 1e-30))
        assert keep.mean() > 0.3, keep.mean()
    for k in OUTS:
        r = ref[k][keep]
        compare(got[k][keep], r, ft, k, overflow_nan_ok=True, floor=1e-26 if ft == "f32" else None)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_zero_bases_and_negative_concentrations(host, ft):
    z = np.zeros(4)
    s = {k: np.full(4, v) for k, v in (("h2so4", 1e12), ("nh3", 0.0), ("negative_ion", 0.0), ("monoterpene", 1e15), ("O3", 1e18), ("OH", 1e12),
                                       ("temp", 208.0), ("condensation_sink", 1e-3))}
    s["h2so4"] = np.array([1e12, 0.0, -1e12, 1e12])
    s["nh3"] = np.array([0.0, 0.0, 1e10, -1e10])
    s["negative_ion"] = z
    _, got = host_rates(host, ft, s)
    assert got["ternary"][0] == 0.0 and got["binary"][0] > 0                      # nh3 = 0: f_y = 0, ternary exactly 0
    assert np.isnan(got["ternary"][1]) and got["binary"][1] == 0.0                 # h2so4 = nh3 = 0: 0/0 in f_y (as the reference)
    assert np.isnan(got["binary"][2]) and np.isnan(got["ternary"][2])             # h2so4 < 0: DomainError → NaN
    assert np.isnan(got["binary"][3]) and np.isnan(got["ternary"][3])             # nh3 < 0: the reference throws for the whole call
    assert got["mixed"][2] > 0                                                      # h2so4² of a negative: the reference's value


def host_apparent(host, ft, cols, id_=None):
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    i = np.ascontiguousarray(id_, dtype=NPT[ft]) if id_ is not None else None
    J = np.empty_like(x[0])
    getattr(host, f"nuc_apparent_{ft}")(C.c_int64(J.size), *[_pp(a, ft) for a in x], _pp(i, ft), _pp(J, ft))
    return x, i, J


def apparent_states(n, seed):
    g = np.random.default_rng(seed)
    return (g.uniform(2, 20, n), 10 ** g.uniform(0, 8, n), 10 ** g.uniform(-2, 1, n), 10 ** g.uniform(-5, -2, n), 10 ** g.uniform(-4, -1, n)), \
        g.uniform(1, 2, n)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_apparent_rate_matches_the_restatement(host, ft):
    cols, id_ = apparent_states(100_000, 9)
    for with_id in (True, False):
        x, i, J = host_apparent(host, ft, cols, id_ if with_id else None)
        ref = R.apparent_nucleation_rate(*[a.astype(np.float64) for a in x], i.astype(np.float64) if with_id else 1.7)
        compare(J, ref, ft, "J_x")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_apparent_rate_ieee_pow_cases(host, ft):
    a = KATS["gpu_modal"]["apparent"]
    cols = [np.array([a[k]] * 3) for k in ("output_diam", "nucleation_rate", "condensation_growth_rate", "coag_sink", "coag_sink_input_diam")]
    cols[3][1] = 1e-12          # m = −Inf
    cols[3][2] = a["coag_sink_input_diam"]       # log(1)/log(1): NaN, as the reference
    _, _, J = host_apparent(host, ft, cols, np.array([a["input_diam"]] * 3))
    assert J[0] == KATS["apparent_derived"]["J_x"] and J[1] == KATS["apparent_derived"]["J_x"]   # 1^(±Inf) = 1: exactly nucleation_rate
    assert np.isnan(J[2])
    # special values everywhere: the restatement's NaN pattern
    g = np.random.default_rng(4)
    cols, id_ = apparent_states(5000, 11)
    cols = [c.copy() for c in cols] + [id_.copy()]
    for c in cols:
        m = g.random(c.size) < 0.1
        c[m] = g.choice(np.array([0.0, -1.0, np.nan, np.inf, 1.5]), int(m.sum()))
    x, i, J = host_apparent(host, ft, cols[:5], cols[5])
    compare(J, R.apparent_nucleation_rate(*[v.astype(np.float64) for v in x], i.astype(np.float64)), ft, "J_x special", overflow_nan_ok=True)


def host_prescribed(host, ft, ion, hom, h, bio):
    _, op, mp = params(ft)
    x = [np.ascontiguousarray(a, dtype=NPT[ft]) for a in (ion, hom, h, bio)]
    o, m = np.empty_like(x[0]), np.empty_like(x[0])
    getattr(host, f"nuc_prescribed_{ft}")(C.byref(op), C.byref(mp), C.c_int64(o.size), *[_pp(a, ft) for a in x], _pp(o, ft), _pp(m, ft))
    return x, o, m


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_prescribed_forms_reproduce_the_known_answers(host, ft):
    k = KATS["organic_unit"]
    hom = np.array(k["hom_c"])
    _, o, _ = host_prescribed(host, ft, np.zeros_like(hom), hom, np.zeros_like(hom), np.zeros_like(hom))
    np.testing.assert_allclose(o.astype(np.float64) * 1e-6, k["rates"], rtol=max(k["rtol"], 3 * RTOL[ft] if ft == "f32" else 0))
    k = KATS["mixed_unit"]
    bio = np.array(k["bioOxOrg"])
    _, _, m = host_prescribed(host, ft, bio, bio, np.full_like(bio, k["h2so4"]), bio)
    np.testing.assert_allclose(m.astype(np.float64) * 1e6, k["rates"], rtol=k["rtol"] if ft == "f64" else 1e-5)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_p3_counts_host(host, ft):
    ip = P.MorrisonMilbrandt2014(ft)
    g = np.random.default_rng(6)
    T = np.concatenate([g.uniform(190, 320, 50_000), [float(ip.T_dep_thres), float(ip.T0), np.nan, np.inf, -np.inf]])
    Nl, Vl, dt = 10 ** g.uniform(6, 9, T.size), 10 ** g.uniform(-18, -12, T.size), g.uniform(1, 300, T.size)
    x = [np.ascontiguousarray(a, dtype=NPT[ft]) for a in (T, Nl, Vl, dt)]
    Nd, Nh = np.empty_like(x[0]), np.empty_like(x[0])
    getattr(host, f"nuc_p3_{ft}")(C.byref(ip), C.c_int64(Nd.size), *[_pp(a, ft) for a in x], _pp(Nd, ft), _pp(Nh, ft))
    ip64 = ip                       # the restatement reads the struct's own (rounded) values: T = T₀ must compare equal in both
    xd = [a.astype(np.float64) for a in x]
    compare(Nd, R.p3_deposition_N_i(ip64, xd[0]), ft, "N_dep")
    compare(Nh, R.p3_het_N_i(ip64, *xd), ft, "N_het")
    assert np.isnan(Nd[-3])                                        # NaN T → NaN (the reference's ifelse would return 0)
    # the reference's GPU test state: the Float32 value is within 1e-3 of the Float64 one and closer to it than the reference's Float32 literal
    h = P3_KATS["P3_het_N_i"]
    y = [np.array([h[k]], dtype=NPT[ft]) for k in ("T", "N_l", "V_l", "dt")]
    o = np.empty(1, dtype=NPT[ft])
    getattr(host, f"nuc_p3_{ft}")(C.byref(ip), C.c_int64(1), *[_pp(a, ft) for a in y], None, _pp(o, ft))
    err = abs(float(o[0]) - h["expected_f64"]) / h["expected_f64"]
    assert err <= RTOL[ft] and abs(float(o[0]) - h["expected_f64"]) < abs(h["expected_f32"] - h["expected_f64"])


# ---- C layout, ABI argument checks, unpinned defaults ------------------------------------------------------------------------------------

def test_struct_layout_matches_c(tmp_path):
    probes = [(f"cmx_{nm}_{fam.sfx}", getattr(fam, nm)) for fam in (_abi.F32, _abi.F64)
              for nm in ("h2so4_nucleation", "organic_nucleation", "mixed_nucleation")]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{REPO}/include/cmx.h"', "int main(void){"]
    for cname, st in probes:
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            src.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(c)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, st in probes:
        assert int(out[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(st, fname).offset, f"{cname}.{fname}"
    # the header's own size contract for the three structs (CMX_ASSERT_NUCLEATION_STRUCT_SIZES) agrees with the mirrors
    import re
    rows = re.findall(r"CMX_STATIC_ASSERT\(\(sizeof\((cmx_\w+)_##SFX\) == (\d+) \* sizeof\(FT\)\)", (REPO / "include" / "cmx.h").read_text())
    assert sorted(n for n, _ in rows) == ["cmx_h2so4_nucleation", "cmx_mixed_nucleation", "cmx_organic_nucleation"]
    for name, nft in rows:
        for fam, w in ((_abi.F32, 4), (_abi.F64, 8)):
            assert C.sizeof(getattr(fam, name[len("cmx_"):])) == int(nft) * w
    assert [f for f, _ in _abi.F64.h2so4_nucleation._fields_][:2] == ["p_b_n", "p_b_i"] and len(_abi.F64.h2so4_nucleation._fields_) == 20
    assert len(_abi.F64.organic_nucleation._fields_) == 11 and len(_abi.F64.mixed_nucleation._fields_) == 3


def test_argument_checks_without_gpu():
    lib = _lib.lib()
    hp, op, mp = params("f32")
    f = lib.cmx_aerosol_nucleation_rates_f32
    col = C.c_void_p(4096)
    ins = [col] * 8
    nul = [None] * 4
    B, OK, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK, _abi.CMX_ERR_UNSUPPORTED
    assert f(C.byref(hp), C.byref(op), C.byref(mp), 10, *ins, *nul, None) == B                         # all outputs NULL
    assert f(C.byref(hp), C.byref(op), C.byref(mp), -1, *ins, col, col, col, col, None) == B           # n < 0
    assert f(C.byref(hp), C.byref(op), C.byref(mp), 16 * 0x7fffffff + 1, *ins, col, col, col, col, None) == UNS
    assert f(None, C.byref(op), C.byref(mp), 10, *ins, col, None, None, None, None) == B               # binary without its struct
    assert f(C.byref(hp), None, None, 10, *ins, None, None, col, None, None) == B                      # organic without its struct
    assert f(C.byref(hp), C.byref(op), None, 10, *ins, None, None, None, col, None) == B               # mixed without its struct
    assert f(C.byref(hp), None, None, 0, *[None] * 8, col, col, None, None, None) == OK                # n = 0
    # every column an output reads is required (only refused calls are made here: an accepted one would launch on the placeholder pointers)
    for k in (0, 1, 2, 6):                                                                             # binary + ternary
        x = list(ins)
        x[k] = None
        assert f(C.byref(hp), None, None, 10, *x, col, col, None, None, None) == B, k
    for k in (2, 3, 4, 5, 6, 7):                                                                       # organic
        x = list(ins)
        x[k] = None
        assert f(None, C.byref(op), None, 10, *x, None, None, col, None, None) == B, k
    for k in (0, 3, 5, 6, 7):                                                                          # mixed
        x = list(ins)
        x[k] = None
        assert f(None, None, C.byref(mp), 10, *x, None, None, None, col, None) == B, k
    g = lib.cmx_nucleation_rates_prescribed_f64
    _, op64, mp64 = params("f64")
    assert g(C.byref(op64), C.byref(mp64), 10, col, col, col, col, None, None, None) == B
    assert g(C.byref(op64), C.byref(mp64), -1, col, col, col, col, col, col, None) == B
    assert g(C.byref(op64), None, 10, col, None, col, col, col, None, None) == B                         # organic needs HOM
    assert g(None, C.byref(mp64), 10, None, None, None, col, None, col, None) == B                       # mixed needs h2so4
    assert g(C.byref(op64), C.byref(mp64), 0, None, None, None, None, col, col, None) == OK
    a = lib.cmx_apparent_nucleation_rate_f32
    assert a(10, col, col, col, col, col, col, None, None) == B                                         # no output
    assert a(-1, col, col, col, col, col, col, col, None) == B
    assert a(10, col, col, col, None, col, col, col, None) == B                                          # coag_sink missing
    assert a(0, None, None, None, None, None, None, col, None) == OK
    p = lib.cmx_p3_ice_nucleation_counts_f64
    ip = P.MorrisonMilbrandt2014("f64")
    assert p(None, 10, col, col, col, col, col, col, None) == B
    assert p(C.byref(ip), 10, col, col, col, col, None, None, None) == B                                  # both outputs NULL
    assert p(C.byref(ip), -1, col, col, col, col, col, col, None) == B
    assert p(C.byref(ip), 10, None, None, None, None, col, None, None) == B                               # T missing
    assert p(C.byref(ip), 10, col, None, col, col, None, col, None) == B                                  # N_het needs N_l
    assert p(C.byref(ip), 0, None, None, None, None, col, None, None) == OK


def test_unpinned_defaults_warn():
    for ctor in (P.H2S04NucleationParameters, P.OrganicNucleationParameters, P.MixedNucleationParameters):
        with pytest.warns(P.UnpinnedParameterWarning):
            st = ctor("f64")
        assert st.unpinned and all(n in P.UNPINNED_DEFAULTS for n in st.unpinned)
    # the values the known answers pin are not flagged
    assert not {"mam3_nucleation_p_b_n_neutral", "mam3_nucleation_a_1_neutral", "mam3_nucleation_a_2_neutral", "mam3_nucleation_a_5",
                "mam3_nucleation_k_H2SO4_mixed_organic_sulfuric_acid_factor"} & set(P.UNPINNED_DEFAULTS)
    # overriding every unpinned name silences the warning
    td = P.create_toml_dict("f64", override={n: P.DEFAULT_PARAMETERS[n] for n in P.UNPINNED_DEFAULTS if n.startswith("mam3_")})
    with warnings.catch_warnings():
        warnings.simplefilter("error", P.UnpinnedParameterWarning)
        assert P.MixedNucleationParameters(td).unpinned == ()


def test_python_api_refuses_cpu_tensors():
    import torch
    import cmx
    t = torch.ones(4, dtype=torch.float64)
    hp, _, _ = params("f64")
    with pytest.raises(ValueError):
        cmx.h2so4_nucleation_rate(t, t, t, t, hp)
    with pytest.raises(ValueError):
        cmx.apparent_nucleation_rate(t, t, t, t, t)
