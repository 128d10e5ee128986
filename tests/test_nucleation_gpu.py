"""Aerosol nucleation rates (src/Nucleation.jl) and the P3 ice-nucleation counts on the device (-m gpu), through the C ABI and cmx.nucleation /
cmx.P3_deposition_N_i / cmx.P3_het_N_i.  The float64 yardstick is the NumPy restatement tests/nucleation_ref.py (pinned by the reference's known answers
in tests/test_nucleation_host.py); the reference's own GPU testsets ("Modal nucleation kernels", the P3 INP kernels, test/gpu_tests.jl:1001-1037,
1094-1153) run as written."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import nucleation_ref as R
import parity
from cmx import _abi
from cmx import parameters as P
from test_nucleation_host import OUTS, apparent_states, params, random_states

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
KATS = json.loads((REPO / "tests" / "golden" / "nucleation_kats.json").read_text())
P3_KATS = json.loads((REPO / "tests" / "golden" / "p3_kats.json").read_text())["het_ice_nucleation"]
DT = {"f32": torch.float32, "f64": torch.float64}
FAMILY = "aerosol nucleation (row g)"
PINNED = "tests/nucleation_ref.py (pinned by test/nucleation_unit_tests.jl KATs)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x, ft, dev):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=DT[ft], device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _fused(ft, cols, want=OUTS):
    import cmx
    hp, op, mp = params(ft)
    return cmx.nucleation_rates(hp, op, mp, h2so4=cols["h2so4"], nh3=cols["nh3"], negative_ion=cols["negative_ion"], monoterpene=cols["monoterpene"],
                                O3=cols["O3"], OH=cols["OH"], temp=cols["temp"], condensation_sink=cols["condensation_sink"], want=want)


def _np(t):
    return None if t is None else t.cpu().numpy().astype(np.float64)


# ---- the reference's known answers and GPU testsets ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_known_answers_through_the_abi(dev, ft):
    import cmx
    hp, op, mp = params(ft)
    tol = {"f32": 1e-3, "f64": 1e-5}[ft]             # the KATs' own rtol 1e-5; Float32 at the parity bound
    k = KATS["h2so4_unit"]
    n = len(k["rates"])
    b, t = cmx.h2so4_nucleation_rate(_t(np.array(k["h2so4_c"]) * 1e6, ft, dev), _t([k["nh3"]] * n, ft, dev), _t([k["negative_ion"]] * n, ft, dev),
                                     _t([k["temp"]] * n, ft, dev), hp)
    assert bool((t == 0).all())                                             # nh3 = 0: the ternary rate is exactly 0
    np.testing.assert_allclose((_np(b) + _np(t)) * 1e-6, k["rates"], rtol=tol)
    k = KATS["organic_unit"]
    n = len(k["rates"])
    o = cmx.organic_nucleation_rate_hom_prescribed(_t([k["negative_ion"]] * n, ft, dev), _t(k["hom_c"], ft, dev), op)
    np.testing.assert_allclose(_np(o) * 1e-6, k["rates"], rtol=tol)
    k = KATS["mixed_unit"]
    n = len(k["rates"])
    m = cmx.organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed(_t([k["h2so4"]] * n, ft, dev), _t(k["bioOxOrg"], ft, dev), mp)
    np.testing.assert_allclose(_np(m) * 1e6, k["rates"], rtol=tol)
    parity.record(f"nucleation KATs {ft}", ft, {"mixed": _np(m) * 1e6}, {"mixed": np.array(k["rates"])}, family=FAMILY,
                  pinned_by="test/nucleation_unit_tests.jl:71-97")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_reference_modal_nucleation_testset(dev, ft):
    """test/gpu_tests.jl:1094-1153 as written (ndrange 5), plus the derived J_x = 1e6 of the apparent-rate case and ternary = 0 at nh3 = 0"""
    import cmx
    hp, op, mp = params(ft)
    g = KATS["gpu_modal"]
    c = lambda v: torch.full((5,), v, dtype=DT[ft], device=dev)  # noqa: E731
    h = g["h2so4"]
    b, t = cmx.h2so4_nucleation_rate(c(h["h2so4"]), c(h["nh3"]), c(h["negative_ion"]), c(h["temp"]), hp)
    assert bool(((b + t) > 0).all())
    _, t0 = cmx.h2so4_nucleation_rate(c(h["h2so4"]), c(0.0), c(h["negative_ion"]), c(h["temp"]), hp)
    assert bool((t0 == 0).all())
    o = g["organic"]
    org = cmx.organic_nucleation_rate(c(o["negative_ion"]), c(o["monoterpene"]), c(o["O3"]), c(o["OH"]), c(o["temp"]), c(o["condensation_sink"]), op)
    assert bool((org > 0).all())
    m = g["mixed"]
    mix = cmx.organic_and_h2so4_nucleation_rate(c(m["h2so4"]), c(m["monoterpene"]), c(m["OH"]), c(m["temp"]), c(m["condensation_sink"]), mp)
    assert bool((mix > 0).all())
    a = g["apparent"]
    J = cmx.apparent_nucleation_rate(c(a["output_diam"]), c(a["nucleation_rate"]), c(a["condensation_growth_rate"]), c(a["coag_sink"]),
                                     c(a["coag_sink_input_diam"]), c(a["input_diam"]))
    assert bool((J == KATS["apparent_derived"]["J_x"]).all()), J          # 1^Inf = 1: exactly, in both precisions


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_reference_p3_inp_testsets(dev, ft):
    """test/gpu_tests.jl:1001-1037 against tests/golden/p3_kats.json; N_het under the expm1 rule (include/cmx.h): the Float32 value within 1e-3 of
    the Float64 one and strictly closer to it than the reference's Float32 literal, compared with the oracle's FLOAT64 output"""
    import cmx
    import oracle_binding as ob
    ip = P.MorrisonMilbrandt2014(ft)
    k = P3_KATS
    c = lambda v: torch.full((1,), v, dtype=DT[ft], device=dev)  # noqa: E731
    Nd = float(cmx.P3_deposition_N_i(ip, c(k["P3_deposition_N_i"]["T"]))[0])
    assert Nd == pytest.approx(k["P3_deposition_N_i"]["expected"], rel=parity.RTOL[ft])
    h = k["P3_het_N_i"]
    Nh = float(cmx.P3_het_N_i(ip, c(h["T"]), c(h["N_l"]), c(h["V_l"]), c(h["dt"]))[0])
    ip64 = P.MorrisonMilbrandt2014("f64")
    ref64 = ob.P3_het_N_i(_abi.F64, ip64, h["T"], h["N_l"], h["V_l"], h["dt"])
    assert ref64 == pytest.approx(h["expected_f64"], rel=1e-9)
    assert abs(Nh - ref64) <= parity.RTOL[ft] * ref64
    assert abs(Nh - ref64) < abs(h["expected_f32"] - ref64)


# ---- parity on random states ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_fused_rates_parity(dev, ft):
    n = 1_000_003
    s = random_states(n, 17)
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    got = _fused(ft, cols)
    x = {k: _np(v) for k, v in cols.items()}
    ref = R.h2so4_nucleation_rate(x["h2so4"], x["nh3"], x["negative_ion"], x["temp"], params("f64")[0])
    refs = {"binary": ref[0], "ternary": ref[1],
            "organic": R.organic_nucleation_rate(x["negative_ion"], x["monoterpene"], x["O3"], x["OH"], x["temp"], x["condensation_sink"], params("f64")[1]),
            "mixed": R.organic_and_h2so4_nucleation_rate(x["h2so4"], x["monoterpene"], x["OH"], x["temp"], x["condensation_sink"], params("f64")[2])}
    g = {k: _np(getattr(got, k)) for k in OUTS}
    for k in OUTS:
        assert not np.isnan(g[k]).any() and not np.isnan(refs[k]).any(), k
    rep = parity.assert_parity(g, refs, parity.RTOL[ft], names=OUTS, what=f"aerosol nucleation {ft}", family=FAMILY, pinned_by=PINNED)
    for k in OUTS:      # every point with a reference value inside the float type's range: the plain relative bound (no exclusions)
        r = refs[k]
        keep = (np.abs(r) > parity.FLOOR[ft]) & (np.abs(r) < parity.CEIL[ft])
        rel = np.abs(g[k][keep] - r[keep]) / np.abs(r[keep])
        assert rel.max() <= parity.RTOL[ft], (k, ft, float(rel.max()))
        print(f"\n[nucleation parity] {k} {ft}: {rep[k]:.3e}, worst plain relative error {rel.max():.3e} over {int(keep.sum())} points")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_apparent_rate_parity(dev, ft):
    import cmx
    cols, id_ = apparent_states(1_000_003, 19)
    t = [_t(c, ft, dev) for c in cols]
    for with_id in (True, False):
        i = _t(id_, ft, dev) if with_id else None
        J = _np(cmx.apparent_nucleation_rate(*t, i))
        ref = R.apparent_nucleation_rate(*[_np(c) for c in t], _np(i) if with_id else 1.7)
        parity.assert_parity({"J_x": J}, {"J_x": ref}, parity.RTOL[ft], names=("J_x",), what=f"apparent nucleation rate {ft}", family=FAMILY,
                             pinned_by="tests/nucleation_ref.py (derived J_x = 1e6 in tests/golden/nucleation_kats.json)")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_p3_counts_parity(dev, ft):
    """T straddling T₀ and T_dep_thres; against the restatement's expm1 form, and against the oracle (Float64): N_dep everywhere, N_het where
    |het_B V_l Δt exp(het_a Tₛ)| ≥ 1e-6 (below that the oracle's own 1 − exp loses Float64 digits)"""
    import cmx
    import oracle_binding as ob
    ip = P.MorrisonMilbrandt2014(ft)
    g = np.random.default_rng(23)
    n = 1_000_003
    T0, Td = float(ip.T0), float(ip.T_dep_thres)
    T = np.concatenate([g.uniform(190, 320, n - 6), [T0, np.nextafter(np.float32(T0), 0), np.nextafter(np.float32(T0), 400), Td, Td - 1, Td + 1]])
    Nl, Vl, dt = 10 ** g.uniform(6, 9, n), 10 ** g.uniform(-18, -12, n), g.uniform(1, 300, n)
    t = [_t(a, ft, dev) for a in (T, Nl, Vl, dt)]
    Nd = _np(cmx.P3_deposition_N_i(ip, t[0]))
    Nh = _np(cmx.P3_het_N_i(ip, *t))
    x = [_np(a) for a in t]
    rd, rh = R.p3_deposition_N_i(ip, x[0]), R.p3_het_N_i(ip, *x)
    parity.assert_parity({"N_dep": Nd, "N_het": Nh}, {"N_dep": rd, "N_het": rh}, parity.RTOL[ft], names=("N_dep", "N_het"),
                         what=f"P3 ice-nucleation counts {ft}", family=FAMILY, pinned_by="tests/nucleation_ref.py (expm1 form; p3_kats.json)")
    assert bool((Nd[x[0] >= T0] == 0).all()) and bool((Nd[x[0] < T0] > 0).all())
    sub = np.linspace(0, n - 1, 3000).astype(int)
    ip64 = P.MorrisonMilbrandt2014("f64")
    od = np.array([ob.P3_deposition_N_i(_abi.F64, ip64, x[0][i]) for i in sub])
    np.testing.assert_allclose(Nd[sub], od, rtol=parity.RTOL[ft], atol=0)
    arg = np.abs(float(ip64.het_B) * x[2] * x[3] * np.exp(float(ip64.het_a) * (float(ip64.T0) - x[0])))
    sh = sub[arg[sub] >= 1e-6]
    oh = np.array([ob.P3_het_N_i(_abi.F64, ip64, x[0][i], x[1][i], x[2][i], x[3][i]) for i in sh])
    np.testing.assert_allclose(Nh[sh], oh, rtol=parity.RTOL[ft], atol=0)
    assert sh.size > 500


# ---- semantics: NaN, negatives, NULL outputs, alignment, fused vs prescribed ------------------------------------------------------------

# the columns each output's VALUE depends on (NaN rule) and the columns the entry requires for it (the reference function's arguments)
NEEDS = {"binary": ("h2so4", "nh3", "negative_ion", "temp"), "ternary": ("h2so4", "nh3", "negative_ion", "temp"),
         "organic": ("negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink"),
         "mixed": ("h2so4", "monoterpene", "OH", "temp", "condensation_sink")}
READS = {"binary": ("h2so4", "negative_ion", "temp"), "ternary": ("h2so4", "nh3", "negative_ion", "temp"),
         "organic": ("negative_ion", "monoterpene", "O3", "OH", "temp", "condensation_sink"),
         "mixed": ("h2so4", "monoterpene", "OH", "temp", "condensation_sink")}


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_nan_and_negative_inputs(dev, ft):
    import cmx
    s = random_states(64, 29)
    for col in s:
        cols = {k: _t(v, ft, dev) for k, v in s.items()}
        cols[col][::3] = float("nan")
        got = _fused(ft, cols)
        for k in OUTS:
            v = getattr(got, k)
            if col in READS[k]:
                assert bool(torch.isnan(v[::3]).all()), (col, k)
            else:
                assert not bool(torch.isnan(v).any()), (col, k)
    # negative bases of non-integer powers: NaN (the reference's DomainError)
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    cols["h2so4"][::2] *= -1
    got = _fused(ft, cols)
    assert bool(torch.isnan(got.binary[::2]).all() and torch.isnan(got.ternary[::2]).all()) and bool((got.mixed[::2] > 0).all())
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    cols["nh3"][::2] *= -1
    got = _fused(ft, cols)
    assert bool(torch.isnan(got.binary[::2]).all() and torch.isnan(got.ternary[::2]).all())
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    cols["condensation_sink"][::2] *= -1                          # HOM < 0
    got = _fused(ft, cols)
    assert bool(torch.isnan(got.organic[::2]).all())
    ip = P.MorrisonMilbrandt2014(ft)
    T = _t([240.0, float("nan"), 280.0], ft, dev)
    Nd = cmx.P3_deposition_N_i(ip, T)
    assert float(Nd[0]) > 0 and bool(torch.isnan(Nd[1])) and float(Nd[2]) == 0       # NaN T → NaN (the reference's ifelse returns 0)
    one = _t([1.0] * 3, ft, dev)
    Nh = cmx.P3_het_N_i(ip, T, one * 1e8, one * 1e-15, one * 10)
    assert bool(torch.isnan(Nh[1])) and not bool(torch.isnan(Nh[0]))


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_every_null_output_combination_is_bit_identical(dev, ft):
    import itertools
    s = random_states(100_003, 31)
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    full = _fused(ft, cols)
    for r in range(1, 4):
        for want in itertools.combinations(OUTS, r):
            got = _fused(ft, {k: (v if any(k in NEEDS[w] for w in want) else None) for k, v in cols.items()}, want=want)
            for k in OUTS:
                if k in want:
                    assert torch.equal(_bits(getattr(got, k)), _bits(getattr(full, k))), (want, k)
                else:
                    assert getattr(got, k) is None


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_offset_views_are_bit_identical(dev, ft):
    import cmx
    n = 50_000
    s = random_states(n + 8, 37)
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    full = _fused(ft, cols)
    for lo in (1, 2, 3):
        got = _fused(ft, {k: v[lo:lo + n] for k, v in cols.items()})
        for k in OUTS:
            assert torch.equal(_bits(getattr(got, k)), _bits(getattr(full, k)[lo:lo + n])), (lo, k)
    # mixed offsets between the columns: one scalar range
    got = _fused(ft, {k: (v[1:1 + n] if k == "temp" else v[0:n]) for k, v in cols.items()})
    ref = _fused(ft, {k: (v[1:1 + n].clone() if k == "temp" else v[0:n]) for k, v in cols.items()})
    for k in OUTS:
        assert torch.equal(_bits(getattr(got, k)), _bits(getattr(ref, k)))
    ac, aid = apparent_states(n + 8, 41)
    at = [_t(c, ft, dev) for c in ac] + [_t(aid, ft, dev)]
    Jf = cmx.apparent_nucleation_rate(*at)
    ip = P.MorrisonMilbrandt2014(ft)
    pt = [cols["temp"], cols["OH"], _t(10 ** np.random.default_rng(1).uniform(-18, -12, n + 8), ft, dev), cols["temp"] * 0 + 30]
    Nh = cmx.P3_het_N_i(ip, *pt)
    for lo in (1, 2, 3):
        assert torch.equal(_bits(cmx.apparent_nucleation_rate(*[c[lo:lo + n] for c in at])), _bits(Jf[lo:lo + n]))
        assert torch.equal(_bits(cmx.P3_het_N_i(ip, *[c[lo:lo + n] for c in pt])), _bits(Nh[lo:lo + n]))


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_fused_matches_the_prescribed_forms(dev, ft):
    """The fused entry against the prescribed entry fed the HOM / bioOxOrg the reference's composition forms (restatement, Float64, rounded to FT).
    Not bit-identical: the device's HOM and bioOxOrg carry the rounding of its exp2 / rcp and of the folded Y·k and unit factors, which the rates
    amplify by their exponents (≈ a_2 + a_5/x for the organic rate, 1 for the mixed one) — bounded by 2e-5 (Float32) / 1e-12 (Float64)."""
    import cmx
    hp, op, mp = params(ft)
    s = random_states(200_003, 43)
    cols = {k: _t(v, ft, dev) for k, v in s.items()}
    got = _fused(ft, cols, want=("organic", "mixed"))
    x = {k: _np(v) for k, v in cols.items()}
    _, op64, mp64 = params("f64")
    hom = _t(R.hom_concentration(x["monoterpene"], x["O3"], x["OH"], x["temp"], x["condensation_sink"], op64), ft, dev)
    bio = _t(R.bio_ox_org(x["monoterpene"], x["OH"], x["temp"], x["condensation_sink"], mp64), ft, dev)
    pres = cmx.nucleation_rates_prescribed(op, mp, negative_ion=cols["negative_ion"] * 1e-6, HOM=hom, h2so4=cols["h2so4"], bioOxOrg=bio)
    bound = {"f32": 2e-5, "f64": 1e-12}[ft]
    for k in ("organic", "mixed"):
        a, b = _np(getattr(got, k)), _np(getattr(pres, k))
        keep = (np.abs(b) > parity.FLOOR[ft]) & (np.abs(b) < parity.CEIL[ft])
        e = np.abs(a[keep] - b[keep]) / np.abs(b[keep]) / np.maximum(1.0, np.abs(np.log(np.abs(b[keep]))))
        assert e.max() <= bound, (k, ft, float(e.max()))
