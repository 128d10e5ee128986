"""SB2006 precipitation susceptibilities (src/PrecipitationSusceptibility.jl), CPU side:

  * the float64 restatement tests/precip_susceptibility_ref.py against the fixture tests/golden/precip_susceptibility_kats.json (the reference test's
    state and its `≈`), against the reference test's own arrangement of the formulas, and against central differences of the logarithm of the
    oracle's autoconversion / accretion rain source;
  * the device point function and its host folding (csrc/cmx_precip_susceptibility.hpp) compiled by g++ (tests/native/precip_susceptibility_host.cpp)
    against the restatement in both float types, at the bounds of the GPU test, with the NaN contract and the abs rule;
  * the argument checks of the C ABI that need no GPU, and the Python wrapper's refusal of CPU tensors."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import precip_susceptibility_ref as R
from cmx import _abi, _lib
from cmx import parameters as P

REPO = Path(__file__).resolve().parent.parent
KATS = json.loads((REPO / "tests" / "golden" / "precip_susceptibility_kats.json").read_text())
NPT = {"f32": np.float32, "f64": np.float64}
CT = {"f32": C.c_float, "f64": C.c_double}
RTOL = {"f32": 1e-3, "f64": 1e-6}              # the project's plain bounds (tests/parity.py), on |x − ref| ≤ rtol·max(|ref|, 1)
OUTS = ("acnv_d_ln_q_lcl", "acnv_d_ln_q_rai", "acnv_d_ln_N_lcl", "accr_d_ln_q_lcl", "accr_d_ln_q_rai", "accr_d_ln_N_lcl")
N_DRAW = 200_003                               # ≥ 2e5 states, odd: the GPU test runs the same draw through the alignment split
NEAR_CAP = 1e-3


def draw(ft, n=N_DRAW, seed=1234):
    """the random draw, rounded to the float type (the values the device sees), as float64"""
    return [a.astype(NPT[ft]).astype(np.float64) for a in R.random_states(n, seed)]


def reference(x, ft):
    """name → float64 column of the restatement at the float type's gates, default parameters"""
    sb = P.SB2006("f64")
    au, ac = R.autoconversion(sb.acnv, *x, R.EPS[ft]), R.accretion(sb.accr, *x, R.EPS[ft])
    return {**{"acnv_" + k: v for k, v in au.items()}, **{"accr_" + k: v for k, v in ac.items()}}


def near_clip(x):
    return R.near_clip(P.SB2006("f64").acnv, x[0], x[2], x[3])


def group_shares(x, ft):
    """share of ALL states in each group the draw must populate"""
    ref = reference(x, ft)
    ql, qr = np.abs(x[0]), np.abs(x[1])
    au_ok = ~np.isnan(ref["acnv_d_ln_q_lcl"])
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = qr / (ql + qr)
    return {"clipped": float(np.mean(au_ok & (ref["acnv_d_ln_N_lcl"] == 0))), "q_rai_below_eps": float(np.mean(au_ok & (qr < R.EPS[ft]))),
            "acnv_gate": float(np.mean(~au_ok)), "accr_gate": float(np.mean(np.isnan(ref["accr_d_ln_q_lcl"]))),
            "tau_above_0.99": float(np.mean(au_ok & (tau > 0.99)))}


def compare(got, x, ft, what):
    """NaN exactly where the restatement has NaN; |x − ref| ≤ rtol·max(|ref|, 1) at every other state, except the autoconversion outputs of the states
    within 1e-5 of the clip x̄_c = x_star (their share is capped).  Returns the worst |x − ref|/max(|ref|, 1) per output."""
    ref = reference(x, ft)
    near = near_clip(x)
    assert near.mean() <= NEAR_CAP, (what, ft, near.mean())
    worst = {}
    for k in OUTS:
        if got.get(k) is None:
            continue
        g, r = np.asarray(got[k], dtype=np.float64), ref[k]
        assert (np.isnan(g) == np.isnan(r)).all(), (what, k, ft, np.flatnonzero(np.isnan(g) != np.isnan(r))[:5])
        keep = ~np.isnan(r) & ~(near if k.startswith("acnv") else False)
        e = np.abs(g[keep] - r[keep]) / np.maximum(np.abs(r[keep]), 1.0)
        worst[k] = float(e.max()) if e.size else 0.0
        print(f"\n[precip susceptibility {what}] {k} {ft}: worst |x - ref|/max(|ref|, 1) = {worst[k]:.3e} over {int(keep.sum())} states")
        assert worst[k] <= RTOL[ft], (what, k, ft, worst[k], g[keep][np.argmax(e)], r[keep][np.argmax(e)])
    return worst


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def test_restatement_reproduces_the_fixture():
    sb = P.SB2006("f64")
    s = KATS["state"]
    x = (s["q_lcl"], s["q_rai"], s["rho"], s["N_lcl"])
    au, ac = R.autoconversion(sb.acnv, *x, R.EPS["f64"]), R.accretion(sb.accr, *x, R.EPS["f64"])
    for name, got in (("autoconversion", au), ("accretion", ac)):
        for f in R.FIELDS:
            e = KATS[name]["d_ln_pp_" + f]
            assert e["provenance"]
            assert float(got[f]) == pytest.approx(e["expected"], rel=KATS["rtol"], abs=0), (name, f)
    assert KATS["rtol"] == 1.5e-8 and KATS["autoconversion"]["d_ln_pp_d_ln_N_lcl"]["expected"] == -2
    assert KATS["autoconversion"]["d_ln_pp_d_ln_N_rai"]["expected"] == 0 and KATS["accretion"]["d_ln_pp_d_ln_N_rai"]["expected"] == 0


def test_restatement_matches_the_reference_tests_arrangement():
    """test/precipitation_susceptibility_tests.jl:59-68 with its own d_ln_phi_*_d_ln_τ (:11-29), at its state and over ungated, unclipped random
    states, at that test's `≈` (rtol sqrt(eps) = 1.5e-8).  States with 1 − τ < 1e-3 are left to the other tests: the reference arrangement divides two
    differences that cancel there ((τ − 1)³ against A (τ − 1) τ^a (1 − τ^a)^b), so it is no yardstick at 1.5e-8."""
    sb = P.SB2006("f64")
    s = KATS["state"]
    ql, qr, rho, N = (np.concatenate([[s[k]], np.abs(c)]) for k, c in zip(("q_lcl", "q_rai", "rho", "N_lcl"), R.random_states(50_000, 3)))
    eps = R.EPS["f64"]
    au, ac = R.autoconversion(sb.acnv, ql, qr, rho, N, eps), R.accretion(sb.accr, ql, qr, rho, N, eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = 1 - ql / (ql + qr)
        keep = ~np.isnan(ac["d_ln_q_lcl"]) & (au["d_ln_N_lcl"] == -2) & (1 - tau >= 1e-3)
        dau, dac = R.d_ln_phi_au_d_ln_tau(sb.acnv, tau), R.d_ln_phi_acc_d_ln_tau(sb.accr, tau)
    assert keep[0] and keep.sum() > 20_000
    k = keep
    np.testing.assert_allclose(au["d_ln_q_lcl"][k], (4 - (1 - tau) * dau)[k], rtol=1.5e-8, atol=0)
    np.testing.assert_allclose(au["d_ln_q_rai"][k], ((1 - tau) * dau)[k], rtol=1.5e-8, atol=1e-15)
    np.testing.assert_allclose(ac["d_ln_q_lcl"][k], (1 - (1 - tau) * dac)[k], rtol=1.5e-8, atol=0)
    np.testing.assert_allclose(ac["d_ln_q_rai"][k], (1 + (1 - tau) * dac)[k], rtol=1.5e-8, atol=0)


FD_WORST = 7.2e-9          # measured: see test_restatement_matches_log_differences_of_the_oracle_rates


def test_restatement_matches_log_differences_of_the_oracle_rates(oracle):
    """Central differences (step 1e-5 in ln q_lcl, ln q_rai, ln N_lcl) of ln CMX_SB_ACNV_DQ_RAI and ln CMX_SB_ACCR_DQ_RAI of the oracle's
    sb2006_process_rates in float64, over the ungated states of the random draw with τ ≥ 1e-3 and |x̄_c/x_star − 1| > 1e-3 (a difference across the
    ifelse at q_rai = ϵ or across the min at x_star is no derivative).  The bound belongs to the difference quotient, not to the closed form: its
    truncation error is h²/6 · |∂³ ln rate/∂(ln x)³| = 1.7e-11 · |∂³…| and its rounding error (eps/h = 2e-11) × the relative rounding of the oracle's rate
    in units of eps.  Measured worst |closed form − quotient| over the 1.6e5 states kept: 7.1e-9 (autoconversion, d/d ln q_rai; d/d ln q_lcl 4.4e-9,
    accretion 2.5e-9 and 1.3e-9, d/d ln N_lcl 6.3e-10 and 0); asserted: 10 × the worst."""
    sb = P.SB2006("f64")
    wr, tps = P.WarmRainParams2M("f64"), P.ThermodynamicsParameters("f64")
    x = [np.abs(a) for a in draw("f64")]
    eps = R.EPS["f64"]
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = x[1] / (x[0] + x[1])
        keep = (x[0] >= eps) & (x[1] >= eps) & (x[3] >= eps) & (tau >= 1e-3) & (np.abs(R.x_ratio(sb.acnv, x[0], x[2], x[3]) - 1) > 1e-3)
    x = [a[keep] for a in x]
    n = x[0].size
    assert n > 100_000
    au, ac = R.autoconversion(sb.acnv, *x, eps), R.accretion(sb.accr, *x, eps)
    q_tot, N_rai, T = np.full(n, 1.5e-2), np.full(n, 1e4), np.full(n, 285.0)

    def ln_rates(ql, qr, N):
        r = oracle.sb2006_process_rates(_abi.F64, wr.c, tps, None, _abi.CMX_SB2006_LIMITED, q_tot, ql, qr, N, N_rai, x[2], T)
        return np.log(r["acnv_dq_rai_dt"]), np.log(r["accr_dq_rai_dt"])
    h = 1e-5
    worst = 0.0
    for j, f in ((0, "d_ln_q_lcl"), (1, "d_ln_q_rai"), (3, "d_ln_N_lcl")):
        up, dn = [a.copy() for a in x], [a.copy() for a in x]
        up[j] = x[j] * np.exp(h)
        dn[j] = x[j] * np.exp(-h)
        (au_u, ac_u), (au_d, ac_d) = ln_rates(up[0], up[1], up[3]), ln_rates(dn[0], dn[1], dn[3])
        for name, ref, fd in (("acnv", au[f], (au_u - au_d) / (2 * h)), ("accr", ac[f], (ac_u - ac_d) / (2 * h))):
            e = float(np.abs(ref - fd).max())
            print(f"\n[precip susceptibility log-difference] {name} {f}: worst |closed form - quotient| = {e:.3e} over {n} states")
            worst = max(worst, e)
            assert e <= 10 * FD_WORST, (name, f, e)
    print(f"\n[precip susceptibility log-difference] worst of all = {worst:.3e}")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_the_draw_populates_every_branch_and_stays_off_the_clip(ft):
    x = draw(ft)
    assert x[0].size >= 200_000
    assert near_clip(x).mean() <= NEAR_CAP                           # the restatement's draw alone meets the cap
    shares = group_shares(x, ft)
    print(f"\n[precip susceptibility draw] {ft}: {shares}")
    for k, v in shares.items():
        assert v >= 0.01, (ft, k, v)
    ql, qr = R.random_states(N_DRAW)[:2]
    for q in (ql, qr):
        assert 0.015 < np.mean(q == 0) < 0.025 and 0.005 < np.mean(q < 0) < 0.015
    assert 0.005 < np.mean(R.random_states(N_DRAW)[3] == 0) < 0.015


# ---- the point function and its host folding ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    out = REPO / "tests" / "native" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libprecip_susceptibility_host.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so),
                    str(REPO / "tests" / "native" / "precip_susceptibility_host.cpp")], check=True)
    return C.CDLL(str(so))


def host_run(host, ft, x, want=OUTS, sb=None):
    sb = sb or P.SB2006(ft)
    cols = [np.ascontiguousarray(a, dtype=NPT[ft]) for a in x]
    out = {k: (np.full(cols[0].size, -7.0, dtype=NPT[ft]) if k in want else None) for k in OUTS}
    pp = lambda a: a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None  # noqa: E731
    outs = (C.POINTER(CT[ft]) * 6)(*[pp(out[k]) for k in OUTS])
    au, ac = any(k.startswith("acnv") for k in want), any(k.startswith("accr") for k in want)
    getattr(host, f"precip_susceptibility_{ft}")(C.byref(sb.acnv) if au else None, C.byref(sb.accr) if ac else None, C.c_int64(cols[0].size),
                                                 *[pp(a) for a in cols], outs)
    return out


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_matches_the_restatement(host, ft):
    x = draw(ft)
    compare(host_run(host, ft, x), x, ft, "host")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_known_answers(host, ft):
    s = KATS["state"]
    got = host_run(host, ft, [np.array([s[k]]) for k in ("q_lcl", "q_rai", "rho", "N_lcl")])
    for proc, name in (("acnv", "autoconversion"), ("accr", "accretion")):
        for f in R.FIELDS:
            e = KATS[name]["d_ln_pp_" + f]["expected"]
            tol = KATS["rtol"] if ft == "f64" else RTOL[ft]           # the fixture's own rtol; Float32 at the project's bound
            assert abs(float(got[f"{proc}_{f}"][0]) - e) <= tol * max(abs(e), 1), (proc, f)
    assert float(got["acnv_d_ln_N_lcl"][0]) == -2.0 and float(got["accr_d_ln_N_lcl"][0]) == 0.0


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_abs_nan_and_gates(host, ft):
    x = draw(ft, 20_001, 7)
    full = host_run(host, ft, x)
    flipped = host_run(host, ft, [-a for a in x])
    absd = host_run(host, ft, [np.abs(a) for a in x])
    for k in OUTS:                                                  # the inputs enter through abs: bit for bit
        assert full[k].tobytes() == flipped[k].tobytes() == absd[k].tobytes(), k
    for j in range(4):                                              # a NaN in any one input: NaN in all six outputs
        y = [a.copy() for a in x]
        y[j][::3] = np.nan
        got = host_run(host, ft, y)
        for k in OUTS:
            assert np.isnan(got[k][::3]).all(), (j, k)
            m = np.ones(y[0].size, bool)
            m[::3] = False
            assert got[k][m].tobytes() == full[k][m].tobytes(), (j, k)
    eps = R.EPS[ft]
    one = lambda *v: [np.array([a]) for a in v]  # noqa: E731
    g = host_run(host, ft, one(5e-4, 1e-5, 0.0, 1e8))               # ρ = 0
    assert all(np.isnan(g[k][0]) for k in OUTS)
    g = host_run(host, ft, one(5e-4, eps / 2, 1.0, 1e8))            # q_rai < ϵ: accretion gated, autoconversion without its τ-dependence
    assert all(np.isnan(g[k][0]) for k in OUTS if k.startswith("accr"))
    assert float(g["acnv_d_ln_q_lcl"][0]) == 4.0 and float(g["acnv_d_ln_q_rai"][0]) == 0.0 and float(g["acnv_d_ln_N_lcl"][0]) == -2.0
    g = host_run(host, ft, one(5e-4, 0.0, 1.0, 1e5))                # clipped: x̄_c = 5e-9 > x_star
    assert float(g["acnv_d_ln_q_lcl"][0]) == 2.0 and float(g["acnv_d_ln_N_lcl"][0]) == 0.0
    for state in (one(eps / 2, 1e-5, 1.0, 1e8), one(5e-4, 1e-5, 1.0, eps / 2), one(0.0, 0.0, 1.0, 1e8)):     # q_lcl < ϵ, N_lcl < ϵ: both gated
        g = host_run(host, ft, state)
        assert all(np.isnan(g[k][0]) for k in OUTS), state


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_is_finite_as_tau_tends_to_one(host, ft):
    """q_lcl at its gate under a large q_rai: 1 − τ and 1 − τ^a vanish together; the form without a division by 1 − τ^a stays finite and inside the bound"""
    eps = R.EPS[ft]
    ql = np.array([eps, 2 * eps, 10 * eps, 1e3 * eps] * 3)
    qr = np.repeat([5e-3, 1e-1, 1.0], 4)
    x = [a.astype(NPT[ft]).astype(np.float64) for a in (ql, qr, np.ones(12), np.full(12, 1e8))]
    got = host_run(host, ft, x)
    assert all(np.isfinite(got[k]).all() for k in OUTS)
    compare(got, x, ft, "host, tau -> 1")


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_point_function_general_exponent_matches_the_integer_one(host, ft):
    """b = 3 takes (1 − τ^a)^(b−1) by multiplication; a b next to 3 takes exp2((b − 1) log2 …): the two agree to the bound at b → 3, and a struct
    with other constants follows the restatement"""
    x = draw(ft, 50_001, 11)
    sb = P.SB2006(ft)
    sb.acnv.b = 2.5
    sb.acnv.A = 250.0
    sb.accr.c = 3.0
    got = host_run(host, ft, x, sb=sb)
    sb64 = P.SB2006("f64")
    sb64.acnv.b, sb64.acnv.A, sb64.accr.c = 2.5, 250.0, 3.0
    au, ac = R.autoconversion(sb64.acnv, *x, R.EPS[ft]), R.accretion(sb64.accr, *x, R.EPS[ft])
    ref = {**{"acnv_" + k: v for k, v in au.items()}, **{"accr_" + k: v for k, v in ac.items()}}
    for k in OUTS:
        ok = ~np.isnan(ref[k])
        assert (np.isnan(got[k]) == ~ok).all(), k
        assert (np.abs(got[k][ok] - ref[k][ok]) <= RTOL[ft] * np.maximum(np.abs(ref[k][ok]), 1)).all(), k


# ---- C ABI argument checks, Python wrapper ---------------------------------------------------------------------------------------------

def test_argument_checks_without_gpu():
    lib = _lib.lib()
    B, OK, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_OK, _abi.CMX_ERR_UNSUPPORTED
    col = C.c_void_p(4096)
    for ft in ("f32", "f64"):
        sb = P.SB2006(ft)
        f = getattr(lib, f"cmx_sb2006_precip_susceptibility_{ft}")
        au, ac = C.byref(sb.acnv), C.byref(sb.accr)
        ins, six, nul = [col] * 4, [col] * 6, [None] * 6
        assert f(au, ac, 10, *ins, *nul, None) == B                                   # no output requested
        assert f(au, ac, -1, *ins, *six, None) == B                                   # n < 0
        assert f(au, ac, 16 * 0x7fffffff + 1, *ins, *six, None) == UNS                # above the count limit
        assert f(None, ac, 10, *ins, col, None, None, None, None, None, None) == B    # an autoconversion output without its struct
        assert f(au, None, 10, *ins, None, None, None, None, col, None, None) == B    # an accretion output without its struct
        assert f(None, None, 10, *ins, *six, None) == B
        assert f(au, ac, 0, *[None] * 4, *six, None) == OK                            # n == 0
        assert f(au, None, 0, *[None] * 4, col, None, None, None, None, None, None) == OK
        for k in range(4):                                                            # every input column is required (only refused calls are made here)
            x = list(ins)
            x[k] = None
            assert f(au, ac, 10, *x, *six, None) == B, k


def test_python_api_refuses_cpu_tensors_and_wrong_schemes():
    import torch
    import cmx
    t = torch.ones(4, dtype=torch.float64)
    sb = P.SB2006("f64")
    for fn in (cmx.precipitation_susceptibility_autoconversion, cmx.precipitation_susceptibility_accretion, cmx.precipitation_susceptibilities):
        with pytest.raises(ValueError):
            fn(sb, t, t, t, t)
    assert cmx.precip_susceptibility_rates._fields == ("d_ln_pp_d_ln_q_lcl", "d_ln_pp_d_ln_q_rai", "d_ln_pp_d_ln_N_lcl", "d_ln_pp_d_ln_N_rai")
