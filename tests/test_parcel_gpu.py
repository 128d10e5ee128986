"""The parcel model on the device (include/cmx.h §(13), cmx/parcel.py) against the NumPy restatement tests/parcel_ref.py.

  * parcel_tendencies: every supported option value, ≥ 2e5 states (an odd count, columns at an odd offset), the project's plain bounds on
    |x − ref| ≤ rtol·max(|ref|, Σ|terms|), NaN exactly where the restatement has NaN;
  * parcel_run, Float64: final state and every trajectory record at 1e-6 on the scales of the issue (S_l, p, T on their own magnitude, q on q_tot,
    N on N_aer + N_liq + N_ice), parcels inside the gate mask left out (≤ 1 %);
  * parcel_run, Float32: four times the reference-only Float32-vs-Float64 spread of the restatement, per variable and ensemble
    (tests/golden/parcel_f32_spread.json, tools/gen_parcel_spread.py) — the code under test takes no part in that bound;
  * splitting, saving, in place, coefficient columns, NaN: bit for bit.
The ensembles are the ones tests/test_parcel_host.py vets on the CPU (finite, exclusion share).  At most 2e5 parcels × 1 step or 4096 parcels × 600 steps.
"""
import numpy as np
import pytest
import torch

import parcel_cases as PC
import parcel_ref as R
from cmx import parcel
from test_parcel_host import compare_tendencies

pytestmark = pytest.mark.gpu
TD = {"f32": torch.float32, "f64": torch.float64}


def dev():
    return torch.device("cuda:0")


def to_dev(cols, ft, pad=0):
    """Columns on the device; pad > 0 places each column `pad` elements into its own allocation (an address that is not 16-byte aligned)."""
    out = []
    for c in cols:
        t = torch.empty(len(c) + pad, dtype=TD[ft], device=dev())
        t[pad:] = torch.from_numpy(np.asarray(c, dtype=PC.NPT[ft]))
        out.append(t[pad:])
    return out


def same_bits(a, b):
    """Bit-for-bit equality (a NaN equals the same NaN)."""
    iv = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def host_rows(t):
    return [r.cpu().numpy() for r in t]


# ---- parcel_tendencies ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("combo", list(PC.TENDENCY_COMBOS))
def test_tendencies_match_the_restatement(ft, combo):
    cfg = PC.TENDENCY_COMBOS[combo]
    pp, prm = PC.build(ft, **cfg["kw"])
    cols, w, nan_at = PC.tendency_states(PC.N_TENDENCY, 21, cfg["T"], prm["tps"])
    Y, w = [c.astype(PC.NPT[ft]) for c in cols], w.astype(PC.NPT[ft])
    ref = R.rhs(np.float64, prm, PC.ref_options(cfg["kw"]), Y, w, margin=PC.MARGIN[ft])
    d = to_dev(Y + [w], ft, pad=1)                        # odd count, odd offset
    out = parcel.parcel_tendencies(d[:9], pp, w=d[9])
    torch.cuda.synchronize()
    dY, proc = host_rows(out.dY[:9]), [out.process_rates[k].cpu().numpy() for k in R.PROCESS]
    report = {}
    worst = compare_tendencies(ft, dY, proc, ref, f"gpu {ft} {combo}", report)
    print(f"parcel_tendencies {ft} {combo}: n={PC.N_TENDENCY} excluded={int(ref['near_gate'].sum())} worst={worst:.3e} "
          + " ".join(f"{k}={v:.1e}" for k, v in report.items()))
    assert not out.dY[9].any()                            # the ln_INPC row
    for j, i in nan_at.items():
        assert all(np.isnan(a[i]) for a in dY + proc), (j, i)
    assert int(np.isnan(dY[1]).sum()) == len(nan_at)      # dp/dt has no other source of NaN: no other parcel is touched


# ---- parcel_run ----------------------------------------------------------------------------------------------------------------------------------
def _run_case(ft, case, steps):
    cfg = PC.RUN_CASES[case]
    pp, prm = PC.build(ft, **cfg["kw"])
    Y0, w = PC.run_ensemble(case, prm)
    Y, w = [c.astype(PC.NPT[ft]) for c in Y0], w.astype(PC.NPT[ft])
    ref = R.run(np.float64, prm, PC.ref_options(cfg["kw"]), Y, w, steps, save_every=PC.SAVE_EVERY, margin=PC.MARGIN[ft])
    d = to_dev(Y + [w], ft)
    sol = parcel.run_parcel(d[:9] + [0.0], 0.0, steps * prm["const_dt"], pp, w=d[9], save_every=PC.SAVE_EVERY)
    torch.cuda.synchronize()
    keep = ~ref["near_gate"]
    assert np.mean(~keep) <= PC.EXCLUDED_CAP
    Y64 = [y.astype(np.float64) for y in Y]
    final = PC.scaled_run_error(host_rows(sol.u[:9]), ref["final"], Y64)[:, keep]
    traj = sol.trajectory.cpu().numpy()
    assert traj.shape == (1 + steps // PC.SAVE_EVERY, 10, PC.N_RUN) and sol.t[-1] == steps * prm["const_dt"]
    recs = np.stack([PC.scaled_run_error(traj[r, :9], ref["trajectory"][r], Y64)[:, keep].max(axis=1) for r in range(traj.shape[0])])
    return final.max(axis=1), recs, int((~keep).sum())


@pytest.mark.parametrize("case", list(PC.RUN_CASES))
def test_run_f64_matches_the_restatement(case):
    steps = PC.RUN_CASES[case]["steps64"]
    final, recs, excluded = _run_case("f64", case, steps)
    print(f"parcel_run f64 {case}: {steps} steps, excluded={excluded}, max scaled error per variable " +
          " ".join(f"{n}={v:.1e}" for n, v in zip(R.STATE, np.maximum(final, recs.max(axis=0)))))
    assert np.all(np.isfinite(final)) and np.all(np.isfinite(recs))
    assert final.max() <= PC.RTOL["f64"], dict(zip(R.STATE, final))
    assert recs.max() <= PC.RTOL["f64"], recs.max(axis=0)


@pytest.mark.parametrize("case", PC.F32_RUN_CASES)
def test_run_f32_within_four_times_the_reference_spread(case):
    steps = PC.RUN_CASES[case]["steps32"]
    spread = PC.load_spread()[case][str(steps)]
    final, _, excluded = _run_case("f32", case, steps)
    print(f"parcel_run f32 {case}: {steps} steps, excluded={excluded}, scaled error / reference spread per variable " +
          " ".join(f"{n}={v:.1e}/{spread[n]:.1e}" for n, v in zip(R.STATE, final)))
    for n, v in zip(R.STATE, final):
        assert np.isfinite(v) and v <= PC.SPREAD_FACTOR * spread[n], (n, v, spread[n])


def _setup(ft, case="abifm_cond_dep_mono", n=1537):
    cfg = PC.RUN_CASES[case]
    pp, prm = PC.build(ft, **cfg["kw"])
    Y0, w = PC.run_ensemble(case, prm)
    d = to_dev([c[:n] for c in Y0] + [w[:n]], ft)
    return pp, prm, d[:9] + [0.0], d[9]


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_splitting_saving_and_in_place_are_bit_identical(ft):
    pp, prm, IC, w = _setup(ft)
    cap = parcel.MAX_STEPS_PER_LAUNCH
    total = cap + 44 if ft == "f64" else 200              # Float64: across the steps-per-launch cap inside one call
    one = parcel.run_parcel(IC, 0.0, float(total), pp, w=w, save_every=50)
    a = 70
    first = parcel.run_parcel(IC, 0.0, float(a), pp, w=w)
    second = parcel.run_parcel(list(first.u), float(a), float(total), pp, w=w)
    assert same_bits(one.u, second.u)
    # record j of the trajectory = the final state of a run of j·save_every steps
    for j in (0, 1, 3):
        r = parcel.run_parcel(IC, 0.0, float(50 * j), pp, w=w)
        assert same_bits(one.trajectory[j], r.u), j
    # in place: the output rows are the input rows
    buf = torch.stack([c if isinstance(c, torch.Tensor) else torch.zeros_like(w) for c in IC]).contiguous()
    got = parcel.run_parcel([buf[j] for j in range(10)], 0.0, float(total), pp, w=w, out=buf)
    assert got.u.data_ptr() == buf.data_ptr() and same_bits(buf, one.u)
    if ft == "f32":                                       # across the cap in Float32 too, where nothing is compared with the restatement
        long1 = parcel.run_parcel(IC, 0.0, float(cap + 30), pp, w=w)
        part = parcel.run_parcel(IC, 0.0, float(cap), pp, w=w)
        long2 = parcel.run_parcel(list(part.u), float(cap), float(cap + 30), pp, w=w)
        assert same_bits(long1.u, long2.u)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_coefficient_columns(ft):
    pp, prm, IC, w = _setup(ft)
    n = w.numel()
    m, c = prm["aerosol_abifm"]["ABIFM_m"], prm["aerosol_abifm"]["ABIFM_c"]
    base = parcel.run_parcel(IC, 0.0, 100.0, pp, w=w)
    full = lambda v: torch.full((n,), v, dtype=TD[ft], device=dev())  # noqa: E731
    same = parcel.run_parcel(IC, 0.0, 100.0, pp, w=w, coefficients={"ABIFM_m": full(m), "ABIFM_c": full(c)})
    assert same_bits(base.u, same.u)                    # a column filled with the struct's value: the NULL-column bits
    # a two-valued column reproduces the two uniform runs, parcel by parcel
    m2, c2 = m * 0.9, c + 0.5
    other_pp, _ = PC.build(ft, **PC.RUN_CASES["abifm_cond_dep_mono"]["kw"])
    other_pp.c.aerosol_abifm.ABIFM_m, other_pp.c.aerosol_abifm.ABIFM_c = m2, c2
    other = parcel.run_parcel(IC, 0.0, 100.0, other_pp, w=w)
    pick = torch.arange(n, device=dev()) % 2 == 1
    # the column holds the struct's values as the float type rounds them, which is what the uniform runs used
    mixed = parcel.run_parcel(IC, 0.0, 100.0, pp, w=w, coefficients={
        "ABIFM_m": torch.where(pick, full(other_pp.c.aerosol_abifm.ABIFM_m), full(pp.c.aerosol_abifm.ABIFM_m)),
        "ABIFM_c": torch.where(pick, full(other_pp.c.aerosol_abifm.ABIFM_c), full(pp.c.aerosol_abifm.ABIFM_c))})
    assert same_bits(mixed.u[:, pick], other.u[:, pick]) and same_bits(mixed.u[:, ~pick], base.u[:, ~pick])
    assert not same_bits(other.u[8], base.u[8])         # the coefficients matter
    # a column of a scheme that is off is not read: a NaN in it touches nothing
    off = parcel.run_parcel(IC, 0.0, 100.0, pp, w=w, coefficients={"linear_c1": full(float("nan"))})
    assert same_bits(off.u, base.u)
    t0 = parcel.parcel_tendencies(IC, pp, w=w)
    t1 = parcel.parcel_tendencies(IC, pp, w=w, coefficients={"ABIFM_m": full(m), "ABIFM_c": full(c)})
    assert same_bits(t0.dY, t1.dY)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_nan_in_one_input_poisons_that_parcel_only(ft):
    pp, prm, IC, w = _setup(ft, n=640)
    base = parcel.run_parcel(IC, 0.0, 60.0, pp, w=w, save_every=20)
    for j in range(10):                                   # the nine state columns and w
        rows = [c.clone() if isinstance(c, torch.Tensor) else c for c in IC]
        ww = w.clone()
        i = 7 + 61 * j
        (rows[j] if j < 9 else ww)[i] = float("nan")
        got = parcel.run_parcel(rows, 0.0, 60.0, pp, w=ww, save_every=20)
        assert bool(got.u[:9, i].isnan().all()) and bool(got.trajectory[1:, :9, i].isnan().all()), j
        others = torch.ones(w.numel(), dtype=torch.bool, device=dev())
        others[i] = False
        assert same_bits(got.u[:, others], base.u[:, others]) and same_bits(got.trajectory[:, :, others], base.trajectory[:, :, others]), j
    with_nan_coef = parcel.run_parcel(IC, 0.0, 60.0, pp, w=w, coefficients={"ABIFM_c": torch.where(
        torch.arange(w.numel(), device=dev()) == 3, torch.full_like(w, float("nan")), torch.full_like(w, prm["aerosol_abifm"]["ABIFM_c"]))})
    assert bool(with_nan_coef.u[:9, 3].isnan().all()) and not bool(with_nan_coef.u[:9, 4:].isnan().any())


def test_run_is_graph_capturable():
    """The entry is a pure launch sequence on the caller's stream (several launches beyond the steps-per-launch cap): capture and replay."""
    pp, prm, IC, w = _setup("f32", n=513)
    total = float(parcel.MAX_STEPS_PER_LAUNCH + 10)
    eager = parcel.run_parcel(IC, 0.0, total, pp, w=w)
    out = torch.zeros_like(eager.u)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        parcel.run_parcel(IC, 0.0, total, pp, w=w, out=out)        # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        parcel.run_parcel(IC, 0.0, total, pp, w=w, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager.u)
