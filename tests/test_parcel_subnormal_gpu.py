"""Float32 parcel states whose droplet or crystal number and content lie in the subnormal range (cmx_parcel.hpp parcel_quot, parcel_cbrt).

Freezing that takes a fixed share of N_liq per step (dN = −J A N) walks N_liq down through the subnormal range of Float32 before it reaches zero: parcel
2763 of the abifm_cond_dep_mono ensemble is there after 146 steps (N_liq = 9.9e-39, q_liq = 3.7e-43).  The hardware reciprocal and logarithm read a
subnormal operand as zero, so q·rcp(N) was Inf where the reference's q/N is 3.7e-5, the droplet radius was Inf, condensation took all the vapour in
one step and the parcel ended as Inf·0 = NaN, while the restatement stays finite in both float types.

The bound.  The tendencies are compared with the Float64 restatement on the Float32 inputs by the rule of tests/test_parcel_gpu.py,
|x − ref| ≤ 1e-3·max(|ref|, Σ|terms|), plus one absolute term that rule has no need of at ordinary states: eps(Float32)·scale/const_dt with the scale
of the run comparison (S_l, p, T their own magnitude, q on q_tot, N on N_aer + N_liq + N_ice).  A tendency error below it moves the state by less than
one rounding of the state variable per step, so it cannot change a run; it is there because a subnormal carries an absolute rounding of 2^-149 rather
than a relative one, so a term such as N_liq·dq/q_liq of subnormal operands has no relative accuracy at all, in the reference's Float32 arithmetic as
little as here.  Every such term is at least 30 orders of magnitude below that allowance; the fault this file guards against exceeded it by 10^7.
"""
import numpy as np
import pytest
import torch

import parcel_cases as PC
import parcel_ref as R
from cmx import parcel

pytestmark = pytest.mark.gpu

CASES = ["abifm_cond_dep_mono", "abifm_cond_dep_gamma"]
N_PROC = {"dN_liq_act": True, "dN_ice_dep": True, "dN_ice_imm": True, "dN_ice_hom": True, "dq_liq_ce": False, "dq_ice_ds": False}


def subnormal_states():
    """Nine Float32 columns and w.  Row 0 is the state found in the ensemble; the others put q, N or both of one species below floatmin(Float32) =
    1.2e-38, with S_l above and below saturation (growth, and the number sink of an evaporating content below 1e-6), next to ordinary neighbours.
    Where the number sink acts (S_l < 1) the mean particle mass q/N is kept representable: below floatmin the radius is zero in any Float32 arithmetic,
    the restatement's included, and the sink with it, which no Float64 yardstick can follow."""
    rows = [
        # S_l,      p_air,      T,          q_vap,        q_liq,    q_ice,     N_aer, N_liq,     N_ice
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 3.67e-43, 3.0555e-7, 0.0, 9.8635e-39, 4387.229),
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 1.0e-10, 3.0555e-7, 0.0, 1.0e-40, 4387.229),      # q/N = 1e30: large, finite
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 1.0e-41, 3.0555e-7, 0.0, 1.0e-39, 4387.229),
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 1.0e-12, 3.0555e-7, 0.0, 3.0e-38, 4387.229),      # N just above floatmin
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 1.0e-44, 3.0555e-7, 0.0, 2.0e3, 4387.229),        # q subnormal, N ordinary
        (0.97, 88866.1328, 243.259903, 3.5e-4, 3.67e-43, 3.0555e-7, 0.0, 9.8635e-39, 4387.229),             # evaporating: the sink divides by q_liq
        (0.97, 88866.1328, 243.259903, 3.5e-4, 1.0e-41, 3.0555e-7, 0.0, 1.0e-36, 4387.229),             # q subnormal, N small and normal
        (0.70, 70000.0, 250.0, 4.0e-4, 1.0e-9, 1.0e-42, 0.0, 1.0e3, 1.0e-39),                               # subliming: the sink divides by q_ice
        (0.70, 70000.0, 250.0, 4.0e-4, 1.0e-9, 2.0e-40, 0.0, 1.0e3, 4.0e-41),
        (1.02, 70000.0, 250.0, 6.0e-4, 1.0e-9, 1.0e-42, 0.0, 1.0e3, 1.0e-39),                               # growing crystals
        (1.0331762, 88866.1328, 243.259903, 3.7284664e-4, 2.0e-8, 3.0555e-7, 0.0, 3.0e3, 4387.229),         # an ordinary neighbour
    ]
    cols = [np.array(c, dtype=np.float32) for c in zip(*rows)]
    assert all(np.any((c > 0) & (c < np.finfo(np.float32).tiny)) for c in (cols[4], cols[5], cols[7], cols[8]))
    return cols, np.full(len(rows), 0.14, dtype=np.float32)


@pytest.mark.parametrize("case", CASES)
def test_tendencies_at_subnormal_number_and_content(case):
    kw = PC.RUN_CASES[case]["kw"]
    pp, prm = PC.build("f32", **kw)
    Y, w = subnormal_states()
    ref = R.rhs(np.float64, prm, PC.ref_options(kw), Y, w, margin=PC.MARGIN["f32"])
    assert not ref["near_gate"].any()
    dev = torch.device("cuda:0")
    out = parcel.parcel_tendencies([torch.from_numpy(c).to(dev) for c in Y], pp, w=torch.from_numpy(w).to(dev))
    torch.cuda.synchronize()
    Y64 = [c.astype(np.float64) for c in Y]
    q_tot, N_tot = Y64[3] + Y64[4] + Y64[5], Y64[6] + Y64[7] + Y64[8]
    step = np.finfo(np.float32).eps / prm["const_dt"]
    state_scale = [np.abs(Y64[0]), np.abs(Y64[1]), np.abs(Y64[2])] + [q_tot] * 3 + [N_tot] * 3
    rows = [(R.STATE[j], out.dY[j].cpu().numpy(), ref["dY"][j], ref["scale"][j], state_scale[j]) for j in range(9)] + \
           [(k, out.process_rates[k].cpu().numpy(), ref["proc"][k], ref["proc_scale"][k], N_tot if is_n else q_tot) for k, is_n in N_PROC.items()]
    for name, x, r, sc, ss in rows:
        x, r = x.astype(np.float64), np.asarray(r, dtype=np.float64)
        assert np.all(np.isfinite(r)), name                     # the restatement is finite at every one of these states
        allowed = PC.RTOL["f32"] * np.maximum(np.abs(r), sc) + step * ss
        print(f"{case} {name}: device {x} restatement {r} allowed {allowed}")
        assert np.all(np.isfinite(x)), (name, x)
        assert np.all(np.abs(x - r) <= allowed), (name, x, r, allowed)


def test_run_through_the_subnormal_range_stays_finite():
    """The recurrence from these states on: N_liq goes on decaying to zero through the subnormal range.  Finite after every step wherever the Float32
    restatement is finite; a state already in the subnormal range is exactly what a split run (a + b steps) hands to its second launch."""
    case = "abifm_cond_dep_mono"
    kw = PC.RUN_CASES[case]["kw"]
    pp, prm = PC.build("f32", **kw)
    Y, w = subnormal_states()
    steps = 40
    with np.errstate(all="ignore"):
        ref = R.run(np.float32, prm, PC.ref_options(kw), Y, w, steps, save_every=1)
    fin = np.isfinite(ref["trajectory"]).all(axis=(0, 1))
    assert fin.all()                                            # the restatement itself stays finite for every one of them
    dev = torch.device("cuda:0")
    sol = parcel.run_parcel([torch.from_numpy(c).to(dev) for c in Y] + [0.0], 0.0, steps * prm["const_dt"], pp, w=torch.from_numpy(w).to(dev), save_every=1)
    torch.cuda.synchronize()
    got = np.isfinite(sol.trajectory[:, :9].cpu().numpy()).all(axis=(0, 1))
    print("finite: restatement", fin, "device", got)
    assert got.all()
