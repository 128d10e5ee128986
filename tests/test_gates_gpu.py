"""The gates at and around their thresholds (tests/gate_cases.py) on the device (-m gpu), both float types, through
cmx_sb2006_process_rates_*, cmx_sb2006_warm_rain_tendencies_* (SB2006 fall speeds), cmx_bulk_2m_cloud_to_rain_*, cmx_mp1m_source_terms_* /
cmx_mp1m_tendencies_* and cmx_sb2006_precip_susceptibility_*.

Every ladder is launched twice — as it is (16-byte aligned columns: the vector body and its tail) and as `[1:]` of a buffer one element longer (the
one-point-per-lane path) — and the two results must agree in every bit.  Raw gates: all 17 rungs, nothing set aside.  Computed gates: 4097 rungs, the
ordinary bound and the reference's side outside the margin, "finite and on one of the two branches" inside.  The printed rows (the side at each exact
threshold, the rungs at which the device's side differs from the reference's) are the measured values DESIGN §6 quotes."""
import pytest
import torch

import gate_cases as G
from cmx import _abi
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FAMILIES = list(G.COLUMNS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _launch(case, cols):
    """one call of the case's entry on device columns → {output name: tensor}"""
    import cmx
    ft = case.ft
    x = [cols[k] for k in G.COLUMNS[case.family]]
    tps = P.ThermodynamicsParameters(ft)
    if case.family == "sb_proc":
        r = cmx.sb2006_process_rates(P.Microphysics2MParams(ft, is_limited=case.limited), tps, *x)
        return {k: getattr(r, k) for k in _abi.SB2006_PROCESS_COLUMNS}
    if case.family == "sb_fused":
        r = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), P.Microphysics2MParams(ft, is_limited=case.limited), tps, *x, vel=cmx.SB2006VelType)
        return {k: getattr(r, k) for k in ("dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "vt_rai_n", "vt_rai_m")}
    if case.family == "bulk2m":
        return {"acnv": cmx.bulk_2m_cloud_to_rain(P.Bulk2MSchemes(ft), "LD2004", cols["q_lcl"], cols["rho"], N_d=cols["N_d"]).acnv}
    if case.family == "mp1m":
        mp = P.Microphysics1MParams(ft, **G.MP1M_OPTIONS[case.optset])
        t = cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *x)
        s = cmx.microphysics_source_terms_1m(mp, tps, *x)
        return {**{k: getattr(t, k) for k in G.TENDENCIES_1M}, **{k: getattr(s, k) for k in _abi.MP1M_SOURCE_COLUMNS}}
    r = cmx.precipitation_susceptibilities(P.SB2006(ft), *x)
    f = {"d_ln_q_lcl": "d_ln_pp_d_ln_q_lcl", "d_ln_q_rai": "d_ln_pp_d_ln_q_rai", "d_ln_N_lcl": "d_ln_pp_d_ln_N_lcl"}
    return {f"{p}_{k}": getattr(side, name) for p, side in (("acnv", r.autoconversion), ("accr", r.accretion)) for k, name in f.items()}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def device_run(dev):
    def run(case, cols):
        aligned = {k: torch.tensor(v, dtype=DT[case.ft], device=dev) for k, v in cols.items()}
        assert all(t.data_ptr() % 16 == 0 for t in aligned.values())
        shifted = {}
        for k, t in aligned.items():
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
            buf[1:] = t
            shifted[k] = buf[1:]
            assert shifted[k].data_ptr() % 16 != 0
        a, b = _launch(case, aligned), _launch(case, shifted)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (case.name, k, "the vector body and the one-point-per-lane path differ")
        return {k: v.cpu().numpy() for k, v in a.items()}
    return run


def _checked(case, got, ref, failures):
    """the checker's verdict; a failure is collected so that one run reports every ladder that fails"""
    try:
        return G.check(case, got, ref)
    except AssertionError as e:
        failures.append(str(e))
        return "FAILED"


@pytest.mark.parametrize("ft", ["f32", "f64"])
@pytest.mark.parametrize("family", FAMILIES)
def test_raw_gates_take_the_reference_side_at_every_rung(dev, oracle, family, ft):
    run = device_run(dev)
    rows, failures = [], []
    for case in (c for c in G.raw_cases(ft) if c.family == family):
        ref = G.reference(oracle, case)
        side = _checked(case, run(case, case.columns()), ref, failures)
        if case.watch:
            rows.append(f"{case.name}: {case.predicate}: {side} at the threshold")
            if side != ("open" if case.open_at_exact else "closed") and side != "FAILED":
                failures.append(f"{case.name}: {side} at the threshold")
    if rows:
        print(f"\n[gates, device, raw] {ft} {family}:\n  " + "\n  ".join(rows))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_computed_gates_stay_on_one_of_the_two_branches(dev, oracle, ft):
    run = device_run(dev)
    rows, failures = [], []
    for case, thr in G.computed_cases(oracle, ft):
        ref = G.reference(oracle, case, threshold=thr)
        m0, m1, _ = G._segments(case, ref)
        window = _checked(case, run(case, case.columns()), ref, failures)
        rows.append(f"{case.name}: stride {case.stride} ulp, margin rungs {m0 - case.half:+d} … {m1 - case.half:+d}, "
                    f"device side differs from the reference's at rungs {window}")
    assert len(rows) == 6
    print(f"\n[gates, device, computed] {ft}:\n  " + "\n  ".join(rows))
    assert not failures, "\n".join(failures)
