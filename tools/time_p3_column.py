"""HIP-event times of the 2M + P3 column step (cmx_mp2m_p3_column_tendencies_sedimentation_*) against the sequence of calls it replaces, alternating
in one process (warm-up first; median of ROUNDS rounds), Float32 and Float64, quadrature order 16, n_col columns of n_lev levels of the mixed-phase
states of tests/p3_column_ref.py.  The sequence is what a host model does today, with the library's own entries:
  1. ρ·(q_ice, n_ice, q_rim, b_rim) in torch, cmx_p3_shape_terminal_velocities               (log λ, v_n, v_m)
  2. cmx_microphysics_2m_p3_tendencies with that log λ (non-finite → 0 in torch)             (the eight tendencies)
  3. cmx_sb2006_warm_rain_tendencies with velocities                                          (the rain fall speeds)
  4. the first-order upwind flux divergence of the six falling species in torch
Prints ms per call for both, their ratio, the sequence's four stages (events between them), and whether the two results agree (log λ and the ice
speeds bit for bit, the tendencies within the rounding bound of tests/test_mp2m_p3_column_gpu.py) at the size that was timed.
    python tools/time_p3_column.py [n_col] [n_lev]"""
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO / "cloudmicrophysics.jl_amd", REPO / "tests"):
    sys.path.insert(0, str(p))
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402
import p3_column_ref as R  # noqa: E402

N_COL = int(float(sys.argv[1])) if len(sys.argv) > 1 else 27_027       # × 74 levels = 2.0e6 states: 10–100 ms per call of a compute-bound pass
N_LEV = int(sys.argv[2]) if len(sys.argv) > 2 else 74
ROUNDS = 7
dev = torch.device("cuda", 0)
SPECIES = (("dq_rai_dt", "q_rai", "w_m"), ("dn_rai_dt", "n_rai", "w_n"), ("dq_ice_dt", "q_ice", "v_m"), ("dn_ice_dt", "n_ice", "v_n"),
           ("dq_rim_dt", "q_rim", "v_m"), ("db_rim_dt", "b_rim", "v_m"))


def make(ft, dt):
    s = R.states(N_COL, N_LEV, seed=19, f32_safe=(ft == "f32"))
    d = {k: torch.from_numpy(v).to(dt).to(dev) for k, v in s.items()}
    dz = torch.from_numpy(R.inv_dz(N_LEV, seed=1)).to(dt).to(dev)
    mp, warm, tps = P.Microphysics2MParams(ft, with_ice=True), P.Microphysics2MParams(ft), P.ThermodynamicsParameters(ft)
    p3, vel_ice = P.ParametersP3(ft), P.Chen2022VelTypeIce(ft)
    cols = [d[k] for k in R.IN_NAMES]
    flat = [c.reshape(-1) for c in cols]
    out = cmx.ColumnTendencies2MP3(*[torch.empty_like(d["rho"]) for _ in range(11)], None, None)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def fused():
        return cmx.column_tendencies_sedimentation_2m_p3(mp, tps, dz, *cols, vel=cmx.SB2006VelType, out=out)

    def sequence():
        marks[0].record()
        rho = flat[0]
        sv = cmx.p3_shape_and_terminal_velocities(p3, vel_ice, rho, rho * flat[7], rho * flat[8], rho * flat[9], rho * flat[10], quad=mp.ice.c.quad)
        marks[1].record()
        ll0 = torch.where(torch.isfinite(sv.log_lambda), sv.log_lambda, torch.zeros_like(sv.log_lambda))
        pt = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *flat, ll0)
        marks[2].record()
        wr = cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), warm, tps, *flat[:7], vel=cmx.SB2006VelType)
        marks[3].record()
        sh = d["rho"].shape
        cl = {k: torch.clamp(d[k], min=0) for k in ("rho", "q_rai", "n_rai", "q_ice", "n_ice", "q_rim", "b_rim")}
        w = {"w_n": wr.vt_rai_n.reshape(sh), "w_m": wr.vt_rai_m.reshape(sh), "v_n": sv.v_n.reshape(sh), "v_m": sv.v_m.reshape(sh)}
        g = dz[None, :] / cl["rho"]
        res = {"dq_lcl_dt": pt.dq_lcl_dt.reshape(sh), "dn_lcl_dt": pt.dn_lcl_dt.reshape(sh)}
        bound = {}
        for name, chi, speed in SPECIES:
            F = (cl["rho"] * cl[chi]) * w[speed]
            up = torch.cat([F[:, 1:], torch.zeros_like(F[:, :1])], dim=1)
            tend = getattr(pt, name).reshape(sh)
            res[name] = tend + (up - F) * g
            bound[name] = tend.abs() + (up + F) * g
        marks[4].record()
        return res, bound, sv

    return fused, sequence, marks


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cases = {ft: make(ft, dt) for ft, dt in (("f32", torch.float32), ("f64", torch.float64))}
agree = {}
for ft, (fused, sequence, _) in cases.items():        # warm-up, and the comparison of the two results
    got = fused()
    res, bound, sv = sequence()
    torch.cuda.synchronize()
    eps = torch.finfo(got.log_lambda.dtype).eps * (8 if ft == "f32" else 64)
    same = all(torch.equal(a.reshape(-1).view(torch.uint8), b.view(torch.uint8)) for a, b in ((got.log_lambda, sv.log_lambda), (got.v_ice_n, sv.v_n), (got.v_ice_m, sv.v_m)))
    same &= torch.equal(got.dq_lcl_dt, res["dq_lcl_dt"]) and torch.equal(got.dn_lcl_dt, res["dn_lcl_dt"])
    worst = max(float(((getattr(got, k) - res[k]).abs() / (eps * bound[k] + torch.finfo(got.log_lambda.dtype).tiny)).max()) for k, _, _ in SPECIES)
    agree[ft] = (same, worst)
    del res, bound, sv
times = {(ft, k): [] for ft in cases for k in ("fused", "sequence")}
stages = {ft: [[] for _ in range(4)] for ft in cases}
for _ in range(ROUNDS):                                # alternating: every case once per round
    for ft, (fused, sequence, marks) in cases.items():
        times[(ft, "fused")].append(timed(fused))
        times[(ft, "sequence")].append(timed(sequence))
        for j in range(4):
            stages[ft][j].append(marks[j].elapsed_time(marks[j + 1]))
n = N_COL * N_LEV
print(f"{n} states ({N_COL} columns x {N_LEV} levels), quadrature order 16, SB2006 rain fall speeds, median of {ROUNDS} alternating rounds")
print(f"{'ft':<4} {'one call, ms':>13} {'sequence, ms':>13} {'call/sequence':>14}   sequence stages, ms: shape+speeds | 2M+P3 tendencies | rain speeds | divergence (torch)")
for ft in cases:
    a, b = statistics.median(times[(ft, "fused")]), statistics.median(times[(ft, "sequence")])
    st = [statistics.median(x) for x in stages[ft]]
    print(f"{ft:<4} {a:>13.3f} {b:>13.3f} {a / b:>14.3f}   {st[0]:.3f} | {st[1]:.3f} | {st[2]:.3f} | {st[3]:.3f}"
          f"   spread of the call {min(times[(ft, 'fused')]):.3f}-{max(times[(ft, 'fused')]):.3f}, of the sequence {min(times[(ft, 'sequence')]):.3f}-{max(times[(ft, 'sequence')]):.3f}")
    print(f"     results agree: log λ / ice speeds / non-sedimenting columns bit for bit = {agree[ft][0]}, sedimenting columns worst error / rounding bound = {agree[ft][1]:.3f}")
