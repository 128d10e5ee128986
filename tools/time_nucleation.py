"""HIP-event times of the nucleation entries, alternating in one process (warm-up first; median of ROUNDS rounds of REPS calls each), at 1e8 points:
  * cmx_aerosol_nucleation_rates_* f32 and f64, all four outputs (8 columns in, 4 out) and binary + ternary only (4 in, 2 out);
  * cmx_apparent_nucleation_rate_* f32 and f64 (6 in, 1 out);
  * cmx_p3_ice_nucleation_counts_* f32 and f64, both outputs (4 in, 2 out).
Prints ms per call, bytes per point and the fraction of 8 TB/s.
    python tools/time_nucleation.py [n_points]"""
import statistics
import sys
import warnings
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "cloudmicrophysics.jl_amd"))
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ROUNDS, REPS, PEAK = 7, 10, 8e12
dev = torch.device("cuda", 0)
warnings.simplefilter("ignore", P.UnpinnedParameterWarning)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def lu(g, lo, hi, dt):      # log-uniform column on the device
    return (10.0 ** (lo + (hi - lo) * torch.rand(N, generator=g, dtype=torch.float64))).to(dt).to(dev)


cases = {}
for ft, dt in (("f32", torch.float32), ("f64", torch.float64)):
    g = torch.Generator(device="cpu").manual_seed(1)
    c = dict(h2so4=lu(g, 8, 16, dt), nh3=lu(g, 8, 18, dt), negative_ion=lu(g, 6, 10, dt), monoterpene=lu(g, 12, 18, dt), O3=lu(g, 16, 19, dt),
             OH=lu(g, 9, 14, dt), temp=(190 + 130 * torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev), condensation_sink=lu(g, -5, -1, dt))
    hp, op, mp = P.H2S04NucleationParameters(ft), P.OrganicNucleationParameters(ft), P.MixedNucleationParameters(ft)
    e = c["temp"].element_size()
    cases[f"aerosol_nucleation_rates {ft} all four"] = ((lambda c=c, hp=hp, op=op, mp=mp: cmx.nucleation_rates(hp, op, mp, **c)), 12 * e)
    cases[f"aerosol_nucleation_rates {ft} binary+ternary"] = ((lambda c=c, hp=hp: cmx.nucleation_rates(
        hp, h2so4=c["h2so4"], nh3=c["nh3"], negative_ion=c["negative_ion"], temp=c["temp"], want=("binary", "ternary"))), 6 * e)
    od, idd = (2 + 18 * torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev), (1 + torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev)
    ap = (od, lu(g, 0, 8, dt), lu(g, -2, 1, dt), lu(g, -5, -2, dt), lu(g, -4, -1, dt), idd)
    cases[f"apparent_nucleation_rate {ft}"] = ((lambda ap=ap: cmx.apparent_nucleation_rate(*ap)), 7 * e)
    ip = P.MorrisonMilbrandt2014(ft)
    p3 = (c["temp"], lu(g, 6, 9, dt), lu(g, -18, -12, dt), (1 + 299 * torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev))
    from cmx.ice_nucleation import _p3_counts
    cases[f"p3_ice_nucleation_counts {ft} N_dep+N_het"] = ((lambda ip=ip, p3=p3: _p3_counts(ip, *p3, True, True, None)), 6 * e)
for k, (fn, _) in cases.items():            # warm-up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(ROUNDS):                     # alternating: every case once per round
    for k, (fn, _) in cases.items():
        times[k].append(timed(fn))
print(f"{'case':<52} {'points':>11} {'ms':>8} {'B/point':>8} {'TB/s':>6} {'of 8 TB/s':>9}")
for k, (_, bpp) in cases.items():
    ms = statistics.median(times[k])
    tbs = N * bpp / (ms * 1e-3) / 1e12
    print(f"{k:<52} {N:>11d} {ms:>8.3f} {bpp:>8d} {tbs:>6.2f} {tbs * 1e12 / PEAK:>9.3f}")
