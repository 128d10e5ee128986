"""HIP-event times of cmx_parcel_run_* (the parcel model integrated inside one kernel, one parcel per lane), alternating in one process (warm-up first;
median of ROUNDS rounds), for an ensemble of n parcels × n_steps forward-Euler steps, f32 and f64, two option sets:
  * every option "None" (the dry adiabat: the thermodynamics of a step alone);
  * ABIFM on Illite + Condensation + Deposition (the configuration of parcel/Example_Immersion_Freezing.jl).
The state and output buffers are allocated once, outside the timed region; no trajectory.  Prints ms per call, ns per parcel-step, the time of ONE launch
of CMX_PARCEL_MAX_STEPS_PER_LAUNCH steps (the call splits n_steps into such launches) and, for scale, the time the same state traffic would take at
8 TB/s: the kernel reads 10 and writes 9 columns once per launch, so anything above that is arithmetic.
    python tools/time_parcel.py [n_parcels] [n_steps]"""
import statistics
import sys
import warnings
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
for p in (REPO / "cloudmicrophysics.jl_amd", REPO / "tests"):
    sys.path.insert(0, str(p))
from cmx import parameters as P  # noqa: E402
from cmx import parcel  # noqa: E402
import parcel_ref as R  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 600
ROUNDS, PEAK = 5, 8e12
dev = torch.device("cuda", 0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cases = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore", P.UnpinnedParameterWarning)
    for ft, dt in (("f32", torch.float32), ("f64", torch.float64)):
        for name, kw in (("all None", {}),
                         ("ABIFM + Condensation + Deposition", dict(heterogeneous="ABIFM", condensation_growth="Condensation", deposition_growth="Deposition",
                                                                   aerosol=parcel.Aerosol(abifm=P.Illite(ft))))):
            pp = parcel.parcel_params(ft, **kw)
            prm = R.parameters(pp.c)
            Y0, w = R.ensemble(N, 1, prm["tps"], prm["rho_w"])      # the draws of the test ensembles: T₀ ~ U(243, 258), w ~ U(0.1, 2), 1-µm droplets
            IC = [torch.from_numpy(np.asarray(c)).to(dt).to(dev) for c in Y0] + [0.0]
            wd = torch.from_numpy(w).to(dt).to(dev)
            out = torch.empty((10, N), dtype=dt, device=dev)
            cases[f"parcel_run {ft} {name}"] = (lambda IC=IC, wd=wd, out=out, pp=pp: parcel.run_parcel(IC, 0.0, STEPS * float(pp.c.const_dt), pp, w=wd, out=out),
                                                IC[0].element_size())
for fn, _ in cases.values():                # warm-up
    fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(ROUNDS):                     # alternating: every case once per round
    for k, (fn, _) in cases.items():
        times[k].append(timed(fn))
cap = parcel.MAX_STEPS_PER_LAUNCH
print(f"{'case':<52} {'parcels':>9} {'steps':>6} {'ms':>9} {'ns/parcel-step':>15} {f'ms per {cap}-step launch':>24} {'state traffic at 8 TB/s, ms':>28}")
for k, (_, e) in cases.items():
    ms = statistics.median(times[k])
    launches = max(1, -(-STEPS // cap))
    traffic = launches * N * 19 * e / PEAK * 1e3
    print(f"{k:<52} {N:>9d} {STEPS:>6d} {ms:>9.3f} {ms * 1e6 / (N * STEPS):>15.4f} {ms * min(cap, STEPS) / STEPS:>24.3f} {traffic:>28.4f}")
