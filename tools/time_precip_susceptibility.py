"""HIP-event times of cmx_sb2006_precip_susceptibility_*, alternating in one process (warm-up first; median of ROUNDS rounds of REPS calls each), at
1e8 points, f32 and f64:
  * the fused call, all six outputs (4 columns in, 6 out: 40 B/point in f32);
  * autoconversion only (4 in, 3 out: 28 B/point in f32).
The outputs are allocated once, outside the timed region.  Prints ms per call, bytes per point and the fraction of 8 TB/s on the algorithmic bytes.
`tools/stream_probe … shapes` times bare copies of the same column counts (4r/6w, 4r/3w) for comparison on the same box.
    python tools/time_precip_susceptibility.py [n_points]"""
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "cloudmicrophysics.jl_amd"))
from cmx import _lib  # noqa: E402
from cmx import parameters as P  # noqa: E402
from cmx._cols import _fam_of, _ptr  # noqa: E402

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
ROUNDS, REPS, PEAK = 7, 10, 8e12
dev = torch.device("cuda", 0)


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


def call(sb, cols, outs, n_acnv, n_accr):
    o = [_ptr(t) for t in outs[:n_acnv]] + [None] * (3 - n_acnv) + [_ptr(t) for t in outs[3:3 + n_accr]] + [None] * (3 - n_accr)
    _lib.call("cmx_sb2006_precip_susceptibility", _fam_of(cols[0]), dev, C.byref(sb.acnv) if n_acnv else None, C.byref(sb.accr) if n_accr else None,
              cols[0].numel(), *[_ptr(c) for c in cols], *o)


cases = {}
for ft, dt in (("f32", torch.float32), ("f64", torch.float64)):
    g = torch.Generator(device="cpu").manual_seed(1)
    # cloudy states: q_lcl, q_rai log-uniform over [1e-9, 5e-3], ρ over [0.3, 1.3], N_lcl log-uniform over [1e6, 3e9]
    cols = (lu(g, -9, -2.3, dt), lu(g, -9, -2.3, dt), (0.3 + torch.rand(N, generator=g, dtype=torch.float64)).to(dt).to(dev), lu(g, 6, 9.5, dt))
    outs = [torch.empty_like(cols[0]) for _ in range(6)]
    sb = P.SB2006(ft)
    e = cols[0].element_size()
    cases[f"sb2006_precip_susceptibility {ft} fused (6 outputs)"] = ((lambda sb=sb, cols=cols, outs=outs: call(sb, cols, outs, 3, 3)), 10 * e)
    cases[f"sb2006_precip_susceptibility {ft} autoconversion only"] = ((lambda sb=sb, cols=cols, outs=outs: call(sb, cols, outs, 3, 0)), 7 * e)
for k, (fn, _) in cases.items():            # warm-up
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(ROUNDS):                     # alternating: every case once per round
    for k, (fn, _) in cases.items():
        times[k].append(timed(fn))
print(f"{'case':<58} {'points':>11} {'ms':>8} {'B/point':>8} {'TB/s':>6} {'of 8 TB/s':>9}")
for k, (_, bpp) in cases.items():
    ms = statistics.median(times[k])
    tbs = N * bpp / (ms * 1e-3) / 1e12
    print(f"{k:<58} {N:>11d} {ms:>8.3f} {bpp:>8d} {tbs:>6.2f} {tbs * 1e12 / PEAK:>9.3f}")
