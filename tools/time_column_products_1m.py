"""HIP-event times of the products with the Jacobian of the 1-moment column step — cmx_mp1m_column_jvp_* WITH the tendencies and the precipitation fluxes
(what a Newton–Krylov iteration asks for), cmx_mp1m_column_vjp_* for all six gradients with every cotangent — beside the primal column entry
(cmx_mp1m_column_tendencies_sedimentation_*, nsub = 0) of the SAME build on the same box and the same columns.  Columns of 64 levels, states of
tools/time_jacobian.py, both float types; every output is allocated once, outside the timed region, and the entries are called through the raw ABI.  All
cases alternate in one session (every case once per round, the median of the rounds); the session is repeated `--runs` times and the spread of the medians
printed.  CMX_LIB selects another build (another K of the Jᵀḡ kernel: -DCMX_COL1M_VJP_K_F32=…).
    python tools/time_column_products_1m.py [--runs 3] [--levels 64] [n_points …]          (default 1e6)"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402
import cmx  # noqa: E402
from cmx import _abi, _lib  # noqa: E402
from cmx import parameters as P  # noqa: E402

DT = TJ.DT


def cases_of(ft, n_col, n_lev, dev):
    n = n_col * n_lev
    cols = [c.to(DT[ft]).to(dev).reshape(n_col, n_lev).contiguous() for c in TJ.states_mp1m(n)]
    mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    stokes, cr, ci = P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft)
    fam = _abi.F32 if ft == "f32" else _abi.F64
    inv_dz = (1.0 / torch.linspace(40.0, 400.0, n_lev, dtype=torch.float64)).to(DT[ft]).to(dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda shape: (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(DT[ft]).to(dev)  # noqa: E731
    v = [c * rnd((n_col, n_lev)) for c in cols[1:]]
    gbar, pbar = [rnd((n_col, n_lev)) for _ in range(4)], [rnd((n_col,)) for _ in range(2)]
    mk = lambda k: torch.empty((k, n_col, n_lev), dtype=DT[ft], device=dev)  # noqa: E731
    oy, ot, og = mk(4), mk(4), mk(6)
    op, opp = torch.empty((2, n_col), dtype=DT[ft], device=dev), torch.empty((2, n_col), dtype=DT[ft], device=dev)
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    params = (C.byref(mp.c), C.byref(tps), C.byref(stokes), C.byref(cr), C.byref(ci), mp.flags)
    tail = (n_col, n_lev, ptr(inv_dz), tab(cols))
    keep = (mp, tps, stokes, cr, ci, cols, v, gbar, pbar, oy, ot, og, op, opp, inv_dz)

    def primal():
        _lib.call("cmx_mp1m_column_tendencies_sedimentation", fam, dev, *params, 0.0, 0.0, 0, *tail, tab(list(ot)), ptr(op[0]), ptr(op[1]))

    def jvp():
        _lib.call("cmx_mp1m_column_jvp", fam, dev, *params, *tail, tab(v), tab(list(oy)), ptr(opp[0]), ptr(opp[1]), tab(list(ot)), ptr(op[0]), ptr(op[1]))

    def vjp():
        _lib.call("cmx_mp1m_column_vjp", fam, dev, *params, *tail, tab(gbar), ptr(pbar[0]), ptr(pbar[1]), tab(list(og)), None, None, None)
    return {f"{ft} primal column step": primal, f"{ft} J v with tendencies": jvp, f"{ft} Jᵀḡ, six gradients": vjp}, keep


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--levels", type=int, default=64)
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}")
    for n in args.sizes or [1_000_000]:
        n_col = n // args.levels
        cases, keep = {}, []
        for ft in ("f32", "f64"):
            c, k = cases_of(ft, n_col, args.levels, dev)
            cases.update(c)
            keep.append(k)
        for fn in cases.values():                   # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in cases}
        for _ in range(args.runs):
            times = {k: [] for k in cases}
            for _ in range(TJ.ROUNDS):              # alternating: every case once per round
                for k, fn in cases.items():
                    times[k].append(TJ.timed(fn))
            for k, t in times.items():
                runs[k].append(statistics.median(t))
        print(f"{'case':<32} {'points':>10} {'levels':>6} {'ms (median of the runs)':>24} {'runs, ms':>30} {'vs primal':>9}")
        for k, r in runs.items():
            base = statistics.median(runs[f"{k[:3]} primal column step"])
            print(f"{k:<32} {n_col * args.levels:>10d} {args.levels:>6d} {statistics.median(r):>24.3f} {' '.join(f'{t:.3f}' for t in r):>30} {statistics.median(r) / base:>9.2f}",
                  flush=True)


if __name__ == "__main__":
    main()
