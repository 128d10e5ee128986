"""HIP-event times and peak extra memory of the fused products with the Jacobian — cmx.warm_rain_vjp_2m / warm_rain_jvp_2m, cmx.vjp_1m / jvp_1m — against what
a caller does without them: the full Jacobian entry followed by torch.einsum with ḡ (Jᵀḡ) or with v (J v).  Both schemes and both float types alternate in
ONE session on one box (every case once per round, the median of the rounds); states are those of tools/time_jacobian.py.  Outputs of the fused entries are
allocated once, outside the timed region; the two-pass way allocates its 24 columns and the einsum result inside it, as a caller's does.  The last column is the Jacobian entry alone, 24 preallocated columns, no contraction: the first of
the two passes.  Peak extra memory: torch.cuda.max_memory_allocated over one call, above what is allocated before it,
with NO output preallocated in either way.
    python tools/time_jacobian_products.py [n_points …]          (default 1e7)"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import time_jacobian as TJ  # noqa: E402
import cmx  # noqa: E402
from cmx import parameters as P  # noqa: E402

DT = TJ.DT


def scheme(name, ft, n, dev):
    """(state columns, jacobian, vjp, jvp) of a scheme on n states"""
    if name == "sb2006":
        cols = [c.to(DT[ft]).to(dev) for c in TJ.states_sb2006(n)]
        mp, tps = P.WarmRainParams2M(ft, True), P.ThermodynamicsParameters(ft)
        return (cols, lambda **kw: cmx.warm_rain_jacobian_2m(mp, tps, *cols, **kw), lambda g, **kw: cmx.warm_rain_vjp_2m(mp, tps, *cols, g, **kw),
                lambda v, **kw: cmx.warm_rain_jvp_2m(mp, tps, *cols, dict(zip(cmx.JACOBIAN_WRT, v)), **kw))
    cols = [c.to(DT[ft]).to(dev) for c in TJ.states_mp1m(n)]
    mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    return (cols, lambda **kw: cmx.jacobian_1m(mp, tps, *cols, **kw), lambda g, **kw: cmx.vjp_1m(mp, tps, *cols, g, **kw),
            lambda v, **kw: cmx.jvp_1m(mp, tps, *cols, dict(zip(cmx.JACOBIAN_WRT_1M, v)), **kw))


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return peak


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("sizes", nargs="*", type=lambda a: int(float(a)))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(f"library: {cmx._lib.LIB_PATH}")
    for n in args.sizes or [10_000_000]:
        cases, memory = {}, {}
        for name in ("sb2006", "mp1m"):
            for ft in ("f32", "f64"):
                cols, jacobian, vjp, jvp = scheme(name, ft, n, dev)
                g = torch.Generator(device="cpu").manual_seed(3)
                gbar = torch.stack([(torch.rand(n, generator=g, dtype=torch.float64) - 0.5).to(DT[ft]).to(dev) for _ in range(4)])
                v = torch.stack([(c * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5).to(DT[ft]).to(dev)) for c in cols[1:]])
                og, oy = torch.empty((6, n), dtype=DT[ft], device=dev), torch.empty((4, n), dtype=DT[ft], device=dev)
                key = f"{name} {ft}"
                cases[f"{key} vjp fused"] = lambda f=vjp, c=list(gbar), o=(og, None): f(c, out=o)
                cases[f"{key} jvp fused"] = lambda f=jvp, c=list(v), o=(oy, None): f(c, out=o)
                cases[f"{key} vjp jacobian + einsum"] = lambda j=jacobian, c=gbar: torch.einsum("ojn,on->jn", j().jac, c)
                cases[f"{key} jvp jacobian + einsum"] = lambda j=jacobian, c=v: torch.einsum("ojn,jn->on", j().jac, c)
                jalone = torch.empty((4, 6, n), dtype=DT[ft], device=dev)
                cases[f"{key} jacobian alone"] = lambda j=jacobian, J=jalone: j(out=(J, None))
                memory[f"{key} vjp fused"] = lambda f=vjp, c=list(gbar): f(c)
                memory[f"{key} jvp fused"] = lambda f=jvp, c=list(v): f(c)
                memory[f"{key} vjp jacobian + einsum"] = lambda j=jacobian, c=gbar: torch.einsum("ojn,on->jn", j().jac, c)
                memory[f"{key} jvp jacobian + einsum"] = lambda j=jacobian, c=v: torch.einsum("ojn,jn->on", j().jac, c)
        for fn in cases.values():                   # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(TJ.ROUNDS):                  # alternating: every case once per round
            for k, fn in cases.items():
                times[k].append(TJ.timed(fn))
        med = {k: statistics.median(t) for k, t in times.items()}
        peak = {k: peak_extra(fn) for k, fn in memory.items()}
        print(f"{'case':<36} {'points':>10} {'fused ms':>9} {'two-pass ms':>11} {'ratio':>6} {'fused MB':>9} {'two-pass MB':>11} {'Jacobian entry alone ms':>24}")
        for name in ("sb2006", "mp1m"):
            for ft in ("f32", "f64"):
                for product in ("vjp", "jvp"):
                    a, b = f"{name} {ft} {product} fused", f"{name} {ft} {product} jacobian + einsum"
                    print(f"{name + ' ' + ft + ' ' + product:<36} {n:>10d} {med[a]:>9.3f} {med[b]:>11.3f} {med[a] / med[b]:>6.3f} {peak[a] / 1e6:>9.1f} {peak[b] / 1e6:>11.1f} {med[f'{name} {ft} jacobian alone']:>24.3f}",
                          flush=True)


if __name__ == "__main__":
    main()
