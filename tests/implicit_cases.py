"""What tests/test_implicit_host.py and tests/test_implicit_gpu.py share for the linearly implicit tendency r = (I − Δt J)⁻¹ f (include/cmx.h §18): the call
into the host build tests/native/implicit_host.cpp, the states of the two real schemes, and the measures.

Measures, all formed in Float64 from values of the float type under test (A = I − Δt J with J and f that type's own Jacobian and tendencies):
  * backward error  ω = max_i |(A r − f)_i| / (Σ_j |A_ij| |r_j| + |f_i|)  — the componentwise (Oettli–Prager) backward error; invariant under any row or
    column scaling of the system, so it judges the solve and not the units.  The yardstick is LAPACK in the same precision (numpy.linalg.solve on copies of A
    and f in the float type): the fused solve's worst ω over a set may be at most 4 × LAPACK's worst over the same set, and never has to be below 16 eps.
  * forward error (Float64)  e = max_j |r_j − r*_j| / c_j  ÷  max_j |r*_j| / c_j  against r* = numpy.linalg.solve in Float64, in the unknowns the kernel solves
    for (c_j = 2^⌊log2 s_j⌋ of the clamped state, 1 for an absent species): the max-norm in which κ∞ of the equilibrated matrix B = D_r A D_c bounds the
    forward error by κ∞ × backward error.  Bound 8 κ∞(B) eps per point; points with κ∞(B) > 1e6 are left out, at most 5 % of a set.
"""
import ctypes as C
import functools

import numpy as np

import jacobian_cases as JC
import jacobian_1m_cases as J1
from jacobian_host_build import CT, NPT, _arr
from cmx import _abi
from cmx import parameters as P

DTS = (0.0, 1.0, 30.0, 300.0)
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}
KAPPA_MAX = 1e6
MAX_LEFT_OUT = 0.05
SPECIES = {"sb2006": _abi.SB2006_JAC_WRT[2:6], "mp1m": _abi.MP1M_JAC_WRT[2:6]}     # wrt indices 2 … 5: the inputs whose tendencies the outputs are


def host_implicit(host, scheme, ft, head, dt, cols, k=0, with_tendencies=True, null=(), no_table=False, sentinel=np.nan):
    """([4, n] r, [4, n] tendencies or None, status) of host_<scheme>_implicit_<ft>(*head, dt, k, n, x, r, tend); null: members of `implicit` left NULL."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    r = np.full((4, x[0].size), sentinel, dtype=NPT[ft])
    tend = np.full((4, x[0].size), sentinel, dtype=NPT[ft]) if with_tendencies else None
    fn = getattr(host, f"host_{scheme}_implicit_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_double(dt), C.c_int(k), C.c_int64(x[0].size), _arr(ft, x), None if no_table else _arr(ft, [None if q in null else r[q] for q in range(4)]),
            _arr(ft, list(tend)) if tend is not None else None)
    return r, tend, rc


def head_sb2006(ft, wr, limited):
    return C.byref(wr.c), C.byref(P.ThermodynamicsParameters(ft)), C.c_uint32(_abi.CMX_SB2006_LIMITED if limited else 0)


def head_mp1m(ft, mp):
    return C.byref(mp.c), C.byref(P.ThermodynamicsParameters(ft)), C.c_uint32(mp.flags)


def head_toy(ft, M):
    return ((CT[ft] * 16)(*[float(v) for v in np.asarray(M, dtype=NPT[ft]).ravel()]),)


@functools.lru_cache(maxsize=None)
def _states(name):
    import oracle_binding as oracle
    oracle.lib()
    if name == "sb2006":
        sets = [JC.interior_states(oracle), JC.points(JC.WARM_RAIN, JC.KAT, JC.BOUNDARY)]
    else:
        sets = [J1.states(oracle, "cold"), J1.states(oracle, "warm"), J1.points(J1.CALLER, J1.SUITE_WARM)]
    cols = [np.concatenate(c) for c in zip(*sets)]
    for c in cols:
        c.setflags(write=False)
    return cols


def sb2006_states(oracle):
    """The interior set of tests/jacobian_cases.py (4096 states, all four species present) followed by its three pinned points; the last one has no rain.
    Computed once and shared read-only."""
    return _states("sb2006")


def mp1m_states(oracle):
    """The cold and the warm set of tests/jacobian_1m_cases.py (4096 states each) followed by its two pinned points.  Computed once and shared read-only."""
    return _states("mp1m")


def system(ft, J, f, dt):
    """A = I − Δt J [n, 4, 4] and f [n, 4] in Float64 from the float type's own J [4, 4, n] (∂f_q/∂s_j) and f [4, n]; Δt rounded to the float type like the entry does."""
    dt = float(NPT[ft](dt))
    A = np.eye(4)[None] - dt * np.moveaxis(np.asarray(J, dtype=np.float64), 2, 0)
    return A, np.asarray(f, dtype=np.float64).T.copy()


def omega(A, r, f):
    """The componentwise backward error per point; r [n, 4]."""
    r = np.asarray(r, dtype=np.float64)
    res = np.abs(np.einsum("nij,nj->ni", A, r) - f)
    den = np.einsum("nij,nj->ni", np.abs(A), np.abs(r)) + np.abs(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(den > 0, res / den, np.where(res > 0, np.inf, 0.0))
    return w.max(axis=1)


def lapack(ft, A, f):
    """numpy.linalg.solve on copies of A and f in the float type (sgesv / dgesv)."""
    return np.linalg.solve(A.astype(NPT[ft]), f.astype(NPT[ft])[..., None])[..., 0]


def omega_bound(ft, A, f):
    """(the bound on the fused solve's worst ω over the set, LAPACK's worst ω)."""
    w = float(omega(A, lapack(ft, A, f), f).max())
    return max(4.0 * w, 16.0 * EPS[ft]), w


def pow2_floor(x):
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, e - 1)


def column_scales(species):
    """c [n, 4]: 2^⌊log2 s⌋ of the clamped state, 1 for an absent species — the kernel's column scales (csrc/cmx_jacobian.hpp implicit_point)."""
    s = np.asarray(species, dtype=np.float64).T
    return pow2_floor(np.where(s > 0, s, 1.0))


def equilibrated(A, c, with_row_scales=False):
    """B = D_r A D_c with the kernel's scales and κ∞(B) per point [, the row scales [n, 4]]."""
    B = A * c[:, None, :]
    rs = 1.0 / pow2_floor(np.abs(B).max(axis=2))
    B = B * rs[:, :, None]
    kappa = np.abs(B).sum(axis=2).max(axis=1) * np.abs(np.linalg.inv(B)).sum(axis=2).max(axis=1)
    return (B, kappa, rs) if with_row_scales else (B, kappa)


def forward_error(r, r_ref, c):
    """The forward error per point in the scaled unknowns."""
    z, z_ref = np.asarray(r, dtype=np.float64) / c, r_ref / c
    return np.abs(z - z_ref).max(axis=1) / np.abs(z_ref).max(axis=1)
