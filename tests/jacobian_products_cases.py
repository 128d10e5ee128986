"""What the tests of the products with the Jacobian share (tests/test_jacobian_products_host.py, tests/test_jacobian_products_gpu.py): the ctypes calls into the
host build tests/native/derivatives_host.cpp, the two schemes' parameter cases as one table, and the MIXED-VECTOR check.

States, reference Jacobians, bounds and the 1 % set-aside cap are those of tests/jacobian_cases.py and tests/jacobian_1m_cases.py, imported, not restated.

THE MIXED-VECTOR CHECK.  Assembling J from unit seeds and handing it to `assert_parity` tests each entry alone; a product is a SUM of entries of very different
sizes and units, so it is tested with vectors that weight every input and output alike.  With B = BOUND[ft] the per-entry bound of the input-scaled measure
(|J_ij − J^ref_ij|·|x_j| < B·s'_i, s'_i = max_j |J^ref_ij|·|x_j| from the REFERENCE alone), draw per state, seeded,
    r_j = ±u, u ∈ [0.5, 1],  v_j = r_j·x_j            (a relative perturbation of every input of order one)
    r'_q = ±u,               ḡ_q = r'_q / s'_q         (every output weighs the same; ḡ_q = 0 where the reference row is identically zero)
and compare with the products of the finite-difference reference formed in Float64, y^ref = J^ref v and g^ref = J^refᵀ ḡ.  Summing the per-entry bound,
    |y_i − y_i^ref|        < B · s'_i · Σ_j |r_j|
    |g_j − g_j^ref|·|x_j|  < B · Σ_q |ḡ_q|·s'_q
    |ḡ·(J v) − (Jᵀḡ)·v|    < 2B · (Σ_j |r_j|)·(Σ_q |ḡ_q|·s'_q)       (the adjoint identity: both sides from the code under test, each within B of the same number)
on the kept states.  The rounding of v and ḡ to Float32 (6e-8 relative) is far below B = 1e-3; in Float64 they are exact inputs.  `mixed_fractions` returns the
worst used fraction of each bound, `assert_mixed` prints and asserts them."""
import ctypes as C

import numpy as np

import jacobian_1m_cases as J1
import jacobian_cases as JC
from jacobian_host_build import CT, JAC, JVP, NPT, VJP, _same_bits, host_fixture, host_plain  # noqa: F401
from jacobian_host_build import host_call as _call
from cmx import _abi
from cmx import parameters as P

host = host_fixture()
BOUND = JC.BOUND


# ---- the two schemes as one table ---------------------------------------------------------------------------------------------------------------
class SB2006:
    name, entry, WRT, OUT = "sb2006", "sb2006", JC.WRT, JC.OUT
    CASES = ((True, False), (False, False), (True, True))        # (limited, perturbed): tests/test_sb2006_jacobian_host.py
    SETS = ("interior", "points")
    INTERIOR = ((True, False), "interior")

    @staticmethod
    def params(ft, case):
        return JC.warm_rain_params(ft, case[0], JC.perturbed_overrides() if case[1] else None)

    @staticmethod
    def flags(mp, case):
        return _abi.CMX_SB2006_LIMITED if case[0] else 0

    @staticmethod
    def reference(case, which):
        return JC.reference(case[0], case[1], which)

    @staticmethod
    def assert_parity(ft, J, case, which, what):
        return JC.assert_parity(ft, J, case[0], case[1], which, what)


class MP1M:
    name, entry, WRT, OUT = "mp1m", "mp1m", J1.WRT, J1.OUT
    CASES = J1.CASES
    SETS = J1.SETS
    INTERIOR = ("default", "cold")

    @staticmethod
    def params(ft, case):
        return J1.params(ft, case)

    @staticmethod
    def flags(mp, case):
        return mp.flags

    @staticmethod
    def reference(case, which):
        return J1.reference(case, which)

    @staticmethod
    def assert_parity(ft, J, case, which, what):
        return J1.assert_parity(ft, J, case, which, what)


SCHEMES = {"sb2006": SB2006, "mp1m": MP1M}
SCHEME_CASES = [(s, c) for s in ("sb2006", "mp1m") for c in SCHEMES[s].CASES]


def head(scheme, ft, case):
    mp = scheme.params(ft, case)
    return mp, (C.byref(mp.c), C.byref(P.ThermodynamicsParameters(ft)), C.c_uint32(scheme.flags(mp, case)))


# ---- calls into the host build ------------------------------------------------------------------------------------------------------------------
def _given(ft, cols):
    return [np.ascontiguousarray(c, dtype=NPT[ft]) if c is not None else None for c in cols]


def host_jacobian(host, entry, ft, head, cols, nout=4, nwrt=6, k=0):
    """([nout, nwrt, n] Jacobian, [nout, n] tendencies, status) of the Jacobian driver in THIS build."""
    n = np.asarray(cols[0]).size
    jac, tend = np.full((nout, nwrt, n), np.nan, dtype=NPT[ft]), np.full((nout, n), np.nan, dtype=NPT[ft])
    rc = _call(host, entry, ft, JAC, head, k, cols, None, [jac[o, j] for o in range(nout) for j in range(nwrt)], tend)
    return jac, tend, rc


def host_jvp(host, entry, ft, head, cols, tangents, nout=4, want=None, with_tendencies=True, table=True):
    """([nout, n] J v, [nout, n] tendencies, status); tangents: one array or None per differentiated input; want: which of the nout products are requested
    (the others keep the sentinel −7); table=False passes a NULL tangent table."""
    n = np.asarray(cols[0]).size
    jvp = np.full((nout, n), -7.0, dtype=NPT[ft])
    tend = np.full((nout, n), -7.0, dtype=NPT[ft]) if with_tendencies else None
    want = [True] * nout if want is None else want
    rc = _call(host, entry, ft, JVP, head, 0, cols, _given(ft, tangents) if table else None, [jvp[o] if want[o] else None for o in range(nout)], tend)
    return jvp, tend, rc


def host_vjp(host, entry, ft, head, cols, cotangents, nwrt=6, nout=4, want=None, k=0, with_tendencies=True, table=True):
    """([nwrt, n] Jᵀḡ, [nout, n] tendencies, status); cotangents: one array or None per output; want: which of the nwrt gradients are requested (the others
    keep the sentinel −7); k: tangents per pass."""
    n = np.asarray(cols[0]).size
    grad = np.full((nwrt, n), -7.0, dtype=NPT[ft])
    tend = np.full((nout, n), -7.0, dtype=NPT[ft]) if with_tendencies else None
    want = [True] * nwrt if want is None else want
    rc = _call(host, entry, ft, VJP, head, k, cols, _given(ft, cotangents) if table else None, [grad[j] if want[j] else None for j in range(nwrt)], tend)
    return grad, tend, rc


def assemble(jvp_of, vjp_of, n, ft, nout=4, nwrt=6):
    """(J column by column from nwrt J v with unit tangents, J row by row from nout Jᵀḡ with unit cotangents); jvp_of(tangents) → [nout, n],
    vjp_of(cotangents) → [nwrt, n]."""
    one = np.ones(n, dtype=NPT[ft])
    Jc = np.stack([jvp_of([one if i == j else None for i in range(nwrt)]) for j in range(nwrt)], axis=1)
    Jr = np.stack([vjp_of([one if i == q else None for i in range(nout)]) for q in range(nout)], axis=0)
    return Jc, Jr


# ---- the mixed-vector check ---------------------------------------------------------------------------------------------------------------------
def mixed_vectors(cols, J_ref, seed=5):
    """(r [6, n], v [6, n], ḡ [4, n], s' [4, n], y_ref [4, n], g_ref [6, n]) of a reference set, all Float64 (module docstring)."""
    x = np.stack([np.asarray(c, dtype=np.float64) for c in cols[1:]])
    J_ref = np.asarray(J_ref, dtype=np.float64)
    nout, nwrt, n = J_ref.shape
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 1.0, (nwrt, n)) * rng.choice([-1.0, 1.0], (nwrt, n))
    rp = rng.uniform(0.5, 1.0, (nout, n)) * rng.choice([-1.0, 1.0], (nout, n))
    s = (np.abs(J_ref) * np.abs(x)[None]).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(s > 0, rp / s, 0.0)
    v = r * x
    return r, v, g, s, np.einsum("ijn,jn->in", J_ref, v), np.einsum("ijn,in->jn", J_ref, g)


def mixed_fractions(y, grad, cols, J_ref, kept, bound, seed=5):
    """The worst used fraction over the kept states of the three bounds of the module docstring: (J v, Jᵀḡ, adjoint identity); y = J v and grad = Jᵀḡ of the
    code under test on mixed_vectors(cols, J_ref, seed).  A non-finite value gives Inf."""
    r, v, g, s, y_ref, g_ref = mixed_vectors(cols, J_ref, seed)
    x = np.stack([np.asarray(c, dtype=np.float64) for c in cols[1:]])
    y, grad = np.asarray(y, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    sr, sg = np.abs(r).sum(axis=0), (np.abs(g) * s).sum(axis=0)

    def worst(err, lim):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
        f = np.where(np.isfinite(f), f, np.inf)
        return float(f[..., kept].max())
    fy = worst(np.abs(y - y_ref), bound * s * sr[None])
    fg = worst(np.abs(grad - g_ref) * np.abs(x), bound * np.broadcast_to(sg[None], grad.shape))
    fa = worst(np.abs((g * y).sum(axis=0) - (grad * v).sum(axis=0)), 2 * bound * sr * sg)
    return fy, fg, fa


def assert_mixed(ft, y, grad, cols, J_ref, kept, what, report=True):
    fy, fg, fa = mixed_fractions(y, grad, cols, J_ref, kept, BOUND[ft])
    if report:
        print(f"{what} {ft}: mixed vectors, worst used fraction of the bound — J v {fy:.3g}, Jᵀḡ {fg:.3g}, adjoint identity {fa:.3g}")
    assert fy < 1.0, (what, "J v", fy)
    assert fg < 1.0, (what, "J^T g", fg)
    assert fa < 1.0, (what, "adjoint", fa)
    return fy, fg, fa
