"""What tests/test_column_products_host.py and tests/test_column_products_gpu.py share: the columns, the finite-difference reference of the Float64 ORACLE's column
step (oracle_binding.sb2006_column_tendencies_sedimentation), the measure, and the ctypes calls into the host build tests/native/column_products_host.cpp.

STATES.  The interior states of tests/jacobian_cases.py (all four species present, away from the gates) arranged into columns, level 0 lowest; at every 13th
point the rain is taken out (q_rai = n_rai = 0: the fall-speed gates, a cell that receives a flux and sends none), so most levels carry rain.  Shapes, the
smallest at which the kernels can go wrong (cmx_sb2006_column_products.hip: one point per lane, a workgroup owns 255 points):
    n7  120 columns of 7 levels = 840 points: the tile boundaries 255, 510 and 765 fall inside columns, at levels 3, 6 and 2
    n1  64 columns of 1 level: every cell is top and surface     n2  32 columns of 2 levels     n3  2 columns of 3 levels

REFERENCE.  J v by central differences of the oracle ALONG v, without assembling J: y_ref = (f(x + t v) − f(x − t v)) / 2t with v_j = r_j·x_j, so x ± t v =
x_j (1 ± t r_j) — the step rule of jacobian_cases.fd_jacobian (h = 1e-6·|x_j|, up to |r_j| ≤ 1) for every input at once; t = 1e-6, and 4e-6 for the
set-aside criterion.  (The realised x⁺ − x⁻ differs from 2 t v by the rounding of x (1 ± t r), ≤ 2⁻⁵³/1e-6 ≈ 1e-10 relative: far below AGREE.)

MEASURE: the input-scaled mixed-vector measure of tests/jacobian_products_cases.py, summed over the stencil — a row of the column Jacobian has the six entries
of its own level and the six of the level above:
    s'_i = max over both blocks of |J^ref_ij|·|x_j|      (from the REFERENCE alone; the two blocks by differencing one input at the even / the odd levels)
    R_i  = Σ_j |r_j| over the own level and the level above (inputs with x_j = 0 carry no tangent and are not counted)
    |y_i − y_i^ref| < B·s'_i·R_i,      B = jacobian_cases.BOUND (1e-5 Float64, 1e-3 Float32)
and the same for the precipitation flux, whose row has the six entries of level 0.  Cotangents weigh every output alike: ḡ_q = r'_q / s'_q, p̄ = r'_p / s'_p.
The adjoint identity couples the levels, so it is summed over each whole column, with the precipitation terms:
    |Σ_k ḡ_k·(J v)_k + p̄·ṗ − Σ_k (Jᵀḡ)_k·v_k| < 2B·(Σ_i Σ_q |ḡ_qi|·s'_qi·R_i + |p̄|·s'_p·R_p)
A point is SET ASIDE only by a criterion of the reference: y_ref at t and at 4t disagree by more than jacobian_cases.AGREE in this measure (a kink of the
column step inside the stencil); a column is set aside for the adjoint identity if one of its points or its precipitation row is.  At most
jacobian_cases.MAX_SET_ASIDE (1 %) of the points and of the columns of a set may be set aside (`checked`; asserted in the host test)."""
import ctypes as C
import functools

import numpy as np

import jacobian_cases as JC
from jacobian_host_build import CT, NPT, _arr, _same_bits, host_fixture  # noqa: F401
from cmx import _abi
from cmx import parameters as P

host = host_fixture("column_products_host")
BOUND, AGREE, MAX_SET_ASIDE = JC.BOUND, JC.AGREE, JC.MAX_SET_ASIDE
WRT, OUT = JC.WRT, JC.OUT
VELS = ("sb", "chen", "chen_gen")
VEL_KIND = {"sb": 1, "chen": 2, "chen_gen": 3}          # csrc/cmx_sb2006.hpp VEL_SB, VEL_CHEN, VEL_CHEN_GEN: what the host build returns
CASES = [(limited, vel, cloud) for limited in (True, False) for vel in VELS for cloud in (False, True)]
CASE_IDS = [f"{'limited' if c[0] else 'notlimited'}-{c[1]}-{'cloud' if c[2] else 'nocloud'}" for c in CASES]
MAIN_CASE = (True, "sb", True)
SHAPES = {"n7": (120, 7), "n1": (64, 1), "n2": (32, 2), "n3": (2, 3)}
_OFFSET = {"n7": 0, "n1": 840, "n2": 904, "n3": 968}


# ---- parameters -----------------------------------------------------------------------------------------------------------------------------------
def rain_vel(ft, vel):
    """The rain fall-speed struct; chen_gen: b_ρ = 0.6, a table that make_chen_log rejects (the general Chen-2022 instantiation, run-time Γ)."""
    v = P.rain_vel_params(ft)
    if vel == "chen_gen":
        v.chen2022.b_rho = 0.6
    return v


def flags(case):
    return (_abi.CMX_SB2006_LIMITED if case[0] else 0) | (_abi.CMX_VEL_SB2006 if case[1] == "sb" else _abi.CMX_VEL_CHEN2022)


def params(ft, case):
    """(warm-rain parameters, thermodynamics, rain fall speed, Stokes cloud fall speed or None) of a case in one float type."""
    return P.WarmRainParams2M(ft, case[0]), P.ThermodynamicsParameters(ft), rain_vel(ft, case[1]), P.StokesRegimeVelType(ft) if case[2] else None


# ---- columns --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _interior():
    import oracle_binding as oracle
    oracle.lib()
    return JC.interior_states(oracle)


def columns(shape):
    """(inv_dz [n_lev], the seven state columns, each (n_col, n_lev), Float64) of a shape."""
    n_col, n_lev = SHAPES[shape]
    lo, n = _OFFSET[shape], n_col * n_lev
    cols = [np.array(c[lo:lo + n], dtype=np.float64).reshape(n_col, n_lev) for c in _interior()]
    dry = (np.arange(lo, lo + n) % 13 == 7).reshape(n_col, n_lev)
    cols[5][dry] = 0.0
    cols[6][dry] = 0.0
    inv_dz = 1.0 / (40.0 + 35.0 * np.arange(n_lev) + 11.0 * (np.arange(n_lev) % 3))
    return inv_dz, cols


def oracle_column(oracle, case, inv_dz, cols):
    """([4, n] tendencies, [n_col] precipitation flux) of the Float64 oracle's column step."""
    wr, tps, vel, stokes = params("f64", case)
    r = oracle.sb2006_column_tendencies_sedimentation(_abi.F64, wr.c, tps, vel, stokes, flags(case), inv_dz, *cols, float32_gates=False, nthreads=4)
    return np.stack([r[k] for k in OUT]), np.array(r["precip_flux"])


# ---- the reference --------------------------------------------------------------------------------------------------------------------------------
def _row_scales(f, inv_dz, cols, step=1e-6):
    """(s' [4, n], s'_p [n_col]) of the module docstring: one input differenced at the even, then at the odd levels, gives the own-level and the
    level-above entry of every row separately (the block Jacobian is upper bidiagonal)."""
    n_col, n_lev = cols[0].shape
    lev = np.arange(n_lev)
    s, sp = np.zeros((4, n_col, n_lev)), np.zeros(n_col)
    for j in range(6):
        x = cols[j + 1]
        for parity in range(min(2, n_lev)):
            on = (lev % 2 == parity)[None, :]
            h = np.where(on, step * np.abs(x), 0.0)
            xp, xm = x + h, x - h
            (fp, pp), (fm, pm) = f(cols[:j + 1] + [xp] + cols[j + 2:]), f(cols[:j + 1] + [xm] + cols[j + 2:])
            d = (fp - fm).reshape(4, n_col, n_lev)
            dx = xp - xm
            with np.errstate(divide="ignore", invalid="ignore"):
                own = np.where(dx != 0, d / dx[None], 0.0) * np.abs(x)[None]                        # rows of the perturbed levels
                up = np.zeros_like(d)
                up[:, :, :-1] = np.where(dx[:, 1:] != 0, d[:, :, :-1] / dx[None, :, 1:], 0.0) * np.abs(x[:, 1:])[None]      # rows below a perturbed level
                if parity == 0:
                    sp = np.maximum(sp, np.abs(np.where(dx[:, 0] != 0, (pp - pm) / dx[:, 0], 0.0) * x[:, 0]))
            s = np.maximum(s, np.where(on[None], np.abs(own), np.abs(up)))
    return s.reshape(4, -1), sp


@functools.lru_cache(maxsize=None)
def _reference(case, shape, seed=5):
    import oracle_binding as oracle
    oracle.lib()
    inv_dz, cols = columns(shape)
    n_col, n_lev = cols[0].shape
    f = lambda c: oracle_column(oracle, case, inv_dz, c)  # noqa: E731
    s, sp = _row_scales(f, inv_dz, cols)
    x = np.stack(cols[1:])                                                   # [6, n_col, n_lev]
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 1.0, x.shape) * rng.choice([-1.0, 1.0], x.shape)
    rq = rng.uniform(0.5, 1.0, (4, n_col * n_lev)) * rng.choice([-1.0, 1.0], (4, n_col * n_lev))
    rp = rng.uniform(0.5, 1.0, n_col) * rng.choice([-1.0, 1.0], n_col)
    v = r * x
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(s > 0, rq / s, 0.0)
        pbar = np.where(sp > 0, rp / sp, 0.0)
    rl = (np.abs(r) * (x != 0)).sum(axis=0)                                  # Σ_j |r_j| per point
    R = rl.copy()
    R[:, :-1] += rl[:, 1:]
    R, Rp = R.reshape(-1), rl[:, 0]

    def along(t):
        (fp, pp), (fm, pm) = f([cols[0]] + list(x + t * v)), f([cols[0]] + list(x - t * v))
        return (fp - fm) / (2 * t), (pp - pm) / (2 * t)
    (y1, p1), (y4, p4) = along(1e-6), along(4e-6)

    def frac(err, lim):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    dis = frac(np.abs(y1 - y4), s * R[None]).max(axis=0)
    disp = frac(np.abs(p1 - p4), sp * Rp)
    kept = dis <= AGREE
    keptp = disp <= AGREE
    keptc = kept.reshape(n_col, n_lev).all(axis=1) & keptp
    ref = dict(case=case, shape=shape, n_col=n_col, n_lev=n_lev, inv_dz=inv_dz, cols=cols, v=list(v), g=list(g), pbar=pbar, s=s, sp=sp, R=R, Rp=Rp, y=y1, yp=p1,
               kept=kept, keptp=keptp, keptc=keptc, worst=float(max(dis.max(), disp.max())))
    for a in (inv_dz, *cols, *ref["v"], *ref["g"], pbar, s, sp, R, Rp, y1, p1, kept, keptp, keptc):
        a.setflags(write=False)
    return ref


def reference_unchecked(case, shape):
    return _reference(tuple(case), shape)


def set_aside_shares(ref):
    """(share of the points, share of the columns) that the reference's criterion sets aside."""
    return float((~ref["kept"]).mean()), float((~ref["keptc"]).mean())


def checked(ref):
    """The 1 % condition on a reference."""
    pts, cls = set_aside_shares(ref)
    assert pts <= MAX_SET_ASIDE and cls <= MAX_SET_ASIDE, (ref["case"], ref["shape"], pts, cls, ref["worst"])
    return ref


def reference(case, shape):
    """The reference of (case, shape), computed once and shared read-only; asserts the 1 % condition."""
    return checked(reference_unchecked(case, shape))


# ---- the measure ----------------------------------------------------------------------------------------------------------------------------------
def _worst(err, lim, kept):
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(lim > 0, err / lim, np.where(err == 0, 0.0, np.inf))
    f = np.where(np.isfinite(f), f, np.inf)[..., kept]
    return float(f.max()) if f.size else 0.0


def jvp_fractions(ref, y, yp, bound):
    """The worst used fraction of the bound over the kept points: (J v, ṗ)."""
    y, yp = np.asarray(y, dtype=np.float64), np.asarray(yp, dtype=np.float64)
    return _worst(np.abs(y - ref["y"]), bound * ref["s"] * ref["R"][None], ref["kept"]), _worst(np.abs(yp - ref["yp"]), bound * ref["sp"] * ref["Rp"], ref["keptp"])


def adjoint_fraction(ref, y, yp, grad, bound):
    """The worst used fraction of the 2B bound of the adjoint identity over the kept columns: y = J v, yp = ṗ, grad = Jᵀḡ of the code under test on the
    reference's v, ḡ, p̄."""
    n_col, n_lev = ref["n_col"], ref["n_lev"]
    y, yp, grad = np.asarray(y, dtype=np.float64), np.asarray(yp, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    g, v = np.stack(ref["g"]), np.stack(ref["v"]).reshape(6, -1)
    lhs = (g * y).sum(axis=0).reshape(n_col, n_lev).sum(axis=1) + ref["pbar"] * yp
    rhs = (grad * v).sum(axis=0).reshape(n_col, n_lev).sum(axis=1)
    lim = 2 * bound * (((np.abs(g) * ref["s"]).sum(axis=0) * ref["R"]).reshape(n_col, n_lev).sum(axis=1) + np.abs(ref["pbar"]) * ref["sp"] * ref["Rp"])
    return _worst(np.abs(lhs - rhs), lim, ref["keptc"])


def assert_products(ft, ref, y, yp, grad, what, report=True):
    fy, fp = jvp_fractions(ref, y, yp, BOUND[ft])
    fa = adjoint_fraction(ref, y, yp, grad, BOUND[ft])
    if report:
        print(f"{what} {ft} {ref['case']} {ref['shape']}: kept {int(ref['kept'].sum())}/{ref['kept'].size} points, {int(ref['keptc'].sum())}/{ref['keptc'].size} columns, "
              f"t-vs-4t {ref['worst']:.3g}; worst used fraction of the bound — J v {fy:.3g}, precipitation {fp:.3g}, adjoint identity {fa:.3g}")
    assert fy < 1.0, (what, "J v", fy)
    assert fp < 1.0, (what, "precip", fp)
    assert fa < 1.0, (what, "adjoint", fa)
    return fy, fp, fa


# ---- calls into the host build --------------------------------------------------------------------------------------------------------------------
def _flat(ft, a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=NPT[ft]) if a is not None else None


def _ptr(ft, a):
    return a.ctypes.data_as(C.POINTER(CT[ft])) if a is not None else None


def _head(ft, case, override_flags=None):
    wr, tps, vel, stokes = keep = params(ft, case)
    return keep, (C.byref(wr.c), C.byref(tps), C.byref(vel), C.byref(stokes) if stokes is not None else None, C.c_uint32(flags(case) if override_flags is None else override_flags))


def host_jvp(host, ft, case, inv_dz, cols, tangents, want=(True,) * 4, want_precip=True, with_primal=True, override_flags=None, sentinel=-7.0):
    """(jvp [4, n], jvp_precip [n_col], tendencies [4, n], precip [n_col], status ≥ 0: the velocity kind that ran) of the host build.  tangents: six arrays or
    None, or None for a NULL table.  Buffers that are not requested keep the sentinel."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    t = [_flat(ft, a) for a in tangents] if tangents is not None else None
    jv, tend = np.full((4, n), sentinel, dtype=NPT[ft]), np.full((4, n), sentinel, dtype=NPT[ft])
    jp, pr = np.full(n_col, sentinel, dtype=NPT[ft]), np.full(n_col, sentinel, dtype=NPT[ft])
    keep, head = _head(ft, case, override_flags)
    fn = getattr(host, f"host_sb2006_column_jvp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, t) if t is not None else None,
            _arr(ft, [jv[q] if want[q] else None for q in range(4)]), _ptr(ft, jp) if want_precip else None,
            _arr(ft, list(tend)) if with_primal else None, _ptr(ft, pr) if with_primal else None)
    return jv, jp, tend, pr, rc


def host_vjp(host, ft, case, inv_dz, cols, cotangents, cot_precip, want=(True,) * 6, with_primal=True, k=0, override_flags=None, sentinel=-7.0):
    """(grad [6, n], tendencies [4, n], precip [n_col], status) of the host build.  cotangents: four arrays or None, or None for a NULL table."""
    n_col, n_lev = np.shape(cols[0])
    n = n_col * n_lev
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    g = [_flat(ft, a) for a in cotangents] if cotangents is not None else None
    pb = _flat(ft, cot_precip)
    grad, tend, pr = np.full((6, n), sentinel, dtype=NPT[ft]), np.full((4, n), sentinel, dtype=NPT[ft]), np.full(n_col, sentinel, dtype=NPT[ft])
    keep, head = _head(ft, case, override_flags)
    fn = getattr(host, f"host_sb2006_column_vjp_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int(k), C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, g) if g is not None else None, _ptr(ft, pb),
            _arr(ft, [grad[j] if want[j] else None for j in range(6)]), _arr(ft, list(tend)) if with_primal else None, _ptr(ft, pr) if with_primal else None)
    return grad, tend, pr, rc


def host_plain(host, ft, case, inv_dz, cols):
    """([4, n] tendencies, [n_col] precipitation flux, status) of the PLAIN instantiation in the host build: the operations of sb2006_column_kernel."""
    n_col, n_lev = np.shape(cols[0])
    x, dz = [_flat(ft, c) for c in cols], _flat(ft, inv_dz)
    y, pr = np.empty((4, n_col * n_lev), dtype=NPT[ft]), np.empty(n_col, dtype=NPT[ft])
    keep, head = _head(ft, case)
    fn = getattr(host, f"host_sb2006_column_plain_{ft}")
    fn.restype = C.c_int32
    rc = fn(*head, C.c_int64(n_col), C.c_int32(n_lev), _ptr(ft, dz), _arr(ft, x), _arr(ft, list(y)), _ptr(ft, pr))
    return y, pr, rc
