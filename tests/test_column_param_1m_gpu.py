"""The derivatives of the 1-moment column step with respect to the PARAMETERS on the device (cmx_mp1m_column_param_jvp_* / _param_vjp_*, include/cmx.h §(28);
cmx.column_param_jvp_1m, cmx.column_param_vjp_1m, cmx.autograd.column_tendencies_sedimentation_1m(…, theta=, names=)): the assertions of
tests/test_column_param_1m_host.py through the C ABI and the kernels — same columns, names, reference, measure and 1 % condition
(tests/column_param_1m_cases.py) — and what only the device has: the tiling of the J_θ δθ kernel, the reduction of the gradient, graph capture, autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

import column_param_1m_cases as KC
from column_param_1m_cases import CASE_IDS, CASES, MAIN_CASE, WHICH
from jacobian_host_build import _build
import cmx
from cmx import _abi
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
KP = {"f32": 4, "f64": 2}      # csrc/cmx_mp1m_column_param.hpp kCol1mParamK


def no_exp(case):
    return tuple(k for k in KC.names(case) if k not in KC.EXPONENT_NAMES)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, ft, dev, shape=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, dtype=np.float64)).to(DT[ft]).to(dev)
    return t.reshape(shape).contiguous() if shape is not None else t


def _eq(a, b):
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


class Setup:
    """The parameters of a case in one float type, the directions θ_p along each of `names`, and a reference's columns on the device."""
    def __init__(self, ft, ref, dev, names=None, case=None):
        self.ft, self.ref, self.case = ft, ref, ref["case"] if case is None else case
        self.names = ref["names"] if names is None else names
        self.structs, tables = KC.directions(ft, self.case, self.names)
        self.dirs = [tuple(t[d] for t in tables) for d in range(len(self.names))]
        self.shape = (ref["n_col"], ref["n_lev"])
        self.inv_dz = _t(ref["inv_dz"], ft, dev)
        self.cols = [_t(c, ft, dev, self.shape) for c in ref["cols"]]
        g, pbar = KC.cotangents(ref)
        self.cot, self.pbar = [_t(a, ft, dev, self.shape) for a in g], [_t(a, ft, dev) for a in pbar]

    def jvp(self, dirs=None, cols=None, inv_dz=None, **kw):
        return cmx.column_param_jvp_1m(*self.structs, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                       self.dirs if dirs is None else dirs, **kw)

    def vjp(self, cot="ref", pbar="ref", dirs=None, cols=None, **kw):
        pb = self.pbar if isinstance(pbar, str) else pbar
        return cmx.column_param_vjp_1m(*self.structs, self.inv_dz, *(self.cols if cols is None else cols), self.cot if isinstance(cot, str) else cot, pb[0], pb[1],
                                       self.dirs if dirs is None else dirs, **kw)

    def primal(self, cols=None):
        r = cmx.column_tendencies_sedimentation_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), *self.structs, self.inv_dz, *(self.cols if cols is None else cols))
        return torch.stack(list(r[:4])), r.precip_rai, r.precip_sno


def _np(r):
    return r.jvp.reshape(r.jvp.shape[0], 4, -1).cpu().numpy(), torch.stack([r.jvp_precip_rai, r.jvp_precip_sno]).cpu().numpy()


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except cmx.CmxStatusError as e:
        return e.status
    return 0


def _assert_gradient(s, jv, jp, grad):
    """grad[d] against Σ ḡ·jvp_d + Σ p̄·ṗ_d summed in float64 on the host from the jvp columns: within BOUND of the size of the terms; the per-point sums
    differ by the rounding of a chain of at most eight fma in the float type, so the difference is in fact within 8 eps·Σ |terms| (the §22 gradient tests)."""
    g = torch.stack(s.cot).reshape(4, -1).cpu().numpy()
    want, size = KC.grad_from_jvp(g, torch.stack(s.pbar).cpu().numpy(), jv, jp)
    eps = np.finfo(KC.NPT[s.ft]).eps
    used = np.max(np.abs(grad - want) / np.where(size > 0, 8 * eps * size, 1.0))
    print(f"device {s.ft} {s.case}: gradient against the jvp columns, worst used fraction of 8 eps·Σ|terms| {used:.3g}")
    assert (np.abs(grad - want) <= min(KC.BOUND[s.ft], 8 * eps) * size).all() and ((size == 0) <= (grad == 0)).all()


# ---- against the differenced oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_case_and_set(dev, oracle, ft, case, which):
    """n7 — tile boundaries inside columns — for default, alt, exponents and the general-Γ rain table, cold and warm, every name of the case (more than
    CMX_PARAM_MAX_DIRS: the wrapper splits the call); the gradient is the sum over the jvp columns in every one of them, the Float64 general-Γ one included."""
    s = Setup(ft, KC.reference(case, which, "n7"), dev)
    jv, jp = _np(s.jvp())
    KC.assert_parity(ft, s.ref, jv, jp, "device")
    idx = {k: i for i, k in enumerate(s.names)}
    for k in KC.SEDIMENTATION_ONLY:
        assert jv[idx[k]].any(), k
    for k in ("latent_heat_vaporization_at_reference", "pressure_triple_point", "thermal_conductivity_of_air"):
        assert not jp[:, idx[k]].any() and jv[idx[k]].any(), k
    _assert_gradient(s, jv, jp, s.vjp().grad.cpu().numpy())


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("shape", ["n1", "n2", "n3"])
def test_small_columns(dev, oracle, ft, shape):
    """One level (every cell top and surface), two, two columns of three."""
    for which in WHICH:
        s = Setup(ft, KC.reference(MAIN_CASE, which, shape), dev)
        jv, jp = _np(s.jvp())
        KC.assert_parity(ft, s.ref, jv, jp, "device")
        _assert_gradient(s, jv, jp, s.vjp().grad.cpu().numpy())


@pytest.mark.parametrize("ft", FTS)
def test_the_device_agrees_with_the_host_build(dev, oracle, ft):
    """Both lie within BOUND of the same reference, so they differ by less than 2·BOUND in the row measure (the host build has libm in the place of the
    hardware transcendental instructions: no bits are shared)."""
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n7"), dev, names=no_exp(MAIN_CASE))
    jv, jp = _np(s.jvp())
    hv, hp, _, _, rc = KC.host_jvp(_build("column_param_1m_host"), ft, s.structs, s.ref["inv_dz"], s.ref["cols"], KC.tables_of(s.dirs))
    assert rc == KC.KIND[MAIN_CASE]
    kept, keptp = s.ref["kept"], s.ref["keptp"]
    e = KC.PC.row_error(jv.transpose(1, 0, 2), hv.transpose(1, 0, 2))[:, :, kept].max()
    ep = KC.PC.row_error(jp, hp)[:, :, keptp].max()
    print(f"{ft}: device against host build, worst row error {e:.3g}, precipitation {ep:.3g}")
    assert e < 2 * KC.BOUND[ft] and ep < 2 * KC.BOUND[ft]


# ---- bit identities ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tendencies_and_precipitation_fluxes_are_the_column_entry(dev, oracle, ft, case):
    """Bit for bit, from both entries, when no direction moves an exponent."""
    s = Setup(ft, KC.reference(case, "cold", "n7"), dev, names=no_exp(case)[:5] + KC.SEDIMENTATION_ONLY)
    want, wr, ws = s.primal()
    r = s.jvp(with_tendencies=True)
    assert _eq(r.tendencies, want) and _eq(r.precip_rai, wr) and _eq(r.precip_sno, ws)
    v = s.vjp(with_tendencies=True)
    assert _eq(v.tendencies, want) and _eq(v.precip_rai, wr) and _eq(v.precip_sno, ws)


@pytest.mark.parametrize("ft", FTS)
def test_a_column_does_not_depend_on_ndir_or_on_the_split(dev, oracle, ft):
    """A jvp column alone, among KP, KP + 1 and 16 directions, and in a call of more than CMX_PARAM_MAX_DIRS names split by the wrapper: the same bits; the
    gradient likewise, and bit-identical across two runs."""
    nm = no_exp(MAIN_CASE)
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n7"), dev, names=nm)
    assert len(nm) > 2 * _abi.CMX_PARAM_MAX_DIRS
    full = s.jvp()
    kp = KP[ft]
    for lo, nd in ((0, 1), (5, 1), (0, kp), (3, kp), (0, kp + 1), (7, kp + 1), (len(nm) - 1, 1), (2, 16), (21, 16)):
        r = s.jvp(dirs=s.dirs[lo:lo + nd])
        assert _eq(r.jvp, full.jvp[lo:lo + nd]) and _eq(r.jvp_precip_rai, full.jvp_precip_rai[lo:lo + nd]) and _eq(r.jvp_precip_sno, full.jvp_precip_sno[lo:lo + nd]), (lo, nd)
    g = s.vjp().grad
    assert _eq(g, s.vjp().grad)
    for lo, nd in ((0, 1), (0, kp), (1, kp + 1), (9, 3), (len(nm) - 1, 1), (20, 16)):
        assert _eq(s.vjp(dirs=s.dirs[lo:lo + nd]).grad, g[lo:lo + nd]), (lo, nd)


@pytest.mark.parametrize("ft", FTS)
def test_results_do_not_depend_on_tile_boundaries(dev, oracle, ft):
    """The same columns at other places of the launch — a call on the columns [c0, c1) of the set moves every tile boundary of the halo kernel, which the
    parameter entry shares with the state products: the same bits.  n7: 7 levels, so a 255-point tile boundary falls inside a column, and 120 columns span
    several tiles."""
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n7"), dev)
    full = s.jvp(with_tendencies=True)
    for c0, c1 in ((1, 120), (5, 77), (36, 38), (0, 37)):
        cut = lambda t: t[..., c0:c1, :].contiguous()  # noqa: E731
        r = s.jvp(cols=[cut(c) for c in s.cols], with_tendencies=True)
        assert _eq(r.jvp, cut(full.jvp)), (c0, c1)
        assert _eq(r.jvp_precip_rai, full.jvp_precip_rai[..., c0:c1]) and _eq(r.jvp_precip_sno, full.jvp_precip_sno[..., c0:c1]), (c0, c1)
        assert _eq(r.tendencies, cut(full.tendencies)) and _eq(r.precip_rai, full.precip_rai[c0:c1]) and _eq(r.precip_sno, full.precip_sno[c0:c1]), (c0, c1)


@pytest.mark.parametrize("ft", FTS)
def test_without_sedimentation_the_derivatives_are_the_pointwise_ones(dev, oracle, ft):
    """inv_dz ≡ 0, directions on mp and tps only: the four jvp rows equal cmx_mp1m_param_jvp_* under == wherever finite (here: everywhere — the flux tangents
    of these columns are finite, and the two fma per species add ∓0)."""
    nm = tuple(k for k in no_exp(MAIN_CASE) if k in P.MICROPHYSICS_1M_DIRECTION_NAMES)
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n7"), dev, names=nm)
    dirs = [(d[0], d[1], type(d[2])(), type(d[3])(), type(d[4])()) for d in s.dirs]
    r = s.jvp(dirs=dirs, inv_dz=torch.zeros_like(s.inv_dz))
    point = cmx.param_jvp_1m(s.structs[0], s.structs[1], *[c.reshape(-1) for c in s.cols], [(d[0], d[1]) for d in s.dirs])
    fin = torch.isfinite(r.jvp.reshape(point.jvp.shape))
    assert bool(fin.all()) and bool((r.jvp.reshape(point.jvp.shape) == point.jvp).all())


@pytest.mark.parametrize("ft", FTS)
def test_the_euler_relation_of_the_rain_fall_speed(dev, oracle, ft):
    """δa = a on all three entries of chen_rain.a: ṗ_rai = precip_rai to a few ulp of Σ |terms| (tests/test_column_param_1m_host.py has the flux part too)."""
    s = Setup(ft, KC.reference(MAIN_CASE, "warm", "n7"), dev, names=no_exp(MAIN_CASE)[:1])
    a = list(P.DEFAULT_PARAMETERS["Chen2022_table_B1_ai"])
    dirs = [{f"Chen2022_table_B1_ai[{i}]": a[i] for i in range(3)}] + [{f"Chen2022_table_B1_ai[{i}]": a[i]} for i in range(3)]
    r = s.jvp(dirs=dirs, with_tendencies=True)
    jp, pr = r.jvp_precip_rai.double().cpu().numpy(), r.precip_rai.double().cpu().numpy()
    terms = np.abs(jp[1:]).sum(axis=0)
    eps = np.finfo(KC.NPT[ft]).eps
    assert (np.abs(jp[0] - pr) <= 8 * eps * terms).all() and pr.any(), np.max(np.abs(jp[0] - pr) / np.where(terms > 0, terms, 1)) / eps
    assert not bool(r.jvp_precip_sno.any())


# ---- the NaN rule, the statuses, graph capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(dev, oracle, ft):
    """A poisoned point, a poisoned flux above level 0 and at level 0, a NaN cotangent."""
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n2"), dev, names=no_exp(MAIN_CASE)[:3] + KC.SEDIMENTATION_ONLY)
    clean = s.jvp()
    for j in range(7):
        bad = [c.clone() for c in s.cols]
        bad[j][5, 1] = float("nan")
        r = s.jvp(cols=bad, with_tendencies=True)
        want, wr, ws = s.primal(cols=bad)
        assert _eq(r.tendencies, want) and _eq(r.precip_rai, wr) and _eq(r.precip_sno, ws), j
        assert bool(torch.isnan(r.jvp[:, :, 5, 1]).all()), j
        assert bool((torch.isnan(r.jvp[0]) == torch.isnan(want)).all()), j      # the flux NaN reaches the cell below exactly where it does in the primal
        keep = torch.ones(s.shape, dtype=torch.bool, device=dev)
        keep[5] = False
        assert _eq(r.jvp[:, :, keep], clean.jvp[:, :, keep]) and _eq(r.jvp_precip_rai, clean.jvp_precip_rai) and _eq(r.jvp_precip_sno, clean.jvp_precip_sno), j
        assert bool(torch.isnan(s.vjp(cols=bad).grad).all()), j
        bad = [c.clone() for c in s.cols]
        bad[j][5, 0] = float("nan")
        r = s.jvp(cols=bad)
        assert bool(torch.isnan(r.jvp_precip_rai[:, 5]).all()) == (j in (0, 5)) and bool(torch.isnan(r.jvp_precip_sno[:, 5]).all()) == (j in (0, 6)), j
        assert bool(torch.isnan(s.vjp(cols=bad).grad).all()), j
    cot = [c.clone() for c in s.cot]
    cot[1][3, 0] = float("nan")
    assert bool(torch.isnan(s.vjp(cot=cot).grad).all())
    for r in range(2):
        pb = [p.clone() for p in s.pbar]
        pb[r][7] = float("nan")
        assert bool(torch.isnan(s.vjp(pbar=pb).grad).all())
    assert not bool(torch.isnan(s.vjp().grad).any())


def test_the_statuses_in_order(dev, oracle):
    s = Setup("f64", KC.reference(MAIN_CASE, "cold", "n3"), dev, names=no_exp(MAIN_CASE)[:3])
    BAD, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED

    def changed(k, setter, q=1):
        d = [tuple(type(x).from_buffer_copy(x) for x in qd) for qd in s.dirs]
        setter(d[q][k])
        return d
    assert _status(s.jvp, dirs=changed(0, lambda m: setattr(m.snow, "rho_i", float("inf")))) == BAD
    assert _status(s.jvp, dirs=changed(2, lambda m: setattr(m, "grav", float("nan")))) == BAD
    assert _status(s.vjp, dirs=changed(4, lambda m: m.large_ice.H.__setitem__(2, float("nan")))) == BAD
    for setter in (lambda m: setattr(m, "b_rho", 1e-3), lambda m: m.b.__setitem__(0, -1e-3)):
        assert _status(s.jvp, dirs=changed(3, setter)) == UNS and _status(s.vjp, dirs=changed(3, setter)) == UNS
    # a non-finite component comes before the direction on b_ρ, the flags before both
    d = changed(3, lambda m: setattr(m, "b_rho", 1e-3))
    d[0][1].cp_v = float("inf")
    assert _status(s.jvp, dirs=d) == BAD
    from cmx import _lib
    from cmx.microphysics1m import _column_products_head_1m, _ptr, _table
    ref, fam, keep, head = _column_products_head_1m(*s.structs, s.inv_dz, s.cols)
    tables = KC.tables_of(s.dirs)
    bad_tables = KC.tables_of(changed(3, lambda m: setattr(m, "b_rho", 1e-3)))
    out = torch.empty((3, 4, *s.shape), dtype=torch.float64, device=dev)
    outp = torch.empty((2, 3, s.shape[0]), dtype=torch.float64, device=dev)
    grad, ws = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(3 * _abi.CMX_PARAM_VJP_PARTIALS, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def raw(jvp_cols, rai, sno, flags=None, t=tables, use=(True,) * 5):
        fn = getattr(_lib.lib(), "cmx_mp1m_column_param_jvp_f64")
        h = list(head)
        if flags is not None:
            h[5] = flags
        with torch.cuda.device(dev):
            return fn(*h, 3, *[C.byref(x[0]) if u else None for x, u in zip(t, use)], _table(jvp_cols), _table(rai), _table(sno), None, None, None, stream)

    def raw_vjp(g, w, flags=None, t=tables):
        fn = getattr(_lib.lib(), "cmx_mp1m_column_param_vjp_f64")
        h = list(head)
        if flags is not None:
            h[5] = flags
        with torch.cuda.device(dev):
            return fn(*h, _table(s.cot), _ptr(s.pbar[0]), _ptr(s.pbar[1]), 3, *[C.byref(x[0]) for x in t], _ptr(g), _ptr(w), None, None, None, stream)
    cols = [out[d, o] for d in range(3) for o in range(4)]
    assert raw(cols, list(outp[0]), list(outp[1])) == 0 and raw_vjp(grad, ws) == 0
    flags = s.structs[0].flags
    obl, pro = _abi.CMX_1M_SED_SNOW_OBLATE, _abi.CMX_1M_SED_SNOW_PROLATE
    # both snow-shape bits, then a single one: before anything about the directions or the outputs
    assert raw([None] * 12, [None] * 3, [None] * 3, flags=flags | obl | pro, t=bad_tables) == BAD
    assert raw([None] * 12, [None] * 3, [None] * 3, flags=flags | obl, t=bad_tables) == UNS and raw_vjp(None, None, flags=flags | pro, t=bad_tables) == UNS
    # d_mp, then grad and workspace, then the outputs, then the directions' contents
    assert raw([None] * 12, [None] * 3, [None] * 3, use=(False, True, True, True, True)) == BAD
    assert raw_vjp(None, ws, t=bad_tables) == BAD and raw_vjp(grad, None, t=bad_tables) == BAD
    assert raw([None] * 12, [None] * 3, [None] * 3, t=bad_tables) == BAD                       # no output at all
    assert raw([s.cols[3]] + cols[1:], list(outp[0]), list(outp[1]), t=bad_tables) == BAD and raw(cols, [s.inv_dz] + list(outp[0])[1:], list(outp[1]), t=bad_tables) == BAD
    assert raw_vjp(s.cot[2].reshape(-1), ws, t=bad_tables) == BAD
    assert raw(cols, list(outp[0]), list(outp[1]), t=bad_tables) == UNS and raw_vjp(grad, ws, t=bad_tables) == UNS
    # d_tps, d_stokes, d_chen_rain, d_chen_ice NULL equal zero tables, bit for bit
    one = s.jvp(dirs=[{"rain_drop_size_distribution_coefficient_n0": 2.0}] * 3)
    assert raw(cols, list(outp[0]), list(outp[1]), t=KC.tables_of([P.column_parameter_direction_1m(s.structs[0], {"rain_drop_size_distribution_coefficient_n0": 2.0})] * 3),
               use=(True, False, False, False, False)) == 0
    torch.cuda.synchronize()
    assert _eq(out, one.jvp) and _eq(outp[0], one.jvp_precip_rai) and _eq(outp[1], one.jvp_precip_sno)
    # n_col = 0: CMX_OK; the gradient entry writes zeros
    empty = [c[:0].contiguous() for c in s.cols]
    assert s.jvp(cols=empty).jvp.shape == (3, 4, 0, 3)
    g = cmx.column_param_vjp_1m(*s.structs, s.inv_dz, *empty, None, None, None, s.dirs).grad
    assert g.shape == (3,) and not bool(g.any())


@pytest.mark.parametrize("ft", FTS)
def test_a_captured_call_replays_bit_identically(dev, oracle, ft):
    """One capture and replay of the jvp entry (and of the gradient entry) on a single stream reproduces the eager bits."""
    s = Setup(ft, KC.reference(MAIN_CASE, "cold", "n7"), dev, names=no_exp(MAIN_CASE)[:2] + KC.SEDIMENTATION_ONLY)
    eager_j, eager_g = s.jvp(), s.vjp()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rj, rg = s.jvp(), s.vjp()
    rj.jvp.fill_(float("nan")), rj.jvp_precip_rai.fill_(float("nan")), rj.jvp_precip_sno.fill_(float("nan")), rg.grad.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(rj.jvp, eager_j.jvp) and _eq(rj.jvp_precip_rai, eager_j.jvp_precip_rai) and _eq(rj.jvp_precip_sno, eager_j.jvp_precip_sno) and _eq(rg.grad, eager_g.grad)


# ---- torch autograd ---------------------------------------------------------------------------------------------------------------------------------
AG_NAMES = ("Chen2022_table_B1_ai[0]", "Chen2022_table_B5_Al[0]", "snow_aspect_ratio", "snow_apparent_density", "density_liquid_water",
            "rain_drop_size_distribution_coefficient_n0", "latent_heat_vaporization_at_reference", "cloud_liquid_sedimentation_number_concentration")


@pytest.mark.parametrize("ft", FTS)
def test_precipitation_and_tendency_losses_reach_theta(dev, oracle, ft):
    """theta.grad of Σ s_p·(precip_rai + precip_sno) plus a tendency loss equals column_param_vjp_1m and matches the oracle's difference quotient within the
    bound of tests/test_param_autograd_gpu.py — BOUND·Σ |ḡ|·s over the rows, the two precipitation rows included —; forward mode agrees with the jvp entry;
    without theta the function returns the bits and the state gradients it returned before."""
    ref = KC.reference(MAIN_CASE, "cold", "n7")
    s = Setup(ft, ref, dev, names=AG_NAMES)
    th0 = KC.theta(MAIN_CASE, AG_NAMES)
    theta = torch.tensor(th0, dtype=torch.float64, requires_grad=True)
    args = (*s.structs, s.inv_dz, *s.cols)
    out = cmx.autograd.column_tendencies_sedimentation_1m(*args, theta=theta, names=AG_NAMES)
    plain = cmx.autograd.column_tendencies_sedimentation_1m(*args)
    want, wr, ws = s.primal()
    for o in range(4):
        assert _eq(out[o], want[o]) and _eq(plain[o], want[o])
    assert _eq(out[4], wr) and _eq(plain[4], wr) and _eq(out[5], ws) and _eq(plain[5], ws)
    # the weights: the reference's cotangents, zero where the reference set a point or a column aside
    g = [c * _t(ref["kept"].astype(np.float64), ft, dev, s.shape) for c in s.cot]
    pb = [p * _t(ref["keptp"].astype(np.float64), ft, dev) for p in s.pbar]
    (sum((g[o] * out[o]).sum() for o in range(4)) + (pb[0] * out[4]).sum() + (pb[1] * out[5]).sum()).backward()
    direct = cmx.column_param_vjp_1m(*args, g, pb[0], pb[1], AG_NAMES).grad.cpu()
    assert theta.grad is not None and theta.grad.dtype == torch.float64 and _eq(theta.grad, direct)
    idx = [ref["names"].index(k) for k in AG_NAMES]
    gq, pq = torch.stack(g).reshape(4, -1).double().cpu().numpy(), torch.stack(pb).double().cpu().numpy()
    want_grad = (np.einsum("oi,opi->p", gq, ref["S"][:, idx]) + np.einsum("rc,rpc->p", pq, ref["Sp"][:, idx])) / th0
    bound = KC.BOUND[ft] * ((np.abs(gq) * np.abs(ref["S"]).max(axis=1)).sum() + (np.abs(pq) * np.abs(ref["Sp"]).max(axis=1)).sum()) / np.abs(th0)
    got = theta.grad.numpy()
    print(f"theta.grad {ft}: worst fraction of the bound {np.max(np.abs(got - want_grad) / bound):.3g}")
    assert (np.abs(got - want_grad) <= bound).all(), (got, want_grad, bound)
    # the state gradients with theta are those of the function without it, bit for bit
    def state_grads(**kw):
        x = [c.clone().requires_grad_(k > 0) for k, c in enumerate(s.cols)]
        o = cmx.autograd.column_tendencies_sedimentation_1m(*s.structs, s.inv_dz, *x, **kw)
        (sum((g[q] * o[q]).sum() for q in range(4)) + (pb[0] * o[4]).sum() + (pb[1] * o[5]).sum()).backward()
        return [c.grad for c in x[1:]]
    for a, b in zip(state_grads(), state_grads(theta=torch.tensor(th0, dtype=torch.float64, requires_grad=True), names=AG_NAMES)):
        assert _eq(a, b)
    # forward mode: a tangent on theta
    import torch.autograd.forward_ad as fwd
    tvec = torch.tensor(th0 * np.array([1.0, -0.5, 0.25, 2.0, 0.0, 1.5, -1.0, 0.75]), dtype=torch.float64)
    with fwd.dual_level():
        o = cmx.autograd.column_tendencies_sedimentation_1m(*args, theta=fwd.make_dual(theta.detach(), tvec), names=AG_NAMES)
        tang = [fwd.unpack_dual(x).tangent for x in o]
    r = s.jvp(dirs=[dict(zip(AG_NAMES, tvec.tolist()))])
    for q in range(4):
        assert _eq(tang[q], r.jvp[0, q])
    assert _eq(tang[4], r.jvp_precip_rai[0]) and _eq(tang[5], r.jvp_precip_sno[0])


def test_a_struct_that_the_dictionary_does_not_build_is_refused(dev, oracle):
    s = Setup("f64", KC.reference(MAIN_CASE, "cold", "n3"), dev, names=AG_NAMES)
    theta = torch.tensor(KC.theta(MAIN_CASE, AG_NAMES), dtype=torch.float64, requires_grad=True)
    mp, tps, stokes, cr, ci = s.structs
    edited = P.Chen2022VelTypeIce("f64")
    edited.large_ice.A[0] = 9.0
    with pytest.raises(ValueError, match="chen_ice"):
        cmx.autograd.column_tendencies_sedimentation_1m(mp, tps, stokes, cr, edited, s.inv_dz, *s.cols, theta=theta, names=AG_NAMES)
    with pytest.raises(ValueError, match="held fixed"):
        cmx.autograd.column_tendencies_sedimentation_1m(*s.structs, s.inv_dz, *s.cols, theta=theta[:1], names=("Chen2022_table_B1_b_rho_coeff",))
    with pytest.raises(ValueError, match="names without theta"):
        cmx.autograd.column_tendencies_sedimentation_1m(*s.structs, s.inv_dz, *s.cols, names=AG_NAMES)
