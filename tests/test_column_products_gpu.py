"""J v and Jᵀḡ of the SB2006 column step with sedimentation on the device (cmx_sb2006_column_jvp_* / _vjp_*, include/cmx.h §(25); cmx.column_jvp_2m,
cmx.column_vjp_2m, cmx.autograd.column_tendencies_sedimentation_2m): the assertions of tests/test_column_products_host.py through the C ABI and the kernels —
same columns, reference, measure and 1 % condition (tests/column_products_cases.py) — then what only the device has: the primal entry to equal bit for bit,
tile boundaries, pointer offsets, the statuses of the entry, torch autograd.  No shape is larger than 840 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import column_products_cases as CC
from column_products_cases import CASE_IDS, CASES, MAIN_CASE
import cmx
from cmx import _abi, _lib, synthetic
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
VEL = {"sb": cmx.SB2006VelType, "chen": cmx.Chen2022VelTypeRain, "chen_gen": cmx.Chen2022VelTypeRain}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, ft, dev, shape=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, dtype=np.float64)).to(DT[ft]).to(dev)      # (a copy: the references are read-only)
    return t.reshape(shape).contiguous() if shape is not None else t


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


class Setup:
    """The parameters of a case in one float type and a reference's columns, tangents and cotangents on the device."""
    def __init__(self, ft, ref, dev, case=None):
        self.ft, self.ref, self.case = ft, ref, ref["case"] if case is None else case
        self.wr, self.tps, self.velp, self.stokes = CC.params(ft, self.case)
        self.kw = dict(vel=VEL[self.case[1]], vel_params=self.velp, cloud_vel=self.stokes)
        sh = (ref["n_col"], ref["n_lev"])
        self.shape = sh
        self.inv_dz = _t(ref["inv_dz"], ft, dev)
        self.cols = [_t(c, ft, dev, sh) for c in ref["cols"]]
        self.tan = {w: _t(v, ft, dev, sh) for w, v in zip(CC.WRT, ref["v"])}
        self.cot = [_t(g, ft, dev, sh) for g in ref["g"]]
        self.pbar = _t(ref["pbar"], ft, dev)

    def jvp(self, tangents=None, cols=None, inv_dz=None, **kw):
        return cmx.column_jvp_2m(self.wr, self.tps, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                 self.tan if tangents is None else tangents, **kw, **self.kw)

    def vjp(self, cot="ref", pbar="ref", cols=None, inv_dz=None, **kw):
        return cmx.column_vjp_2m(self.wr, self.tps, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                 self.cot if isinstance(cot, str) else cot, self.pbar if isinstance(pbar, str) else pbar, **kw, **self.kw)

    def primal(self, cols=None, inv_dz=None):
        r = cmx.column_tendencies_sedimentation(self.wr, self.tps, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                                want_precip_flux=True, **self.kw)
        return torch.stack(list(r[:4])), r.precip_flux


def _flat(t):
    return t.reshape(t.shape[0], -1).cpu().numpy()


# ---- 1, 2: J v against the differenced oracle, the adjoint identity per column ---------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_products_match_the_differenced_oracle_and_are_adjoint(dev, oracle, ft, case):
    """LIMITED on and off, every velocity kind (chen_gen: a table that make_chen_log rejects), cloud sedimentation on and off; 840 points, three tile
    boundaries inside columns."""
    s = Setup(ft, CC.reference(case, "n7"), dev)
    y, g = s.jvp(), s.vjp()
    assert g.wrt == CC.WRT and y.tendencies is None and y.precip_flux is None and g.grad.shape == (6, *s.shape) and y.jvp_precip.shape == (s.shape[0],)
    CC.assert_products(ft, s.ref, _flat(y.jvp), y.jvp_precip.cpu().numpy(), _flat(g.grad), "device")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("shape", ["n1", "n2", "n3"])
def test_small_columns(dev, oracle, ft, shape):
    s = Setup(ft, CC.reference(MAIN_CASE, shape), dev)
    y, g = s.jvp(), s.vjp()
    CC.assert_products(ft, s.ref, _flat(y.jvp), y.jvp_precip.cpu().numpy(), _flat(g.grad), "device")


# ---- 3: structure, exact ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_a_seed_at_one_level_reaches_its_own_level_and_one_neighbour_only(dev, oracle, ft):
    """Two columns of three levels, and the two columns of the 840-point set that straddle a tile boundary: nothing crosses from the top level of column c to
    level 0 of column c + 1, neighbours in the flat index."""
    for shape, seeds in (("n3", [(c, k) for c in range(2) for k in range(3)]), ("n7", [(35, 6), (36, 0), (36, 3), (36, 4), (72, 5), (72, 6)])):
        s = Setup(ft, CC.reference(MAIN_CASE, shape), dev)
        n_col, n_lev = s.shape
        for c, k in seeds:
            at = torch.zeros(s.shape, dtype=DT[ft], device=dev)
            at[c, k] = 1.0
            y = s.jvp({w: t * at for w, t in s.tan.items()})
            touched = (y.jvp != 0).any(dim=0)
            allowed = torch.zeros(s.shape, dtype=torch.bool, device=dev)
            allowed[c, max(k - 1, 0):k + 1] = True
            assert not bool((touched & ~allowed).any()) and bool(touched[c, k]) and (k == 0 or bool(touched[c, k - 1])), (shape, c, k)
            assert bool(((y.jvp_precip != 0) == ((torch.arange(n_col, device=dev) == c) & (k == 0))).all()), (shape, c, k)
            g = s.vjp([t * at for t in s.cot], None)
            touched = (g.grad != 0).any(dim=0)
            allowed = torch.zeros(s.shape, dtype=torch.bool, device=dev)
            allowed[c, k:k + 2] = True
            assert not bool((touched & ~allowed).any()) and bool(touched[c, k]) and (k == n_lev - 1 or bool(touched[c, k + 1])), (shape, c, k)
        c = int(np.flatnonzero(s.ref["sp"] > 0)[-1])      # a column that rains at the surface
        pbar = torch.zeros(n_col, dtype=DT[ft], device=dev)
        pbar[c] = 1.0
        touched = (s.vjp([None] * 4, pbar).grad != 0).any(dim=0)
        assert bool(touched[c, 0]) and int(touched.sum()) == 1, shape


@pytest.mark.parametrize("ft", FTS)
def test_j_and_its_transpose_from_unit_seeds_agree_entry_by_entry(dev, oracle, ft):
    """A column of three levels: J (13 rows, 18 columns) column by column from unit tangents and row by row from unit cotangents, within the entry bound
    B·s'_i of the input-scaled measure."""
    ref = CC.reference(MAIN_CASE, "n3")
    s = Setup(ft, ref, dev)
    n_lev = s.shape[1]
    cols = [c[:1].contiguous() for c in s.cols]
    unit = lambda k: (torch.arange(n_lev, device=dev) == k).to(DT[ft])[None].contiguous()  # noqa: E731
    Jc, Jr = np.zeros((4 * n_lev + 1, 6 * n_lev)), np.zeros((4 * n_lev + 1, 6 * n_lev))
    for k in range(n_lev):
        for j, w in enumerate(CC.WRT):
            y = s.jvp({w: unit(k)}, cols=cols)
            Jc[:-1, 6 * k + j] = _flat(y.jvp).T.reshape(-1)
            Jc[-1, 6 * k + j] = float(y.jvp_precip[0])
        for q in range(4):
            Jr[4 * k + q] = _flat(s.vjp([unit(k) if i == q else None for i in range(4)], None, cols=cols).grad).T.reshape(-1)
    Jr[-1] = _flat(s.vjp([None] * 4, torch.ones(1, dtype=DT[ft], device=dev), cols=cols).grad).T.reshape(-1)
    x = np.stack([np.asarray(c)[0] for c in ref["cols"][1:]]).T.reshape(-1)
    sc = np.concatenate([ref["s"][:, :n_lev].T.reshape(-1), ref["sp"][:1]])
    frac = np.abs(Jc - Jr) * np.abs(x)[None] / (CC.BOUND[ft] * sc[:, None])
    print(f"device {ft}: J from unit tangents against J from unit cotangents, worst used fraction of the entry bound {frac.max():.3g}")
    assert frac.max() < 1.0 and (Jc != 0).sum() > 50
    for k in range(n_lev):
        for m in range(n_lev):
            if m not in (k, k + 1):
                assert not Jc[4 * k:4 * k + 4, 6 * m:6 * m + 6].any() and not Jr[4 * k:4 * k + 4, 6 * m:6 * m + 6].any()
    assert not Jc[-1, 6:].any() and not Jr[-1, 6:].any()


# ---- 4: bit identities -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tendencies_and_precipitation_flux_are_the_primal_entry(dev, oracle, ft, case):
    """On the interior columns and on a broad synthetic state (zeros, negative values, every gate), whatever is requested next to them."""
    s = Setup(ft, CC.reference(case, "n7"), dev)
    syn = [c.reshape(s.shape).contiguous() for c in synthetic.sb2006_state(s.shape[0] * s.shape[1], dtype=DT[ft], device=dev, seed=11)]
    for label, cols in (("interior", s.cols), ("synthetic", syn)):
        want, wantp = s.primal(cols)
        y = s.jvp(cols=cols, with_tendencies=True)
        assert _eq(y.tendencies, want) and _eq(y.precip_flux, wantp), label
        y = s.jvp({}, cols=cols, with_tendencies=True)
        assert _eq(y.tendencies, want) and _eq(y.precip_flux, wantp), label
        g = s.vjp(cols=cols, with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(g.precip_flux, wantp), label
        g = s.vjp([None, s.cot[1], None, None], None, cols=cols, wrt=CC.WRT[4:1:-1], with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(g.precip_flux, wantp), label
        g = s.vjp([None] * 4, None, cols=cols, wrt=(), with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(g.precip_flux, wantp), label


def _raw(s, product, dev, tables, extra=()):
    """The status of the raw entry; tables: the pointer tables and pointers after the state columns, in ABI order."""
    fam = _abi.F32 if s.ft == "f32" else _abi.F64
    try:
        return _lib.call(f"cmx_sb2006_column_{product}", fam, dev, C.byref(s.wr.c), C.byref(s.tps), C.byref(s.velp), C.byref(s.stokes) if s.stokes is not None else None,
                         CC.flags(s.case), s.shape[0], s.shape[1], C.c_void_p(s.inv_dz.data_ptr()), *[C.c_void_p(c.data_ptr()) for c in s.cols], *tables)
    except _lib.CmxStatusError as e:
        return e.status


def _tab(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("ft", FTS)
def test_a_null_member_leaves_the_other_members_unchanged(dev, oracle, ft):
    """Any output pointer may be NULL; what is written does not depend on what else is, bit for bit; a buffer that was not requested keeps its sentinel."""
    s = Setup(ft, CC.reference(MAIN_CASE, "n7"), dev)
    full_y, full_g = s.jvp(), s.vjp([s.cot[0], None, s.cot[2], s.cot[3]])
    rng = np.random.default_rng(3)
    mk = lambda k: torch.full((k, *s.shape), -7.0, dtype=DT[ft], device=dev)  # noqa: E731
    for trial in range(4):
        want = rng.random(4) < 0.5
        want[trial] = True
        got, gp = mk(4), torch.full((s.shape[0],), -7.0, dtype=DT[ft], device=dev)
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab([got[o] if want[o] else None for o in range(4)]), _p(gp) if trial % 2 else None,
                                    None, None]) == 0
        wantg = rng.random(6) < 0.5
        wantg[trial] = True
        gotg = mk(6)
        assert _raw(s, "vjp", dev, [_tab([s.cot[0], None, s.cot[2], s.cot[3]]), _p(s.pbar), _tab([gotg[j] if wantg[j] else None for j in range(6)]), None, None]) == 0
        torch.cuda.synchronize()
        for o in range(4):
            assert _eq(got[o], full_y.jvp[o]) if want[o] else bool((got[o] == -7.0).all()), (trial, o)
        assert _eq(gp, full_y.jvp_precip) if trial % 2 else bool((gp == -7.0).all()), trial
        for j in range(6):
            assert _eq(gotg[j], full_g.grad[j]) if wantg[j] else bool((gotg[j] == -7.0).all()), (trial, j)


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("cloud", [False, True])
def test_without_sedimentation_the_products_are_the_pointwise_ones(dev, oracle, ft, cloud):
    """inv_dz = 0: the flux terms multiply by an exact zero; J v and Jᵀḡ equal cmx.warm_rain_jvp_2m / warm_rain_vjp_2m under == (finite flux tangents)."""
    s = Setup(ft, CC.reference((True, "sb", cloud), "n7"), dev)
    zero = torch.zeros_like(s.inv_dz)
    y, g = s.jvp(inv_dz=zero), s.vjp(pbar=None, inv_dz=zero)
    py = cmx.warm_rain_jvp_2m(s.wr, s.tps, *s.cols, s.tan)
    pg = cmx.warm_rain_vjp_2m(s.wr, s.tps, *s.cols, s.cot)
    assert bool(torch.isfinite(y.jvp).all()) and bool(torch.isfinite(y.jvp_precip).all())
    assert bool((y.jvp == py.jvp).all()) and bool((g.grad == pg.grad).all())


@pytest.mark.parametrize("ft", FTS)
def test_results_do_not_depend_on_tile_boundaries_or_alignment(dev, oracle, ft):
    """The same columns at other places of the launch — a call on the columns [c0, c1) of the set moves every tile boundary — and through pointers offset by
    1, 2 and 3 elements: the same bits."""
    s = Setup(ft, CC.reference(MAIN_CASE, "n7"), dev)
    ry, rg = s.jvp(with_tendencies=True), s.vjp(with_tendencies=True)
    for c0, c1 in ((1, 120), (5, 77), (36, 38), (0, 37)):
        cut = lambda t: t[..., c0:c1, :].contiguous()  # noqa: E731
        y = s.jvp({w: cut(t) for w, t in s.tan.items()}, cols=[cut(c) for c in s.cols], with_tendencies=True)
        g = s.vjp([cut(t) for t in s.cot], s.pbar[c0:c1].contiguous(), cols=[cut(c) for c in s.cols], with_tendencies=True)
        assert _eq(y.jvp, cut(ry.jvp)) and _eq(y.tendencies, cut(ry.tendencies)) and _eq(y.jvp_precip, ry.jvp_precip[c0:c1]) and _eq(y.precip_flux, ry.precip_flux[c0:c1]), (c0, c1)
        assert _eq(g.grad, cut(rg.grad)) and _eq(g.tendencies, cut(rg.tendencies)) and _eq(g.precip_flux, rg.precip_flux[c0:c1]), (c0, c1)
    n = s.shape[0] * s.shape[1]
    for off in (1, 2, 3):
        def shift(t):
            buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
            buf[off:] = t.reshape(-1)
            return buf[off:].view(t.shape)
        cols = [shift(c) for c in s.cols]
        assert all(c.data_ptr() % (4 * c.element_size()) == off * c.element_size() for c in cols)
        y = s.jvp({w: shift(t) for w, t in s.tan.items()}, cols=cols, inv_dz=shift(s.inv_dz), with_tendencies=True)
        g = s.vjp([shift(t) for t in s.cot], shift(s.pbar), cols=cols, inv_dz=shift(s.inv_dz), with_tendencies=True)
        assert _eq(y.jvp, ry.jvp) and _eq(y.tendencies, ry.tendencies) and _eq(y.jvp_precip, ry.jvp_precip) and _eq(g.grad, rg.grad) and _eq(g.tendencies, rg.tendencies), off
        # … and into outputs offset the same way, with guard values on both sides
        bufs = [torch.full((off + k * n + 1,), -7.0, dtype=DT[ft], device=dev) for k in (4, 6)]
        oy, og = bufs[0][off:-1].view(4, *s.shape), bufs[1][off:-1].view(6, *s.shape)
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab(list(oy)), None, None, None]) == 0
        assert _raw(s, "vjp", dev, [_tab(s.cot), _p(s.pbar), _tab(list(og)), None, None]) == 0
        torch.cuda.synchronize()
        assert _eq(oy, ry.jvp) and _eq(og, rg.grad) and all(bool((b[:off] == -7.0).all()) and float(b[-1]) == -7.0 for b in bufs), off


# ---- 5: the NaN rule and the argument checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(dev, oracle, ft):
    """A NaN in a state input, a tangent or a cotangent of a point → every output of that point; a NaN in an input of the fluxes reaches the cell below exactly
    as in the primal; a NaN in ḡ or ρ of the level below reaches x̄ through λ.  No other point changes, bit for bit.  32 columns of 2 levels."""
    s = Setup(ft, CC.reference(MAIN_CASE, "n2"), dev)
    cy, cg = s.jvp(with_tendencies=True), s.vjp(with_tendencies=True)
    top, bot = (5, 1), (5, 0)
    others = torch.ones(s.shape, dtype=torch.bool, device=dev)
    others[5] = False

    def with_nan(ts, j, at):
        ts = [t.clone() for t in ts]
        ts[j][at] = float("nan")
        return ts
    for j in range(7):
        bad = with_nan(s.cols, j, top)
        want, wantp = s.primal(bad)
        y, g = s.jvp(cols=bad, with_tendencies=True), s.vjp(cols=bad, with_tendencies=True)
        assert bool(torch.isnan(y.jvp[:, 5, 1]).all()) and bool(torch.isnan(g.grad[:, 5, 1]).all()), j
        assert _eq(y.tendencies, want) and _eq(g.tendencies, want) and _eq(y.precip_flux, wantp) and _eq(g.precip_flux, wantp), j
        assert bool((torch.isnan(y.jvp) == torch.isnan(want)).all()), j      # the flux NaN reaches the cell below in J v exactly where it does in the primal
        assert bool(torch.isnan(want[:, 5, 0]).any()) == (j in (0, 3, 4, 5, 6)), j
        assert _eq(y.jvp[:, others], cy.jvp[:, others]) and _eq(y.jvp_precip, cy.jvp_precip) and _eq(g.grad[:, others], cg.grad[:, others]), j
        bad = with_nan(s.cols, j, bot)
        g = s.vjp(cols=bad)
        assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and _eq(g.grad[:, others], cg.grad[:, others]), j
        assert bool(torch.isnan(g.grad[2:, 5, 1]).any()) == (j == 0), j     # ρ of the level below enters λ of the point above
    for j, w in enumerate(CC.WRT):
        y = s.jvp(dict(zip(CC.WRT, with_nan(list(s.tan.values()), j, top))), with_tendencies=True)
        assert bool(torch.isnan(y.jvp[:, 5, 1]).all()) and bool(torch.isnan(y.tendencies[:, 5, 1]).all()) and _eq(y.jvp[:, others], cy.jvp[:, others]), w
    for q in range(4):
        g = s.vjp(with_nan(s.cot, q, bot), with_tendencies=True)
        assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and bool(torch.isnan(g.tendencies[:, 5, 0]).all()) and _eq(g.grad[:, others], cg.grad[:, others]), q
        assert bool(torch.isnan(g.grad[2:, 5, 1]).all()) and _eq(g.grad[:2, 5, 1], cg.grad[:2, 5, 1]), q      # T and q_tot do not enter the fluxes
    pbar = s.pbar.clone()
    pbar[5] = float("nan")
    g = s.vjp(pbar=pbar)
    assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and _eq(g.grad[:, 5, 1], cg.grad[:, 5, 1]) and _eq(g.grad[:, others], cg.grad[:, others])


def test_argument_checks(dev, oracle):
    """The statuses of the primal entry in its order, NULL tables, a call with no output, an output that is an input, the empty call."""
    ft = "f64"
    s = Setup(ft, CC.reference(MAIN_CASE, "n3"), dev)
    BAD = _abi.CMX_ERR_BAD_ARG
    n = s.shape[0] * s.shape[1]
    out4, out6, outp = torch.full((4, n), -7.0, dtype=DT[ft], device=dev), torch.full((6, n), -7.0, dtype=DT[ft], device=dev), torch.full((2,), -7.0, dtype=DT[ft], device=dev)
    jv = [_tab([s.tan[w] for w in CC.WRT]), _tab(list(out4)), _p(outp), None, None]
    vj = [_tab(s.cot), _p(s.pbar), _tab(list(out6)), None, None]
    assert _raw(s, "jvp", dev, jv) == 0 and _raw(s, "vjp", dev, vj) == 0
    fam = _abi.F64

    def status(product, tables, flags=None, n_col=None, n_lev=None, wr=s.wr.c, vel=s.velp, cols=None, inv_dz=s.inv_dz):
        try:
            return _lib.call(f"cmx_sb2006_column_{product}", fam, dev, C.byref(wr) if wr is not None else None, C.byref(s.tps), C.byref(vel) if vel is not None else None,
                             C.byref(s.stokes), CC.flags(s.case) if flags is None else flags, s.shape[0] if n_col is None else n_col, s.shape[1] if n_lev is None else n_lev,
                             _p(inv_dz), *[_p(c) for c in (s.cols if cols is None else cols)], *tables)
        except _lib.CmxStatusError as e:
            return e.status
    for product, tables in (("jvp", jv), ("vjp", vj)):
        assert status(product, tables, wr=None) == BAD and status(product, tables, vel=None) == BAD
        assert status(product, tables, n_col=-1) == BAD and status(product, tables, n_lev=0) == BAD
        assert status(product, tables, flags=_abi.CMX_SB2006_LIMITED) == BAD                                              # no fall-speed scheme
        assert status(product, tables, flags=_abi.CMX_SB2006_LIMITED | _abi.CMX_VEL_SB2006 | _abi.CMX_VEL_CHEN2022) == BAD      # both
        assert status(product, tables, flags=CC.flags(s.case) | (1 << 9)) == BAD                                          # an unknown bit
        assert status(product, tables, n_col=2 ** 40, n_lev=2 ** 20) == _abi.CMX_ERR_UNSUPPORTED
        assert status(product, tables, n_col=0) == 0
        assert status(product, tables, cols=s.cols[:3] + [None] + s.cols[4:]) == BAD and status(product, tables, inv_dz=None) == BAD
        assert status(product, tables, wr=P.WarmRainParams2M(ft, False).c) == BAD                                         # the limited variant of a struct without limiters
    # no output at all
    assert _raw(s, "jvp", dev, [jv[0], None, None, None, None]) == BAD and _raw(s, "jvp", dev, [jv[0], _tab([None] * 4), None, _tab([None] * 4), None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], None, None, None]) == BAD and _raw(s, "vjp", dev, [vj[0], vj[1], _tab([None] * 6), _tab([None] * 4), None]) == BAD
    # an output that is an input column, a tangent or a cotangent
    assert _raw(s, "jvp", dev, [jv[0], _tab([s.cols[5], None, None, None]), None, None, None]) == BAD
    assert _raw(s, "jvp", dev, [jv[0], _tab([s.tan["q_rai"], None, None, None]), None, None, None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], _tab([s.cot[2]] + [None] * 5), None, None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], None, None, _p(s.pbar)]) == BAD
    # a NULL tangent table is a zero tangent, NULL cotangents no cotangent: exact zeros; only the precipitation flux requested
    out4.fill_(-7.0), out6.fill_(-7.0)
    assert _raw(s, "jvp", dev, [None, _tab(list(out4)), None, None, None]) == 0 and _raw(s, "vjp", dev, [None, None, _tab(list(out6)), None, None]) == 0
    precip = torch.full((2,), -7.0, dtype=DT[ft], device=dev)
    assert _raw(s, "jvp", dev, [None, None, None, None, _p(precip)]) == 0
    torch.cuda.synchronize()
    assert not bool(out4.any()) and not bool(out6.any()) and not bool(torch.signbit(out6).any()) and _eq(precip, s.primal()[1])
    with pytest.raises(ValueError):
        s.jvp({"rho": s.cols[0]})
    with pytest.raises(ValueError):
        s.vjp(wrt=("rho",))


# ---- 6: autograd -----------------------------------------------------------------------------------------------------------------------------------
def _autograd_fn(s, scale, scale_p):
    """The column step as a function of RELATIVE perturbations u of the six inputs (x = x0·u), its outputs in units of the reference's row scales: every
    input and every output of order one, as torch.autograd.gradcheck needs them."""
    def fn(*u):
        x = [x0 * ui for x0, ui in zip(s.cols[1:], u)]
        out = cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, s.cols[0], *x, **s.kw)
        return tuple(o / sc for o, sc in zip(out[:4], scale)) + (out[4] / scale_p,)
    return fn


def test_gradcheck_in_float64(dev, oracle):
    """Reverse and forward mode against torch's central differences, two columns of three levels and four columns of the 7-level set.  Tolerance: the
    differences of step 1e-6 in the relative perturbation agree with those of 4e-6 within 1.5e-9 of a row's scale on these columns (the reference's own
    criterion, tests/column_products_cases.py); 1e-7 leaves a factor of 60 and is a hundredth of the Float64 bound."""
    for shape, ncol in (("n3", 2), ("n7", 4)):
        ref = CC.reference(MAIN_CASE, shape)
        s = Setup("f64", ref, dev)
        s.cols = [c[:ncol].contiguous() for c in s.cols]
        n_lev = s.shape[1]
        scale = [_t(ref["s"][q].reshape(s.shape)[:ncol], "f64", dev) for q in range(4)]
        scale_p = _t(np.where(ref["sp"][:ncol] > 0, ref["sp"][:ncol], 1.0), "f64", dev)      # a column that is dry at the surface: its flux is 0, in any unit
        u = [torch.ones((ncol, n_lev), dtype=torch.float64, device=dev, requires_grad=True) for _ in range(6)]
        assert torch.autograd.gradcheck(_autograd_fn(s, scale, scale_p), u, eps=1e-6, atol=1e-7, rtol=1e-7, check_forward_ad=True, nondet_tol=0.0)


@pytest.mark.parametrize("ft", FTS)
def test_precipitation_loss_fills_the_gradients_of_the_rain_columns(dev, oracle, ft):
    """loss = precip_flux.sum(): one Jᵀḡ launch; only level 0 receives a gradient, and it is the entry's with p̄ = 1.  The forward pass is the primal entry,
    bit for bit; forward-mode AD is the J v entry."""
    s = Setup(ft, CC.reference(MAIN_CASE, "n7"), dev)
    x = [c.clone().requires_grad_(True) for c in s.cols[1:]]
    out = cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, s.cols[0], *x, **s.kw)
    want, wantp = s.primal()
    assert all(_eq(o, w) for o, w in zip(out[:4], want)) and _eq(out[4], wantp)
    out[4].sum().backward()
    g = s.vjp([None] * 4, torch.ones_like(s.pbar))
    for k, xi in enumerate(x):
        assert xi.grad is not None and _eq(xi.grad, g.grad[k])
    q_rai, n_rai = x[4].grad, x[5].grad
    assert bool((q_rai[:, 0] != 0).any()) and bool((n_rai[:, 0] != 0).any()) and not bool(q_rai[:, 1:].any()) and not bool(x[0].grad.any())
    # a loss over the tendencies and the flux: every cotangent in one launch
    for xi in x:
        xi.grad = None
    out = cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, s.cols[0], *x, **s.kw)
    (sum((o * c).sum() for o, c in zip(out[:4], s.cot)) + (out[4] * s.pbar).sum()).backward()
    g = s.vjp()
    assert all(_eq(xi.grad, g.grad[k]) for k, xi in enumerate(x))
    import torch.autograd.forward_ad as fwAD
    with fwAD.dual_level():
        duals = [fwAD.make_dual(c, s.tan[w]) for c, w in zip(s.cols[1:], CC.WRT)]
        out = cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, s.cols[0], *duals, **s.kw)
        tangents = [fwAD.unpack_dual(o).tangent for o in out]
    y = s.jvp()
    assert all(_eq(t, y.jvp[q]) for q, t in enumerate(tangents[:4])) and _eq(tangents[4], y.jvp_precip)


def test_the_gradient_of_rho_or_inv_dz_is_an_error(dev, oracle):
    s = Setup("f64", CC.reference(MAIN_CASE, "n3"), dev)
    with pytest.raises(NotImplementedError):
        cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz, s.cols[0].clone().requires_grad_(True), *s.cols[1:], **s.kw)
    with pytest.raises(NotImplementedError):
        cmx.autograd.column_tendencies_sedimentation_2m(s.wr, s.tps, s.inv_dz.clone().requires_grad_(True), *s.cols, **s.kw)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_captured_calls_replay_bit_identically(dev, oracle, ft):
    """One stream, no parallel branches: both entries are pure launches (no allocation, no synchronisation)."""
    s = Setup(ft, CC.reference(MAIN_CASE, "n7"), dev)
    eager_y, eager_g = s.jvp(), s.vjp()
    oy, og = torch.empty_like(eager_y.jvp), torch.empty_like(eager_g.grad)
    op = torch.empty_like(eager_y.jvp_precip)

    def call():
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab(list(oy)), _p(op), None, None]) == 0
        assert _raw(s, "vjp", dev, [_tab(s.cot), _p(s.pbar), _tab(list(og)), None, None]) == 0
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in (oy, og, op):
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(oy, eager_y.jvp) and _eq(og, eager_g.grad) and _eq(op, eager_y.jvp_precip)
