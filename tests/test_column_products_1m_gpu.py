"""J v and Jᵀḡ of the 1-moment column step with sedimentation on the device (cmx_mp1m_column_jvp_* / _vjp_*, include/cmx.h §(27); cmx.column_jvp_1m,
cmx.column_vjp_1m, cmx.autograd.column_tendencies_sedimentation_1m): the assertions of tests/test_column_products_1m_host.py through the C ABI and the
kernels — same columns, reference, measure and 1 % condition (tests/column_products_1m_cases.py) — then what only the device has: the primal entry to equal
bit for bit, tile boundaries, pointer offsets, the statuses of the entry, graph capture, torch autograd.  No shape is larger than 840 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import column_products_1m_cases as CC
from column_products_1m_cases import CASE_IDS, CASES, MAIN_CASE, WHICH
import cmx
from cmx import _abi, _lib, synthetic

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
INST, M1 = cmx.Instantaneous(), cmx.Microphysics1Moment()
Q_RAI, Q_SNO = CC.WRT.index("q_rai"), CC.WRT.index("q_sno")


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
    def __init__(self, ft, ref, dev):
        self.ft, self.ref, self.case = ft, ref, ref["case"]
        self.mp, self.tps, self.stokes, self.cr, self.ci = CC.params(ft, self.case)
        self.head = (self.mp, self.tps, self.stokes, self.cr, self.ci)
        sh = (ref["n_col"], ref["n_lev"])
        self.shape = sh
        self.inv_dz = _t(ref["inv_dz"], ft, dev)
        self.cols = [_t(c, ft, dev, sh) for c in ref["cols"]]
        self.tan = {w: _t(v, ft, dev, sh) for w, v in zip(CC.WRT, ref["v"])}
        self.cot = [_t(g, ft, dev, sh) for g in ref["g"]]
        self.pbar = [_t(p, ft, dev) for p in ref["pbar"]]

    def jvp(self, tangents=None, cols=None, inv_dz=None, **kw):
        return cmx.column_jvp_1m(*self.head, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                 self.tan if tangents is None else tangents, **kw)

    def vjp(self, cot="ref", pbar="ref", cols=None, inv_dz=None, **kw):
        pbar = self.pbar if isinstance(pbar, str) else ([None, None] if pbar is None else pbar)
        return cmx.column_vjp_1m(*self.head, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols),
                                 self.cot if isinstance(cot, str) else cot, pbar[0], pbar[1], **kw)

    def primal(self, cols=None, inv_dz=None):
        r = cmx.column_tendencies_sedimentation_1m(INST, M1, *self.head, self.inv_dz if inv_dz is None else inv_dz, *(self.cols if cols is None else cols))
        return torch.stack(list(r[:4])), torch.stack([r.precip_rai, r.precip_sno])

    def autograd(self, rho, *x, inv_dz=None):
        return cmx.autograd.column_tendencies_sedimentation_1m(*self.head, self.inv_dz if inv_dz is None else inv_dz, rho, *x)


def _flat(t):
    return t.reshape(t.shape[0], -1).cpu().numpy()


def _jp(y):
    return torch.stack([y.jvp_precip_rai, y.jvp_precip_sno])


def _pp(r):
    return torch.stack([r.precip_rai, r.precip_sno])


# ---- J v against the differenced oracle, the adjoint identity per column ---------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_products_match_the_differenced_oracle_and_are_adjoint(dev, oracle, ft, case, which):
    """Every parameter case — the compile-time and the run-time-flags instantiation, the general Γ — on the cold and the warm set; 840 points, three tile
    boundaries inside columns."""
    s = Setup(ft, CC.reference(case, which, "n7"), dev)
    y, g = s.jvp(), s.vjp()
    assert g.wrt == CC.WRT and y.tendencies is None and y.precip_rai is None and y.precip_sno is None and g.grad.shape == (6, *s.shape)
    assert y.jvp_precip_rai.shape == (s.shape[0],) and y.jvp_precip_sno.shape == (s.shape[0],)
    CC.assert_products(ft, s.ref, _flat(y.jvp), _jp(y).cpu().numpy(), _flat(g.grad), "device")


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("shape", ["n1", "n2", "n3"])
def test_small_columns(dev, oracle, ft, shape, which):
    s = Setup(ft, CC.reference(MAIN_CASE, which, shape), dev)
    y, g = s.jvp(), s.vjp()
    CC.assert_products(ft, s.ref, _flat(y.jvp), _jp(y).cpu().numpy(), _flat(g.grad), "device")


# ---- structure, exact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_a_seed_at_one_level_reaches_its_own_level_and_one_neighbour_only(dev, oracle, ft):
    """Two columns of three levels, and the columns of the 840-point set that straddle the tile boundaries 255 / 510 / 765 (columns 36, 72, 109): nothing
    crosses from the top level of column c to level 0 of column c + 1, neighbours in the flat index.  A unit cot_precip_rai touches level 0 of its column
    only, in the q_rai gradient; cot_precip_sno likewise in q_sno."""
    for shape, seeds in (("n3", [(c, k) for c in range(2) for k in range(3)]),
                         ("n7", [(35, 6), (36, 0), (36, 3), (36, 4), (72, 5), (72, 6), (73, 0), (109, 1), (109, 2), (109, 6), (110, 0)])):
        s = Setup(ft, CC.reference(MAIN_CASE, "cold", shape), dev)
        n_col, n_lev = s.shape
        for c, k in seeds:
            at = torch.zeros(s.shape, dtype=DT[ft], device=dev)
            at[c, k] = 1.0
            y = s.jvp({w: t * at for w, t in s.tan.items()})
            touched = (y.jvp != 0).any(dim=0)
            allowed = torch.zeros(s.shape, dtype=torch.bool, device=dev)
            allowed[c, max(k - 1, 0):k + 1] = True
            assert not bool((touched & ~allowed).any()) and bool(touched[c, k]) and (k == 0 or bool(touched[c, k - 1])), (shape, c, k)
            here = (torch.arange(n_col, device=dev) == c) & (k == 0)
            for r, jp in enumerate(_jp(y)):
                rains = bool(s.cols[5 + r][c, 0] > 0)          # a cell whose species was taken out sends no flux
                assert bool(((jp != 0) == (here & rains)).all()), (shape, c, k, r)
            g = s.vjp([t * at for t in s.cot], None)
            touched = (g.grad != 0).any(dim=0)
            allowed = torch.zeros(s.shape, dtype=torch.bool, device=dev)
            allowed[c, k:k + 2] = True
            assert not bool((touched & ~allowed).any()) and bool(touched[c, k]) and (k == n_lev - 1 or bool(touched[c, k + 1])), (shape, c, k)
        for r, j in ((0, Q_RAI), (1, Q_SNO)):
            c = int(np.flatnonzero(s.ref["sp"][r] > 0)[-1])      # a column that rains / snows at the surface
            pbar = [None, None]
            pbar[r] = torch.zeros(n_col, dtype=DT[ft], device=dev)
            pbar[r][c] = 1.0
            touched = s.vjp([None] * 4, pbar).grad != 0
            assert bool(touched[j, c, 0]) and int(touched.sum()) == 1, (shape, r)


@pytest.mark.parametrize("ft", FTS)
def test_j_and_its_transpose_from_unit_seeds_agree_entry_by_entry(dev, oracle, ft):
    """A column of three levels: J (14 rows, 18 columns) column by column from unit tangents and row by row from unit cotangents, within the entry bound
    B·s'_i of the input-scaled measure."""
    ref = CC.reference(MAIN_CASE, "warm", "n3")
    s = Setup(ft, ref, dev)
    n_lev = s.shape[1]
    cols = [c[:1].contiguous() for c in s.cols]
    unit = lambda k: (torch.arange(n_lev, device=dev) == k).to(DT[ft])[None].contiguous()  # noqa: E731
    one = torch.ones(1, dtype=DT[ft], device=dev)
    Jc, Jr = np.zeros((4 * n_lev + 2, 6 * n_lev)), np.zeros((4 * n_lev + 2, 6 * n_lev))
    for k in range(n_lev):
        for j, w in enumerate(CC.WRT):
            y = s.jvp({w: unit(k)}, cols=cols)
            Jc[:-2, 6 * k + j] = _flat(y.jvp).T.reshape(-1)
            Jc[-2:, 6 * k + j] = _jp(y)[:, 0].cpu().numpy()
        for q in range(4):
            Jr[4 * k + q] = _flat(s.vjp([unit(k) if i == q else None for i in range(4)], None, cols=cols).grad).T.reshape(-1)
    for r in range(2):
        Jr[-2 + r] = _flat(s.vjp([None] * 4, [one if i == r else None for i in range(2)], cols=cols).grad).T.reshape(-1)
    x = np.stack([np.asarray(c)[0] for c in ref["cols"][1:]]).T.reshape(-1)
    sc = np.concatenate([ref["s"][:, :n_lev].T.reshape(-1), ref["sp"][:, 0]])
    frac = np.abs(Jc - Jr) * np.abs(x)[None] / (CC.BOUND[ft] * sc[:, None])
    print(f"device {ft}: J from unit tangents against J from unit cotangents, worst used fraction of the entry bound {frac.max():.3g}")
    assert frac.max() < 1.0 and (Jc != 0).sum() > 50
    for k in range(n_lev):
        for m in range(n_lev):
            if m not in (k, k + 1):
                assert not Jc[4 * k:4 * k + 4, 6 * m:6 * m + 6].any() and not Jr[4 * k:4 * k + 4, 6 * m:6 * m + 6].any()
    assert not Jc[-2:, 6:].any() and not Jr[-2:, 6:].any()


# ---- bit identities --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tendencies_and_precipitation_fluxes_are_the_primal_entry(dev, oracle, ft, case):
    """On the reference columns and on a broad synthetic state (zeros, negative values, every gate), whatever is requested next to them."""
    s = Setup(ft, CC.reference(case, "cold", "n7"), dev)
    syn = [c.reshape(s.shape).contiguous() for c in synthetic.mp1m_state(s.shape[0] * s.shape[1], dtype=DT[ft], device=dev, seed=11)]
    for label, cols in (("reference", s.cols), ("synthetic", syn)):
        want, wantp = s.primal(cols)
        y = s.jvp(cols=cols, with_tendencies=True)
        assert _eq(y.tendencies, want) and _eq(_pp(y), wantp), label
        y = s.jvp({}, cols=cols, with_tendencies=True)
        assert _eq(y.tendencies, want) and _eq(_pp(y), wantp), label
        g = s.vjp(cols=cols, with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(_pp(g), wantp), label
        g = s.vjp([None, s.cot[1], None, None], None, cols=cols, wrt=CC.WRT[4:1:-1], with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(_pp(g), wantp), label
        g = s.vjp([None] * 4, None, cols=cols, wrt=(), with_tendencies=True)
        assert _eq(g.tendencies, want) and _eq(_pp(g), wantp), label


def _tab(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(s, product, dev, tables, flags=None, n_col=None, n_lev=None, mp="own", chen_ice="own", cols=None, inv_dz="own", in_table=True):
    """The status of the raw entry; tables: the pointer tables and pointers after `in`, in ABI order."""
    fam = _abi.F32 if s.ft == "f32" else _abi.F64
    cols = s.cols if cols is None else cols
    inv_dz = s.inv_dz if isinstance(inv_dz, str) else inv_dz
    mp = s.mp.c if isinstance(mp, str) else mp
    ci = s.ci if isinstance(chen_ice, str) else chen_ice
    try:
        return _lib.call(f"cmx_mp1m_column_{product}", fam, dev, C.byref(mp) if mp is not None else None, C.byref(s.tps), C.byref(s.stokes), C.byref(s.cr),
                         C.byref(ci) if ci is not None else None, s.mp.flags if flags is None else flags, s.shape[0] if n_col is None else n_col,
                         s.shape[1] if n_lev is None else n_lev, _p(inv_dz), _tab(cols) if in_table else None, *tables)
    except _lib.CmxStatusError as e:
        return e.status


@pytest.mark.parametrize("ft", FTS)
def test_a_null_member_leaves_the_other_members_unchanged(dev, oracle, ft):
    """Any output pointer may be NULL; what is written does not depend on what else is, bit for bit — a gradient's bits are independent of `wrt` —; a buffer
    that was not requested keeps its sentinel."""
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n7"), dev)
    cot = [s.cot[0], None, s.cot[2], s.cot[3]]
    full_y, full_g = s.jvp(), s.vjp(cot)
    rng = np.random.default_rng(3)
    mk = lambda k: torch.full((k, *s.shape), -7.0, dtype=DT[ft], device=dev)  # noqa: E731
    for trial in range(4):
        want = rng.random(4) < 0.5
        want[trial] = True
        got, gp = mk(4), torch.full((2, s.shape[0]), -7.0, dtype=DT[ft], device=dev)
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab([got[o] if want[o] else None for o in range(4)]), _p(gp[0]) if trial % 2 else None,
                                    None if trial % 2 else _p(gp[1]), None, None, None]) == 0
        wantg = rng.random(6) < 0.5
        wantg[trial] = True
        gotg = mk(6)
        assert _raw(s, "vjp", dev, [_tab(cot), _p(s.pbar[0]), _p(s.pbar[1]), _tab([gotg[j] if wantg[j] else None for j in range(6)]), None, None, None]) == 0
        torch.cuda.synchronize()
        for o in range(4):
            assert _eq(got[o], full_y.jvp[o]) if want[o] else bool((got[o] == -7.0).all()), (trial, o)
        for r in range(2):
            assert _eq(gp[r], _jp(full_y)[r]) if (trial % 2) == (1 - r) else bool((gp[r] == -7.0).all()), (trial, r)
        for j in range(6):
            assert _eq(gotg[j], full_g.grad[j]) if wantg[j] else bool((gotg[j] == -7.0).all()), (trial, j)
    # through the wrapper: any subset in any order
    for wrt in (("q_sno",), ("q_rai", "T"), CC.WRT[::-1]):
        g = s.vjp(cot, wrt=wrt)
        assert g.wrt == tuple(wrt) and all(_eq(g.grad[k], full_g.grad[CC.WRT.index(w)]) for k, w in enumerate(wrt)), wrt


@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_without_sedimentation_the_products_are_the_pointwise_ones(dev, oracle, ft, case):
    """inv_dz = 0: the flux terms multiply by an exact zero; J v and Jᵀḡ equal cmx.jvp_1m / cmx.vjp_1m under == (finite flux tangents)."""
    s = Setup(ft, CC.reference(case, "warm", "n7"), dev)
    zero = torch.zeros_like(s.inv_dz)
    y, g = s.jvp(inv_dz=zero), s.vjp(pbar=None, inv_dz=zero)
    py = cmx.jvp_1m(s.mp, s.tps, *s.cols, s.tan)
    pg = cmx.vjp_1m(s.mp, s.tps, *s.cols, s.cot)
    assert bool(torch.isfinite(y.jvp).all()) and bool(torch.isfinite(_jp(y)).all())
    assert bool((y.jvp == py.jvp).all()) and bool((g.grad == pg.grad).all())


@pytest.mark.parametrize("ft", FTS)
def test_results_do_not_depend_on_tile_boundaries_alignment_or_the_number_of_columns(dev, oracle, ft):
    """The same columns at other places of the launch — a call on the columns [c0, c1) of the set moves every tile boundary; one column alone; all 120 — and
    through pointers offset by 1, 2 and 3 elements: the same bits."""
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n7"), dev)
    ry, rg = s.jvp(with_tendencies=True), s.vjp(with_tendencies=True)
    for c0, c1 in ((1, 120), (5, 77), (36, 38), (0, 37), (36, 37), (119, 120)):
        cut = lambda t: t[..., c0:c1, :].contiguous()  # noqa: E731
        cutp = lambda t: t[..., c0:c1].contiguous()  # noqa: E731
        y = s.jvp({w: cut(t) for w, t in s.tan.items()}, cols=[cut(c) for c in s.cols], with_tendencies=True)
        g = s.vjp([cut(t) for t in s.cot], [cutp(p) for p in s.pbar], cols=[cut(c) for c in s.cols], with_tendencies=True)
        assert _eq(y.jvp, cut(ry.jvp)) and _eq(y.tendencies, cut(ry.tendencies)) and _eq(_jp(y), cutp(_jp(ry))) and _eq(_pp(y), cutp(_pp(ry))), (c0, c1)
        assert _eq(g.grad, cut(rg.grad)) and _eq(g.tendencies, cut(rg.tendencies)) and _eq(_pp(g), cutp(_pp(rg))), (c0, c1)
    n = s.shape[0] * s.shape[1]
    for off in (1, 2, 3):
        def shift(t):
            buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
            buf[off:] = t.reshape(-1)
            return buf[off:].view(t.shape)
        cols = [shift(c) for c in s.cols]
        assert all(c.data_ptr() % (4 * c.element_size()) == off * c.element_size() for c in cols)
        y = s.jvp({w: shift(t) for w, t in s.tan.items()}, cols=cols, inv_dz=shift(s.inv_dz), with_tendencies=True)
        g = s.vjp([shift(t) for t in s.cot], [shift(p) for p in s.pbar], cols=cols, inv_dz=shift(s.inv_dz), with_tendencies=True)
        assert _eq(y.jvp, ry.jvp) and _eq(y.tendencies, ry.tendencies) and _eq(_jp(y), _jp(ry)) and _eq(g.grad, rg.grad) and _eq(g.tendencies, rg.tendencies), off
        # … and into outputs offset the same way, with guard values on both sides
        bufs = [torch.full((off + k * n + 1,), -7.0, dtype=DT[ft], device=dev) for k in (4, 6)]
        oy, og = bufs[0][off:-1].view(4, *s.shape), bufs[1][off:-1].view(6, *s.shape)
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab(list(oy)), None, None, None, None, None]) == 0
        assert _raw(s, "vjp", dev, [_tab(s.cot), _p(s.pbar[0]), _p(s.pbar[1]), _tab(list(og)), None, None, None]) == 0
        torch.cuda.synchronize()
        assert _eq(oy, ry.jvp) and _eq(og, rg.grad) and all(bool((b[:off] == -7.0).all()) and float(b[-1]) == -7.0 for b in bufs), off


# ---- the NaN rule and the argument checks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_the_nan_rule(dev, oracle, ft):
    """A NaN in a state input, a tangent or a cotangent of a point → every output of that point; a NaN in ρ or a species' q reaches the cell below through that
    species' flux exactly as in the primal, and the precipitation outputs at level 0; a NaN in ḡ of the level below reaches x̄ through λ, ρ of the level
    below as a non-finite value.  No other point changes, bit for bit.  32 columns of 2 levels."""
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n2"), dev)
    cy, cg = s.jvp(with_tendencies=True), s.vjp(with_tendencies=True)
    top, bot = (5, 1), (5, 0)
    others = torch.ones(s.shape, dtype=torch.bool, device=dev)
    others[5] = False

    def with_nan(ts, j, at, value=float("nan")):
        ts = [t.clone() for t in ts]
        ts[j][at] = value
        return ts
    for j in range(7):
        bad = with_nan(s.cols, j, top)
        want, wantp = s.primal(bad)
        y, g = s.jvp(cols=bad, with_tendencies=True), s.vjp(cols=bad, with_tendencies=True)
        assert bool(torch.isnan(y.jvp[:, 5, 1]).all()) and bool(torch.isnan(g.grad[:, 5, 1]).all()), j
        assert _eq(y.tendencies, want) and _eq(g.tendencies, want) and _eq(_pp(y), wantp) and _eq(_pp(g), wantp), j
        assert bool((torch.isnan(y.jvp) == torch.isnan(want)).all()), j      # the flux NaN reaches the cell below in J v exactly where it does in the primal
        assert torch.isnan(want[:, 5, 0]).tolist() == [j == 0 or j == 3 + q for q in range(4)], j
        assert _eq(y.jvp[:, others], cy.jvp[:, others]) and _eq(_jp(y), _jp(cy)) and _eq(g.grad[:, others], cg.grad[:, others]), j
        bad = with_nan(s.cols, j, bot)
        y, g = s.jvp(cols=bad, with_tendencies=True), s.vjp(cols=bad)
        assert torch.isnan(_jp(y)[:, 5]).tolist() == [j in (0, 5), j in (0, 6)] and bool((torch.isnan(_pp(y)) == torch.isnan(_jp(y))).all()), j
        assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and _eq(g.grad[:, others], cg.grad[:, others]), j
        assert bool((~torch.isfinite(g.grad[2:, 5, 1])).all()) == (j == 0) and bool((~torch.isfinite(g.grad[2:, 5, 1])).any()) == (j == 0), j     # ρ of the level below enters λ of the point above
        assert _eq(g.grad[:2, 5, 1], cg.grad[:2, 5, 1]), j
    for j, w in enumerate(CC.WRT):
        y = s.jvp(dict(zip(CC.WRT, with_nan(list(s.tan.values()), j, top))), with_tendencies=True)
        assert bool(torch.isnan(y.jvp[:, 5, 1]).all()) and bool(torch.isnan(y.tendencies[:, 5, 1]).all()) and _eq(y.jvp[:, others], cy.jvp[:, others]), w
        assert torch.isnan(y.jvp[:, 5, 0]).tolist() == [j == 2 + q for q in range(4)], w      # a NaN tangent reaches Ḟ of its own species by plain IEEE arithmetic
    for q in range(4):
        g = s.vjp(with_nan(s.cot, q, bot), with_tendencies=True)
        assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and bool(torch.isnan(g.tendencies[:, 5, 0]).all()) and _eq(g.grad[:, others], cg.grad[:, others]), q
        assert torch.isnan(g.grad[:, 5, 1]).tolist() == [j == 2 + q for j in range(6)], q      # ḡ_q of the level below → λ[q] → the gradient of q_s, s = q, alone
    for r in range(2):
        pbar = [p.clone() for p in s.pbar]
        pbar[r][5] = float("nan")
        g = s.vjp(pbar=pbar)
        assert bool(torch.isnan(g.grad[:, 5, 0]).all()) and _eq(g.grad[:, 5, 1], cg.grad[:, 5, 1]) and _eq(g.grad[:, others], cg.grad[:, others]), r
    if ft == "f64":      # Float64: ρ ≤ 0 is poisoned like a NaN ρ
        bad = with_nan(s.cols, 0, top, 0.0)
        want, wantp = s.primal(bad)
        y, g = s.jvp(cols=bad, with_tendencies=True), s.vjp(cols=bad, with_tendencies=True)
        assert bool(torch.isnan(y.jvp[:, 5]).all()) and bool(torch.isnan(g.grad[:, 5, 1]).all()) and _eq(y.tendencies, want) and _eq(g.tendencies, want)


def test_argument_checks(dev, oracle):
    """The statuses of the primal entry in its order, the snow-shape bits, NULL tables, a call with no output, an output that is an input, the empty call."""
    ft = "f64"
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n3"), dev)
    BAD, UNS = _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
    n = s.shape[0] * s.shape[1]
    out4, out6, outp = torch.full((4, n), -7.0, dtype=DT[ft], device=dev), torch.full((6, n), -7.0, dtype=DT[ft], device=dev), torch.full((2, 2), -7.0, dtype=DT[ft], device=dev)
    jv = [_tab([s.tan[w] for w in CC.WRT]), _tab(list(out4)), _p(outp[0]), _p(outp[1]), None, None, None]
    vj = [_tab(s.cot), _p(s.pbar[0]), _p(s.pbar[1]), _tab(list(out6)), None, None, None]
    assert _raw(s, "jvp", dev, jv) == 0 and _raw(s, "vjp", dev, vj) == 0
    both = _abi.CMX_1M_SED_SNOW_OBLATE | _abi.CMX_1M_SED_SNOW_PROLATE
    for product, tables in (("jvp", jv), ("vjp", vj)):
        assert _raw(s, product, dev, tables, mp=None) == BAD and _raw(s, product, dev, tables, chen_ice=None) == BAD
        assert _raw(s, product, dev, tables, n_col=-1) == BAD and _raw(s, product, dev, tables, n_lev=0) == BAD
        assert _raw(s, product, dev, tables, flags=s.mp.flags | both) == BAD
        assert _raw(s, product, dev, tables, flags=s.mp.flags | (1 << 30)) == BAD                                         # an unknown option bit
        assert _raw(s, product, dev, tables, flags=s.mp.flags | _abi.CMX_1M_SED_SNOW_OBLATE) == UNS                       # the snow shapes are not built
        assert _raw(s, product, dev, tables, flags=s.mp.flags | _abi.CMX_1M_SED_SNOW_PROLATE) == UNS
        assert _raw(s, product, dev, tables, flags=(1 << 30) | _abi.CMX_1M_SED_SNOW_PROLATE) == BAD                       # the option bits are checked first
        assert _raw(s, product, dev, tables, n_col=2 ** 40, n_lev=2 ** 20) == UNS
        assert _raw(s, product, dev, tables, n_col=0) == 0 and _raw(s, product, dev, tables, n_col=0, in_table=False, inv_dz=None) == 0
        assert _raw(s, product, dev, tables, cols=s.cols[:3] + [None] + s.cols[4:]) == BAD and _raw(s, product, dev, tables, inv_dz=None) == BAD
        assert _raw(s, product, dev, tables, in_table=False) == BAD
    # no output at all
    assert _raw(s, "jvp", dev, [jv[0], None, None, None, None, None, None]) == BAD
    assert _raw(s, "jvp", dev, [jv[0], _tab([None] * 4), None, None, _tab([None] * 4), None, None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], vj[2], None, None, None, None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], vj[2], _tab([None] * 6), _tab([None] * 4), None, None]) == BAD
    # an output that is an input column, inv_dz, a tangent or a cotangent
    assert _raw(s, "jvp", dev, [jv[0], _tab([s.cols[5], None, None, None]), None, None, None, None, None]) == BAD
    assert _raw(s, "jvp", dev, [jv[0], _tab([s.tan["q_rai"], None, None, None]), None, None, None, None, None]) == BAD
    assert _raw(s, "jvp", dev, [jv[0], None, None, None, None, _p(s.inv_dz), None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], vj[2], _tab([s.cot[2]] + [None] * 5), None, None, None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], vj[2], None, None, _p(s.pbar[0]), None]) == BAD
    assert _raw(s, "vjp", dev, [vj[0], vj[1], vj[2], None, None, None, _p(s.pbar[1])]) == BAD
    # a NULL tangent table is a zero tangent, NULL cotangents no cotangent: exact zeros; only one precipitation flux requested
    out4.fill_(-7.0), out6.fill_(-7.0)
    assert _raw(s, "jvp", dev, [None, _tab(list(out4)), None, None, None, None, None]) == 0
    assert _raw(s, "vjp", dev, [None, None, None, _tab(list(out6)), None, None, None]) == 0
    precip = torch.full((2,), -7.0, dtype=DT[ft], device=dev)
    assert _raw(s, "jvp", dev, [None, None, None, None, None, None, _p(precip)]) == 0
    torch.cuda.synchronize()
    assert not bool(out4.any()) and not bool(out6.any()) and not bool(torch.signbit(out6).any()) and _eq(precip, s.primal()[1][1])
    with pytest.raises(ValueError):
        s.jvp({"rho": s.cols[0]})
    with pytest.raises(ValueError):
        s.vjp(wrt=("rho",))


# ---- autograd --------------------------------------------------------------------------------------------------------------------------------------
def _autograd_fn(s, scale, scale_p):
    """The column step as a function of RELATIVE perturbations u of the six inputs (x = x0·u), its outputs in units of the reference's row scales: every
    input and every output of order one, as torch.autograd.gradcheck needs them."""
    def fn(*u):
        x = [x0 * ui for x0, ui in zip(s.cols[1:], u)]
        out = s.autograd(s.cols[0], *x)
        return tuple(o / sc for o, sc in zip(out[:4], scale)) + tuple(o / sc for o, sc in zip(out[4:], scale_p))
    return fn


def test_gradcheck_in_float64(dev, oracle):
    """Reverse and forward mode against torch's central differences, two columns of three levels and four columns of the 7-level set (warm: no point of it is
    set aside).  Tolerance: in these units an entry is J_ij·x_j / s'_i, at most one in size; a central difference at the relative step 1e-6 carries a
    truncation error of the order of the step squared, 1e-12, and a rounding error of 2⁻⁵³ / 1e-6 ≈ 1e-10 times |out_i| / s'_i; the reference's own
    differences at 1e-6 and 4e-6 agree within 8.6e-8 summed over a stencil of up to twelve entries (tests/column_products_1m_cases.py).  1e-7 is a hundredth
    of the Float64 bound in the same units."""
    for shape, ncol in (("n3", 2), ("n7", 4)):
        ref = CC.reference(MAIN_CASE, "warm", shape)
        s = Setup("f64", ref, dev)
        s.cols = [c[:ncol].contiguous() for c in s.cols]
        n_lev = s.shape[1]
        scale = [_t(ref["s"][q].reshape(s.shape)[:ncol], "f64", dev) for q in range(4)]
        scale_p = [_t(np.where(ref["sp"][r, :ncol] > 0, ref["sp"][r, :ncol], 1.0), "f64", dev) for r in range(2)]      # a column that is dry at the surface: its flux is 0, in any unit
        u = [torch.ones((ncol, n_lev), dtype=torch.float64, device=dev, requires_grad=True) for _ in range(6)]
        assert torch.autograd.gradcheck(_autograd_fn(s, scale, scale_p), u, eps=1e-6, atol=1e-7, rtol=1e-7, check_forward_ad=True, nondet_tol=0.0)


@pytest.mark.parametrize("ft", FTS)
def test_precipitation_loss_fills_the_gradients_of_the_state(dev, oracle, ft):
    """loss = precip_rai.sum() + precip_sno.sum(): one Jᵀḡ launch fills the grads of the six differentiated inputs; at level 0 it is non-zero for q_rai and
    q_sno, above level 0 exactly zero, and it is the entry's with p̄ = 1.  The forward pass is the primal wrapper's, bit for bit; a loss over all six outputs
    is column_vjp_1m with every cotangent; forward-mode AD is column_jvp_1m."""
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n7"), dev)
    x = [c.clone().requires_grad_(True) for c in s.cols[1:]]
    out = s.autograd(s.cols[0], *x)
    want, wantp = s.primal()
    assert len(out) == 6 and all(_eq(o, w) for o, w in zip(out[:4], want)) and _eq(out[4], wantp[0]) and _eq(out[5], wantp[1])
    (out[4].sum() + out[5].sum()).backward()
    ones = torch.ones(s.shape[0], dtype=DT[ft], device=dev)
    g = s.vjp([None] * 4, [ones, ones])
    for k, xi in enumerate(x):
        assert xi.grad is not None and xi.grad.shape == s.shape and _eq(xi.grad, g.grad[k])
    for k, xi in enumerate(x):
        assert not bool(xi.grad[:, 1:].any()), CC.WRT[k]
        assert bool((xi.grad[:, 0] != 0).any()) == (k in (Q_RAI, Q_SNO)), CC.WRT[k]
    # a loss over the tendencies and both fluxes: every cotangent in one launch
    for xi in x:
        xi.grad = None
    out = s.autograd(s.cols[0], *x)
    (sum((o * c).sum() for o, c in zip(out[:4], s.cot)) + (out[4] * s.pbar[0]).sum() + (out[5] * s.pbar[1]).sum()).backward()
    g = s.vjp()
    assert all(_eq(xi.grad, g.grad[k]) for k, xi in enumerate(x))
    # a subset of the inputs: the same bits
    xr = s.cols[5].clone().requires_grad_(True)
    out = s.autograd(*s.cols[:5], xr, s.cols[6])
    (sum((o * c).sum() for o, c in zip(out[:4], s.cot)) + (out[4] * s.pbar[0]).sum() + (out[5] * s.pbar[1]).sum()).backward()
    assert _eq(xr.grad, g.grad[Q_RAI])
    import torch.autograd.forward_ad as fwAD
    with fwAD.dual_level():
        duals = [fwAD.make_dual(c, s.tan[w]) for c, w in zip(s.cols[1:], CC.WRT)]
        out = s.autograd(s.cols[0], *duals)
        tangents = [fwAD.unpack_dual(o).tangent for o in out]
    y = s.jvp()
    assert all(_eq(t, y.jvp[q]) for q, t in enumerate(tangents[:4])) and _eq(tangents[4], y.jvp_precip_rai) and _eq(tangents[5], y.jvp_precip_sno)


def test_the_gradient_of_rho_or_inv_dz_is_an_error(dev, oracle):
    s = Setup("f64", CC.reference(MAIN_CASE, "cold", "n3"), dev)
    with pytest.raises(NotImplementedError):
        s.autograd(s.cols[0].clone().requires_grad_(True), *s.cols[1:])
    with pytest.raises(NotImplementedError):
        s.autograd(*s.cols, inv_dz=s.inv_dz.clone().requires_grad_(True))


# ---- graph capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
def test_captured_calls_replay_bit_identically(dev, oracle, ft):
    """One stream, no parallel branches: both entries are pure launches (no allocation, no synchronisation)."""
    s = Setup(ft, CC.reference(MAIN_CASE, "cold", "n7"), dev)
    eager_y, eager_g = s.jvp(), s.vjp()
    oy, og = torch.empty_like(eager_y.jvp), torch.empty_like(eager_g.grad)
    op = torch.empty_like(_jp(eager_y))

    def call():
        assert _raw(s, "jvp", dev, [_tab([s.tan[w] for w in CC.WRT]), _tab(list(oy)), _p(op[0]), _p(op[1]), None, None, None]) == 0
        assert _raw(s, "vjp", dev, [_tab(s.cot), _p(s.pbar[0]), _p(s.pbar[1]), _tab(list(og)), None, None, None]) == 0
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in (oy, og, op):
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert _eq(oy, eager_y.jvp) and _eq(og, eager_g.grad) and _eq(op, _jp(eager_y))
