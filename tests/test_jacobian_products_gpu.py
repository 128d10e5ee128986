"""The products with the Jacobian on the device (cmx_sb2006_warm_rain_jvp_* / _vjp_*, cmx_mp1m_jvp_* / _vjp_*; cmx.warm_rain_jvp_2m, warm_rain_vjp_2m, jvp_1m,
vjp_1m): the assertions of tests/test_jacobian_products_host.py through the kernels — J assembled from unit-seed products through the schemes' assert_parity
(same states, finite-difference reference, bounds and 1 % condition: tests/jacobian_cases.py, tests/jacobian_1m_cases.py), the mixed-vector bounds of
tests/jacobian_products_cases.py — then the primal against the tendencies entries bit for bit, subset / NULL independence through the raw ABI, the edges of
the launch path, the NaN rule and graph capture.  Unit-seed products are COMPARED with the Jacobian entry's columns and the differences printed; equality
is asserted in the host build only (the device compiler decides per kernel which tangent terms are structural zeros, csrc/cmx_dual.hpp).  No shape is larger
than 4096 points."""
import ctypes as C

import numpy as np
import pytest
import torch

import jacobian_products_cases as PC
from jacobian_products_cases import SCHEME_CASES, SCHEMES
import cmx
from cmx import _abi, _lib, synthetic
from cmx import parameters as P

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
FTS = ["f64", "f32"]
NAMES = ["sb2006", "mp1m"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _tend_2m(mp, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *cols))[:4])


def _tend_1m(mp, tps, cols):
    return torch.stack(list(cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mp, tps, *cols)))


API = {"sb2006": dict(jvp=cmx.warm_rain_jvp_2m, vjp=cmx.warm_rain_vjp_2m, jac=cmx.warm_rain_jacobian_2m, tend=_tend_2m, stem="cmx_sb2006_warm_rain",
                      synthetic=synthetic.sb2006_state),
       "mp1m": dict(jvp=cmx.jvp_1m, vjp=cmx.vjp_1m, jac=cmx.jacobian_1m, tend=_tend_1m, stem="cmx_mp1m", synthetic=synthetic.mp1m_state)}


def _dev_cols(cols, ft, dev):
    return [torch.from_numpy(np.array(c, dtype=np.float64)).to(DT[ft]).to(dev) if c is not None else None for c in cols]      # (copies: the references are read-only)


def _eq(a, b):
    """Same bits, NaN = NaN."""
    return a.shape == b.shape and bool(torch.all((a == b) | (torch.isnan(a) & torch.isnan(b))))


def _setup(name, ft, dev, n=None):
    """(scheme, api, mp, tps, state columns, tangents dict, cotangents list) on the scheme's interior set, the first n states."""
    scheme, api = SCHEMES[name], API[name]
    case, which = scheme.INTERIOR
    cols, J_ref, _, _ = scheme.reference(case, which)
    n = cols[0].size if n is None else n
    _, v, g, *_ = PC.mixed_vectors([c[:n] for c in cols], J_ref[:, :, :n])
    return (scheme, api, scheme.params(ft, case), P.ThermodynamicsParameters(ft), _dev_cols([c[:n] for c in cols], ft, dev),
            dict(zip(scheme.WRT, _dev_cols(v, ft, dev))), _dev_cols(g, ft, dev))


# ---- parity -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name,case", SCHEME_CASES)
def test_assembled_jacobians_match_central_differences_of_the_oracle(dev, oracle, ft, name, case):
    """J column by column from six unit-tangent J v, J row by row from four unit-cotangent Jᵀḡ, each through the scheme's assert_parity (both measures, the
    same 1e-5 / 1e-3, `float32_bound` for the one exception row); then the mixed-vector bounds.  Every (case, set) of the two schemes."""
    scheme, api = SCHEMES[name], API[name]
    mp, tps = scheme.params(ft, case), P.ThermodynamicsParameters(ft)
    for which in scheme.SETS:
        ref_cols, J_ref, kept, _ = scheme.reference(case, which)
        cols = _dev_cols(ref_cols, ft, dev)
        one = torch.ones_like(cols[0])
        Jc = torch.stack([api["jvp"](mp, tps, *cols, {w: one}).jvp for w in scheme.WRT], dim=1)
        Jr = torch.stack([api["vjp"](mp, tps, *cols, [one if i == q else None for i in range(4)]).grad for q in range(4)], dim=0)
        scheme.assert_parity(ft, Jc.cpu().numpy(), case, which, "device J from J v")
        scheme.assert_parity(ft, Jr.cpu().numpy(), case, which, "device J from Jᵀḡ")
        _, v, g, *_ = PC.mixed_vectors(ref_cols, J_ref)
        y = api["jvp"](mp, tps, *cols, dict(zip(scheme.WRT, _dev_cols(v, ft, dev)))).jvp
        gr = api["vjp"](mp, tps, *cols, _dev_cols(g, ft, dev))
        assert gr.wrt == scheme.WRT and gr.tendencies is None and gr.grad.shape == (6, cols[0].numel()) and y.shape == (4, cols[0].numel())
        PC.assert_mixed(ft, y.cpu().numpy(), gr.grad.cpu().numpy(), ref_cols, J_ref, kept, f"device {name} {case} {which}")


# ---- unit seeds against the Jacobian entry: reported, not asserted ------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_unit_seed_products_against_the_jacobian_entry_are_reported(dev, oracle, ft, name):
    scheme, api, mp, tps, cols, _, _ = _setup(name, ft, dev)
    J = api["jac"](mp, tps, *cols).jac
    one = torch.ones_like(cols[0])
    Jc = torch.stack([api["jvp"](mp, tps, *cols, {w: one}).jvp for w in scheme.WRT], dim=1)
    Jr = torch.stack([api["vjp"](mp, tps, *cols, [one if i == q else None for i in range(4)]).grad for q in range(4)], dim=0)
    x = [c.cpu().numpy() for c in cols[1:]]
    for what, A in (("J v", Jc), ("Jᵀḡ", Jr)):
        differ = int((~((A == J) | (torch.isnan(A) & torch.isnan(J)))).sum())
        worst = float(PC.JC.input_scaled_error(A.cpu().numpy(), J.cpu().numpy(), x).max())
        print(f"{name} {ft}: unit-seed {what} against the Jacobian entry — {differ} of {J.numel()} elements differ in bits, worst input-scaled difference {worst:.3g}")


# ---- the primal ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_tendencies_are_bit_identical_to_the_tendencies_entry(dev, oracle, ft, name):
    """with_tendencies=True gives the columns of the tendencies entry on the same tensors, bit for bit, on the interior set and on the broad synthetic set
    (zeros, negative values, every gate) — whatever is requested next to them."""
    scheme, api, mp, tps, cols, tan, cot = _setup(name, ft, dev)
    syn = list(api["synthetic"](4096, dtype=DT[ft], device=dev))
    for label, c in (("interior", cols), ("synthetic", syn)):
        want = api["tend"](mp, tps, c)
        assert _eq(api["jvp"](mp, tps, *c, tan, with_tendencies=True).tendencies, want), label
        assert _eq(api["jvp"](mp, tps, *c, {}, with_tendencies=True).tendencies, want), label
        assert _eq(api["vjp"](mp, tps, *c, cot, with_tendencies=True).tendencies, want), label
        assert _eq(api["vjp"](mp, tps, *c, [None, cot[1], None, None], wrt=scheme.WRT[4:1:-1], with_tendencies=True).tendencies, want), label
        assert _eq(api["vjp"](mp, tps, *c, [None] * 4, wrt=(), with_tendencies=True).tendencies, want), label


# ---- subset / NULL independence through the raw ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_a_null_member_leaves_the_other_members_unchanged(dev, oracle, ft, name):
    """Any output pointer may be NULL; a column that is written does not depend on which others are, bit for bit, and a buffer that was not requested keeps
    its sentinel.  J v: the four products; Jᵀḡ: the six gradients (more than one pass at every K) with a subset of the cotangents."""
    scheme, api, mp, tps, cols, tan, cot = _setup(name, ft, dev, 257)
    fam = _abi.F32 if ft == "f32" else _abi.F64
    flags = scheme.flags(mp, scheme.INTERIOR[0])
    tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])  # noqa: E731
    state = [C.c_void_p(c.data_ptr()) for c in cols]
    full_y = api["jvp"](mp, tps, *cols, tan).jvp
    cots = [cot[0], None, cot[2], cot[3]]
    full_g = api["vjp"](mp, tps, *cols, cots).grad
    rng = np.random.default_rng(3)
    for trial in range(4):
        want = rng.random(4) < 0.5
        want[trial] = True
        got = torch.full((4, 257), -7.0, dtype=DT[ft], device=dev)
        _lib.call(api["stem"] + "_jvp", fam, dev, C.byref(mp.c), C.byref(tps), flags, 257, *state, tab([tan[w] for w in scheme.WRT]),
                  tab([got[o] if want[o] else None for o in range(4)]), None)
        wantg = rng.random(6) < 0.5
        wantg[trial] = True
        gotg = torch.full((6, 257), -7.0, dtype=DT[ft], device=dev)
        _lib.call(api["stem"] + "_vjp", fam, dev, C.byref(mp.c), C.byref(tps), flags, 257, *state, tab(cots), tab([gotg[j] if wantg[j] else None for j in range(6)]), None)
        torch.cuda.synchronize()
        for o in range(4):
            assert _eq(got[o], full_y[o]) if want[o] else bool((got[o] == -7.0).all()), (trial, o)
        for j in range(6):
            assert _eq(gotg[j], full_g[j]) if wantg[j] else bool((gotg[j] == -7.0).all()), (trial, j)


# ---- the edges of the launch path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_sizes_alignment_and_the_empty_call(dev, oracle, ft, name):
    scheme, api, mp, tps, base, tan, cot = _setup(name, ft, dev, 1000)
    ry, rg = api["jvp"](mp, tps, *base, tan, with_tendencies=True), api["vjp"](mp, tps, *base, cot, with_tendencies=True)
    shift = lambda c, n: torch.cat([c[:1], c[:n]])[1:]  # noqa: E731
    for n in (1, 63, 64, 65, 257, 1000):
        cut = lambda ts: [t[:n].contiguous() for t in ts]  # noqa: E731
        y = api["jvp"](mp, tps, *cut(base), dict(zip(scheme.WRT, cut(tan.values()))), with_tendencies=True)
        g = api["vjp"](mp, tps, *cut(base), cut(cot), with_tendencies=True)
        assert _eq(y.jvp, ry.jvp[:, :n]) and _eq(y.tendencies, ry.tendencies[:, :n]) and _eq(g.grad, rg.grad[:, :n]) and _eq(g.tendencies, rg.tendencies[:, :n]), n
        # inputs and outputs as views offset by one element: no column starts on a 16-byte boundary; guard values on both sides
        cols = [shift(c, n) for c in base]
        bufs = [torch.full((1 + k * n + 1,), -7.0, dtype=DT[ft], device=dev) for k in (4, 4, 6, 4)]
        oy, ty, og, tg = [b[1:-1].view(-1, n) for b in bufs]
        assert all(c.data_ptr() % 16 != 0 for c in cols) and all(o.data_ptr() % 16 != 0 for o in (oy, ty, og, tg))
        y = api["jvp"](mp, tps, *cols, {w: shift(t, n) for w, t in tan.items()}, with_tendencies=True, out=(oy, ty))
        g = api["vjp"](mp, tps, *cols, [shift(t, n) for t in cot], with_tendencies=True, out=(og, tg))
        assert y.jvp.data_ptr() == oy.data_ptr() and g.grad.data_ptr() == og.data_ptr()
        assert _eq(oy, ry.jvp[:, :n]) and _eq(ty, ry.tendencies[:, :n]) and _eq(og, rg.grad[:, :n]) and _eq(tg, rg.tendencies[:, :n]), n
        assert all(float(b[0]) == float(b[-1]) == -7.0 for b in bufs), n      # nothing written outside the columns
    # n = 0 returns without touching memory
    guard = torch.full((8,), -7.0, dtype=DT[ft], device=dev)
    empty = [guard[4:4] for _ in range(7)]
    y = api["jvp"](mp, tps, *empty, {scheme.WRT[0]: guard[4:4]}, with_tendencies=True, out=(guard[4:4].view(4, 0), guard[4:4].view(4, 0)))
    g = api["vjp"](mp, tps, *empty, [guard[4:4]] * 4, with_tendencies=True, out=(guard[4:4].view(6, 0), guard[4:4].view(4, 0)))
    torch.cuda.synchronize()
    assert y.jvp.numel() == 0 and g.grad.numel() == 0 and bool((guard == -7.0).all())


# ---- the NaN rule -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_a_nan_poisons_every_output_of_its_point_only(dev, oracle, ft, name):
    """One point of 130, every state column, every tangent column and every cotangent column."""
    scheme, api, mp, tps, cols, tan, cot = _setup(name, ft, dev, 130)
    cy, cg = api["jvp"](mp, tps, *cols, tan, with_tendencies=True), api["vjp"](mp, tps, *cols, cot, with_tendencies=True)
    others = torch.arange(130, device=dev) != 77

    def poisoned(r, clean, what):
        for a, b in zip(r[:2], clean[:2]):
            assert bool(torch.isnan(a[:, 77]).all()) and _eq(a[:, others], b[:, others]), what

    def with_nan(ts, j):
        ts = [t.clone() for t in ts]
        ts[j][77] = float("nan")
        return ts
    for j in range(7):
        bad = with_nan(cols, j)
        poisoned(api["jvp"](mp, tps, *bad, tan, with_tendencies=True), cy, ("state", j, "jvp"))
        poisoned(api["vjp"](mp, tps, *bad, cot, with_tendencies=True), cg, ("state", j, "vjp"))
    for j in range(6):
        bad = dict(zip(scheme.WRT, with_nan(list(tan.values()), j)))
        poisoned(api["jvp"](mp, tps, *cols, bad, with_tendencies=True), cy, ("tangent", j))
    for q in range(4):
        poisoned(api["vjp"](mp, tps, *cols, with_nan(cot, q), with_tendencies=True), cg, ("cotangent", q))


# ---- graph capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", FTS)
@pytest.mark.parametrize("name", NAMES)
def test_captured_calls_replay_bit_identically(dev, oracle, ft, name):
    """One stream, no parallel branches: both entries are pure launch sequences (no allocation, no synchronisation)."""
    scheme, api, mp, tps, cols, tan, cot = _setup(name, ft, dev, 1000)
    mk = lambda k: torch.empty((k, 1000), dtype=DT[ft], device=dev)  # noqa: E731
    out = [mk(4), mk(4), mk(6), mk(4)]

    def call():
        api["jvp"](mp, tps, *cols, tan, with_tendencies=True, out=(out[0], out[1]))
        api["vjp"](mp, tps, *cols, cot, with_tendencies=True, out=(out[2], out[3]))
    call()
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in out:
        o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(_eq(o, e) for o, e in zip(out, eager))
    # new state in the captured columns: the replay follows it and equals an eager call on the same memory
    for c in cols:
        c.copy_(c.flip(0))
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in out]
    assert not _eq(replayed[0], eager[0]) and not _eq(replayed[2], eager[2])
    call()
    torch.cuda.synchronize()
    assert all(_eq(o, r) for o, r in zip(out, replayed))
