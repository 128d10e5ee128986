"""The ensemble forms of the implicit column steps (include/cmx.h §29, continuation) on the GPU.  The contract is EQUALITY: member e of every output
has the bits of the §(21) single entry called with member e's parameters — its own thermodynamics parameters included — on member e's state.

Shapes (n_col, n_lev): the smallest at which this kernel can go wrong.  With 256 lanes and 4 chunks a workgroup owns ⌊1024 / n_lev⌋ columns, so
(151, 7) gives two workgroups per member, the second with 5 columns, chunk edges inside columns and member starts at odd offsets; (1, 300) one column
longer than a chunk (the LDS carry); (5, 1) a single level.  Δt = 300 s with nsub = 2 throughout: with one substep the latent heating never feeds back
and the per-member Lv, Ls would be dead."""
import pytest
import torch

import cmx
from cmx import parameters as P
from ensemble_cases import DT, E, inv_dz, members_1m, members_2m, same_bits, state_1m, state_2m
from ensemble_implicit_cases import DT_STEP, NSUB, RUNTIME_1M, members_tps, step_1m, step_2m

pytestmark = pytest.mark.gpu

FTS = ["f32", "f64"]
COL_SHAPES = [(151, 7), (1, 300), (5, 1)]
SCHEMES = ["2m", "1m"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _assert_member(got, ref, e, what):
    for name, g, r in zip(type(ref)._fields, got, ref):
        assert (g is None) == (r is None), (what, e, name)
        if g is not None:
            assert same_bits(g[e], r), (what, e, name)


def _assert_same(a, b, what):
    for name, x, y in zip(type(a)._fields, a, b):
        assert same_bits(x, y), (what, name)


# one configuration per scheme for the tests that are about the layout, not the instantiation
def _step(dev, ft, scheme, cols, dz, **kw):
    if scheme == "2m":
        return step_2m(dev, ft, True, "sb", True, dz, cols, **kw)
    return step_1m(dev, ft, {}, dz, cols, **kw)


def _state(dev, ft, scheme, lead=(E,), shape=(151, 7)):
    mk = state_2m if scheme == "2m" else state_1m
    return mk((*lead, *shape), ft, dev), inv_dz(shape[1], ft, dev)


# ---- 1. bit equality with the E single calls ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", COL_SHAPES)
@pytest.mark.parametrize("cloud", [False, True])
@pytest.mark.parametrize("vel", ["sb", "chen"])
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("ft", FTS)
def test_sb2006_implicit_step_members_equal_single_entry(dev, ft, limited, vel, cloud, shape):
    got, refs = step_2m(dev, ft, limited, vel, cloud, inv_dz(shape[1], ft, dev), state_2m((E, *shape), ft, dev))
    assert got.dq_rai_dt.shape == (E, *shape) and got.precip_flux.shape == (E, shape[0])
    for e in range(E):
        _assert_member(got, refs[e], e, f"2M implicit step {ft} limited={limited} vel={vel} cloud={cloud} {shape}")


@pytest.mark.parametrize("shape", COL_SHAPES)
@pytest.mark.parametrize("options", [{}, RUNTIME_1M], ids=["default", "runtime"])
@pytest.mark.parametrize("ft", FTS)
def test_1m_implicit_step_members_equal_single_entry(dev, ft, options, shape):
    got, refs = step_1m(dev, ft, options, inv_dz(shape[1], ft, dev), state_1m((E, *shape), ft, dev))
    assert got.dq_rai_dt.shape == (E, *shape) and got.precip_rai.shape == (E, shape[0]) and got.precip_sno.shape == (E, shape[0])
    for e in range(E):
        _assert_member(got, refs[e], e, f"1M implicit step {ft} {sorted(options)} {shape}")


# ---- 2. the power of the tps member: member 1's own latent heats change its single call -----------------------------------------------------------

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_member_1_own_thermodynamics_changes_its_single_call(dev, ft, scheme):
    """Otherwise the equality above would not notice an ensemble kernel that takes Lv and Ls from the wrong place."""
    cols, dz = _state(dev, ft, scheme, lead=())
    own, dflt = members_tps(ft)[1], P.ThermodynamicsParameters(ft)
    res = []
    for tps in (own, dflt):
        if scheme == "2m":
            mps, vels, stokes = members_2m(ft)
            res.append(cmx.column_implicit_step_2m(mps[1], tps, dz, *cols, DT_STEP, NSUB, True, vel=cmx.SB2006VelType, vel_params=vels[1], cloud_vel=stokes[1],
                                                   want_precip_flux=True))
        else:
            mps, stokes, chen_rain, chen_ice = members_1m(ft)
            res.append(cmx.column_implicit_step_1m(mps[1], tps, stokes[1], chen_rain[1], chen_ice[1], dz, *cols, DT_STEP, NSUB, True))
    torch.cuda.synchronize()
    assert any(not same_bits(a, b) for a, b in zip(*res))
    # … and the ensemble's member 1 is the one with its own
    got, _ = _step(dev, ft, scheme, cols, dz, shared=True, singles=False)
    _assert_member(got, res[0], 1, f"{scheme} member 1, own tps")


# ---- 3. shared state ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_shared_state_equals_the_state_repeated(dev, ft, scheme):
    cols, dz = _state(dev, ft, scheme, lead=())
    shared, refs = _step(dev, ft, scheme, cols, dz, shared=True)
    repeated, _ = _step(dev, ft, scheme, [c.unsqueeze(0).repeat(E, 1, 1).contiguous() for c in cols], dz, singles=False)
    _assert_same(shared, repeated, f"{scheme} shared state")
    for e in range(E):
        _assert_member(shared, refs[e], e, f"{scheme} shared state")


# ---- 4. nothing crosses a member --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_nan_in_member_1_leaves_the_other_members_untouched(dev, ft, scheme):
    """Member 1's first point follows member 0's last point in memory and its last point precedes member 2's first: a NaN in either must not change a
    bit of members 0 and 2, and member 1 is what the single entry makes of the poisoned state."""
    cols, dz = _state(dev, ft, scheme)
    clean, _ = _step(dev, ft, scheme, cols, dz, singles=False)
    bad = [c.clone() for c in cols]
    bad[5][1].view(-1)[0] = float("nan")         # q_rai of the first point of member 1
    bad[3][1].view(-1)[-1] = float("nan")        # q_lcl of its last point
    got, refs = _step(dev, ft, scheme, bad, dz)
    for name, a, b in zip(type(got)._fields, got, clean):
        assert same_bits(a[0], b[0]), (scheme, name, "member 0 changed")
        assert same_bits(a[2], b[2]), (scheme, name, "member 2 changed")
    _assert_member(got, refs[1], 1, f"{scheme} poisoned member")
    assert bool(torch.isnan(got.dq_rai_dt[1].view(-1)[0]))


# ---- 5. any alignment -------------------------------------------------------------------------------------------------------------------------------

def _offset_view(t, k=1):
    """The same values in a view that starts k elements into its storage."""
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_columns_offset_by_one_element_give_the_same_bits(dev, ft, scheme):
    cols, dz = _state(dev, ft, scheme)
    aligned, _ = _step(dev, ft, scheme, cols, dz, singles=False)
    shifted, _ = _step(dev, ft, scheme, [_offset_view(c) for c in cols], dz, singles=False)
    _assert_same(aligned, shifted, f"{scheme} inputs off by one element")
    if scheme == "2m":      # the wrapper with out=: the outputs off by one element too
        out = type(aligned)(*[_offset_view(torch.full_like(a, float("nan"))) for a in aligned])
        shifted_all, _ = _step(dev, ft, scheme, [_offset_view(c) for c in cols], dz, out=out, singles=False)
        _assert_same(aligned, shifted_all, "2m every column off by one element")


# ---- 6. the optional fluxes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_without_the_precipitation_fluxes(dev, ft, scheme):
    cols, dz = _state(dev, ft, scheme)
    full, _ = _step(dev, ft, scheme, cols, dz, singles=False)
    kw = {"want_precip_flux": False} if scheme == "2m" else {"precip": False}
    bare, _ = _step(dev, ft, scheme, cols, dz, singles=False, **kw)
    assert all(p is None for p in bare[4:])
    for name, a, b in zip(type(full)._fields[:4], full, bare):
        assert same_bits(a, b), (scheme, name)


# ---- 7. one member ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("ft", FTS)
def test_member_0_of_one_and_of_three_members_agree(dev, ft, scheme):
    cols, dz = _state(dev, ft, scheme)
    three, _ = _step(dev, ft, scheme, cols, dz, singles=False)
    one, refs = _step(dev, ft, scheme, [c[:1].contiguous() for c in cols], dz, n_members=1)
    for name, a, b in zip(type(three)._fields, three, one):
        assert same_bits(a[0], b[0]), (scheme, name)
    _assert_member(one, refs[0], 0, f"{scheme} E = 1")


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", FTS)
def test_captured_call_replays_bit_identically_and_sees_a_table_update(dev, ft):
    """One ensemble call in a capture (a single launch), replayed twice.  The table is an ordinary device buffer the kernel reads: after member 2's block is
    overwritten in place with member 1's — its Lv and Ls included —, the replay gives member 1's result for member 2's state."""
    mps, vels, stokes = members_2m(ft)
    tps = members_tps(ft)
    tab = cmx.ensemble.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels, cloud_vel=stokes).to(dev)
    cols, dz = state_2m((E, 151, 7), ft, dev), inv_dz(7, ft, dev)
    out = cmx.ColumnTendencies2M(*[torch.empty((E, 151, 7), dtype=DT[ft], device=dev) for _ in range(4)], torch.empty((E, 151), dtype=DT[ft], device=dev))
    call = lambda: cmx.ensemble.column_implicit_step_2m(tab, dz, *cols, DT_STEP, NSUB, True, out=out)      # noqa: E731
    call()
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        for o in out:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(out._fields, out, eager):
            assert same_bits(a, b), name
    s = tab.desc.stride
    tab.table[2 * s:3 * s].copy_(tab.table[s:2 * s])
    g.replay()
    torch.cuda.synchronize()
    ref = cmx.column_implicit_step_2m(mps[1], tps[1], dz, *[c[2] for c in cols], DT_STEP, NSUB, True, vel=cmx.SB2006VelType, vel_params=vels[1],
                                      cloud_vel=stokes[1], want_precip_flux=True)
    torch.cuda.synchronize()
    _assert_member(out, ref, 2, "replay after a table update")
    for name, a, b in zip(out._fields, out, eager):
        assert same_bits(a[:2], b[:2]), name
