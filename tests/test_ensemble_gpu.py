"""The parameter-ensemble entries (include/cmx.h §29) on the GPU.  The contract is EQUALITY: member e of every output of an ensemble call has the bits
of the single entry called with member e's parameters on member e's state — the kernels run the single kernels' own text on the same operands.

Shapes: the smallest at which the kernels can go wrong.  Pointwise n = 1027 — with 4 Float32 points per lane and 128-lane workgroups three workgroups
per member, the last one partial, and n mod 4 = 3 so members 1 and 2 start misaligned (per-member head and tail) — and n = 1.  Columns 151 × 7 = 1057
points — more than one Float32 tile of 255 lanes × 4 points, several Float64 tiles, tile and member boundaries inside columns and at odd offsets —, 5 × 1
and one column of 300 levels."""
import numpy as np
import pytest
import torch

import parity
from cmx import _abi
from cmx import parameters as P
from ensemble_cases import DT, E, inv_dz, members_1m, members_2m, same_bits, state_1m, state_2m

pytestmark = pytest.mark.gpu

FTS = ["f32", "f64"]
COL_SHAPES = [(151, 7), (5, 1), (1, 300)]
RUNTIME_1M = {"snow_autoconversion": P.WithSupersaturation, "rain_autoconversion": P.PrescribedNd}      # one run-time-flags option set


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _vel(name):
    import cmx
    return {"none": None, "sb": cmx.SB2006VelType, "chen": cmx.Chen2022VelTypeRain}[name]


def _assert_member(got, ref, e, what):
    for name, g, r in zip(type(ref)._fields, got, ref):
        assert (g is None) == (r is None), (what, e, name)
        if g is not None:
            assert torch.equal(g[e], r) or same_bits(g[e], r), (what, e, name)      # (torch.equal is False for equal NaNs)
            assert same_bits(g[e], r), (what, e, name)


# ---- the four families: ensemble call and the E single calls it replaces ------------------------------------------------------------------------

def _pointwise_2m(dev, ft, limited, vel, cols, n_members=E, shared=False, out=None):
    import cmx
    mps, vels, _ = members_2m(ft, limited, n_members)
    tps = P.ThermodynamicsParameters(ft)
    tab = cmx.ensemble.pack_2m(mps, tps, vel=_vel(vel), vel_params=vels if vel != "none" else None).to(dev)
    got = cmx.ensemble.warm_rain_tendencies_2m(tab, *cols, shared_state=shared, out=out)
    refs = [cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mps[e], tps, *[c if shared else c[e] for c in cols], vel=_vel(vel),
                                             vel_params=vels[e] if vel != "none" else None) for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs


def _pointwise_1m(dev, ft, options, cols, n_members=E, shared=False, out=None):
    import cmx
    mps, *_ = members_1m(ft, n_members, **options)
    tps = P.ThermodynamicsParameters(ft)
    tab = cmx.ensemble.pack_1m(mps, tps).to(dev)
    assert tab.desc.runtime_flags == (1 if options else 0)
    got = cmx.ensemble.tendencies_1m(tab, *cols, shared_state=shared, out=out)
    refs = [cmx.bulk_microphysics_tendencies_1m(cmx.Instantaneous(), cmx.Microphysics1Moment(), mps[e], tps, *[c if shared else c[e] for c in cols])
            for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs


def _column_2m(dev, ft, limited, vel, cloud, dz, cols, n_members=E, shared=False, out=None):
    import cmx
    mps, vels, stokes = members_2m(ft, limited, n_members)
    tps = P.ThermodynamicsParameters(ft)
    tab = cmx.ensemble.pack_2m(mps, tps, vel=_vel(vel), vel_params=vels, cloud_vel=stokes if cloud else None).to(dev)
    got = cmx.ensemble.column_tendencies_sedimentation_2m(tab, dz, *cols, shared_state=shared, want_precip_flux=True, out=out)
    refs = [cmx.column_tendencies_sedimentation(mps[e], tps, dz, *[c if shared else c[e] for c in cols], vel=_vel(vel), vel_params=vels[e],
                                                cloud_vel=stokes[e] if cloud else None, want_precip_flux=True) for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs


def _column_1m(dev, ft, options, nsub, dz, cols, n_members=E, shared=False):
    import cmx
    mps, stokes, chen_rain, chen_ice = members_1m(ft, n_members, **options)
    tps = P.ThermodynamicsParameters(ft)
    tab = cmx.ensemble.pack_1m(mps, tps, stokes=stokes, chen_rain=chen_rain, chen_ice=chen_ice).to(dev)
    kw = dict(dt=20.0, nsub=nsub) if nsub else {}
    got = cmx.ensemble.column_tendencies_sedimentation_1m(tab, dz, *cols, shared_state=shared, **kw)
    mode = cmx.LinearizedAverage() if nsub else cmx.Instantaneous()
    refs = [cmx.column_tendencies_sedimentation_1m(mode, cmx.Microphysics1Moment(), mps[e], tps, stokes[e], chen_rain[e], chen_ice[e], dz,
                                                   *[c if shared else c[e] for c in cols], **kw) for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs


# one configuration of each family for the tests that are about the layout, not the instantiation
def _family(dev, ft, fam, cols, dz=None, **kw):
    if fam == "tend2m":
        return _pointwise_2m(dev, ft, True, "sb", cols, **kw)
    if fam == "tend1m":
        return _pointwise_1m(dev, ft, {}, cols, **kw)
    if fam == "col2m":
        return _column_2m(dev, ft, True, "sb", True, dz, cols, **kw)
    return _column_1m(dev, ft, {}, 0, dz, cols, **kw)


FAMILIES = ["tend2m", "tend1m", "col2m", "col1m"]


def _family_state(dev, ft, fam, lead=(E,), seed=None):
    """(cols, dz) of the family's standard shape with the leading dimensions `lead` (members, or () for one state)."""
    mk = state_2m if fam.endswith("2m") else state_1m
    kw = {} if seed is None else {"seed": seed}
    if fam.startswith("tend"):
        return mk((*lead, 1027), ft, dev, **kw), None
    return mk((*lead, 151, 7), ft, dev, **kw), inv_dz(7, ft, dev)


# ---- 1. bit equality with the single entries ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1027, 1])
@pytest.mark.parametrize("vel", ["none", "sb", "chen"])
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("ft", FTS)
def test_warm_rain_tendencies_members_equal_single_entry(dev, ft, limited, vel, n):
    got, refs = _pointwise_2m(dev, ft, limited, vel, state_2m((E, n), ft, dev))
    assert (got.vt_rai_n is None) == (vel == "none")
    for e in range(E):
        _assert_member(got, refs[e], e, f"2M tendencies {ft} limited={limited} vel={vel} n={n}")
    assert not same_bits(got.dq_rai_dt[0], got.dq_rai_dt[1]) or n == 1      # the members do differ


@pytest.mark.parametrize("n", [1027, 1])
@pytest.mark.parametrize("options", [{}, RUNTIME_1M], ids=["default", "runtime"])
@pytest.mark.parametrize("ft", FTS)
def test_1m_tendencies_members_equal_single_entry(dev, ft, options, n):
    got, refs = _pointwise_1m(dev, ft, options, state_1m((E, n), ft, dev))
    for e in range(E):
        _assert_member(got, refs[e], e, f"1M tendencies {ft} {sorted(options)} n={n}")


@pytest.mark.parametrize("shape", COL_SHAPES)
@pytest.mark.parametrize("cloud", [False, True])
@pytest.mark.parametrize("vel", ["sb", "chen"])
@pytest.mark.parametrize("limited", [True, False])
@pytest.mark.parametrize("ft", FTS)
def test_sb2006_column_step_members_equal_single_entry(dev, ft, limited, vel, cloud, shape):
    got, refs = _column_2m(dev, ft, limited, vel, cloud, inv_dz(shape[1], ft, dev), state_2m((E, *shape), ft, dev))
    for e in range(E):
        _assert_member(got, refs[e], e, f"2M column {ft} limited={limited} vel={vel} cloud={cloud} {shape}")


@pytest.mark.parametrize("shape", COL_SHAPES)
@pytest.mark.parametrize("nsub", [0, 2])
@pytest.mark.parametrize("options", [{}, RUNTIME_1M], ids=["default", "runtime"])
@pytest.mark.parametrize("ft", FTS)
def test_1m_column_step_members_equal_single_entry(dev, ft, options, nsub, shape):
    got, refs = _column_1m(dev, ft, options, nsub, inv_dz(shape[1], ft, dev), state_1m((E, *shape), ft, dev))
    for e in range(E):
        _assert_member(got, refs[e], e, f"1M column {ft} {sorted(options)} nsub={nsub} {shape}")


# ---- 2. shared state ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("ft", FTS)
def test_shared_state_equals_the_state_repeated(dev, ft, fam):
    cols, dz = _family_state(dev, ft, fam, lead=())
    shared, refs = _family(dev, ft, fam, cols, dz, shared=True)
    repeated, _ = _family(dev, ft, fam, [c.unsqueeze(0).repeat(E, *[1] * c.dim()).contiguous() for c in cols], dz)
    for name, a, b in zip(type(shared)._fields, shared, repeated):
        assert same_bits(a, b), (fam, name)
    for e in range(E):
        _assert_member(shared, refs[e], e, f"{fam} shared state")


@pytest.mark.parametrize("ft", FTS)
def test_shared_state_vector_path(dev, ft):
    """n a multiple of the vector width: the shared-state call keeps 16-byte accesses (inputs and outputs stay aligned from member to member)."""
    cols = state_2m((1024,), ft, dev)
    shared, refs = _pointwise_2m(dev, ft, True, "sb", cols, shared=True)
    for e in range(E):
        _assert_member(shared, refs[e], e, "2M tendencies shared state, n = 1024")


# ---- 3. nothing leaks across a member boundary --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,poison", [(f, float("nan")) for f in FAMILIES] + [("col2m", 1e30), ("col1m", 1e30)],
                         ids=[f"{f}-nan" for f in FAMILIES] + ["col2m-huge", "col1m-huge"])
@pytest.mark.parametrize("ft", FTS)
def test_no_leak_across_members(dev, ft, fam, poison):
    """Member 1's first point follows member 0's last point in memory.  A NaN there — or, for the column steps, a large finite value, which a halo that is
    read and multiplied by zero would still turn into a NaN or an Inf — must not change one bit of member 0: its top-of-last-column cells and
    precipitation fluxes included."""
    cols, dz = _family_state(dev, ft, fam)
    clean, _ = _family(dev, ft, fam, cols, dz)
    bad = [c.clone() for c in cols]
    for c in bad:
        c[1].view(-1)[0] = poison
    got, refs = _family(dev, ft, fam, bad, dz)
    for name, a, b in zip(type(got)._fields, got, clean):
        if a is not None:
            assert same_bits(a[0], b[0]), (fam, name, "member 0 changed")
            assert same_bits(a[2], b[2]), (fam, name, "member 2 changed")
    _assert_member(got, refs[1], 1, f"{fam} poisoned member")          # … and member 1 is what the single entry makes of the poisoned state
    if poison != poison:
        assert bool(torch.isnan(got[0][1].view(-1)[0]))


# ---- 4. misaligned base pointers ----------------------------------------------------------------------------------------------------------------

def _offset_view(t, k=1):
    """The same values in a view that starts k elements into its storage."""
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("ft", FTS)
def test_misaligned_columns_give_the_same_bits(dev, ft, fam):
    cols, dz = _family_state(dev, ft, fam)
    aligned, _ = _family(dev, ft, fam, cols, dz)
    shifted_in, _ = _family(dev, ft, fam, [_offset_view(c) for c in cols], dz)          # inputs off by one element, outputs aligned: one point per lane
    for name, a, b in zip(type(aligned)._fields, aligned, shifted_in):
        assert same_bits(a, b), (fam, name)
    if fam in ("tend2m", "tend1m", "col2m"):                                            # the wrappers with out=: every column off by one element —
        out = type(aligned)(*[None if a is None else _offset_view(torch.full_like(a, float("nan"))) for a in aligned])      # the per-member split
        shifted_all, _ = _family(dev, ft, fam, [_offset_view(c) for c in cols], dz, out=out)
        for name, a, b in zip(type(aligned)._fields, aligned, shifted_all):
            assert same_bits(a, b), (fam, name)


# ---- 5. one member ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("ft", FTS)
def test_one_member_equals_the_single_entry(dev, ft, fam):
    cols, dz = _family_state(dev, ft, fam, lead=(1,))
    got, refs = _family(dev, ft, fam, cols, dz, n_members=1)
    _assert_member(got, refs[0], 0, f"{fam} E = 1")


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", FTS)
def test_captured_column_call_replays_bit_identically(dev, ft):
    """One ensemble column call in a capture (a single linear sequence of launches), replayed twice.  The table is an ordinary device buffer the
    kernels read: a member updated in place between replays is seen by the next replay."""
    import cmx
    mps, vels, stokes = members_2m(ft)
    tps = P.ThermodynamicsParameters(ft)
    tab = cmx.ensemble.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels, cloud_vel=stokes).to(dev)
    cols, dz = state_2m((E, 151, 7), ft, dev), inv_dz(7, ft, dev)
    out = cmx.ColumnTendencies2M(*[torch.empty((E, 151, 7), dtype=DT[ft], device=dev) for _ in range(4)], torch.empty((E, 151), dtype=DT[ft], device=dev))
    call = lambda: cmx.ensemble.column_tendencies_sedimentation_2m(tab, dz, *cols, out=out)      # noqa: E731
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
    # member 0's block replaced by member 1's, in place: the replay gives member 1's results for member 0's state
    s = tab.desc.stride
    tab.table[:s].copy_(tab.table[s:2 * s])
    g.replay()
    torch.cuda.synchronize()
    ref = cmx.column_tendencies_sedimentation(mps[1], tps, dz, *[c[0] for c in cols], vel=cmx.SB2006VelType, vel_params=vels[1], cloud_vel=stokes[1],
                                              want_precip_flux=True)
    torch.cuda.synchronize()
    _assert_member(out, ref, 0, "replay after a table update")


# ---- 7. the oracle, independently of the single entry -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ft", FTS)
def test_member_2_matches_the_oracle(dev, oracle, ft):
    import cmx
    n = 20_011
    mps, vels, _ = members_2m(ft)
    tab = cmx.ensemble.pack_2m(mps, P.ThermodynamicsParameters(ft), vel=cmx.SB2006VelType, vel_params=vels).to(dev)
    cols = state_2m((E, n), ft, seed=23)
    got = cmx.ensemble.warm_rain_tendencies_2m(tab, *[c.to(dev) for c in cols])
    torch.cuda.synchronize()
    mps64, vels64, _ = members_2m("f64")
    ref = oracle.sb2006_warm_rain_tendencies(_abi.F64, mps64[2].c, P.ThermodynamicsParameters("f64"), vels64[2],
                                             _abi.CMX_SB2006_LIMITED | _abi.CMX_VEL_SB2006, *[c[2].numpy().astype(np.float64) for c in cols],
                                             float32_gates=(ft == "f32"), nthreads=4)
    g = {k: getattr(got, k)[2].cpu().numpy() for k in got._fields}
    rep = parity.assert_parity(g, ref, parity.RTOL[ft], what=f"ensemble member 2 {ft}", family="SB2006 2M warm rain (a1)")
    print(f"\n[ensemble parity] {ft}: {rep}")
