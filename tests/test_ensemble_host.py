"""The host side of the parameter-ensemble entries (include/cmx.h §29), without a GPU: the statuses of the packs, block independence, the argument validation
of the ensemble entries (every one of these calls returns before any HIP runtime call and never dereferences the table pointer) and the checks of the
Python wrappers."""
import ctypes as C

import pytest
import torch

import cmx
from cmx import _abi, _lib
from cmx import ensemble as ens
from cmx import parameters as P
from ensemble_cases import E, members_1m, members_2m

FTS = ["f32", "f64"]
OK, BAD, UNS = _abi.CMX_OK, _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
HUGE = 16 * 0x7fffffff + 1       # one more than kMaxPoints (cmx_launch.hpp)
TABLE = C.c_void_p(0x10)         # a "device" pointer no host code may touch


def _arr(ctype, items):
    return (ctype * len(items))(*items)


def _pack_2m_raw(ft, mps, vels, stokes, flags, n=None, table_bytes=None, table=True, desc=True):
    fam = _abi.family(ft)
    lib = _lib.lib()
    n = len(mps) if n is None else n
    stride = getattr(lib, f"cmx_sb2006_ensemble_table_stride_{ft}")()
    buf = (C.c_ubyte * (len(mps) * stride))()
    d = _abi.EnsembleDesc()
    st = getattr(lib, f"cmx_sb2006_ensemble_pack_{ft}")(
        _arr(fam.warm_rain_2m, [m.c for m in mps]), _arr(fam.thermo, [P.ThermodynamicsParameters(ft)] * len(mps)),
        _arr(fam.rain_vel, vels) if vels else None, _arr(fam.stokes_vel, stokes) if stokes else None, flags, n,
        buf if table else None, len(buf) if table_bytes is None else table_bytes, C.byref(d) if desc else None)
    return st, bytes(buf), d, stride


@pytest.mark.parametrize("ft", FTS)
def test_pack_2m_statuses(ft):
    lim, sb, ch = _abi.CMX_SB2006_LIMITED, _abi.CMX_VEL_SB2006, _abi.CMX_VEL_CHEN2022
    mps, vels, stokes = members_2m(ft)
    assert _pack_2m_raw(ft, mps, vels, stokes, lim | sb)[0] == OK
    assert _pack_2m_raw(ft, mps, None, None, lim)[0] == OK                          # no fall speed: the pointwise entry without vt_rai_*
    assert _pack_2m_raw(ft, mps, vels, None, lim | sb, n=0)[0] == BAD               # n_members < 1
    assert _pack_2m_raw(ft, mps, vels, None, lim | sb, table=False)[0] == BAD
    assert _pack_2m_raw(ft, mps, vels, None, lim | sb, desc=False)[0] == BAD
    assert _pack_2m_raw(ft, mps, vels, None, lim | sb | 8)[0] == BAD                # unknown flag bit
    assert _pack_2m_raw(ft, mps, vels, None, lim)[0] == BAD                         # fall-speed parameters, no scheme
    assert _pack_2m_raw(ft, mps, vels, None, lim | sb | ch)[0] == BAD               # … both schemes
    st, _, _, stride = _pack_2m_raw(ft, mps, vels, None, lim | sb, table_bytes=E * 16)
    assert st == BAD and stride % 16 == 0                                           # buffer shorter than n_members · stride
    # a member that fails a check of the single entry gives that check's status
    bad, _, _ = members_2m(ft)
    bad[1].c.seifert_beheng.pdf_r.N0_min = 2 * bad[1].c.seifert_beheng.pdf_r.N0_max
    assert _pack_2m_raw(ft, bad, vels, None, lim | sb)[0] == BAD                    # unordered limiter pair under CMX_SB2006_LIMITED
    nl, nlvels, _ = members_2m(ft, limited=False)
    assert _pack_2m_raw(ft, nl, nlvels, None, sb)[0] == OK
    nlvels[2].sb2006.aR = nlvels[2].sb2006.bR
    assert _pack_2m_raw(ft, nl, nlvels, None, sb)[0] == BAD                         # aR ≥ bR with the not-limited SB2006 fall speed
    assert _pack_2m_raw(ft, nl, nlvels, None, ch)[0] == OK                          # (the Chen-2022 fall speed does not read aR, bR)
    # members that disagree on a dispatch choice: the default member has the integer exponents, the other a perturbed one
    mixed, _, _ = members_2m(ft)
    mixed[1].c.seifert_beheng.acnv.b *= 1.01
    assert _pack_2m_raw(ft, mixed, vels, None, lim | sb)[0] == UNS
    assert _pack_2m_raw(ft, mixed[1:2], vels[1:2], None, lim | sb)[0] == OK         # … each on its own packs
    assert _pack_2m_raw(ft, mixed[1:2], vels[1:2], None, lim | sb)[2].integer_exponents == 0


@pytest.mark.parametrize("ft", FTS)
def test_pack_1m_statuses(ft):
    fam, lib = _abi.family(ft), _lib.lib()
    mps, stokes, chen_rain, chen_ice = members_1m(ft)
    stride = getattr(lib, f"cmx_mp1m_ensemble_table_stride_{ft}")()
    assert stride % 16 == 0
    buf, d = (C.c_ubyte * (E * stride))(), _abi.EnsembleDesc()
    mp_a, tps_a = _arr(fam.microphysics_1m, [m.c for m in mps]), _arr(fam.thermo, [P.ThermodynamicsParameters(ft)] * E)
    sed = (_arr(fam.stokes_vel, stokes), _arr(fam.chen2022_rain_vel, chen_rain), _arr(fam.chen2022_ice_vel, chen_ice))
    f = getattr(lib, f"cmx_mp1m_ensemble_pack_{ft}")
    flags = mps[0].flags
    assert f(mp_a, tps_a, *sed, flags, E, buf, len(buf), C.byref(d)) == OK
    assert (d.magic, d.scheme, d.float_type, d.flags, d.n_members, d.stride) == (_abi.CMX_ENSEMBLE_MAGIC, _abi.CMX_ENSEMBLE_SCHEME_MP1M,
                                                                                   4 if ft == "f32" else 8, flags, E, stride)
    assert (d.runtime_flags, d.sedimentation, d.general_gamma) == (0, 1, 0)
    assert f(mp_a, tps_a, None, None, None, flags, E, buf, len(buf), C.byref(d)) == OK and d.sedimentation == 0
    assert f(None, tps_a, *sed, flags, E, buf, len(buf), C.byref(d)) == BAD
    assert f(mp_a, None, *sed, flags, E, buf, len(buf), C.byref(d)) == BAD
    assert f(mp_a, tps_a, sed[0], None, sed[2], flags, E, buf, len(buf), C.byref(d)) == BAD             # the fall-speed parameters: all three or none
    assert f(mp_a, tps_a, *sed, flags, 0, buf, len(buf), C.byref(d)) == BAD
    assert f(mp_a, tps_a, *sed, flags, E, None, len(buf), C.byref(d)) == BAD
    assert f(mp_a, tps_a, *sed, flags, E, buf, len(buf), None) == BAD
    assert f(mp_a, tps_a, *sed, flags, E, buf, len(buf) - 1, C.byref(d)) == BAD
    both = _abi.CMX_1M_SED_SNOW_OBLATE | _abi.CMX_1M_SED_SNOW_PROLATE
    assert f(mp_a, tps_a, *sed, flags | both, E, buf, len(buf), C.byref(d)) == BAD
    assert f(mp_a, tps_a, *sed, flags | _abi.CMX_1M_RAIN_ACNV_PRESCRIBED_ND, E, buf, len(buf), C.byref(d)) == BAD      # two variants of one process
    assert f(mp_a, tps_a, *sed, flags | _abi.CMX_1M_SED_SNOW_OBLATE, E, buf, len(buf), C.byref(d)) == UNS              # the unshaped step only
    # members that disagree on a dispatch choice: default slope-parameter exponents against a perturbed fall-speed exponent
    mixed, *_ = members_1m(ft)
    mixed[2].c.vel_rain.ve *= 1.01
    assert f(_arr(fam.microphysics_1m, [m.c for m in mixed]), tps_a, *sed, flags, E, buf, len(buf), C.byref(d)) == UNS
    assert f(_arr(fam.microphysics_1m, [mixed[2].c]), tps_a, *sed, flags, 1, buf, len(buf), C.byref(d)) == OK and d.runtime_flags == 1


@pytest.mark.parametrize("ft", FTS)
def test_block_of_a_member_depends_on_that_member_only(ft):
    lim, sb = _abi.CMX_SB2006_LIMITED, _abi.CMX_VEL_SB2006
    mps, vels, stokes = members_2m(ft)
    st_ab, ab, d, stride = _pack_2m_raw(ft, mps[:2], vels[:2], stokes[:2], lim | sb)
    st_b, b, d1, _ = _pack_2m_raw(ft, mps[1:2], vels[1:2], stokes[1:2], lim | sb)
    assert st_ab == OK and st_b == OK
    assert ab[stride:2 * stride] == b[:stride] and ab[:stride] != ab[stride:2 * stride]
    assert stride % 16 == 0 and (d.n_members, d.flags, d.stride, d1.n_members) == (2, lim | sb, stride, 1)
    assert (d.magic, d.scheme, d.float_type, d.vel_kind, d.integer_exponents, d.cloud_vel) == (_abi.CMX_ENSEMBLE_MAGIC, _abi.CMX_ENSEMBLE_SCHEME_SB2006,
                                                                                              4 if ft == "f32" else 8, 1, 1, 1)
    m1, s1, cr1, ci1 = members_1m(ft)
    ta = ens.pack_1m(m1[:2], P.ThermodynamicsParameters(ft), stokes=s1[:2], chen_rain=cr1[:2], chen_ice=ci1[:2])
    tb = ens.pack_1m(m1[1:2], P.ThermodynamicsParameters(ft), stokes=s1[1:2], chen_rain=cr1[1:2], chen_ice=ci1[1:2])
    s = ta.desc.stride
    assert torch.equal(ta.table[s:], tb.table) and not torch.equal(ta.table[:s], ta.table[s:])


def _desc(ft, scheme):
    if scheme == "sb2006":
        mps, vels, stokes = members_2m(ft)
        return ens.pack_2m(mps, P.ThermodynamicsParameters(ft), vel=cmx.SB2006VelType, vel_params=vels, cloud_vel=stokes).desc
    mps, stokes, chen_rain, chen_ice = members_1m(ft)
    return ens.pack_1m(mps, P.ThermodynamicsParameters(ft), stokes=stokes, chen_rain=chen_rain, chen_ice=chen_ice).desc


def _copy(d, **kw):
    c = _abi.EnsembleDesc.from_buffer_copy(d)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("ft", FTS)
def test_ensemble_entry_argument_validation_without_gpu(ft):
    """Every call below returns before any HIP runtime call; TABLE is not a valid address on the host."""
    lib = _lib.lib()
    cols = lambda k: [C.c_void_p(0x1000 * (j + 1)) for j in range(k)]      # noqa: E731
    null = lambda k: [None] * k                                             # noqa: E731
    d2, d1 = _desc(ft, "sb2006"), _desc(ft, "mp1m")
    d2_novel = ens.pack_2m(members_2m(ft)[0], P.ThermodynamicsParameters(ft), vel=None).desc
    d1_nosed = ens.pack_1m(members_1m(ft)[0], P.ThermodynamicsParameters(ft)).desc
    other = "f64" if ft == "f32" else "f32"
    in7, out4 = (C.c_void_p * 7)(*[0x1000 * (j + 1) for j in range(7)]), (C.c_void_p * 4)(*[0x9000 + 0x1000 * j for j in range(4)])
    # (entry, its desc, the argument lists in front of and behind (desc, table, n_members, ens_flags) with sizes s, the array arguments present / absent)
    t2 = getattr(lib, f"cmx_sb2006_warm_rain_tendencies_ensemble_{ft}")
    t1 = getattr(lib, f"cmx_mp1m_tendencies_ensemble_{ft}")
    c2 = getattr(lib, f"cmx_sb2006_column_tendencies_sedimentation_ensemble_{ft}")
    c1 = getattr(lib, f"cmx_mp1m_column_tendencies_sedimentation_ensemble_{ft}")
    calls = {
        "t2": (d2, lambda d, tab, E_, fl, n, arrs=True: t2(d, tab, E_, fl, n, *(cols(13) if arrs else null(13)), None)),
        "t1": (d1, lambda d, tab, E_, fl, n, arrs=True: t1(d, tab, E_, fl, n, *(cols(11) if arrs else null(11)), None)),
        "c2": (d2, lambda d, tab, E_, fl, n, arrs=True: c2(d, tab, E_, fl, n, 7, *(cols(13) if arrs else null(13)), None)),
        "c1": (d1, lambda d, tab, E_, fl, n, arrs=True: c1(d, tab, E_, fl, 0.0, 0.0, 0, n, 7, C.c_void_p(0x100) if arrs else None, in7 if arrs else None,
                                                           out4 if arrs else None, None, None, None)),
    }
    for name, (d, call) in calls.items():
        ref = C.byref(d)
        big = HUGE if name[0] == "t" else HUGE // 7 + 1
        assert call(ref, TABLE, E, 0, 0, arrs=False) == OK, name                      # a per-member size of 0
        assert call(ref, TABLE, E, _abi.CMX_ENSEMBLE_SHARED_STATE, 0, arrs=False) == OK, name
        assert call(None, TABLE, E, 0, 0) == BAD, name
        assert call(ref, None, E, 0, 0) == BAD, name
        assert call(ref, TABLE, E, 0, -1) == BAD, name
        assert call(ref, TABLE, E, 0, big) == UNS, name                               # per member above the single entry's limit
        assert call(C.byref(_copy(d, magic=0)), TABLE, E, 0, 0) == BAD, name
        assert call(C.byref(_copy(d, scheme=3 - d.scheme)), TABLE, E, 0, 0) == BAD, name
        assert call(C.byref(_desc(other, "sb2006" if name.endswith("2") else "mp1m")), TABLE, E, 0, 0) == BAD, name      # the other float type
        assert call(ref, TABLE, 0, 0, 0) == BAD, name
        assert call(C.byref(_copy(d, n_members=0)), TABLE, 0, 0, 0) == BAD, name
        assert call(ref, TABLE, E + 1, 0, 0) == BAD, name                             # n_members against the desc
        assert call(C.byref(_copy(d, stride=d.stride + 16)), TABLE, E, 0, 0) == BAD, name
        assert call(ref, TABLE, E, 2, 0) == BAD, name                                 # unknown ens_flags bit
        assert call(C.byref(_copy(d, n_members=65536)), TABLE, 65536, 0, 0) == UNS, name      # the y limit of a grid
        assert call(C.byref(_copy(d, n_members=65535)), TABLE, 65535, 0, 0) == OK, name
        assert call(ref, TABLE, E, 0, 10, arrs=False) == BAD, name                    # NULL arrays
    # the column entries on tables packed without their fall-speed parameters; vt_rai_* from a table without a fall speed
    assert calls["c2"][1](C.byref(d2_novel), TABLE, E, 0, 10) == BAD
    assert calls["c1"][1](C.byref(d1_nosed), TABLE, E, 0, 10) == BAD
    assert t2(C.byref(d2_novel), TABLE, E, 0, 10, *cols(13), None) == BAD
    assert t2(C.byref(d2_novel), TABLE, E, 0, 0, *cols(13), None) == OK
    # the 1-moment column step: nsub < 0, and dt ≤ 0 or q_min < 0 with nsub > 0
    r1 = C.byref(d1)
    assert c1(r1, TABLE, E, 0, 0.0, 0.0, -1, 0, 7, None, None, None, None, None, None) == BAD
    assert c1(r1, TABLE, E, 0, 0.0, 0.0, 2, 0, 7, None, None, None, None, None, None) == BAD
    assert c1(r1, TABLE, E, 0, -1.0, 10.0, 2, 0, 7, None, None, None, None, None, None) == BAD
    assert c1(r1, TABLE, E, 0, 1e-9, 10.0, 2, 0, 7, None, None, None, None, None, None) == OK
    assert c2(C.byref(d2), TABLE, E, 0, 5, 0, *cols(13), None) == BAD                 # n_lev < 1


def test_wrapper_checks_and_broadcasting():
    ft = "f32"
    mps, vels, stokes = members_2m(ft)
    tps = P.ThermodynamicsParameters(ft)
    one = ens.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels)                       # tps broadcast …
    many = ens.pack_2m(mps, [tps] * E, vel=cmx.SB2006VelType, vel_params=vels)                # … equals one per member
    assert isinstance(one, cmx.EnsembleTable) and len(one) == E and one.table.dtype == torch.uint8 and one.table.numel() == E * one.desc.stride
    assert torch.equal(one.table, many.table) and one.to("cpu").desc is one.desc
    dflt = ens.pack_2m(mps, tps)                                                               # default fall-speed parameters, broadcast
    assert dflt.desc.vel_kind == 1 and not torch.equal(dflt.table, one.table)
    t2 = P.ThermodynamicsParameters(ft)
    t2.LH_v0 *= 1.01
    assert not torch.equal(ens.pack_2m(mps, [tps, t2, tps]).table, dflt.table)
    with pytest.raises(ValueError):
        ens.pack_2m(mps, [tps, tps])                                                           # two entries for three members
    with pytest.raises(TypeError):
        ens.pack_2m(mps, P.ThermodynamicsParameters("f64"))
    with pytest.raises(TypeError):
        ens.pack_2m(mps + members_2m("f64")[0][:1], tps)
    with pytest.raises(ValueError):
        ens.pack_2m([mps[0], members_2m(ft, limited=False)[0][1]], tps)                        # is_limited differs
    with pytest.raises(ValueError):
        ens.pack_2m([], tps)
    mixed, _, _ = members_2m(ft)
    mixed[1].c.seifert_beheng.accr.c = 4.5
    with pytest.raises(cmx.CmxStatusError) as ei:
        ens.pack_2m(mixed, tps)
    assert ei.value.status == UNS
    m1, s1, cr1, ci1 = members_1m(ft)
    with pytest.raises(TypeError):
        ens.pack_1m(m1, tps, stokes=s1)                                                        # all three fall-speed structs or none
    with pytest.raises(ValueError):
        ens.pack_1m([m1[0], P.Microphysics1MParams(ft, snow_autoconversion=P.WithSupersaturation)], tps)
    with pytest.raises(TypeError):
        ens.pack_1m(mps, tps)
    tab1 = ens.pack_1m(m1, tps, stokes=s1[0], chen_rain=cr1, chen_ice=ci1[0])                  # one struct broadcast, one sequence
    assert len(tab1) == E and tab1.desc.sedimentation == 1
    # state checks happen before anything touches a device: CPU columns are refused, as by the single-entry wrappers
    x = [torch.zeros(E, 8) for _ in range(7)]
    with pytest.raises(ValueError, match="GPU"):
        ens.warm_rain_tendencies_2m(one, *x)
    with pytest.raises(TypeError):
        ens.tendencies_1m(one, *x)                                                             # a table of the other scheme
    with pytest.raises(TypeError):
        ens.warm_rain_tendencies_2m("table", *x)


@pytest.mark.gpu
def test_wrapper_shape_and_dtype_checks_on_device():
    dev = torch.device("cuda:0")
    mps, vels, stokes = members_2m("f32")
    tab = ens.pack_2m(mps, P.ThermodynamicsParameters("f32"), vel=cmx.SB2006VelType, vel_params=vels)
    x = [torch.ones(E, 8, device=dev) for _ in range(7)]
    with pytest.raises(ValueError, match="device"):
        ens.warm_rain_tendencies_2m(tab, *x)                                                   # the table is still on the host
    tab = tab.to(dev)
    with pytest.raises(ValueError):
        ens.warm_rain_tendencies_2m(tab, *[c[:2] for c in x])                                  # two members of state for three
    with pytest.raises(ValueError):
        ens.warm_rain_tendencies_2m(tab, *x, shared_state=True)                                # a shared state has no member dimension
    with pytest.raises(TypeError):
        ens.warm_rain_tendencies_2m(tab, *[c.double() for c in x])
    with pytest.raises(ValueError):
        ens.warm_rain_tendencies_2m(tab, *x[:6], x[6].t().contiguous().t())                    # not contiguous
    with pytest.raises(ValueError):
        ens.column_tendencies_sedimentation_2m(tab, torch.ones(8, device=dev), *x)             # (E, n_col, n_lev) expected
    x3 = [c.reshape(E, 2, 4) for c in x]
    with pytest.raises(ValueError):
        ens.column_tendencies_sedimentation_2m(tab, torch.ones(5, device=dev), *x3)            # inv_dz: n_lev values
    out = ens.column_tendencies_sedimentation_2m(tab, torch.ones(4, device=dev), *x3, want_precip_flux=True)
    assert out.dq_rai_dt.shape == (E, 2, 4) and out.precip_flux.shape == (E, 2)
    with pytest.raises(ValueError):
        ens.warm_rain_tendencies_2m(tab, *x, out=cmx.WarmRainTendencies2M(*[torch.empty(E, 9, device=dev) for _ in range(6)]))
