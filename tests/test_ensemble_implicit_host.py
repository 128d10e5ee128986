"""The host side of the ensemble forms of the implicit column steps (include/cmx.h §29, continuation), without a GPU: the argument ladder of the four
entries — every call below returns before any HIP runtime call and never dereferences the table pointer —, the SB2006 block with its two latent-heat
ratios, and the checks of the Python wrappers that come before anything touches a device."""
import ctypes as C
import struct

import pytest
import torch

import cmx
from cmx import _abi, _lib
from cmx import ensemble as ens
from cmx import parameters as P
from ensemble_cases import E, members_1m, members_2m
from ensemble_implicit_cases import members_tps

FTS = ["f32", "f64"]
OK, BAD, UNS = _abi.CMX_OK, _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
HUGE = 16 * 0x7fffffff + 1       # one more than kMaxPoints (cmx_launch.hpp)
TABLE = C.c_void_p(0x10)         # a "device" pointer no host code may touch
NONNEG = _abi.CMX_STEP_NONNEGATIVE


def _desc(ft, scheme, fall_speeds=True):
    tps = P.ThermodynamicsParameters(ft)
    if scheme == "sb2006":
        mps, vels, stokes = members_2m(ft)
        if not fall_speeds:
            return ens.pack_2m(mps, tps, vel=None).desc
        return ens.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels, cloud_vel=stokes).desc
    mps, stokes, chen_rain, chen_ice = members_1m(ft)
    if not fall_speeds:
        return ens.pack_1m(mps, tps).desc
    return ens.pack_1m(mps, tps, stokes=stokes, chen_rain=chen_rain, chen_ice=chen_ice).desc


def _copy(d, **kw):
    c = _abi.EnsembleDesc.from_buffer_copy(d)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("scheme", ["sb2006", "mp1m"])
@pytest.mark.parametrize("ft", FTS)
def test_implicit_step_ensemble_argument_ladder_without_gpu(ft, scheme):
    """The statuses of §(29) for the implicit column steps, in their order; TABLE is not a valid address on the host."""
    f = getattr(_lib.lib(), f"cmx_{scheme}_column_implicit_step_ensemble_{ft}")
    d, d_nofall = _desc(ft, scheme), _desc(ft, scheme, fall_speeds=False)
    other = _desc("f64" if ft == "f32" else "f32", scheme)
    in7, out4 = (C.c_void_p * 7)(*[0x1000 * (j + 1) for j in range(7)]), (C.c_void_p * 4)(*[0x9000 + 0x1000 * j for j in range(4)])
    DZ = C.c_void_p(0x100)

    def call(desc, tab, E_, fl, n_col, n_lev=7, dt=300.0, nsub=2, step=NONNEG, arrs=True, drop=None):
        ref = C.byref(desc) if desc is not None else None
        if scheme == "sb2006":
            a = [C.c_void_p(0x1000 * (j + 1)) if arrs else None for j in range(11)]
            if drop is not None:
                a[drop] = None
            return f(ref, tab, E_, fl, dt, nsub, step, n_col, n_lev, DZ if arrs else None, *a, None, None)
        i7 = in7 if arrs else None
        if drop is not None:
            i7 = (C.c_void_p * 7)(*[0 if j == drop else 0x1000 * (j + 1) for j in range(7)])
        return f(ref, tab, E_, fl, dt, nsub, step, n_col, n_lev, DZ if arrs else None, i7, out4 if arrs else None, None, None, None)

    # 1. NULL desc or table — before anything else, bad counts included
    assert call(None, TABLE, E, 0, -1) == BAD
    assert call(d, None, E, 0, 0) == BAD
    # 2. the counts
    assert call(d, TABLE, E, 0, -1) == BAD
    assert call(d, TABLE, E, 0, 5, n_lev=0) == BAD
    assert call(d, TABLE, E, 0, HUGE // 7 + 1) == UNS                                # per member above the single entry's limit …
    assert call(_copy(d, magic=0), TABLE, E, 0, HUGE // 7 + 1) == UNS                # … which comes before the descriptor checks
    # 3. ens_check
    assert call(_copy(d, magic=0), TABLE, E, 0, 0) == BAD
    assert call(_copy(d, scheme=3 - d.scheme), TABLE, E, 0, 0) == BAD
    assert call(other, TABLE, E, 0, 0) == BAD                                        # the other float type
    assert call(d, TABLE, 0, 0, 0) == BAD
    assert call(d, TABLE, E + 1, 0, 0) == BAD                                        # n_members against the desc
    assert call(_copy(d, stride=d.stride + 16), TABLE, E, 0, 0) == BAD
    assert call(d, TABLE, E, 2, 0) == BAD                                            # unknown ens_flags bit
    assert call(_copy(d, n_members=65536), TABLE, 65536, 0, 0) == UNS                # the y limit of a grid
    assert call(_copy(d, n_members=65535), TABLE, 65535, 0, 0, arrs=False) == OK
    # 4. n_col = 0: nothing to do, whatever the arrays, the table's fall speeds and the step arguments are
    assert call(d, TABLE, E, 0, 0, arrs=False) == OK
    assert call(d, TABLE, E, _abi.CMX_ENSEMBLE_SHARED_STATE, 0, arrs=False) == OK
    assert call(d_nofall, TABLE, E, 0, 0, arrs=False, dt=-1.0, nsub=0, step=8) == OK
    # 5. a NULL required array; a table packed without the fall-speed parameters
    assert call(d, TABLE, E, 0, 10, arrs=False) == BAD
    for j in range(7):
        assert call(d, TABLE, E, 0, 10, drop=j) == BAD
    assert call(d_nofall, TABLE, E, 0, 10) == BAD
    # 6. Δt, nsub and the step flags, as implicit_average_step_ok checks them
    for kw in (dict(dt=0.0), dict(dt=-300.0), dict(dt=float("inf")), dict(dt=float("nan")), dict(nsub=0), dict(nsub=-1),
               dict(nsub=_abi.CMX_IMPLICIT_AVERAGE_MAX_NSUB + 1), dict(step=NONNEG | 2), dict(dt=1e-308 if ft == "f64" else 1e-42, nsub=4)):
        assert call(d, TABLE, E, 0, 10, **kw) == BAD, kw


def _pack_2m_bytes(ft, mps, tps, vels, stokes):
    t = ens.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels, cloud_vel=stokes)
    return bytes(t.table.numpy().tobytes()), t.desc.stride


@pytest.mark.parametrize("ft", FTS)
def test_sb2006_block_holds_the_members_latent_heat_ratios(ft):
    """The stride stays a multiple of 16 bytes, a block stays a function of its member alone, and two members that differ only in tps.LH_v0 differ in
    the block — among other constants in Lv, the value before the last one of the block's members, which is LH_v0/cp_d in the float type."""
    mps, vels, stokes = members_2m(ft)
    tps = members_tps(ft)
    both, stride = _pack_2m_bytes(ft, mps[:2], tps[:2], vels[:2], stokes[:2])
    alone, _ = _pack_2m_bytes(ft, mps[1:2], tps[1:2], vels[1:2], stokes[1:2])
    assert stride % 16 == 0 and stride == getattr(_lib.lib(), f"cmx_sb2006_ensemble_table_stride_{ft}")()
    assert both[stride:] == alone and both[:stride] != both[stride:]
    # the same member twice, the second with LH_v0 scaled: the blocks differ, and the Lv slot is one of the differences
    t0, t1 = P.ThermodynamicsParameters(ft), P.ThermodynamicsParameters(ft)
    t1.LH_v0 *= 1.01
    two, _ = _pack_2m_bytes(ft, [mps[0], mps[0]], [t0, t1], [vels[0], vels[0]], [stokes[0], stokes[0]])
    a, b = two[:stride], two[stride:]
    assert a != b
    size, fmt = (4, "<f") if ft == "f32" else (8, "<d")
    # the block: SbConsts, four cloud fall-speed constants, Lv, Ls, then zero padding to the stride
    used = stride
    while used > 0 and a[used - size:used] == bytes(size) and b[used - size:used] == bytes(size):
        used -= size
    lv = [struct.unpack(fmt, blk[used - 2 * size:used - size])[0] for blk in (a, b)]
    ls = [struct.unpack(fmt, blk[used - size:used])[0] for blk in (a, b)]
    rnd = (lambda v: C.c_float(v).value) if ft == "f32" else (lambda v: v)
    assert lv == [rnd(t.LH_v0 / t.cp_d) for t in (t0, t1)] and lv[0] != lv[1]
    assert ls == [rnd(t.LH_s0 / t.cp_d) for t in (t0, t1)] and ls[0] == ls[1]


def test_wrapper_checks_before_any_device_call():
    ft = "f32"
    mps, vels, stokes = members_2m(ft)
    tps = P.ThermodynamicsParameters(ft)
    tab2 = ens.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels)
    m1, s1, cr1, ci1 = members_1m(ft)
    tab1 = ens.pack_1m(m1, tps, stokes=s1, chen_rain=cr1, chen_ice=ci1)
    x = [torch.zeros(E, 2, 4) for _ in range(7)]
    dz = torch.ones(4)
    for f, tab, wrong in ((ens.column_implicit_step_2m, tab2, tab1), (ens.column_implicit_step_1m, tab1, tab2)):
        for dt, nsub in ((0.0, 1), (-1.0, 1), (float("inf"), 1), (300.0, 0), (300.0, 1.5), (300.0, True), (300.0, _abi.CMX_IMPLICIT_AVERAGE_MAX_NSUB + 1)):
            with pytest.raises(ValueError):
                f(tab, dz, *x, dt, nsub)
        with pytest.raises(ValueError, match="GPU"):
            f(tab, dz, *x, 300.0, 2)                                  # CPU columns are refused, as by the single-entry wrappers
        with pytest.raises(TypeError):
            f(wrong, dz, *x, 300.0, 2)                                # a table of the other scheme
        with pytest.raises(TypeError):
            f("table", dz, *x, 300.0, 2)


@pytest.mark.gpu
def test_wrapper_shape_and_aliasing_checks_on_device():
    dev = torch.device("cuda:0")
    ft = "f32"
    mps, vels, stokes = members_2m(ft)
    tps = P.ThermodynamicsParameters(ft)
    tab = ens.pack_2m(mps, tps, vel=cmx.SB2006VelType, vel_params=vels)
    x = [torch.full((E, 2, 4), 1e-3, device=dev) for _ in range(7)]
    dz = torch.ones(4, device=dev)
    with pytest.raises(ValueError, match="device"):
        ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2)                                       # the table is still on the host
    novel = ens.pack_2m(mps, tps, vel=None).to(dev)
    with pytest.raises(ValueError, match="fall-speed"):
        ens.column_implicit_step_2m(novel, dz, *x, 300.0, 2)
    tab = tab.to(dev)
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *[c[:2] for c in x], 300.0, 2)                      # two members of state for three
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2, shared_state=True)                    # a shared state has no member dimension
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *[c.reshape(E, 8) for c in x], 300.0, 2)            # (E, n_col, n_lev) expected
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, torch.ones(5, device=dev), *x, 300.0, 2)                # inv_dz: n_lev values
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *x, 1e-42, 4)                                       # dt / nsub is no normal Float32 number
    mk = lambda shape: torch.empty(shape, device=dev)      # noqa: E731
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2, out=cmx.ColumnTendencies2M(mk((E, 2, 5)), *[mk((E, 2, 4)) for _ in range(3)], None))
    with pytest.raises(ValueError):
        ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2, out=cmx.ColumnTendencies2M(*[mk((E, 2, 4)) for _ in range(4)], mk((E, 3))))
    with pytest.raises(ValueError, match="in place"):
        ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2, out=cmx.ColumnTendencies2M(x[3], *[mk((E, 2, 4)) for _ in range(3)], None))
    out = ens.column_implicit_step_2m(tab, dz, *x, 300.0, 2, want_precip_flux=True)
    assert out.dq_rai_dt.shape == (E, 2, 4) and out.precip_flux.shape == (E, 2)
    m1, s1, cr1, ci1 = members_1m(ft)
    nosed = ens.pack_1m(m1, tps).to(dev)
    with pytest.raises(ValueError, match="stokes"):
        ens.column_implicit_step_1m(nosed, dz, *x, 300.0, 2)
    tab1 = ens.pack_1m(m1, tps, stokes=s1, chen_rain=cr1, chen_ice=ci1).to(dev)
    with pytest.raises(ValueError):
        ens.column_implicit_step_1m(tab1, dz, *[c[0] for c in x], 300.0, 2)                      # no member dimension without shared_state
    o1 = ens.column_implicit_step_1m(tab1, dz, *[c[0] for c in x], 300.0, 2, shared_state=True)
    assert o1.dq_rai_dt.shape == (E, 2, 4) and o1.precip_rai.shape == (E, 2) and o1.precip_sno.shape == (E, 2)
    assert ens.column_implicit_step_1m(tab1, dz, *x, 300.0, 2, precip=False).precip_rai is None
