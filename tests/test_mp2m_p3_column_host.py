"""The 2M + P3 column step without a GPU: every status of the entry's argument checks (each returns before any HIP runtime call — the column
addresses below are never dereferenced) in the order include/cmx.h (9b) states, and the wrapper's TypeError / ValueError cases (raised
before the library is called)."""
import ctypes as C

import pytest
import torch

from cmx import _abi, _lib
from cmx import parameters as P

_OK, _BAD, _UNS = _abi.CMX_OK, _abi.CMX_ERR_BAD_ARG, _abi.CMX_ERR_UNSUPPORTED
SB, CHEN = _abi.CMX_P3COL_VEL_SB2006, _abi.CMX_P3COL_VEL_CHEN2022
FAKE = 4096          # a non-NULL "device address"


class _Call:
    """Default-valid arguments of cmx_mp2m_p3_column_tendencies_sedimentation_<ft>; `run(**changes)` calls the entry with some replaced."""

    def __init__(self, ft, limited=True):
        self.fn = getattr(_lib.lib(), f"cmx_mp2m_p3_column_tendencies_sedimentation_{ft}")
        self.mp = P.Microphysics2MParams(ft, with_ice=True, is_limited=limited)
        self.tps = P.ThermodynamicsParameters(ft)
        self.vel = P.rain_vel_params(ft)
        self.stokes = P.StokesRegimeVelType(ft)
        self.ins = (C.c_void_p * 13)(*[FAKE] * 13)
        self.outs = (C.c_void_p * 8)(*[FAKE] * 8)
        self.base = dict(wr=C.pointer(self.mp.warm_rain.c), ice=C.pointer(self.mp.ice.c), tps=C.pointer(self.tps), vel=C.pointer(self.vel), cloud=None,
                         flags=self.mp.ice.flags | SB, brent=0, p=1e-6, n_col=3, n_lev=5, inv_dz=FAKE, ins=self.ins, outs=self.outs, ll=FAKE, v_n=FAKE,
                         v_m=FAKE, pr=None, pi=None)

    def run(self, **kw):
        a = dict(self.base, **kw)
        return self.fn(a["wr"], a["ice"], a["tps"], a["vel"], a["cloud"], a["flags"], a["brent"], a["p"], a["n_col"], a["n_lev"], a["inv_dz"], a["ins"],
                       a["outs"], a["ll"], a["v_n"], a["v_m"], a["pr"], a["pi"], None)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_every_status_in_check_order(ft):
    c = _Call(ft)
    lim = c.mp.ice.flags
    # parameter structs, the two host arrays, the counts
    for k in ("wr", "ice", "tps", "vel", "ins", "outs"):
        assert c.run(**{k: None}) == _BAD, k
    assert c.run(n_col=-1) == _BAD
    assert c.run(n_lev=0) == _BAD and c.run(n_lev=-3) == _BAD
    # flags: an unknown bit (CMX_P3_INPUT_IS_STATE is not a flag of this entry), both or neither velocity scheme
    assert c.run(flags=lim | SB | _abi.CMX_P3_INPUT_IS_STATE) == _BAD
    assert c.run(flags=lim | SB | (1 << 10)) == _BAD
    assert c.run(flags=lim) == _BAD
    assert c.run(flags=lim | SB | CHEN) == _BAD
    # … each of these before the size rule: a bad flag with an oversized count is a bad argument
    huge = 16 * 0x7fffffff // 5 + 1
    assert c.run(flags=lim, n_col=huge) == _BAD
    # n_col · n_lev above one launch
    assert c.run(n_col=huge) == _UNS
    assert c.run(n_col=16 * 0x7fffffff + 1, n_lev=1) == _UNS
    assert c.run(n_col=4 * (0x7fffffff - 7) + 1, n_lev=1) == _UNS          # the collision kernel's smallest tile (4 states)
    # no columns: OK whatever the column pointers are (the checks above still apply)
    empty = (C.c_void_p * 13)()
    assert c.run(n_col=0) == _OK
    assert c.run(n_col=0, inv_dz=None, ins=empty, outs=(C.c_void_p * 8)(), ll=None, v_n=None, v_m=None) == _OK
    assert c.run(n_col=0, flags=lim) == _BAD
    # a NULL required column
    for k in ("inv_dz", "ll", "v_n", "v_m"):
        assert c.run(**{k: None}) == _BAD, k
    for j in range(11):
        ins = (C.c_void_p * 13)(*[FAKE] * 13)
        ins[j] = None
        assert c.run(ins=ins) == _BAD, j
    for j in range(8):
        outs = (C.c_void_p * 8)(*[FAKE] * 8)
        outs[j] = None
        assert c.run(outs=outs) == _BAD, j
    # the quantile level and the quadrature order of steps 1 and 2, refused before the first launch
    for p in (0.0, 0.5, -1e-6, float("nan")):
        assert c.run(p=p) == _BAD, p
    n_quad = c.mp.ice.c.quad.n
    for n in (0, _abi.CMX_QUAD_MAX + 1):
        c.mp.ice.c.quad.n = n
        assert c.run() == _BAD, n
    c.mp.ice.c.quad.n = n_quad


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_parameter_domain_checks(ft):
    """The limited rain PSD needs ordered limiter pairs, the not-limited SB2006 fall speed aR < bR — as for the 2M column step."""
    c = _Call(ft, limited=False)
    assert c.mp.ice.flags & _abi.CMX_P3_RAIN_PDF_LIMITED == 0
    assert c.run(flags=c.mp.ice.flags | SB | _abi.CMX_P3_RAIN_PDF_LIMITED) == _BAD       # a struct without limiters, asked for the limited PSD
    aR = c.vel.sb2006.aR
    c.vel.sb2006.aR = c.vel.sb2006.bR
    assert c.run() == _BAD
    c.vel.sb2006.aR = aR


def test_optional_columns_may_be_null_at_the_abi():
    """log_lambda_guess and inpc_log_shift (in[11], in[12]), cloud_vel and both precipitation outputs are optional: with n_col = 0 nothing is
    launched, and the NULLs are not what a status is returned for."""
    c = _Call("f32")
    ins = (C.c_void_p * 13)(*[FAKE] * 11, None, None)
    assert c.run(n_col=0, ins=ins, cloud=None, pr=None, pi=None) == _OK
    assert c.run(n_col=0, ins=ins, cloud=C.pointer(c.stokes), pr=FAKE, pi=FAKE, flags=c.mp.ice.flags | CHEN | _abi.CMX_P3_NO_ASPECT_RATIO) == _OK


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: the wrapper's checks run, the library is never reached."""
    @property
    def is_cuda(self):
        return True


def _cols(ft, n_col=4, n_lev=6):
    dt = torch.float32 if ft == "f32" else torch.float64
    return [torch.ones(n_col, n_lev, dtype=dt).as_subclass(_FakeCuda) for _ in range(11)], torch.ones(n_lev, dtype=dt).as_subclass(_FakeCuda)


def test_wrapper_type_and_value_errors():
    import cmx
    ft = "f32"
    cols, inv_dz = _cols(ft)
    mp, tps = P.Microphysics2MParams(ft, with_ice=True), P.ThermodynamicsParameters(ft)
    f = cmx.column_tendencies_sedimentation_2m_p3
    with pytest.raises(TypeError):
        f(P.Microphysics2MParams(ft), tps, inv_dz, *cols)                                   # no ice parameters
    with pytest.raises(TypeError):
        f(P.WarmRainParams2M(ft), tps, inv_dz, *cols)
    with pytest.raises(TypeError):
        f(P.Microphysics2MParams("f64", with_ice=True), tps, inv_dz, *cols)                 # float type of the parameters
    with pytest.raises(TypeError):
        f(mp, P.ThermodynamicsParameters("f64"), inv_dz, *cols)
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, cloud_vel=P.StokesRegimeVelType("f64"))
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, vel_params=P.rain_vel_params("f64"))
    with pytest.raises(TypeError):
        f(mp, tps, inv_dz, *cols, vel=object())
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, vel=None)                                                 # the column step needs a rain fall-speed scheme
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz[:5], *cols)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz.double(), *cols)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *[c.reshape(-1) for c in cols])                                  # not (n_col, n_lev)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10][:, :5])                                     # a column of another shape
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10].double())
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols[:10], cols[10].t().contiguous().t())                       # not contiguous
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, log_lambda_guess=cols[0][:, :5])
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, inpc_log_shift=cols[0].double())
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *[torch.ones(4, 6) for _ in range(11)])                          # not on the GPU
    mixed = P.Microphysics2MParams(ft, with_ice=True)
    mixed.ice = P.P3IceParams(ft, is_limited=False)
    with pytest.raises(ValueError):
        f(mixed, tps, inv_dz, *cols)                                                        # warm_rain and ice disagree on is_limited
    bad_out = cmx.ColumnTendencies2MP3(*[torch.ones(4, 6).as_subclass(_FakeCuda) for _ in range(10)], torch.ones(4, 5).as_subclass(_FakeCuda), None, None)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, out=bad_out)
    bad_pf = cmx.ColumnTendencies2MP3(*[torch.ones(4, 6).as_subclass(_FakeCuda) for _ in range(11)], torch.ones(3).as_subclass(_FakeCuda), None)
    with pytest.raises(ValueError):
        f(mp, tps, inv_dz, *cols, out=bad_pf)


def test_public_names():
    import cmx
    assert cmx.ColumnTendencies2MP3._fields == ("dq_lcl_dt", "dn_lcl_dt", "dq_rai_dt", "dn_rai_dt", "dq_ice_dt", "dn_ice_dt", "dq_rim_dt", "db_rim_dt",
                                                "log_lambda", "v_ice_n", "v_ice_m", "precip_rai", "precip_ice")
    assert cmx.column_tendencies_sedimentation_2m_p3 is cmx.bulk_tendencies.column_tendencies_sedimentation_2m_p3
    # the rain fall-speed choice has bits of its own in this entry's flag word: bits 1 and 2 are P3 flags there
    p3 = _abi.CMX_P3_INPUT_IS_STATE | _abi.CMX_P3_SLOPE_CONSTANT | _abi.CMX_P3_NO_ASPECT_RATIO | _abi.CMX_P3_RAIN_PDF_LIMITED
    assert (SB | CHEN) & p3 == 0 and SB != CHEN
