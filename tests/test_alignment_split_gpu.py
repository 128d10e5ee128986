"""Every streaming entry point splits its points by one rule (csrc/cmx_split.hpp): a scalar head up to the columns' common vector boundary,
the vector body, a scalar tail — or one scalar range when the columns sit at different offsets.  include/cmx.h promises that any alignment
is accepted and gives the same bits.  Here each entry runs on columns at a common shift (every input and output column one or three
elements past an aligned address: head + body + tail) and at mixed shifts (one and two elements: one scalar range), and its outputs must
be bit-identical to the same call on aligned columns.  The two column steps have their own such tests (test_column_gpu.py,
test_mp1m_column.py: ragged shapes and tile invariance)."""
import ctypes as C

import pytest
import torch

from cmx import _abi
from cmx import parameters as P

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
SHIFTS = {"common1": lambda k: 1, "common3": lambda k: 3, "mixed": lambda k: 1 + k % 2}      # element offset of column k


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Layout:
    """Hands out columns of n points, each at SHIFTS[shift](k) elements past an aligned allocation (k counts the columns handed out,
    inputs and outputs alike); shift None: fresh aligned tensors."""

    def __init__(self, shift, n, dtype, dev):
        self.off, self.n, self.dtype, self.dev, self.k = SHIFTS[shift] if shift else (lambda k: 0), n, dtype, dev, 0

    def empty(self):
        o = self.off(self.k)
        self.k += 1
        return torch.empty(self.n + 4, dtype=self.dtype, device=self.dev)[o:o + self.n]

    def copy(self, t):
        return self.empty().copy_(t)


def _check_same_bits(run, ins, shift, n, dtype, dev):
    """run(layout, ins) -> output columns; inputs and outputs from the layout."""
    ref = run(Layout(None, n, dtype, dev), ins)
    got = run(Layout(shift, n, dtype, dev), ins)
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        if shift != "mixed":
            assert a.data_ptr() % 16 != 0
        assert torch.equal(a.view(BITS[dtype]), b.view(BITS[dtype])), f"output {k}"


def _unif(g, n, lo, hi, dtype, dev, log=False):
    x = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    return (10 ** x if log else x).to(dtype).to(dev)


CASES = [(ft, shift, n) for ft in ("f32", "f64") for shift in SHIFTS for n in (3, 4099)]
IDS = [f"{ft}-{shift}-n{n}" for ft, shift, n in CASES]


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_sb2006_tendencies(dev, ft, shift, n):
    import cmx
    from cmx import synthetic
    mp, tps = P.Microphysics2MParams(ft), P.ThermodynamicsParameters(ft)
    st = [c.to(dev) for c in synthetic.sb2006_state(n, dtype=DT[ft], seed=3)]

    def run(lay, ins):
        out = cmx.WarmRainTendencies2M(*[lay.empty() for _ in range(6)])
        cmx.bulk_microphysics_tendencies(cmx.Microphysics2Moment(), mp, tps, *[lay.copy(c) for c in ins], vel=cmx.SB2006VelType, out=out)
        return list(out)
    _check_same_bits(run, st, shift, n, DT[ft], dev)


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
@pytest.mark.parametrize("mode", ["instantaneous", "linearized"])
def test_mp1m_tendencies(dev, ft, shift, n, mode):
    """Instantaneous: f32x4 / one-point-per-lane f64 body.  LinearizedAverage: the f32 packed-pair body (8-byte split)."""
    import cmx
    from cmx import synthetic
    mp, tps = P.Microphysics1MParams(ft), P.ThermodynamicsParameters(ft)
    st = [c.to(dev) for c in synthetic.mp1m_state(n, dtype=DT[ft], seed=4)]
    extra = (cmx.LinearizedAverage(), 30.0, 2) if mode == "linearized" else (cmx.Instantaneous(), None, 1)

    def run(lay, ins):
        out = cmx.Tendencies1M(*[lay.empty() for _ in range(4)])
        cmx.bulk_microphysics_tendencies_1m(extra[0], cmx.Microphysics1Moment(), mp, tps, *[lay.copy(c) for c in ins], extra[1], extra[2], out=out)
        return list(out)
    _check_same_bits(run, st, shift, n, DT[ft], dev)


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_mp0m_tendencies(dev, ft, shift, n):
    """Both outputs (tendency and its q_tot derivative) with the q_vap_sat threshold column."""
    import cmx
    mp = P.Microphysics0MParams(ft)
    g = torch.Generator().manual_seed(5)
    st = [_unif(g, n, -5e-4, 3.5e-3, DT[ft], dev), _unif(g, n, -2e-4, 1.8e-3, DT[ft], dev), _unif(g, n, 0.0, 0.2, DT[ft], dev)]
    fn = getattr(cmx._lib.lib(), f"cmx_mp0m_tendencies_{ft}")

    def run(lay, ins):
        x = [lay.copy(c) for c in ins]
        out = [lay.empty(), lay.empty()]
        rc = fn(C.byref(mp.precip), n, *[C.c_void_p(t.data_ptr()) for t in x + out], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0
        return out
    _check_same_bits(run, st, shift, n, DT[ft], dev)


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_ice_nucleation(dev, ft, shift, n):
    import cmx
    from cmx import synthetic
    tps, du, koop = P.ThermodynamicsParameters(ft), P.Kaolinite(ft), P.Koop2000(ft)
    st = [c.to(dev) for c in synthetic.ice_nucleation_state(n, dtype=DT[ft], seed=6)]
    counts = []

    def run(lay, ins):
        nerr = torch.zeros(_abi.CMX_ICENUC_ERR_WORDS, dtype=torch.int64, device=dev)
        out = cmx.IceNucleationRates(*[lay.empty() for _ in range(5)], nerr)
        cmx.ice_nucleation_rates(tps, du, koop, *[lay.copy(c) for c in ins], want=out._fields[:5], out=out)
        counts.append(cmx.domain_error_count(out))
        return list(out[:5])
    _check_same_bits(run, st, shift, n, DT[ft], dev)
    assert counts[0] == counts[1]


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_cloud_diagnostics(dev, ft, shift, n):
    from cmx import cloud_diagnostics as CD
    rain = P.Microphysics1MParams(ft).c.rain
    sb = P.SB2006(P.create_toml_dict(ft, P.SB2006_LIMITERS_OVERRIDE), True)
    g = torch.Generator().manual_seed(7)
    st = [_unif(g, n, 0.3, 1.3, DT[ft], dev), _unif(g, n, -8, -2.5, DT[ft], dev, log=True), _unif(g, n, -9, -2.5, DT[ft], dev, log=True),
          _unif(g, n, 5, 9.5, DT[ft], dev, log=True), _unif(g, n, 0, 6.5, DT[ft], dev, log=True)]
    st[2][::3] = 0                                                   # no rain at every third point

    def run(lay, ins):
        out = CD.Diagnostics(*[lay.empty() for _ in range(4)])
        CD.cloud_diagnostics(rain, sb, 1000.0, *[lay.copy(c) for c in ins], out=out)
        return list(out)
    _check_same_bits(run, st, shift, n, DT[ft], dev)


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_arg_activation_per_mode(dev, ft, shift, n):
    """Shared distribution (5 modes): number, mass and S_max; the four optional sink columns are absent (NULL)."""
    import cmx
    from cmx import synthetic
    ap, aip, tps = P.AerosolActivationParameters(ft), P.AirProperties(ft), P.ThermodynamicsParameters(ft)
    ad = synthetic.arg_config3_distribution()
    st = [c.to(dev) for c in synthetic.arg_state(n, dtype=DT[ft], seed=8)]

    def run(lay, ins):
        x = [lay.copy(c) for c in ins]
        out = ([lay.empty() for _ in range(5)], [lay.empty() for _ in range(5)], lay.empty())
        cmx.aerosol_activation(ap, ad, aip, tps, *x, want=("N_act", "M_act", "S_max"), out=out)
        return out[0] + out[1] + [out[2]]
    _check_same_bits(run, st, shift, n, DT[ft], dev)


@pytest.mark.parametrize("ft,shift,n", CASES, ids=IDS)
def test_arg_activation_columns(dev, ft, shift, n):
    """Per-element aerosol (3 modes from columns, molar mass included): the mode columns are split with the state."""
    import cmx
    from cmx import synthetic
    ap, aip, tps = P.AerosolActivationParameters(ft), P.AirProperties(ft), P.ThermodynamicsParameters(ft)
    st = [c.to(dev) for c in synthetic.arg_state(n, dtype=DT[ft], seed=9)]
    g = torch.Generator().manual_seed(10)
    modes = [[_unif(g, n, -8.0, -6.0, DT[ft], dev, log=True), _unif(g, n, 1.3, 2.2, DT[ft], dev), _unif(g, n, 6.0, 9.5, DT[ft], dev, log=True),
              _unif(g, n, 0.1, 1.3, DT[ft], dev), _unif(g, n, 0.05, 0.15, DT[ft], dev)] for _ in range(3)]
    flat = st + [c for m in modes for c in m]

    def run(lay, ins):
        x = [lay.copy(c) for c in ins]
        mc = [cmx.ModeColumns(*x[4 + 5 * k:9 + 5 * k]) for k in range(3)]
        out = cmx.ActivationResult([lay.empty() for _ in range(3)], [lay.empty() for _ in range(3)], lay.empty())
        cmx.aerosol_activation_columns(ap, mc, aip, tps, *x[:4], want=("N_act", "M_act", "S_max"), out=out)
        return out.N_act + out.M_act + [out.S_max]
    _check_same_bits(run, flat, shift, n, DT[ft], dev)
