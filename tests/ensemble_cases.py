"""Members and states of the parameter-ensemble tests (tests/test_ensemble_host.py, tests/test_ensemble_gpu.py): E = 3 parameter sets per scheme that differ
visibly — a rate coefficient, a limiter and a fall-speed coefficient each moved by 5–30 % — and agree in every choice the library makes from parameter
values (integer SB2006 exponents, fitted Γ of the Chen-2022 rain table, default 1-moment exponents), so that one table holds them."""
import torch

from cmx import parameters as P

E = 3
DT = {"f32": torch.float32, "f64": torch.float64}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64}

# member 0 is the default set
_SCALE_2M = [
    {},
    {"acnv.kcc": 1.2, "pdf_r.N0_max": 0.8, "pdf_r.lambda_max": 0.9, "evap.av": 1.1},
    {"acnv.kcc": 0.8, "accr.kcr": 1.3, "pdf_r.N0_min": 1.25, "pdf_r.xr_max": 0.85, "brek.kbr": 1.15},
]
_SCALE_VEL = [{}, {"sb2006.bR": 1.1, "chen2022.a0": 1.1}, {"sb2006.aR": 0.93, "sb2006.cR": 1.2, "chen2022.a2": 0.9}]
_SCALE_STOKES = [1.0, 1.15, 0.9]      # nu_air


def members_2m(ft, limited=True, n_members=E):
    """(mps, vel_params, cloud_vel): lists of WarmRainParams2M, cmx_rain_vel and cmx_stokes_vel structs."""
    mps, vels, stokes = [], [], []
    for e in range(n_members):
        wr = P.WarmRainParams2M(ft, limited)
        sb = wr.c.seifert_beheng
        for path, f in _SCALE_2M[e].items():
            grp, name = path.split(".")
            setattr(getattr(sb, grp), name, getattr(getattr(sb, grp), name) * f)
        vel = P.rain_vel_params(ft)
        for path, f in _SCALE_VEL[e].items():
            grp, name = path.split(".")
            if name in ("a0", "a1", "a2"):
                vel.chen2022.a[int(name[1])] *= f
            else:
                setattr(getattr(vel, grp), name, getattr(getattr(vel, grp), name) * f)
        st = P.StokesRegimeVelType(ft)
        st.nu_air *= _SCALE_STOKES[e]
        mps.append(wr)
        vels.append(vel)
        stokes.append(st)
    return mps, vels, stokes


def members_1m(ft, n_members=E, **options):
    """(mps, stokes, chen_rain, chen_ice): lists of Microphysics1MParams and the three fall-speed structs."""
    mps, stokes, chen_rain, chen_ice = [], [], [], []
    for e in range(n_members):
        mp = P.Microphysics1MParams(ft, **options)
        st, cr, ci = P.StokesRegimeVelType(ft), P.Chen2022VelTypeRain(ft), P.Chen2022VelTypeIce(ft)
        if e == 1:
            mp.c.process_params.e_lcl_rai *= 1.2               # a rate coefficient
            mp.c.process_params.rain_autoconversion.q_threshold *= 0.8      # a limiter
            mp.c.process_params.snow_autoconversion.tau *= 1.3
            cr.a[0] *= 1.1                                     # fall-speed coefficients
            ci.large_ice.A[0] *= 1.05
            st.nu_air *= 1.15
        if e == 2:
            mp.c.process_params.e_rai_sno *= 0.75
            mp.c.process_params.rain_autoconversion.tau *= 0.7
            mp.c.process_params.snow_autoconversion.q_threshold *= 1.25
            mp.c.rain.n0 *= 1.2
            cr.a[1] *= 0.9
            ci.small_ice.A[0] *= 0.95
            st.nu_air *= 0.9
        mps.append(mp)
        stokes.append(st)
        chen_rain.append(cr)
        chen_ice.append(ci)
    return mps, stokes, chen_rain, chen_ice


def state_2m(shape, ft, device="cpu", seed=21):
    from cmx import synthetic
    n = 1
    for s in shape:
        n *= s
    return [c.reshape(shape).contiguous().to(device) for c in synthetic.sb2006_state(n, dtype=DT[ft], seed=seed)]


def state_1m(shape, ft, device="cpu", seed=22):
    from cmx import synthetic
    n = 1
    for s in shape:
        n *= s
    return [c.reshape(shape).contiguous().to(device) for c in synthetic.mp1m_state(n, dtype=DT[ft], seed=seed)]


def inv_dz(n_lev, ft, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    return (1.0 / (30.0 + 470.0 * torch.rand(n_lev, generator=g, dtype=torch.float64))).to(DT[ft]).to(device)


def same_bits(a, b):
    """Bit equality of two tensors (NaN payloads and the sign of zero included); None equals None."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))
