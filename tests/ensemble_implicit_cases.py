"""What the tests of the ensemble forms of the implicit column steps share (tests/test_ensemble_implicit_host.py, tests/test_ensemble_implicit_gpu.py)
beyond tests/ensemble_cases.py: the members' thermodynamics parameters — member 1 has its own latent heats, so the per-member Lv and Ls of the substeps
are exercised — and the ensemble call next to the E single calls it replaces."""
import torch

from cmx import parameters as P
from ensemble_cases import E, members_1m, members_2m

DT_STEP, NSUB = 300.0, 2      # Δt of a single-column model; two substeps, so that the latent heating of the first feeds the second
RUNTIME_1M = {"snow_autoconversion": P.WithSupersaturation, "rain_autoconversion": P.PrescribedNd}      # the run-time-flags option set of test_ensemble_gpu.py


def members_tps(ft, n_members=E):
    """One cmx_thermo struct per member: the default set, but member 1 with LH_v0 and LH_s0 moved by about 1 %."""
    tps = [P.ThermodynamicsParameters(ft) for _ in range(n_members)]
    if n_members > 1:
        tps[1].LH_v0 *= 1.01
        tps[1].LH_s0 *= 0.99
    return tps


def vel_type(name):
    import cmx
    return {"sb": cmx.SB2006VelType, "chen": cmx.Chen2022VelTypeRain}[name]


def step_2m(dev, ft, limited, vel, cloud, dz, cols, n_members=E, shared=False, out=None, want_precip_flux=True, singles=True, tps=None):
    """(ensemble result, [single result per member]) of the SB2006 implicit column step."""
    import cmx
    mps, vels, stokes = members_2m(ft, limited, n_members)
    tps = members_tps(ft, n_members) if tps is None else tps
    tab = cmx.ensemble.pack_2m(mps, tps, vel=vel_type(vel), vel_params=vels, cloud_vel=stokes if cloud else None).to(dev)
    got = cmx.ensemble.column_implicit_step_2m(tab, dz, *cols, DT_STEP, NSUB, True, shared_state=shared, want_precip_flux=want_precip_flux, out=out)
    refs = []
    if singles:
        refs = [cmx.column_implicit_step_2m(mps[e], tps[e], dz, *[c if shared else c[e] for c in cols], DT_STEP, NSUB, True, vel=vel_type(vel),
                                            vel_params=vels[e], cloud_vel=stokes[e] if cloud else None, want_precip_flux=want_precip_flux)
                for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs


def step_1m(dev, ft, options, dz, cols, n_members=E, shared=False, precip=True, singles=True, tps=None):
    """(ensemble result, [single result per member]) of the 1-moment implicit column step."""
    import cmx
    mps, stokes, chen_rain, chen_ice = members_1m(ft, n_members, **options)
    tps = members_tps(ft, n_members) if tps is None else tps
    tab = cmx.ensemble.pack_1m(mps, tps, stokes=stokes, chen_rain=chen_rain, chen_ice=chen_ice).to(dev)
    assert tab.desc.runtime_flags == (1 if options else 0)
    got = cmx.ensemble.column_implicit_step_1m(tab, dz, *cols, DT_STEP, NSUB, True, shared_state=shared, precip=precip)
    refs = []
    if singles:
        refs = [cmx.column_implicit_step_1m(mps[e], tps[e], stokes[e], chen_rain[e], chen_ice[e], dz, *[c if shared else c[e] for c in cols], DT_STEP, NSUB,
                                            True, precip=precip) for e in range(n_members)]
    torch.cuda.synchronize()
    return got, refs
