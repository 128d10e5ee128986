"""What tests/test_implicit_average_host.py and tests/test_implicit_average_gpu.py share for the sub-stepped implicit average (include/cmx.h §19): the call
into the host build tests/native/implicit_average_host.cpp and THE RECIPE — the definition of §19 written out over the implicit entry of §18, once in NumPy
over the host build of that entry (implicit_cases.host_implicit) and once in torch over the device wrappers, every product, sum and select a separate
operation of the float type:

    dt_f = FT(dt);  h = dt_f / FT(nsub);  inv_h = FT(1)/h;  inv_dt = FT(1)/dt_f;  Lv = LH_v0/cp_d;  Ls = LH_s0/cp_d
    repeat nsub times:
        r    = implicit entry (ρ, T, q_tot, s; Δt = h)
        sn_j = s_j + r_j*h
        nonnegative:  lo_j = (s_j < 0 ? s_j : 0);  sn_j = (sn_j < lo_j ? lo_j : sn_j)
        d_j  = (sn_j − s_j) * inv_h
        T    = T + heating(d) * h          SB2006: Lv*(d_0 + d_2); 1-moment: Lv*(d_0 + d_2) + Ls*(d_1 + d_3); toy: no temperature
        s    = sn
    average_j = (s_j − s0_j) * inv_dt
"""
import ctypes as C

import numpy as np

import implicit_cases as IC
import jacobian_products_cases as PC
from jacobian_host_build import NPT, _arr
from cmx import _abi
from cmx import parameters as P

# the option cases of tests/test_implicit_gpu.py::CASES
CASES = [("sb2006", (True, False)), ("sb2006", (False, False)), ("sb2006", (True, True)), ("sb2006", (False, True)), ("mp1m", "default"), ("mp1m", "alt")]
DEFAULT = {"sb2006": (True, False), "mp1m": "default"}
NSUBS = (1, 2, 5)
DTS = (1.0, 30.0, 300.0)
# (index of T among the columns or None, first species column)
LAYOUT = {"sb2006": (1, 3), "mp1m": (1, 3), "toy": (None, 1)}
STATES = {"sb2006": IC.sb2006_states, "mp1m": IC.mp1m_states}


def head(name, ft, case):
    """(parameter object, ctypes head) of a scheme's option case."""
    return PC.head(PC.SCHEMES[name], ft, case)


def constants(ft, dt, nsub, tps=None):
    """(h, inv_h, inv_dt, Lv, Ls) as scalars of the float type, formed as make_mp1m_lin_args forms them."""
    FT = NPT[ft]
    dt_f = FT(dt)
    h = dt_f / FT(nsub)
    tps = tps if tps is not None else P.ThermodynamicsParameters(ft)
    return h, FT(1) / h, FT(1) / dt_f, FT(tps.LH_v0) / FT(tps.cp_d), FT(tps.LH_s0) / FT(tps.cp_d)


def host_average(host, scheme, ft, head_, dt, nsub, cols, nonnegative=True, step_flags=None, k=0, null=(), no_table=False, sentinel=np.nan):
    """([4, n] average, status) of host_<scheme>_implicit_average_<ft>(*head, dt, nsub, step_flags, k, n, x, avg); null: members of `average` left NULL."""
    x = [np.ascontiguousarray(c, dtype=NPT[ft]) for c in cols]
    avg = np.full((4, x[0].size), sentinel, dtype=NPT[ft])
    fn = getattr(host, f"host_{scheme}_implicit_average_{ft}")
    fn.restype = C.c_int32
    flags = (_abi.CMX_STEP_NONNEGATIVE if nonnegative else 0) if step_flags is None else step_flags
    rc = fn(*head_, C.c_double(dt), C.c_int32(nsub), C.c_uint32(flags), C.c_int(k), C.c_int64(x[0].size), _arr(ft, x),
            None if no_table else _arr(ft, [None if q in null else avg[q] for q in range(4)]))
    return avg, rc


def host_recipe(implicit_host, scheme, ft, head_, dt, nsub, cols, nonnegative=True):
    """[4, n] average of the recipe in NumPy over the host build of the implicit entry (tests/native/implicit_host.cpp)."""
    FT = NPT[ft]
    h, inv_h, inv_dt, Lv, Ls = constants(ft, dt, nsub)
    iT, i0 = LAYOUT[scheme]
    x = [np.array(c, dtype=FT) for c in cols]
    s0 = [x[i0 + j].copy() for j in range(4)]
    with np.errstate(all="ignore"):
        for _ in range(nsub):
            r, _, rc = IC.host_implicit(implicit_host, scheme, ft, head_, float(h), x, with_tendencies=False)
            assert rc == _abi.CMX_OK
            d = []
            for j in range(4):
                s = x[i0 + j]
                sn = s + r[j] * h
                if nonnegative:
                    lo = np.where(s < 0, s, FT(0))
                    sn = np.where(sn < lo, lo, sn)
                d.append((sn - s) * inv_h)
                x[i0 + j] = sn
            if scheme == "sb2006":
                x[iT] = x[iT] + (Lv * (d[0] + d[2])) * h
            elif scheme == "mp1m":
                x[iT] = x[iT] + (Lv * (d[0] + d[2]) + Ls * (d[1] + d[3])) * h
        out = np.stack([(x[i0 + j] - s0[j]) * inv_dt for j in range(4)])
    assert out.dtype == FT
    return out


def device_recipe(implicit, name, ft, mp, tps, cols, dt, nsub, nonnegative=True):
    """[4, n] average of the recipe in torch over the device wrapper `implicit` (cmx.warm_rain_implicit_tendencies_2m / cmx.implicit_tendencies_1m): explicit
    torch.mul, torch.add, torch.sub and torch.where, one rounding each; the scalars are exact values of the float type."""
    import torch
    h, inv_h, inv_dt, Lv, Ls = (float(v) for v in constants(ft, dt, nsub, tps))
    iT, i0 = LAYOUT[name]
    x = [c.clone() for c in cols]
    s0 = [x[i0 + j].clone() for j in range(4)]
    zero = torch.zeros((), dtype=x[0].dtype, device=x[0].device)
    for _ in range(nsub):
        r = implicit(mp, tps, *x, h).implicit
        d = []
        for j in range(4):
            s = x[i0 + j]
            sn = torch.add(s, torch.mul(r[j], h))
            if nonnegative:
                lo = torch.where(s < 0, s, zero)
                sn = torch.where(sn < lo, lo, sn)
            d.append(torch.mul(torch.sub(sn, s), inv_h))
            x[i0 + j] = sn
        heat = torch.mul(torch.add(d[0], d[2]), Lv)
        if name == "mp1m":
            heat = torch.add(heat, torch.mul(torch.add(d[1], d[3]), Ls))
        x[iT] = torch.add(x[iT], torch.mul(heat, h))
    return torch.stack([torch.mul(torch.sub(x[i0 + j], s0[j]), inv_dt) for j in range(4)])


def negative_share(ft, avg, cols, dt, i0=3):
    """The share of states at which a species that started ≥ 0 ends below −s0·4 eps:  average·Δt ≥ −s0·(1 + 4 eps) is violated."""
    s0 = np.stack([np.asarray(c, dtype=np.float64) for c in cols[i0:i0 + 4]])
    step = np.asarray(avg, dtype=np.float64) * float(NPT[ft](dt))
    bad = (s0 >= 0) & ~(step >= -s0 * (1.0 + 4.0 * IC.EPS[ft]))
    return float(bad.any(axis=0).mean())
