"""Gates of the schemes at and around their thresholds: the catalogue, the ladders, the reference and the checker shared by
tests/test_gates_host.py and tests/test_gates_gpu.py.

Everywhere else in the suite the points next to a discontinuity of a scheme are set aside (`near_branch` / `near_gate` / `near_clip`) and nothing is
asserted about them.  Here every such point gets an assertion of its own.  A case is a LADDER: one input column runs through consecutive values of the
kernel's float type FT centred on a threshold, every other column is held at a fixed state in which all species are present.

RAW gates (`raw_cases`) compare an input column (or N = ρ·n with ρ = 1, so N = n exactly) with a constant.  17 rungs: the threshold and its 8 neighbours
on each side (`np.nextafter` steps).  Asserted at all 17 rungs, nothing set aside: every column is exactly 0 where the reference's is exactly 0 and
non-zero where the reference's is, and every column meets the ordinary bound of tests/parity.py.

  SB2006 (process rates, fused tendencies with the SB2006 fall speeds; limited and not limited), state ρ = 1, T = 285, q_tot = 7e-3, q_lcl = 1e-3,
  N_lcl = 1e8, q_rai = 5e-4, N_rai = 1e4 (S = −0.48: evaporation is on); the not-limited N_rai ladders hold q_rai = 4·eps(FT) (see raw_cases):
    q_lcl < eps(FT)   CM2:420, :463     open at eps      autoconversion, accretion, cloud self-collection
    q_rai < eps(FT)   CM2:463, :558     open at eps      accretion, rain self-collection, evaporation
    N_lcl < eps(FT)   CM2:420, :463     open at eps      autoconversion, accretion
    N_rai < eps(FT)   CM2:558           open at eps      rain self-collection, breakup, number-weighted fall speed
    N_rai ≤ eps(FT)   CM2:824, S < 0    closed at eps    evaporation (both moments; process rates only: 1e-9 of the fused sums and less)
  cmx_bulk_2m_cloud_to_rain_* (LD2004, step threshold), ρ = 1, N_d = 1e3 (Float32) / 1e-9 (Float64) so that R_6 > R_6C at q_lcl = eps(FT):
    q_lcl ≤ eps(FT)   CM2:951           closed at eps    autoconversion
  1-moment (source terms and tendencies), state ρ = 1, T = 270, q_tot = 6e-3, q_lcl = 1e-3, q_icl = 2e-4, q_rai = 5e-4, q_sno = 3e-4, ϵ = cbrt(floatmin(FT)):
    q_lcl, q_icl, q_rai, q_sno > ϵ   cmx_mp1m.hpp has_*   closed at ϵ   the accretion terms of that species
  1-moment, T against T_freeze (the FT-rounded parameter), same state with q_tot = 8e-3 (q_vap above saturation over ice: deposition is on):
    T ≥ T_freeze   BMT:174 is_warm                open at T_freeze     warm / cold accretion pairs                     default, tdep
    T > T_freeze   NonEq:59 deposition limit      closed at T_freeze   deposition on cloud ice is allowed AT T_freeze  default
    T < T_freeze   CM1:444 WithSupersaturation    closed at T_freeze   ice autoconversion                              supersat
  (with `tdep` the INP number tends to 0 as T → T_freeze, so the deposition rate is continuous there and the limit itself shows in the default set;
  the `tdep` ladder pins the routing and the finite, small deposition next to the threshold.  The melt terms ∝ max(T − T_freeze, 0) are continuous.)
The open-side magnitudes are measured on the reference and asserted to be above parity.FLOOR in tests/test_gates_host.py (`open_magnitude`).

THE REFERENCE of a ladder is the oracle in Float64 arithmetic with every threshold set to the value the FT kernel holds: `float32_gates` for the eps
family, and for T_freeze in Float32 the parameter `temperature_water_freeze` overridden with its Float32-rounded value (273.149993896484375) through
`P.ParamDict("f64", {...})` handed to both Microphysics1MParams and ThermodynamicsParameters.  Without the override the Float64 oracle compares
T = float32(273.15) with the double 273.15 and calls it cold; a Float32 reference, whose T_freeze IS that float, calls it warm.

COMPUTED gates (`computed_cases`) compare a quantity formed in the kernel.  The threshold is located by bisecting the Float64 oracle along one input
(no closed formula: the limited PSD moves x̄_r), the ladder has 4097 rungs — consecutive floats in Float32, a constant power-of-two ulp stride in Float64,
the smallest that keeps at most 25 % of the ladder inside the margin:
    Φ_br at Dr = Dr_th (CM2:596)          along q_rai   limited, not limited     margin |Dr/Dr_th − 1| ≤ 1e-5 / 1e-11 (the oracle's `branch_margin`, unchanged)
    clip x̄_c = x* (CM2:406)               along q_lcl   susceptibilities         margin |x̄_c/x* − 1| < 1e-5 (`near_clip`, unchanged, both float types)
    x̄_r/x* < eps(FT) of evaporation :824   along N_rai   not limited              margin 1e-5 / 1e-11 relative in x̄_r (NEW: this gate had none)
Outside the margin: the ordinary bound and the reference's side.  Inside: every output finite, and within the ordinary bound of the reference at the
last rung below the margin or at the first rung above it, that bound widened by the change of the same reference column between the two outermost
rungs inside the margin on that side.  `switch_window` gives the rungs at which the side the outputs show differs from the reference's.
The evaporation number gate turns out to be invisible in the outputs: at x̄_r = eps(FT)·x* the factor e^{−t*} with t* = ∛(6 x*/x̄_r) = ∛(6/eps) is
e^{−369} (Float32 gate) or e^{−3e5} (Float64 gate), so the number tendency on its open side is ≤ 1e-118 in the first case and −0 in the second.  The
threshold is still bisected on the oracle's own output (its sign bit) and the ladder is held to the same assertions; tests/test_gates_host.py asserts on
the reference that the open side stays below parity.FLOOR, i.e. that no placement of this gate inside the ladder can move an output.

Zero pattern: every column must be exactly 0 where the reference's is exactly 0.  The other direction — non-zero where the reference's is — is asserted
literally for the gated (`watch`) columns of a case, which are products far from zero, and for every other column through the ordinary bound: a zero
fails it unless the bound itself admits 0, which happens only where the reference value is rounding of its operands (|ref| ≤ CTOL·scale: the Kessler
logistic integral at q_lcl = 2.3e-13 is 3.1e-17 against operands of 1e-13 and is 0 in Float32 arithmetic, the reference's own included) or below
parity.FLOOR, "zero for the kernel's float type" everywhere in this suite (the hardware transcendental units flush subnormals).

Test infrastructure only: imports neither torch nor the device library.  A `run(case, cols)` callable (oracle, host build or device) maps the columns
of a case to {output name: array}."""
import dataclasses

import numpy as np

import parity
import precip_susceptibility_ref as R
from cmx import _abi
from cmx import parameters as P

NPT = {"f32": np.float32, "f64": np.float64}
INT = {"f32": np.int32, "f64": np.int64}
EPS = {ft: float(np.finfo(NPT[ft]).eps) for ft in NPT}                                  # ϵ_numerics_2M_* = eps(FT)
EPS_1M = {"f32": float(np.cbrt(np.finfo(np.float32).tiny)), "f64": float(np.cbrt(np.finfo(np.float64).tiny))}   # ϵ_numerics = cbrt(floatmin(FT))
T_FREEZE = P.DEFAULT_PARAMETERS["temperature_water_freeze"]
T_FREEZE_FT = {"f32": float(np.float32(T_FREEZE)), "f64": T_FREEZE}
MARGIN = {"f32": 1e-5, "f64": 1e-11}          # branch_margin of the oracle (Dr) — also taken for the evaporation number gate (x̄_r)
CLIP_MARGIN = 1e-5                            # near_clip
HALF_RAW, HALF_COMPUTED = 8, 2048
MAX_INSIDE, MIN_OUTSIDE = 0.25, 64

COLUMNS = {
    "sb_proc": ("q_tot", "q_lcl", "q_rai", "N_lcl", "N_rai", "rho", "T"),
    "sb_fused": ("rho", "T", "q_tot", "q_lcl", "n_lcl", "q_rai", "n_rai"),
    "bulk2m": ("q_lcl", "rho", "N_d"),
    "mp1m": ("rho", "T", "q_tot", "q_lcl", "q_icl", "q_rai", "q_sno"),
    "susc": ("q_lcl", "q_rai", "rho", "N_lcl"),
}
SB_STATE = dict(rho=1.0, T=285.0, q_tot=7e-3, q_lcl=1e-3, N_lcl=1e8, q_rai=5e-4, N_rai=1e4)
MP1M_STATE = dict(rho=1.0, T=270.0, q_tot=6e-3, q_lcl=1e-3, q_icl=2e-4, q_rai=5e-4, q_sno=3e-4)
SUSC_STATE = dict(q_lcl=1e-3, q_rai=1e-4, rho=1.0, N_lcl=1e7)
MP1M_OPTIONS = {
    "default": {},
    "supersat": dict(snow_autoconversion=P.WithSupersaturation()),
    "tdep": dict(cloud_ice_formation=P.TemperatureDependent()),          # the "tdep" set of tests/test_mp1m_gpu.py
}
TENDENCIES_1M = ("dq_lcl_dt", "dq_icl_dt", "dq_rai_dt", "dq_sno_dt")
# the tendency whose Σ|terms| is the operand scale of a cancelling source term (tests/test_mp1m_gpu.py)
CANCEL_1M = {"S_phase_change_vap_lcl": "dq_lcl_dt", "S_phase_change_vap_icl": "dq_icl_dt", "S_phase_change_vap_rai": "dq_rai_dt",
             "S_phase_change_vap_sno": "dq_sno_dt", "S_melt_icl_lcl": "dq_icl_dt", "S_melt_sno_rai": "dq_sno_dt",
             "S_accr_melt_lcl_sno": "dq_sno_dt", "S_accr_melt_rai_sno": "dq_sno_dt", "S_acnv_icl_sno": "dq_icl_dt", "S_acnv_lcl_rai": "dq_lcl_dt"}
SUSC_OUTS = ("acnv_d_ln_q_lcl", "acnv_d_ln_q_rai", "acnv_d_ln_N_lcl", "accr_d_ln_q_lcl", "accr_d_ln_q_rai", "accr_d_ln_N_lcl")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str                 # key of COLUMNS: which entry the ladder runs through
    ft: str
    var: str                    # the column that runs through the ladder
    center: float               # the threshold as an FT value
    state: tuple                # ((column, value), …) of the other columns
    predicate: str = ""         # the reference's comparison, for the catalogue
    open_above: bool = True     # the watched process is on for var above the threshold
    open_at_exact: bool = True  # … and at the threshold itself
    watch: tuple = ()           # columns that are exactly 0 on the closed side and far from 0 on the open side
    limited: bool = True
    optset: str = "default"
    half: int = HALF_RAW
    stride: int = 1
    margin: float = 0.0         # computed gates only
    gate: str = ""              # computed gates: "breakup" | "clip" | "evap_number"

    @property
    def computed(self):
        return bool(self.gate)

    @property
    def n(self):
        return 2 * self.half + 1

    def values(self, shift=0):
        return rungs(self.center, self.ft, self.half, self.stride, shift)

    def columns(self, shift=0):
        """name → FT column of the ladder (`shift`: the whole ladder moved by that many rungs)"""
        st = dict(self.state)
        v = self.values(shift)
        return {k: (v if k == self.var else np.full(v.size, st[k], dtype=NPT[self.ft])) for k in COLUMNS[self.family]}


def rungs(center, ft, half, stride=1, shift=0):
    """2·half + 1 values of FT, `stride` ulps apart, centred on FT(center) (+ shift rungs); positive values only"""
    c = np.array([center], dtype=NPT[ft])
    assert c[0] > 0 and np.isfinite(c[0])
    k = (np.arange(-half, half + 1, dtype=np.int64) + int(shift)) * int(stride)
    return (c.view(INT[ft]).astype(np.int64) + k).astype(INT[ft]).view(NPT[ft])


def _state(base, var, **over):
    st = dict(base)
    st.update(over)
    st.pop(var, None)
    return tuple(sorted(st.items()))


# ---- (a) the raw gates ---------------------------------------------------------------------------------------------------------------------

def raw_cases(ft):
    eps, e1 = EPS[ft], EPS_1M[ft]
    out = []
    for limited in (True, False):
        tag = "limited" if limited else "notlimited"
        # N_rai = eps(FT) under q_rai ≥ eps(FT) means drops of ≥ 1 kg: the limited PSD clamps them to xr_max, the not-limited one takes them as they are
        # (e^{κ_br ΔD} overflows Float32 and, above q_rai ≈ 1e-5, Float64), so its N_rai ladders hold the smallest q_rai the gate q_rai < eps(FT) allows
        rain = {} if limited else dict(q_rai=4 * eps)
        sb = [
            ("q_lcl", "q_lcl", "q_lcl < eps(FT)", True, ("acnv_dq_rai_dt", "accr_dq_rai_dt", "lcl_self_collection"), {}, True),
            ("q_rai", "q_rai", "q_rai < eps(FT)", True, ("accr_dq_rai_dt", "rain_self_collection", "evap_dq_rai_dt"), {}, True),
            ("N_lcl", "N_lcl", "N_lcl < eps(FT)", True, ("acnv_dq_rai_dt", "accr_dq_rai_dt"), {}, True),
            ("N_rai", "N_rai", "N_rai < eps(FT)", True, ("rain_self_collection", "rain_breakup", "rain_vel_n"), rain, True),
            # the same ladder, read at the evaporation columns; the fused sums cannot resolve evaporation at N_rai = eps (1e-9 of dq_rai_dt and less)
            ("evap.N_rai", "N_rai", "N_rai <= eps(FT), S < 0", False, ("evap_dN_rai_dt", "evap_dq_rai_dt"), rain, False),
        ]
        for name, var, pred, at_exact, watch, over, fused in sb:
            out.append(Case(f"sb2006.{tag}.process.{name}", "sb_proc", ft, var, eps, _state(SB_STATE, var, **over), pred, True, at_exact, watch, limited))
            if fused:
                f = {"N_lcl": "n_lcl", "N_rai": "n_rai"}
                fst = {f.get(k, k): v for k, v in SB_STATE.items()}
                out.append(Case(f"sb2006.{tag}.fused.{name}", "sb_fused", ft, f.get(var, var), eps, _state(fst, f.get(var, var), **over), pred, True,
                                at_exact, (), limited))
    out.append(Case("bulk2m.ld2004.q_lcl", "bulk2m", ft, "q_lcl", eps, (("N_d", 1e3 if ft == "f32" else 1e-9), ("rho", 1.0)),
                    "q_lcl <= eps(FT)", True, False, ("acnv",)))
    mp = [("q_lcl", ("S_accr_lcl_rai", "S_accr_lcl_sno_cold")), ("q_icl", ("S_accr_icl_rai", "S_accr_icl_sno", "S_accr_freeze_icl_rai")),
          ("q_rai", ("S_accr_lcl_rai", "S_accr_rai_sno_cold", "S_accr_icl_rai")), ("q_sno", ("S_accr_lcl_sno_cold", "S_accr_icl_sno", "S_accr_rai_sno_cold"))]
    for var, watch in mp:
        out.append(Case(f"mp1m.{var}", "mp1m", ft, var, e1, _state(MP1M_STATE, var), f"{var} > cbrt(floatmin(FT))", True, False, watch))
    tst = _state(MP1M_STATE, "T", q_tot=8e-3)
    tf = T_FREEZE_FT[ft]
    out.append(Case("mp1m.T.is_warm.default", "mp1m", ft, "T", tf, tst, "T >= T_freeze", True, True, ("S_accr_lcl_sno_warm", "S_accr_rai_sno_warm")))
    out.append(Case("mp1m.T.deposition_limit.default", "mp1m", ft, "T", tf, tst, "T > T_freeze", False, True, ("S_phase_change_vap_icl",)))
    out.append(Case("mp1m.T.ice_acnv.supersat", "mp1m", ft, "T", tf, tst, "T < T_freeze", False, False, ("S_acnv_icl_sno",), optset="supersat"))
    out.append(Case("mp1m.T.is_warm.tdep", "mp1m", ft, "T", tf, tst, "T >= T_freeze", True, True, ("S_accr_lcl_sno_warm", "S_accr_rai_sno_warm"),
                    optset="tdep"))
    return out


# ---- the reference -------------------------------------------------------------------------------------------------------------------------

def _f64(cols, names):
    return [np.asarray(cols[k], dtype=np.float64) for k in names]


def mp1m_reference_parameters(ft, optset, round_t_freeze=True):
    """(Microphysics1MParams, ThermodynamicsParameters) of the Float64 oracle with T_freeze as the FT kernel holds it"""
    td = P.ParamDict("f64", {"temperature_water_freeze": T_FREEZE_FT[ft]} if round_t_freeze else None)
    return P.Microphysics1MParams(td, **MP1M_OPTIONS[optset]), P.ThermodynamicsParameters(td)


def _sb_fused_oracle(oracle, ft, limited, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, margin):
    flags = (_abi.CMX_SB2006_LIMITED if limited else 0) | _abi.CMX_VEL_SB2006
    return oracle.sb2006_warm_rain_tendencies(_abi.F64, P.WarmRainParams2M("f64", limited).c, P.ThermodynamicsParameters("f64"), P.rain_vel_params("f64"),
                                              flags, rho, T, q_tot, q_lcl, n_lcl, q_rai, n_rai, float32_gates=(ft == "f32"), branch_margin=margin)


def reference(oracle, case, cols=None, **kw):
    """{"out": name → float64 column, "scale": name → operand scale or None, "floor": smallest denominator of the relative bound} (+ "near": inside the
    margin, for a computed gate) of the Float64 oracle at the thresholds of case.ft"""
    cols = case.columns() if cols is None else cols
    ft, f32g = case.ft, case.ft == "f32"
    ref = {"scale": {}, "floor": parity.FLOOR[ft]}
    if case.family in ("sb_proc", "sb_fused"):
        margin = case.margin if case.gate == "breakup" else MARGIN[ft]
        if case.family == "sb_proc":
            q_tot, q_lcl, q_rai, N_lcl, N_rai, rho, T = _f64(cols, COLUMNS["sb_proc"])
            flags = (_abi.CMX_SB2006_LIMITED if case.limited else 0) | _abi.CMX_VEL_SB2006
            ref["out"] = oracle.sb2006_process_rates(_abi.F64, P.WarmRainParams2M("f64", case.limited).c, P.ThermodynamicsParameters("f64"),
                                                     P.rain_vel_params("f64"), flags, q_tot, q_lcl, q_rai, N_lcl, N_rai, rho, T, float32_gates=f32g)
            fused = _sb_fused_oracle(oracle, ft, case.limited, rho, T, q_tot, q_lcl, N_lcl / rho, q_rai, N_rai / rho, margin)
            tau = P.DEFAULT_PARAMETERS["Horn2012_number_concentration_adjustment_timescale"]
            ref["scale"] = {"rain_vel_n": fused["scale"]["vt_rai_n"], "rain_vel_m": fused["scale"]["vt_rai_m"],
                            "numadj_rai": 2 * np.abs(N_rai / rho) / tau, "numadj_lcl": 2 * np.abs(N_lcl / rho) / tau}   # (n_target − n)/τ cancels
        else:
            fused = _sb_fused_oracle(oracle, ft, case.limited, *_f64(cols, COLUMNS["sb_fused"]), margin)
            ref["out"] = {k: fused[k] for k in parity.OUT_NAMES}
            ref["scale"] = dict(fused["scale"])
        if case.gate == "breakup":
            ref["near"] = fused["near_branch"]
        elif case.gate == "evap_number":
            N = np.asarray(cols["N_rai"], dtype=np.float64)
            ref["near"] = np.abs(kw["threshold"] / N - 1) < case.margin          # not limited: x̄_r = ρ q_rai/N_rai, relative in x̄_r
    elif case.family == "bulk2m":
        q_lcl, rho, N_d = _f64(cols, COLUMNS["bulk2m"])
        a, _ = oracle.bulk_2m_cloud_to_rain(_abi.F64, P.Bulk2MSchemes("f64"), _abi.CMX_2M_LD2004, q_lcl, None, rho, N_d, float32_gates=f32g)
        ref["out"] = {"acnv": a}
    elif case.family == "mp1m":
        mp, tps = mp1m_reference_parameters(ft, case.optset, kw.get("round_t_freeze", True))
        r = oracle.mp1m(_abi.F64, mp.c, tps, mp.flags, *_f64(cols, COLUMNS["mp1m"]), float32_gates=f32g)
        ref["out"] = {**{k: r[k] for k in TENDENCIES_1M}, **r["sources"]}
        ref["scale"] = {**r["scale"], **{k: r["scale"][t] for k, t in CANCEL_1M.items()}}
    elif case.family == "susc":
        sb = P.SB2006("f64")
        x = _f64(cols, COLUMNS["susc"])
        au, ac = R.autoconversion(sb.acnv, *x, R.EPS[ft]), R.accretion(sb.accr, *x, R.EPS[ft])
        ref["out"] = {**{"acnv_" + k: v for k, v in au.items()}, **{"accr_" + k: v for k, v in ac.items()}}
        ref["floor"] = 1.0                                                   # that entry's bound: |x − ref| ≤ rtol·max(|ref|, 1)
        ref["near"] = R.near_clip(sb.acnv, x[0], x[2], x[3], case.margin)
    else:
        raise ValueError(case.family)
    ref["out"] = {k: np.asarray(v, dtype=np.float64) for k, v in ref["out"].items()}
    return ref


def oracle_run(oracle, **kw):
    """the reference as a `run` callable (what the mutations of tests/test_gates_host.py hand to the checker)"""
    return lambda case, cols: reference(oracle, case, cols, **kw)["out"]


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------

def _allowed(ref, ft, k, i):
    """the ordinary bound as an absolute error at rung(s) i: RTOL·max(|ref|, floor) + CTOL·scale"""
    r = ref["out"][k][i]
    sc = ref["scale"].get(k)
    return parity.RTOL[ft] * np.maximum(np.abs(r), ref["floor"]) + (parity.CTOL[ft] * np.asarray(sc, dtype=np.float64)[i] if sc is not None else 0.0)


def _ordinary(case, got, ref, k, keep):
    """zero / NaN pattern and the ordinary parity bound of column k at the rungs `keep`; returns the failing rungs"""
    ft = case.ft
    x, r = np.asarray(got[k], dtype=np.float64), ref["out"][k]
    assert x.shape == r.shape, (case.name, k, x.shape, r.shape)
    e = parity.scaled_err(x, r, ref["scale"].get(k), ref["floor"], parity.CEIL[ft], parity.CTOL[ft] / parity.RTOL[ft])
    bad = ~(np.nan_to_num(e, nan=np.inf) <= parity.RTOL[ft])
    bad |= np.isnan(x) != np.isnan(r)
    bad |= (r == 0) & (x != 0)                                              # exactly 0 where the reference is
    if k in case.watch:
        bad |= (r != 0) & (x == 0)                                          # the gated columns: non-zero wherever the reference is
    return np.flatnonzero(bad & keep)


def _fail(case, k, idx, got, ref, note=""):
    i = int(idx[0])
    raise AssertionError(f"{case.name} [{case.ft}] {k}{note}: {idx.size} rung(s) fail, first at offset {i - case.half:+d} ({case.var} = {case.values()[i]!r}): "
                         f"got {np.asarray(got[k])[i]!r}, reference {ref['out'][k][i]!r}")


def exact_side(case, out):
    """'open' / 'closed' / 'mixed': whether the watched columns are non-zero at the threshold itself"""
    nz = [bool(np.asarray(out[k])[case.half] != 0) for k in case.watch]
    return "open" if all(nz) else "closed" if not any(nz) else "mixed"


def check_raw(case, got, ref):
    """all rungs, nothing set aside; returns the side the outputs show at the exact threshold (None without watched columns)"""
    keep = np.ones(case.n, dtype=bool)
    for k in ref["out"]:
        idx = _ordinary(case, got, ref, k, keep)
        if idx.size:
            _fail(case, k, idx, got, ref)
    return exact_side(case, got) if case.watch else None


def _segments(case, ref):
    """(first, last) rung inside the margin, the reference's switch t (first rung on the upper side); the margin must be one run of rungs around t"""
    near = np.asarray(ref["near"], dtype=bool)
    inside = np.flatnonzero(near)
    assert inside.size and np.all(np.diff(inside) == 1), (case.name, "the margin is not one run of rungs")
    m0, m1 = int(inside[0]), int(inside[-1])
    assert m0 >= 1 and m1 <= case.n - 2, (case.name, "the margin reaches the end of the ladder")
    up = upper_side(case, ref["out"], ref)
    t = int(np.argmax(up))
    assert up[t] and not up[:t].any() and up[t:].all() and m0 < t <= m1, (case.name, "the reference does not switch once, inside the margin", t, m0, m1)
    return m0, m1, t


INDICATOR = {"breakup": "rain_breakup", "evap_number": "evap_dN_rai_dt", "clip": "acnv_d_ln_N_lcl"}


def upper_side(case, out, ref):
    """per rung: do the outputs show the branch of the UPPER end of the ladder?  Process columns and susceptibilities carry an indicator column
    (rain_breakup ≠ 0, d ln/d ln N_lcl = 0 once clipped, the evaporation number tendency ≡ 0 above); the fused tendencies are classified by which end's
    reference value dn_rai_dt is nearer to, measured in the distance between the two."""
    if case.family == "sb_fused":
        x, r = np.asarray(out["dn_rai_dt"], dtype=np.float64), ref["out"]["dn_rai_dt"]
        return np.abs(x - r[-1]) < np.abs(x - r[0])
    x = np.asarray(out[INDICATOR[case.gate]], dtype=np.float64)
    if case.gate == "breakup":
        return x != 0
    if case.gate == "clip":
        return x == 0
    return ~np.signbit(x)              # evap_number: min(0, negative) = −tiny or −0 while the gate is open, +0 once x̄_r/x* < eps


def check_computed(case, got, ref):
    """outside the margin: as a raw gate.  Inside: finite and on one of the two branches.  Returns the switch window (None: the side agrees everywhere)."""
    ft = case.ft
    m0, m1, t = _segments(case, ref)
    near = np.asarray(ref["near"], dtype=bool)
    lo, hi = m0 - 1, m1 + 1                                                   # the last rung below the margin, the first above
    for k in ref["out"]:
        idx = _ordinary(case, got, ref, k, ~near)
        if idx.size:
            _fail(case, k, idx, got, ref)
        x, r = np.asarray(got[k], dtype=np.float64), ref["out"][k]
        ins = np.arange(m0, m1 + 1)
        if not np.isfinite(x[ins]).all():
            _fail(case, k, ins[~np.isfinite(x[ins])], got, ref, " (not finite inside the margin)")
        # the change of the reference across the margin on each side, from the two outermost rungs inside the margin on that side
        w_lo, w_hi = abs(r[t - 1] - r[m0]), abs(r[m1] - r[t])
        ok = (np.abs(x[ins] - r[lo]) <= _allowed(ref, ft, k, lo) + w_lo) | (np.abs(x[ins] - r[hi]) <= _allowed(ref, ft, k, hi) + w_hi)
        if not ok.all():
            _fail(case, k, ins[~ok], got, ref, " (on neither branch inside the margin)")
    return switch_window(case, got, ref)


def switch_window(case, got, ref):
    """(first, last) offset from the ladder's centre of the rungs at which the outputs' side differs from the reference's; None if nowhere"""
    if case.gate == "evap_number":
        return None                    # both sides are zero for the float type: there is no side to read off the outputs
    d = np.flatnonzero(upper_side(case, got, ref) != upper_side(case, ref["out"], ref))
    return (int(d[0]) - case.half, int(d[-1]) - case.half) if d.size else None


def check(case, got, ref):
    return check_computed(case, got, ref) if case.computed else check_raw(case, got, ref)


def open_magnitude(case, ref):
    """(smallest |watched column| on the open side, largest on the closed side) over the ladder, on the reference"""
    i = np.arange(case.n) - case.half
    is_open = (i > 0) if case.open_above else (i < 0)
    is_open = is_open | ((i == 0) & case.open_at_exact)
    mags = np.array([np.abs(ref["out"][k]) for k in case.watch])
    return float(mags[:, is_open].min()), float(mags[:, ~is_open].max())


# ---- (b) the computed gates ----------------------------------------------------------------------------------------------------------------

def bisect(is_upper, lo, hi):
    """the smallest double x in (lo, hi] with is_upper(x), for a predicate that is False at lo and True at hi and switches once"""
    assert not is_upper(lo) and is_upper(hi)
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        if is_upper(mid):
            hi = mid
        else:
            lo = mid
    return float(hi)


def _probe(oracle, case_kw, var):
    """x → the reference's side of one point (Float64 oracle, the gates of the case's float type)"""
    def f(x):
        c = Case(center=float(x), half=0, **case_kw)
        cols = {k: np.array([x if k == var else dict(c.state)[k]], dtype=np.float64) for k in COLUMNS[c.family]}
        ref = reference(oracle, c, cols, threshold=float(x))
        return bool(upper_side(c, ref["out"], ref)[0])
    return f


_COMPUTED = {}


def computed_cases(oracle, ft):
    """the computed-gate ladders of one float type, with the threshold bisected on the oracle and (Float64) the stride chosen once per gate; cached"""
    if ft in _COMPUTED:
        return _COMPUTED[ft]
    out = []
    brk = dict(SB_STATE, q_tot=7e-3)                                           # ρ = 1, N_rai = 1e4, T = 285, q_tot = 7e-3, q_lcl = 1e-3, N_lcl = 1e8
    specs = []
    for limited in (True, False):
        tag = "limited" if limited else "notlimited"
        specs.append((dict(name=f"sb2006.{tag}.process.breakup", family="sb_proc", ft=ft, var="q_rai", state=_state(brk, "q_rai"), limited=limited,
                           gate="breakup", margin=MARGIN[ft], predicate="Dr < Dr_th", watch=("rain_breakup",)), 1e-6, 5e-3))
    specs.append((dict(name="sb2006.notlimited.process.evap_number", family="sb_proc", ft=ft, var="N_rai", state=_state(SB_STATE, "N_rai", q_rai=1e-6),
                       limited=False, gate="evap_number", margin=MARGIN[ft], predicate="x_r/x* < eps(FT)", open_above=False),
                  1e-6 / (EPS[ft] * 2.6e-10) / 100, 1e-6 / (EPS[ft] * 2.6e-10) * 100))
    specs.append((dict(name="sb2006.susceptibility.clip", family="susc", ft=ft, var="q_lcl", state=_state(SUSC_STATE, "q_lcl"), gate="clip",
                       margin=CLIP_MARGIN, predicate="x_c < x*", open_above=False), 1e-4, 1e-1))
    for kw, lo, hi in specs:
        thr = bisect(_probe(oracle, kw, kw["var"]), lo, hi)
        case = _with_stride(oracle, Case(center=thr, half=HALF_COMPUTED, **kw), thr)
        out.append((case, thr))
        if kw["gate"] == "breakup":                                            # the same ladder through the fused entry
            f = {"N_lcl": "n_lcl", "N_rai": "n_rai"}
            out.append((dataclasses.replace(case, name=case.name.replace("process", "fused"), family="sb_fused", watch=(),
                                            state=tuple(sorted((f.get(k, k), v) for k, v in case.state))), thr))
    _COMPUTED[ft] = out
    return out


def inside_fraction(oracle, case, thr):
    ref = reference(oracle, case, threshold=thr)
    return float(np.mean(ref["near"]))


def _with_stride(oracle, case, thr):
    """Float32: consecutive floats.  Float64: the smallest power-of-two ulp stride with at most MAX_INSIDE of the ladder inside the margin."""
    if case.ft == "f32":
        return case
    stride = 1
    while inside_fraction(oracle, dataclasses.replace(case, stride=stride), thr) > MAX_INSIDE:
        stride *= 2
        assert stride < 2 ** 40, case.name
    return dataclasses.replace(case, stride=stride)
