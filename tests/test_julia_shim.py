"""julia/CMXExt.jl — the reference-side binding — checked statically against the reference's struct
definitions (the fixture tests/golden/julia_reference.json) and include/cmx.h by tools/check_julia_shim.py (Julia is not in the image).  The mutation cases prove that the checker
sees the mistakes it is there for, including the one VERDICT r03 found in INTEGRATION.md (`mp.options`, a field that does not exist)."""
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
import check_julia_shim as cjs  # noqa: E402

TEXT = cjs.SHIM.read_text(encoding="utf-8")


def test_shim_agrees_with_header_and_reference():
    findings, summary = cjs.run(verbose=False)
    assert findings == []
    assert summary["mirror_structs"] >= 20 and summary["direct_layout_rows"] >= 35 and summary["ccall_families"] >= 36
    assert summary["c_structs_without_julia_side"] == []
    assert summary["field_accesses"] >= 150 and summary["qualified_names"] >= 100


def test_every_entry_family_is_bound():
    hdr, shim = cjs.Header(), cjs.Shim()
    assert set(hdr.protos) == {c[0] for c in shim.ccalls}
    assert len(hdr.protos) >= 36


def _mutate(old, new, count=1):
    assert TEXT.count(old) >= 1, old
    return TEXT.replace(old, new, count)


MUTATIONS_HEADER_ONLY = [
    # a ccall whose argument type differs from the prototype
    ("(Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Int64, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{Cvoid}),\n        Ref(pack(mp)), Ref(CmxThermo(tps)), option_bits(mp), length(ρ),",
     "(Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int64, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{FT}, Ptr{Cvoid}),\n        Ref(pack(mp)), Ref(CmxThermo(tps)), option_bits(mp), length(ρ),",
     "cmx_mp1m_tendencies: argument types differ"),
    # the round-1 mistake: a 12-field thermo struct
    ("    T_freeze::FT\n    cv_l::FT\nend", "    T_freeze::FT\nend", "CmxThermo == cmx_thermo: field names/order differ"),
    # two fields swapped
    ("    R_v::FT\n    R_d::FT\n", "    R_d::FT\n    R_v::FT\n", "CmxThermo == cmx_thermo: field names/order differ"),
    # wrong flag value
    ("const CMX_1M_SNOW_MELT = UInt32(1) << 11", "const CMX_1M_SNOW_MELT = UInt32(1) << 12", "const CMX_1M_SNOW_MELT"),
    # wrong array length of the quadrature table
    ("    node::NTuple{128, FT}", "    node::NTuple{100, FT}", "CmxQuadrature.node"),
    # an argument dropped from a call
    ("_dp(FT, dn_frz), _dp(FT, dq_frz), stream)", "_dp(FT, dn_frz), stream)", "cmx_liquid_freezing_rate: 10 argument values for 11"),
    # a binding removed
    ('ccall(_fn("cmx_water_activity", FT)', 'ccall(_fn("cmx_water_activity_gone", FT)', "no such entry family"),
    # an unclosed block
    ("    _check(st, \"cmx_deposition_J\")\n    return J\nend", "    _check(st, \"cmx_deposition_J\")\n    return J\n", "lint"),
    # another ABI version
    ("const CMX_VERSION_MINOR = 5", "const CMX_VERSION_MINOR = 3", "CMX_VERSION_MINOR"),
]

MUTATIONS_REFERENCE = [
    # INTEGRATION.md read `mp.options`; the field is `processes` (src/parameters/Microphysics1MParams.jl:84-91)
    ("option_bits(mp::CMP.Microphysics1MParams) = option_bits(mp.processes)", "option_bits(mp::CMP.Microphysics1MParams) = option_bits(mp.options)",
     "CMP.Microphysics1MParams has no field 'options'"),
    # a nested access that hides the member's type from the checker
    ("_tau_relax(wr.condevap)", "wr.condevap.τ_relax", "nested access"),
    # a reference struct claimed to have the C layout although a field is missing on the C side
    ("    (CMP.Koop2000, (), :cmx_koop2000),", "    (CMP.Koop2001, (), :cmx_koop2000),", "the reference defines no struct Koop2001"),
    ("    (CMP.LD2004, (), :cmx_ld2004),", "    (CMP.LD2004, (), :cmx_koop2000),", "DIRECT_LAYOUT CMP.LD2004 => cmx_koop2000: field lists differ"),
    # a process-parameter entry the reference's NamedTuple does not have
    ("_pp_e(pp.rain_snow_accretion, FT),", "_pp_e(pp.rain_snow_collisions, FT),", "process_params has no entry 'rain_snow_collisions'"),
    # a misspelt Greek field
    ("CmxAcnv1M(a.τ, a.q_threshold, a.k)", "CmxAcnv1M(a.tau, a.q_threshold, a.k)", "CMP.Acnv1M has no field 'tau'"),
    # a Thermodynamics accessor that does not exist
    ("TDP.cv_l(tps))", "TDP.cv_liquid(tps))", "TDP.cv_liquid"),
]


@pytest.mark.parametrize("old,new,expect", MUTATIONS_HEADER_ONLY, ids=[m[2][:40] for m in MUTATIONS_HEADER_ONLY])
def test_checker_catches_header_mismatches(old, new, expect):
    findings, _ = cjs.run(verbose=False, shim_text=_mutate(old, new))
    assert any(expect in f for f in findings), findings


@pytest.mark.parametrize("old,new,expect", MUTATIONS_REFERENCE, ids=[m[2][:40] for m in MUTATIONS_REFERENCE])
def test_checker_catches_reference_mismatches(old, new, expect):
    findings, _ = cjs.run(verbose=False, shim_text=_mutate(old, new))
    assert any(expect in f for f in findings), findings


def test_transliteration_matches_every_direct_struct():
    """The header's ASCII spelling of every reference field handed over as it is (νc → nu_c, ρ0 → rho_0, Δa_w_min → delta_a_w_min …)."""
    assert cjs.translit("νc") == "nu_c" and cjs.translit("ρ0") == "rho_0" and cjs.translit("Δa_w_min") == "delta_a_w_min"
    assert cjs.translit("c₁") == "c1" and cjs.translit("Sᵢ_max") == "S_i_max" and cjs.translit("b_ρ") == "b_rho" and cjs.translit("κrr") == "kappa_rr"
    ref = cjs.Reference()
    assert [f for f, _ in ref.structs["Microphysics1MParams"]] == ["processes", "process_params", "cloud", "precip", "air_properties", "terminal_velocity"]
    assert "rain_snow_accretion" in ref.process_param_keys and {"τ_relax", "frostenberg", "e", "coeff_disp", "r_ice_snow"} <= ref.process_param_inner
