"""Float64 NumPy restatement of src/Nucleation.jl (the reference's aerosol nucleation rates) and of CMI_het.P3_deposition_N_i / P3_het_N_i
(src/IceNucleation.jl:162-166, 202-205) — the yardstick of tests/test_nucleation_host.py and tests/test_nucleation_gpu.py.

Semantics: NumPy's power is IEEE pow, as Julia's ^ (0^p = 0, 1^y = 1 for every y, x^0 = 1); x/0 = ±Inf; log(0) = −Inf.  Where Julia throws
DomainError — a negative base of a non-integer power, log of a negative number — the result is NaN (the library's convention).  P3_het_N_i is the
library's −N_l·expm1(x) form (include/cmx.h); `p3_het_N_i_reference_form` is the reference's N_l (1 − exp(x)).
"""
import numpy as np


def _f(p, name):
    return float(getattr(p, name))


def _a(x):
    return np.asarray(x, dtype=np.float64)


def h2so4_nucleation_rate(h2so4_conc, nh3_conc, negative_ion_conc, temp, p):
    """Nucleation.jl:51-90 → (binary_rate, ternary_rate)"""
    h2so4_conc, nh3_conc, ion, temp = map(_a, (h2so4_conc, nh3_conc, negative_ion_conc, temp))
    with np.errstate(all="ignore"):
        h = h2so4_conc * 1e-6                       # :60-61 — negative_ion is not converted
        a = nh3_conc * 1e-6
        ref = 1e6

        def k(u, v, w):
            return np.exp(_f(p, u) - np.exp(_f(p, v) * (temp / 1000 - _f(p, w))))

        def f_y(pt, pA, ay):
            # (h/ref)^p_t / (a/ref)^p_A formed as one power of the ratio of logarithms (IEEE: 0/0 → NaN, x/0 → Inf, 0/x → 0), as the library does:
            # the reference's literal form underflows its denominator to 0 at tiny nh3 (0/0 = NaN at h2so4 = 0, Inf where the ratio is finite)
            ratio = np.exp(_f(p, pt) * np.log(h / ref) - _f(p, pA) * np.log(a / ref))
            return (a / ref) / (_f(p, ay) + ratio)
        k_b_n, k_b_i = k("u_b_n", "v_b_n", "w_b_n"), k("u_b_i", "v_b_i", "w_b_i")
        k_t_n, k_t_i = k("u_t_n", "v_t_n", "w_t_n"), k("u_t_i", "v_t_i", "w_t_i")
        f_n, f_i = f_y("p_t_n", "p_A_n", "a_n"), f_y("p_t_i", "p_A_i", "a_i")
        binary = k_b_n * (h / ref) ** _f(p, "p_b_n") + k_b_i * (h / ref) ** _f(p, "p_b_i") * ion
        ternary = k_t_n * f_n * (h / ref) ** _f(p, "p_t_n") + k_t_i * f_i * (h / ref) ** _f(p, "p_t_i") * ion
        # h2so4 < 0 or nh3 < 0 (−Inf included: Julia's ^ throws for every negative base of a non-integer power, NumPy's pow(−Inf, y) is +Inf):
        # the powers throw before either rate is formed
        bad = (a < 0) | (h < 0)
        binary = np.where(bad, np.nan, binary)
        ternary = np.where(bad, np.nan, ternary)
    return binary * 1e6, ternary * 1e6


def organic_nucleation_rate_hom_prescribed(negative_ion_conc, HOM_conc, p):
    """Nucleation.jl:137-157"""
    ion, hom = _a(negative_ion_conc), _a(HOM_conc)
    with np.errstate(all="ignore"):
        x = hom / 1e7
        x = np.where(x < 0, np.nan, x)                      # DomainError of the non-integer power (−Inf included)
        rate = (_f(p, "a_1") * x ** (_f(p, "a_2") + _f(p, "a_5") / x)
                + _f(p, "a_3") * x ** (_f(p, "a_4") + _f(p, "a_5") / x) * ion)
    return rate * 1e6


def hom_concentration(monoterpene_conc, O3_conc, OH_conc, temp, condensation_sink, p):
    """The HOM concentration [cm⁻³] organic_nucleation_rate forms (Nucleation.jl:115-129)."""
    mt, o3, oh, temp, cs = map(_a, (monoterpene_conc, O3_conc, OH_conc, temp, condensation_sink))
    with np.errstate(all="ignore"):
        mt, o3, oh = mt * 1e-6, o3 * 1e-6, oh * 1e-6
        k_MTO3 = _f(p, "k_MTO3") * np.exp(_f(p, "exp_MTO3") / temp)
        k_MTOH = _f(p, "k_MTOH") * np.exp(_f(p, "exp_MTOH") / temp)
        return (_f(p, "Y_MTO3") * k_MTO3 * mt * o3 + _f(p, "Y_MTOH") * k_MTOH * mt * oh) / cs


def organic_nucleation_rate(negative_ion_conc, monoterpene_conc, O3_conc, OH_conc, temp, condensation_sink, p):
    """Nucleation.jl:106-135: all four concentrations ×1e-6 (:117-120)"""
    hom = hom_concentration(monoterpene_conc, O3_conc, OH_conc, temp, condensation_sink, p)
    return organic_nucleation_rate_hom_prescribed(_a(negative_ion_conc) * 1e-6, hom, p)


def organic_and_h2so4_nucleation_rate_bioOxOrg_prescribed(h2so4_conc, bioOxOrg, p):
    """Nucleation.jl:192-206 (h2so4 NOT converted: :202 is commented out)"""
    h, bio = _a(h2so4_conc), _a(bioOxOrg)
    with np.errstate(all="ignore"):
        k = 1e-6 * _f(p, "k_H2SO4org")
        bio = bio * 1e-6
        return 0.5 * k * h ** 2 * bio * 1e6


def bio_ox_org(monoterpene_conc, OH_conc, temp, condensation_sink, p):
    """The bioOxOrg [m⁻³] organic_and_h2so4_nucleation_rate forms (Nucleation.jl:180-184)."""
    mt, oh, temp, cs = map(_a, (monoterpene_conc, OH_conc, temp, condensation_sink))
    with np.errstate(all="ignore"):
        k = _f(p, "k_MTOH") * np.exp(_f(p, "exp_MTOH") / temp)
        return k * mt * oh / cs * 1e6


def organic_and_h2so4_nucleation_rate(h2so4_conc, monoterpene_conc, OH_conc, temp, condensation_sink, p):
    """Nucleation.jl:172-190 composed with :192-206.  The unit factors cancel pairwise (bioOxOrg ×1e6 then ×1e-6, k_H2SO4org ×1e-6 and the result
    ×1e6) and are cancelled here, as in the library: identical in real arithmetic, without the overflow of the ×1e6 intermediate at extreme inputs."""
    mt, oh, temp, cs, h = map(_a, (monoterpene_conc, OH_conc, temp, condensation_sink, h2so4_conc))
    with np.errstate(all="ignore"):
        k = _f(p, "k_MTOH") * np.exp(_f(p, "exp_MTOH") / temp)
        return 0.5 * _f(p, "k_H2SO4org") * h ** 2 * (k * mt * oh / cs)


def apparent_nucleation_rate(output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam=1.7):
    """Nucleation.jl:23-37 (log of a negative ratio: DomainError → NaN)"""
    od, nr, gr, cs, csi, id_ = map(_a, (output_diam, nucleation_rate, condensation_growth_rate, coag_sink, coag_sink_input_diam, input_diam))
    with np.errstate(all="ignore"):
        m = np.log(cs / csi) / np.log(od / id_)
        g = 1 / (m + 1) * ((od / id_) ** (m + 1) - 1)
        # the same γ without the cancellation at m → −1 (the library's form, include/cmx.h): where both are finite they agree to the rounding of
        # the reference's form, so the well-conditioned value is the yardstick
        r = od / id_
        with_expm1 = np.expm1((m + 1) * np.log(r)) / (m + 1)
        g = np.where(np.isfinite(with_expm1) & np.isfinite(g) & (r != 1), with_expm1, g)
        return nr * np.exp(-g * id_ * csi / gr)


def p3_deposition_N_i(ip, T, nan_rule=True):
    """IceNucleation.jl:162-166.  nan_rule: a NaN T gives NaN (the library); False: the reference's ifelse returns 0 there."""
    T = _a(T)
    with np.errstate(all="ignore"):
        Tp = np.maximum(_f(ip, "T_dep_thres"), T)            # Julia's max propagates NaN
        N = 1000 * _f(ip, "c1") * np.exp(_f(ip, "c2") * (_f(ip, "T0") - Tp))
        out = np.where(T < _f(ip, "T0"), N, 0.0)
    return np.where(np.isnan(T), np.nan, out) if nan_rule else out


def _het_x(ip, T, N_l, V_l, dt):
    return -_f(ip, "het_B") * _a(V_l) * _a(dt) * np.exp(_f(ip, "het_a") * (_f(ip, "T0") - _a(T)))


def p3_het_N_i(ip, T, N_l, V_l, dt):
    """IceNucleation.jl:202-205 in the library's form −N_l·expm1(x) (no cancellation for |x| ≪ 1)"""
    with np.errstate(all="ignore"):
        return -_a(N_l) * np.expm1(_het_x(ip, T, N_l, V_l, dt))


def p3_het_N_i_reference_form(ip, T, N_l, V_l, dt, dtype=np.float64):
    """the reference's own arithmetic N_l (1 − exp(x)) in `dtype`"""
    with np.errstate(all="ignore"):
        x = _het_x(ip, T, N_l, V_l, dt).astype(dtype)
        return _a(N_l).astype(dtype) * (dtype(1) - np.exp(x))
