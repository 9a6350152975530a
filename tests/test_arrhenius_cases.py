"""CPU tests of rate-constant formation: the reference and the classes of tests/arrhenius_cases.py against mpmath, and
kinetica_jl_amd/csrc/exp_tab.hpp itself through its host replay (tests/native_exp: the header's text under a C++ compiler, the
reciprocal seed as a division). What only the device can show - v_ldexp_f64 into subnormals, v_rcp_f64, the store paths - is
in tests/test_gpu_rate_constants.py.

Measured (largest relative error in units of 2^-53, 2e6 arguments in [-708, 708] plus the index ties): exp_tab_t<512> 1.98,
exp_tab_t<128> 1.86; subnormal results within 0.99 quanta. The class rules on the replay: largest error / bound 0.93 (dense
inputs; 0.77 on the constructed ones). k_ref against mpmath: 2e-19."""
import mpmath
import numpy as np
import pytest

from tests import arrhenius_cases as ac
from tests import exp_host as eh
from tests.arrhenius_cases import LD

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def sweep_args():
    return np.random.default_rng(11).uniform(-708.0, 708.0, 2_000_000)


def test_table_entries_are_correctly_rounded():
    tab = eh.exp2_table()
    with mpmath.workdps(60):
        want = np.array([float(mpmath.power(2, mpmath.mpf(j) / 512)) for j in range(512)])     # mpf -> float rounds to nearest
    assert np.array_equal(tab, want), np.nonzero(tab != want)[0]


@pytest.mark.parametrize("TAB", [512, 128])
def test_exp_tab_normal_results(TAB, sweep_args):
    x = np.concatenate([sweep_args, ac.rint_ties(TAB)])
    ties = ac.rint_ties(TAB)
    assert len(ties) >= 2000 and (ties < 0).any() and (ties > 0).any()
    ref = np.exp(x.astype(LD))
    err = np.abs(eh.exp_tab(x, TAB).astype(LD) - ref) / ref
    worst = float(err.max()) / U53
    print(f"exp_tab_t<{TAB}>: {worst:.3f} x 2^-53 over {len(x)} arguments")
    # 1.25 x the 1.98 measured: entries that were not correctly rounded would add 0.5
    assert worst <= 2.5


@pytest.mark.parametrize("TAB", [512, 128])
def test_exp_tab_subnormal_results_and_exact_points(TAB):
    x = np.random.default_rng(12).uniform(-745.0, -708.4, 200_000)
    ref = np.exp(x.astype(LD))
    got = eh.exp_tab(x, TAB)
    quanta = np.abs(got.astype(LD) - ref) / LD(2) ** -1074
    print(f"exp_tab_t<{TAB}> subnormal: {float(quanta.max()):.3f} quanta")
    assert float(quanta.max()) <= 1.0
    assert (got[x > -744.0] > 0).all()
    assert eh.exp_tab(np.array([0.0, -0.0]), TAB).tolist() == [1.0, 1.0]
    # beyond the ends: 0 and +inf, no NaN (the clamp of the Arrhenius form keeps |x| <= 800)
    assert eh.exp_tab(np.array([-746.0, -800.0, 710.0, 800.0]), TAB).tolist() == [0.0, 0.0, np.inf, np.inf]


def _constructed():
    Ea, A = ac.edge_parameters(64)
    for cap in ac.CAPS:
        for T in ac.T_LIST:
            yield Ea, A, T, cap


def test_reference_against_mpmath():
    """k_ref on every constructed element whose value is a normal long double, against 50 digits: 1e-18 relative."""
    worst, n = 0.0, 0
    Ea, A = ac.edge_parameters(40)
    tiny = np.finfo(LD).tiny
    for cap in ac.CAPS:
        for T in ac.T_LIST:
            ref = ac.k_ref(Ea, A, T, cap[0], cap[1])
            mp = ac.mp_reference(Ea, A, T, cap[0], cap[1])
            for i in range(len(Ea)):
                if mp[i] is None or not np.isfinite(ref[i]) or not ref[i] > tiny:
                    continue
                with mpmath.workdps(50):
                    m, e = np.frexp(ref[i])                                         # the long double, exactly
                    mine = mpmath.ldexp(mpmath.mpf(int(m * LD(2) ** 64)), int(e) - 64)
                    rel = abs(mine / mp[i] - 1) if mpmath.isfinite(mp[i]) and mp[i] != 0 else None
                if rel is None:
                    continue
                worst = max(worst, float(rel)); n += 1
    print(f"k_ref against mpmath: {worst:.2e} over {n} elements")
    assert n > 1000 and worst <= 1e-18


def test_classes_of_the_constructed_inputs():
    """Nothing of the constructed inputs is left out, every class occurs for both forms at R = 64, and at most 1 % of a
    dense draw is left out."""
    for form in ac.FORMS:
        tot = dict.fromkeys(ac.CLASSES, 0)
        for Ea, A, T, cap in _constructed():
            for k, v in ac.class_counts(ac.classify(Ea, A, T, cap[0], cap[1], form)).items():
                tot[k] += v
        print(form, tot)
        assert tot["left_out"] == 0
        assert all(tot[c] > 0 for c in ac.CLASSES if c != "left_out"), tot
    Ea, A = ac.dense_parameters(1025, 5)
    for form in ac.FORMS:
        for cap in ac.CAPS:
            n_out = sum(ac.class_counts(ac.classify(Ea, A, T, cap[0], cap[1], form))["left_out"] for T in ac.dense_temperatures(16, 6))
            assert n_out <= 0.01 * 16 * 1025


@pytest.mark.parametrize("form", ["fast_512", "fast_128", "literal"])
def test_class_rules_on_the_host_replay(form):
    """Every element of the constructed and the dense inputs obeys its class's rule - the |q| > 2.9e6 element (Ea = -6e5 at
    T = 0.02) included: the quotient is clamped at both ends, no conversion leaves the int range."""
    worst = 0.0
    kind = "literal" if form == "literal" else "fast"
    sets = list(_constructed())
    Ea, A = ac.dense_parameters(1025, 5)
    sets += [(Ea, A, T, cap) for cap in ac.CAPS for T in ac.dense_temperatures(8, 7)]
    seen_big_q = False
    for Ea, A, T, cap in sets:
        info = ac.classify(Ea, A, T, cap[0], cap[1], kind)
        dev = eh.arrhenius(Ea, A, T, cap[0], cap[1], form)
        ok, ratio = ac.check(dev, info)
        bad = np.nonzero(~ok)[0]
        assert len(bad) == 0, [(cap, float(T), Ea[i], A[i], ac.CLASSES[info["cls"][i]], dev[i], float(info["ref"][i])) for i in bad[:5]]
        worst = max(worst, ratio.max())
        big = np.abs(info["q"]) > 2.9e6
        big &= np.isfinite(info["q"])
        if big.any():
            seen_big_q = True
            assert np.all(np.isin(info["cls"][big], [ac.CLS["cap_limit"], ac.CLS["zero_limit"], ac.CLS["undefined"], ac.CLS["literal_overflow"]]))
    assert seen_big_q
    print(f"{form}: largest error / bound {worst:.3f}")
    assert worst <= 1.0
