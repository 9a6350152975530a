"""GPU tests of the statistics across a stored ensemble: kin_ensemble_moments / _quantiles / _correlate read the members' saved
states where the last kin_solve_ensemble* call left them, and solving.solve_network_ensemble(statistics=...).

A Monte-Carlo run over uncertain rate constants: synthetic_crn(300, 1500) on the resident route, 64 members at 1000 K, 21 saved
rows, every member with its own k = k0 exp(0.3 z), z standard normal, on the 8 reactions with the largest time-integrated flux
of the unperturbed solve; the inputs of the correlation are the z.
  stored ensemble (no trajectory downloaded) against the host entries over a second call's download: bit for bit
  Spearman coefficients against scipy.stats.spearmanr on the download, five species, every row and input: 1e-12
  the inputs matter: some |r| > 0.5 at the last row"""
import warnings

import numpy as np
import pytest
import scipy.stats

import member_stats_cases as mc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn
from test_gpu_ensemble_analysis import kp

pytestmark = pytest.mark.gpu
QS = (0.05, 0.5, 0.95)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_monte_carlo_over_rate_constants():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    k0 = h.rates_at(1000.0)
    u0 = np.zeros(300); u0[0] = 1.0
    p = kp(2e-3, save=1e-4)
    h.set_rates(k0)
    t, us, rc, _, _ = h.solve(p, u0)
    assert rc == 0 and len(t) == 21
    top = np.argsort(-np.abs(h.solution_flux(w=S.flux_weights(t))))[:8]
    K = 64
    z = np.random.default_rng(21).standard_normal((K, 8))
    k = np.tile(k0, (K, 1))
    k[:, top] *= np.exp(0.3 * z)
    U0 = np.tile(u0, (K, 1))
    sel = [0, 7, 150, 299, 42]

    def stored():
        return dict(m=h.ensemble_moments(), q=h.ensemble_quantiles(QS), qs=h.ensemble_quantiles(QS, species=sel),
                    rs=h.ensemble_correlate(z, rank=True), rp=h.ensemble_correlate(z, species=sel, rank=False))

    t0, none, ns0, rcs0, _ = h.solve_ensemble(p, U0, k=k, trajectories=False)
    assert none is None and np.all(rcs0 == 0) and np.all(ns0 == 21)
    a = stored()
    t1, u, ns, rcs, _ = h.solve_ensemble(p, U0, k=k, trajectories=True)
    assert u.shape == (K, 21, 300) and np.array_equal(ns, ns0)
    b = stored()
    host = dict(m=h.members_moments(u), q=h.members_quantiles(u, QS), qs=h.members_quantiles(u, QS, species=sel),
                rs=h.members_correlate(u, z, rank=True), rp=h.members_correlate(u, z, species=sel, rank=False))
    for got in (a, b):
        assert got["m"]["count"] == host["m"]["count"] == K
        for q in ("mean", "var", "min", "max"):
            assert _same(got["m"][q], host["m"][q]), q
        for q in ("q", "qs", "rs", "rp"):
            assert _same(got[q], host[q]), q
    assert np.array_equal(a["m"]["max"], u.max(axis=0)) and np.array_equal(a["m"]["min"], u.min(axis=0))
    assert np.all(a["q"][0] <= a["q"][1]) and np.all(a["q"][1] <= a["q"][2])
    # Spearman against SciPy on the download: the five species that vary most at the last row
    five = np.argsort(-a["m"]["var"][-1])[:5]
    worst = 0.0
    for j in range(21):
        for i in five:
            for c in range(8):
                with np.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ref = scipy.stats.spearmanr(z[:, c], u[:, j, i]).statistic
                got = a["rs"][j, i, c]
                if np.isnan(ref):                            # a constant column (the start row): 0.0 by rule
                    assert got == 0.0 and u[:, j, i].min() == u[:, j, i].max()
                else:
                    worst = max(worst, abs(got - ref))
    strongest = float(np.abs(a["rs"][-1]).max())
    print(f"Spearman against SciPy: max deviation {worst:.2e}; strongest |r| at the last row {strongest:.3f}")
    assert worst <= 1e-12
    assert strongest > 0.5                                   # the inputs matter
    assert np.all(np.abs(a["rs"]) <= 1.0 + 1e-12) and np.all(np.isfinite(a["rs"])) and np.all(np.isfinite(a["rp"]))
    # the high-level call on the same handle
    st = S.ensemble_statistics(h, t1, quantiles=QS, species=sel, inputs=z, rank=True)
    assert st.count == K and _same(st.mean, host["m"]["mean"]) and _same(st.quantiles, host["qs"]) and _same(st.corr, host["rs"][:, sel])
    assert st.p.tolist() == list(QS) and st.species.tolist() == sel and st.rank is True and np.array_equal(st.t, t1)
    h.close()


def test_a_member_that_fails_early_takes_no_part():
    """The recipe of test_gpu_ensemble_analysis.py: member 1's rate constants are absurd and its step budget ends it early."""
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    T = np.array([900.0, 1000.0, 1100.0, 1200.0])
    kbad = np.array([h.rates_at(float(Ti)) for Ti in T]); kbad[1] *= 1e40
    p = kp(2e-3, save=1e-4, maxiters=3000)
    t, u, ns, rcs, _ = h.solve_ensemble(p, np.tile(u0, (4, 1)), k=kbad, trajectories=True)
    assert rcs[1] != 0 and ns[1] < 21 and all(ns[m] == 21 for m in (0, 2, 3))
    m = h.ensemble_moments()
    assert m["count"] == 3
    up = u.copy(); up[1] = np.nan                            # never read: the host entry over the download with the same mask
    ref = h.members_moments(up, use=[1, 0, 1, 1])
    for q in ("mean", "var", "min", "max"):
        assert m[q].tobytes() == ref[q].tobytes() and np.all(np.isfinite(m[q]))
    assert h.ensemble_quantiles(QS).tobytes() == h.members_quantiles(up, QS, use=[1, 0, 1, 1]).tobytes()
    X = T[:, None]
    assert h.ensemble_correlate(X).tobytes() == h.members_correlate(up, X, use=[1, 0, 1, 1]).tobytes()
    assert h.ensemble_moments(use=[1, 0, 0, 1])["count"] == 2
    for call in (lambda: h.ensemble_moments(use=[1, 1, 1, 1]), lambda: h.ensemble_quantiles(QS, use=[0, 1, 0, 0]),
                 lambda: h.ensemble_correlate(X, use=[1, 1, 0, 0])):
        with pytest.raises(capi.KineticaHipError) as e:
            call()
        assert e.value.code == capi.KIN_ERR_INVALID_ARG
    h.close()


def test_solve_network_ensemble_statistics_over_heating_rates():
    from kinetica_jl_amd import conditions as C
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    rates = [1e5, 2e5, 3e5, 4e5]
    methods = []
    for r in rates:
        u0 = np.zeros(n); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=r, X_start=900.0, X_end=1300.0)}), calc))
    plain = S.solve_network_ensemble(methods, sd, rd)
    assert all(o.sol.ensemble_stats is None for o in plain)      # the default: the call as it always was
    sel = [0, 5, 17]
    lean = S.solve_network_ensemble(methods, sd, rd, trajectories=False,
                                    statistics=dict(species=sel, inputs=np.log(rates)[:, None], rank=True))
    st = lean[0].sol.ensemble_stats
    assert isinstance(st, S.EnsembleStatistics) and all(o.sol.ensemble_stats is st for o in lean)
    assert all(o.sol.u is None and o.sol.retcode == "Success" for o in lean)
    rows = len(lean[0].sol.t)
    assert st.count == 4 and np.array_equal(st.t, lean[0].sol.t) and st.mean.shape == (rows, n)
    assert np.all(st.min <= st.mean) and np.all(st.mean <= st.max) and np.all(st.var >= 0.0)
    assert st.quantiles.shape == (3, rows, 3) and st.corr.shape == (rows, 3, 1) and st.species.tolist() == sel and st.rank is True
    # against the downloaded trajectories of the plain call
    u = np.stack([o.sol.u for o in plain])
    assert np.array_equal(st.max, u.max(axis=0)) and np.array_equal(st.min, u.min(axis=0))
    assert mc.same_bits_or_zero(st.quantiles, mc.ref_quantiles(u, QS, sel)), mc.mismatches(st.quantiles, mc.ref_quantiles(u, QS, sel))
    full = S.solve_network_ensemble(methods, sd, rd, statistics=True)
    assert full[0].sol.ensemble_stats.quantiles.shape == (3, rows, n) and full[0].sol.ensemble_stats.corr is None
    np.testing.assert_array_equal(full[0].sol.u, plain[0].sol.u)
