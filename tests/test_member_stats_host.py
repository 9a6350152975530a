"""CPU tests of the cross-member statistics' host side: the restated rules of member_stats_cases.py against NumPy / SciPy,
kin_members_inputs_host against the restatement, solve_network_ensemble's argument checks and the EnsembleStatistics container.
No device is touched."""
import math
import warnings

import numpy as np
import pytest
import scipy.stats

import member_stats_cases as mc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S


def _ulp_distance(a, b, scale):
    return np.abs(a - b) / np.spacing(scale)


def test_quantile_rule_against_numpy_linear():
    """numpy.quantile(method="linear") interpolates by a lerp that switches its form at g >= 0.5; the header's rule is the one
    form x[lo] + (x[lo+1] - x[lo]) g. Bit-equal in most cases, within 4 ulp of max(|x[lo]|, |x[lo+1]|) in all (the two forms
    round a difference, a product and a sum each: measured at most 2.0 ulp over 32 000 such samples)."""
    rng = np.random.default_rng(3)
    equal = total = 0
    worst = 0.0
    for trial in range(400):
        n = int(rng.integers(1, 60))
        x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)
        x[rng.random(n) < 0.3] = 0.0
        xs = np.sort(x)
        for p in np.concatenate([[0.0, 1.0, 0.5], rng.random(5)]):
            got, ref = mc.quantile_rule(xs, p), np.quantile(x, p, method="linear")
            h = (n - 1) * p
            lo = int(np.floor(h))
            scale = max(abs(xs[lo]), abs(xs[min(lo + 1, n - 1)]), 1e-300)
            worst = max(worst, float(_ulp_distance(got, ref, scale)))
            equal += got == ref
            total += 1
    print(f"{equal} of {total} bit-equal, worst {worst:.2f} ulp")
    assert worst <= 4.0 and equal > total // 2


def test_quantile_rule_edges():
    xs = np.array([1.0, 2.0, 4.0, np.inf])
    assert mc.quantile_rule(xs, 0.0) == 1.0 and mc.quantile_rule(xs, 1.0) == np.inf and mc.quantile_rule(xs, 1 / 3) == 2.0
    assert mc.quantile_rule(xs, 0.5) == 3.0 and mc.quantile_rule(xs, 0.9) == np.inf
    assert mc.quantile_rule(np.array([7.0]), 0.3) == 7.0
    u = np.zeros((3, 1, 2)); u[:, 0, 0] = [3.0, np.nan, 1.0]; u[:, 0, 1] = [3.0, -0.0, 1.0]
    q = mc.ref_quantiles(u, [0.0, 0.5, 1.0])
    assert np.all(np.isnan(q[:, 0, 0])) and q[:, 0, 1].tolist() == [0.0, 1.0, 3.0]
    assert mc.ref_quantiles(u, [0.5], use=[1, 0, 1])[0, 0].tolist() == [2.0, 2.0]      # the NaN's member takes no part
    assert np.all(mc.ref_quantiles(u, [0.5], use=[0, 0, 0]) == 0.0)


def test_restated_spearman_against_scipy_with_heavy_ties():
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 200):
        for _ in range(20):
            x = rng.integers(0, 4, n).astype(float)
            y = np.where(rng.random(n) < 0.4, 0.0, rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15, 15, n))
            y[rng.random(n) < 0.1] = -0.0                    # ties with +0.0
            r, _ = mc.pearson_exact(mc.ranks(x), mc.ranks(y))
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")              # (SciPy warns about a constant side)
                ref = scipy.stats.spearmanr(x, y).statistic
            if np.isnan(ref):                                # SciPy: a constant side is undefined; here it is 0.0 by rule
                assert r == 0.0 and (x.min() == x.max() or y.min() == y.max())
            else:
                assert abs(r - ref) <= 1e-14


def test_ranks_are_average_tie_and_exact():
    assert mc.ranks(np.array([0.0, -0.0, 5.0, -1.0, 5.0, 5.0])).tolist() == [2.5, 2.5, 5.0, 1.0, 5.0, 5.0]


@pytest.mark.parametrize("rank", [True, False])
def test_inputs_host_against_the_restatement(rank):
    rng = np.random.default_rng(9)
    for K in (1, 2, 3, 64, 257, 1000):
        X = np.stack([rng.standard_normal(K), 1e6 + rng.standard_normal(K), rng.integers(0, 3, K).astype(float), np.full(K, 0.1),
                      np.exp(3 * rng.standard_normal(K))], axis=1)
        for label, use in mc.masks(K) + [("odd", (np.arange(K) % 2).astype(np.int32))]:
            n, got = capi.members_inputs(X, use=use, rank=rank)
            n_ref, ref = mc.ref_inputs(X, use, rank)
            assert n == n_ref == len(mc.participants(K, use)) and got.shape == (n, X.shape[1])
            if n < 2:
                assert np.all(got == 0.0)
                continue
            assert np.all(got[:, 3] == 0.0)                  # no spread, whatever 0.1 n / n rounds to
            # within 4 ulp (of the entry, and never coarser than an ulp of the column's largest entry times 2^-10)
            tol = 4 * np.maximum(np.spacing(np.abs(ref)), np.spacing(np.abs(ref).max(axis=0)) * 2.0 ** -10)
            assert np.all(np.abs(got - ref) <= tol), (K, label, float(np.max(np.abs(got - ref) / tol)))
            x = X[mc.participants(K, use)]
            spread = x.min(axis=0) != x.max(axis=0)
            assert np.all(got[:, ~spread] == 0.0)
            # unit norm (8 ulp from entries within 4 ulp, exact sums) and zero sum (entries within 4 ulp of ones that sum to 0)
            assert all(abs(math.fsum(c * c) - 1.0) <= 1e-14 for c in got.T[spread])
            assert all(abs(math.fsum(c)) <= 8 * n * 2.0 ** -52 for c in got.T)
            if rank:
                r = mc.ranks(x)                              # multiples of 0.5: the ranks themselves are exact
                assert np.all(r * 2 == np.round(r * 2)) and np.all(r.sum(axis=0) == n * (n + 1) / 2)
                # ... and so are the entry's: scaled back by the exact root and mean, they round to the restated ranks
                d = r - (n + 1) / 2
                back = got * np.sqrt((d * d).sum(axis=0)) + (n + 1) / 2
                assert np.all((np.round(2 * back) / 2 == r)[:, spread]) and np.all(np.abs(back - r)[:, spread] <= 1e-9 * n)


def test_inputs_host_nan_and_arguments():
    X = np.array([[1.0, np.nan], [2.0, 3.0], [4.0, 5.0]])
    n, got = capi.members_inputs(X, rank=True)
    assert n == 3 and np.all(np.isnan(got[:, 1])) and np.all(np.abs(got[:, 0] - mc.normalised([1.0, 2.0, 3.0])) <= 4 * np.spacing(1.0))
    n, got = capi.members_inputs(X, use=[0, 1, 1], rank=False)
    assert n == 2 and np.allclose(got, [[-np.sqrt(0.5)] * 2, [np.sqrt(0.5)] * 2], rtol=0, atol=2e-16)
    with pytest.raises(ValueError):
        capi.members_inputs(X, use=[1, 1])
    with pytest.raises(ValueError):
        capi.members_inputs(np.zeros(3))
    import ctypes
    n64 = ctypes.c_int64(0)
    assert capi.lib().kin_members_inputs_host(-1, 2, None, None, 1, ctypes.byref(n64), None) == capi.KIN_ERR_INVALID_ARG
    assert capi.lib().kin_members_inputs_host(2, 2, None, None, 1, None, None) == capi.KIN_ERR_INVALID_ARG
    assert capi.lib().kin_members_inputs_host(5, 2, None, None, 1, ctypes.byref(n64), None) == capi.KIN_OK and n64.value == 5


def _methods(n_members=2):
    from kinetica_jl_amd import conditions as C
    from kinetica_jl_amd.synth import synthetic_crn
    n = 20
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    methods = []
    for i in range(n_members):
        u0 = np.zeros(n); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, 1e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        cs = C.ConditionSet({"T": C.LinearGradientProfile(rate=1e5 * (i + 1), X_start=900.0, X_end=1000.0)})
        methods.append(S.VariableODESolve(pars, cs, calc))
    return methods, sd, rd


@pytest.mark.parametrize("bad", [
    "yes", 3, ["quantiles"], dict(quantile=(0.5,)), dict(quantiles=(0.5, 1.5)), dict(quantiles=(-0.1,)), dict(quantiles="median"),
    dict(quantiles=(np.nan,)), dict(species=[0.5]), dict(species=[-1]), dict(species=[[0, 1]]), dict(species=[20]),
    dict(inputs=[1.0, 2.0]), dict(inputs=np.zeros((3, 2))), dict(inputs=[["a", "b"], ["c", "d"]]), dict(use=[1]), dict(use=[1, 0, 1]),
])
def test_malformed_statistics_raise_before_the_gpu(bad):
    methods, sd, rd = _methods()
    if capi.device_count() == 0:
        # nothing may reach the device: without one, anything else than ValueError would be KIN_ERR_DEVICE
        with pytest.raises(ValueError, match="statistics"):
            S.solve_network_ensemble(methods, sd, rd, statistics=bad)
    else:
        with pytest.raises(ValueError, match="statistics"):
            S.solve_network_ensemble(methods, sd, rd, statistics=bad)


def test_statistics_arguments_defaults():
    kw = S._statistics_arguments(True, 4)
    assert kw["quantiles"].tolist() == [0.05, 0.5, 0.95] and kw["species"] is None and kw["inputs"] is None and kw["rank"] is True
    assert S._statistics_arguments(None, 4) is None
    kw = S._statistics_arguments(dict(quantiles=None, species=(3, 1), inputs=np.ones((4, 2)), rank=0), 4)
    assert kw["quantiles"].tolist() == [] and kw["species"].tolist() == [3, 1] and kw["inputs"].shape == (4, 2) and kw["rank"] is False


def test_ensemble_statistics_container():
    import dataclasses
    assert [f.name for f in dataclasses.fields(S.EnsembleStatistics)] == ["t", "count", "mean", "var", "min", "max", "quantiles", "p",
                                                                           "species", "corr", "rank"]
    t = np.linspace(0.0, 1.0, 3)
    z = np.arange(6.0).reshape(3, 2)
    q = np.stack([z - 1, z, z + 1])
    st = S.EnsembleStatistics(t, 5, z, z * z, z - 2, z + 2, quantiles=q, p=np.array([0.05, 0.5, 0.95]))
    assert st.corr is None and st.species is None and st.rank is True and st.count == 5
    assert np.array_equal(st.std, z)
    lo, hi = st.envelope()
    assert np.array_equal(lo, z - 1) and np.array_equal(hi, z + 1)
    with pytest.raises(ValueError):
        st.envelope(0.1, 0.9)
    assert "ensemble_stats" in [f.name for f in dataclasses.fields(S.ODESolution)]
    assert S.ODESolution(t, None, "Success").ensemble_stats is None
    assert "ensemble_statistics" in S.__all__ and "EnsembleStatistics" in S.__all__


def test_hipnetwork_has_the_entries():
    for name in ("members_moments", "members_quantiles", "members_correlate", "ensemble_moments", "ensemble_quantiles",
                 "ensemble_correlate", "members_moments_dev", "members_quantiles_dev", "members_correlate_dev"):
        assert callable(getattr(capi.HipNetwork, name))
    assert capi.MEMBERS_MAX_SORTED == 4096
    text = open(capi.LIB_PATH.replace("kinetica_jl_amd/libkinetica_hip.so", "include/kinetica_hip.h")).read() \
        if capi.LIB_PATH.endswith("kinetica_jl_amd/libkinetica_hip.so") else None
    if text is not None:
        assert f"#define KIN_MEMBERS_MAX_SORTED {capi.MEMBERS_MAX_SORTED}" in text
