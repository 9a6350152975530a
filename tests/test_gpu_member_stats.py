"""GPU tests of the cross-member statistics over synthetic blocks (kin_members_moments / _quantiles / _correlate and their device
forms; no solve is needed) against the NumPy restatement of member_stats_cases.py.

Gates, EPS = 2^-53, n the participants (set by the feature's definition or derived in member_stats_cases.py, not measured):
  count, min, max   exact
  mean              |got - ref| <= (n + 8) EPS sum |x| / n                          (delta below)
  variance          (2 n + 16) EPS S / (n - 1) + n delta^2 / (n - 1), S the exact sum of squared deviations; exactly 0.0 for n = 1
  quantiles         bit for bit the restated rule, zeros compared by value
  correlations      CORR_C (n + 16) EPS (1 + sqrt(n) (|xbar| / sqrt(Sxx) + |ybar| / sqrt(Syy))) with CORR_C = 4 (derivation:
                    member_stats_cases.py); exactly 0.0 without spread or for n < 2. The value (Pearson) cases leave the subnormal
                    column out - squares of subnormal deviations underflow, the header says so - and every other finite
                    column's gate is asserted to stay below 1e-9, so centring is not what they test.
A column holding a NaN is NaN in every statistic; the +Inf column's mean, maximum and p = 1 quantile are +Inf."""
import ctypes
import itertools

import numpy as np
import pytest

import member_stats_cases as mc
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
EPS = mc.EPS
P = np.array([0.0, 0.05, 0.25, 0.5, 0.77, 0.95, 1.0])
KS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
SHAPES = [(N, L, K) for N in (5, 70) for L in (1, 3) for K in KS]

_handles = {}


def handle(N):
    if N not in _handles:
        _handles[N] = capi.HipNetwork(*mc.chain_network(N))
    return _handles[N]


def spearman_species(N):
    return None if N == 5 else [0, 1, 2, 3, 4, 63, 64, 65, 69]


def pearson_species(N):
    return [s for s in (spearman_species(N) or range(5)) if s != mc.SP_SUBNORMAL]


@pytest.mark.parametrize("N,L,K", SHAPES)
def test_moments(N, L, K):
    h, u = handle(N), mc.block(K, L, N)
    for label, use in mc.masks(K):
        got, ref = h.members_moments(u, use=use), mc.ref_moments(u, use)
        n = ref["count"]
        assert got["count"] == n, label
        assert mc.same_bits_or_zero(got["min"], ref["min"]) and mc.same_bits_or_zero(got["max"], ref["max"]), label
        if n == 0:
            assert all(np.all(got[q] == 0.0) for q in ("mean", "var", "min", "max"))
            continue
        fin = np.isfinite(ref["abs_mean"])
        delta = (n + 8) * EPS * ref["abs_mean"][fin]
        err = np.abs(got["mean"][fin] - ref["mean"][fin])
        assert np.all(err <= delta), (label, float(np.max(err / np.maximum(delta, 1e-300))))
        if n == 1:
            assert np.all(got["var"][fin] == 0.0)
        else:
            vb = (2 * n + 16) * EPS * ref["S"][fin] / (n - 1) + n * delta ** 2 / (n - 1)
            verr = np.abs(got["var"][fin] - ref["var"][fin])
            assert np.all(verr <= vb), (label, float(np.max(verr / np.maximum(vb, 1e-300))))
        # the non-finite columns: NaN everywhere / an infinite mean and maximum, no variance
        nan = np.isnan(ref["abs_mean"])
        assert nan[0, mc.SP_NAN] and all(np.all(np.isnan(got[q][nan])) for q in ("mean", "var", "min", "max")), label
        inf = np.isinf(ref["abs_mean"])
        assert inf[L - 1, mc.SP_INF] and np.all(got["mean"][inf] == np.inf) and np.all(got["max"][inf] == np.inf), label
        assert np.all(np.isnan(got["var"][inf])) and np.all(np.isfinite(got["min"][inf]) | (n == 1)), label


@pytest.mark.parametrize("N,L,K", SHAPES)
def test_quantiles(N, L, K):
    h, u = handle(N), mc.block(K, L, N)
    for (label, use), species in itertools.product(mc.masks(K), [None] if N == 5 else [None, spearman_species(N)]):
        got, ref = h.members_quantiles(u, P, species=species, use=use), mc.ref_quantiles(u, P, species, use)
        assert mc.same_bits_or_zero(got, ref), (label, species, mc.mismatches(got, ref))
        if label != "none" and species is None:
            assert np.all(np.isnan(got[:, 0, mc.SP_NAN])) and got[-1, L - 1, mc.SP_INF] == np.inf


def check_correlation(got, ref, bound, small=None):
    ruled = np.isinf(bound)                                  # 0.0 or NaN by rule: compared exactly
    assert mc.same_bits_or_zero(got[ruled], ref[ruled])
    err = np.abs(got[~ruled] - ref[~ruled])
    assert np.all(np.isfinite(got[~ruled])) and np.all(err <= bound[~ruled]), float(np.max(err / bound[~ruled], initial=0.0))
    if small is not None:
        assert np.all(bound[~ruled] < small)
    return int((~ruled).sum())


@pytest.mark.parametrize("N,L,K", SHAPES)
def test_correlations(N, L, K):
    h, u, X = handle(N), mc.block(K, L, N), mc.inputs(K)
    gated = 0
    for label, use in mc.masks(K):
        sp = spearman_species(N)
        gated += check_correlation(h.members_correlate(u, X, species=sp, rank=True, use=use), *mc.ref_correlate(u, X, sp, True, use))
        sp = pearson_species(N)
        gated += check_correlation(h.members_correlate(u, X, species=sp, rank=False, use=use), *mc.ref_correlate(u, X, sp, False, use),
                                   small=1e-9)
    assert gated > 0 or K < 3      # (two participants with a tie or a zero pair may leave nothing to gate)


def everything(h, u, X, use=None):
    m = h.members_moments(u, use=use)
    return [np.float64(m["count"]), m["mean"], m["var"], m["min"], m["max"], h.members_quantiles(u, P, use=use),
            h.members_quantiles(u, P, species=[4, 2, 0], use=use), h.members_correlate(u, X, rank=True, use=use),
            h.members_correlate(u, X, rank=False, use=use), h.members_correlate(u, X, species=[4, 3], rank=True, use=use)]


@pytest.mark.parametrize("K", [65, 257])
def test_blocking_and_repeats_change_no_bit(K, monkeypatch):
    N, L = 70, 3
    h, u, X = handle(N), mc.block(K, L, N), mc.inputs(K)
    use = np.ones(K, np.int32); use[1::5] = 0
    base = everything(h, u, X, use)
    runs = [everything(h, u, X, use)]
    for cols in ("1", "7"):
        monkeypatch.setenv("KIN_MEMBERS_BLOCK_COLUMNS", cols)
        runs.append(everything(h, u, X, use))
    monkeypatch.delenv("KIN_MEMBERS_BLOCK_COLUMNS")
    for run in runs:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(base, run))


def test_device_entries_equal_the_host_entries():
    import torch
    N, L, K = 70, 3, 257
    h, u, X = handle(N), mc.block(K, L, N), mc.inputs(K)
    use = np.ones(K, np.int32); use[::3] = 0
    sp = [4, 63, 2, 0]
    d_u = torch.tensor(u, dtype=torch.float64, device="cuda:0")
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda:0")
    d_m = [new(L, N) for _ in range(4)]
    d_q, d_qs, d_r, d_p = new(len(P), L, N), new(len(P), L, len(sp)), new(L, len(sp), 4), new(L, N, 4)
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    n = h.members_moments_dev(K, L, d_u.data_ptr(), use=use, d_mean=d_m[0].data_ptr(), d_var=d_m[1].data_ptr(), d_min=d_m[2].data_ptr(),
                              d_max=d_m[3].data_ptr())
    h.members_quantiles_dev(K, L, d_u.data_ptr(), P, d_q.data_ptr(), use=use)
    h.members_quantiles_dev(K, L, d_u.data_ptr(), P, d_qs.data_ptr(), species=sp, use=use)
    h.members_correlate_dev(K, L, d_u.data_ptr(), X, d_r.data_ptr(), species=sp, rank=True, use=use)
    h.members_correlate_dev(K, L, d_u.data_ptr(), X, d_p.data_ptr(), rank=False, use=use)
    torch.cuda.synchronize()
    m = h.members_moments(u, use=use)
    assert n == m["count"] == int(use.sum())
    for d, q in zip(d_m, ("mean", "var", "min", "max")):
        assert d.cpu().numpy().tobytes() == m[q].tobytes(), q
    assert d_q.cpu().numpy().tobytes() == h.members_quantiles(u, P, use=use).tobytes()
    assert d_qs.cpu().numpy().tobytes() == h.members_quantiles(u, P, species=sp, use=use).tobytes()
    assert d_r.cpu().numpy().tobytes() == h.members_correlate(u, X, species=sp, rank=True, use=use).tobytes()
    assert d_p.cpu().numpy().tobytes() == h.members_correlate(u, X, rank=False, use=use).tobytes()
    # only one output wanted: the others are left alone
    d_only = new(L, N)
    torch.cuda.synchronize()
    h.members_moments_dev(K, L, d_u.data_ptr(), use=use, d_var=d_only.data_ptr())
    torch.cuda.synchronize()
    assert d_only.cpu().numpy().tobytes() == m["var"].tobytes()


def test_the_participant_limit_of_the_sorted_passes():
    """KIN_MEMBERS_MAX_SORTED participants sort (the largest LDS image); one more is KIN_ERR_UNSUPPORTED with the limit in the
    message, while the moments and the value correlation take any K."""
    N, L, K = 5, 1, capi.MEMBERS_MAX_SORTED + 1
    h, u, X = handle(N), mc.block(K, L, N), mc.inputs(K)
    use = np.ones(K, np.int32); use[17] = 0
    assert mc.same_bits_or_zero(h.members_quantiles(u, P, use=use), mc.ref_quantiles(u, P, None, use))
    check_correlation(h.members_correlate(u, X, rank=True, use=use), *mc.ref_correlate(u, X, None, True, use))
    for call in (lambda: h.members_quantiles(u, P), lambda: h.members_correlate(u, X, rank=True)):
        with pytest.raises(capi.KineticaHipError) as e:
            call()
        assert e.value.code == capi.KIN_ERR_UNSUPPORTED and str(capi.MEMBERS_MAX_SORTED) in str(e.value)
    got, ref = h.members_moments(u), mc.ref_moments(u)
    assert got["count"] == K and mc.same_bits_or_zero(got["max"], ref["max"])
    sp = pearson_species(N)
    check_correlation(h.members_correlate(u, X, species=sp, rank=False), *mc.ref_correlate(u, X, sp, False, None), small=1e-9)


def test_status_codes():
    N, L, K = 5, 3, 3
    h, u, X = handle(N), mc.block(K, L, N), mc.inputs(K)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    for bad in ([-0.1], [0.5, 1.0000001], [np.nan]):
        assert code(lambda: h.members_quantiles(u, bad)) == capi.KIN_ERR_INVALID_ARG
    for bad in ([5], [-1], [0, 7]):
        assert code(lambda: h.members_quantiles(u, [0.5], species=bad)) == capi.KIN_ERR_INVALID_ARG
        assert code(lambda: h.members_correlate(u, X, species=bad)) == capi.KIN_ERR_INVALID_ARG
    one = capi.HipNetwork(*mc.chain_network(N, index_base=1), index_base=1)      # species ids are in the base the handle was created with
    assert code(lambda: one.members_quantiles(u, [0.5], species=[0])) == capi.KIN_ERR_INVALID_ARG
    assert mc.same_bits_or_zero(one.members_quantiles(u, [0.5], species=[5, 1]), mc.ref_quantiles(u, [0.5], [4, 0]))
    one.close()
    L_ = capi.lib()
    PD, pd = ctypes.POINTER(ctypes.c_double), lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    uc, p, Xc, cnt = np.ascontiguousarray(u), np.array([0.5]), np.ascontiguousarray(X), ctypes.c_int64(0)
    null = PD()
    assert L_.kin_members_moments(h.handle, K, L, pd(uc), None, None, null, null, null, null) == capi.KIN_ERR_INVALID_ARG
    assert L_.kin_members_quantiles(h.handle, K, L, pd(uc), None, None, 0, pd(p), 1, null) == capi.KIN_ERR_INVALID_ARG
    assert L_.kin_members_correlate(h.handle, K, L, pd(uc), None, None, 0, pd(Xc), 4, 1, null) == capi.KIN_ERR_INVALID_ARG
    assert L_.kin_members_moments(h.handle, -1, L, pd(uc), None, ctypes.byref(cnt), null, null, null, null) == capi.KIN_ERR_INVALID_ARG
    assert L_.kin_members_quantiles(h.handle, K, L, pd(uc), None, None, 0, pd(p), -1, pd(np.empty(L * N))) == capi.KIN_ERR_INVALID_ARG
    # no stored ensemble
    out = np.empty((L, N, 4))
    assert L_.kin_ensemble_moments(h.handle, None, ctypes.byref(cnt), pd(out), null, null, null) == capi.KIN_ERR_STATE
    assert L_.kin_ensemble_quantiles(h.handle, None, None, 0, pd(p), 1, pd(out)) == capi.KIN_ERR_STATE
    assert L_.kin_ensemble_correlate(h.handle, None, None, 0, pd(Xc), 4, 1, pd(out)) == capi.KIN_ERR_STATE
    # count alone is an output; an empty selection is an empty result
    assert L_.kin_members_moments(h.handle, K, L, pd(uc), None, ctypes.byref(cnt), null, null, null, null) == capi.KIN_OK and cnt.value == K
    assert h.members_quantiles(u, [0.5], species=[]).shape == (1, L, 0)
