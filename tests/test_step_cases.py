"""The references of tests/step_cases.py against the oracle (oracle/bdf.py, SciPy's BDF), on machines without a GPU - a wrong
reference must not pass for a wrong kernel - and the condition on the inputs of every corrector case the GPU file runs: each
quantity the decision tests sits at least 1e-6 (relative) from its threshold, orders above any reduction bound."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.integrate._ivp import bdf as sbdf

from oracle import bdf as obdf
from tests import step_cases as sc

LD = sc.LD


def within(dev, ref, bound, slack=0.0):
    dev = np.asarray(dev, LD)
    return bool(np.all(np.abs(dev - ref) <= bound + slack))


@pytest.mark.parametrize("order", sc.ORDERS)
@pytest.mark.parametrize("factor", sc.FACTORS + (0.3, 3.7))
def test_change_D_is_the_oracles_and_scipys(order, factor):
    rng = np.random.default_rng(order)
    D = sc.signed_decades(rng, (8, 50))
    ref = sc.ref_change_D(D, order, factor)
    Do, Ds = D.copy(), D.copy()
    obdf.change_D(Do, order, factor)
    sbdf.change_D(Ds, order, factor)
    RU, A = sc.ru_matrix(order, factor)
    assert np.all(np.abs(sbdf.compute_R(order, factor).dot(sbdf.compute_R(order, 1)) - RU) <= 1e-14 * A)   # (entries cancel: relative to |R| |U|)
    for got in (Do, Ds):
        for j in range(order + 1):
            # (numpy's matrix product in double, any factor: a few dozen roundings on the same sums of magnitudes)
            assert within(got[j], ref[j][0], 8 * ref[j][1]), (order, factor, j)
        assert np.array_equal(got[order + 1:], D[order + 1:])


def robertson():
    def f(y):
        return np.array([-0.04 * y[0] + 1e4 * y[1] * y[2], 0.04 * y[0] - 1e4 * y[1] * y[2] - 3e7 * y[1] ** 2, 3e7 * y[1] ** 2])

    def jac(y):
        return sp.csr_matrix(np.array([[-0.04, 1e4 * y[2], 1e4 * y[1]], [0.04, -1e4 * y[2] - 6e7 * y[1], -1e4 * y[1]], [0.0, 6e7 * y[1], 0.0]]))
    return f, jac


def test_predictor_accept_and_dense_output_follow_the_oracle():
    """pre-state of every attempt of a stiff solve (captured where the oracle hands it to its corrector) -> the reference
    operations -> the oracle's own predictor, post-state and dense output; every order is reached"""
    f, jac = robertson()
    o = obdf.OracleBDF(f, jac, 3, 1e-10, 1e-8)
    assert o.restart(0.0, [1.0, 0.0, 0.0], 40.0)
    init = sc.ref_init_D(np.array([1.0, 0.0, 0.0]), f(np.array([1.0, 0.0, 0.0])), o.h_abs)
    for j in range(8):
        assert within(o.D[j], *init[j])
    rec = {}
    inner = o._corrector_cached

    def capture(c, y_pred, psi, scale):
        out = inner(c, y_pred, psi, scale)
        rec.update(D=o.D.copy(), order=o.order, y_pred=y_pred.copy(), psi=psi.copy(), scale=scale.copy(), d=out[3].copy(), y_new=out[2].copy())
        return out
    o._corrector_cached = capture
    o.iters_left = 10 ** 6
    seen = set()
    for _ in range(400):
        assert o.step(40.0) == "ok"
        order = rec["order"]
        seen.add(order)
        pred = sc.ref_predict(rec["D"], order, 1e-10, 1e-8)
        for name, got in (("y", rec["y_pred"]), ("psi", rec["psi"]), ("scale", rec["scale"])):
            assert within(got, *pred[sc.ROW[name]]), (name, order)
        acc = sc.ref_accept(rec["D"], rec["d"], order)
        for j in range(order + 3):
            assert within(o.D[j], *acc[j]), (j, order)
        assert within(rec["y_new"], acc[0][0], 4 * acc[0][1])          # the new state is the new D[0]
        for frac in (0.25, 0.5, 1.0):
            ts = o.t - frac * o.h_abs
            ref = sc.ref_interp(o.D, order, ts, o.t, o.h_abs)[sc.ROW["out"]]
            # (times here are not dyadic: the oracle's own weights round like the host's, a few units more)
            assert within(o.interpolate(ts), ref[0], 16 * ref[1]), (order, frac)
        o.select_order()
        if o.t >= 40.0:
            break
    assert seen == {1, 2, 3, 4, 5}, seen


def oracle_newton(updates, crate=1.0, crate_fresh=False, reused=False, n=40, seed=3):
    """OracleBDF._newton driven by prescribed linear-solve results; the same updates through ref_newton_sums / ref_decide"""
    rng = np.random.default_rng(seed)
    y0 = 10.0 ** rng.uniform(-12, 0, n)
    scale = sc.ATOL + sc.RTOL * y0
    z = sc.unit_rms(rng, n)
    dys = [g * z * scale if np.isfinite(g) else np.full(n, g) for g in updates]
    o = obdf.OracleBDF(lambda y: np.zeros(n), None, n, sc.ATOL, sc.RTOL)
    it = iter(dys)
    o._f = lambda y: np.zeros(n)
    o._lusolve = lambda LU, b: next(it)
    o.LU, o.c_fact = None, 1e-3
    o.cur_crate, o.crate_fresh = crate, crate_fresh
    o.slot_is_fresh = not reused
    conv, n_iter, y, d = o._newton(y0.copy(), 1e-3, np.zeros(n), scale)
    # the reference chain
    ctrl = sc.clean_ctrl()
    st = np.zeros((28, n))
    st[sc.ROW["y"]], st[sc.ROW["scale"]] = y0, scale
    entry = dict(order=3, atol=sc.ATOL, rtol=sc.RTOL, upd=1.0, tol=o.newton_tol, rate_max=o.lu_rate_max if reused else 1.0, crate0=crate,
                 tol_first=o.newton_tol if crate_fresh else -1.0, dy_first_max=o.crate_dy_max, maxit=obdf.NEWTON_MAXITER)
    branches = []
    for k, dy in enumerate(dys):
        st[sc.ROW["x"]] = dy
        sums, c, branch, done, margins = sc.newton_reference(st, dict(entry, iter=k), ctrl)
        assert not sc.margins_ok(margins), (updates, k, sc.margins_ok(margins))
        branches.append(branch)
        ctrl = {q: float(v[0]) for q, v in c.items()}
        st[sc.ROW["y"]], st[sc.ROW["d"]] = np.asarray(sums["y"][0], float), np.asarray(sums["d"][0], float)
        if done:
            break
    assert (bool(ctrl["converged"]), int(ctrl["n_iter"])) == (conv, n_iter), (updates, branches, conv, n_iter)
    assert ctrl["crate"] == pytest.approx(o.cur_crate, rel=1e-13), (updates, branches)
    if conv:
        assert np.allclose(st[sc.ROW["y"]], y, rtol=1e-15, atol=0) and np.allclose(st[sc.ROW["d"]], d, rtol=1e-14, atol=1e-300)
    return branches


@pytest.mark.parametrize("kw, branches", [
    (dict(updates=[0.01]), ["converged_first_tol"]),
    (dict(updates=[0.1], crate=0.1, crate_fresh=True), ["converged_carried_rate"]),
    (dict(updates=[0.1, 0.01], crate=1.0, crate_fresh=True), ["refused_crate_estimate_continue", "converged_rate"]),
    (dict(updates=[0.1, 0.01], crate=0.1, crate_fresh=False), ["refused_estimate_continue", "converged_rate"]),
    (dict(updates=[0.25, 0.02], crate=0.05, crate_fresh=True), ["refused_dymax_continue", "converged_rate"]),
    (dict(updates=[0.1, 0.01], crate=0.5, crate_fresh=True), ["refused_estimate_continue", "converged_rate"]),
    (dict(updates=[0.0]), ["zero_update"]),
    (dict(updates=[0.1, 0.02], reused=True), ["refused_crate_estimate_continue", "diverged_rate_max"]),
    (dict(updates=[0.1, 0.012], reused=True, crate=0.5), ["refused_estimate_continue", "converged_rate"]),
    (dict(updates=[0.1, 0.09]), ["refused_crate_estimate_continue", "diverged_estimate"]),
    (dict(updates=[1.0, 0.2, 0.02]), ["refused_crate_dymax_estimate_continue", "continue", "converged_rate"]),
    (dict(updates=[1.0, 0.2, 0.08, 0.004]), ["refused_crate_dymax_estimate_continue", "continue", "continue", "converged_rate"]),
    (dict(updates=[1.0, 0.2, 0.08, 0.04]), ["refused_crate_dymax_estimate_continue", "continue", "continue", "diverged_estimate"]),
    (dict(updates=[np.inf]), ["nonfinite"]),
    (dict(updates=[0.1, np.nan], crate=0.4), ["refused_estimate_continue", "nonfinite"]),
])
def test_decision_function_takes_the_oracles_branches(kw, branches):
    """(the kernel's `exhausted` end - the last allowed iteration neither converged nor diverged - needs an iteration limit of 1:
    with the oracle's limit of 4 the last iteration's two estimates are the same number; the GPU file reaches it with maxit = 1)"""
    assert oracle_newton(**kw) == branches


def test_every_gpu_corrector_case_keeps_its_distance_from_every_threshold():
    names = set()
    for cid, build in sc.newton_case_list():
        st, xloc, entry, ctrl = build()
        sums, c, branch, done, margins = sc.newton_reference(st, entry, ctrl)
        assert not sc.margins_ok(margins), (cid, sc.margins_ok(margins))
        assert sums["neg_margin"] > 1e-6, (cid, sums["neg_margin"])      # no y_new within rounding of a sign change
        name = cid.split("-n")[0]
        if name in sc.DECISION_CASES:
            assert (branch, float(c["spec_go"][0])) == sc.DECISION_CASES[name][3:], (cid, branch, c["spec_go"])
            names.add(branch)
        else:
            assert branch == "converged_first_tol" and float(c["err_norm"][0]) < 1, cid
    # one case per branch of the decision
    assert names >= {"converged_first_tol", "converged_carried_rate", "zero_update", "converged_rate", "diverged_rate_max",
                     "diverged_estimate", "continue", "nonfinite", "behind", "refused_crate_estimate_exhausted",
                     "refused_crate_estimate_continue", "refused_dymax_continue", "refused_estimate_continue"}, names


def test_norms_and_explicit_pair_references():
    """first-step norms against the oracle's expressions (OracleBDF.restart), the Dormand-Prince error norm against SciPy's"""
    rng = np.random.default_rng(5)
    n = 300
    y, f0, f1 = sc.signed_decades(rng, n), sc.signed_decades(rng, n), sc.signed_decades(rng, n)
    r = sc.ref_norms(y, f0, f1, 1e-10, 1e-8)
    scale = 1e-10 + np.abs(y) * 1e-8
    for key, val in (("scratch0", obdf.rms(y / scale)), ("scratch1", obdf.rms(f0 / scale)), ("scratch2", obdf.rms((f1 - f0) / scale)),
                     ("scratch3", float(np.max(np.abs(f0) / (0.1 * np.abs(y) + scale))))):
        assert within(val, r[key][0], 4 * r[key][1]), key
    assert sc.ref_norms(y, f0, None, 1e-10, 1e-8)["scratch2"][0] == 0
    K = sc.signed_decades(rng, (7, n))
    yn = y + K.T.dot(sc.RK_B)
    e = sc.ref_rk_error(y, yn, K, sc.RK_E, 1e-10, 1e-8)
    val = obdf.rms(K.T.dot(sc.RK_E) / (1e-10 + 1e-8 * np.maximum(np.abs(y), np.abs(yn))))
    assert within(val, e["err_norm"][0], 4 * e["err_norm"][1])
    c = sc.ref_rk_combine(y, K, sc.RK_B, 6)[sc.ROW["out"]]
    assert within(yn, c[0], 4 * c[1])
