"""GPU tests of the stored ensemble's analysis: kin_ensemble_size / _max / _dot / _flux read the members' saved states where
the last kin_solve_ensemble* call left them on the device - on the resident, thread and lockstep routes, with and without a
downloaded trajectory - and solving.solve_network_ensemble(fluxes=..., trajectories=...).

References: a second call that downloads u. Bounds (EPS = 2^-53; derived, not measured):
  maxima   exact (np.array_equal with np.max over the member's own saved rows) where those rows are finite
  dot      |got - u_j . w| <= (N + 8) EPS sum_i |w_i u_i|
  flux     against kin_flux_batched over the member's downloaded rows with the same weights and rate constants, two finite sums
           of the same terms: 2 (L + 8) EPS sum_j |w_j rate_j|, L the rows of the save grid; and bit for bit against the
           segmented pass's host entry over the downloaded states."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def kp(t1, chunk=1e-3, save=None, chunks=True, **kw):
    d = dict(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def _analysis(h, src, wdot):
    K, rows, n, ns = h.ensemble_size()
    return dict(K=K, rows=rows, n=n, ns=ns, umax=h.ensemble_max(), dot=h.ensemble_dot(wdot), flux=h.ensemble_flux(**src))


def _same(a, b):
    assert (a["K"], a["rows"], a["n"]) == (b["K"], b["rows"], b["n"]) and np.array_equal(a["ns"], b["ns"])
    for q in ("umax", "dot", "flux"):
        assert np.array_equal(a[q], b[q], equal_nan=True), q


def check_stored_ensemble(h, solve, sources, expect_failed=()):
    """solve(trajectories) runs the ensemble call; sources(t, ns) gives kin_ensemble_flux's arguments. Analyses the call that
    downloads nothing, then the call that downloads u, compares the two and checks the second against its u."""
    n = h.n
    wdot = np.random.default_rng(11).uniform(0.5, 2.0, n)
    t0, u_none, ns0, rcs0, _ = solve(False)
    assert u_none is None
    a0 = _analysis(h, sources(t0, ns0), wdot)
    t, u, ns, rcs, _ = solve(True)
    src = sources(t, ns)
    a = _analysis(h, src, wdot)
    assert np.array_equal(t0, t) and np.array_equal(ns0, ns) and np.array_equal(rcs0, rcs)
    _same(a0, a)                                             # out_u == NULL changes nothing
    K, rows = u.shape[:2]
    assert (a["K"], a["rows"], a["n"]) == (K, rows, n) and np.array_equal(a["ns"], ns)
    for m in expect_failed:
        assert rcs[m] != 0 and ns[m] < rows, (m, rcs, ns)
    assert all(rcs[m] == 0 and ns[m] == rows for m in range(K) if m not in expect_failed)
    # bit for bit the segmented pass's host entry over the downloaded states (the rows past n_saved hold zeros there: poisoned)
    up = u.copy()
    for m in range(K):
        up[m, ns[m]:] = np.nan
    host = h.flux_segmented(up, seg_n=ns, **{("T" if q == "T_rows" else q): v for q, v in src.items()})
    assert np.array_equal(host, a["flux"], equal_nan=True)
    w = src["w"]
    for m in range(K):
        nm = int(ns[m])
        um = u[m, :nm]
        assert np.all(u[m, nm:] == 0.0) and np.all(a["dot"][m, nm:] == 0.0)
        if nm == 0:
            assert np.all(a["umax"][m] == 0.0) and np.all(a["flux"][m] == 0.0)
            continue
        if not np.isfinite(um).all():
            continue                                         # (a blown-up member: covered by the bit-for-bit comparison above)
        assert np.array_equal(a["umax"][m], um.max(axis=0)), m
        dref = um @ wdot
        dbound = (n + 8) * EPS * (np.abs(um) @ np.abs(wdot)) + 1e-300
        assert np.all(np.abs(a["dot"][m, :nm] - dref) <= dbound), m
        one = {}
        if "T_rows" in src:
            one["T"] = src["T_rows"][m, :nm]
        elif "k_row" in src:
            one["k"], one["k_row"] = src["k"], src["k_row"][m, :nm]
        fb, rates = h.flux_batched(um, w=w[m, :nm], want_rates=True, **one)
        fbound = 2 * (rows + 8) * EPS * (np.abs(w[m, :nm, None] * rates)).sum(axis=0) + 1e-300
        err = np.abs(a["flux"][m] - fb)
        print(f"member {m}: n_saved {nm}, flux max err/bound {np.max(err / fbound):.3f}, finite {np.isfinite(fb).all()}")
        assert np.all(err <= fbound), m
        if nm > 1:
            assert np.any(a["flux"][m] != 0.0)
    return a, t, u, ns, rcs


def test_resident_route_static_temperatures():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    T = np.array([900.0, 1000.0, 1100.0, 1200.0])
    p = kp(2e-3, save=1e-4)
    a, t, u, ns, rcs = check_stored_ensemble(
        h, lambda tr: h.solve_ensemble(p, np.tile(u0, (4, 1)), T=T, trajectories=tr),
        lambda t, ns: S.ensemble_flux_sources("static", t, ns, T=T))
    assert len(t) == 21 and a["rows"] == 21
    assert not np.array_equal(a["flux"][0], a["flux"][3])            # the temperatures matter
    h.close()


def test_resident_route_with_a_member_that_fails_early():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    T = np.array([900.0, 1000.0, 1100.0, 1200.0])
    kbad = np.array([h.rates_at(float(Ti)) for Ti in T]); kbad[1] *= 1e40
    p = kp(2e-3, save=1e-4, maxiters=3000)

    def sources(t, ns):
        src = S.ensemble_flux_sources("static", t, ns)              # k_row = m into the members' own k
        src["k"] = kbad
        return src

    a, t, u, ns, rcs = check_stored_ensemble(h, lambda tr: h.solve_ensemble(p, np.tile(u0, (4, 1)), k=kbad, trajectories=tr),
                                             sources, expect_failed=(1,))
    # the failed member's maximum is over its own rows only: where one of them stays below zero the zero rows behind would win
    n1 = int(ns[1])
    if n1 and np.isfinite(u[1, :n1]).all():
        assert np.array_equal(a["umax"][1], u[1, :n1].max(axis=0))
    h.close()


@pytest.mark.parametrize("route", ["threads", "lockstep"])
def test_thread_and_lockstep_routes(route, monkeypatch):
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", route)
    net, Ea, A = synthetic_crn(1000, 5000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    rng = np.random.default_rng(6)
    U0 = np.zeros((3, 1000)); U0[:, 0] = 1.0; U0[:, 1:4] = rng.uniform(0.0, 0.1, (3, 3))
    ts, Ts = np.arange(6) * 3e-4, np.linspace(900.0, 1300.0, 6)
    p = kp(2e-3, save=5e-4)
    a, t, u, ns, rcs = check_stored_ensemble(
        h, lambda tr: h.solve_ensemble(p, U0, tstops=ts, T_stops=Ts, trajectories=tr),
        lambda t, ns: S.ensemble_flux_sources("discrete", t, ns, tstops=ts, T_stops=Ts))
    assert a["rows"] == 5
    if route == "lockstep":
        # blocks of fewer members reuse the solver's buffer: the members' rows are then kept in the handle's own copy
        monkeypatch.setenv("KIN_ENSEMBLE_MAX_MEMBERS", "2")
        t2, u2, ns2, rcs2, _ = h.solve_ensemble(p, U0, tstops=ts, T_stops=Ts, trajectories=False)
        b = _analysis(h, S.ensemble_flux_sources("discrete", t2, ns2, tstops=ts, T_stops=Ts), np.random.default_rng(11).uniform(0.5, 2.0, 1000))
        _same(a, b)
    h.close()


def _methods(discrete):
    from kinetica_jl_amd import conditions as C
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    ramps = [(900.0, 1300.0, 2e5), (900.0, 1100.0, 4e5), (1000.0, 1200.0, 1e6)] if discrete else \
        [(900.0, 1300.0, 2e5), (1000.0, 1200.0, 1e5), (1300.0, 1000.0, -3e5)]
    methods = []
    for i, (T0, T1, r) in enumerate(ramps):
        u0 = np.zeros(n); u0[0] = 1.0; u0[i + 1] = 0.1
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        cs = C.ConditionSet({"T": C.LinearGradientProfile(rate=r, X_start=T0, X_end=T1)}, **(dict(ts_update=1e-4) if discrete else {}))
        methods.append(S.VariableODESolve(pars, cs, calc))
    return methods, sd, rd, calc


@pytest.mark.parametrize("discrete", [False, True], ids=["continuous", "discrete_members"])
def test_solve_network_ensemble_fluxes_and_no_trajectories(discrete):
    methods, sd, rd, calc = _methods(discrete)
    plain = S.solve_network_ensemble(methods, sd, rd)
    assert all(o.sol.fluxes is None for o in plain)                  # the defaults: what the function did before
    res = S.solve_network_ensemble(methods, sd, rd, fluxes=True)
    lean = S.solve_network_ensemble(methods, sd, rd, fluxes=True, trajectories=False)
    for o0, o, ol in zip(plain, res, lean):
        assert o.sol.retcode == "Success"
        np.testing.assert_array_equal(o0.sol.u, o.sol.u)
        np.testing.assert_array_equal(o0.sol.umax, o.sol.umax)
        rows = len(o.sol.t)
        ref = S.reaction_fluxes(o, calc, rates=True)
        bound = 2 * (rows + 8) * EPS * np.abs(ref.weights[:, None] * ref.rates).sum(axis=0) + 1e-300
        fl = o.sol.fluxes
        assert isinstance(fl, S.ReactionFluxes) and fl.rates is None
        print(f"max err/bound {np.max(np.abs(fl.flux - ref.flux) / bound):.3f}")
        assert np.all(np.abs(fl.flux - ref.flux) <= bound)
        assert np.array_equal(fl.weights, ref.weights)
        assert np.array_equal(fl.top(5), ref.top(5))
        assert np.any(fl.flux != 0.0)
        # no trajectory downloaded: the times, the device's maxima and the same fluxes
        assert ol.sol.u is None and ol.sol.retcode == "Success"
        np.testing.assert_array_equal(ol.sol.t, o.sol.t)
        np.testing.assert_array_equal(ol.sol.umax, o.sol.u.max(axis=0))
        np.testing.assert_array_equal(ol.sol.fluxes.flux, fl.flux)


def test_lifetime_of_the_record():
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(300); u0[0] = 1.0
    wdot = np.ones(300)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    for fn in (h.ensemble_size, h.ensemble_max, lambda: h.ensemble_dot(wdot), h.ensemble_flux):
        assert code(fn) == capi.KIN_ERR_STATE                        # before any ensemble call
    h.rates_at(1000.0)
    ts_, us_, rc, _, _ = h.solve(kp(2e-3), u0)                       # a single solve stores no ensemble
    assert rc == 0 and code(h.ensemble_size) == capi.KIN_ERR_STATE
    p = kp(2e-3, save=2.5e-4)
    T4 = np.array([900.0, 1000.0, 1100.0, 1200.0])
    t, u4, ns4, rcs4, _ = h.solve_ensemble(p, np.tile(u0, (4, 1)), T=T4)
    src4 = S.ensemble_flux_sources("static", t, ns4, T=T4)
    a4 = _analysis(h, src4, wdot)
    assert a4["K"] == 4 and a4["rows"] == 9
    # a kin_solve in between: the stored ensemble gives the same answers, or KIN_ERR_STATE - nothing else
    ts_, us_, rc, _, _ = h.solve(kp(2e-3, save=1e-4), u0)
    assert rc == 0 and len(ts_) == 21
    try:
        _same(a4, _analysis(h, src4, wdot))
    except capi.KineticaHipError as e:
        assert e.code == capi.KIN_ERR_STATE
    # a second ensemble call of another K (and another grid): sizes and results are the second call's
    T2 = np.array([950.0, 1150.0])
    p2 = kp(2e-3, save=5e-4)
    t2, u2, ns2, rcs2, _ = h.solve_ensemble(p2, np.tile(u0, (2, 1)), T=T2)
    a2 = _analysis(h, S.ensemble_flux_sources("static", t2, ns2, T=T2), wdot)
    assert a2["K"] == 2 and a2["rows"] == 5 and a2["umax"].shape == (2, 300) and a2["flux"].shape == (2, 1500)
    for m in range(2):
        assert np.array_equal(a2["umax"][m], u2[m].max(axis=0))
    # a failed ensemble call (bad arguments) leaves the earlier record or none: never a wrong one
    with pytest.raises(capi.KineticaHipError):
        h.solve_ensemble(kp(2e-3, chunks=False), np.tile(u0, (3, 1)), T=T4[:3])       # no save grid
    try:
        assert h.ensemble_size()[0] == 2
    except capi.KineticaHipError as e:
        assert e.code == capi.KIN_ERR_STATE
    h.close()
