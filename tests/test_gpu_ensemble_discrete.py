"""GPU tests of kin_solve_ensemble_discrete: K trajectories of one network under discrete rate updates, one stop schedule per
member (reference: a VariableODESolve whose ConditionSet has ts_update, solve_utils.jl:435-509, swept over heating rates).
Resident route: every member bit-identical to a K = 1 kin_solve_ensemble and to kin_solve with its own stops; the new entry
with one schedule for all bit-identical to the shared-stops kin_solve_ensemble on every route; thread route: every member
bit-identical to kin_solve; lockstep route: within the step-sequence tolerance of kin_solve; a known answer and
oracle/bdf.py; failure isolation and argument errors; solving.solve_network_ensemble end to end."""
import ctypes

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import bdf as obdf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

COUNTERS = ("n_steps", "n_rejected", "n_rhs", "n_jac", "n_factor", "n_linsolve", "n_newton_fail", "n_restarts", "n_retries", "n_lu_reused")


def kp(t1, chunk=1e-3, save=None, chunks=True, **kw):
    d = dict(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def units(u, ref, atol=1e-10, rtol=1e-8):
    return float((np.abs(u - ref) / (atol + rtol * np.abs(ref))).max())


STOP_COUNTS = [1, 3, 6, 10, 15, 21, 28, 36, 45, 5, 12, 40]


def _schedules(K, t1, counts=STOP_COUNTS):
    """Member m: a ramp from 900 K at its own rate, sampled at counts[m] stops from 0 to a t_end before t1 (one stop: 1000 K
    held from 0 on); different stop counts and grids."""
    out = []
    for m in range(K):
        n = counts[m % len(counts)]
        if n == 1:
            out.append((np.zeros(1), np.array([1000.0])))
            continue
        tend = t1 * (0.4 + 0.05 * (m % 12))
        ts = np.linspace(0.0, tend, n)
        out.append((ts, 900.0 + (300.0 + 20.0 * m) * ts / tend))
    return out


def _u0(K, n, seed):
    rng = np.random.default_rng(seed)
    U0 = np.zeros((K, n)); U0[:, 0] = 1.0; U0[:, 1:4] = rng.uniform(0.0, 0.1, (K, 3))
    return U0


def test_resident_members_are_their_k1_calls_and_kin_solve():
    n, K, t1 = 300, 12, 2e-3
    net, Ea, A = synthetic_crn(n, 5 * n)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    U0 = _u0(K, n, 3)
    stops = _schedules(K, t1)
    p = kp(t1, save=2.5e-4)
    t, u, ns, rcs, sts = h.solve_ensemble_discrete(p, U0, stops)
    assert (rcs == 0).all() and u.shape == (K, len(t), n) and (ns == len(t)).all() and len(t) == 9
    for m in range(K):
        ts_, Ts_ = stops[m]
        t1_, u1_, ns1, rc1, st1 = h.solve_ensemble(p, U0[m:m + 1], tstops=ts_, T_stops=Ts_)
        assert rc1[0] == 0 and np.array_equal(t1_, t) and np.array_equal(u1_[0], u[m]), m
        for key in ("n_steps", "n_restarts", "n_factor"):
            assert st1[0][key] == sts[m][key], (m, key)
        tk, uk, rck, stk, _ = h.solve(p, U0[m], tstops=ts_, T_stops=Ts_)      # kin_solve: the resident kernel at this size
        assert rck == 0 and np.array_equal(tk, t) and np.array_equal(uk, u[m]) and stk["n_steps"] == sts[m]["n_steps"], m
    # more stops, more restarts (a stop inside a chunk restarts the integration there)
    assert sts[8]["n_restarts"] > sts[1]["n_restarts"] > sts[0]["n_restarts"]
    # the schedules matter: members on different schedules differ
    assert units(u[0], u[1]) > 1e3
    h.close()


def _shared_vs_per_member(h, p, U0, ts, Ts):
    K = len(U0)
    a = h.solve_ensemble_discrete(p, U0, [(ts, Ts)] * K)
    b = h.solve_ensemble(p, U0, tstops=ts, T_stops=Ts)
    assert (a[3] == 0).all() and (b[3] == 0).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert [s["n_steps"] for s in a[4]] == [s["n_steps"] for s in b[4]]
    return a


def test_shared_schedule_is_the_shared_stops_call_on_every_route(monkeypatch):
    # resident, more members than compute units: the build with two workgroups per compute unit (resident_w4.hip)
    net, Ea, A = synthetic_crn(100, 500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    ts, Ts = np.arange(6) * 3e-4, np.linspace(900.0, 1300.0, 6)
    K = 300
    a = _shared_vs_per_member(h, kp(2e-3, save=5e-4), _u0(K, 100, 5), ts, Ts)
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", "0")                       # ... and the one-workgroup build: the same bits
    t0, u0_, _, rcs0, _ = h.solve_ensemble_discrete(kp(2e-3, save=5e-4), _u0(K, 100, 5), [(ts, Ts)] * K)
    monkeypatch.delenv("KIN_RESIDENT_SHARED_CU")
    assert (rcs0 == 0).all() and np.array_equal(u0_, a[1])
    h.close()
    # host threads and lockstep rounds, at a size both take
    net, Ea, A = synthetic_crn(1000, 5000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    U0 = _u0(3, 1000, 6)
    for route in ("threads", "lockstep"):
        monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", route)
        _shared_vs_per_member(h, kp(2e-3, save=5e-4), U0, ts, Ts)
    # lockstep blocks of fewer members (stop_ptr offset with the block): the same members as one block
    stops = _schedules(3, 2e-3, counts=[4, 1, 9])
    tb, ub, _, rcb, _ = h.solve_ensemble_discrete(kp(2e-3), U0, stops)
    monkeypatch.setenv("KIN_ENSEMBLE_MAX_MEMBERS", "2")
    tm, um, _, rcm, _ = h.solve_ensemble_discrete(kp(2e-3), U0, stops)
    assert (rcb == 0).all() and (rcm == 0).all() and np.array_equal(tm, tb) and np.array_equal(um, ub)
    h.close()


def _thread_case(K):
    n, t1 = 2000, 2e-3
    net, Ea, A = synthetic_crn(n, 5 * n)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    U0 = _u0(K, n, 7)
    stops = _schedules(K, t1, counts=[3, 1, 12, 6, 20])
    p = kp(t1)
    t, u, ns, rcs, sts = h.solve_ensemble_discrete(p, U0, stops)
    assert (rcs == 0).all() and (ns == 3).all() and sts[0]["lu_slots"] > 64        # the host-driven integrator's cache
    for m in range(K):
        ts, us, rc, st, _ = h.solve(p, U0[m], tstops=stops[m][0], T_stops=stops[m][1])
        assert rc == 0 and np.array_equal(ts, t) and np.array_equal(us, u[m]), m
        for key in COUNTERS:
            assert st[key] == sts[m][key], (m, key)
    h.close()


def test_large_network_members_are_kin_solve_calls_on_threads():
    _thread_case(3)


def test_threads_take_several_members_each(monkeypatch):
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", "threads")
    monkeypatch.setenv("KIN_ENSEMBLE_THREADS", "2")
    _thread_case(5)


def test_lockstep_members_with_their_own_schedules(monkeypatch):
    """The network of test_lockstep_ensemble_of_a_large_network, forced into lockstep rounds, each member on its own schedule:
    within the step-sequence tolerance of its solo kin_solve (the host-driven integrator) and bit-identical between the batched
    and the per-member dense inverse."""
    monkeypatch.setenv("KIN_ENSEMBLE_BATCHED", "1")
    net, Ea, A = synthetic_crn(10000, 50000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    u0 = np.zeros(10000); u0[0] = 1.0
    stops = _schedules(3, 2e-3, counts=[5, 1, 3])
    U0 = np.tile(u0, (3, 1))
    t, u, ns, rcs, sts = h.solve_ensemble_discrete(kp(2e-3), U0, stops)
    assert (rcs == 0).all() and (ns == 3).all() and sts[0]["lu_dense_dim"] > 900
    for i in range(3):
        ts, us, rc, st, _ = h.solve(kp(2e-3), u0, tstops=stops[i][0], T_stops=stops[i][1])
        assert rc == 0 and np.array_equal(ts, t)
        assert units(u[i], us) < 50
        assert abs(sts[i]["n_steps"] - st["n_steps"]) <= 0.02 * st["n_steps"] + 2
    monkeypatch.setenv("KIN_ENSEMBLE_GJ_BATCHED", "0")
    t1, u1, _, rcs1, sts1 = h.solve_ensemble_discrete(kp(2e-3), U0, stops)
    monkeypatch.delenv("KIN_ENSEMBLE_GJ_BATCHED")
    assert (rcs1 == 0).all() and np.array_equal(u1, u) and [q["n_steps"] for q in sts1] == [q["n_steps"] for q in sts]
    h.close()


def test_a_to_b_step_schedules_against_the_closed_form_and_the_oracle():
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    net = from_lists(2, [[(0, 1)]], [[(1, 1)]])
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A)
    stops = [(np.array([0.0]), np.array([600.0])),
             (np.array([0.0, 0.3, 1.1]), np.array([500.0, 650.0, 550.0])),
             (np.arange(8) * 0.25, np.linspace(500.0, 800.0, 8)),
             (np.array([0.0, 0.05, 0.6, 0.75, 1.5]), np.array([700.0, 520.0, 610.0, 580.0, 640.0]))]
    K = len(stops)
    pd = dict(tspan=(0.0, 2.0), solve_chunkstep=0.5, save_interval=0.25)
    t, u, ns, rcs, _ = h.solve_ensemble_discrete(kp(2.0, chunk=0.5, save=0.25), np.tile([1.0, 0.0], (K, 1)), stops)
    assert (rcs == 0).all() and len(t) == 9
    on = orc.OracleNetwork.from_flat(net)
    for m, (ts, Ts) in enumerate(stops):
        k = np.array([orc.arrhenius(Ea, A, float(T))[0] for T in Ts])
        ends = np.append(ts[1:], np.inf)
        truth = np.array([np.exp(-np.sum(k * np.clip(np.minimum(tt, ends) - ts, 0.0, None))) for tt in t])
        assert units(u[m, :, 0], truth) < 100, m
        assert units(u[m, :, 1], 1.0 - truth) < 100, m
        to, uo, rco, _ = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), 2, pd,
                                                   np.array([1.0, 0.0]), tstops=ts,
                                                   k_of_stop=lambda i, Ts=Ts: orc.arrhenius(Ea, A, float(Ts[i])))
        assert rco == 0 and np.array_equal(to, t) and units(u[m], uo) < 100, m
    h.close()


def test_failure_isolation_and_argument_errors():
    n, t1 = 300, 2e-3
    net, Ea, A = synthetic_crn(n, 5 * n)
    h = capi.HipNetwork.from_flat(net)
    U0 = _u0(3, n, 9)
    stops = _schedules(3, t1, counts=[4, 7, 2])
    p = kp(t1, maxiters=20000)     # (member 1 needs 3 169 steps; a failed member's tolerance retries stay bounded)
    with pytest.raises(capi.KineticaHipError) as e:                         # no Arrhenius parameters
        h.solve_ensemble_discrete(p, U0, stops)
    assert e.value.code == capi.KIN_ERR_STATE
    h.set_arrhenius(Ea, A, k_max=1e12)
    tg, ug, nsg, rcg, _ = h.solve_ensemble_discrete(p, U0, stops)
    assert (rcg == 0).all()
    bad = list(stops)
    bad[1] = (np.array([0.0, 1e-3]), np.array([1000.0, np.nan]))            # member 1's rates turn non-finite at its second stop
    tb, ub, nsb, rcb, _ = h.solve_ensemble_discrete(p, U0, bad)
    assert rcb[1] != 0 and rcb[0] == 0 and rcb[2] == 0 and nsb[1] < len(tg)
    assert np.array_equal(ub[0], ug[0]) and np.array_equal(ub[2], ug[2]) and np.array_equal(tb, tg)
    empty = (np.zeros(0), np.zeros(0))
    decreasing = (np.array([0.0, 1e-3, 5e-4]), np.array([900.0, 1000.0, 950.0]))
    for b in (empty, decreasing):
        for members in ([stops[0], b, stops[2]], [b, stops[1], stops[2]]):
            with pytest.raises(capi.KineticaHipError) as e:
                h.solve_ensemble_discrete(p, U0, members)
            assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:                         # no save grid
        h.solve_ensemble_discrete(kp(t1, chunks=False), U0, stops)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    # null stop_ptr / tstops / T_stops, straight through the C ABI
    rows = ctypes.c_int64(0)
    ptr = np.array([0, 4, 11, 13], np.int64)
    t_all = np.concatenate([s[0] for s in stops]); T_all = np.concatenate([s[1] for s in stops])
    pd = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    args = [pd(U0), ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), pd(t_all), pd(T_all)]
    assert capi.lib().kin_solve_ensemble_discrete(h._h, ctypes.byref(p), 3, *args, ctypes.byref(rows), None, None, None, None, None) == capi.KIN_OK
    assert rows.value == 3
    for i in (1, 2, 3):
        a = list(args); a[i] = None
        assert capi.lib().kin_solve_ensemble_discrete(h._h, ctypes.byref(p), 3, *a, ctypes.byref(rows), None, None, None, None,
                                                      None) == capi.KIN_ERR_INVALID_ARG, i
    h.close()


def test_solve_network_ensemble_end_to_end():
    from kinetica_jl_amd import conditions as C
    from kinetica_jl_amd import solving as S
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    ramps = [(900.0, 1300.0, 2e5), (900.0, 1100.0, 4e5), (1000.0, 1200.0, 1e6)]
    methods = []
    for i, (T0, T1, r) in enumerate(ramps):
        u0 = np.zeros(n); u0[0] = 1.0; u0[i + 1] = 0.1
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        cs = C.ConditionSet({"T": C.LinearGradientProfile(rate=r, X_start=T0, X_end=T1)}, ts_update=1e-4)
        methods.append(S.VariableODESolve(pars, cs, calc))
    res = S.solve_network_ensemble(methods, sd, rd)
    assert len(res) == 3
    assert len({len(o.sol_k) for o in res}) == 3                               # three stop grids of different lengths
    for m, out in zip(methods, res):
        assert out.sol.retcode == "Success" and out.pars is m.pars and out.sol_vcs is None
        solo = S.solve_network(m, sd, rd)
        np.testing.assert_array_equal(solo.sol.t, out.sol.t)
        np.testing.assert_array_equal(solo.sol.u, out.sol.u)
        np.testing.assert_array_equal(solo.sol.umax, out.sol.umax)
        np.testing.assert_array_equal(solo.sol_k.t, out.sol_k.t)
        for s in (0, len(out.sol_k) // 2, len(out.sol_k) - 1):
            np.testing.assert_array_equal(solo.sol_k.u[s], out.sol_k.u[s])
