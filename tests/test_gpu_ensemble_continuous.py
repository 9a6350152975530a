"""GPU tests of kin_solve_ensemble_continuous: K trajectories of one network under continuous rate updates, one temperature
profile per member (reference: a VariableODESolve without ts_update, methods.jl:363-653). Resident route (one workgroup per
member, rate_mode 3 of resident_core.hpp): every member bit-identical to a K = 1 call, within the step-sequence tolerance of
kin_solve_continuous and within the solver tolerance of oracle/bdf.py; thread route (larger networks): every member
bit-identical to kin_solve_continuous; argument errors; solving.solve_network_ensemble end to end."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import bdf as obdf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def kp(t1, chunk=1e-3, save=None, chunks=True, **kw):
    d = dict(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def units(u, ref, atol=1e-10, rtol=1e-8):
    return float((np.abs(u - ref) / (atol + rtol * np.abs(ref))).max())


def _profiles(K, t1):
    """Ramps over 900 - 1300 K: different rates, start temperatures and node counts (some profiles end before t1, some hold)."""
    out = []
    for m in range(K):
        T0 = 900.0 + 25.0 * (m % 5)
        T1 = 1300.0 - 30.0 * (m % 4) if m % 3 else 950.0 + 20.0 * m
        n = 2 + (m % 4) * 3
        tend = t1 * (1.0 if m % 2 else 0.75)
        tn = np.linspace(0.0, tend, n)
        out.append((tn, T0 + (T1 - T0) * tn / tend))
    return out


def _oracle(net, Ea, A, pars, u0, tn, Tn):
    on = orc.OracleNetwork.from_flat(net)
    return obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), net.n_species, pars, u0,
                                     k_of_time=lambda tg: orc.arrhenius(Ea, A, float(np.interp(tg, tn, Tn)), k_max=1e12))


def test_resident_members_are_their_k1_calls_and_agree_with_the_references():
    n, K, t1 = 300, 12, 2e-3
    net, Ea, A = synthetic_crn(n, 5 * n)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    rng = np.random.default_rng(3)
    U0 = np.zeros((K, n)); U0[:, 0] = 1.0; U0[:, 1] = rng.uniform(0.0, 0.5, K)
    nodes = _profiles(K, t1)
    p = kp(t1, save=2.5e-4)
    t, u, ns, rcs, sts = h.solve_ensemble_continuous(p, U0, nodes)
    assert (rcs == 0).all() and u.shape == (K, len(t), n)
    # save grid and rows as kin_solve_ensemble's
    ts_, us_, ns_, rcs_, _ = h.solve_ensemble(p, U0[:2], T=np.array([1000.0, 1100.0]))
    np.testing.assert_array_equal(t, ts_)
    assert (ns == len(t)).all() and (ns_ == len(t)).all()
    for m in range(K):
        t1_, u1_, ns1, rc1, st1 = h.solve_ensemble_continuous(p, U0[m:m + 1], [nodes[m]])
        assert rc1[0] == 0 and np.array_equal(t1_, t) and np.array_equal(u1_[0], u[m]), m
        assert st1[0]["n_steps"] == sts[m]["n_steps"] and st1[0]["n_factor"] == sts[m]["n_factor"]
    # the rates move with T(t): members on different profiles differ
    assert units(u[0], u[1]) > 1e3
    for m in (1, 6):
        tn, Tn = nodes[m]
        ts, us, rc, st, _ = h.solve_continuous(p, U0[m], tn, Tn)
        assert rc == 0 and np.array_equal(ts, t)
        assert units(u[m], us) <= 201, m                 # step-sequence tolerance
        to, uo, rco, sto = _oracle(net, Ea, A, dict(tspan=(0.0, t1), save_interval=2.5e-4), U0[m], tn, Tn)
        assert rco == 0 and np.array_equal(to, t) and units(u[m], uo) <= 100, m
    # a member whose profile turns non-finite fails; the others keep their bits (a shared maxiters, as kbad in
    # test_few_members_of_a_large_network_are_kin_solve_calls_on_threads)
    pm = kp(t1, save=2.5e-4, maxiters=3000)
    tg, ug, nsg, rcg, _ = h.solve_ensemble_continuous(pm, U0[:3], nodes[:3])
    assert (rcg == 0).all()
    bad = list(nodes[:3])
    bad[1] = (np.array([0.0, 1e-3, 1.0001e-3, t1]), np.array([1000.0, 1000.0, np.nan, np.nan]))
    tb, ub, nsb, rcb, _ = h.solve_ensemble_continuous(pm, U0[:3], bad)
    assert rcb[1] != 0 and rcb[0] == 0 and rcb[2] == 0 and nsb[1] < len(t)
    assert np.array_equal(ub[0], ug[0]) and np.array_equal(ub[2], ug[2])
    h.close()


def test_a_to_b_ramps_against_quadrature():
    from scipy.integrate import quad
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    net = from_lists(2, [[(0, 1)]], [[(1, 1)]])
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A)
    rates = [50.0, 100.0, 200.0, 400.0]
    nodes = [(np.array([0.0, 2.0]), np.array([500.0, 500.0 + 2.0 * r])) for r in rates]
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(kp(2.0, chunk=0.5, save=0.25), np.tile([1.0, 0.0], (4, 1)), nodes)
    assert (rcs == 0).all() and len(t) == 9
    for m, r in enumerate(rates):
        kfun = lambda tt: float(orc.arrhenius(Ea, A, 500.0 + r * tt)[0])
        truth = np.array([np.exp(-quad(kfun, 0.0, tt, epsabs=1e-13, epsrel=1e-13)[0]) for tt in t])
        assert units(u[m, :, 0], truth) < 100, r
    h.close()


def _thread_case(K, monkeypatch=None):
    n, t1 = 2000, 2e-3
    net, Ea, A = synthetic_crn(n, 5 * n)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    U0 = np.zeros((K, n)); U0[:, 0] = 1.0
    nodes = _profiles(K, t1)
    p = kp(t1)
    t, u, ns, rcs, sts = h.solve_ensemble_continuous(p, U0, nodes)
    assert (rcs == 0).all() and (ns == 3).all()
    for m in range(K):
        ts, us, rc, st, _ = h.solve_continuous(p, U0[m], *nodes[m])
        assert rc == 0 and np.array_equal(ts, t) and np.array_equal(us, u[m]), m
        for key in ("n_steps", "n_rejected", "n_rhs", "n_jac", "n_factor", "n_linsolve", "n_newton_fail", "n_restarts", "n_retries", "n_lu_reused"):
            assert st[key] == sts[m][key], (m, key)
    h.close()


def test_large_network_members_are_kin_solve_continuous_calls_on_threads():
    _thread_case(3)


def test_threads_take_several_members_each(monkeypatch):
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", "threads")
    monkeypatch.setenv("KIN_ENSEMBLE_THREADS", "2")
    _thread_case(5)


def test_argument_errors(monkeypatch):
    net = from_lists(2, [[(0, 1)]], [[(1, 1)]])
    h = capi.HipNetwork.from_flat(net)
    u0 = np.tile([1.0, 0.0], (2, 1))
    ok = (np.array([0.0, 1.0]), np.array([500.0, 600.0]))
    p = kp(1.0, chunk=0.5, save=0.25)
    with pytest.raises(capi.KineticaHipError) as e:            # no Arrhenius parameters
        h.solve_ensemble_continuous(p, u0, [ok, ok])
    assert e.value.code == capi.KIN_ERR_STATE
    h.set_arrhenius([8.0e4], [1.0e-17])
    empty = (np.zeros(0), np.zeros(0))
    for bad in (empty, (np.array([0.0]), np.array([500.0])), (np.array([0.0, 1.0, 0.5]), np.array([500.0, 600.0, 550.0]))):
        for members in ([ok, bad], [bad, ok]):                 # an empty profile, one node, decreasing t - in either place
            with pytest.raises(capi.KineticaHipError) as e:
                h.solve_ensemble_continuous(p, u0, members)
            assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:            # every member empty
        h.solve_ensemble_continuous(p, u0, [empty, empty])
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:            # no save grid
        h.solve_ensemble_continuous(kp(1.0, chunks=False), u0, [ok, ok])
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", "lockstep")
    with pytest.raises(capi.KineticaHipError) as e:
        h.solve_ensemble_continuous(p, u0, [ok, ok])
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED
    monkeypatch.delenv("KIN_ENSEMBLE_ROUTE")
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(p, u0, [ok, ok])
    assert (rcs == 0).all() and np.array_equal(u[0], u[1])
    h.close()


def test_solve_network_ensemble_end_to_end():
    from kinetica_jl_amd import conditions as C
    from kinetica_jl_amd import solving as S
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    ramps = [(900.0, 1300.0, 2e5), (1000.0, 1200.0, 1e5), (1300.0, 1000.0, -3e5)]
    methods = []
    for i, (T0, T1, r) in enumerate(ramps):
        u0 = np.zeros(n); u0[0] = 1.0; u0[i + 1] = 0.1
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=r, X_start=T0, X_end=T1)}), calc))
    res = S.solve_network_ensemble(methods, sd, rd)
    assert len(res) == 3
    for m, out in zip(methods, res):
        assert out.sol.retcode == "Success" and out.pars is m.pars
        prof = m.conditions.profiles[0]
        np.testing.assert_array_equal(out.sol_vcs["T"], np.interp(out.sol.t, prof.sol.t, prof.sol.u))
        solo = S.solve_network(m, sd, rd)
        np.testing.assert_array_equal(solo.sol.t, out.sol.t)
        assert units(out.sol.u, solo.sol.u) <= 201
        assert units(out.sol.umax, solo.sol.umax) <= 201      # kin_solution_max of kin_solve_continuous
