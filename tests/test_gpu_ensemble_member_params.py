"""GPU tests of per-member Arrhenius parameters in ensembles (kin_solve_ensemble_continuous_params / _discrete_params,
HipNetwork.solve_ensemble_continuous / _discrete with Ea= / A=, solving.solve_network_ensemble over calculators that differ in
value, solving.sample_arrhenius). The references are code that existed before: the shared-parameter path on a second handle
set to the member's (Ea, A), the closed form, the quadrature of test_gpu_ensemble_continuous.py, oracle/bdf.py through its
k_of_time, and the explicit-k form of kin_ensemble_flux.

The network: 120 species, 601 reactions - R odd and no multiple of 512, so the stride loops' tail and the flux pass's clamped
last pair are exercised. synthetic_crn builds forward / reverse pairs only (an odd count raises), so it is the first 601
reactions of synthetic_crn(120, 602). K = 5 members with parameters distinct in every member (member 0, the last and the
middle ones catch offset errors), 2 ms, save interval 2.5e-4, the profiles of test_gpu_ensemble_continuous.py."""
import ctypes

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import bdf as obdf
from oracle import oracle as orc
from test_gpu_ensemble_continuous import _profiles, kp, units

pytestmark = pytest.mark.gpu

N, R, K, T1, SAVE = 120, 601, 5, 2e-3, 2.5e-4
COUNTERS = ("n_steps", "n_rejected", "n_rhs", "n_jac", "n_factor", "n_linsolve", "n_newton_fail", "n_chunks", "n_restarts", "n_retries",
            "final_abstol", "final_reltol", "lu_dense_dim", "lu_sparse_rows", "lu_rounds", "lu_nnz", "n_lu_reused", "lu_slots",
            "n_bad_pivot", "n_lu_dropped")      # every field of kin_stats but wall_seconds


def _odd_network(n, r_odd):
    net, Ea, A = synthetic_crn(n, r_odd + 1)
    return net.subset(np.arange(r_odd)), Ea[:r_odd].copy(), A[:r_odd].copy()


def _member_params(Ea, A, k, seed=11):
    """Barriers off by up to 3 kJ/mol, prefactors by up to e, independently in every member and reaction."""
    rng = np.random.default_rng(seed)
    return Ea[None, :] + rng.uniform(-3e3, 3e3, (k, len(Ea))), A[None, :] * np.exp(rng.uniform(-1.0, 1.0, (k, len(A))))


class Case:
    def __init__(self):
        self.net, self.Ea, self.A = _odd_network(N, R)
        assert self.net.n_reactions == R and R % 2 == 1 and R % 512 != 0
        self.EaK, self.AK = _member_params(self.Ea, self.A, K)
        rng = np.random.default_rng(3)
        self.U0 = np.zeros((K, N)); self.U0[:, 0] = 1.0; self.U0[:, 1] = rng.uniform(0.0, 0.5, K)
        self.nodes = _profiles(K, T1)
        # stop grids of different lengths (one stop: 1000 K held from 0 on), as _schedules of test_gpu_ensemble_discrete.py
        self.stops = []
        for m, n in enumerate([3, 1, 6, 4, 9]):
            if n == 1:
                self.stops.append((np.zeros(1), np.array([1000.0])))
            else:
                tend = T1 * (0.4 + 0.05 * m)
                ts = np.linspace(0.0, tend, n)
                self.stops.append((ts, 900.0 + (300.0 + 20.0 * m) * ts / tend))
        self.p = kp(T1, save=SAVE)

    def handle(self, Ea=None, A=None):
        h = capi.HipNetwork.from_flat(self.net)
        h.set_arrhenius(self.Ea if Ea is None else Ea, self.A if A is None else A, k_max=1e12)
        return h


@pytest.fixture(scope="module")
def case():
    return Case()


def _pd(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _raw(h, name, p, U0, Ea, A, pairs):
    """The _params entry itself, NULLs included (the Python methods take the existing entry when no parameters are given)."""
    k = len(U0)
    ptr = np.zeros(k + 1, np.int64); ptr[1:] = np.cumsum([len(a) for a, _ in pairs])
    t_all = np.ascontiguousarray(np.concatenate([a for a, _ in pairs])); T_all = np.ascontiguousarray(np.concatenate([b for _, b in pairs]))
    U0 = np.ascontiguousarray(U0)
    return h._ensemble(getattr(capi.lib(), name), p, k, _pd(U0), _pd(Ea), _pd(A), ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                       _pd(t_all), _pd(T_all))


def _same_call(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for m, (sa, sb) in enumerate(zip(a[4], b[4])):
        for key in COUNTERS:
            assert sa[key] == sb[key], (m, key)


@pytest.mark.parametrize("shared_cu", ["0", "1"])
def test_continuous_members_are_k1_calls_on_a_handle_with_their_parameters(case, monkeypatch, shared_cu):
    """Item 1, both resident builds (KIN_RESIDENT_SHARED_CU as test_gpu_ensemble_discrete.py selects them)."""
    monkeypatch.setenv("KIN_RESIDENT_SHARED_CU", shared_cu)
    h = case.handle()
    t, u, ns, rcs, sts = h.solve_ensemble_continuous(case.p, case.U0, case.nodes, Ea=case.EaK, A=case.AK)
    assert (rcs == 0).all() and u.shape == (K, len(t), N) and (ns == len(t)).all() and len(t) == 9
    ts_, us_, _, rcs_, _ = h.solve_ensemble_continuous(case.p, case.U0, case.nodes)          # the handle's parameters for all
    assert (rcs_ == 0).all()
    for m in range(K):
        h2 = case.handle(case.EaK[m], case.AK[m])
        t1, u1, ns1, rc1, st1 = h2.solve_ensemble_continuous(case.p, case.U0[m:m + 1], [case.nodes[m]])
        h2.close()
        assert rc1[0] == 0 and np.array_equal(t1, t) and np.array_equal(u1[0], u[m]), m
        assert st1[0]["n_steps"] == sts[m]["n_steps"] and st1[0]["n_factor"] == sts[m]["n_factor"], m
        d = units(u[m], us_[m])
        print(f"member {m}: own parameters against the handle's: {d:.3g} units")
        assert d > 1e3, m
    h.close()


@pytest.mark.parametrize("kind", ["continuous", "discrete"])
def test_nulls_and_copies_of_the_handles_parameters_change_no_bit(case, kind):
    """Item 2, first half: the new entry with NULLs, and with K copies of the handle's parameters, against the existing entry."""
    h = case.handle()
    pairs = case.nodes if kind == "continuous" else case.stops
    old = (h.solve_ensemble_continuous if kind == "continuous" else h.solve_ensemble_discrete)(case.p, case.U0, pairs)
    assert (old[3] == 0).all()
    name = f"kin_solve_ensemble_{kind}_params"
    _same_call(_raw(h, name, case.p, case.U0, None, None, pairs), old)
    EaC, AC = np.ascontiguousarray(np.tile(case.Ea, (K, 1))), np.ascontiguousarray(np.tile(case.A, (K, 1)))
    _same_call(_raw(h, name, case.p, case.U0, EaC, AC, pairs), old)
    h.close()


def test_thread_route_leaves_the_handle_as_it_was(case, monkeypatch):
    """Item 2, second half: kin_rates_at and a shared call on the parent handle before and after a per-member call."""
    monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", "threads")
    monkeypatch.setenv("KIN_ENSEMBLE_THREADS", "2")
    h = case.handle()
    k0 = h.rates_at(1000.0)
    before = h.solve_ensemble_continuous(case.p, case.U0, case.nodes)
    mine = h.solve_ensemble_continuous(case.p, case.U0, case.nodes, Ea=case.EaK, A=case.AK)
    assert (before[3] == 0).all() and (mine[3] == 0).all() and units(mine[1][K - 1], before[1][K - 1]) > 1e3
    assert np.array_equal(h.rates_at(1000.0), k0)
    _same_call(h.solve_ensemble_continuous(case.p, case.U0, case.nodes), before)
    h.close()


@pytest.mark.parametrize("route", ["resident", "threads", "lockstep"])
def test_discrete_members_on_every_route(case, monkeypatch, route):
    """Item 3. Resident and thread route: bit-identical to kin_solve on a handle set to the member's parameters, with the
    member's stops. Lockstep: the bound test_lockstep_members_with_their_own_schedules applies to lockstep members against
    their solo kin_solve on the host-driven integrator - 50 units, step counts within 2 % + 2 - and blocks of fewer members
    (the parameters offset with the block) give the bits of one block."""
    if route != "resident":
        monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", route)
    if route == "threads":
        monkeypatch.setenv("KIN_ENSEMBLE_THREADS", "2")          # a thread takes several members, one after the other
    h = case.handle()
    t, u, ns, rcs, sts = h.solve_ensemble_discrete(case.p, case.U0, case.stops, Ea=case.EaK, A=case.AK)
    assert (rcs == 0).all() and (ns == len(t)).all() and len(t) == 9
    if route == "lockstep":
        monkeypatch.setenv("KIN_ENSEMBLE_MAX_MEMBERS", "2")
        tb, ub, _, rcb, _ = h.solve_ensemble_discrete(case.p, case.U0, case.stops, Ea=case.EaK, A=case.AK)
        monkeypatch.delenv("KIN_ENSEMBLE_MAX_MEMBERS")
        assert (rcb == 0).all() and np.array_equal(tb, t) and np.array_equal(ub, u)
        monkeypatch.setenv("KIN_RESIDENT", "0")                  # the reference: kin_solve on the host-driven integrator
    h.close()
    for m in range(K):
        h2 = case.handle(case.EaK[m], case.AK[m])
        tk, uk, rck, stk, _ = h2.solve(case.p, case.U0[m], tstops=case.stops[m][0], T_stops=case.stops[m][1])
        h2.close()
        assert rck == 0 and np.array_equal(tk, t), m
        if route == "lockstep":
            d = units(u[m], uk)
            print(f"lockstep member {m}: {d:.3g} units, steps {sts[m]['n_steps']} against {stk['n_steps']}")
            assert d < 50, m
            assert abs(sts[m]["n_steps"] - stk["n_steps"]) <= 0.02 * stk["n_steps"] + 2, m
        else:
            assert np.array_equal(uk, u[m]) and stk["n_steps"] == sts[m]["n_steps"], m
    assert units(u[0], u[K - 1]) > 1e3


def test_a_to_b_against_the_closed_form_the_quadrature_and_the_oracle():
    """Item 4: A -> B, K = 4, distinct Ea and distinct A per member. Flat profile: exp(-k_m t); ramp: the quadrature and the
    bound (100 units) of test_a_to_b_ramps_against_quadrature; member 2 of the ramp against oracle/bdf.py under the bound the
    continuous test uses for it (100 units)."""
    from scipy.integrate import quad
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    EaK = np.array([[7.6e4], [8.0e4], [8.3e4], [8.7e4]]); AK = np.array([[3.0e-17], [1.0e-17], [0.4e-17], [2.0e-17]])
    net = from_lists(2, [[(0, 1)]], [[(1, 1)]])
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A)
    p = kp(2.0, chunk=0.5, save=0.25)
    U0 = np.tile([1.0, 0.0], (4, 1))
    flat = [(np.array([0.0, 2.0]), np.array([640.0, 640.0]))] * 4
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(p, U0, flat, Ea=EaK, A=AK)
    assert (rcs == 0).all() and len(t) == 9
    for m in range(4):
        k = float(orc.arrhenius(EaK[m], AK[m], 640.0)[0])
        d = units(u[m, :, 0], np.exp(-k * t))
        print(f"flat, member {m}: k = {k:.4g}, {d:.3g} units")
        assert d < 100 and units(u[m, :, 1], 1.0 - np.exp(-k * t)) < 100, m
    assert units(u[0], u[3]) > 1e3
    r = 100.0
    ramp = [(np.array([0.0, 2.0]), np.array([500.0, 500.0 + 2.0 * r]))] * 4
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(p, U0, ramp, Ea=EaK, A=AK)
    assert (rcs == 0).all() and len(t) == 9
    for m in range(4):
        kfun = lambda tt: float(orc.arrhenius(EaK[m], AK[m], 500.0 + r * tt)[0])
        truth = np.array([np.exp(-quad(kfun, 0.0, tt, epsabs=1e-13, epsrel=1e-13)[0]) for tt in t])
        d = units(u[m, :, 0], truth)
        print(f"ramp, member {m}: {d:.3g} units")
        assert d < 100, m
    on = orc.OracleNetwork.from_flat(net)
    tn, Tn = ramp[2]
    to, uo, rco, _ = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), 2,
                                               dict(tspan=(0.0, 2.0), solve_chunkstep=0.5, save_interval=0.25), np.array([1.0, 0.0]),
                                               k_of_time=lambda tg: orc.arrhenius(EaK[2], AK[2], float(np.interp(tg, tn, Tn))))
    assert rco == 0 and np.array_equal(to, t) and units(u[2], uo) <= 100
    h.close()


@pytest.mark.parametrize("rows", [None, "1"])
def test_flux_on_the_per_member_record(monkeypatch, rows):
    """Item 5: ensemble_flux(w, T_rows) on a per-member record against ensemble_flux(w, k, k_row) with one kin_arrhenius_eval
    row per (member, row), bit for bit (the identity test_reuse_changes_no_bit establishes for shared parameters). 2 201
    reactions: with KIN_FLUX_ROWS=1 a segment's reactions take two parts (1 024 pairs each; the temperature form's default is
    one part of two rows at this size). Member 0 has a flat profile - its rate constants stay in registers from row to row -,
    the others ramp."""
    n, r = 300, 2201
    net, Ea, A = _odd_network(n, r)
    if rows is not None:
        monkeypatch.setenv("KIN_FLUX_ROWS", rows)
    plan = capi.flux_plan_host(n, r, K * 9, 256, temperature_form=True, segmented=True)
    assert plan["parts"] == (2 if rows == "1" else 1)
    EaK, AK = _member_params(Ea, A, K, seed=12)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    U0 = np.zeros((K, n)); U0[:, 0] = 1.0
    nodes = _profiles(K, T1)
    nodes[0] = (np.array([0.0, T1]), np.array([1100.0, 1100.0]))
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(kp(T1, save=SAVE), U0, nodes, Ea=EaK, A=AK)
    assert (rcs == 0).all() and (ns == len(t)).all()
    L = len(t)
    T_rows = np.stack([np.interp(t, tn, Tn) for tn, Tn in nodes])
    assert len(set(T_rows[0])) == 1 and len(set(T_rows[1])) > 1
    w = np.random.default_rng(5).uniform(0.5, 1.5, (K, L)) * SAVE
    krows = np.stack([capi.arrhenius_eval(EaK[m], AK[m], float(T_rows[m, j]), k_max=1e12) for m in range(K) for j in range(L)])
    ref = h.ensemble_flux(w=w, k=krows, k_row=np.arange(K * L).reshape(K, L))
    got = h.ensemble_flux(w=w, T_rows=T_rows)
    assert got.shape == (K, r) and got.tobytes() == ref.tobytes() and np.any(got[K - 1] != 0.0)
    # ... and not what the handle's own parameters give
    shared = h.ensemble_flux(w=w, k=np.stack([capi.arrhenius_eval(Ea, A, float(T), k_max=1e12) for T in T_rows.ravel()]),
                             k_row=np.arange(K * L).reshape(K, L))
    assert not np.array_equal(shared[K - 1], got[K - 1])
    h.close()


def test_refusals_and_record_lifetime(case):
    """Item 6."""
    h = case.handle()
    t, u, ns, rcs, _ = h.solve_ensemble_continuous(case.p, case.U0, case.nodes, Ea=case.EaK, A=case.AK)
    assert (rcs == 0).all()
    L = len(t)
    T_rows = np.stack([np.interp(t, tn, Tn) for tn, Tn in case.nodes])
    krows = np.stack([capi.arrhenius_eval(case.EaK[m], case.AK[m], float(T_rows[m, j]), k_max=1e12) for m in range(K) for j in range(L)])
    k_row = np.arange(K * L).reshape(K, L)
    calls = [lambda **kw: h.ensemble_drg(**kw), lambda **kw: h.ensemble_drgep(np.array([0]), **kw), lambda **kw: h.ensemble_pfa(**kw),
             lambda **kw: h.ensemble_reaction_importance(**kw), lambda **kw: h.ensemble_timescale(**kw)]
    for i, call in enumerate(calls):
        with pytest.raises(capi.KineticaHipError) as e:
            call(T_rows=T_rows)
        assert e.value.code == capi.KIN_ERR_UNSUPPORTED and "k_row" in str(e.value) and "per-member" in str(e.value), i
        call(k=krows, k_row=k_row)
    # states only: either record
    assert h.ensemble_max().shape == (K, N) and h.ensemble_moments()["count"] == K
    # a following shared call leaves a shared record: the T_rows form works again
    t2, _, _, rcs2, _ = h.solve_ensemble_continuous(case.p, case.U0, case.nodes)
    assert (rcs2 == 0).all()
    for call in calls:
        call(T_rows=T_rows)
    # exactly one of Ea / A, straight through the C ABI; no kin_set_arrhenius; a wrong shape from Python
    for name, pairs in (("kin_solve_ensemble_continuous_params", case.nodes), ("kin_solve_ensemble_discrete_params", case.stops)):
        for Ea, A in ((case.EaK, None), (None, case.AK)):
            with pytest.raises(capi.KineticaHipError) as e:
                _raw(h, name, case.p, case.U0, None if Ea is None else np.ascontiguousarray(Ea), None if A is None else np.ascontiguousarray(A), pairs)
            assert e.value.code == capi.KIN_ERR_INVALID_ARG
    h.close()
    bare = capi.HipNetwork.from_flat(case.net)
    for solve, pairs in ((bare.solve_ensemble_continuous, case.nodes), (bare.solve_ensemble_discrete, case.stops)):
        with pytest.raises(capi.KineticaHipError) as e:
            solve(case.p, case.U0, pairs, Ea=case.EaK, A=case.AK)
        assert e.value.code == capi.KIN_ERR_STATE
        for Ea, A in ((case.EaK[:, :-1], case.AK), (case.EaK, case.AK[:-1]), (case.EaK, None), (case.EaK.astype(complex), case.AK)):
            with pytest.raises(ValueError):
                solve(case.p, case.U0, pairs, Ea=Ea, A=A)
    bare.close()


def test_sobol_design_over_rate_parameters_end_to_end(case):
    """Item 7: sobol_design -> sample_arrhenius -> solve_network_ensemble(statistics=sobol, fluxes=True); input 0 moves
    barriers, input 1 prefactors, input 2 no reaction. Two members against solve_network of their own method within the
    step-sequence bound of the continuous end-to-end test (201 units)."""
    from kinetica_jl_amd import conditions as C
    M, P = 8, 3
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(N)])
    rd = S.RxData.from_flat(case.net)
    calc = S.PrecalculatedArrheniusCalculator(case.Ea, case.A, k_max=1e12)
    X = S.sobol_design(M, P, seed=4)
    spec = [("Ea", np.arange(0, R, 3), 3e3), ("lnA", np.arange(1, R, 3), 1.0), ("Ea", [], 3e3)]
    calcs = S.sample_arrhenius(calc, X, spec)
    u0 = np.zeros(N); u0[0] = 1.0; u0[1] = 0.2

    def method(c):
        pars = S.ODESimulationParams(tspan=(0.0, T1), u0=u0.copy(), save_interval=SAVE, low_k_cutoff="none")
        return S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=2e5, X_start=900.0, X_end=1300.0)}), c)
    methods = [method(c) for c in calcs]
    res = S.solve_network_ensemble(methods, sd, rd, statistics=dict(quantiles=None, sobol=dict(M=M, P=P)), fluxes=True,
                                   member_calculators=True)
    assert len(res) == M * (P + 2) and all(o.sol.retcode == "Success" for o in res)
    sb = res[0].sol.ensemble_stats.sobol
    u = np.stack([o.sol.u for o in res])
    hn = capi.HipNetwork.from_flat(case.net)
    ref = hn.members_sobol(u, M, P)
    hn.close()
    for name in ("first", "total", "mean", "var"):
        assert getattr(sb, name).tobytes() == ref[name].tobytes(), name
    assert sb.count == M
    # equal rows of the design give bit-identical members: block 2 + 2 is block A with the dummy column taken from B
    for m in range(M):
        assert np.array_equal(res[4 * M + m].sol.u, res[m].sol.u), m
        assert np.array_equal(res[4 * M + m].sol.fluxes.flux, res[m].sol.fluxes.flux), m
    assert np.all(sb.total[..., 2][sb.var > 0.0] == 0.0) and np.any(sb.var > 0.0)
    assert sb.total[-1, :, 0].max() > 0.0 and sb.total[-1, :, 1].max() > 0.0
    assert units(res[0].sol.u, res[M].sol.u) > 1e3          # samples of A and B differ
    assert np.any(res[0].sol.fluxes.flux != res[M].sol.fluxes.flux)
    for i in (1, 3 * M + 2):
        solo = S.solve_network(method(calcs[i]), sd, rd)
        np.testing.assert_array_equal(solo.sol.t, res[i].sol.t)
        d = units(res[i].sol.u, solo.sol.u)
        print(f"member {i} against its solve_network: {d:.3g} units")
        assert d <= 201, i
