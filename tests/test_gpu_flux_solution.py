"""GPU tests of the flux pass over stored solutions (kin_solution_flux) and of the host layer's reaction_fluxes.
Bounds as in test_gpu_flux.py: rates 4 2^-53 relative, flux (B + 8) 2^-53 sum_b |w_b rate_b|, the temperature form
+ (2 |Ea / (R T_b)| + 16) 2^-53 per term."""
import math

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TOL = 1e-13          # the sweep tolerance of test_gpu_parity.py
RGAS = 8.314462618


def kp(tspan, chunkstep, save):
    return capi.KinParams(tspan0=tspan[0], tspan1=tspan[1], abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0,
                          solve_chunks=1, ban_negatives=0, solve_chunkstep=chunkstep, maxiters=100000, save_interval=save)


def _ab():
    return S.SpeciesData.from_names(["A", "B"]), S.RxData(1, [[1]], [[2]], [[1]], [[1]])


def test_a_to_b_static():
    k, t_end, dt = 100.0, 0.01, 1e-4
    # the stored solution, read where it lives, against the same pass over the downloaded states
    h = capi.HipNetwork.from_flat(from_lists(2, [[(0, 1)]], [[(1, 1)]]))
    h.set_rates([k])
    t, u, rc, st, status = h.solve(kp((0.0, t_end), 1e-3, dt), [1.0, 0.0])
    assert rc == 0 and len(t) == 101
    w = S.flux_weights(t)
    f_sol, r_sol = h.solution_flux(w=w, want_rates=True)
    f_host, r_host = h.flux_batched(u, w=w, want_rates=True)
    assert np.array_equal(f_sol, f_host) and np.array_equal(r_sol, r_host)
    # ... with an explicit k row through k_row, and with weights of 1
    f_row = h.solution_flux(w=w, k=np.array([[k]]), k_row=np.zeros(len(t), np.int64))
    assert np.array_equal(f_row, f_sol)
    assert np.array_equal(h.solution_flux(), h.flux_batched(u))
    h.close()
    # the host layer on a solve_network output
    sd, rd = _ab()
    calc = S.DummyKineticCalculator([k])
    pars = S.ODESimulationParams(tspan=(0.0, t_end), u0=[1.0, 0.0], solve_chunkstep=1e-3, save_interval=dt, low_k_cutoff="none")
    out = S.solve_network(S.StaticODESolve(pars, C.ConditionSet({"T": 300.0}), calc), sd, rd)
    assert len(out.sol.t) == 101
    rf = S.reaction_fluxes(out, calc)
    w = S.flux_weights(out.sol.t)
    assert np.array_equal(rf.weights, w) and rf.rates is None
    terms = w * k * out.sol.u[:, 0]
    B = len(w)
    assert abs(rf.flux[0] - math.fsum(terms)) <= (B + 8) * EPS * np.abs(terms).sum() + 1e-300
    # the trapezoid bound for k e^(-k t): t_end dt^2 k^3 / 12 = 8.34e-6 (actual error 5.3e-6), plus 100 tolerance units
    # of the solve itself (max e)
    closed = 1.0 - math.exp(-k * t_end)
    print("flux", rf.flux[0], "closed form", closed, "difference", rf.flux[0] - closed)
    assert abs(rf.flux[0] - closed) <= t_end * dt ** 2 * k ** 3 / 12 + 1e-6
    # production - consumption is the weighted sum of the sweep's du
    h = capi.HipNetwork(*out.rd.flat(out.sd.n), index_base=1)
    h.set_rates([k])
    DU = h.rhs_batched(out.sol.u)
    h.close()
    scale = (np.abs(w)[:, None] * (k * np.abs(out.sol.u[:, :1]))).sum(axis=0)      # sum_b |w_b| abs_rhs_b, the same for A and B
    assert np.all(np.abs((rf.production - rf.consumption) - (w[:, None] * DU).sum(axis=0)) <= TOL * scale)
    assert rf.production[0] == 0.0 and rf.consumption[1] == 0.0 and rf.production[1] == rf.flux[0] == rf.consumption[0]


def test_a_to_b_discrete_updates():
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    t_end = 0.01
    Tst = np.where(np.arange(5) % 2 == 0, 900.0, 1100.0)
    h = capi.HipNetwork.from_flat(from_lists(2, [[(0, 1)]], [[(1, 1)]]))
    h.set_arrhenius(Ea, A)
    h.rates_at(900.0)
    grid = h.solve(kp((0.0, t_end), 1e-3, 5e-4), [1.0, 0.0])[0]
    tstops = grid[:20:4].copy()                                       # every 2e-3 s, bit for bit the saved times
    np.testing.assert_allclose(tstops, np.arange(5) * 2e-3, rtol=0, atol=1e-15)
    t, u, rc, st, status = h.solve(kp((0.0, t_end), 1e-3, 5e-4), [1.0, 0.0], tstops=tstops, T_stops=Tst)
    assert rc == 0 and len(t) == 21
    held = S.held_stop_index(t, tstops)
    assert np.array_equal(t, grid)                                    # saved times coincide with stops ...
    assert np.array_equal(held[::4], [0, 1, 2, 3, 4, 4])              # ... and a row at a stop uses the new temperature
    kdev = np.array([capi.arrhenius_eval(Ea, A, T)[0] for T in Tst])  # the device's own Arrhenius: no slack needed
    ref = kdev[held] * u[:, 0]
    _, rates = h.solution_flux(T_rows=Tst[held], want_rates=True)
    assert np.all(np.abs(rates[:, 0] - ref) <= 4 * EPS * np.abs(ref) + 1e-300)
    # the host layer on the same solution: ArrheniusRates carries the stop temperatures
    sd, rd = _ab()
    calc = S.PrecalculatedArrheniusCalculator(Ea, A)
    cs = C.ConditionSet({"T": C.LinearDirectProfile(rate=1.0e4, X_start=900.0, X_end=1000.0)}, ts_update=2e-3)   # carrier of discrete_updates
    pars = S.ODESimulationParams(tspan=(0.0, t_end), u0=[1.0, 0.0], solve_chunkstep=1e-3, save_interval=5e-4, low_k_cutoff="none")
    sol_k = S.ArrheniusRates(tstops, Tst, Ea, A, None, 1.0)
    out = S.ODESolveOutput(sd, rd, S.ODESolution(t, u, "Success", k=sol_k), sol_k, None, pars, cs)
    rf = S.reaction_fluxes(out, calc, rates=True)
    assert np.array_equal(rf.rates, rates)
    # a host rate table (any calculator): through k_row, and through the table the solve left on the device
    table = kdev[:, None].copy()
    t2, u2, rc2, _, _ = h.solve(kp((0.0, t_end), 1e-3, 5e-4), [1.0, 0.0], tstops=tstops, k_table=table)
    assert rc2 == 0 and np.array_equal(t2, t)
    ref2 = kdev[held] * u2[:, 0]
    w = S.flux_weights(t2)
    f_row, r_row = h.solution_flux(w=w, k=table, k_row=held, want_rates=True)
    f_tab, r_tab = h.solution_flux(w=w, k_row=held, want_rates=True)
    assert np.all(np.abs(r_row[:, 0] - ref2) <= 4 * EPS * np.abs(ref2) + 1e-300)
    assert np.array_equal(r_row, r_tab) and np.array_equal(f_row, f_tab)
    out2 = S.ODESolveOutput(sd, rd, S.ODESolution(t2, u2, "Success"), S.DiscreteRates(tstops, table), None, pars, cs)
    rf2 = S.reaction_fluxes(out2, calc, rates=True)              # sol_k without temperatures (as load_output returns it): rows of sol_k.u
    assert np.array_equal(rf2.rates, r_row) and np.array_equal(rf2.flux, f_row)
    h.close()


def test_continuous_profile():
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    sd, rd = _ab()
    calc = S.PrecalculatedArrheniusCalculator(Ea, A)
    cs = C.ConditionSet({"T": C.LinearGradientProfile(rate=100.0, X_start=500.0, X_end=700.0)})   # no ts_update: continuous
    pars = S.ODESimulationParams(tspan=(0.0, 2.0), u0=[1.0, 0.0], solve_chunkstep=0.5, save_interval=0.25, low_k_cutoff="none")
    out = S.solve_network(S.VariableODESolve(pars, cs, calc), sd, rd)
    assert out.sol.retcode == "Success" and len(out.sol.t) == 9
    rf = S.reaction_fluxes(out, calc, rates=True)
    T = np.asarray(out.sol_vcs["T"])
    ref = np.array([orc.arrhenius(Ea, A, Tb)[0] for Tb in T]) * out.sol.u[:, 0]
    bound = (4 + 2 * np.abs(Ea[0] / (RGAS * T)) + 16) * EPS * np.abs(ref) + 1e-300
    assert np.all(np.abs(rf.rates[:, 0] - ref) <= bound)
    terms = rf.weights * ref
    fb = (len(T) + 8) * EPS * np.abs(terms).sum() + ((2 * np.abs(Ea[0] / (RGAS * T)) + 16) * EPS * np.abs(terms)).sum() + 1e-300
    assert abs(rf.flux[0] - math.fsum(terms)) <= fb


def test_300_species_network_top_reactions_and_gross_rates():
    net, Ea, A = synthetic_crn(300, 1500)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(300)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0={"S0": 1.0}, solve_chunkstep=1e-3, save_interval=1e-4, low_k_cutoff="none")
    out = S.solve_network(S.StaticODESolve(pars, C.ConditionSet({"T": 1000.0}), calc), sd, rd)
    assert out.sol.retcode == "Success" and out.rd.nr == 1500
    rf = S.reaction_fluxes(out, calc)
    on = orc.OracleNetwork.from_flat(net)
    k = capi.arrhenius_eval(Ea, A, 1000.0, 1e12)
    ref = np.stack([on.rates(k, ub) for ub in out.sol.u])
    w = rf.weights
    B = len(w)
    terms = w[:, None] * ref
    flux_np = terms.sum(axis=0)
    assert np.all(np.abs(rf.flux - flux_np) <= 2 * (B + 8) * EPS * np.abs(terms).sum(axis=0) + 1e-300)   # both sums carry the bound
    assert np.array_equal(rf.top(5), np.argsort(-np.abs(flux_np), kind="stable")[:5])
    # gross rates are sums of non-negative terms - up to rounding and up to what the reference's own rates show below
    # zero (a saved state may hold concentrations a few rounding errors below zero)
    absf = np.abs(terms).sum(axis=0)
    negf = np.maximum(-terms, 0.0).sum(axis=0)
    rr = np.repeat(np.arange(net.n_reactions), np.diff(net.reac_ptr))
    pr = np.repeat(np.arange(net.n_reactions), np.diff(net.prod_ptr))
    slack_p, slack_c = np.zeros(300), np.zeros(300)
    np.add.at(slack_p, net.prod_idx, net.prod_sto * ((B + 8) * EPS * absf + negf)[pr])
    np.add.at(slack_c, net.reac_idx, net.reac_sto * ((B + 8) * EPS * absf + negf)[rr])
    assert np.all(rf.production >= -slack_p) and np.all(rf.consumption >= -slack_c)
    assert rf.production.max() > 0 and rf.consumption[0] > 0
