"""GPU tests of the event times of stored trajectories: kin_ensemble_events reads the members' saved states where the last
kin_solve_ensemble* call left them, kin_solution_events those of the last kin_solve; solving.event_times, sobol_indices(of=...)
and solve_network_ensemble(events=...) on top.

The ensemble is the one of test_gpu_ensemble_sobol.py: synthetic_crn(300, 1500) on the resident route at 1000 K, 21 saved rows,
a Saltelli design of M = 16 base samples over P = 4 inputs (K = 96 members) on the three reactions that carry the most flux.
  stored ensemble, trajectories downloaded or not, and the host entry over the download: bit for bit, and against
  event_cases.ref_events on the download
  u_peak is kin_ensemble_max's array, byte for byte
  the half-life of A in A -> B against ln 2 / k"""
import math

import numpy as np
import pytest

import event_cases as ec
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn
from test_gpu_ensemble_analysis import kp

pytestmark = pytest.mark.gpu
M, P = 16, 4
K = M * (P + 2)
# what is asked of the ensemble: an induction time, a half-life, the falling edge of a pulse, an absolute threshold after t_min
REQUESTS = [
    dict(level=0.1, kind="of_peak", direction="rise", start="begin"),
    dict(level=0.5, kind="of_start", direction="fall", start="begin"),
    dict(level=0.5, kind="of_peak", direction="fall", start="peak", never=2e-3),
    dict(level=1e-6, kind="abs", direction="rise", start="begin", row_begin=3),
]


@pytest.fixture(scope="module")
def design():
    """The handle after the design's solve with trajectories downloaded, and everything the tests compare with."""
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    k0 = h.rates_at(1000.0)
    u0 = np.zeros(300); u0[0] = 1.0
    p = kp(2e-3, save=1e-4)
    h.set_rates(k0)
    t, us, rc, _, _ = h.solve(p, u0)
    assert rc == 0 and len(t) == 21
    single = dict(t=t, u=us, umax=h.solution_max(),
                  events=[h.solution_events(**r) for r in REQUESTS])
    top = np.argsort(-np.abs(h.solution_flux(w=S.flux_weights(t))))[:3]
    X = S.sobol_design(M, P, seed=7)
    k = np.tile(k0, (K, 1))
    k[:, top] *= np.exp(0.6 * (X[:, :3] - 0.5))
    U0 = np.tile(u0, (K, 1))
    t0, none, ns0, rcs0, _ = h.solve_ensemble(p, U0, k=k, trajectories=False)
    assert none is None and np.all(rcs0 == 0) and np.all(ns0 == 21)
    lean = [h.ensemble_events(t0, **r) for r in REQUESTS]
    t1, u, ns, rcs, _ = h.solve_ensemble(p, U0, k=k, trajectories=True)
    assert u.shape == (K, 21, 300) and np.array_equal(ns, ns0) and np.array_equal(t0, t1)
    yield dict(h=h, t=t1, u=u, ns=ns, lean=lean, single=single)
    h.close()


@pytest.mark.parametrize("q", range(len(REQUESTS)))
def test_three_routes_agree_with_each_other_and_the_restatement(design, q):
    h, t, u, ns, req = design["h"], design["t"], design["u"], design["ns"], REQUESTS[q]
    stored = h.ensemble_events(t, **req)
    host = h.events_segmented(u, t, seg_n=ns, **req)
    ref = ec.ref_events(u, t, seg_n=ns, **req)
    for name in ec.OUTPUTS:
        assert stored[name].shape == (K, 300)
        assert ec.same_bits(design["lean"][q][name], stored[name]) and ec.same_bits(host[name], stored[name]), name
        assert ec.same_bits(stored[name], ref[name]), name
    if req.get("row_begin", 0) == 0:
        assert stored["u_peak"].tobytes() == h.ensemble_max().tobytes()
    found = ~np.isnan(stored["t_cross"]) if "never" not in req else stored["t_cross"] != req["never"]
    assert found.sum() > K and np.all(stored["t_cross"][found] >= t[req.get("row_begin", 0)]) and np.all(stored["t_cross"][found] <= t[-1] + 1e-15)
    # every member's own times [K][n_rows]: the same grid given per member gives the same bytes
    per = h.ensemble_events(np.tile(t, (K, 1)), **req)
    assert all(ec.same_bits(per[name], stored[name]) for name in ec.OUTPUTS)


def test_solution_route(design):
    s = design["single"]
    for req, got in zip(REQUESTS, s["events"]):
        ref = ec.ref_events(s["u"][None], s["t"], **req)
        for name in ec.OUTPUTS:
            assert got[name].shape == (300,) and ec.same_bits(got[name], ref[name][0]), (req, name)
    assert s["events"][0]["u_peak"].tobytes() == s["umax"].tobytes()


def test_half_life_of_a_first_order_decay():
    """A -> B with rate constant k: u_A = exp(-k t), half-life ln 2 / k. The gate is the sum of
      the chord's error over one save interval dt: u_A is convex, the chord lies above it by at most k^2 dt^2 u / 8, which the
        slope k u turns into at most k dt^2 / 8 in time (1.25e-6 s for k = 1000 / s, dt = 1e-4 s);
      the solve's error: the saved values are within C (reltol u + abstol) of exp(-k t) with C = 100 allowed for the growth of
        the local error the controller holds at (reltol, abstol) = (1e-8, 1e-10) into a global one and for the interpolation
        onto the save grid; at the crossing u = 1/2, and the two values around it move the crossing by at most
        2 C (reltol + abstol) / (k / 2) (4.04e-9 s)."""
    k, dt, C = 1000.0, 1e-4, 100.0
    h = capi.HipNetwork(2, [0, 1], [0], [1], [0, 1], [1], [1])
    h.set_rates([k])
    p = kp(2e-3, save=dt)
    t, u, rc, _, _ = h.solve(p, np.array([1.0, 0.0]))
    assert rc == 0 and len(t) == 21
    ev = h.solution_events(level=0.5, kind="of_start", direction="fall")
    gate = k * dt * dt / 8.0 + 2.0 * C * (p.reltol + p.abstol) / (0.5 * k)
    print(f"half-life {ev['t_cross'][0]!r}, ln 2 / k {math.log(2.0) / k!r}, gate {gate!r}")
    assert abs(ev["t_cross"][0] - math.log(2.0) / k) <= gate
    assert ev["u_peak"][0] == 1.0 and ev["t_peak"][0] == t[0] and ev["t_peak"][1] == t[-1]
    assert ev["t_cross"][1] == t[0]                        # B starts at 0: l = 0 is met at the first row
    rise = h.solution_events(level=0.5, kind="abs", direction="rise")      # B reaches 1/2 when A does
    assert abs(rise["t_cross"][1] - math.log(2.0) / k) <= gate
    h.close()


def test_sobol_indices_of_event_times(design):
    h, t = design["h"], design["t"]
    events = dict(level=0.5, kind="of_peak", direction="rise")
    sel = [0, 7, 150, 299]
    for of in ("t_peak", "t_cross"):
        block = np.ascontiguousarray(h.ensemble_events(t, **events)[of][:, None, :])
        ref = h.members_sobol(block, M, P, species=sel)
        si = S.sobol_indices(h, t, M, P, species=sel, of=of, events=events)
        assert isinstance(si, S.SobolIndices) and si.count == M and si.first.shape == (1, len(sel), P)
        for name in ("first", "total", "mean", "var"):
            assert ec.same_bits(getattr(si, name), ref[name]), (of, name)
    st = S.ensemble_statistics(h, t, quantiles=(0.5,), species=sel, of="t_peak", events=events)
    mom = h.members_moments(np.ascontiguousarray(h.ensemble_events(t)["t_peak"][:, None, :]))
    assert st.count == K and st.mean.shape == (1, 300) and ec.same_bits(st.mean, mom["mean"]) and st.quantiles.shape == (1, 1, len(sel))
    ev = S.event_times(h, t=t, species=sel, t_min=2.5e-4, **events)
    raw = h.ensemble_events(t, row_begin=3, **events)
    assert all(ec.same_bits(getattr(ev, name), raw[name][:, sel]) for name in ec.OUTPUTS) and ev.species.tolist() == sel


def test_solve_network_ensemble_attaches_the_event_times():
    from kinetica_jl_amd import conditions as C
    n = 300
    net, Ea, A = synthetic_crn(n, 5 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    methods = []
    for x in (0.0, 0.3, 0.7, 1.0):
        u0 = np.zeros(n); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=1e5 * (1.0 + 3.0 * x), X_start=900.0,
                                                                                             X_end=1300.0)}), calc))
    events = dict(level=0.5, kind="of_start", direction="fall", species=[0, 5, 17])
    plain = S.solve_network_ensemble(methods, sd, rd)
    assert all(o.sol.events is None for o in plain)      # the default: the call as it always was
    with pytest.raises(ValueError):
        S.solve_network_ensemble(methods, sd, rd, events=dict(events, species=[n]))
    full = S.solve_network_ensemble(methods, sd, rd, events=events)
    lean = S.solve_network_ensemble(methods, sd, rd, trajectories=False, events=events)
    ev = lean[0].sol.events
    assert isinstance(ev, S.EventTimes) and all(o.sol.events is ev for o in lean) and lean[0].sol.u is None
    u = np.stack([o.sol.u for o in plain])
    ref = ec.ref_events(u, plain[0].sol.t, 0.5, kind="of_start", direction="fall")
    for name in ec.OUTPUTS:
        got = getattr(ev, name)
        assert got.shape == (len(methods), 3) and ec.same_bits(got, getattr(full[0].sol.events, name)), name
        assert ec.same_bits(got, ref[name][:, [0, 5, 17]]), name
    assert ev.species.tolist() == [0, 5, 17] and np.array_equal(ev.t, plain[0].sol.t)
    assert np.all(ev.t_cross[:, 0] > 0.0) and np.all(ev.t_cross[:, 0] < plain[0].sol.t[-1])      # the feed falls to half of its start
    one = S.event_times(plain[1], level=0.5, kind="of_start", direction="fall", species=["S0", 5, "S17"])
    assert all(ec.same_bits(getattr(one, name), getattr(ev, name)[1]) for name in ec.OUTPUTS)
    for a, b in zip(full, plain):
        np.testing.assert_array_equal(a.sol.u, b.sol.u)
