"""GPU tests of observables over stored trajectories: kin_ensemble_observables reads the members' saved states where the last
kin_solve_ensemble* call left them and, with store, puts its result in their place, marked as a record of observables;
kin_solution_observables reads those of the last kin_solve; solving.ensemble_observables / solution_observables and
solve_network_ensemble(observables=...) on top.

The ensemble: synthetic_crn(20, 100), six members on ramps from 900 K at 1e5 .. 4e5 K/s that hold at 1300 K, 2 ms, a row every
2.5e-4 s (9 rows). Members with different n_saved come from a resampling onto the temperature axis with store: the slow members
do not reach the last queries."""
import numpy as np
import pytest

import event_cases as ec
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import synthetic_crn
from test_gpu_ensemble_analysis import kp

pytestmark = pytest.mark.gpu
N, R = 20, 100
RATES = [1e5 * (1.0 + 3.0 * f) for f in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)]
K = len(RATES)
AT = np.arange(900.0, 1300.0 + 1.0, 50.0)
T1, SAVE = 2e-3, 2.5e-4
EPS = 2.0 ** -53

# lumped classes, a weighted sum with a negative weight, singletons, ratios (one of a form by itself), all species at weight 1
SPEC = {"light": [0, 1, 2, 3], "heavy": {7: 2.0, 9: 0.5, 11: -1.0}, "feed": 0, "total": list(range(N)), "x_feed": ("ratio", "feed", "total"),
        "sel": ("ratio", "light", "heavy"), "one": ("ratio", "total", "total"), "s5": 5}


def _nodes(rate):
    te = 400.0 / rate
    if te < T1:
        return np.array([0.0, te, T1]), np.array([900.0, 1300.0, 1300.0])
    return np.array([0.0, T1]), np.array([900.0, round(900.0 + rate * T1, 6)])


def _solve(h, trajectories=True):
    U0 = np.zeros((K, N)); U0[:, 0] = 1.0; U0[:, 3] = 0.25
    return h.solve_ensemble_continuous(kp(T1, save=SAVE), U0, [_nodes(r) for r in RATES], trajectories=trajectories)


@pytest.fixture(scope="module")
def stored():
    net, Ea, A = synthetic_crn(N, R)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    t, u, ns, rcs, _ = _solve(h)
    assert u.shape == (K, 9, N) and np.all(rcs == 0) and np.all(ns == 9)
    T = np.array([np.interp(t, *_nodes(r)) for r in RATES])
    yield dict(h=h, t=t, u=u, ns=ns, T=T, spec=S.observables(N, SPEC))
    h.close()


def _restore(d):
    t, u, ns, _, _ = _solve(d["h"])
    assert u.tobytes() == d["u"].tobytes() and np.array_equal(ns, d["ns"])


def _short_members(d):
    """The record resampled onto the temperature axis with store: members of different n_saved. Returns (block[K][Q][N] with
    zeros past a member's rows, n_saved)."""
    h = d["h"]
    out = h.ensemble_resample(d["T"], AT, store=True)
    ns = h.ensemble_size()[3]
    assert len(set(ns.tolist())) > 1 and ns.max() == len(AT) and 0 < ns.min() < len(AT)
    block = out.copy()
    for m in range(K):
        block[m, ns[m]:] = 0.0
    return block, ns


def test_stored_entry_equals_the_host_entry_on_the_download(stored):
    h, u, ns, spec = stored["h"], stored["u"], stored["ns"], stored["spec"]
    arrays = spec.arrays()
    for pitch in (None, N):
        got = h.ensemble_observables(*arrays, pitch=pitch)
        host = h.observables_segmented(u, *arrays, pitch=pitch, seg_n=ns)
        cpu = capi.observables_host(u, *arrays, pitch=pitch, seg_n=ns)
        assert got.shape == (K, 9, spec.G if pitch is None else N) and got.tobytes() == host.tobytes() and ec.same_bits(got, cpu), pitch
    assert h.ensemble_observable_count() == 0 and h.ensemble_size()[1] == 9            # nothing was stored
    r = S.ensemble_observables(h, SPEC)
    assert r.names == tuple(SPEC) and r.G == len(SPEC) and r.values.tobytes() == h.ensemble_observables(*arrays).tobytes()
    v = r.values
    assert np.all(v[:, :, 6] == 1.0) and v[:, :, 2].tobytes() == u[:, :, 0].tobytes() and v[:, :, 7].tobytes() == u[:, :, 5].tobytes()
    try:      # members of different n_saved, NaN-free zeros behind them
        block, ns2 = _short_members(stored)
        for pitch in (None, N):
            got = h.ensemble_observables(*arrays, pitch=pitch)
            assert got.tobytes() == h.observables_segmented(block, *arrays, pitch=pitch, seg_n=ns2).tobytes()
            assert all(not got[m, ns2[m]:].any() for m in range(K))
    finally:
        _restore(stored)


def test_a_full_length_form_agrees_with_ensemble_dot(stored):
    """One form over all species against kin_ensemble_dot. The two sum in different orders, so the bits need not agree: each is
    within (N + 1) 2^-53 sum |w_i u_i| of the exact value - N - 1 additions and one product per term, (1 + e)^(N) - 1 to first
    order - and the gate is the sum of the two bounds."""
    h, u = stored["h"], stored["u"]
    w = np.linspace(-1.5, 2.0, N)
    got = h.ensemble_observables([0, N], np.arange(N), w, [0], [-1])[:, :, 0]
    dot = h.ensemble_dot(w)
    gate = 2 * (N + 1) * EPS * (np.abs(u) @ np.abs(w))
    worst = np.max(np.abs(got - dot) - gate)
    print(f"largest |observable - dot| - gate: {worst!r}; largest gate {gate.max()!r}")
    assert np.all(np.abs(got - dot) <= gate)


def test_mole_fractions_sum_to_one(stored):
    """x_i = u_i / T with T the computed total, summed exactly (math.fsum) here. Each division has a relative error of at most
    2^-53; T differs from the exact total by at most (N - 1) 2^-53 sum |u_i| (every term passes through fewer than N additions,
    its product by the weight 1.0 is exact); so |sum x_i - 1| <= N 2^-53 sum |u_i| / |T| to first order, and sum |u_i| / |T| is 1
    up to the solver's tolerance for states that are concentrations: inside the gate (N + 2) 2^-53."""
    import math
    h = stored["h"]
    x = S.ensemble_observables(h, S.mole_fractions(N)).values
    assert x.shape == (K, 9, N)
    s = np.array([[math.fsum(row) for row in member] for member in x.tolist()])
    gate = (N + 2) * EPS
    print(f"largest |sum x - 1| {np.abs(s - 1.0).max()!r}, gate {gate!r}")
    assert np.all(np.abs(s - 1.0) <= gate)


def test_a_stored_record_of_observables_is_what_the_column_passes_read(stored):
    h, t, spec = stored["h"], stored["t"], stored["spec"]
    arrays, G = spec.arrays(), spec.G
    X = np.column_stack([np.array(RATES), np.cos(np.arange(K))])
    try:
        block_u, ns = _short_members(stored)                               # members of different n_saved
        before = h.ensemble_size()
        block = h.ensemble_observables(*arrays, store=True)                # pitch N by default with store
        assert block.shape == (K, len(AT), N) and not block[:, :, G:].any()
        assert block.tobytes() == h.observables_segmented(block_u, *arrays, pitch=N, seg_n=ns).tobytes()
        after = h.ensemble_size()
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3]) and h.ensemble_observable_count() == G
        full = ns == len(AT)
        mom, ref = h.ensemble_moments(), h.members_moments(block, use=full)
        assert mom["count"] == int(full.sum()) and all(ec.same_bits(mom[q], ref[q]) for q in ("mean", "var", "min", "max"))
        p, cols = [0.1, 0.5, 0.9], np.arange(G)
        assert ec.same_bits(h.ensemble_quantiles(p, species=cols), h.members_quantiles(block, p, species=cols, use=full))
        assert ec.same_bits(h.ensemble_correlate(X, species=cols), h.members_correlate(block, X, species=cols, use=full))
        ev_kw = dict(level=0.5, kind="of_peak")
        ev, ev_ref = h.ensemble_events(AT, **ev_kw), h.events_segmented(block, AT, seg_n=ns, **ev_kw)
        assert all(ec.same_bits(ev[q], ev_ref[q]) for q in ec.OUTPUTS)
        assert h.ensemble_max().tobytes() == np.array([block[m, :ns[m]].max(axis=0) if ns[m] else np.zeros(N) for m in range(K)]).tobytes()
        # the passes that need species and reactions refuse the record, and say why
        for call in (lambda: h.ensemble_flux(T_rows=np.full((K, len(AT)), 1000.0)), lambda: h.ensemble_drg(T_rows=np.full((K, len(AT)), 1000.0)),
                     lambda: h.ensemble_drgep([0], T_rows=np.full((K, len(AT)), 1000.0)), lambda: h.ensemble_pfa(T_rows=np.full((K, len(AT)), 1000.0)),
                     lambda: h.ensemble_reaction_importance(T_rows=np.full((K, len(AT)), 1000.0)),
                     lambda: h.ensemble_timescale(T_rows=np.full((K, len(AT)), 1000.0))):
            with pytest.raises(capi.KineticaHipError) as e:
                call()
            assert e.value.code == capi.KIN_ERR_STATE and "observables" in str(e.value)
        # a store that cannot be: the record stays
        for kw in (dict(pitch=G), dict(pitch=N + 1)):
            with pytest.raises(capi.KineticaHipError) as e:
                h.ensemble_observables(*arrays, store=True, **kw)
            assert e.value.code == capi.KIN_ERR_INVALID_ARG
        with pytest.raises(capi.KineticaHipError) as e:
            h.ensemble_observables([0], [], [], [], [], store=True)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG and h.ensemble_observable_count() == G
        # resampling the record keeps the mark
        at2 = np.array([925.0, 1000.0, 1100.0])
        rs = h.ensemble_resample(AT, at2, store=True)
        assert h.ensemble_observable_count() == G and h.ensemble_size()[1] == 3
        ns3 = h.ensemble_size()[3]
        assert ec.same_bits(rs, h.resample_segmented(block, AT, at2, seg_n=ns))
        block3 = rs.copy()
        for m in range(K):
            block3[m, ns3[m]:] = 0.0
        # observables of observables: the columns are numbered like species
        spec2 = S.observables(N, {"both": [0, 1], "ratio": ("ratio", "both", "f"), "f": 2})
        twice = h.ensemble_observables(*spec2.arrays(), store=True)
        assert twice.tobytes() == h.observables_segmented(block3, *spec2.arrays(), pitch=N, seg_n=ns3).tobytes()
        assert h.ensemble_observable_count() == 3 and np.array_equal(h.ensemble_size()[3], ns3)
        assert h.ensemble_observables(*S.observables(N, {"c0": 0, "c1": 1, "c2": 2}).arrays()).tobytes() == twice[:, :, :3].tobytes()
    finally:
        _restore(stored)
    # the next solve replaced the record: states again
    assert h.ensemble_observable_count() == 0 and h.ensemble_size()[1] == 9
    assert h.ensemble_flux(T_rows=stored["T"]).shape == (K, R)


def test_store_without_a_download(stored):
    h, spec = stored["h"], stored["spec"]
    try:
        r = S.ensemble_observables(h, spec, store=True, download=False)
        assert r.values is None and r.G == spec.G and h.ensemble_observable_count() == spec.G
        cols = S.observables(N, {f"c{g}": g for g in range(spec.G)})
        again = S.ensemble_observables(h, cols).values
    finally:
        _restore(stored)
    assert again.tobytes() == S.ensemble_observables(h, spec).values.tobytes()


def test_solution_observables_after_a_solve():
    net, Ea, A = synthetic_crn(N, R)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    h.set_rates(h.rates_at(1100.0))
    u0 = np.zeros(N); u0[0] = 1.0
    t, u, rcode, _, _ = h.solve(kp(1e-3, save=1e-4), u0)
    assert rcode == 0 and len(t) == 11
    spec = S.observables(N, SPEC)
    for pitch in (None, N, spec.G + 3):
        got = h.solution_observables(*spec.arrays(), pitch=pitch)
        assert got.tobytes() == h.observables_segmented(u[None], *spec.arrays(), pitch=pitch)[0].tobytes()
    r = S.solution_observables(h, SPEC)
    assert r.values.shape == (11, spec.G) and r.values.tobytes() == h.solution_observables(*spec.arrays()).tobytes()
    h.close()


def test_solve_network_ensemble_computes_observables_before_the_statistics():
    from kinetica_jl_amd import conditions as C
    net, Ea, A = synthetic_crn(N, R)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(N)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    methods = []
    for rate in RATES:
        u0 = np.zeros(N); u0[0] = 1.0; u0[3] = 0.25
        pars = S.ODESimulationParams(tspan=(0.0, T1), u0=u0, save_interval=SAVE, low_k_cutoff="none")
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=rate, X_start=900.0, X_end=1300.0)}), calc))
    named = {"light": ["S0", "S1", "S2", "S3"], "heavy": {"S7": 2.0, "S9": 0.5, "S11": -1.0}, "feed": "S0", "total": [f"S{i}" for i in range(N)],
             "x_feed": ("ratio", "feed", "total"), "sel": ("ratio", "light", "heavy"), "one": ("ratio", "total", "total"), "s5": 5}
    G = len(named)
    ev_kw = dict(level=0.5, kind="of_peak", species=[0, 4])
    stat_kw = dict(quantiles=[0.5], species=list(range(G)))
    plain = S.solve_network_ensemble(methods, sd, rd)
    assert all(o.sol.observables is None for o in plain)                   # the default: the call as it always was
    full = S.solve_network_ensemble(methods, sd, rd, observables=named, statistics=stat_kw, events=ev_kw)
    lean = S.solve_network_ensemble(methods, sd, rd, observables=named, statistics=stat_kw, events=ev_kw, trajectories=False)
    ob = full[0].sol.observables
    assert isinstance(ob, S.Observables) and all(o.sol.observables is ob for o in full) and ob.names == tuple(named) and ob.G == G
    assert all(o.sol.observables is lean[0].sol.observables for o in lean) and lean[0].sol.observables.values is None and lean[0].sol.u is None
    u = np.stack([o.sol.u for o in plain])
    t = plain[0].sol.t
    spec = S.observables(sd, named)
    assert spec.form_idx.tolist() == S.observables(N, SPEC).form_idx.tolist()
    # the explicit sequence on a handle of its own: the states handed over, the observables stored, the passes over the record
    h = capi.HipNetwork(*rd.flat(N), index_base=1)
    try:
        block = h.observables_segmented(u, *spec.arrays(1), pitch=N)
        assert ob.values.tobytes() == block[:, :, :G].tobytes()
        mom = h.members_moments(block)
        q = h.members_quantiles(block, [0.5], species=np.arange(G) + 1)
        ev = h.events_segmented(block, t, level=0.5, kind="of_peak")
    finally:
        h.close()
    for outs in (full, lean):
        st, e = outs[0].sol.ensemble_stats, outs[0].sol.events
        assert st.count == K and all(ec.same_bits(getattr(st, name), mom[name][:, :G]) for name in ("mean", "var", "min", "max"))
        assert ec.same_bits(st.quantiles, q) and st.species.tolist() == list(range(G))
        assert all(ec.same_bits(getattr(e, name), ev[name][:, [0, 4]]) for name in ec.OUTPUTS)
    for a, b in zip(full, plain):      # what refers to the solve's own rows is the plain call's
        assert a.sol.u.tobytes() == b.sol.u.tobytes() and a.sol.umax.tobytes() == b.sol.umax.tobytes()
    # no selection: the G observables, not the N columns of the record
    dflt = S.solve_network_ensemble(methods, sd, rd, observables=named, statistics=True, events=dict(level=0.5, kind="of_peak"), trajectories=False)
    st, e = dflt[0].sol.ensemble_stats, dflt[0].sol.events
    assert st.species.tolist() == list(range(G)) and st.mean.shape[1] == G and st.quantiles.shape[2] == G
    assert e.species.tolist() == list(range(G)) and all(ec.same_bits(getattr(e, name), ev[name][:, :G]) for name in ec.OUTPUTS)
    # species ids now number the observables: one past them is refused before the device
    with pytest.raises(ValueError, match="observables"):
        S.solve_network_ensemble(methods, sd, rd, observables=named, statistics=dict(species=[G]))
    with pytest.raises(ValueError):
        S.solve_network_ensemble(methods, sd, rd, observables={"a": "nope"})
