"""CPU tests of the discrete-update ensemble's interface (kin_solve_ensemble_discrete, HipNetwork.solve_ensemble_discrete,
solving.solve_network_ensemble over ts_update sets): the header and the binding agree; solve_network_ensemble hands every
member its own stops - what discrete_stop_temperatures gives for its set - and builds each member's output from the ensemble's
result as solve_network would; it refuses what it cannot run before it touches the GPU; its low-k cutoff is the intersection
of the members' cutoffs. tests/test_gpu_ensemble_discrete.py runs the solves."""
import re

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S
from oracle import oracle as orc

from tests.test_capi_symbols import HEADER


def test_header_declares_the_entry_and_the_binding_knows_it():
    text = open(HEADER).read()
    assert "kin_solve_ensemble_discrete" in capi.SYMBOLS
    assert re.search(r"int kin_solve_ensemble_discrete\(kin_network\* h, const kin_params\* params, int64_t K, const double\* u0,\s*"
                     r"const int64_t\* stop_ptr, const double\* tstops, const double\* T_stops,\s*"
                     r"int64_t\* n_rows, double\* out_t, double\* out_u, int64_t\* n_saved,\s*"
                     r"int32_t\* retcodes, kin_stats\* stats\);", text)
    assert int(re.search(r"#define KIN_ABI_VERSION (\d+)", text).group(1)) == capi.ABI_VERSION == 6
    assert hasattr(capi.HipNetwork, "solve_ensemble_discrete")


def _net():
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])   # A -> B (low barrier), A -> C (high barrier)
    return sd, rd


def _ramp(T0, T1, rate, ts_update=0.1):
    return C.ConditionSet({"T": C.LinearGradientProfile(rate=rate, X_start=T0, X_end=T1)}, ts_update=ts_update)


def _pars(u0, **kw):
    d = dict(tspan=(0.0, 1.0), u0=u0, solve_chunkstep=0.5, save_interval=0.25, low_k_cutoff="none")
    d.update(kw)
    return S.ODESimulationParams(**d)


class _Recorder:
    """Stand-in for capi.HipNetwork: records what the ensemble call hands it and answers with a canned result of the right
    shapes (5 save times, member 1 failed after 3 rows)."""
    seen = {}

    def __init__(self, *flat, index_base=1):
        self.n = flat[0]
        _Recorder.seen.clear()
        _Recorder.seen["n"] = self.n

    def set_arrhenius(self, Ea, A, k_max=None, t_mult=1.0):
        _Recorder.seen["arrhenius"] = (np.array(Ea), np.array(A), k_max, t_mult)

    def solve_ensemble_discrete(self, params, u0, stops):
        K = len(u0)
        _Recorder.seen.update(params=params, u0=np.array(u0), stops=[(np.array(a), np.array(b)) for a, b in stops])
        t = np.linspace(0.0, 1.0, 5)
        u = np.arange(K * 5 * self.n, dtype=float).reshape(K, 5, self.n) * 0.01
        ns = np.array([5] + [3] * (K - 1), np.int64)
        rcs = np.array([0] + [3] * (K - 1), np.int32)
        sts = [dict(n_steps=100 + m, final_abstol=1e-10, final_reltol=1e-8) for m in range(K)]
        _Recorder.seen["result"] = (t, u)
        return t, u, ns, rcs, sts

    def solve_ensemble_continuous(self, *a, **k):
        raise AssertionError("a discrete-update ensemble took the continuous entry")

    def close(self):
        _Recorder.seen["closed"] = True


def test_discrete_sets_with_different_heating_rates_reach_the_handle_with_their_own_stops(monkeypatch):
    monkeypatch.setattr(capi, "HipNetwork", _Recorder)
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    sd, rd = _net()
    Ea, A = [8.0e4, 2.0e5], [1.0e-17, 1.0e-17]
    calc = S.PrecalculatedArrheniusCalculator(Ea, A)
    methods = [S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), calc),     # t_end 1.0: 11 stops
               S.VariableODESolve(_pars([0.5, 0.5, 0.0]), _ramp(500.0, 600.0, 400.0), calc)]     # t_end 0.25: 4 stops
    out = S.solve_network_ensemble(methods, sd, rd)
    seen = _Recorder.seen
    assert seen["closed"] and len(out) == 2
    np.testing.assert_array_equal(seen["u0"], [[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]])
    np.testing.assert_array_equal(seen["arrhenius"][0], Ea)
    assert seen["params"].tspan1 == 1.0 and seen["params"].save_interval == 0.25
    # each member's own (tstops, T(tstops)) - what solve_network hands kin_solve for its set
    lens = []
    for m, (ts, Ts) in zip(methods, seen["stops"]):
        ts_ref, T_ref = S.discrete_stop_temperatures(m.conditions)
        np.testing.assert_array_equal(ts, ts_ref)
        np.testing.assert_array_equal(Ts, T_ref)
        lens.append(len(ts))
    assert lens[0] != lens[1] and min(lens) >= 2
    assert seen["stops"][0][1][-1] == 700.0 and seen["stops"][1][1][-1] == 600.0
    # the outputs follow from the canned result and the member's own stops, as solve_network fills them
    t, u = seen["result"]
    for i, (m, o) in enumerate(zip(methods, out)):
        n_i = 5 if i == 0 else 3
        np.testing.assert_array_equal(o.sol.t, t[:n_i])
        np.testing.assert_array_equal(o.sol.u, u[i, :n_i])
        np.testing.assert_array_equal(o.sol.umax, u[i, :n_i].max(axis=0))
        assert o.sol.retcode == ("Success" if i == 0 else "Unstable") and o.sol.stats["n_steps"] == 100 + i
        assert o.sol_vcs is None and o.sol.k is o.sol_k and o.pars is m.pars and o.conditions is m.conditions
        ts, Ts = seen["stops"][i]
        assert isinstance(o.sol_k, S.ArrheniusRates) and len(o.sol_k) == len(ts)
        np.testing.assert_array_equal(o.sol_k.t, ts)
        for s in (0, len(ts) - 1):
            np.testing.assert_array_equal(o.sol_k.u[s], orc.arrhenius(Ea, A, float(Ts[s])))
        assert np.asarray(o.sol_k.u).shape == (len(ts), 2)


def test_mixed_static_and_explicit_lists_raise_before_any_handle(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a handle was created")
    monkeypatch.setattr(capi, "HipNetwork", boom)
    sd, rd = _net()
    calc = S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17])
    disc = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), calc)
    cont = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), C.ConditionSet({"T": C.LinearGradientProfile(rate=200.0, X_start=500.0, X_end=700.0)}), calc)
    for mixed in ([disc, cont], [cont, disc]):
        with pytest.raises(ValueError, match="kin_solve_ensemble"):
            S.solve_network_ensemble(mixed, sd, rd)
    stat = S.StaticODESolve(_pars([1.0, 0.0, 0.0]), C.ConditionSet({"T": 600.0}), calc)
    with pytest.raises(ValueError, match="solve_network"):
        S.solve_network_ensemble([disc, stat], sd, rd)
    dummy = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), S.DummyKineticCalculator([1.0, 2.0]))
    with pytest.raises(ValueError, match="Arrhenius"):
        S.solve_network_ensemble([disc, dummy], sd, rd)
    expl = S.VariableODESolve(_pars([0.5, 0.0, 0.0], solver="RK45"), _ramp(500.0, 600.0, 100.0), calc)
    with pytest.raises(ValueError, match="BDF"):
        S.solve_network_ensemble([expl], sd, rd)
    with pytest.raises(ValueError, match="BDF"):
        S.solve_network_ensemble([S.VariableODESolve(_pars([1.0, 0.0, 0.0], solver="RK45"), _ramp(500.0, 700.0, 200.0), calc),
                                  S.VariableODESolve(_pars([0.5, 0.0, 0.0], solver="RK45"), _ramp(500.0, 600.0, 100.0), calc)], sd, rd)
    # discrete sets that agree pass the checks and reach the handle (refused here by the stand-in)
    with pytest.raises(AssertionError, match="handle"):
        S.solve_network_ensemble([disc, S.VariableODESolve(_pars([0.5, 0.5, 0.0]), _ramp(500.0, 600.0, 100.0), calc)], sd, rd)


def test_union_low_k_cutoff_over_discrete_sets_keeps_a_reaction_only_one_member_needs(monkeypatch):
    """A -> C has a high barrier: a cold member's cutoff removes it, a hot member's keeps it. The ensemble keeps it; with two
    cold members it goes, exactly as apply_low_k_cutoff removes it for each of them."""
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    Ea, A = [8.0e4, 3.0e5], [1.0e-17, 1.0e-17]
    pars = _pars([1.0, 0.0, 0.0], low_k_cutoff="auto")
    cold, hot = _ramp(500.0, 600.0, 100.0), _ramp(500.0, 1500.0, 1000.0, ts_update=0.05)
    k_cold, k_hot = orc.arrhenius(Ea, A, 600.0)[1], orc.arrhenius(Ea, A, 1500.0)[1]
    cut = pars.reltol / pars.tspan[-1] / pars.low_k_maxconc ** 2
    assert k_cold < cut < k_hot                  # the case is what it claims to be
    for sets, kept in (([cold, hot], 2), ([hot, cold], 2), ([cold, cold], 1), ([hot], 2)):
        sd, rd = _net()
        calc = S.PrecalculatedArrheniusCalculator(Ea, A)
        for cs in sets:
            C.solve_variable_conditions(cs, pars, reset=True)
            assert cs.discrete_updates
        removed = S.apply_ensemble_low_k_cutoff(rd, calc, pars, sets)
        assert rd.nr == kept and len(calc.Ea) == kept and len(removed) == 2 - kept
        if len(sets) == 1 or sets[0] is sets[1]:
            sd2, rd2 = _net()
            calc2 = S.PrecalculatedArrheniusCalculator(Ea, A)
            S.apply_low_k_cutoff(rd2, calc2, pars, sets[0])
            assert rd2.nr == rd.nr and np.array_equal(calc2.Ea, calc.Ea)
