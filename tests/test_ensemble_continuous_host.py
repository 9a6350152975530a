"""CPU tests of the continuous-rate ensemble's interface (kin_solve_ensemble_continuous, HipNetwork.solve_ensemble_continuous,
solving.solve_network_ensemble): the header and the binding agree, solve_network_ensemble refuses what it cannot run before
it touches the GPU, and its low-k cutoff is the intersection of the members' cutoffs. tests/test_gpu_ensemble_continuous.py
runs the solves."""
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
    assert "kin_solve_ensemble_continuous" in capi.SYMBOLS
    assert re.search(r"int kin_solve_ensemble_continuous\(kin_network\* h, const kin_params\* params, int64_t K, const double\* u0,\s*"
                     r"const int64_t\* node_ptr, const double\* t_nodes, const double\* T_nodes,", text)
    assert int(re.search(r"#define KIN_ABI_VERSION (\d+)", text).group(1)) == capi.ABI_VERSION == 6
    assert "solve_network_ensemble" in S.__all__


def _net():
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])   # A -> B (low barrier), A -> C (high barrier)
    return sd, rd


def _ramp(T0, T1, rate):
    return C.ConditionSet({"T": C.LinearGradientProfile(rate=rate, X_start=T0, X_end=T1)})


def _pars(u0, **kw):
    d = dict(tspan=(0.0, 1.0), u0=u0, solve_chunkstep=0.5, save_interval=0.25, low_k_cutoff="none")
    d.update(kw)
    return S.ODESimulationParams(**d)


def _fail_on_handle(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a handle was created")
    monkeypatch.setattr(capi, "HipNetwork", boom)


def test_mismatched_methods_raise_before_any_handle(monkeypatch):
    _fail_on_handle(monkeypatch)
    sd, rd = _net()
    calc = S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17])
    ok = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), calc)
    # pars differing in a field other than u0
    bad_p = S.VariableODESolve(_pars([1.0, 0.0, 0.0], reltol=1e-6), _ramp(500.0, 600.0, 100.0), calc)
    with pytest.raises(ValueError, match="reltol"):
        S.solve_network_ensemble([ok, bad_p], sd, rd)
    # another calculator
    other = S.PrecalculatedArrheniusCalculator([8.0e4, 2.1e5], [1.0e-17, 1.0e-17])
    with pytest.raises(ValueError, match="calculator"):
        S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.0, 0.0]), _ramp(500.0, 600.0, 100.0), other)], sd, rd)
    # another filter
    filt = S.RxFilter([lambda sd_, rd_: [True, False]])
    with pytest.raises(ValueError, match="filter"):
        S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.0, 0.0]), _ramp(500.0, 600.0, 100.0), calc, filt)], sd, rd)
    # a discrete-update set, a static solve, a non-Arrhenius calculator: the other entry points
    disc = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), C.ConditionSet({"T": C.LinearGradientProfile(rate=200.0, X_start=500.0, X_end=700.0)},
                                                                     ts_update=0.1), calc)
    with pytest.raises(ValueError, match="kin_solve_ensemble"):
        S.solve_network_ensemble([ok, disc], sd, rd)
    stat = S.StaticODESolve(_pars([1.0, 0.0, 0.0]), C.ConditionSet({"T": 600.0}), calc)
    with pytest.raises(ValueError, match="solve_network"):
        S.solve_network_ensemble([stat], sd, rd)
    dummy = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), S.DummyKineticCalculator([1.0, 2.0]))
    with pytest.raises(ValueError, match="Arrhenius"):
        S.solve_network_ensemble([dummy], sd, rd)
    with pytest.raises(ValueError):
        S.solve_network_ensemble([], sd, rd)
    # methods that agree pass the checks and reach the handle (refused here by the stand-in)
    with pytest.raises(AssertionError, match="handle"):
        S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.5, 0.0]), _ramp(500.0, 600.0, 100.0), calc)], sd, rd)


def test_union_low_k_cutoff_keeps_a_reaction_only_one_member_needs(monkeypatch):
    """A -> C has a high barrier: a cold member's cutoff removes it, a hot member's keeps it. The ensemble keeps it; with two
    cold members it goes, exactly as apply_low_k_cutoff removes it for each of them."""
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    Ea, A = [8.0e4, 3.0e5], [1.0e-17, 1.0e-17]
    pars = _pars([1.0, 0.0, 0.0], low_k_cutoff="auto")
    cold, hot = _ramp(500.0, 600.0, 100.0), _ramp(500.0, 1500.0, 1000.0)
    k_cold, k_hot = orc.arrhenius(Ea, A, 600.0)[1], orc.arrhenius(Ea, A, 1500.0)[1]
    cut = pars.reltol / pars.tspan[-1] / pars.low_k_maxconc ** 2
    assert k_cold < cut < k_hot                  # the case is what it claims to be
    for sets, kept in (([cold, hot], 2), ([hot, cold], 2), ([cold, cold], 1), ([hot], 2)):
        sd, rd = _net()
        calc = S.PrecalculatedArrheniusCalculator(Ea, A)
        for cs in sets:
            C.solve_variable_conditions(cs, pars, reset=True)
        removed = S.apply_ensemble_low_k_cutoff(rd, calc, pars, sets)
        assert rd.nr == kept and len(calc.Ea) == kept and len(removed) == 2 - kept
        if len(sets) == 1 or sets[0] is sets[1]:
            sd2, rd2 = _net()
            calc2 = S.PrecalculatedArrheniusCalculator(Ea, A)
            S.apply_low_k_cutoff(rd2, calc2, pars, sets[0])
            assert rd2.nr == rd.nr and np.array_equal(calc2.Ea, calc.Ea)


def test_every_members_calculator_is_spliced(monkeypatch):
    """Members with distinct but equal calculator objects: the cutoff splices each of them, as each member's own solve_network
    would (the solve itself is refused here by a stand-in for the handle)."""
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    _fail_on_handle(monkeypatch)
    Ea, A = [8.0e4, 3.0e5], [1.0e-17, 1.0e-17]
    calcs = [S.PrecalculatedArrheniusCalculator(Ea, A) for _ in range(3)]
    methods = [S.VariableODESolve(_pars([1.0, 0.0, 0.0], low_k_cutoff="auto"), _ramp(500.0, 600.0, 100.0), c) for c in calcs]
    methods.append(S.VariableODESolve(_pars([0.5, 0.0, 0.0], low_k_cutoff="auto"), _ramp(500.0, 600.0, 100.0), calcs[1]))
    sd, rd = _net()
    with pytest.raises(AssertionError, match="handle"):
        S.solve_network_ensemble(methods, sd, rd)
    for c in calcs:                                  # A -> C is below every member's cutoff: gone from each object, once
        np.testing.assert_array_equal(c.Ea, [8.0e4])
    assert rd.nr == 2                                # copy_network: the caller's network is untouched
