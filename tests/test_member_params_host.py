"""Host-side tests of per-member Arrhenius parameters in ensembles (no device): the two new symbols and their binding,
solving.sample_arrhenius, and solve_network_ensemble(member_calculators=True)'s checks of calculators that differ - refused for
what the handle holds once (k_max, t_mult, length), accepted for values, and still the shared call for calculators equal in
value; without the flag, calculators that differ in value are refused as before."""
import ctypes
import os

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S
from oracle import oracle as orc

NEW_SYMBOLS = ["kin_solve_ensemble_continuous_params", "kin_solve_ensemble_discrete_params"]


def test_symbols_are_exported_and_bound():
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    for name in NEW_SYMBOLS:
        fn = getattr(capi.lib(), name)
        old = getattr(capi.lib(), name[:-len("_params")])
        # the existing entry's arguments with Ea, A between u0 and the pointer array
        assert fn.argtypes is not None and len(fn.argtypes) == len(old.argtypes) + 2
        assert list(fn.argtypes[:4]) == list(old.argtypes[:4]) and list(fn.argtypes[6:]) == list(old.argtypes[4:])
        assert fn.argtypes[4] is fn.argtypes[5] is ctypes.POINTER(ctypes.c_double)
    assert capi.lib().kin_abi_version() == capi.ABI_VERSION == 6


def test_sample_arrhenius_maps_the_rows_as_documented():
    Ea = np.array([8.0e4, 9.0e4, 1.0e5, 1.1e5, 1.2e5])
    A = np.array([1e-17, 2e-17, 3e-17, 4e-17, 5e-17])
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e9, t_unit="s")
    X = np.array([[0.5, 0.5, 0.5], [0.0, 1.0, 0.25], [1.0, 0.0, 0.9], [0.75, 0.5, 0.0]])
    spec = [("Ea", [0, 3], 4e3), ("lnA", [1, 3], 2.0), ("Ea", [], 5e3)]
    out = S.sample_arrhenius(calc, X, spec)
    assert len(out) == 4 and all(isinstance(c, S.PrecalculatedArrheniusCalculator) for c in out)
    assert len({id(c) for c in out}) == 4 and all(c is not calc for c in out)
    for c, x in zip(out, X):
        e, a = Ea.copy(), A.copy()
        e[[0, 3]] += 4e3 * (2.0 * x[0] - 1.0)
        a[[1, 3]] *= np.exp(2.0 * (2.0 * x[1] - 1.0))
        np.testing.assert_array_equal(c.Ea, e)
        np.testing.assert_array_equal(c.A, a)
        assert c.k_max == 1e9 and c.t_mult == calc.t_mult
    # the centre of the cube leaves the calculator's values; the dummy column moves nothing
    np.testing.assert_array_equal(out[0].Ea, Ea)
    np.testing.assert_array_equal(out[0].A, A)
    same_but_dummy = S.sample_arrhenius(calc, np.array([[0.3, 0.6, 0.0], [0.3, 0.6, 1.0]]), spec)
    np.testing.assert_array_equal(same_but_dummy[0].Ea, same_but_dummy[1].Ea)
    np.testing.assert_array_equal(same_but_dummy[0].A, same_but_dummy[1].A)
    # calc untouched, and no array shared with it
    np.testing.assert_array_equal(calc.Ea, Ea)
    np.testing.assert_array_equal(calc.A, A)
    out[1].Ea[0] = 0.0
    assert calc.Ea[0] == 8.0e4
    # a Saltelli design: one calculator per row
    Xs = S.sobol_design(4, 3, seed=2)
    assert len(S.sample_arrhenius(calc, Xs, spec)) == 4 * 5
    for bad_X, bad_spec in ((X[:, :2], spec), (X + 1.0, spec), (X, [("k", [0], 1.0)] * 3), (X, [("Ea", [5], 1.0)] * 3),
                            (X, [("Ea", [-1], 1.0)] * 3), (X, [("Ea", [0])] * 3)):
        with pytest.raises(ValueError):
            S.sample_arrhenius(calc, bad_X, bad_spec)
    with pytest.raises(ValueError):
        S.sample_arrhenius(S.DummyKineticCalculator([1.0] * 5), X, spec)
    assert "sample_arrhenius" in S.__all__ and "sample_arrhenius" in S.sobol_design.__doc__


def _net():
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])   # A -> B, A -> C
    return sd, rd


def _ramp(T0, T1, rate, **kw):
    return C.ConditionSet({"T": C.LinearGradientProfile(rate=rate, X_start=T0, X_end=T1)}, **kw)


def _pars(u0, **kw):
    d = dict(tspan=(0.0, 1.0), u0=u0, solve_chunkstep=0.5, save_interval=0.25, low_k_cutoff="none")
    d.update(kw)
    return S.ODESimulationParams(**d)


class _Recorder:
    """Stands in for capi.HipNetwork: records what solve_network_ensemble hands to the ensemble call and stops there."""
    calls = []

    class Stop(Exception):
        pass

    def __init__(self, *a, **k):
        pass

    def set_arrhenius(self, Ea, A, k_max=None, t_mult=1.0):
        self.set = (np.array(Ea), np.array(A), k_max, t_mult)

    def _record(self, name, params, u0, pairs, **kw):
        _Recorder.calls.append((name, self.set, kw))
        raise _Recorder.Stop()

    def solve_ensemble_continuous(self, params, u0, nodes, **kw):
        self._record("continuous", params, u0, nodes, **kw)

    def solve_ensemble_discrete(self, params, u0, stops, **kw):
        self._record("discrete", params, u0, stops, **kw)

    def close(self):
        pass


def test_differing_k_max_t_mult_or_length_raise_before_any_handle(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a handle was created")
    monkeypatch.setattr(capi, "HipNetwork", boom)
    sd, rd = _net()
    calc = S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17], k_max=1e9)
    ok = S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0), calc)
    for other, word in ((S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17], k_max=1e8), "k_max"),
                        (S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17]), "k_max"),
                        (S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5], [1.0e-17, 1.0e-17], k_max=1e9, t_unit="ms"), "t_mult"),
                        (S.PrecalculatedArrheniusCalculator([8.0e4, 2.0e5, 1.0e5], [1.0e-17] * 3, k_max=1e9), "length")):
        with pytest.raises(ValueError, match=word):
            S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.0, 0.0]), _ramp(500.0, 600.0, 100.0), other)], sd, rd,
                                     member_calculators=True)
    # values alone may differ: the checks pass and the handle is reached (refused here by the stand-in)
    other = S.PrecalculatedArrheniusCalculator([8.0e4, 2.1e5], [1.0e-17, 3.0e-17], k_max=1e9)
    with pytest.raises(AssertionError, match="handle"):
        S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.0, 0.0]), _ramp(500.0, 600.0, 100.0), other)], sd, rd,
                                 member_calculators=True)
    # ... when asked for: without member_calculators the refusal of before stands, and names the flag
    with pytest.raises(ValueError, match="member_calculators"):
        S.solve_network_ensemble([ok, S.VariableODESolve(_pars([0.5, 0.0, 0.0]), _ramp(500.0, 600.0, 100.0), other)], sd, rd)


@pytest.mark.parametrize("discrete", [False, True])
def test_equal_calculators_take_the_shared_call_and_differing_ones_hand_over_their_rows(monkeypatch, discrete):
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    monkeypatch.setattr(capi, "HipNetwork", _Recorder)
    kw = dict(ts_update=0.1) if discrete else {}
    Ea, A = [8.0e4, 9.0e4], [1.0e-17, 1.0e-17]

    def run(calcs):
        _Recorder.calls.clear()
        sd, rd = _net()
        methods = [S.VariableODESolve(_pars([1.0, 0.0, 0.0]), _ramp(500.0, 700.0, 200.0, **kw), c) for c in calcs]
        with pytest.raises(_Recorder.Stop):
            S.solve_network_ensemble(methods, sd, rd, member_calculators=True)
        assert len(_Recorder.calls) == 1
        return _Recorder.calls[0]
    # distinct objects, equal values: exactly the call made before - no Ea / A passed
    name, handle_set, passed = run([S.PrecalculatedArrheniusCalculator(Ea, A) for _ in range(3)])
    assert name == ("discrete" if discrete else "continuous") and passed == {}
    # values differ: every member's rows, in the order of the methods; the handle holds the first method's
    calcs = [S.PrecalculatedArrheniusCalculator(Ea, A), S.PrecalculatedArrheniusCalculator([8.1e4, 9.0e4], A),
             S.PrecalculatedArrheniusCalculator(Ea, [2.0e-17, 1.0e-17])]
    name, handle_set, passed = run(calcs)
    assert sorted(passed) == ["A", "Ea"]
    np.testing.assert_array_equal(passed["Ea"], [c.Ea for c in calcs])
    np.testing.assert_array_equal(passed["A"], [c.A for c in calcs])
    np.testing.assert_array_equal(handle_set[0], calcs[0].Ea)


def test_low_k_cutoff_uses_each_members_own_calculator(monkeypatch):
    """A -> C is below the cutoff with the high barrier and above it with the low one: the ensemble keeps it as long as one
    member's own calculator keeps it; every distinct calculator object is spliced once."""
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: orc.arrhenius(Ea, A, T, k_max=k_max, t_mult=t_mult))
    monkeypatch.setattr(capi, "HipNetwork", _Recorder)
    A = [1.0e-17, 1.0e-17]
    pars = _pars([1.0, 0.0, 0.0], low_k_cutoff="auto")
    cut = pars.reltol / pars.tspan[-1] / pars.low_k_maxconc ** 2
    assert orc.arrhenius([3.0e5], [1e-17], 600.0)[0] < cut < orc.arrhenius([1.5e5], [1e-17], 600.0)[0]
    for barriers, kept in (([3.0e5, 3.0e5], 1), ([3.0e5, 1.5e5], 2), ([1.5e5, 3.0e5], 2)):
        _Recorder.calls.clear()
        calcs = [S.PrecalculatedArrheniusCalculator([8.0e4, b], A) for b in barriers]
        methods = [S.VariableODESolve(_pars([1.0, 0.0, 0.0], low_k_cutoff="auto"), _ramp(500.0, 600.0, 100.0), c) for c in calcs]
        methods.append(S.VariableODESolve(_pars([0.5, 0.0, 0.0], low_k_cutoff="auto"), _ramp(500.0, 600.0, 100.0), calcs[1]))
        sd, rd = _net()
        with pytest.raises(_Recorder.Stop):
            S.solve_network_ensemble(methods, sd, rd, member_calculators=True)
        for c in calcs:
            assert len(c.Ea) == kept and len(c.A) == kept
        passed = _Recorder.calls[0][2]
        if barriers[0] == barriers[1]:
            assert passed == {}          # equal in value: the shared call
        else:
            assert passed["Ea"].shape == (3, kept) and np.array_equal(passed["Ea"][2], passed["Ea"][1])
