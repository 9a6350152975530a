"""Host-side tests (no device) of the six analysis functions of `solving` that run one pass over the saved states of a solve:
reaction_fluxes, drg_coefficients, pfa_coefficients, drgep_importance, reaction_importance and species_timescales. A stand-in
for capi.HipNetwork records how the handle is built, whether set_arrhenius is called, the method called with its arguments,
and close() - for a static solve, discrete-update solves with the Arrhenius calculator (temperatures at the stops, or a table
of rows) and with a Dummy calculator, and a continuous solve."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S

T_SAVED = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
U_SAVED = np.arange(15.0).reshape(5, 3) / 16.0
EA, A_PRE = np.array([8.0e4, 9.0e4]), np.array([1.0e-17, 3.0e-17])
K_300 = np.array([0.125, 4.0])                          # what the stand-in for kin_arrhenius_eval gives
T_STOPS, TEMPS = np.array([0.0, 0.3, 0.6, 0.9]), np.array([500.0, 530.0, 560.0, 590.0])
HELD = np.array([0, 0, 1, 2, 3])                        # held_stop_index(T_SAVED, T_STOPS)
K_STOPS = np.arange(8.0).reshape(4, 2) + 1.0
T_CONT = np.array([500.0, 525.0, 550.0, 575.0, 600.0])
E, E2 = 3, 5                                            # edges / pairs of the stand-in's patterns


class _Recorder:
    """Stands in for capi.HipNetwork: records the construction, set_arrhenius, the one method called and close()."""
    made = []
    fail = False

    class Boom(Exception):
        pass

    def __init__(self, *a, **kw):
        self.init, self.set, self.calls, self.closed = (a, kw), None, [], 0
        _Recorder.made.append(self)

    def set_arrhenius(self, Ea, A, k_max=None, t_mult=1.0):
        assert self.set is None and not self.calls      # (once, and before the pass)
        self.set = (np.array(Ea), np.array(A), k_max, t_mult)

    def close(self):
        self.closed += 1

    def _call(self, name, a, kw, result):
        assert not self.closed
        self.calls.append((name, a, kw))
        if _Recorder.fail:
            raise _Recorder.Boom()
        return result

    def flux_batched(self, *a, **kw):
        flux = np.array([2.0, 0.5])
        return self._call("flux_batched", a, kw, (flux, np.ones((len(a[0]), 2))) if kw.get("want_rates") else flux)

    def drg_pattern(self, *a, **kw):
        return self._call("drg_pattern", a, kw, (np.array([0, 1, 2, E]), np.array([1, 2, 0])))

    def pfa_pattern(self, *a, **kw):
        return self._call("pfa_pattern", a, kw, (np.array([0, 2, 3, E2]), np.array([1, 2, 2, 0, 1])))

    def drg_batched(self, *a, **kw):
        return self._call("drg_batched", a, kw, np.arange(float(E)))

    def pfa_batched(self, *a, **kw):
        return self._call("pfa_batched", a, kw, np.arange(float(E2)))

    def drgep_batched(self, *a, **kw):
        return self._call("drgep_batched", a, kw, np.array([1.0, 0.5, 0.25]))

    def reaction_importance_batched(self, *a, **kw):
        return self._call("reaction_importance_batched", a, kw, np.array([1.0, 0.125]))

    def timescale_batched(self, *a, **kw):
        n = len(a[0])
        return self._call("timescale_batched", a, kw, dict(summary=np.arange(9.0).reshape(3, 3), norm=np.arange(float(n))))


@pytest.fixture
def rec(monkeypatch):
    _Recorder.made.clear()
    monkeypatch.setattr(_Recorder, "fail", False)
    monkeypatch.setattr(capi, "HipNetwork", _Recorder)
    monkeypatch.setattr(capi, "arrhenius_eval", lambda Ea, A, T, k_max=None, t_mult=1.0: K_300.copy())
    return _Recorder


def _net():
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])   # A -> B, A -> C
    return sd, rd


def _arrhenius():
    return S.PrecalculatedArrheniusCalculator(EA, A_PRE, k_max=1e9, t_unit="ms")


def _out(kind):
    """(ODESolveOutput, calculator, the rate-constant keywords the pass must get, whether T is the source)."""
    sd, rd = _net()
    pars = S.ODESimulationParams(tspan=(0.0, 1.0), u0=[1.0, 0.0, 0.0], solve_chunkstep=0.5)
    sol = S.ODESolution(T_SAVED.copy(), U_SAVED.copy(), "Success")
    ramp = C.LinearGradientProfile(rate=100.0, X_start=500.0, X_end=600.0)
    calc, sol_k, sol_vcs = _arrhenius(), None, None
    if kind == "static":
        conds, src = C.ConditionSet({"T": 300.0}), dict(k=K_300[None, :], k_row=np.zeros(5, np.int64))
    elif kind == "discrete-arrhenius":
        conds, src = C.ConditionSet({"T": ramp}, ts_update=0.3), dict(T=TEMPS[HELD])
        sol_k = S.ArrheniusRates(T_STOPS, TEMPS, EA, A_PRE, 1e9, calc.t_mult)
    elif kind == "discrete-table":
        conds, src = C.ConditionSet({"T": ramp}, ts_update=0.3), dict(k=K_STOPS, k_row=HELD)
        sol_k = S.DiscreteRates(T_STOPS, K_STOPS.copy())
    elif kind == "discrete-dummy":
        calc = S.DummyKineticCalculator([3.0, 5.0])
        conds, src = C.ConditionSet({"T": ramp}, ts_update=0.3), dict(k=np.array([[3.0, 5.0]]), k_row=np.zeros(5, np.int64))
        sol_k = S.DiscreteRates(T_STOPS, np.tile([3.0, 5.0], (4, 1)))
    elif kind == "continuous":
        conds, src = C.ConditionSet({"T": ramp}), dict(T=T_CONT)
        sol_vcs = {"T": T_CONT.copy()}
    return S.ODESolveOutput(sd, rd, sol, sol_k, sol_vcs, pars, conds), calc, src, "T" in src


KINDS = ["static", "discrete-arrhenius", "discrete-table", "discrete-dummy", "continuous"]
# function, its own arguments, the methods called in order with their positional arguments after u and their own keywords
PASSES = {
    "reaction_fluxes": (S.reaction_fluxes, dict(weights=None, rates=True), [("flux_batched", (), dict(w=np.ones(5), want_rates=True))]),
    "drg_coefficients": (S.drg_coefficients, dict(pairing=False), [("drg_pattern", None, {}), ("drg_batched", (), dict(pairing=False))]),
    "pfa_coefficients": (S.pfa_coefficients, dict(pairing=False), [("pfa_pattern", None, {}), ("pfa_batched", (), dict(pairing=False))]),
    "drgep_importance": (S.drgep_importance, dict(targets=["C", 0], pairing=False, importance=np.array([0.5, 0.0, 1.0])),
                         [("drgep_batched", ([2, 0],), dict(pairing=False, importance=np.array([0.5, 0.0, 1.0])))]),
    "reaction_importance": (S.reaction_importance, dict(species=["B", 2], pairing=False, importance=np.array([0.25, 0.0])),
                            [("reaction_importance_batched", (), dict(species=[1, 2], pairing=False, importance=np.array([0.25, 0.0])))]),
    "species_timescales": (S.species_timescales, {}, [("timescale_batched", (), dict(summary=None))]),
}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[q], b[q]) for q in a)
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _check_handle(hd, calc, uses_T):
    sd, rd = _net()
    a, kw = hd.init
    assert kw == {"index_base": 1} and len(a) == 7 and a[0] == sd.n
    for x, y in zip(a[1:], rd.flat(sd.n)[1:]):
        np.testing.assert_array_equal(x, y)
    if uses_T:
        assert hd.set is not None and hd.set[2:] == (calc.k_max, calc.t_mult) == (1e9, 1e-3)
        np.testing.assert_array_equal(hd.set[0], EA)
        np.testing.assert_array_equal(hd.set[1], A_PRE)
    else:
        assert hd.set is None
    assert hd.closed == 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(PASSES))
def test_the_pass_gets_the_states_and_the_rate_constants_the_solve_held(rec, name, kind):
    fn, own, expected = PASSES[name]
    out, calc, src, uses_T = _out(kind)
    fn(out, calc, **own)
    (hd,) = rec.made
    _check_handle(hd, calc, uses_T)
    assert [c[0] for c in hd.calls] == [e[0] for e in expected]
    for (_, a, kw), (_, more, own_kw) in zip(hd.calls, expected):
        if more is None:            # the pattern query: the pairing alone, however it is passed
            assert (a, kw) in (((False,), {}), ((), {"pairing": False}))
            continue
        np.testing.assert_array_equal(a[0], U_SAVED)
        assert a[0].flags.c_contiguous and a[0].dtype == np.float64
        assert len(a) == 1 + len(more) and all(_same(x, y) for x, y in zip(a[1:], more))
        assert _same(kw, dict(own_kw, **src)), (kw, src)


@pytest.mark.parametrize("name", list(PASSES))
def test_the_handle_is_closed_once_when_the_pass_raises(rec, monkeypatch, name):
    fn, own, _ = PASSES[name]
    monkeypatch.setattr(_Recorder, "fail", True)
    out, calc, _, _ = _out("continuous")
    with pytest.raises(_Recorder.Boom):
        fn(out, calc, **own)
    (hd,) = rec.made
    assert hd.closed == 1 and len(hd.calls) == 1 and hd.set is not None


@pytest.mark.parametrize("name", list(PASSES))
def test_a_calculator_of_another_length_is_refused_before_any_handle(rec, name):
    fn, own, _ = PASSES[name]
    out, _, _, _ = _out("static")
    with pytest.raises(ValueError, match="does not match number of reactions"):
        fn(out, S.DummyKineticCalculator([1.0, 2.0, 3.0]), **own)
    assert rec.made == []


def test_results_are_what_the_methods_returned(rec):
    out, calc, _, _ = _out("continuous")
    rf = S.reaction_fluxes(out, calc, rates=True)
    np.testing.assert_array_equal(rf.flux, [2.0, 0.5])
    np.testing.assert_array_equal(rf.weights, S.flux_weights(T_SAVED))
    np.testing.assert_array_equal(rec.made[-1].calls[0][2]["w"], S.flux_weights(T_SAVED))
    assert rf.rates.shape == (5, 2) and S.reaction_fluxes(out, calc).rates is None
    np.testing.assert_array_equal(rf.production, [0.0, 2.0, 0.5])
    w = np.arange(5.0)
    np.testing.assert_array_equal(S.reaction_fluxes(out, calc, weights=w).weights, w)
    for fn, pattern, nnz in ((S.drg_coefficients, ([0, 1, 2, E], [1, 2, 0]), E), (S.pfa_coefficients, ([0, 2, 3, E2], [1, 2, 2, 0, 1]), E2)):
        rowptr, colidx, coef = fn(out, calc)
        np.testing.assert_array_equal(rowptr, pattern[0])
        np.testing.assert_array_equal(colidx, pattern[1])
        np.testing.assert_array_equal(coef, np.arange(float(nnz)))
        assert rec.made[-1].calls[-1][2]["pairing"] is True
    np.testing.assert_array_equal(S.drgep_importance(out, calc, [1]), [1.0, 0.5, 0.25])
    np.testing.assert_array_equal(S.reaction_importance(out, calc), [1.0, 0.125])
    assert rec.made[-1].calls[0][2]["species"] is None
    ts = S.species_timescales(out, calc)
    np.testing.assert_array_equal(ts.t, T_SAVED)
    np.testing.assert_array_equal(ts.summary, np.arange(9.0).reshape(3, 3))
    np.testing.assert_array_equal(ts.norm, np.arange(5.0))
    with pytest.raises(ValueError, match="weights must have one entry per saved time"):
        S.reaction_fluxes(out, calc, weights=np.ones(4))
    with pytest.raises(ValueError, match='weights must be "trapezoid", None or an array'):
        S.reaction_fluxes(out, calc, weights="simpson")
    assert all(hd.closed == 1 for hd in rec.made)


@pytest.mark.parametrize("kind", KINDS)
def test_t_min_masks_states_sources_and_times_alike(rec, kind):
    out, calc, src, uses_T = _out(kind)
    earlier = S.Timescales(T_SAVED, np.ones(3), np.zeros(3), 2.0 * np.ones(3), np.ones(5))
    ts = S.species_timescales(out, calc, t_min=0.5, summary=earlier)
    keep = slice(2, 5)
    (hd,) = rec.made
    _check_handle(hd, calc, uses_T)
    ((name, a, kw),) = hd.calls
    assert name == "timescale_batched" and len(a) == 1
    np.testing.assert_array_equal(a[0], U_SAVED[keep])
    assert a[0].flags.c_contiguous
    want = dict(src, summary=earlier.summary)
    for q in ("k_row", "T"):          # one entry per saved time; k holds the rows k_row indexes and stays whole
        if q in want:
            want[q] = want[q][keep]
    assert _same(kw, want), (kw, want)
    np.testing.assert_array_equal(ts.t, T_SAVED[keep])
    np.testing.assert_array_equal(ts.norm, np.arange(3.0))
    # a t_min past the end: no state counts, and the call is still made
    ts = S.species_timescales(out, calc, t_min=2.0)
    assert len(ts.t) == 0 and rec.made[-1].calls[0][1][0].shape == (0, 3) and rec.made[-1].closed == 1
