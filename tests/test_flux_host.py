"""Host-side tests of the reaction-flux analysis (no device): flux_weights, held_stop_index, the gross production /
consumption of ReactionFluxes, the exported symbols and the calculator check of reaction_fluxes."""
import ctypes
import json
import os

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLUX_SYMBOLS = ["kin_flux_batched", "kin_flux_batched_dev", "kin_solution_flux"]


def test_flux_weights_uniform_and_non_uniform():
    np.testing.assert_array_equal(S.flux_weights([0.0, 1.0, 2.0, 3.0]), [0.5, 1.0, 1.0, 0.5])
    t = np.array([0.0, 0.25, 1.0, 3.0])
    w = S.flux_weights(t)
    np.testing.assert_array_equal(w, [0.125, 0.5, 1.375, 1.0])
    assert w.sum() == t[-1] - t[0]
    # the trapezoid rule is exact for a linear integrand
    assert w @ (2.0 * t + 1.0) == pytest.approx(3.0 ** 2 + 3.0, rel=1e-15)
    rng = np.random.default_rng(0)
    t = np.cumsum(rng.uniform(0.1, 1.0, 50))
    assert S.flux_weights(t).sum() == pytest.approx(t[-1] - t[0], rel=1e-14)


def test_flux_weights_one_and_two_rows():
    np.testing.assert_array_equal(S.flux_weights([0.7]), [0.0])
    np.testing.assert_array_equal(S.flux_weights([1.0, 1.5]), [0.25, 0.25])


@pytest.mark.parametrize("t", [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], []])
def test_flux_weights_rejects_non_increasing_times(t):
    with pytest.raises(ValueError):
        S.flux_weights(t)


def test_held_stop_index():
    tstops = np.array([1.0, 2.0, 3.0])
    t = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.999, 3.0, 7.0])
    #              before the first stop: 0 | at a stop: that stop | after the last: the last
    np.testing.assert_array_equal(S.held_stop_index(t, tstops), [0, 0, 0, 0, 1, 1, 2, 2])
    assert S.held_stop_index(t, tstops).dtype == np.int64
    np.testing.assert_array_equal(S.held_stop_index([0.0, 0.1], [0.0]), [0, 0])


def test_production_and_consumption_on_the_doc_crn():
    d = json.load(open(os.path.join(GOLDEN, "doc_crn.json")))
    # A -> B + C, B + C -> A, B -> D, D -> B, C + D -> E, E -> C + D (per reaction [[species, stoichiometry], ...], 0-based)
    side = lambda L, j: [[int(e[j]) + (1 - j) for e in r] for r in L]
    rd = S.RxData(len(d["reacs"]), side(d["reacs"], 0), side(d["prods"], 0), side(d["reacs"], 1), side(d["prods"], 1))
    assert d["species"] == ["A", "B", "C", "D", "E"] and rd.nr == 6
    f = np.array([1.0, 0.5, 4.0, 0.25, 8.0, 0.125])
    rf = S.ReactionFluxes.from_flux(f, rd, 5, np.ones(3))
    np.testing.assert_array_equal(rf.production, [f[1], f[0] + f[3], f[0] + f[5], f[2] + f[5], f[4]])
    np.testing.assert_array_equal(rf.consumption, [f[0], f[1] + f[2], f[1] + f[4], f[3] + f[4], f[5]])
    np.testing.assert_array_equal(rf.top(2), [4, 2])
    assert rf.rates is None and np.array_equal(rf.flux, f)


def test_hand_built_gross_rates_and_top():
    # 2A -> B, A -> 2B, A + M -> B + M (collider: M is produced and consumed), B -> A + B
    rd = S.RxData(4, [[1], [1], [1, 3], [2]], [[2], [2], [2, 3], [1, 2]], [[2], [1], [1, 1], [1]], [[1], [2], [1, 1], [1, 1]])
    flux = np.array([1.0, -8.0, 0.25, 2.0])
    rf = S.ReactionFluxes.from_flux(flux, rd, 3, np.ones(2))
    np.testing.assert_array_equal(rf.production, [2.0, 1.0 - 16.0 + 0.25 + 2.0, 0.25])
    np.testing.assert_array_equal(rf.consumption, [2.0 - 8.0 + 0.25, 2.0, 0.25])
    np.testing.assert_array_equal(rf.top(3), [1, 3, 0])            # by |flux|
    np.testing.assert_array_equal(rf.top(10), [1, 3, 0, 2])


def test_flux_symbols_exported_and_listed():
    for name in FLUX_SYMBOLS:
        assert name in capi.SYMBOLS
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in FLUX_SYMBOLS:
        assert hasattr(L, name), name
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "kinetica_hip.h")).read()
    for name in FLUX_SYMBOLS:
        assert f"int {name}(" in header
    for name in ("flux_batched", "flux_batched_dev", "solution_flux"):
        assert callable(getattr(capi.HipNetwork, name))


def test_reaction_fluxes_rejects_a_calculator_of_another_length():
    sd = S.SpeciesData.from_names(["A", "B"])
    rd = S.RxData(1, [[1]], [[2]], [[1]], [[1]])
    pars = S.ODESimulationParams(tspan=(0.0, 1.0), u0=[1.0, 0.0], solve_chunkstep=0.5)
    out = S.ODESolveOutput(sd, rd, S.ODESolution(np.array([0.0, 1.0]), np.array([[1.0, 0.0], [0.5, 0.5]]), "Success"), None, None, pars,
                           C.ConditionSet({"T": 300.0}))
    with pytest.raises(ValueError):
        S.reaction_fluxes(out, S.DummyKineticCalculator([1.0, 2.0]))
    with pytest.raises(ValueError):
        S.reaction_fluxes(out, S.PrecalculatedArrheniusCalculator([1.0, 2.0, 3.0], [1.0, 1.0, 1.0]))
    with pytest.raises(ValueError):
        S.reaction_fluxes(out, S.DummyKineticCalculator([1.0]), weights="simpson")     # (checked before any device call as well)
