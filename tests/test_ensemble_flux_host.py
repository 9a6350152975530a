"""Host-side tests of the ensemble analysis (no GPU): solving.ensemble_flux_sources - the per-(member, row) weights and
rate-constant keys kin_ensemble_flux takes - for the four kinds of ensemble, ODESolution.fluxes, and the six new symbols in
the binding's list and the built library."""
import ctypes
import os

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S

NEW_SYMBOLS = ["kin_flux_segmented", "kin_flux_segmented_dev", "kin_ensemble_size", "kin_ensemble_max", "kin_ensemble_dot",
               "kin_ensemble_flux"]

T_GRID = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 2.5])        # uneven on purpose: the trapezoid weights differ from row to row
N_SAVED = np.array([6, 0, 1, 3, 2], np.int64)


def _check_weights(w, t, n_saved):
    assert w.shape == (len(n_saved), len(t))
    for m, n in enumerate(n_saved):
        assert np.all(w[m, n:] == 0.0), m                                  # zero past n_saved
        if n >= 1:
            assert np.array_equal(w[m, :n], S.flux_weights(t[:n])), m      # the member's own times, not the grid's
        if n <= 1:
            assert np.all(w[m] == 0.0), m                                  # no row, or one row: nothing to integrate over
    assert w[0].sum() == pytest.approx(t[-1] - t[0], rel=1e-15)


def test_static_sources_per_member_k_and_per_member_T():
    src = S.ensemble_flux_sources("static", T_GRID, N_SAVED)
    _check_weights(src["w"], T_GRID, N_SAVED)
    assert set(src) == {"w", "k_row"} and src["k_row"].dtype == np.int64
    assert np.array_equal(src["k_row"], np.arange(5)[:, None] * np.ones((1, 6), np.int64))
    T = np.array([900.0, 950.0, 1000.0, 1050.0, 1100.0])
    src = S.ensemble_flux_sources("static", T_GRID, N_SAVED, T=T)
    _check_weights(src["w"], T_GRID, N_SAVED)
    assert set(src) == {"w", "T_rows"} and np.array_equal(src["T_rows"], np.repeat(T[:, None], 6, axis=1))
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("static", T_GRID, N_SAVED, T=T[:4])


def test_shared_discrete_stops_as_temperatures_and_as_table_rows():
    tstops = np.array([0.0, 0.5, 0.75, 1.5])                 # saved times 0.5 and 1.5 ARE stops: they take that stop's rates
    Ts = np.array([900.0, 1000.0, 1100.0, 1200.0])
    held = np.array([0, 0, 1, 2, 3, 3])
    assert np.array_equal(S.held_stop_index(T_GRID, tstops), held)
    src = S.ensemble_flux_sources("discrete", T_GRID, N_SAVED, tstops=tstops, T_stops=Ts)
    _check_weights(src["w"], T_GRID, N_SAVED)
    assert np.array_equal(src["T_rows"], np.repeat(Ts[held][None, :], 5, axis=0))
    src = S.ensemble_flux_sources("discrete", T_GRID, N_SAVED, tstops=tstops)
    assert src["k_row"].dtype == np.int64 and np.array_equal(src["k_row"], np.repeat(held[None, :], 5, axis=0))
    # a first stop later than the first saved time: the first stop's rates hold before it (kin_solve's hold)
    src = S.ensemble_flux_sources("discrete", T_GRID, N_SAVED, tstops=np.array([0.3, 1.0]))
    assert np.array_equal(src["k_row"][0], [0, 0, 0, 1, 1, 1])
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("discrete", T_GRID, N_SAVED)


def test_per_member_schedules():
    stops = [(np.array([0.0]), np.array([1000.0])),
             (np.array([0.0, 0.5, 1.0]), np.array([900.0, 950.0, 1000.0])),
             (np.array([0.0, 0.25, 0.26, 2.5]), np.array([800.0, 810.0, 820.0, 830.0])),
             (np.arange(11) * 0.25, 900.0 + 10.0 * np.arange(11)),
             (np.array([0.0, 2.0]), np.array([700.0, 750.0]))]
    src = S.ensemble_flux_sources("discrete_members", T_GRID, N_SAVED, stops=stops)
    _check_weights(src["w"], T_GRID, N_SAVED)
    assert src["T_rows"].shape == (5, 6)
    for m, (ts, Ts) in enumerate(stops):
        assert np.array_equal(src["T_rows"][m], Ts[S.held_stop_index(T_GRID, ts)]), m
    assert np.array_equal(src["T_rows"][1], [900.0, 900.0, 950.0, 1000.0, 1000.0, 1000.0])      # 0.5 and 1.0 are stops
    assert np.array_equal(src["T_rows"][2], [800.0, 810.0, 820.0, 820.0, 820.0, 830.0])
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("discrete_members", T_GRID, N_SAVED, stops=stops[:4])


def test_continuous_profiles_are_np_interp():
    nodes = [(np.array([0.0, 2.5]), np.array([900.0, 1400.0])),
             (np.array([0.0, 1.0, 2.5]), np.array([1000.0, 1200.0, 1100.0])),
             (np.array([0.0, 2.5]), np.array([1000.0, 1000.0])),                  # a static profile as two equal nodes
             (np.linspace(0.0, 2.5, 26), 900.0 + 100.0 * np.sin(np.linspace(0.0, 2.5, 26))),
             (np.array([0.5, 2.0]), np.array([800.0, 900.0]))]                   # saved times outside the nodes: held ends
    src = S.ensemble_flux_sources("continuous", T_GRID, N_SAVED, nodes=nodes)
    _check_weights(src["w"], T_GRID, N_SAVED)
    for m, (tn, Tn) in enumerate(nodes):
        assert np.array_equal(src["T_rows"][m], np.interp(T_GRID, tn, Tn)), m
    assert np.all(src["T_rows"][2] == 1000.0)
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("continuous", T_GRID, N_SAVED, nodes=nodes[:2])


def test_bad_kind_and_bad_counts():
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("ramp", T_GRID, N_SAVED)
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("static", T_GRID, [7])
    with pytest.raises(ValueError):
        S.ensemble_flux_sources("static", T_GRID, [-1])
    src = S.ensemble_flux_sources("static", T_GRID, np.zeros(0, np.int64))       # no members
    assert src["w"].shape == (0, 6) and src["k_row"].shape == (0, 6)


def test_ode_solution_fluxes_defaults_to_none():
    sol = S.ODESolution(np.zeros(1), np.zeros((1, 2)), "Success")
    assert sol.fluxes is None
    fl = S.ReactionFluxes(np.zeros(1), np.zeros(2), np.zeros(2), np.zeros(1))
    assert S.ODESolution(np.zeros(1), None, "Success", fluxes=fl).fluxes is fl


def test_new_symbols_listed_and_exported():
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
    assert os.path.exists(capi.LIB_PATH)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    header = open(os.path.join(os.path.dirname(os.path.abspath(capi.__file__)), "..", "include", "kinetica_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    for name in ("flux_segmented", "flux_segmented_dev", "ensemble_size", "ensemble_max", "ensemble_dot", "ensemble_flux"):
        assert callable(getattr(capi.HipNetwork, name)), name
