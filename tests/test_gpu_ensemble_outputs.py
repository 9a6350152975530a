"""GPU test of what an ensemble call leaves in its outputs past the rows its members saved (kinetica_jl_amd/csrc/solver.hpp:
finish_members, behind every route): out_t is the furthest member's save times and zeros from its n_saved on, out_u is zeros
past each member's n_saved. Through the C entry itself, into buffers prefilled with NaN, with members that all fail early."""
import ctypes

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from tests.test_gpu_resident import ROB, ROB_K, kp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route", ["resident", "threads", "lockstep"])
def test_outputs_past_the_saved_rows_are_zeros_on_every_route(monkeypatch, route):
    K = 2
    if route == "resident":
        # (tests/test_gpu_resident.py: a member that fails) the second rate constant overflows the state
        net, n = ROB, 3
        p = kp(40.0, chunks=False, save=4.0, maxiters=2000)
        k = np.tile(ROB_K * np.array([1.0, 1e30, 1.0]), (K, 1))
        u0 = np.tile([1.0, 0.0, 0.0], (K, 1))
    else:
        # (tests/test_gpu_ensemble_discrete.py: the size both forced routes take; tests/test_gpu_resident.py: k * 1e40)
        monkeypatch.setenv("KIN_ENSEMBLE_ROUTE", route)
        n = 1000
        net, Ea, A = synthetic_crn(n, 5 * n)
        p = kp(2e-3, save=5e-4, maxiters=3000)
        u0 = np.zeros((K, n)); u0[:, 0] = 1.0
    h = capi.HipNetwork.from_flat(net)
    if route != "resident":
        h.set_arrhenius(Ea, A, k_max=1e12)
        k = np.tile(h.rates_at(1000.0) * 1e40, (K, 1))
    L, PD = capi.lib(), ctypes.POINTER(ctypes.c_double)
    pd = lambda a: a.ctypes.data_as(PD)
    rows = ctypes.c_int64(0)
    args = (h._h, ctypes.byref(p), K, pd(u0), pd(k), None, None, None, None, 0, ctypes.byref(rows))
    assert L.kin_solve_ensemble(*args, None, None, None, None, None) == 0
    cap = rows.value
    assert cap == (11 if route == "resident" else 5)
    t, u = np.full(cap, np.nan), np.full((K, cap, n), np.nan)
    ns, rcs, stats = np.full(K, -1, np.int64), np.zeros(K, np.int32), (capi.KinStats * K)()
    status = L.kin_solve_ensemble(*args, pd(t), pd(u), ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  rcs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), stats)
    assert status == 0
    assert (rcs != 0).all() and (ns >= 0).all() and (ns < cap).all()          # every member failed before the end of the grid
    n_best = int(ns.max())
    print(f"{route}: n_saved {ns.tolist()}, retcodes {rcs.tolist()}, out_t {t.tolist()}")
    assert np.isfinite(t[:n_best]).all() and (np.diff(t[:n_best]) > 0).all()
    assert np.array_equal(t[n_best:], np.zeros(cap - n_best))
    for m in range(K):
        assert np.array_equal(u[m, ns[m]:], np.zeros((cap - ns[m], n))), m
    h.close()
