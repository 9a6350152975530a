"""CPU tests of the resident integrator's continuous rate mode (ResParams::rate_mode 3 of kinetica_jl_amd/csrc/resident_core.hpp:
the rates re-formed at T(t) of every step attempt and at every segment start, LU-cache slots at most 50 accepted steps old, no
warm chunk continuation) through its sequential replay (tests/native_cont: the backend of tests/native/resident_host.cpp plus
apply_T). References: quadrature for A -> B under a ramp, and oracle/bdf.py's continuous hook (k_of_time) - the rules
Solver::pre_attempt of solver.cpp follows. No GPU involved; tests/test_gpu_ensemble_continuous.py checks the device kernel."""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_int, c_int64, c_void_p

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import bdf as obdf
from oracle import oracle as orc
from tests.res_host import HostResident, ResResult

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_cont")
_LIB = os.path.join(_HERE, "libkin_resident_cont_host.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        capi.lib()                      # libkinetica_hip.so first (the replay links its host-side C++)
        if not os.path.exists(_LIB):
            subprocess.check_call(["make", "-C", _HERE, "-s"])
        L = ctypes.CDLL(_LIB)
        PD = POINTER(c_double)
        L.res_cont_solve.argtypes = [c_void_p, POINTER(capi.KinParams), PD, PD, PD, c_int64, c_int, PD, PD, POINTER(c_int64), POINTER(ResResult)]
        L.res_host_rows.restype = c_int64
        L.res_host_rows.argtypes = [POINTER(capi.KinParams)]
        _lib = L
    return _lib


def cont_solve(hr, pars, u0, t_nodes, T_nodes, n_slots=0):
    """The replayed controller under continuous rate updates on the network of HostResident `hr` (its Arrhenius parameters)."""
    L = lib()
    pd = lambda a: a.ctypes.data_as(POINTER(c_double))
    u0, tn, Tn = (np.ascontiguousarray(a, np.float64) for a in (u0, t_nodes, T_nodes))
    rows = L.res_host_rows(ctypes.byref(pars))
    t = np.empty(rows); u = np.empty((rows, hr.n))
    ns = c_int64(0)
    res = ResResult()
    rc = L.res_cont_solve(hr._h, ctypes.byref(pars), pd(u0), pd(tn), pd(Tn), len(tn), n_slots, pd(t), pd(u), ctypes.byref(ns), ctypes.byref(res))
    return t[:ns.value], u[:ns.value], rc, res.as_dict()


def kp(t1, chunk=1e-3, save=None, chunks=True, **kw):
    d = dict(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def units(u, ref, atol=1e-10, rtol=1e-8):
    return (np.abs(u - ref) / (atol + rtol * np.abs(ref))).max()


def oracle_cont(net, Ea, A, pars, u0, T_of, k_max=None):
    on = orc.OracleNetwork.from_flat(net)
    return obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), net.n_species, pars, u0,
                                     k_of_time=lambda tg: orc.arrhenius(Ea, A, T_of(tg), k_max=k_max))


def test_ramp_a_to_b_against_quadrature():
    """A -> B under a 500 -> 700 K ramp (the test_continuous_rate_updates_n3 case): A(t) = exp(-int_0^t k(T(s)) ds)."""
    from scipy.integrate import quad
    Ea, A = np.array([8.0e4]), np.array([1.0e-17])
    net = from_lists(2, [[(0, 1)]], [[(1, 1)]])
    hr = HostResident(net)
    hr.set_arrhenius(Ea, A)
    tn, Tn = np.array([0.0, 2.0]), np.array([500.0, 700.0])
    t, u, rc, st = cont_solve(hr, kp(2.0, chunk=0.5, save=0.25), [1.0, 0.0], tn, Tn)
    assert rc == 0 and len(t) == 9
    np.testing.assert_array_equal(t, 0.25 * np.arange(9))
    kfun = lambda tt: float(orc.arrhenius(Ea, A, 500.0 + 100.0 * tt)[0])
    truth = np.array([np.exp(-quad(kfun, 0.0, tt, epsabs=1e-13, epsrel=1e-13)[0]) for tt in t])
    assert units(u[:, 0], truth) < 100
    assert st["n_restarts"] == 4                 # one per chunk, none inside
    # the rates move: a static solve at the start temperature ends far from the ramp's state
    t0, u0_, rc0, _ = cont_solve(hr, kp(2.0, chunk=0.5, save=0.25), [1.0, 0.0], tn, np.array([500.0, 500.0]))
    assert rc0 == 0 and units(u0_[-1, 0], truth[-1]) > 1e4
    hr.close()


def test_controller_takes_the_steps_of_the_oracle_under_a_ramp():
    """300-species CRN, 900 -> 1300 K over 4 ms in 1 ms chunks: the replayed controller and oracle/bdf.py (continuous hook)
    take the same steps and factorisations within the bounds of test_controller_takes_the_steps_of_the_independent_cpu_implementation,
    restart once per chunk and agree within 20 tolerance units."""
    net, Ea, A = synthetic_crn(300, 1500)
    u0 = np.zeros(300); u0[0] = 1.0
    tn = np.linspace(0.0, 4e-3, 9)
    Tn = 900.0 + 1e5 * tn
    hr = HostResident(net)
    hr.set_arrhenius(Ea, A, k_max=1e12)
    t, u, rc, st = cont_solve(hr, kp(4e-3), u0, tn, Tn)
    to, uo, rco, sto = oracle_cont(net, Ea, A, dict(tspan=(0.0, 4e-3)), u0, lambda tg: np.interp(tg, tn, Tn), k_max=1e12)
    assert rc == 0 and rco == 0
    np.testing.assert_array_equal(t, to)
    assert abs(st["n_steps"] - sto["n_steps"]) <= 0.01 * sto["n_steps"] + 1, (st, sto)
    assert abs(st["n_factor"] - sto["n_factor"]) <= 0.05 * sto["n_factor"] + 2, (st, sto)
    assert st["n_restarts"] == st["n_chunks"] == 4
    assert units(u, uo) < 20
    # solve_chunks == 2 (warm continuation) is solve_chunks == 1 under continuous rates: the same steps, bit for bit
    t2, u2, rc2, st2 = cont_solve(hr, kp(4e-3, solve_chunks=2), u0, tn, Tn)
    assert rc2 == 0 and st2 == st
    np.testing.assert_array_equal(u2, u)
    hr.close()


@pytest.mark.parametrize("seed,T0,rate", [(4, 1200.0, -3e4), (2, 1100.0, 2e4)])
def test_tolerance_retries_follow_the_oracle(seed, T0, rate):
    """Continuous cases on which oracle/bdf.py needs tolerance retries (the ramps of tools/robustness_continuous.py on 300-species
    networks at rtol 1e-6): the replayed controller - which re-forms the rates at every retried chunk's start - takes the same
    number of retries, ends with the same final tolerances and returns the same retcode."""
    net, Ea, A = synthetic_crn(300, 1500, seed=seed)
    u0 = np.zeros(300); u0[0] = 1.0
    tn = np.linspace(0.0, 1e-2, 21)
    Tn = T0 + rate * tn
    hr = HostResident(net)
    hr.set_arrhenius(Ea, A, k_max=1e12)
    t, u, rc, st = cont_solve(hr, kp(1e-2, chunk=2.5e-3, save=2.5e-3, maxiters=200000, dtmin=1e-30, abstol=1e-8, reltol=1e-6), u0, tn, Tn)
    to, uo, rco, sto = oracle_cont(net, Ea, A, dict(tspan=(0.0, 1e-2), solve_chunkstep=2.5e-3, save_interval=2.5e-3, maxiters=200000,
                                                    dtmin=1e-30, abstol=1e-8, reltol=1e-6), u0, lambda tg: np.interp(tg, tn, Tn), k_max=1e12)
    assert sto["n_retries"] >= 1
    assert st["n_retries"] == sto["n_retries"] and rc == rco == 0
    assert st["final_reltol"] == sto["final_reltol"] and st["final_abstol"] == sto["final_abstol"]
    np.testing.assert_array_equal(t, to)
    hr.close()


def test_flat_profile_takes_the_static_steps_and_pays_the_jacobian_age_bound():
    """What the continuous ensemble's cost per member-step rests on: a FLAT profile takes the static solve's
    steps, but the 50-step bound on the age of a slot's Jacobian refuses every slot once the Jacobian is older, and the
    factorisation that replaces it reuses that Jacobian - so the solve refactorises at most steps. 300 species, 1 000 K, 2 ms
    in 1 ms chunks: 899 steps / 603 factorisations continuous against 892 / 77 static."""
    from oracle import oracle as orc_
    net, Ea, A = synthetic_crn(300, 1500)
    u0 = np.zeros(300); u0[0] = 1.0
    hr = HostResident(net)
    hr.set_arrhenius(Ea, A, k_max=1e12)
    t, u, rc, st = cont_solve(hr, kp(2e-3), u0, np.array([0.0, 2e-3]), np.array([1000.0, 1000.0]))
    ts, us, rcs, sts = hr.solve(kp(2e-3), u0, k0=orc_.arrhenius(Ea, A, 1000.0, k_max=1e12))
    assert rc == rcs == 0
    np.testing.assert_array_equal(t, ts)
    assert abs(st["n_steps"] - sts["n_steps"]) <= 0.01 * sts["n_steps"] + 1, (st, sts)
    assert units(u, us) < 20
    assert st["n_factor"] > 5 * sts["n_factor"] and st["n_factor"] > 0.5 * st["n_steps"], (st, sts)
    assert st["n_jac"] <= 2 * sts["n_jac"] + 2, (st, sts)          # the Jacobians are not renewed: the factorisations are
    hr.close()
