"""GPU tests of the LU cache: the drift guard and the slot rules in every integrator, against the references of
tests/cache_cases.py (module docstring there: the reference, the derived bound, the cases).

Probe level (kin_cache_probe: the integrators' own launchers, nothing computed by the probe).
  path 0 - launch_jac_diag, launch_drift_test in Solver's form (pinned host target) and in the lockstep ensemble's (offset
  output, copied afterwards), drop_drifted; path 1 - the resident kernel: ph_factor's saved diagonal, DevBackend::drift_check
  on wavefront 0 with ph_drift on all eight. Per case: jd bit for bit the diagonal of the given values; drift within the derived
  bound, bit for bit on the exact cases, at least 1e299 where the reference is unbounded; the drop decisions and their count
  those of the reference; unused slots report 0 and stay unused. The slot-rule table through DevBackend::nearest_slot /
  victim_slot equals the reference and the templates of bdf_rules.hpp (host replay) answer for answer.
Solve level. A reversible first-order star (J depends on the rate constants alone), discrete stops with a k_table, three
  schedules: rates unchanged, every rate x 16 from one stop on, every rate / 16. In every driver - kin_solve host-driven and
  resident, kin_solve_ensemble resident (two workgroups per compute unit, K = 3), lockstep, threads, the host replay,
  oracle/bdf.py - unchanged rates drop nothing (every drift is exactly 0), a jump drops at least one slot and at most n_factor,
  costs factorisations, and leaves the trajectory within 100 tolerance units of the oracle's; one slot means no band and no guard.

  Every one of the seven drivers takes the same steps on this problem (n_steps 240 / 299 / 212, n_factor 25 / 35 / 27 for
  unchanged / x 16 / / 16), so every driver's n_lu_dropped is compared with the host replay's and equals it: 0 / 16 / 9.

Largest error / bound (printed per case with pytest -s), measured on an MI355X: path 0 0.423 (both forms of the launch: the same
bits), path 1 0.434; the network with special stoichiometries 0.127 on both; a float64 NumPy evaluation on the CPU 0.434
(tests/test_cache_cases.py). Every exact case: the reference bit for bit, error 0.

Mutation check (value-only changes on a scratch build, one at a time, selected through KIN_LIB_PATH / KIN_RES_HOST_PATH, nothing of
it kept): which tests of this file fail, and what the suite did before - its solve-level GPU modules run whole (test_gpu_solve,
_configs, _resident, _ensemble, _ensemble_discrete, _ensemble_continuous, _ensemble_analysis, _boundary_r2 without its three
Newton-matrix solves, _flux_solution, _drg_reduce: 86 tests), and for mutation 8 the whole non-GPU suite as well.
  1 slot_drift_kernel returns 0: 11 fail - host_path_drift at every N, special_stoichiometries, guard_fires for the host-driven
    kin_solve and the lockstep ensemble (n_lu_dropped = 0 after a jump).
    Before: 1 of 86 failed, test_c4_ramp_prefix_against_truth - a stored truth, its largest deviation 35.8 units against 29 allowed.
  2 slot_drift_kernel reads a.c[0] for every slot: the same 11 fail.
    Before: MISSED - all 86 passed.
  3 slot_drift_kernel's loop stops at element 1024: 2 fail - host_path_drift[N1025] and [N2049] (the spikes at 1024 and N - 1).
    Before: MISSED.
  4 fmax(q, 1 / q) becomes q in slot_drift_kernel (a shrinking diagonal is not seen): the same 11 fail as for 1.
    Before: MISSED.
  5 ph_drift covers slots below 8 only: 6 fail - resident_kernel_drift[N65] and [N400] (9, 63, 64 slots: the sentinel comes
    back), special_stoichiometries, guard_fires for the resident kin_solve, the shared-CU ensemble and the threads (which solve a
    network of this size in the resident kernel).
    Before: 5 of 86 failed, all of them comparisons of one resident run with another bit for bit (test_gpu_resident,
    test_gpu_ensemble_discrete): slots 8 .. 63 are judged by whatever the LDS held, which differs from launch to launch. No test
    said what was wrong, and a kernel that zeroed its LDS would have passed.
  6 drop_drifted uses < for <=: 9 fail - host_path_drift at every N and special_stoichiometries (the exact cases at the
    threshold: drift 1.0 must be kept).
    Before: MISSED.
  7 DevBackend::nearest_slot resolves ties to the higher index: resident_slot_rules fails (exact tie, full 64).
    Before: MISSED.
  8 slot_nearest's age test uses >=: resident_slot_rules fails (restart age: the device disagrees with the mutated template), and
    without a device test_slot_rules_through_the_host_templates[restart age] of tests/test_cache_cases.py.
    Before: MISSED - all 86 GPU tests and all 407 non-GPU tests passed.
  9 DevBackend::victim_slot picks the largest last_use: resident_slot_rules fails (every LRU row).
    Before: MISSED.
  So the previous suite noticed two of the nine, one through a stored trajectory and one through run-to-run differences; the
  seven others changed no assertion's outcome."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from oracle import bdf as obdf
from oracle import oracle as orc
from tests import cache_cases as cc
from tests import res_host

pytestmark = pytest.mark.gpu

WORST = {0: 0.0, 1: 0.0}          # largest error / bound seen per path (printed by the tests)


# ------------------------------------------------------------------------------------------------------------ probe level
def check_drift(h, path, case, seed=0):
    rowptr, col = h.jac_pattern()
    jv_slots, jv_now = cc.jac_values(case, rowptr, col, seed)
    out = h.cache_probe(path, jv_slots, case.c, case.valid, jv_now, case.max_drift)
    label = f"path {path} {case.name}"
    assert np.array_equal(out["jd"], case.jd_old, equal_nan=True), label
    forms = [out["drift"]] + ([out["drift_offset"]] if path == 0 else [])
    v = case.valid != 0
    fin = np.isfinite(case.ref)
    for got in forms:
        assert np.all(got[~v] == 0.0), label                                      # an unused slot reports 0
        err = np.abs(got[fin] - case.ref[fin])
        nz = case.bound[fin] > 0
        if nz.any():
            ratio = float(np.max(err[nz] / case.bound[fin][nz]))
            WORST[path] = max(WORST[path], ratio)
            print(f"{label}: error / bound {ratio:.3f}")
        assert np.all(err <= case.bound[fin]), (label, got, case.ref)
        if case.exact:
            assert np.array_equal(got, case.ref), (label, got, case.ref)
        assert np.all(got[~fin] >= cc.UNBOUNDED), (label, got)
    if path == 0:
        assert np.array_equal(forms[0], forms[1], equal_nan=True), label
        assert out["clean"] and out["n_tested"] == case.ns and out["n_dropped_offset"] == int(case.dropped.sum()), label
    assert np.array_equal(out["dropped"], case.dropped), (label, out["drift"], case.ref)
    assert np.array_equal(out["valid_after"] != 0, v & ~case.dropped), label
    assert out["n_dropped"] == int(case.dropped.sum()), label


@pytest.mark.parametrize("N,cases", cc.host_cases(), ids=[f"N{N}" for N in cc.HOST_N])
def test_host_path_drift(N, cases):
    h = capi.HipNetwork.from_flat(cc.chain_net(N))
    for i, case in enumerate(cases):
        check_drift(h, 0, case, i)
    h.close()
    print(f"path 0 worst error / bound so far {WORST[0]:.3f}")


@pytest.mark.parametrize("N,cases", cc.resident_cases(), ids=[f"N{N}" for N in cc.RES_N])
def test_resident_kernel_drift(N, cases):
    h = capi.HipNetwork.from_flat(cc.chain_net(N))
    for i, case in enumerate(cases):
        check_drift(h, 1, case, i)
    h.close()
    print(f"path 1 worst error / bound so far {WORST[1]:.3f}")


def test_special_stoichiometries_both_paths():
    """2A -> B, A -> 2B, a collider, a product that is also a reactant: the diagonal positions come from a pattern that is no chain's"""
    net = cc.special_net()
    h = capi.HipNetwork.from_flat(net)
    for i, case in enumerate(cc.special_net_cases(net.n_species)):
        check_drift(h, 0, case, i)
        check_drift(h, 1, case, i)
    h.close()


def test_resident_slot_rules():
    h = capi.HipNetwork.from_flat(cc.chain_net(5))
    for name, t, qs, exp in cc.slot_rule_rows():
        if len(t["valid"]) > cc.RES_MAX_SLOTS:
            continue
        got = h.cache_probe(1, table=t, queries=qs)
        for q, g, (near, victim) in zip(qs, got, exp):
            host = res_host.slot_rules(t, q)
            assert g[0] == near and g[0] == host[0], (name, q, g, near, host)
            if victim is not None:
                assert g[1] == victim and g[1] == host[1], (name, q, g, victim, host)
    h.close()


def test_argument_checks():
    net = cc.chain_net(5)
    h = capi.HipNetwork.from_flat(net)
    case = cc.placement_case(5)
    rowptr, col = h.jac_pattern()
    jv_slots, jv_now = cc.jac_values(case, rowptr, col)
    P32, P64, PD = capi.POINTER(capi.c_int32), capi.POINTER(capi.c_int64), capi.POINTER(capi.c_double)
    jd = np.zeros((130, 5)); drift = np.zeros((2, 130)); out = np.zeros(130, np.int32); info = np.zeros(8, np.int64)
    cf = np.ones(130); va = np.ones(130, np.int32)
    pd = lambda a: a.ctypes.data_as(PD)

    def call(path, mode, ns, jvs=jv_slots, now=jv_now, c=cf, v=va, stamps=None, nq=0, qd=None, qi=None):
        return capi.lib().kin_cache_probe(h._h, path, mode, ns, None if jvs is None else pd(jvs), pd(c), v.ctypes.data_as(P32),
                                          None if now is None else pd(now), 1.0, None if stamps is None else stamps.ctypes.data_as(P64), nq,
                                          None if qd is None else pd(qd), None if qi is None else qi.ctypes.data_as(P64), pd(jd), pd(drift),
                                          out.ctypes.data_as(P32), info.ctypes.data_as(P64))
    E = capi.KIN_ERR_INVALID_ARG
    assert call(2, 0, 1) == E and call(0, 2, 1) == E
    assert call(0, 0, 0) == E and call(0, 0, cc.LU_MAX_SLOTS + 1) == E and call(1, 0, cc.RES_MAX_SLOTS + 1) == E
    assert call(0, 0, 1, jvs=None) == E and call(1, 0, 1, now=None) == E
    st = np.zeros((3, 4), np.int64); qd = np.array([[1.0, 0.3]]); qi = np.array([[0, 50, 0, -1, 4]], np.int64)
    assert call(0, 1, 4, stamps=st, nq=1, qd=qd, qi=qi) == E                      # the rules belong to path 1
    assert call(1, 1, 65, stamps=st, nq=1, qd=qd, qi=qi) == E and call(1, 1, 4, stamps=st, nq=0, qd=qd, qi=qi) == E
    assert call(1, 1, 4, stamps=None, nq=1, qd=qd, qi=qi) == E
    qi_bad = np.array([[0, 50, 0, -1, 65]], np.int64)
    assert call(1, 1, 4, stamps=st, nq=1, qd=qd, qi=qi_bad) == E
    assert call(1, 1, 4, stamps=st, nq=1, qd=qd, qi=qi) == capi.KIN_OK
    h.close()
    # a network the resident kernel does not take: state and rates beyond a compute unit's LDS
    big = cc.chain_net(6000)
    hb = capi.HipNetwork.from_flat(big)
    nnz = len(hb.jac_pattern()[1])
    with pytest.raises(capi.KineticaHipError) as e:
        hb.cache_probe(1, np.zeros((1, nnz)), [1.0], [1], np.zeros(nnz))
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED
    hb.close()


# ------------------------------------------------------------------------------------------------------------ solve level
KEYS = ("n_steps", "n_factor", "n_lu_dropped", "n_restarts")
_ref = {}


def kp(**kw):
    d = dict(tspan0=0.0, tspan1=cc.GUARD_T1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=0, ban_negatives=0,
             solve_chunkstep=1e-3, maxiters=100000, save_interval=cc.GUARD_SAVE, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def units(u, ref):
    return float((np.abs(u - ref) / (1e-10 + 1e-8 * np.abs(ref))).max())


def references():
    """the oracle's and the host replay's solves of the three schedules, once"""
    if not _ref:
        net, k, u0 = cc.guard_problem()
        on = orc.OracleNetwork.from_flat(net)
        hr = res_host.HostResident(net)
        for name in cc.GUARD_SCHEDULES:
            tab = cc.guard_table(k, name)
            to, uo, rco, sto = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), net.n_species,
                                                         dict(tspan=(0.0, cc.GUARD_T1), solve_chunks=False, save_interval=cc.GUARD_SAVE), u0,
                                                         tstops=cc.GUARD_TSTOPS, k_of_stop=lambda i: tab[i])
            th, uh, rch, sth = hr.solve(kp(), u0, tstops=cc.GUARD_TSTOPS, k_table=tab)
            assert rco == 0 and rch == 0 and np.allclose(to, th)
            _ref[name] = dict(t=to, oracle=(uo, sto), replay=(uh, sth))
        hr.close()
    return _ref


def check_guard(label, runs):
    """runs: schedule -> (u, stats) of one driver"""
    ref = references()
    same = runs["same"][1]
    print(label, {name: {q: st[q] for q in KEYS} for name, (_, st) in runs.items()})
    assert same["n_lu_dropped"] == 0, label
    for name in ("up", "down"):
        u, st = runs[name]
        assert 1 <= st["n_lu_dropped"] <= st["n_factor"], (label, name, st)
        assert st["n_factor"] > same["n_factor"], (label, name, st["n_factor"], same["n_factor"])
    for name, (u, st) in runs.items():
        assert units(u, ref[name]["oracle"][0]) < 100.0, (label, name)
        rp = ref[name]["replay"][1]
        if st["n_steps"] == rp["n_steps"]:
            assert st["n_lu_dropped"] == rp["n_lu_dropped"], (label, name, st["n_lu_dropped"], rp["n_lu_dropped"])


def test_guard_in_the_oracle_and_the_host_replay():
    ref = references()
    check_guard("oracle/bdf.py", {n: r["oracle"] for n, r in ref.items()})
    check_guard("host replay", {n: r["replay"] for n, r in ref.items()})


def _solo(h, k, u0, name):
    t, u, rc, st, _ = h.solve(kp(), u0, tstops=cc.GUARD_TSTOPS, k_table=cc.guard_table(k, name))
    assert rc == 0 and np.allclose(t, references()[name]["t"])
    return u, st


def _ensemble(h, k, u0, name, K=3):
    t, u, ns, rcs, sts = h.solve_ensemble(kp(), np.tile(u0, (K, 1)), tstops=cc.GUARD_TSTOPS, k_table=cc.guard_table(k, name))
    assert (rcs == 0).all() and np.allclose(t, references()[name]["t"])
    for m in range(1, K):                                                          # identical members
        assert np.array_equal(u[m], u[0]) and sts[m]["n_lu_dropped"] == sts[0]["n_lu_dropped"] and sts[m]["n_factor"] == sts[0]["n_factor"]
    return u[0], sts[0]


DRIVERS = {
    "kin_solve host-driven": (dict(KIN_RESIDENT="0"), _solo),
    "kin_solve resident": (dict(), _solo),
    "ensemble resident shared CU": (dict(KIN_RESIDENT_SHARED_CU="1"), _ensemble),
    "ensemble lockstep": (dict(KIN_ENSEMBLE_ROUTE="lockstep"), _ensemble),
    "ensemble threads": (dict(KIN_ENSEMBLE_ROUTE="threads"), _ensemble),
}


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_guard_fires_when_it_must_and_only_then(driver, monkeypatch):
    env, run = DRIVERS[driver]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    net, k, u0 = cc.guard_problem()
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    runs = {name: run(h, k, u0, name) for name in cc.GUARD_SCHEDULES}
    h.close()
    check_guard(driver, runs)


@pytest.mark.parametrize("resident", ("0", "1"))
def test_one_slot_means_no_guard(resident, monkeypatch):
    """KIN_LU_CACHE_SLOTS=1: no reuse band, so nothing to guard - a jump drops nothing"""
    monkeypatch.setenv("KIN_LU_CACHE_SLOTS", "1")
    monkeypatch.setenv("KIN_RESIDENT", resident)
    net, k, u0 = cc.guard_problem()
    h = capi.HipNetwork.from_flat(net)                                             # (the host-driven solver reads the switch once per handle)
    h.set_rates(k)
    for name in ("up", "down"):
        u, st = _solo(h, k, u0, name)
        assert st["n_lu_dropped"] == 0 and st["lu_slots"] == 1, (name, st)
        assert units(u, references()[name]["oracle"][0]) < 100.0
    h.close()
