"""The host-driven integrator (KIN_RESIDENT=0) as a backend of the shared BDF controller (csrc/resident_core.hpp:
ResidentBdf<HostBackend>, the backend in csrc/solver.cpp): relations between its own switches and entry points that hold whatever
the step sequence is - what is asynchronous in the backend (speculative batches, the deferred accept, the flag of a vanished pivot
that arrives with the corrector's result) must not show in the results.

Networks: A -> B and A -> B -> C of tests/test_gpu_driver_schedule.py, and a stiff 12-species network of synth.py whose solve at
1 000 K takes ~700 steps with ~220 rejected attempts and ~900 reused factorisations. The environment switches are read when a
handle's solver is built, so every case solves on a handle of its own; the undisturbed solve of each network is computed once.

All of these relations held on the commit before the controller was shared (this file passed there unchanged)."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from tests.test_gpu_driver_schedule import NETS as SMALL, errscale, rate_rows

pytestmark = pytest.mark.gpu

COUNTERS = ("n_steps", "n_rejected", "n_factor", "n_lu_reused", "n_newton_fail", "n_restarts")
SWITCHES = ("KIN_SPECULATE", "KIN_FUSE_NEWTON", "KIN_LU_BAND", "KIN_LU_CACHE_SLOTS", "KIN_INJECT_BAD_PIVOT")
STIFF = synthetic_crn(12, 40)
NETS = ("a_to_b", "chain3", "stiff12")


def kp(name, mode=1, save=True, **kw):
    """three chunks with four save intervals each; save=False: complete timespan, every step saved"""
    end, chunk = (3e-3, 1e-3) if name == "stiff12" else (1.0, 0.25)
    d = dict(tspan0=0.0, tspan1=end, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=mode if save else 0,
             ban_negatives=0, solve_chunkstep=chunk, maxiters=100000, save_interval=chunk / 4 if save else -1.0, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def handle(name):
    """(handle with its rates set, u0)"""
    if name == "stiff12":
        net, Ea, A = STIFF
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        h.set_rates(h.rates_at(1000.0))
        u0 = np.zeros(net.n_species); u0[:3] = [1.0, 0.5, 0.25]
        return h, u0
    h = capi.HipNetwork.from_flat(SMALL[name])
    h.set_rates(rate_rows(name, [3.0])[0])
    u0 = np.zeros(SMALL[name].n_species); u0[0] = 1.0
    return h, u0


def solve(monkeypatch, name, pars, **env):
    """(t, u, retcode, stats) of one host-driven solve on a fresh handle under the given switches"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KIN_RESIDENT", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    h, u0 = handle(name)
    t, u, rc, st, status = h.solve(pars, u0)
    h.close()
    assert status == (capi.KIN_OK if rc == 0 else capi.KIN_ERR_SOLVE_FAILED)
    assert st["lu_slots"] == (1 if env.get("KIN_LU_CACHE_SLOTS") == 1 else 128)   # the host-driven integrator ran
    return t, u, rc, st


@pytest.fixture(scope="module")
def plain():
    """the undisturbed solve of every network, computed once and left unchanged"""
    mp = pytest.MonkeyPatch()
    try:
        out = {n: solve(mp, n, kp(n)) for n in NETS}
    finally:
        mp.undo()
    for n, (t, u, rc, st) in out.items():
        print(f"{n}: steps {st['n_steps']} rejected {st['n_rejected']} factorisations {st['n_factor']} reused {st['n_lu_reused']}")
        assert rc == 0 and st["n_bad_pivot"] == 0 and st["n_retries"] == 0
        u.setflags(write=False); t.setflags(write=False)
    # the stiff network is there for its rejections and its reuse
    assert out["stiff12"][3]["n_rejected"] > 50 and out["stiff12"][3]["n_lu_reused"] > 100
    return out


@pytest.mark.parametrize("name", NETS)
def test_speculation_does_not_show_in_the_result(monkeypatch, plain, name):
    res = {on: solve(monkeypatch, name, kp(name), KIN_SPECULATE=on) for on in (0, 1)}
    for on, (t, u, rc, st) in res.items():
        print(f"{name} KIN_SPECULATE={on}: " + " ".join(f"{c} {st[c]}" for c in COUNTERS))
    (t0, u0, rc0, st0), (t1, u1, rc1, st1) = res[0], res[1]
    assert rc0 == rc1 == 0
    assert np.array_equal(t0, t1) and np.array_equal(u0, u1)
    assert [st0[c] for c in COUNTERS] == [st1[c] for c in COUNTERS]
    # ... and the default is one of the two
    assert np.array_equal(u1, plain[name][1]) and [st1[c] for c in COUNTERS] == [plain[name][3][c] for c in COUNTERS]


@pytest.mark.parametrize("name", NETS)
def test_single_steps_are_the_every_step_solve(monkeypatch, name):
    t, u, rc, st = solve(monkeypatch, name, kp(name, save=False))
    assert rc == 0 and len(t) == st["n_steps"] + 1      # the initial state, then every accepted step
    h, u0 = handle(name)
    h.integrator_init(kp(name, save=False), u0)
    tt, uu = [], []
    while h.integrator_step(1) == 1:
        t1, u1, rc1, _ = h.integrator_state()
        assert rc1 == 0
        tt.append(t1); uu.append(u1)
    h.close()
    print(f"{name}: {len(tt)} single steps, every-step solve {len(t) - 1}")
    assert np.array_equal(np.array(tt), t[1:]) and np.array_equal(np.array(uu), u[1:])


@pytest.mark.parametrize("attempt", [0, 7])
@pytest.mark.parametrize("name", NETS)
def test_injected_bad_pivot(monkeypatch, plain, name, attempt):
    """KIN_INJECT_BAD_PIVOT=n: the n-th step attempt of the call finds the flag of a vanished pivot raised"""
    t, u, rc, st = solve(monkeypatch, name, kp(name), KIN_INJECT_BAD_PIVOT=attempt)
    dev = errscale(u, plain[name][1])
    print(f"{name} attempt {attempt}: bad pivots {st['n_bad_pivot']} rc {rc} rejected {st['n_rejected']} jac {st['n_jac']} deviation {dev:.2f} units")
    assert rc == 0 and st["n_bad_pivot"] == 1
    assert np.array_equal(t, plain[name][0]) and dev < 100


@pytest.mark.parametrize("switch", [dict(KIN_LU_BAND=0), dict(KIN_LU_CACHE_SLOTS=1)])
@pytest.mark.parametrize("name", NETS)
def test_without_the_cache(monkeypatch, plain, name, switch):
    """no reuse band: a new factorisation at every change of c; a matrix kept across an error-test rejection is used unscaled"""
    t, u, rc, st = solve(monkeypatch, name, kp(name), **switch)
    dev = errscale(u, plain[name][1])
    print(f"{name} {switch}: rc {rc} steps {st['n_steps']} rejected {st['n_rejected']} factorisations {st['n_factor']} reused {st['n_lu_reused']} "
          f"deviation {dev:.2f} units")
    assert rc == 0 and st["n_lu_reused"] == 0 and st["n_lu_dropped"] == 0
    assert np.array_equal(t, plain[name][0]) and dev < 100
    if name == "stiff12":
        assert st["n_rejected"] > 0        # the rejected-step case (the first-order networks may solve without a rejection)


@pytest.mark.parametrize("name", NETS)
def test_forced_tolerance_retry(monkeypatch, name):
    """too few step attempts allowed per chunk: adaptive_solve! tightens the tolerances and retries"""
    pars = kp(name, maxiters=40)
    t, u, rc, st = solve(monkeypatch, name, pars)
    print(f"{name}: rc {rc} retries {st['n_retries']} final tolerances {st['final_abstol']:.1e} {st['final_reltol']:.1e}")
    assert st["n_retries"] >= 1
    assert st["final_abstol"] <= pars.abstol / 10 and st["final_reltol"] <= pars.reltol / 10
    assert st["final_abstol"] == pytest.approx(pars.abstol / 10 ** st["n_retries"]) and st["final_reltol"] == pytest.approx(pars.reltol / 10 ** st["n_retries"])
