"""The solve driver's schedule (kinetica_jl_amd/csrc/resident_core.hpp: res_drive), pinned in every integrator it drives: the
host-driven Solver (KIN_RESIDENT=0), the resident kernel, and the CPU replay of the kernel's controller (tests/res_host.py) where
the case can be expressed there. What is pinned is what the driver decides, not what the integrator computes: the save times
(exactly), the row count, the return code, and n_chunks / n_restarts / n_retries as integers; the values only have to be the
solution, A(t) = exp(-int k) piecewise, within the usual 100 tolerance units.

Two first-order networks whose first species decays with the rate constant in force: A -> B, and the chain A -> B -> C (second
rate constant 2 throughout). Chunks of 0.5 over (0, 1) unless a case says otherwise.

n_restarts counts every segment start, warm ones (solve_chunks = 2: Solver::resume_chunk, ResidentBdf::resume) included - as
tests/test_gpu_resident.py::test_warm_chunk_continuation_in_all_three_drivers has it (10 warm chunks, 10 restarts) - so it is the
number of segments in both chunk modes; what a warm chunk start saves shows in the step count
(test_warm_chunk_starts_follow_the_rate_changes)."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists

pytestmark = pytest.mark.gpu

NETS = {"a_to_b": from_lists(2, [[(0, 1)]], [[(1, 1)]]),
        "chain3": from_lists(3, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(2, 1)]])}
DRIVERS = ("host", "resident", "replay")
MAXITERS = 1      # KIN_RETCODE_MAXITERS


def rate_rows(net_name, k):
    return np.array([[ki] if net_name == "a_to_b" else [ki, 2.0] for ki in k])


def kp(span=(0.0, 1.0), mode=1, chunk=0.5, save=0.25, **kw):
    d = dict(tspan0=span[0], tspan1=span[1], abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=mode, ban_negatives=0,
             solve_chunkstep=chunk, maxiters=100000, save_interval=-1.0 if save is None else save, dtmin=0.0)
    d.update(kw)
    return capi.KinParams(**d)


def errscale(u, ref, abstol=1e-10, reltol=1e-8):
    return (np.abs(u - ref) / (abstol + reltol * np.abs(ref))).max()


def decay(t, t0, tstops, k):
    """A(t) of A' = -k(t) A, A(t0) = 1: k[i] in force from tstops[i] on (zero-order hold), k[0] before tstops[1]"""
    edges = np.concatenate(([-np.inf], np.asarray(tstops, float)[1:], [np.inf])) if tstops is not None else np.array([-np.inf, np.inf])
    integral = sum(k[i] * np.clip(np.minimum(t, edges[i + 1]) - max(t0, edges[i]), 0.0, None) for i in range(len(k)))
    return np.exp(-integral)


@pytest.fixture(scope="module")
def handles():
    from tests.res_host import HostResident
    hs = {n: (capi.HipNetwork.from_flat(net), HostResident(net)) for n, net in NETS.items()}
    yield hs
    for h, hr in hs.values():
        h.close(); hr.close()


def solve(handles, monkeypatch, driver, net_name, pars, k, tstops=None):
    """(t, u, retcode, stats) of one solve; k: the first rate constant per stop (one value: static rates)"""
    h, hr = handles[net_name]
    u0 = np.zeros(NETS[net_name].n_species); u0[0] = 1.0
    rows = rate_rows(net_name, k)
    ts = None if tstops is None else np.asarray(tstops, float)
    if driver == "replay":
        t, u, rc, st = hr.solve(pars, u0, k0=rows[0]) if ts is None else hr.solve(pars, u0, tstops=ts, k_table=rows)
        return t, u, st["retcode"], st
    if driver == "host":
        monkeypatch.setenv("KIN_RESIDENT", "0")
    else:
        monkeypatch.delenv("KIN_RESIDENT", raising=False)
    if ts is None:
        h.set_rates(rows[0])
        t, u, rc, st, status = h.solve(pars, u0)
    else:
        t, u, rc, st, status = h.solve(pars, u0, tstops=ts, k_table=rows)
    assert status == (capi.KIN_OK if rc == 0 else capi.KIN_ERR_SOLVE_FAILED)
    assert (st["lu_slots"] > 64) == (driver == "host")        # the integrator that ran (the resident kernel's cache: 64 slots at most)
    return t, u, rc, st


GRID = [0.0, 0.25, 0.5, 0.75, 1.0]
# name: (kp arguments, tstops, k per stop, save times, n_chunks, segments)
CASES = {
    "stop_on_a_chunk_boundary": (dict(), [0.0, 0.5], [1.0, 4.0], GRID, 2, 2),
    "stop_inside_a_chunk": (dict(), [0.0, 0.3], [1.0, 4.0], GRID, 2, 3),
    "two_stops_inside_one_chunk": (dict(), [0.0, 0.1, 0.4], [1.0, 4.0, 2.0], GRID, 2, 4),
    "stop_at_zero": (dict(), [0.0], [3.0], GRID, 2, 2),
    "stops_at_and_beyond_the_end_are_ignored": (dict(), [0.0, 1.0, 5.0], [1.0, 9.0, 9.0], GRID, 2, 2),
    "static_rates_save_interval_divides_the_chunk": (dict(), None, [1.0], GRID, 2, 2),
    # collect(0:0.2:0.5) = [0, 0.2, 0.4]: each chunk's last local point is dropped, except on the final chunk
    "save_interval_does_not_divide_the_chunk": (dict(save=0.2), None, [1.0], [0.0, 0.2, 0.5, 0.7, 0.9], 2, 2),
    "stop_inside_a_chunk_off_the_save_grid": (dict(save=0.2), [0.0, 0.3], [1.0, 4.0], [0.0, 0.2, 0.5, 0.7, 0.9], 2, 3),
    # complete timespan (solve_chunks = 0): one chunk in global time
    "complete_timespan_with_stops": (dict(mode=0), [0.0, 0.3, 0.6], [1.0, 4.0, 2.0], GRID, 1, 3),
    # ... whose stops before tspan0 have passed at the start: the rates of stop 1 are in force from 0.5 on
    "stop_before_tspan0": (dict(mode=0, span=(0.5, 1.5)), [0.0, 0.2, 1.0], [1.0, 4.0, 2.0], [0.5, 0.75, 1.0, 1.25, 1.5], 1, 2),
}
CASE_MODES = [(c, m) for c, v in CASES.items() for m in ((0,) if v[0].get("mode") == 0 else (1, 2))]


@pytest.mark.parametrize("net_name", list(NETS))
@pytest.mark.parametrize("case,mode", CASE_MODES)
def test_schedule(handles, monkeypatch, net_name, case, mode):
    args, tstops, k, grid, n_chunks, segments = CASES[case]
    pars = kp(**dict(args, mode=mode))
    for driver in DRIVERS:
        t, u, rc, st = solve(handles, monkeypatch, driver, net_name, pars, k, tstops)
        print(f"{case} mode {mode} {net_name} {driver}: rows {len(t)} rc {rc} chunks {st['n_chunks']} restarts {st['n_restarts']} "
              f"retries {st['n_retries']} steps {st['n_steps']} errscale {errscale(u[:, 0], decay(t, pars.tspan0, tstops, k)) if len(t) == len(grid) else -1:.2f}")
        assert rc == 0 and len(t) == len(grid), driver
        np.testing.assert_allclose(t, grid, rtol=0, atol=1e-15, err_msg=driver)
        assert (st["n_chunks"], st["n_restarts"], st["n_retries"]) == (n_chunks, segments, 0), driver
        assert errscale(u[:, 0], decay(t, pars.tspan0, tstops, k)) < 100, driver
        # every reaction conserves the sum, and so do the corrector's linear solves and the dense output, to rounding
        np.testing.assert_allclose(u.sum(axis=1), 1.0, rtol=1e-11, err_msg=driver)


@pytest.mark.parametrize("net_name", list(NETS))
def test_warm_chunk_starts_follow_the_rate_changes(handles, monkeypatch, net_name):
    """solve_chunks = 2, four chunks of 0.25: static rates make three warm chunk starts; with a rate update at 0.5 the starts at 0.25
    and 0.75 are warm and the one at 0.5 re-initialises. Same rows as solve_chunks = 1, a segment start counted per chunk, fewer
    steps."""
    for driver in DRIVERS:
        steps = {}
        for name, tstops, k in (("static", None, [1.0]), ("update", [0.0, 0.5], [1.0, 4.0])):
            for mode in (1, 2):
                t, u, rc, st = solve(handles, monkeypatch, driver, net_name, kp(mode=mode, chunk=0.25), k, tstops)
                assert rc == 0 and (st["n_chunks"], st["n_restarts"], st["n_retries"]) == (4, 4, 0), (driver, name, mode)
                np.testing.assert_allclose(t, GRID, rtol=0, atol=1e-15)
                assert errscale(u[:, 0], decay(t, 0.0, tstops, k)) < 100, (driver, name, mode)
                steps[name, mode] = st["n_steps"]
        print(f"{net_name} {driver}: steps {steps}")
        assert steps["static", 2] < steps["static", 1] and steps["update", 2] < steps["update", 1], (driver, steps)


# the first chunk (k = 0.01, integrated once, at the default tolerances) takes 22 step attempts on A -> B and 42 on the chain in
# the CPU replay; the second (k = 200) needs 244 for its first save point at 0.75, more at tighter tolerances: maxiters = 60 ends
# every attempt of the second chunk before it saved anything but its first row
SLOW_THEN_FAST = ([0.0, 0.5], [0.01, 200.0])


@pytest.mark.parametrize("net_name", list(NETS))
@pytest.mark.parametrize("adaptive", (True, False))
def test_maxiters_inside_the_second_chunk(handles, monkeypatch, net_name, adaptive):
    """adaptive_solve!: MaxIters in the second chunk is retried at tolerances / 10, five attempts in all, each from the chunk's
    start with the rows of the attempt before taken back; without adaptive_tols there is one attempt. MaxIters is an ordinary
    return code."""
    tstops, k = SLOW_THEN_FAST
    pars = kp(maxiters=60, adaptive_tols=int(adaptive))
    for driver in DRIVERS:
        t, u, rc, st = solve(handles, monkeypatch, driver, net_name, pars, k, tstops)
        print(f"{net_name} {driver} adaptive {adaptive}: rows {len(t)} rc {rc} chunks {st['n_chunks']} restarts {st['n_restarts']} retries "
              f"{st['n_retries']} steps {st['n_steps']} tols {st['final_abstol']:.3e} {st['final_reltol']:.3e}")
        assert rc == MAXITERS and st["n_chunks"] == 2, driver
        # chunk 0: rows 0 and 0.25 (its last local point is the next chunk's first); chunk 1: its first row, once
        assert len(t) == 3, driver
        np.testing.assert_allclose(t, [0.0, 0.25, 0.5], rtol=0, atol=1e-15, err_msg=driver)
        assert errscale(u[:, 0], decay(t, 0.0, tstops, k)) < 100, driver
        if adaptive:
            assert (st["n_retries"], st["n_restarts"]) == (4, 1 + 5), driver
            assert st["final_abstol"] == pytest.approx(1e-14, rel=1e-12) and st["final_reltol"] == pytest.approx(1e-12, rel=1e-12), driver
        else:
            assert (st["n_retries"], st["n_restarts"]) == (0, 1 + 1), driver
            assert (st["final_abstol"], st["final_reltol"]) == (1e-10, 1e-8), driver


@pytest.mark.parametrize("net_name", list(NETS))
def test_every_step_is_saved_without_a_grid(handles, monkeypatch, net_name):
    """save_interval < 0 without chunks (saveat = []), host-driven path only (the others need a grid): the first row is the
    initial state at tspan0, then one row per accepted step, the last at tspan1; a segment ends on a step, so the stop is a row."""
    tstops, k = [0.0, 0.5], [1.0, 4.0]
    pars = kp(span=(0.25, 1.0), mode=0, save=None)
    t, u, rc, st = solve(handles, monkeypatch, "host", net_name, pars, k, tstops)
    print(f"{net_name}: rows {len(t)} steps {st['n_steps']} restarts {st['n_restarts']}")
    assert rc == 0 and (st["n_chunks"], st["n_restarts"], st["n_retries"]) == (1, 2, 0)
    assert len(t) == st["n_steps"] + 1 and t[0] == 0.25 and t[-1] == 1.0 and np.all(np.diff(t) > 0) and 0.5 in t
    assert np.array_equal(u[0], [1.0] + [0.0] * (u.shape[1] - 1))
    assert errscale(u[:, 0], decay(t, 0.25, tstops, k)) < 100
    np.testing.assert_allclose(u.sum(axis=1), 1.0, rtol=1e-11)
