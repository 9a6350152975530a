"""GPU tests of the resident kernel's own copies of the BDF step (kinetica_jl_amd/csrc/resident.hip: ph_vec, ph_save_y, set_time,
ph_norms, ph_init_D, predict_body, ph_change_D, ph_accept, ph_interp, newton_body's update and five sums; resident_core.hpp:
res_corrector_loop, and the controller's device-built change_D matrix and interpolation weights), each run ONCE through
kin_step_probe's paths 3 (default build) and 4 (shared-CU build: 128 registers, phases inlined) and compared with the
extended-precision references of tests/step_cases.py - never with another device path, never with the CPU replay. The probe runs
an operation the way resident_bdf_kernel does: wavefront 0 builds the controller and calls its (or the backend's) method, which
posts the command; wavefronts 1-7 decode it in worker_loop. What an operation writes is compared within the bound derived next
to its reference, everything else the probe returns - the other rows of the member's block, the rows of D above those the
operation may touch (a sentinel), the other fields of the control block, the other members' blocks - bit for bit. Every launch
asserts from the probe's `info` the shape it is named after (species, trips of a 512-stride loop and wavefronts owning a species
as the KERNEL counted them, the build; the nonlinear case its dense block and fused solve form).

The cases, their construction and the bounds of the solve and of a whole attempt: tests/resident_step_cases.py (shared with
tests/test_resident_step_host.py, which runs the same tables against the CPU replay's backend).

Measured on one MI355X, largest error / bound per case group (printed at the end of the module, pytest -s); the file takes 5 s
(121 tests; paths 3 and 4 gave the same figures to the digits shown):
  init_D 0.49, predict 0.61, accept 0.70, change_D 0.11 (the device-built matrix: step_cases.ref_change_D's count holds
  unchanged), interp 0.21, vec 0.33, norms 0.25; one iteration on pairs: backward error 0.010 of BWD_MAX, update 0.33, raw sums
  0.15; nonlinear (synthetic 300, m > 0, fused): residual system entry by entry 0.15, update 0.33, sums 0.005; whole attempts 0.33;
  three members in one launch 0.62 (elementwise), 0.32 (attempts). The CPU replay on the same tables
  (tests/test_resident_step_host.py): the same figures but predict / attempt 0.61 and vec 0.59 (no fused multiply-add).
  No kernel was found wrong, and nothing in the replay or the shared rules.

Mutation check (one change at a time on a scratch build of the four resident translation units, selected through KIN_LIB_PATH,
nothing of it kept; every mutation keeps index ranges and barriers): which tests of this file fail, and what
test_gpu_resident.py + test_gpu_ensemble_continuous.py + test_gpu_ensemble_discrete.py (27 tests) did. The counts are of the
101 tests the file had then: test_one_corrector_iteration_with_non_finite_inputs and the non-finite cases of the nonlinear test
and of whole_attempt (nonfinite_update_inf, nonfinite_state_nan) were added afterwards and have not been run under the mutations.
The table is NOT complete for the trajectory files: under mutation 5 their run was cut at its time limit, under 6 it was not made.
  1 newton_body reads D[order - 1] in the order - 1 sum: 22 fail - one_corrector_iteration_on_pairs (16: every size, both paths),
    _nonlinear (2), three_members_in_one_launch (4). The 27 trajectory tests: all passed.
  2 newton_body uses ec for ec_p: 44 fail - the 22 of mutation 1 and whole_attempt, every converged case on both paths (22).
    Trajectory tests: all passed.
  3 worker_loop decodes OP_PREDICT with d1, d2 swapped (the leader's call unchanged): 16 fail - elementwise_phases_every_order at
    n = 65, 511, 512, 513, 1024, 1025 on both paths (12) and three_members_in_one_launch (4); n = 2 and 64 PASS: there wavefront 0
    owns every species and no worker decodes anything that is stored. The failure exists only because the probe runs the real
    dispatch - a probe calling ph_predict directly cannot see it. Trajectory tests: all passed.
  4 worker_loop passes with_f1 = false for OP_NORMS: 14 fail - first_step_norms at n >= 65 on both paths (12; n = 2, 64 pass, as
    above: the real dispatch again), three_members_in_one_launch at 1025 (2). Trajectory tests: all passed.
  5 ph_change_D reads ru[a * 6 + q]: 22 fail - elementwise_phases_every_order everywhere (16), three_members_in_one_launch (4),
    arguments_are_rejected_... (2: the solve behind the probes is not the parent's any more). Trajectory tests: 12 of the first 14
    had failed when the run reached its 240 s limit (the integrator grinds); not taken further, and no mutated trajectory
    run was started after it.
  6 ph_accept omits row order + 2: 20 fail - elementwise_phases_every_order everywhere (16), three_members_in_one_launch (4). Trajectory tests: not run (see 5).
  7 ph_interp ignores `row`: 20 fail - elementwise_phases_every_order everywhere (16), three_members_in_one_launch (4).
    Trajectory tests: 7 failed (solution rows land in row 0), 20 passed.
  8 res_corrector_loop tests rate > rate_max: NO test of this file fails (all 101 pass) - the two differ only at rate == rate_max
    exactly, which no computed update reaches. tests/test_resident_step_host.py, which compiles the same header, fails
    test_corrector_loop_diverges_at_a_rate_equal_to_rate_max (scripted sums: 1/2, 1/8, rate_max 1/4). Trajectory tests: all passed.
  9 the deep-negative mark is lost (1.0 instead of RES_NEG_MARK): 24 fail - one_corrector_iteration_on_pairs (16), _nonlinear
    (2), three_members_in_one_launch (4), whole_attempt deep_negative (2). Trajectory tests: all passed."""
import time

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from tests import linalg_cases as lc
from tests import resident_step_cases as rc
from tests import step_cases as sc
from tests.step_cases import ROW

pytestmark = pytest.mark.gpu

PATHS = (3, 4)
_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for hh, _ in _HANDLES.values():
        hh.close()
    _HANDLES.clear()
    if rc.MEASURED:
        print("\nresident step probe: largest error / bound per case group")
        for group, v in sorted(rc.MEASURED.items()):
            print(f"  {group:44s} {v:.3f}")
        print(f"  wall {time.time() - t0:.0f} s")


def pair_handle(n):
    if n not in _HANDLES:
        net = rc.pair_net(n)
        hh = capi.HipNetwork.from_flat(net)
        hh.set_rates(rc.pair_rates(n))
        _HANDLES[n] = (hh, rc.Net(net, rc.pair_rates(n)))
    return _HANDLES[n]


def check_info(info, n, path, **more):
    want = dict(rc.expected_shape(n), waves_per_eu=2 if path == 3 else 4, **more)
    assert {q: info[q] for q in want} == want, (info, want)
    assert info["dyn_lds"] > 0


def runner(hh, path, n, **more):
    """one member through path 3 / 4; every launch asserts the shape it reached"""
    def run(op, st, ctrl, entry):
        out = hh.step_probe(path, op, st, ctrl, entry)
        check_info(out["info"], n, path, **more)
        assert out["seq"] == 0 and np.all(np.isnan(out["pub"][:10])) and np.all(out["pub"][10:] == -1)      # nothing is published
        return out["state"], out["ctrl"]
    return run


# ------------------------------------------------------------------------------------------------------ elementwise phases
@pytest.mark.parametrize("n", rc.SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_elementwise_phases_every_order(path, n):
    """init_D, predict (ctl->predict()), accept, change_D (matrix built on the device) at every factor, interp (weights built on
    the device) into both solution rows with its time - orders 1 to 5"""
    hh, _ = pair_handle(n)
    rc.check_elementwise(runner(hh, path, n), n, f"path {path} ")


@pytest.mark.parametrize("n", rc.SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_vector_operations_and_saves(path, n):
    """the six VecOps (the clipped copy keeps NaN and -0.0), save_y into both solution rows, set_time"""
    hh, _ = pair_handle(n)
    rc.check_vec(runner(hh, path, n), n, f"path {path} ")


@pytest.mark.parametrize("n", rc.SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_first_step_norms(path, n):
    """with and without f1; NaN / Inf in f0, f1 and y"""
    hh, _ = pair_handle(n)
    rc.check_norms(runner(hh, path, n), n, f"path {path} ")


# ------------------------------------------------------------------------------------------------------- one iteration
@pytest.mark.parametrize("n", rc.SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_one_corrector_iteration_on_pairs(path, n):
    """SUM_CASES (orders 1, 3, 5; upd 1 and 0.8; no, a shallow, a deep negative entry) with the slot factorised at c and at
    another c_fact: the x the iteration used as a solution of its own residual system, then y, d and the five raw sums (the
    analysis eliminates every pair: no dense block, except for the single pair of n = 2, which is one)"""
    hh, N = pair_handle(n)
    for i, (order, upd, negative) in enumerate(sc.SUM_CASES):
        for c_fact in (rc.PAIR_C, 0.75 * rc.PAIR_C):
            st, entry = rc.newton_case(N, 5000 + 10 * n + i, order, upd, negative, rc.PAIR_C, c_fact, pairs=True)
            rc.check_newton(runner(hh, path, n, m=1 if n == 2 else 0), N, st, entry, negative, True, f"path {path} ")


@pytest.mark.parametrize("n", rc.SIZES)
@pytest.mark.parametrize("path", PATHS)
def test_one_corrector_iteration_with_non_finite_inputs(path, n):
    """psi = Inf / NaN (a non-finite update on a finite state: s Inf / NaN, se non-finite), y = Inf / NaN on the inert species
    (odd n; se exactly +inf for the infinite state under a finite update): the raw sums newton_body returns, orders 1, 3, 5"""
    hh, N = pair_handle(n)
    rc.check_newton_plants(runner(hh, path, n, m=1 if n == 2 else 0), N, 8000 + 10 * n, True, f"path {path} ")


def N_dense(hh, n):
    """the dense block the handle's analysis leaves (from the linear-algebra probe's info: what `m` of this probe must repeat)"""
    return hh.resident_probe(np.ones((1, n)), np.array([1e-3]), np.ones((1, n)))["info"]["m"]


@pytest.mark.parametrize("path", PATHS)
def test_one_corrector_iteration_nonlinear(path):
    """synthetic_crn(300, 1500): the fused solve form with a dense block, Jacobian at a state of its own (row 26)"""
    net, _, _ = synthetic_crn(300, 1500)
    hh, on, k = lc.static_handle(net, 5, lo=0.0, hi=2.0)
    try:
        N = rc.Net(net, k)
        seen = {}

        def run(op, st, ctrl, entry):
            out = hh.step_probe(path, op, st, ctrl, entry)
            check_info(out["info"], 300, path, solve_form=0)
            seen.update(out["info"])
            return out["state"], out["ctrl"]
        for i, (order, upd, negative) in enumerate(sc.SUM_CASES):
            for c_fact in (1e-3, 0.75e-3):
                st, entry = rc.newton_case(N, 900 + i, order, upd, negative, 1e-3, c_fact, pairs=False)
                rc.check_newton(run, N, st, entry, negative, False, f"path {path} nonlinear ")
        rc.check_newton_plants(run, N, 950, False, f"path {path} nonlinear ")
        assert seen["m"] > 0 and seen["m"] == N_dense(hh, 300), seen
    finally:
        hh.close()


# --------------------------------------------------------------------------------------------------------- whole attempts
@pytest.mark.parametrize("name", rc.ATTEMPT_CASES)
@pytest.mark.parametrize("path", PATHS)
def test_whole_attempt(path, name):
    """b.corrector(in): predictor, iterations and their decisions in one command - one case per branch an attempt can reach
    (resident_step_cases.ATTEMPT_CASES), at every size; branch sequence, n_iter, flags, crate, err*, y, d, psi, scale"""
    for n in rc.attempt_sizes(name):
        hh, _ = pair_handle(n)
        rc.check_attempt(runner(hh, path, n), n, name, f"path {path} ")


# ----------------------------------------------------------------------------------------------------- members of a launch
MEMBER_ATTEMPTS = ("refused_crate_then_rate", "converged_first_tol", "diverged_estimate")


@pytest.mark.parametrize("n", (65, 1025))
@pytest.mark.parametrize("path", PATHS)
def test_three_members_in_one_launch(path, n):
    """K = 3 workgroups with different states, orders, factors, tolerances and control blocks, the entries listed in reverse:
    every member's block against its own reference (per-member addressing through ResTrajDev and the argument list)"""
    hh, N = pair_handle(n)
    K = 3
    g = f"path {path} members "
    for op in ("predict", "accept", "change_D", "init_D", "norms", "interp", "newton", "corrector"):
        states, entries, ctrls = [], [], []
        for m in range(K):
            if op == "newton":
                o, upd, negative = sc.SUM_CASES[m]
                st, e = rc.newton_case(N, 300 + m, o, upd, negative, rc.PAIR_C, (1.0, 0.75, 1.25)[m] * rc.PAIR_C, pairs=True)
            elif op == "corrector":
                st, e = rc.attempt_case(n, MEMBER_ATTEMPTS[m], seed=m)
            else:
                st = sc.make_state(n, 500 + 10 * n + m)
                e = dict(order=1 + (2 * m + 1) % 5, atol=10.0 ** -(10 + m), rtol=10.0 ** -(6 + m), h=sc.FACTORS[m],
                         aux=m % 2 if op in ("init_D", "norms") else 0, row=m % 2, **sc.INTERP_T)
            states.append(st); entries.append(e)
            ctrls.append(sc.dirty_ctrl() if op in ("newton", "corrector") else sc.dirty_ctrl(crate=0.1 * (m + 1)))
        out = hh.step_probe(path, op, np.stack(states), np.stack([sc.ctrl_array(c) for c in ctrls]),
                            [dict(entries[m], member=m) for m in reversed(range(K))])
        check_info(out["info"], n, path)
        for m in range(K):
            got, gc, st, e, what = out["state"][m], out["ctrl"][m], states[m], entries[m], (op, "member", m)
            member = lambda op_, st_, ct_, e_: (got, gc)          # the member's part of the one launch, for the shared checks
            if op == "newton":
                rc.check_newton(member, N, st, e, sc.SUM_CASES[m][2], True, g)
                continue
            if op == "corrector":
                rc.check_attempt(member, n, MEMBER_ATTEMPTS[m], g, seed=m)
                continue
            D = st[:8]
            refs, crefs = {
                "predict": lambda: (sc.ref_predict(D, e["order"], e["atol"], e["rtol"]), {}),
                "accept": lambda: (sc.ref_accept(D, st[ROW["d"]], e["order"]), {}),
                "change_D": lambda: (sc.ref_change_D(D, e["order"], e["h"]), {}),
                "init_D": lambda: (sc.ref_init_D(st[ROW["ytmp" if e["aux"] else "y"]], st[ROW["f0"]], e["h"]), {}),
                "norms": lambda: ({}, sc.ref_norms(st[ROW["y"]], st[ROW["f0"]], st[ROW["f1"]] if e["aux"] else None, e["atol"], e["rtol"])),
                "interp": lambda: ({ROW["out"] + e["row"]: sc.ref_interp(D, e["order"], **sc.INTERP_T)[ROW["out"]]},
                                   {f"scratch{e['row']}": (sc.INTERP_T["ts"], None)}),
            }[op]()
            rc.check_state(g, got, st, refs, what)
            rc.check_ctrl(g, gc, ctrls[m], crefs, what)


# --------------------------------------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("path", PATHS)
def test_arguments_are_rejected_before_any_launch_and_leave_the_handle_as_it_was(path, monkeypatch):
    """order outside 1 .. 5, solution row outside {0, 1}, n that is not the handle's, a member out of range, an unknown operation:
    KIN_ERR_INVALID_ARG; an operation the path does not have (and CORRECTOR on paths 0 and 2): KIN_ERR_UNSUPPORTED; a resident solve
    afterwards is bit for bit that of a fresh handle"""
    net, Ea, A = synthetic_crn(300, 1500)
    u0 = np.zeros(300); u0[0] = 1.0
    pars = capi.KinParams(tspan0=0.0, tspan1=2e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                          ban_negatives=0, solve_chunkstep=1e-3, maxiters=100000, save_interval=-1.0)
    res = []
    for with_probe in (False, True):
        hh = capi.HipNetwork.from_flat(net)
        hh.set_arrhenius(Ea, A, k_max=1e12)
        hh.rates_at(1000.0)
        if with_probe:
            first = hh.solve(pars, u0)
            st = sc.make_state(300, 3)
            ct = sc.ctrl_array(sc.clean_ctrl())
            good = dict(order=2, atol=1e-10, rtol=1e-8)

            def code(*a, **kw):
                with pytest.raises(capi.KineticaHipError) as e:
                    hh.step_probe(*a, **kw)
                return e.value.code
            assert code(path, "predict", st, ct, dict(good, order=0)) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "predict", st, ct, dict(good, order=6)) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "interp", st, ct, dict(good, row=2, **sc.INTERP_T)) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "interp", st, ct, dict(good, row=-1, **sc.INTERP_T)) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "predict", sc.make_state(301, 3), ct, good) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "predict", st, ct, dict(good, member=1)) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "predict", np.stack([st, st]), np.stack([ct, ct]), [dict(good, member=0), dict(good, member=0)]) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "predict", np.stack([st, st]), np.stack([ct, ct]), [dict(good, member=0)]) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "vec", st, ct, dict(good, aux=capi.STEP_VEC_OPS["interp"])) == capi.KIN_ERR_INVALID_ARG
            assert code(path, "vec", st, ct, dict(good, aux=9)) == capi.KIN_ERR_INVALID_ARG
            monkeypatch.setitem(capi.STEP_OPS, "bogus", 12)
            assert code(path, "bogus", st, ct, good) == capi.KIN_ERR_INVALID_ARG
            for op in ("accept_predict", "rk_combine", "rk_error"):
                assert code(path, op, st, ct, dict(good, aux=1)) == capi.KIN_ERR_UNSUPPORTED
            assert code(0, "corrector", st, ct, good) == capi.KIN_ERR_UNSUPPORTED
            assert code(2, "corrector", st[None], ct[None], [dict(good, member=0)]) == capi.KIN_ERR_UNSUPPORTED
            # ... and real launches of both kinds, so the solve below meets a handle whose resident workspaces the probe resized
            out = hh.step_probe(path, "predict", st, ct, good)
            check_info(out["info"], 300, path)
            e = dict(order=1, atol=sc.ATOL, rtol=sc.RTOL, upd=1.0, c=1e-4, c_fact=1e-4, tol=sc.TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0,
                     dy_first_max=0.2, ec=sc.ERRC[1], ec_m=0.0, ec_p=sc.ERRC[2])
            st[ROW["u"]] = 10.0 ** np.random.default_rng(0).uniform(-6, 0, 300)
            hh.step_probe(path, "corrector", np.stack([st, st]), np.stack([ct, ct]), [dict(e, member=0), dict(e, member=1)])
        res.append(hh.solve(pars, u0))
        hh.close()
    (t0, us0, rc0, st0, _), (t1, us1, rc1, st1, _) = res
    assert rc0 == 0 and rc1 == 0 and np.array_equal(t0, t1) and np.array_equal(us0, us1)
    assert {q: v for q, v in st0.items() if q != "wall_seconds"} == {q: v for q, v in st1.items() if q != "wall_seconds"}
    assert np.array_equal(first[1], us0)


def test_rates_are_needed_for_the_corrector_operations_only():
    hh = capi.HipNetwork.from_flat(rc.pair_net(64))
    try:
        st = sc.make_state(64, 1)
        ct = sc.ctrl_array(sc.clean_ctrl())
        hh.step_probe(3, "accept", st, ct, dict(order=1))
        with pytest.raises(capi.KineticaHipError) as e:
            hh.step_probe(3, "newton", st, ct, dict(order=1, atol=1e-10, rtol=1e-8, upd=1.0, c=1e-3, c_fact=1e-3))
        assert e.value.code == capi.KIN_ERR_STATE
    finally:
        hh.close()
