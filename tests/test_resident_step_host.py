"""The CPU replay's backend (tests/native/resident_host.cpp: HostBackend, and ResidentBdf over it) operation by operation, without a
GPU: the case tables of tests/resident_step_cases.py - the ones tests/test_gpu_resident_step.py runs through the resident kernel -
against res_host_step_op, with the same references and bounds (tests/step_cases.py; BWD_MAX for the solve). The replay is what the
GPU-less suite trusts for step counts; its vector operations, norms, change_D / interp through the controller, its corrector
iteration and its whole attempt had not been compared with anything.

And res_corrector_loop (resident_core.hpp) alone: the second, sequential statement of newton_decide, run over a scripted backend
whose iterations return prescribed sums, against ref_decide chained iteration by iteration - every entry of
step_cases.DECISION_CASES an attempt can stand for (the attempt's own iteration limit, no rate taken from the control block, no
ban on negatives, no factorisation flag, not a launch behind a decision), with scripted iterations in front where the entry is a
later iteration, and the one branch no device case reaches: exhausted, at the exact equality of estimate and tolerance."""
import numpy as np
import pytest

from tests import res_host
from tests import resident_step_cases as rc
from tests import step_cases as sc
from tests.step_cases import LD

_NETS = {}


def host_net(n):
    if n not in _NETS:
        _NETS[n] = (res_host.HostResident(rc.pair_net(n)), rc.Net(rc.pair_net(n), rc.pair_rates(n)))
    return _NETS[n]


def runner(H, k):
    def run(op, st, ctrl, entry):
        if op == "vec" and entry["aux"] >= 6:
            op = {6: "save_y", 8: "set_time"}[entry["aux"]]
        out = H.step_op(op, st, ctrl, entry, k)
        assert out is not None, "arguments out of range"
        return out
    return run


@pytest.mark.parametrize("n", rc.SIZES)
def test_replay_elementwise_phases(n):
    H, N = host_net(n)
    rc.check_elementwise(runner(H, N.k), n, "replay ")
    rc.check_vec(runner(H, N.k), n, "replay ")
    rc.check_norms(runner(H, N.k), n, "replay ")


@pytest.mark.parametrize("n", rc.SIZES)
def test_replay_one_corrector_iteration(n):
    """SUM_CASES at every size, the slot factorised at c and at another c_fact"""
    H, N = host_net(n)
    for i, (order, upd, negative) in enumerate(sc.SUM_CASES):
        for c_fact in (rc.PAIR_C, 0.75 * rc.PAIR_C):
            st, entry = rc.newton_case(N, 5000 + 10 * n + i, order, upd, negative, rc.PAIR_C, c_fact, pairs=True)
            rc.check_newton(runner(H, N.k), N, st, entry, negative, True, "replay ")


@pytest.mark.parametrize("n", rc.SIZES)
def test_replay_one_corrector_iteration_with_non_finite_inputs(n):
    """psi = Inf / NaN (a non-finite update on a finite state), y = Inf / NaN on the inert species (odd n): the raw sums as
    non-finite values, se exactly +inf for an infinite state under a finite update"""
    H, N = host_net(n)
    rc.check_newton_plants(runner(H, N.k), N, 8000 + 10 * n, True, "replay ")


def test_replay_one_corrector_iteration_nonlinear():
    """synthetic_crn(300, 1500), the nonlinear table of the GPU file: fused solve form with a dense block"""
    from kinetica_jl_amd.synth import synthetic_crn
    net, _, _ = synthetic_crn(300, 1500)
    k = rc.synthetic_rates(net)
    H, N = res_host.HostResident(net), rc.Net(net, k)
    assert H.info["m"] > 0 and H.info["solve_mode"] == 0, H.info
    for i, (order, upd, negative) in enumerate(sc.SUM_CASES):
        for c_fact in (1e-3, 0.75e-3):
            st, entry = rc.newton_case(N, 900 + i, order, upd, negative, 1e-3, c_fact, pairs=False)
            rc.check_newton(runner(H, k), N, st, entry, negative, False, "replay nonlinear ")
    rc.check_newton_plants(runner(H, k), N, 950, False, "replay nonlinear ")
    H.close()


@pytest.mark.parametrize("name", rc.ATTEMPT_CASES)
def test_replay_whole_attempt(name):
    for n in rc.attempt_sizes(name):
        H, N = host_net(n)
        rc.check_attempt(runner(H, N.k), n, name, "replay ")


def test_replay_rejects_arguments_out_of_range():
    H, N = host_net(64)
    st = sc.make_state(64, 1)
    for entry in (dict(order=0), dict(order=6), dict(row=2), dict(row=-1)):
        assert H.step_op("accept", st, sc.ctrl_array(sc.clean_ctrl()), entry) is None
    assert H.step_op("vec", st, sc.ctrl_array(sc.clean_ctrl()), dict(aux=6)) is None


# ------------------------------------------------------------------------------------------ res_corrector_loop, scripted
def flat_sums(n, dy, err=0.1):
    """the sums of an iteration whose update norm is dy: n equal terms"""
    t = np.full(n, LD(dy) ** 2); z = np.zeros(n, LD)
    e = np.full(n, LD(err) ** 2)
    return dict(s=(t, z), se=(e, z), sm=(e, z), sp=(e, z), neg=False, deep=False, neg_margin=1.0)


def script(sums_list):
    return [[float(q["s"][0].sum()), float(q["se"][0].sum()), float(q["sm"][0].sum()), float(q["sp"][0].sum()),
             rc.NEG_MARK if q["deep"] else 1.0 if q["neg"] else 0.0] for q in sums_list]


# iterations in front of a DECISION_CASES entry that is a later iteration: update norms that neither converge nor diverge and end
# at the entry's dy_norm_old (1 -> 0.35 -> 0.1: divergence estimates 0.023 / 0.011 <= 0.03 <= convergence estimates 0.19 / 0.04)
PRELUDES = {(1, 0.1): [0.1], (1, 1.0): [1.0], (3, 0.1): [1.0, 0.35, 0.1]}


def scripted_cases():
    out = []
    for name, (inp, ent, ct, _, _) in sc.DECISION_CASES.items():
        if {"maxit", "crate_from_ctrl", "ban_negatives", "publish_always"} & set(ent) or ct.get("lu_bad") or ct.get("newton_done"):
            continue
        out.append(name)
    return out


def check_scripted(n, sums_list, entry, what):
    want, branches, margins = rc.decide_chain(lambda it: sums_list[it], n, entry)
    assert not sc.margins_ok(margins, rel=1e-6), (what, sc.margins_ok(margins, rel=1e-6))
    a = res_host.corrector_loop(n, script(sums_list[:len(branches)] + [flat_sums(n, 7.0)]), tol=entry["tol"], rate_max=entry["rate_max"],
                                crate0=entry["crate0"], tol_first=entry["tol_first"], dy_first_max=entry["dy_first_max"])
    conv = bool(want["converged"][0])
    assert a["predicts"] == 1 and a["iterations"] == len(branches) and a["n_iter"] == len(branches), (what, branches, a)
    assert (a["done"], a["converged"], a["nonfinite"]) == (1, conv, float(want["nonfinite"][0])), (what, branches, a)
    neg = int(want["any_negative"][0]) if conv else 0
    assert (a["any_negative"], a["deep_negative"]) == (neg > 0, neg == 3), (what, a)
    for f, q in (("err", "err_norm"), ("err_m", "err_m_norm"), ("err_p", "err_p_norm")):
        ref = want[q] if conv else (LD(0), LD(0))
        assert rc.close("scripted loop", a[f], *ref), (what, f, a[f], float(ref[0]))
    cr, cb = want["crate"]
    assert rc.close("scripted loop", a["crate"], cr, LD(0) if cb is None else cb), (what, a["crate"], float(cr))
    return branches


@pytest.mark.parametrize("name", scripted_cases())
def test_corrector_loop_takes_the_decisions_of_the_reference(name):
    inp, ent, ct, branch, _ = sc.DECISION_CASES[name]
    for n in (257, 1025):
        st, xloc, e, ctrl = sc.decision_case(name, n=n, order=3, seed=n)
        sums = sc.ref_newton_sums(st[sc.ROW["x"]], st[sc.ROW["scale"]], st[sc.ROW["y"]], st[sc.ROW["d"]], st[:8], 3, 1.0, sc.ATOL, sc.RTOL)
        sums = {q: ((v[0], np.zeros_like(v[1])) if q in ("s", "se", "sm", "sp") else v) for q, v in sums.items()}    # handed over exactly
        it = e["iter"]
        prelude = [flat_sums(n, dy) for dy in PRELUDES[(it, ctrl["dy_norm_old"])]] if it else []
        entry = dict(tol=e["tol"], rate_max=e["rate_max"], crate0=ctrl["crate"] if it else e["crate0"], tol_first=-1.0 if it else e["tol_first"],
                     dy_first_max=e["dy_first_max"])
        # an entry that continues is followed by an update of a fiftieth of its norm, which converges by its rate
        tail = [flat_sums(n, 0.02 * inp["g"])] if branch.endswith("continue") else []
        branches = check_scripted(n, prelude + [sums] + tail, entry, (name, n))
        assert len(branches) == it + 1 + len(tail) and branches[it] == branch, (name, branches, branch)
        assert not tail or branches[-1] == "converged_rate", (name, branches)


def test_corrector_loop_diverges_at_a_rate_equal_to_rate_max():
    """rate >= rate_max, not >: update norms 1/2 and 1/8 (n = 64 equal terms: sums, quotient and square root are exact) give a rate
    of exactly rate_max = 1/4. With > the attempt would go on (divergence estimate 0.0026, convergence estimate 0.042)."""
    n = 64
    dys = (0.5, 0.125)
    for dy in dys:
        assert np.sqrt(float(flat_sums(n, dy)["s"][0].sum()) / n) == dy
    a = res_host.corrector_loop(n, script([flat_sums(n, dy) for dy in dys] + [flat_sums(n, 0.001)]), tol=0.03, rate_max=0.25, crate0=1.0,
                                tol_first=-1.0, dy_first_max=0.2)
    assert (a["done"], a["converged"], a["n_iter"], a["iterations"], a["nonfinite"]) == (1, 0, 2, 2, 0) and a["crate"] == 0.3, a
    c, branches, _ = rc.decide_chain(lambda it: flat_sums(n, dys[it]), n, dict(tol=0.03, rate_max=0.25, crate0=1.0, tol_first=-1.0, dy_first_max=0.2))
    assert branches == ["refused_crate_dymax_estimate_continue", "diverged_rate_max"] and float(c["crate"][0]) == 0.3


def test_corrector_loop_continues_and_exhausts():
    """the cases that continue, followed to a decision; and exhausted: four iterations, the last with rate / (1 - rate) dy == tol
    exactly (rate 1/2, dy = tol: neither above nor below)"""
    n = 64
    entry = dict(tol=0.03, rate_max=1.0, crate0=1.0, tol_first=-1.0, dy_first_max=0.2)
    b = check_scripted(n, [flat_sums(n, dy) for dy in (1.0, 0.2, 0.02)], entry, "continues")
    assert b == ["refused_crate_dymax_estimate_continue", "continue", "converged_rate"]
    # dy = tol exactly: s = n dy^2 must come back as dy from sqrt(s / n); 0.03125 = 2^-5 does
    tol = 0.03125
    e2 = dict(entry, tol=tol)
    dys = (8 * tol, 4 * tol, 2 * tol, tol)
    for dy in dys:
        assert np.sqrt(float(flat_sums(n, dy)["s"][0].sum()) / n) == dy
    a = res_host.corrector_loop(n, script([flat_sums(n, dy) for dy in dys]), tol=tol, rate_max=1.0, crate0=1.0, tol_first=-1.0, dy_first_max=0.2)
    assert (a["done"], a["converged"], a["n_iter"], a["iterations"], a["nonfinite"]) == (1, 0, 4, 4, 0) and a["crate"] == 0.5, a
    c, branches, _ = rc.decide_chain(lambda it: flat_sums(n, dys[it]), n, e2)
    assert branches[-1] == "exhausted" and not c["converged"][0]
