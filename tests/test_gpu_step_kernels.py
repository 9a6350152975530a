"""GPU tests of the vector kernels between the phases of a step and of the corrector's decision (solver_kernels.hip:
bdf_init_D / predict / accept / accept_predict / change_D / interp / norms / newton kernels, stagec_newton_kernel, rk_combine /
rk_error; ensemble_kernels.inc: e_vec / e_accept / e_change_D / e_init_D / e_norms / e_predict / e_newton; and the bodies both
sets of kernels call, step_dev.hpp: open_attempt, predict_elem, accept_elem, init_D_elem, interp_elem, norms_body, newton_pre /
newton_apply / newton_rows / newton_finish, newton_decide), each
run ONCE through kin_step_probe on constructed state and compared with the extended-precision references of
tests/step_cases.py - never with another device path. Everything the probe returns is compared: what an operation writes within
the bound derived next to its reference, everything else (the other buffers of the block, the rows of D above those the
operation may touch - filled with a sentinel -, the other fields of the control block, the members an entry list leaves out)
bit for bit. Flags and counters must be equal; every decision case asserts the branch of the decision it reached, every fused
case the task kinds of its stage-C plan (from the probe's `info`).

No plan has a one-wavefront row of more than 256 entries - build_seg_plan gives every row above SegPlanHost::SEG_LEN = 256
entries a whole workgroup, and seg_traverse (segsum_dev.hpp), which stagec_newton_kernel runs its rows through, asserts that bound
at compile time next to its one round of four entries per lane (the 16-entries-per-lane branch the kernels once carried for
longer rows was unreachable and is gone). The long-row path that test_corrector_update_fused_into_the_solve_and_separate mentions at
10 000 species is not reached there with the present analysis (stage C of synthetic_crn(10000, 50000): 54 ELL groups, 5 615
one-wavefront rows, longest 173, no whole-workgroup row). A sparse species gets a stage-C row above 256 entries only where the
elimination admits degrees above 256, i.e. from 4 000 species on (lu_options_for: max_degree 400): star_net below, 4 000
species, is the smallest such network of this suite (11 whole-workgroup rows, the 1024-thread build of the kernel).
A diverged attempt's y and d are not compared: the update is applied unconditionally and the next predictor rebuilds both
(solver_kernels.hip, above bdf_newton_kernel), so that state is never read.
Paths 0, 1 and 2 share the corrector's arithmetic since the bodies moved into step_dev.hpp; each path is still compared with the
references only.

Measured on one MI355X, largest error / bound per case group (printed at the end of the module, pytest -s); the file takes 7 s
(321 tests, the reports of the module's own clock and of pytest agree):
  predict 0.70, accept 0.70, accept_predict 0.71, init_D 0.50, change_D 0.11, interp 0.21 (paths 0 and 2 alike: the same
  operations in the same order), vec 0.33, norms 0.24, corrector sums / decision 0.33 (paths 0 and 2), members of a launch 0.64,
  the update inside the solve 0.32 - 0.33 (dense sweep, synthetic 300, star 4000), rk_combine 0.61, rk_error 0.03.
  No kernel was found wrong.

Mutation check (one change at a time on a scratch build, selected through KIN_LIB_PATH, nothing of it kept): which tests of this
file fail, and what test_gpu_solve.py + test_gpu_ensemble.py (23 tests) - the suite's view of these kernels before - did.
  1 bdf_newton_kernel reads D[order - 1] for the order - 1 sum: 79 fail - corrector_sums at orders 3 and 5 on both paths (52),
    every converged corrector_decision case (26), chained_iterations. Before: all 23 passed.
    With the one body (newton_pre reads D[order - 1]): 164 fail - corrector_sums at orders 3 and 5 on paths 0 and 2 (52 + 52),
    corrector_decision on both (26 + 22), chained_iterations (2), corrector_update_inside_the_solve (path 1, all 7),
    ensemble_entry_lists (3).
  2 error_const[order] in the order + 1 sum: 66 fail - corrector_sums at orders 1 and 3 (39), corrector_decision (26),
    chained_iterations. Before: 1 failed (test_c2_synthetic_matches_oracle, a trajectory comparison).
    With the one body (newton_apply uses ec for ec_p): 138 fail - corrector_sums at orders 1 and 3 on paths 0 and 2 (39 + 39),
    corrector_decision (26 + 22), chained_iterations (2), corrector_update_inside_the_solve (7), ensemble_entry_lists (3).
  3 newton_totals without the += 64 rounds: 10 fail - corrector_sums at n = 65537 (65 workgroups), all five cases on both paths;
    n = 65536 passes. Before: test_corrector_update_fused_into_the_solve_and_separate (2 cases).
  4 e_newton_kernel indexes reps[blockIdx.y]: 2 fail - ensemble_entry_lists K = 3 and 17 (K = 1 passes). Before: all 23 passed.
    The same two with the kernel as a wrapper of newton_rows.
  5 stagec_newton_kernel skips newton_apply in the dense block's last, partly filled wavefront: 5 fail -
    corrector_update_inside_the_solve dense 1, 63, 65, 129 and synthetic 300 (m = 108); dense 64 and star 4000 (m = 320) pass.
    Before: 6 failed (trajectory and step-count comparisons).
  6a newton_decide tests rate <= rate_max: 23 fail - corrector_decision every case with a rate (20), chained_iterations (2),
    undecided_launch_publishes_only_when_told_to. Before: 6 failed.
  6b newton_decide without the dy_first_max condition: 4 fail - corrector_decision first_refused_update_too_large (n = 257,
    1025, both paths). Before: 2 failed (test_c2_synthetic_matches_oracle, test_restart_rules_take_the_same_steps_...).
  7 bdf_accept_predict_kernel predicts from the column before the accept: 12 fail - accept_predict at every size (11),
    a_solve_after_the_probe (the solve no longer ends as before). Before: the two files did not finish within 400 s (the
    integrator stops advancing); not determined further."""
import time

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from tests import linalg_cases as lc
from tests import step_cases as sc
from tests.step_cases import LD, ROW

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    if MEASURED:
        print("\nstep probe: largest error / bound per case group")
        for group, v in sorted(MEASURED.items()):
            print(f"  {group:34s} {v:.3f}")
        print(f"  wall {time.time() - t0:.0f} s")


@pytest.fixture(scope="module")
def h():
    """paths 0 and 2 take only the device and the stream from the handle: any network will do"""
    hh = lc.static_handle(lc.pairs_net(4), 1)[0]
    yield hh
    hh.close()


# ------------------------------------------------------------------------------------------------------------------ helpers
def close(group, dev, ref, bound):
    """dev within bound of ref (equal non-finite values count as equal); records the largest error / bound"""
    dev = np.asarray(dev, LD); ref = np.asarray(ref, LD); bound = np.asarray(bound, LD)
    with np.errstate(invalid="ignore"):
        err = np.abs(dev - ref)
        ok = (dev == ref) | (err <= bound) | (np.isnan(dev) & np.isnan(ref))
        m = np.isfinite(err) & (bound > 0) & np.isfinite(bound)
        if np.any(m):
            MEASURED[group] = max(MEASURED.get(group, 0.0), float(np.max(err[m] / bound[m])))
    return bool(np.all(ok))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def check_state(group, got, given, refs, what):
    """rows in refs within their bound, every other row of the block as given, bit for bit"""
    for r in range(capi.STEP_ROWS):
        if r in refs:
            assert close(group, got[r], *refs[r]), (what, "row", r)
        else:
            assert same_bits(got[r], given[r]), (what, "row", r, "was touched")


def check_ctrl(group, got, given, refs, what):
    """fields in refs equal (bound None) or within their bound, every other field as given"""
    got, given = sc.ctrl_dict(got), sc.ctrl_dict(sc.ctrl_array(given))
    for f in sc.FIELDS:
        if f in refs and refs[f][1] is not None:
            assert close(group, got[f], *refs[f]), (what, f, got[f], float(refs[f][0]))
        else:
            want = float(refs[f][0]) if f in refs else given[f]
            assert got[f] == want or (np.isnan(got[f]) and np.isnan(want)), (what, f, got[f], want)


def unpublished(out):
    return out["seq"] == 0 and np.all(np.isnan(out["pub"][:10])) and np.all(out["pub"][10:] == -1)


def published(out, seq):
    return out["seq"] == seq and same_bits(out["pub"], out["ctrl"] if out["ctrl"].ndim == 1 else out["ctrl"][0])


def probe(h, path, op, st, ctrl, entry, xloc=None):
    """one member through path 0 / 1, or as a one-entry list through path 2; returns (state, ctrl, out)"""
    if path == 2:
        out = h.step_probe(2, op, st[None], sc.ctrl_array(ctrl)[None], [dict(entry, member=0)], xloc)
        return out["state"][0], out["ctrl"][0], out
    out = h.step_probe(path, op, st, sc.ctrl_array(ctrl), entry, xloc)
    return out["state"], out["ctrl"], out


PREDICT_CLEARS = {f: (0, None) for f in ("newton_done", "converged", "n_iter", "nonfinite", "any_negative", "ticket", "dy_norm_old",
                                         "dy_norm", "err_norm", "err_m_norm", "err_p_norm")}


def accept_predict_refs(st, ao, order, atol, rtol, copy_out):
    acc = sc.ref_accept(st[:8], st[ROW["d"]], ao)
    Dn = st[:8].astype(LD); Db = np.zeros_like(Dn)
    for j, (v, b) in acc.items():
        Dn[j], Db[j] = v, b
    refs = dict(acc)
    refs.update(sc.ref_predict(Dn, order, atol, rtol, D_bound=Db))
    if copy_out:
        refs[ROW["out"]] = acc[0]
    return refs


# ------------------------------------------------------------------------------------------------------ elementwise kernels
@pytest.mark.parametrize("n", sc.SIZES_ELEM)
@pytest.mark.parametrize("path", (0, 2))
def test_elementwise_operations_every_order(h, path, n):
    """init_D (from y and from ytmp), predict, accept (order 5 writes row 7; with and without copy_out), change_D, interp"""
    atol, rtol = 1e-10, 1e-8
    g = f"path {path} "
    for from_ytmp in (0, 1):
        st = sc.make_state(n, 11 * n + from_ytmp)
        got, gc, _ = probe(h, path, "init_D", st, sc.dirty_ctrl(), dict(aux=from_ytmp, h=0.375e-3))
        check_state(g + "init_D", got, st, sc.ref_init_D(st[ROW["ytmp" if from_ytmp else "y"]], st[ROW["f0"]], 0.375e-3), ("init_D", from_ytmp))
        check_ctrl(g + "init_D", gc, sc.dirty_ctrl(), {}, "init_D")
    for order in sc.ORDERS:
        seed = 100 * n + order
        # predict: reads rows 0 .. order, clears exactly the listed control fields (crate, lu_bad, spec_go, scratch stay)
        st = sc.make_state(n, seed, d_rows=order + 1)
        got, gc, _ = probe(h, path, "predict", st, sc.dirty_ctrl(), dict(order=order, atol=atol, rtol=rtol))
        check_state(g + "predict", got, st, sc.ref_predict(st[:8], order, atol, rtol), ("predict", order))
        check_ctrl(g + "predict", gc, sc.dirty_ctrl(), PREDICT_CLEARS, ("predict", order))
        # accept: rows 0 .. order + 2
        for copy_out in ((0, 1) if path == 0 else (0,)):
            st = sc.make_state(n, seed + 1, d_rows=order + 3)
            got, gc, _ = probe(h, path, "accept", st, sc.dirty_ctrl(), dict(order=order, copy_out=copy_out))
            refs = sc.ref_accept(st[:8], st[ROW["d"]], order)
            if copy_out:
                refs[ROW["out"]] = refs[0]
            check_state(g + "accept", got, st, refs, ("accept", order, copy_out))
            check_ctrl(g + "accept", gc, sc.dirty_ctrl(), {}, "accept")
        # change_D: rows 0 .. order (the ensemble's kernel rewrites rows up to 5 with the identity: the same bits)
        for factor in sc.FACTORS:
            st = sc.make_state(n, seed + 2, d_rows=order + 1)
            got, gc, _ = probe(h, path, "change_D", st, sc.dirty_ctrl(), dict(order=order, h=factor))
            check_state(g + "change_D", got, st, sc.ref_change_D(st[:8], order, factor), ("change_D", order, factor))
            check_ctrl(g + "change_D", gc, sc.dirty_ctrl(), {}, "change_D")
        # interp
        st = sc.make_state(n, seed + 3, d_rows=order + 1)
        got, gc, _ = probe(h, path, "interp", st, sc.dirty_ctrl(), dict(order=order, **sc.INTERP_T))
        check_state(g + "interp", got, st, sc.ref_interp(st[:8], order, **sc.INTERP_T), ("interp", order))
        check_ctrl(g + "interp", gc, sc.dirty_ctrl(), {}, "interp")


@pytest.mark.parametrize("n", sc.SIZES_ELEM)
def test_accept_predict(h, n):
    """the accept of a step of order ao and the predictor of order ao - 1, ao, ao + 1 in one launch; go absent, *go = 1, and
    *go = 0: nothing but newton_done = 1 changes"""
    atol, rtol = 1e-10, 1e-8
    for ao in sc.ORDERS:
        for order in (ao - 1, ao, ao + 1):
            if not 1 <= order <= 5:
                continue
            for go, copy_out in ((0, 0), (1, 1)):
                st = sc.make_state(n, 1000 * n + 10 * ao + order, d_rows=ao + 3)
                ctrl = sc.dirty_ctrl(spec_go=1)
                got, gc, _ = probe(h, 0, "accept_predict", st, ctrl, dict(order=order, aux=ao, atol=atol, rtol=rtol, go=go, copy_out=copy_out))
                check_state("accept_predict", got, st, accept_predict_refs(st, ao, order, atol, rtol, copy_out), ("accept_predict", ao, order, go))
                check_ctrl("accept_predict", gc, ctrl, PREDICT_CLEARS, ("accept_predict", ao, order, go))
        st = sc.make_state(n, 77 * n + ao, d_rows=ao + 3)
        ctrl = sc.dirty_ctrl(spec_go=0, newton_done=0)
        got, gc, _ = probe(h, 0, "accept_predict", st, ctrl, dict(order=ao, aux=ao, atol=atol, rtol=rtol, go=1, copy_out=1))
        check_state("accept_predict", got, st, {}, ("accept_predict held back", ao))
        check_ctrl("accept_predict", gc, ctrl, dict(newton_done=(1, None)), ("accept_predict held back", ao))


@pytest.mark.parametrize("n", sc.SIZES_ELEM)
def test_small_vector_operations_of_the_ensemble(h, n):
    st = sc.make_state(n, 31 * n)
    y, cs, D0, f0, outr = (st[ROW[q]].astype(LD) for q in ("y", "cs", "D", "f0", "out"))
    z = np.zeros(n, LD)
    axpy = y + LD(0.375) * f0
    cases = dict(load_u0={ROW["y"]: (outr, z)}, cs_from_y={ROW["cs"]: (y, z)}, y_from_cs_clipped={ROW["y"]: (np.where(cs < 0, 0, cs), z)},
                 y_from_d0={ROW["y"]: (D0, z)}, ytmp_from_d0={ROW["ytmp"]: (D0, z)}, save_y={ROW["out"]: (y, z)},
                 ytmp_axpy={ROW["ytmp"]: (axpy, 3 * sc.U * (np.abs(y) + np.abs(LD(0.375) * f0)))})     # a product and a sum
    for name, refs in cases.items():
        got, gc, _ = probe(h, 2, "vec", st, sc.dirty_ctrl(), dict(aux=capi.STEP_VEC_OPS[name], h=0.375))
        check_state("path 2 vec", got, st, refs, name)
        check_ctrl("path 2 vec", gc, sc.dirty_ctrl(), {}, name)


# ------------------------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("n", sc.SIZES_RED)
@pytest.mark.parametrize("path", (0, 2))
def test_first_step_norms(h, path, n):
    """without f1 (scratch[2] = 0), with f1, a NaN in f0 (flag set, the maximum ignores the entry), an Inf in f1"""
    atol, rtol = 1e-10, 1e-8
    for variant in ("no_f1", "f1", "nan_f0", "inf_f1"):
        st = sc.make_state(n, 7 * n + len(variant))
        if variant == "nan_f0":
            st[ROW["f0"], n // 2] = np.nan
        if variant == "inf_f1":
            st[ROW["f1"], n - 1] = np.inf
        with_f1 = variant != "no_f1"
        got, gc, _ = probe(h, path, "norms", st, sc.dirty_ctrl(), dict(aux=int(with_f1), atol=atol, rtol=rtol))
        ref = sc.ref_norms(st[ROW["y"]], st[ROW["f0"]], st[ROW["f1"]] if with_f1 else None, atol, rtol)
        check_state(f"path {path} norms", got, st, {}, variant)
        check_ctrl(f"path {path} norms", gc, sc.dirty_ctrl(), ref, (variant, n))
        assert sc.ctrl_dict(gc)["nonfinite"] == (variant in ("nan_f0", "inf_f1"))
        if variant == "nan_f0" and n > 1:
            assert np.isnan(sc.ctrl_dict(gc)["scratch1"]) and np.isfinite(sc.ctrl_dict(gc)["scratch3"])


# ------------------------------------------------------------------------------------------------------- corrector update
NEWTON_CASES = dict(sc.newton_case_list())


def check_newton(group, path, got, gc, out, st, ctrl, entry, expect_branch=None):
    sums, c, branch, done, margins = sc.newton_reference(st, entry, ctrl)
    assert not sc.margins_ok(margins), sc.margins_ok(margins)      # (tests/test_step_cases.py checks the listed cases without a GPU)
    if expect_branch is not None:
        assert branch == expect_branch, (branch, expect_branch)
    refs = {}
    if branch != "behind" and not branch.startswith(("diverged", "nonfinite")):
        refs = {ROW["y"]: sums["y"], ROW["d"]: sums["d"]}
    elif branch != "behind":
        got = got.copy(); got[ROW["y"]], got[ROW["d"]] = st[ROW["y"]], st[ROW["d"]]       # a diverged attempt's state is never read
    check_state(group, got, st, refs, branch)
    check_ctrl(group, gc, ctrl, c, branch)
    if path != 2:
        if branch != "behind" and (done or entry.get("publish_always")):
            assert published(out, entry["seq"]), (branch, out["seq"])
        else:
            assert unpublished(out), (branch, out["seq"], out["pub"])
    return branch, c


@pytest.mark.parametrize("path", (0, 2))
@pytest.mark.parametrize("cid", [c for c in NEWTON_CASES if c.startswith("sums")])
def test_corrector_sums(h, path, cid):
    """the five sums across the reduction sizes (orders 1, 3, 5: the guards of the order - 1 and order + 1 sums; upd = 1 and
    0.8; x scattered through a random permutation; no negative entry, a shallow one in the last workgroup's last element, a
    deep one): update norm, the three error norms, the negative mark, y and d"""
    st, xloc, entry, ctrl = NEWTON_CASES[cid]()
    got, gc, out = probe(h, path, "newton", st, ctrl, entry, xloc)
    branch, c = check_newton(f"path {path} newton sums", path, got, gc, out, st, ctrl, entry, "converged_first_tol")
    want_neg = 1 if "shallow" in cid else 3 if "deep" in cid else 0
    assert sc.ctrl_dict(gc)["any_negative"] == want_neg and sc.ctrl_dict(gc)["converged"] == 1


def decision_params():
    """every decision case on path 0; on path 2 those the ensemble's kernel has the arguments for (its iteration limit is fixed,
    it takes no carried rate from the control block and no ban on negatives)"""
    out = []
    for cid in NEWTON_CASES:
        if cid.startswith("sums"):
            continue
        ent = sc.DECISION_CASES[cid.split("-n")[0]][1]
        out.append((0, cid))
        if not {"maxit", "crate_from_ctrl", "ban_negatives"} & set(ent):
            out.append((2, cid))
    return out


@pytest.mark.parametrize("path, cid", decision_params())
def test_corrector_decision(h, path, cid):
    """every branch of newton_decide, reached by a constructed update and asserted as reached; crate, spec_go term by term,
    publication exactly when the launch decided (path 0); a launch behind a decision changes nothing and publishes nothing"""
    st, xloc, entry, ctrl = NEWTON_CASES[cid]()
    name = cid.split("-n")[0]
    got, gc, out = probe(h, path, "newton", st, ctrl, entry, xloc)
    branch, c = check_newton(f"path {path} newton decision", path, got, gc, out, st, ctrl, entry, sc.DECISION_CASES[name][3])
    assert sc.ctrl_dict(gc)["spec_go"] == sc.DECISION_CASES[name][4]


def test_undecided_launch_publishes_only_when_told_to(h):
    st, xloc, entry, ctrl = sc.decision_case("second_continues")
    for always in (0, 1):
        e = dict(entry, publish_always=always)
        got, gc, out = probe(h, 0, "newton", st, ctrl, e, xloc)
        check_newton("path 0 newton decision", 0, got, gc, out, st, ctrl, e, "continue")
        assert sc.ctrl_dict(gc)["newton_done"] == 0
        assert published(out, e["seq"]) if always else unpublished(out)


@pytest.mark.parametrize("path", (0, 2))
def test_chained_iterations_see_the_state_the_one_before_left(h, path):
    """iteration 0 (refused: rate unknown) -> iteration 1 on the returned block: the rate comes from dy_norm_old, crate from
    ctrl; then a third launch behind the decision is a no-op"""
    st, xloc, entry, ctrl = sc.decision_case("first_refused_rate_unknown", n=1025)
    got, gc, out = probe(h, path, "newton", st, ctrl, entry, xloc)
    check_newton(f"path {path} newton decision", path, got, gc, out, st, ctrl, entry, "refused_crate_estimate_continue")
    st1 = got.copy(); st1[ROW["x"]] = 0.1 * st[ROW["x"]]
    ctrl1 = sc.ctrl_dict(gc)
    e1 = dict(entry, iter=1, seq=8)
    got1, gc1, out1 = probe(h, path, "newton", st1, ctrl1, e1, xloc)
    check_newton(f"path {path} newton decision", path, got1, gc1, out1, st1, ctrl1, e1, "converged_rate")
    assert sc.ctrl_dict(gc1)["crate"] == pytest.approx(0.3) and sc.ctrl_dict(gc1)["n_iter"] == 2
    e2 = dict(entry, iter=2, seq=9, publish_always=1)
    got2, gc2, out2 = probe(h, path, "newton", got1, sc.ctrl_dict(gc1), e2, xloc)
    check_newton(f"path {path} newton decision", path, got2, gc2, out2, got1, sc.ctrl_dict(gc1), e2, "behind")


# ----------------------------------------------------------------------------------------------------- members of a launch
@pytest.mark.parametrize("K", (1, 3, 17))
def test_ensemble_entry_lists(h, K):
    """K members in one launch: the entry list reversed, and a strict subset (members outside it come back bit for bit);
    orders, tolerances, factors and update norms differ per entry; one member of the corrector launch is already decided"""
    n = 1025
    lists = [list(range(K))[::-1]] + ([list(range(K))[1::2][::-1]] if K > 1 else [])
    for members in lists:
        for op in ("predict", "accept", "change_D", "init_D", "norms", "interp", "newton"):
            states, ctrls, entries, xloc = [], [], [], None
            for m in range(K):
                order = 1 + (m * 2 + 1) % 5
                atol, rtol = 10.0 ** -(10 + m % 3), 10.0 ** -(6 + m % 4)
                if op == "newton":
                    name = ("first_converged_by_tol", "behind_a_decision", "first_refused_rate_unknown", "first_converged_by_carried_rate",
                            "go_deep_negative")[m % 5]
                    inp, ent, ct, _, _ = sc.DECISION_CASES[name]
                    upd = 1.0 - 0.05 * (m % 3)
                    stm, xl = sc.newton_inputs(n, 9000 + m, order, upd=upd, **inp)
                    xloc = xl if xloc is None else xloc
                    entry = dict(order=order, atol=sc.ATOL, rtol=sc.RTOL, upd=upd, tol=(sc.TOL, 0.05)[m % 2], rate_max=1.0, crate0=1.0,
                                 tol_first=-1.0, dy_first_max=0.2, iter=0, maxit=sc.MAXIT, seq=0)
                    entry.update({q: v for q, v in ent.items() if q != "publish_always"})
                    ctrl = sc.clean_ctrl(**ct)
                else:
                    stm = sc.make_state(n, 500 * K + m)
                    ctrl = sc.dirty_ctrl(crate=0.1 * (m + 1))
                    entry = dict(order=order, atol=atol, rtol=rtol, h=sc.FACTORS[m % 4], aux=m % 2 if op in ("init_D", "norms") else 0, **sc.INTERP_T)
                states.append(stm); ctrls.append(ctrl); entries.append(entry)
            S = np.stack(states); C = np.stack([sc.ctrl_array(c) for c in ctrls])
            out = h.step_probe(2, op, S, C, [dict(entries[m], member=m) for m in members], xloc)
            for m in range(K):
                got, gc, st, e = out["state"][m], out["ctrl"][m], states[m], entries[m]
                what = (op, K, "member", m, "list", members)
                if m not in members:
                    assert same_bits(got, st) and same_bits(gc, C[m]), what + ("not in the list, but touched",)
                    continue
                g = "path 2 members"
                if op == "newton":
                    check_newton(g, 2, got, gc, out, st, ctrls[m], e)
                    continue
                D = st[:8]
                refs, crefs = {
                    "predict": lambda: (sc.ref_predict(D, e["order"], e["atol"], e["rtol"]), PREDICT_CLEARS),
                    "accept": lambda: (sc.ref_accept(D, st[ROW["d"]], e["order"]), {}),
                    "change_D": lambda: (sc.ref_change_D(D, e["order"], e["h"]), {}),
                    "init_D": lambda: (sc.ref_init_D(st[ROW["ytmp" if e["aux"] else "y"]], st[ROW["f0"]], e["h"]), {}),
                    "norms": lambda: ({}, sc.ref_norms(st[ROW["y"]], st[ROW["f0"]], st[ROW["f1"]] if e["aux"] else None, e["atol"], e["rtol"])),
                    "interp": lambda: (sc.ref_interp(D, e["order"], **sc.INTERP_T), {}),
                }[op]()
                check_state(g, got, st, refs, what)
                check_ctrl(g, gc, ctrls[m], crefs, what)


# --------------------------------------------------------------------------------------------- the update inside the solve
def star_net(stars=(10, 4), q=320, ring=16, per=29, n_total=4000):
    """A core of q hubs (each bound to its 2 * ring ring neighbours: above the analysis' hub degree, so all of them form the
    dense block), stars of a centre and k leaves with `per` hubs each, and disjoint pairs up to n_total species. The leaves go
    in the first elimination round; their centre then sees every hub of its leaves (29 k neighbours: eliminated in a later round
    only under the options of networks from 4 000 species on), and its stage-C row - and those of its leaves - gather over all
    of them: k = 10 gives rows of 290 entries (whole workgroups), k = 4 rows of 116 (one wavefront); the pairs are ELL rows."""
    reacs, prods = [], []

    def rev(i, j):
        reacs.extend([[(i, 1)], [(j, 1)]]); prods.extend([[(j, 1)], [(i, 1)]])
    for i in range(q):
        for o in range(1, ring + 1):
            rev(i, (i + o) % q)
    n, hub = q, 0
    for k in stars:
        z = n; n += 1
        for _ in range(k):
            leaf = n; n += 1
            rev(z, leaf)
            for _ in range(per):
                rev(leaf, hub % q); hub += 1
    while n + 2 <= n_total:
        reacs.extend([[(n, 1)], [(n + 1, 2)]]); prods.extend([[(n + 1, 1)], [(n, 1)]]); n += 2
    return from_lists(n, reacs, prods)


FUSED_NETS = {
    # name: (builder, dense block m, kinds the stage-C plan must have: groups / wave rows / block rows / 1024-thread build)
    "dense 1": (lambda: lc.dense_sweep_net(1)[0], 1, (True, False, False)),
    "dense 63": (lambda: lc.dense_sweep_net(63)[0], 63, (True, False, False)),
    "dense 64": (lambda: lc.dense_sweep_net(64)[0], 64, (True, False, False)),
    "dense 65": (lambda: lc.dense_sweep_net(65)[0], 65, (True, False, False)),
    "dense 129": (lambda: lc.dense_sweep_net(129)[0], 129, (True, False, False)),
    "synthetic 300": (lambda: synthetic_crn(300, 1500)[0], None, (True, True, False)),
    "star 4000": (star_net, 320, (True, True, True)),
}


@pytest.mark.parametrize("name", FUSED_NETS)
def test_corrector_update_inside_the_solve(name):
    """path 1: J(u) evaluated, I - c J factorised, b placed, SparseLU::solve_newton with the step state. The update and the
    sums against the reference applied to the x the launch produced; that x against the residual bound of the Newton tests
    and against kin_newton_probe's x for the same inputs. Orders 1, 3, 5; the dense-block tasks behind the plan's tasks
    across a wavefront boundary (m = 63, 64, 65, 129); ELL groups, one-wavefront rows, whole-workgroup rows (1024 threads)."""
    build, m, (has_g, has_s, has_b) = FUSED_NETS[name]
    net = build()
    hh, on, k = lc.static_handle(net, 5, lo=0.0, hi=2.0)
    try:
        n = net.n_species
        rng = np.random.default_rng(n)
        u = 10.0 ** rng.uniform(-3, 0, n)
        c = 1e-3
        M = lc.newton_matrix(on, k, u, c)
        for order, negative in ((1, None), (3, "shallow"), (5, None)):
            upd = 1.0 if order != 3 else 0.8
            st, _ = sc.newton_inputs(n, 40 + order, order, g=0.01, upd=upd, negative=negative)
            b = M @ st[ROW["x"]]
            st[ROW["u"]], st[ROW["b"]] = u, b
            st[ROW["x"]] = sc.SENTINEL
            entry = dict(order=order, atol=sc.ATOL, rtol=sc.RTOL, upd=upd, tol=sc.TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0,
                         dy_first_max=0.2, iter=0, maxit=sc.MAXIT, seq=11, c=c)
            ctrl = sc.clean_ctrl()
            out = hh.step_probe(1, "newton", st, sc.ctrl_array(ctrl), entry)
            info = out["info"]
            assert (info["groups"] > 0, info["wave_rows"] > 0, info["block_rows"] > 0) == (has_g, has_s, has_b), info
            assert info["wg"] == (1024 if has_b else 256) and info["wave_rows_long"] == 0 and (m is None or info["m"] == m), info
            tasks = info["groups"] + info["wave_rows"] + (info["m"] + 63) // 64
            assert info["grid"] == (info["block_rows"] + (tasks + 15) // 16 if has_b else (tasks + 3) // 4), info
            if has_b:
                assert info["max_row"] > 256, info
            x = out["state"][ROW["x"]]
            # the solve: this launch's x as a solution of M x = b, and next to kin_newton_probe's
            xn = hh.newton_probe(u, c, b)["x"][0]
            denom = float(np.max(abs(M) @ np.abs(x))) + float(np.max(np.abs(b)))
            assert float(np.max(np.abs(lc.residual_ld(M, x, b)))) / denom < lc.BWD_MAX
            assert float(np.max(np.abs(lc.residual_ld(M, x - xn, np.zeros(n))))) / denom < 2 * lc.BWD_MAX
            # the update: reference on the x the launch produced (in its row of the block the probe returned)
            st_ref = st.copy(); st_ref[ROW["x"]] = x
            sums, cref, branch, done, margins = sc.newton_reference(st_ref, entry, ctrl)
            assert not sc.margins_ok(margins) and sums["neg_margin"] > 1e-6, (sc.margins_ok(margins), sums["neg_margin"])
            check_newton("path 1 " + name.split()[0], 1, out["state"], out["ctrl"], out, st_ref, ctrl, entry, "converged_first_tol")
            assert sc.ctrl_dict(out["ctrl"])["any_negative"] == (1 if negative else 0)
    finally:
        hh.close()


def test_fused_path_refuses_a_network_without_a_dense_block():
    """pairs_net(20): two sparse rounds eliminate everything, m = 0 - no dense block, no fused solve"""
    hh = lc.static_handle(lc.pairs_net(20), 1)[0]
    st = sc.make_state(40, 1)
    with pytest.raises(capi.KineticaHipError) as e:
        hh.step_probe(1, "newton", st, sc.ctrl_array(sc.clean_ctrl()), dict(order=1, atol=1e-10, rtol=1e-8, upd=1.0, tol=0.03, c=1e-3))
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED
    hh.close()


def test_arguments_the_kernels_would_index_with_are_checked(h):
    st, xloc, entry, ctrl = sc.decision_case("first_converged_by_tol", n=65)
    bad = xloc.copy(); bad[3] = 65
    for kw, x in ((dict(order=6), xloc), (dict(), bad), (dict(iter=4), xloc)):
        with pytest.raises(capi.KineticaHipError) as e:
            h.step_probe(0, "newton", st, sc.ctrl_array(ctrl), dict(entry, **kw), x)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:
        h.step_probe(2, "accept", st[None], sc.ctrl_array(ctrl)[None], [dict(order=1, member=1)])
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:
        h.step_probe(2, "rk_error", st[None], sc.ctrl_array(ctrl)[None], [dict(order=1)])
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------- explicit pair
@pytest.mark.parametrize("n", sc.SIZES_RED)
def test_explicit_pair(h, n):
    """rk_combine with 1, 6 and 7 stages; rk_error's sum and flags, with a negative entry and a NaN in y_new; the error launch
    always publishes"""
    atol, rtol = 1e-10, 1e-8
    st = sc.make_state(n, 3 * n)
    K = st[ROW["K"]:ROW["K"] + 7]
    if n <= 4097:
        for stages in (1, 6, 7):
            w = 0.125 * np.where(sc.RK_B == 0, 0.01, sc.RK_B)
            got, gc, out = probe(h, 0, "rk_combine", st, sc.dirty_ctrl(), dict(aux=stages, w=w))
            check_state("rk_combine", got, st, sc.ref_rk_combine(st[ROW["y"]], K, w, stages), ("rk_combine", stages))
            check_ctrl("rk_combine", gc, sc.dirty_ctrl(), {}, "rk_combine")
            assert unpublished(out)
    for variant in ("positive", "negative", "nan"):
        st = sc.make_state(n, 5 * n)
        st[ROW["y_new"]] = np.abs(st[ROW["y_new"]])
        if variant == "negative":
            st[ROW["y_new"], n - 1] = -1e-30
        if variant == "nan":
            st[ROW["y_new"], n // 2] = np.nan
        ctrl = sc.dirty_ctrl(nonfinite=0, any_negative=0)
        e = 0.125 * sc.RK_E
        got, gc, out = probe(h, 0, "rk_error", st, ctrl, dict(atol=atol, rtol=rtol, w=e, seq=5))
        ref = sc.ref_rk_error(st[ROW["y"]], st[ROW["y_new"]], st[ROW["K"]:ROW["K"] + 7], e, atol, rtol)
        check_state("rk_error", got, st, {}, variant)
        check_ctrl("rk_error", gc, ctrl, ref, (variant, n))
        assert (sc.ctrl_dict(gc)["any_negative"], sc.ctrl_dict(gc)["nonfinite"]) == (variant == "negative", variant == "nan")
        assert published(out, 5)


# ------------------------------------------------------------------------------------------------ the handle afterwards
def test_a_solve_after_the_probe_is_the_solve_of_a_fresh_handle(monkeypatch):
    """probes of all three paths on a handle, then a host-driven solve on it: bit for bit the solve of a fresh handle"""
    monkeypatch.setenv("KIN_RESIDENT", "0")
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
            first = hh.solve(pars, u0)         # (a solve before, so the probe meets a handle with a history)
            st, xloc, entry, ctrl = sc.decision_case("first_converged_by_tol", n=300)
            st[ROW["u"]] = 10.0 ** np.random.default_rng(0).uniform(-6, 0, 300)
            st[ROW["b"]] = st[ROW["x"]]
            hh.step_probe(0, "newton", st, sc.ctrl_array(ctrl), entry, xloc)
            hh.step_probe(1, "newton", st, sc.ctrl_array(ctrl), dict(entry, c=1e-4))
            hh.step_probe(2, "predict", st[None], sc.ctrl_array(ctrl)[None], [dict(entry, member=0)])
        res.append(hh.solve(pars, u0))
        hh.close()
    (t0, us0, rc0, st0, _), (t1, us1, rc1, st1, _) = res
    assert rc0 == 0 and rc1 == 0 and np.array_equal(t0, t1) and np.array_equal(us0, us1)
    assert {q: v for q, v in st0.items() if q != "wall_seconds"} == {q: v for q, v in st1.items() if q != "wall_seconds"}
    assert np.array_equal(first[1], us0)
