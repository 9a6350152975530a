"""Shared by tests/test_gpu_resident_step.py (kin_step_probe, paths 3 and 4: the resident kernel through its own dispatch) and
tests/test_resident_step_host.py (the CPU replay's backend, tests/native/resident_host.cpp): the constructed networks, the case
tables and the checks, written over a `run(op, state, ctrl, entry) -> (state, ctrl)` callable so that both files run the same
cases. References and bounds are those of tests/step_cases.py (extended there where the resident kernel needs it); the only other
numbers are BWD_MAX of tests/linalg_cases.py and exact comparisons. A plain module: no fixtures, no test collection.

Networks. pair_net(n): disjoint reversible pairs A_i <-> B_i (species 2 i and 2 i + 1) with ONE rate constant PAIR_K = 2^10, plus
an inert species where n is odd. With c = PAIR_C = 2^-10 every product k u and c f is exact, a pair's two species are kept within
a factor of two of each other (their difference is exact), and the Newton matrix I - c_fact J is block diagonal with 2 x 2 blocks
[[1 + a, -a], [-a, 1 + a]], a = c_fact k: inverse (1 + 2 a)^-1 [[1 + a, a], [a, 1 + a]] of infinity norm 1, eigenvalue 1 along
(1, 1) and 1 + 2 a along (1, -1). An update along (1, -1) therefore contracts by rho = 1 - upd (1 + 2 c k) / (1 + 2 a) per
iteration: the first update's norm and the later iterations' rate are the case's to choose.

One iteration (NEWTON). The iteration forms its own residual b = c f(y) - psi - d, so for a target update x_t the case sets
psi = c f(y) - d - (I - c_fact J(u)) x_t in np.longdouble (term lists of tests/jac_cases.py) and rounds it. The x the probe
returns is judged as a solution of M x = b_ref, b_ref the residual in extended precision from the ROUNDED psi:
  * pair networks: max |M x - b_ref| / (max |M||x| + max |b_ref|) < BWD_MAX (linalg_cases.solve_errors' backward error) - the
    construction keeps the residual's own rounding (at most 3 roundings of |c f| + |psi| + |d|) far below that;
  * every network, entry by entry: |M x - b_ref|_i <= BWD_MAX (max |M||x| + max |b_ref|) + (L_i + 6) u (|c| S_i + |psi_i| + |d_i|), the
    second term being jac_cases.bound_resid - the bound of the residual's rounding, which on a nonlinear network with c f of
    1e9 update sizes is what dominates (the same cancellation every Newton iteration of a stiff solve lives with).
y, d and the five sums are then compared with step_cases.ref_newton_sums evaluated on the RETURNED x: derived bounds only.

A whole attempt (CORRECTOR), order 1: y_0 = fl(D[0] + D[1]) is ONE addition, which the reference repeats in double - the
predictor's y is known bit for bit -, psi = D[1] gamma_1 / alpha_1 is a product by 1 and a division (ref_predict's 3 u), the scale
within 3 u. From there the reference chains
ref_newton_sums -> ref_decide per iteration with every x recomputed in longdouble from the chain's own y and d, and carries
absolute error bounds along (attempt_chain): the residual's inputs (c k (e_yA + e_yB) + e_d + e_psi), its three roundings, the solve
(|x_dev - x| <= ||M^-1||_inf (e_b + BWD_MAX denom), ||M^-1||_inf = 1), the update. Every threshold an attempt passes is asserted
to be at least 1e-3 (relative) away from the tested quantity - three orders above any of these bounds - so device and reference
cannot legitimately take different branches.
  `exhausted` cannot be reached by an attempt of RES_NEWTON_MAXITER iterations except at an exact equality: on the last iteration
the divergence estimate rate^1 / (1 - rate) dy and the convergence estimate are the same number, above tol it diverged, below it
converged. tests/test_resident_step_host.py reaches the equality with scripted sums; no device case exists for it.
  A non-finite STATE with a converged update needs a species no reaction couples (an infinite y_A makes f_B infinite): the inert
species, i.e. odd n only. The same species carries the attempt cases with a NaN state (its error weight is NaN, so the update norm
is: the attempt ends as non-finite) and with psi = Inf: the predictor forms y and psi from the same rows of D, so an infinite psi
comes with an infinite predicted state, and the update norm is Inf / Inf. An Inf update on a FINITE state, and NaN / Inf in psi
and y one at a time, are cases of the single iteration (NEWTON_PLANTS), where psi and y are rows of their own; there the raw sums
are compared as non-finite values."""
import numpy as np

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists
from tests import jac_cases as jc
from tests import linalg_cases as lc
from tests import step_cases as sc
from tests.step_cases import LD, ROW, U

SIZES = (2, 64, 65, 511, 512, 513, 1024, 1025)
PAIR_K, PAIR_C = 1024.0, 2.0 ** -10
NEG_MARK = 4294967296.0          # bdf_rules.hpp: BDF_NEG_MARK
MEASURED = {}


def pair_net(n):
    p = n // 2
    return from_lists(n, [[(2 * i, 1)] for i in range(p)] + [[(2 * i + 1, 1)] for i in range(p)],
                      [[(2 * i + 1, 1)] for i in range(p)] + [[(2 * i, 1)] for i in range(p)])


def synthetic_rates(net, seed=5, lo=0.0, hi=2.0):
    """the rate constants linalg_cases.static_handle(net, seed, lo, hi) sets, without a handle"""
    return 10.0 ** np.random.default_rng(seed).uniform(lo, hi, net.n_reactions)


def pair_rates(n):
    return np.full(2 * (n // 2), PAIR_K)


def expected_shape(n):
    """what kin_step_probe's info must say of a network of n species: trips of the 512-stride loops, wavefronts owning a species"""
    return dict(N=n, trips=(n + 511) // 512, waves_owning=(min(n, 512) + 63) // 64)


# ------------------------------------------------------------------------------------------------------------ comparisons
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


def check_state(group, got, given, refs, what, skip=()):
    """rows in refs within their bound, every other row of the block as given, bit for bit (skip: rows judged elsewhere)"""
    for r in range(capi.STEP_ROWS):
        if r in skip:
            continue
        if r in refs:
            assert close(group, got[r], *refs[r]), (what, "row", r)
        else:
            assert same_bits(got[r], given[r]), (what, "row", r, "was touched")


def check_ctrl(group, got, given, refs, what):
    """fields in refs equal (bound None) or within their bound, every other field as given, bit for bit"""
    got, given = sc.ctrl_dict(got), sc.ctrl_dict(sc.ctrl_array(given))
    for f in sc.FIELDS:
        if f in refs and refs[f][1] is not None:
            assert close(group, got[f], *refs[f]), (what, f, got[f], float(refs[f][0]))
        else:
            want = float(refs[f][0]) if f in refs else given[f]
            assert got[f] == want or (np.isnan(got[f]) and np.isnan(want)), (what, f, got[f], want)


# ------------------------------------------------------------------------------------------------------ elementwise phases
ATOL_E, RTOL_E = 1e-10, 1e-8


def check_elementwise(run, n, g=""):
    """init_D (from y, from ytmp), predict, accept, change_D at every factor, interp into both solution rows - every order. The
    control block comes back untouched except for the time of the interpolated row."""
    dirty = sc.dirty_ctrl()
    for from_ytmp in (0, 1):
        st = sc.make_state(n, 11 * n + from_ytmp)
        got, gc = run("init_D", st, sc.ctrl_array(dirty), dict(aux=from_ytmp, h=0.375e-3))
        check_state(g + "init_D", got, st, sc.ref_init_D(st[ROW["ytmp" if from_ytmp else "y"]], st[ROW["f0"]], 0.375e-3), ("init_D", from_ytmp))
        check_ctrl(g + "init_D", gc, dirty, {}, "init_D")
    for order in sc.ORDERS:
        seed = 100 * n + order
        st = sc.make_state(n, seed, d_rows=order + 1)
        got, gc = run("predict", st, sc.ctrl_array(dirty), dict(order=order, atol=ATOL_E, rtol=RTOL_E))
        check_state(g + "predict", got, st, sc.ref_predict(st[:8], order, ATOL_E, RTOL_E), ("predict", order))
        check_ctrl(g + "predict", gc, dirty, {}, ("predict", order))
        st = sc.make_state(n, seed + 1, d_rows=order + 3)
        got, gc = run("accept", st, sc.ctrl_array(dirty), dict(order=order))
        check_state(g + "accept", got, st, sc.ref_accept(st[:8], st[ROW["d"]], order), ("accept", order))
        check_ctrl(g + "accept", gc, dirty, {}, "accept")
        for factor in sc.FACTORS:
            st = sc.make_state(n, seed + 2, d_rows=order + 1)
            got, gc = run("change_D", st, sc.ctrl_array(dirty), dict(order=order, h=factor))
            check_state(g + "change_D", got, st, sc.ref_change_D(st[:8], order, factor), ("change_D", order, factor))
            check_ctrl(g + "change_D", gc, dirty, {}, "change_D")
        for row in (0, 1):
            st = sc.make_state(n, seed + 3 + row, d_rows=order + 1)
            got, gc = run("interp", st, sc.ctrl_array(dirty), dict(order=order, row=row, **sc.INTERP_T))
            ref = sc.ref_interp(st[:8], order, **sc.INTERP_T)[ROW["out"]]
            check_state(g + "interp", got, st, {ROW["out"] + row: ref}, ("interp", order, row))
            check_ctrl(g + "interp", gc, dirty, {f"scratch{row}": (sc.INTERP_T["ts"], None)}, ("interp", order, row))


def check_vec(run, n, g=""):
    """the six VecOps, save_y into both solution rows, set_time; the clipped copy meets a NaN, a -0.0 and negative entries"""
    dirty = sc.dirty_ctrl()
    st = sc.make_state(n, 31 * n)
    cs = st[ROW["cs"]]
    cs[0] = -0.0
    cs[n - 1] = np.nan
    if n > 2:
        cs[n // 2] = -1.5
    y, D0, f0, u0 = (st[ROW[q]].astype(LD) for q in ("y", "D", "f0", "u"))
    z = np.zeros(n, LD)
    cases = dict(load_u0={ROW["y"]: (u0, z)}, cs_from_y={ROW["cs"]: (y, z)}, y_from_cs_clipped={ROW["y"]: (sc.ref_clipped(cs), z)},
                 y_from_d0={ROW["y"]: (D0, z)}, ytmp_from_d0={ROW["ytmp"]: (D0, z)}, ytmp_axpy={ROW["ytmp"]: sc.ref_axpy(st[ROW["y"]], st[ROW["f0"]], 0.375)})
    for name, refs in cases.items():
        got, gc = run("vec", st, sc.ctrl_array(dirty), dict(aux=capi.STEP_VEC_OPS[name], h=0.375))
        check_state(g + "vec", got, st, refs, name)
        check_ctrl(g + "vec", gc, dirty, {}, name)
        if name == "y_from_cs_clipped":      # a copy: bit for bit, the sign of -0.0 and the NaN's payload included
            assert same_bits(got[ROW["y"]], sc.ref_clipped(cs)), name
    # a second state for the clip: negative entries first and last (at n = 2 the plants above leave none), the rest mixed
    st2 = sc.make_state(n, 37 * n)
    st2[ROW["cs"], 0], st2[ROW["cs"], n - 1] = -1.5, -2.0 ** -1060
    assert np.any(st2[ROW["cs"]] < 0)
    got, gc = run("vec", st2, sc.ctrl_array(dirty), dict(aux=capi.STEP_VEC_OPS["y_from_cs_clipped"]))
    check_state(g + "vec", got, st2, {ROW["y"]: (sc.ref_clipped(st2[ROW["cs"]]), z)}, "clip, negative entries")
    assert same_bits(got[ROW["y"]], sc.ref_clipped(st2[ROW["cs"]])) and got[ROW["y"], 0] == 0.0 and got[ROW["y"], n - 1] == 0.0
    for row in (0, 1):
        got, gc = run("vec", st, sc.ctrl_array(dirty), dict(aux=capi.STEP_VEC_OPS["save_y"], row=row, t=0.8125))
        check_state(g + "vec", got, st, {ROW["out"] + row: (y, z)}, ("save_y", row))
        check_ctrl(g + "vec", gc, dirty, {f"scratch{row}": (0.8125, None)}, ("save_y", row))
        got, gc = run("vec", st, sc.ctrl_array(dirty), dict(aux=capi.STEP_VEC_OPS["set_time"], row=row, t=0.4375))
        check_state(g + "vec", got, st, {}, ("set_time", row))
        check_ctrl(g + "vec", gc, dirty, {f"scratch{row}": (0.4375, None)}, ("set_time", row))


NORM_VARIANTS = ("no_f1", "f1", "nan_f0", "inf_f0", "nan_f1", "inf_f1", "nan_y", "inf_y")


def norms_state(n, variant):
    st = sc.make_state(n, 7 * n + len(variant) + NORM_VARIANTS.index(variant))
    bad = dict(nan=np.nan, inf=np.inf).get(variant[:3])
    if bad is not None:
        st[ROW[variant[4:]], (n // 2 if variant.endswith("f0") else n - 1)] = bad
    return st, variant not in ("no_f1", "nan_f0", "inf_f0")


def check_norms(run, n, g=""):
    """with and without f1; NaN and Inf in f0, f1 (flag set, a NaN leaves the maximum) and in y (no flag: the sums show it)"""
    dirty = sc.dirty_ctrl()
    for variant in NORM_VARIANTS:
        st, with_f1 = norms_state(n, variant)
        got, gc = run("norms", st, sc.ctrl_array(dirty), dict(aux=int(with_f1), atol=ATOL_E, rtol=RTOL_E))
        ref = sc.ref_norms(st[ROW["y"]], st[ROW["f0"]], st[ROW["f1"]] if with_f1 else None, ATOL_E, RTOL_E)
        check_state(g + "norms", got, st, {}, variant)
        check_ctrl(g + "norms", gc, dirty, ref, (variant, n))
        assert sc.ctrl_dict(gc)["nonfinite"] == (variant[4:] in ("f0", "f1") and variant[:3] in ("nan", "inf")), variant


# ------------------------------------------------------------------------------------------------------- one iteration
def tie_pairs(n, g, special=()):
    """y_hook of newton_inputs: B_i = A_i + delta_i (or A_i = B_i - delta_i where B_i is one of the `special` indices the case
    planted a value at), delta_i = 8 g scale_i: c f is then about 8 update sizes and B_i - A_i is exact"""
    def hook(y):
        y = y.copy()
        for i in range(n // 2):
            a, b = 2 * i, 2 * i + 1
            anchor = b if b in special and a not in special else a
            other = a + b - anchor
            delta = 8.0 * g * (sc.ATOL + sc.RTOL * abs(y[anchor])) if np.isfinite(y[anchor]) else 0.0
            y[other] = y[anchor] + (delta if anchor == a else -delta)
        return y
    return hook


class Net:
    """a network with its rate constants and the extended-precision term lists"""

    def __init__(self, net, k):
        self.net, self.k, self.n = net, np.asarray(k, np.float64), net.n_species
        self.ref = jc.Reference(net)

    def jac_apply(self, u, x, absolute=False):
        """J(u) x (or |J(u)| |x|) in longdouble"""
        vals = self.ref.jac(self.k, u)[0]
        if absolute:
            vals, x = np.abs(vals), np.abs(x)
        out = np.zeros(self.n, LD)
        np.add.at(out, self.ref.rows, vals * np.asarray(x, LD)[self.ref.cols])
        return out


# non-finite inputs of one iteration (mirroring DECISION_CASES' nonfinite_update_inf / _nan and nonfinite_state_converged):
# psi = Inf / NaN at species n // 3 makes the residual, hence x, hence the update non-finite there with a finite state;
# y = Inf / NaN on the inert species (odd n) is a non-finite state under a finite update
NEWTON_PLANTS = ("inf_psi", "nan_psi", "inf_y", "nan_y")


def newton_plants(n):
    return NEWTON_PLANTS if n % 2 else NEWTON_PLANTS[:2]


def newton_case(N, seed, order, upd, negative, c, c_fact, pairs, plant=None):
    """(state, entry) of one iteration whose update is about 0.01 error weights (step_cases.newton_inputs; SUM_CASES); plant: one
    of NEWTON_PLANTS"""
    n, g = N.n, 0.01
    hook = tie_pairs(n, g, special=(n - 1, n // 2)) if pairs else None
    if plant in ("inf_y", "nan_y"):
        assert pairs and n % 2
        tie = hook

        def hook(y):
            y = tie(y)
            y[n - 1] = np.inf if plant == "inf_y" else np.nan
            return y
    st, _ = sc.newton_inputs(n, seed, order, g=g, upd=upd, negative=negative, y_hook=hook)
    rng = np.random.default_rng(seed + 1)
    st[ROW["u"]] = st[ROW["y"]] if pairs else 10.0 ** rng.uniform(-3, 0, n)
    x_t = st[ROW["x"]].astype(LD)
    f = N.ref.rhs(N.k, st[ROW["y"]])[0]
    Mx = x_t - LD(c_fact) * N.jac_apply(st[ROW["u"]], x_t)
    st[ROW["psi"]] = np.asarray(LD(c) * f - st[ROW["d"]].astype(LD) - Mx, np.float64)
    if plant in ("inf_psi", "nan_psi"):
        st[ROW["psi"], n // 3] = np.inf if plant == "inf_psi" else np.nan
    st[ROW["x"]] = sc.SENTINEL
    entry = dict(order=order, atol=sc.ATOL, rtol=sc.RTOL, upd=upd, c=c, c_fact=c_fact, ec=sc.ERRC[order],
                 ec_m=sc.ERRC[order - 1] if order > 1 else 0.0, ec_p=sc.ERRC[order + 1] if order < 5 else 0.0)
    return st, entry


def check_newton(run, N, st, entry, negative, pairs, g="", plant=None):
    """plant (NEWTON_PLANTS): psi planted - x is non-finite where the residual is, the solve is not judged, the update norm's sum
    s must be the reference's non-finite value (Inf stays Inf, a NaN makes it NaN: dy / scale, its square and the sum do the
    same in any order), se, sm, sp must be non-finite where the reference's are (step_cases.ref_newton_sums: only that is
    specified once the update is non-finite); y planted - everything is judged as usual, se is exactly +inf for y = Inf."""
    dirty = sc.dirty_ctrl()
    got, gc = run("newton", st, sc.ctrl_array(dirty), entry)
    n, order, c, c_fact = N.n, entry["order"], entry["c"], entry["c_fact"]
    x = got[ROW["x"]]
    psi_planted = plant in ("inf_psi", "nan_psi")
    if psi_planted:
        j = n // 3
        assert not np.isfinite(x[j]), "x"
        if pairs:                                  # (a pair couples nothing else: every other pair's x stays finite)
            assert np.all(np.isfinite(np.delete(x, [j, j ^ 1] if j ^ 1 < 2 * (n // 2) else [j]))), "x"
    else:
        assert np.all(np.isfinite(x)), "x"
        # the solve
        b, scale_b, L = N.ref.resid(N.k, st[ROW["y"]], c, st[ROW["psi"]], st[ROW["d"]])
        xl = x.astype(LD)
        u = st[ROW["u"]]
        r = xl - LD(c_fact) * N.jac_apply(u, xl) - b
        denom = np.max(np.abs(xl) + abs(LD(c_fact)) * N.jac_apply(u, xl, absolute=True)) + np.max(np.abs(b))
        if pairs:
            e_bwd = float(np.max(np.abs(r)) / denom)
            MEASURED[g + "newton backward error / BWD_MAX"] = max(MEASURED.get(g + "newton backward error / BWD_MAX", 0.0), e_bwd / lc.BWD_MAX)
            assert e_bwd < lc.BWD_MAX, e_bwd
        assert close(g + "newton solve, entrywise", r, np.zeros(n, LD), LD(lc.BWD_MAX) * denom + jc.bound_resid(scale_b, L)), "M x = b"
    # the update and the sums, on the x the iteration used
    sums = sc.ref_newton_sums(x, st[ROW["scale"]], st[ROW["y"]], st[ROW["d"]], st[:8], order, entry["upd"], sc.ATOL, sc.RTOL)
    assert sums["neg_margin"] > 1e-6, sums["neg_margin"]
    check_state(g + "newton update", got, st, {ROW["y"]: sums["y"], ROW["d"]: sums["d"]}, ("newton", order, plant), skip=(ROW["x"],))
    refs = dict(dy_norm=sc.sum_with_bound(*sums["s"], n), err_norm=sc.sum_with_bound(*sums["se"], n), err_m_norm=sc.sum_with_bound(*sums["sm"], n),
                err_p_norm=sc.sum_with_bound(*sums["sp"], n), any_negative=(3 if sums["deep"] else 1 if sums["neg"] else 0, None), lu_bad=(0, None))
    gd = sc.ctrl_dict(gc)
    if plant is not None:
        with np.errstate(invalid="ignore"):
            S = {q: float(refs[q][0]) for q in ("dy_norm", "err_norm", "err_m_norm", "err_p_norm")}
        if psi_planted:
            assert not np.isfinite(S["dy_norm"]) and not np.isfinite(S["err_norm"]), S
            assert gd["dy_norm"] == S["dy_norm"] or (np.isnan(gd["dy_norm"]) and np.isnan(S["dy_norm"])), (plant, gd["dy_norm"], S["dy_norm"])
        else:
            assert np.isfinite(S["dy_norm"]) and not np.isfinite(S["err_norm"]), S
            if plant == "inf_y":
                assert gd["err_norm"] == np.inf, gd["err_norm"]
        for q in ("err_norm", "err_m_norm", "err_p_norm"):      # non-finite where the reference's is; else within the bound, below
            if not np.isfinite(S[q]):
                assert not np.isfinite(gd[q]), (plant, q, gd[q])
                refs[q] = (gd[q], None)
        if psi_planted:
            refs["dy_norm"] = (gd["dy_norm"], None)
    check_ctrl(g + "newton sums", gc, dirty, refs, ("newton", order, plant))
    assert gd["any_negative"] == (3 if sums["deep"] else 1 if sums["neg"] else 0)
    if plant is None:
        assert gd["any_negative"] == (1 if negative == "shallow" else 3 if negative == "deep" else 0)
    if order == 1:
        assert gd["err_m_norm"] == 0.0
    if order == 5:
        assert gd["err_p_norm"] == 0.0


def check_newton_plants(run, N, seed, pairs, g=""):
    """every plant of NEWTON_PLANTS the network has a species for, at orders 1, 3 and 5"""
    for plant in (newton_plants(N.n) if pairs else NEWTON_PLANTS[:2]):
        for order in (1, 3, 5):
            c = PAIR_C if pairs else 1e-3
            st, entry = newton_case(N, seed + order, order, 1.0, None, c, 0.75 * c, pairs, plant=plant)
            check_newton(run, N, st, entry, None, pairs, g, plant=plant)


# --------------------------------------------------------------------------------------------------------- whole attempts
def a_for_rate(rho, upd=1.0):
    """a = c_fact k with 1 - upd (1 + 2 c k) / (1 + 2 a) = rho at c k = 1"""
    return (3.0 * upd / (1.0 - rho) - 1.0) / 2.0


# name -> (g: first update's norm in error weights, rho: contraction of the later ones, entry arguments, plant, branches reached
# iteration by iteration, converged)
ATTEMPT_CASES = {
    "converged_first_tol": (0.01, 0.0, dict(), None, ["converged_first_tol"], 1),
    "converged_carried_rate": (0.1, 0.0, dict(crate0=0.1, tol_first=sc.TOL), None, ["converged_carried_rate"], 1),
    "refused_crate_then_rate": (0.1, 0.1, dict(crate0=1.0, tol_first=sc.TOL), None, ["refused_crate_estimate_continue", "converged_rate"], 1),
    "refused_test_off_then_rate": (0.1, 0.1, dict(crate0=0.1, tol_first=-1.0), None, ["refused_estimate_continue", "converged_rate"], 1),
    "refused_dymax_then_rate": (0.25, 0.1, dict(crate0=0.05, tol_first=sc.TOL), None, ["refused_dymax_continue", "converged_rate"], 1),
    "refused_estimate_then_rate": (0.1, 0.1, dict(crate0=0.5, tol_first=sc.TOL), None, ["refused_estimate_continue", "converged_rate"], 1),
    "four_iterations": (1.0, 0.32, dict(), None, ["refused_crate_dymax_estimate_continue", "continue", "continue", "converged_rate"], 1),
    "diverged_rate_max": (0.1, 0.2, dict(rate_max=0.15), None, ["refused_crate_estimate_continue", "diverged_rate_max"], 0),
    "diverged_estimate": (0.1, 0.9, dict(), None, ["refused_crate_estimate_continue", "diverged_estimate"], 0),
    "zero_update": (0.0, 0.0, dict(), None, ["zero_update"], 1),
    "nonfinite_update": (0.01, 0.0, dict(), "nan_psi", ["nonfinite"], 0),
    "nonfinite_update_inf": (0.01, 0.0, dict(), "inf_psi_inert", ["nonfinite"], 0),
    "nonfinite_state_converged": (0.01, 0.0, dict(), "inf_inert", ["converged_first_tol"], 1),
    "nonfinite_state_nan": (0.01, 0.0, dict(), "nan_inert", ["nonfinite"], 0),
    "shallow_negative": (0.01, 0.0, dict(), "shallow", ["converged_first_tol"], 1),
    "deep_negative": (0.01, 0.0, dict(), "deep", ["converged_first_tol"], 1),
}


def attempt_sizes(name):
    return tuple(n for n in SIZES if n % 2) if str(ATTEMPT_CASES[name][3]).endswith("_inert") else SIZES


def attempt_case(n, name, seed=0):
    """(state, entry) of a whole attempt of order 1 on pair_net(n): D[0] + D[1] = the state, D[1] = alpha_1 psi"""
    g, rho, ent, plant, _, _ = ATTEMPT_CASES[name]
    rng = np.random.default_rng(77000 + 13 * n + seed)
    p = n // 2
    st = sc.make_state(n, 7000 + n + seed, d_rows=3)
    y = 10.0 ** rng.uniform(-12, 0, n)
    special = ()
    if plant == "shallow":
        y[n - 1 - (n % 2)] = -3.0 * sc.ATOL; special = (n - 1 - (n % 2),)
    if plant == "deep":
        y[2 * (p // 2)] = -1e4 * sc.ATOL; special = (2 * (p // 2),)
    y = tie_pairs(n, g, special)(y)
    scale = sc.ATOL + sc.RTOL * np.abs(y)
    upd = 1.0
    a = a_for_rate(rho, upd)
    c, c_fact = PAIR_C, a / PAIR_K
    z = rng.choice([-1.0, 1.0], p) * rng.uniform(0.5, 1.5, p)
    z *= np.sqrt(n / (2.0 * np.sum(z * z))) if p else 1.0
    x_t = np.zeros(n, LD)
    v = LD(g) * z.astype(LD) * scale[0:2 * p:2].astype(LD) / LD(upd)
    x_t[0:2 * p:2], x_t[1:2 * p:2] = v, -v
    yl = y.astype(LD)
    f = np.zeros(n, LD)
    f[0:2 * p:2] = LD(PAIR_K) * (yl[1:2 * p:2] - yl[0:2 * p:2]); f[1:2 * p:2] = -f[0:2 * p:2]
    Mx = x_t.copy()
    Mx[0:2 * p:2] = (1 + LD(a)) * x_t[0:2 * p:2] - LD(a) * x_t[1:2 * p:2]
    Mx[1:2 * p:2] = (1 + LD(a)) * x_t[1:2 * p:2] - LD(a) * x_t[0:2 * p:2]
    psi = np.asarray(LD(c) * f - Mx, np.float64)
    if plant == "nan_psi":
        psi[2 * (p // 3)] = np.nan
    st[1] = psi * sc.ALPHA[1]
    st[0] = y - st[1]
    if plant == "inf_inert":
        assert n % 2
        st[0, n - 1], st[1, n - 1] = np.inf, 0.0
    if plant == "nan_inert":             # a NaN state: its error weight is NaN, so the update norm is, and the attempt ends as non-finite
        assert n % 2
        st[0, n - 1], st[1, n - 1] = np.nan, 0.0
    if plant == "inf_psi_inert":         # psi = D[1] / alpha_1 = Inf (the predicted state holds D[1] too: it is Inf as well)
        assert n % 2
        st[0, n - 1], st[1, n - 1] = 1.0, np.inf
    st[2] = scale * sc.signed_decades(rng, n, -2, 0)
    st[ROW["u"]] = np.abs(st[ROW["u"]])
    entry = dict(order=1, atol=sc.ATOL, rtol=sc.RTOL, upd=upd, c=c, c_fact=c_fact, tol=sc.TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0,
                 dy_first_max=0.2, ec=sc.ERRC[1], ec_m=0.0, ec_p=sc.ERRC[2])
    entry.update(ent)
    return st, entry


def pair_solve(n, a, b):
    """x = (I - c_fact J)^-1 b on pair_net(n) in longdouble: (1 + 2 a)^-1 [[1 + a, a], [a, 1 + a]] per pair, the inert species x = b"""
    p = n // 2
    x = np.array(b, LD)
    bA, bB = b[0:2 * p:2], b[1:2 * p:2]
    with np.errstate(invalid="ignore", over="ignore"):
        x[0:2 * p:2] = ((1 + LD(a)) * bA + LD(a) * bB) / (1 + 2 * LD(a))
        x[1:2 * p:2] = ((1 + LD(a)) * bB + LD(a) * bA) / (1 + 2 * LD(a))
    return x


def decide_chain(sums_of, n, entry, maxit=sc.MAXIT):
    """ref_decide iteration by iteration as res_corrector_loop takes its decisions: sums_of(it) -> the sums of iteration `it`
    (step_cases.ref_newton_sums' dict). The control block of one iteration is the next one's input; the rate's bound gets the
    relative error of the norm before it (ref_decide takes dy_norm_old as exact). Returns (final control block {field: (value,
    bound)}, branches, margins of every iteration)."""
    ctrl = sc.clean_ctrl(crate=entry["crate0"])
    branches, margins = [], []
    old = (LD(0), LD(0))
    for it in range(maxit):
        sums = sums_of(it)
        c, branch, done, mg = sc.ref_decide(sums, n, ctrl, iter=it, maxit=maxit, tol=entry["tol"], rate_max=entry["rate_max"], crate0=entry["crate0"],
                                            tol_first=entry["tol_first"], dy_first_max=entry["dy_first_max"])
        if it > 0 and c["crate"][1] is not None and old[0] > 0:
            c["crate"] = (c["crate"][0], c["crate"][1] + c["crate"][0] * old[1] / old[0])
        branches.append(branch); margins += mg
        old = c["dy_norm"]
        if c["newton_done"][0]:
            return c, branches, margins
        ctrl = {f: float(v[0]) for f, v in c.items()}
    raise AssertionError("an attempt ends with its last iteration")


def attempt_chain(n, st, entry):
    """the reference of a whole attempt on pair_net(n) (module docstring): (control block, branches, margins, y, d, psi, scale as
    (value, bound) pairs of the last iteration)"""
    p = n // 2
    c, a, upd = entry["c"], entry["c_fact"] * PAIR_K, entry["upd"]
    D = st[:8]
    y = (st[0] + st[1]).astype(LD)                     # one addition, repeated in double
    psi = st[1].astype(LD) * LD(sc.GAMMA[1]) / LD(sc.ALPHA[1])
    psi_e = 3 * U * np.abs(psi)                        # (ref_predict: 2 order + 1)
    scale = LD(sc.ATOL) + LD(sc.RTOL) * np.abs(y)
    scale_e = 3 * U * scale
    state = dict(y=y, ye=np.zeros(n, LD), d=np.zeros(n, LD), de=np.zeros(n, LD))

    def sums_of(it):
        y, ye, d, de = state["y"], state["ye"], state["d"], state["de"]
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.zeros(n, LD); fe = np.zeros(n, LD)
            f[0:2 * p:2] = LD(PAIR_K) * (y[1:2 * p:2] - y[0:2 * p:2]); f[1:2 * p:2] = -f[0:2 * p:2]
            fe[0:2 * p:2] = LD(PAIR_K) * (ye[1:2 * p:2] + ye[0:2 * p:2]); fe[1:2 * p:2] = fe[0:2 * p:2]
            b = LD(c) * f - psi - d
            # k u and c f exact (powers of two); the row's sum of two terms and the two subtractions: three roundings
            be = LD(c) * fe + de + psi_e + 4 * U * (np.abs(LD(c) * f) + np.abs(psi) + np.abs(d))
            x = pair_solve(n, a, b)
            absMx = np.abs(x) * (1 + LD(a)); absMx[0:2 * p:2] += LD(a) * np.abs(x[1:2 * p:2]); absMx[1:2 * p:2] += LD(a) * np.abs(x[0:2 * p:2])
            if n % 2:
                absMx[n - 1] = np.abs(x[n - 1])
            fin = np.isfinite(x) & np.isfinite(b)
            denom = (np.max(absMx[fin]) + np.max(np.abs(b[fin]))) if np.any(fin) else LD(0)
            xe = be.copy()
            xe[0:2 * p:2] = np.maximum(be[0:2 * p:2], be[1:2 * p:2]); xe[1:2 * p:2] = xe[0:2 * p:2]
            xe = xe + LD(lc.BWD_MAX) * denom
            xe = np.where(np.isfinite(xe), xe, 0)
        sums = sc.ref_newton_sums(x, scale, y, d, D, 1, upd, sc.ATOL, sc.RTOL, x_err=xe, scale_err=scale_e, y_err=ye, d_err=de)
        state.update(y=sums["y"][0], ye=sums["y"][1], d=sums["d"][0], de=sums["d"][1], sums=sums)
        return sums

    ctrl, branches, margins = decide_chain(sums_of, n, entry)
    return ctrl, branches, margins, (state["y"], state["ye"]), (state["d"], state["de"]), (psi, psi_e), (scale, scale_e), state["sums"]


def check_attempt(run, n, name, g="", seed=0):
    _, _, _, plant, want_branches, want_conv = ATTEMPT_CASES[name]
    st, entry = attempt_case(n, name, seed)
    dirty = sc.dirty_ctrl()
    got, gc = run("corrector", st, sc.ctrl_array(dirty), entry)
    c, branches, margins, y, d, psi, scale, sums = attempt_chain(n, st, entry)
    assert branches == want_branches, (branches, want_branches)
    assert not sc.margins_ok(margins, rel=1e-3), sc.margins_ok(margins, rel=1e-3)
    conv = bool(c["converged"][0])
    assert conv == bool(want_conv)
    if conv:
        assert sums["neg_margin"] > 1e-6
    neg = int(c["any_negative"][0]) if conv else 0
    assert neg == dict(shallow=1, deep=3).get(plant, 0)
    z = (LD(0), None)
    refs = dict(newton_done=(1, None), converged=(int(conv), None), n_iter=(len(branches), None), nonfinite=c["nonfinite"], any_negative=(neg, None),
                crate=c["crate"], lu_bad=(0, None), err_norm=c["err_norm"] if conv else z, err_m_norm=c["err_m_norm"] if conv else z,
                err_p_norm=c["err_p_norm"] if conv else z)
    check_ctrl(g + "attempt", gc, dirty, refs, (name, n))
    gd = sc.ctrl_dict(gc)
    assert gd["nonfinite"] == (1 if plant in ("nan_psi", "inf_inert", "nan_inert", "inf_psi_inert") else 0), name
    if conv:
        assert gd["err_m_norm"] == 0.0            # order 1 has no order - 1 sum
    rows = {ROW["psi"]: psi, ROW["scale"]: scale}
    if conv:
        rows.update({ROW["y"]: y, ROW["d"]: d})
        skip = ()
    else:
        skip = (ROW["y"], ROW["d"])                # a diverged attempt's state is never read (the step is retried from D)
    check_state(g + "attempt", got, st, rows, (name, n), skip=skip)
