"""Shared by tests/test_step_cases.py (no GPU) and tests/test_gpu_step_kernels.py: extended-precision references of the vector
operations between the phases of a BDF / Dormand-Prince step (kin_step_probe runs each of them once on the device), the
corrector's decision as a plain function of its five sums, the case lists, and the error bounds. A plain module: no fixtures, no
test collection.

The references are written from oracle/bdf.py (OracleBDF.step, _newton, interpolate, change_D - SciPy's BDF underneath) in
np.longdouble (64-bit mantissa), not from the kernels. tests/test_step_cases.py checks them against the oracle itself.

Bounds. u = 2^-53. Nothing below is fitted to what a device returned.
  * elementwise: a value computed by a chain of k floating-point operations on exact inputs differs from the exact result by at
    most (k + 1) u times the sum of the magnitudes added (standard forward bound k u / (1 - k u) of a sum of products, one unit
    of slack for u^2 terms and for the reference's own rounding, 2^-64 per operation). A fused multiply-add only removes a
    rounding. Where an input of the chain is itself a computed value, its bound is added.
  * reduced: every reduced quantity is a sum of n non-negative terms t_i. In ANY summation order the computed sum is within
    (n - 1) u of the exact sum of the computed terms, relatively; the computed terms carry an absolute error e_i each, worked
    out per term from the chain that produced it (e_i may be large relative to t_i where d + dy cancels). So
    |S_dev - S_ref| <= sum e_i + (n + 1) u S_ref, and a norm sqrt(S / n) (division and square root: two more roundings,
    the square root halves a relative error) is within  (sum e_i + (n + 1) u S) / (2 sqrt(S n)) + 3 u norm.
    For terms without cancellation e_i <= c u t_i and the whole is (n + c + 4) u / 2 relative: 'terms + a constant'.
"""
import numpy as np

from kinetica_jl_amd import capi
from oracle import bdf as obdf

LD = np.longdouble
U = LD(2.0) ** -53
GAMMA, ALPHA, ERRC = obdf.GAMMA, obdf.ALPHA, obdf.ERROR_CONST
NEG_DEEP = obdf.NEG_DEEP          # a species below -NEG_DEEP error weights: the deep flag (bdf_rules.hpp: BDF_NEG_DEEP)
MAXIT = obdf.NEWTON_MAXITER
ROW = capi.STEP_ROW
FIELDS = capi.STEP_CTRL_FIELDS
SENTINEL = -3.5e200               # fills the rows of D an operation must not touch
D_ROWS = 8

# sizes at which a kernel's structure changes: a wavefront, a workgroup of the elementwise kernels, RED_ELEMS = 1024 (one / two
# workgroups of the reductions, the stride of the norms kernel), five workgroups with one element in the last, 64 / 65
# workgroups (second round of newton_totals' lane loop)
SIZES_ELEM = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
SIZES_RED = SIZES_ELEM + (65536, 65537)
ORDERS = (1, 2, 3, 4, 5)
# step-size factors of change_D and the times of the dense output are dyadic: the host builds (i - 1 - factor j) / i and
# (ts - (t - h j)) / (h (1 + j)) with exact numerators and denominators, one rounding per quotient (the bounds below count that)
FACTORS = (0.25, 0.8125, 1.5, 10.0)
INTERP_T = dict(ts=0.96875, t=1.0, h_abs=0.125)
ATOL, RTOL = 1e-14, 1e-8          # the corrector cases: dy of a few weights cannot change the sign of a y >= 1e-12
TOL = 0.03                        # bdf_newton_tol(1e-8)


# ---------------------------------------------------------------------------------------------------------------- inputs
def signed_decades(rng, shape, lo=-12, hi=0):
    """mixed signs over 12 decades: sums over the rows of D cancel for real"""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(lo, hi, shape)


def make_state(n, seed, K=None, d_rows=D_ROWS):
    """every row of the block filled (what an operation leaves alone is then visible), rows of D from d_rows up the sentinel,
    scale consistent with y"""
    rng = np.random.default_rng(seed)
    st = signed_decades(rng, (K or 1, capi.STEP_ROWS, n))
    st[:, ROW["scale"]] = ATOL + RTOL * np.abs(st[:, ROW["y"]])
    st[:, d_rows:D_ROWS] = SENTINEL
    return st if K else st[0]


def dirty_ctrl(**kw):
    """a control block with every field set (a predictor has to clear exactly its list); ticket 0 as between launches"""
    c = dict(dy_norm_old=0.5, dy_norm=0.25, err_norm=0.125, err_m_norm=0.0625, err_p_norm=0.03125, crate=0.375, scratch0=1.0,
             scratch1=2.0, scratch2=3.0, scratch3=4.0, newton_done=1, converged=1, n_iter=3, nonfinite=1, any_negative=3, ticket=0,
             lu_bad=1, spec_go=1)
    c.update(kw)
    return c


def clean_ctrl(**kw):
    """as a predictor leaves it, the carried rate unknown"""
    c = {f: 0 for f in FIELDS}
    c.update(crate=1.0)
    c.update(kw)
    return c


def ctrl_array(c):
    return np.array([float(c[f]) for f in FIELDS])


def ctrl_dict(a):
    return {f: float(v) for f, v in zip(FIELDS, a)}


# ------------------------------------------------------------------------------------------------- elementwise references
# each returns {row index: (reference, bound)} of the rows the operation writes (longdouble arrays)
def ref_predict(D, order, atol, rtol, D_bound=None):
    """OracleBDF.step: y_pred = sum D[0..order], psi = D[1..order]^T gamma / alpha, scale = atol + rtol |y_pred|, d = 0.
    y: `order` additions -> (order + 1) u sum |D_j|; psi: order products, order - 1 additions, one division -> (2 order + 1) u
    sum |D_j gamma_j| / alpha; scale: a product and a sum on the COMPUTED y -> rtol * bound(y) + 3 u scale.
    D_bound: bounds of the rows of D where they are computed values themselves (accept_predict)."""
    D = D.astype(LD)
    Db = np.zeros_like(D) if D_bound is None else D_bound
    y = D[:order + 1].sum(axis=0)
    by = Db[:order + 1].sum(axis=0) + (order + 1) * U * np.abs(D[:order + 1]).sum(axis=0)
    g = GAMMA[1:order + 1].astype(LD)[:, None]
    psi = (D[1:order + 1] * g).sum(axis=0) / LD(ALPHA[order])
    bpsi = ((Db[1:order + 1] * g).sum(axis=0) + (2 * order + 1) * U * np.abs(D[1:order + 1] * g).sum(axis=0)) / LD(ALPHA[order])
    scale = LD(atol) + LD(rtol) * np.abs(y)
    return {ROW["y"]: (y, by), ROW["psi"]: (psi, bpsi), ROW["d"]: (np.zeros_like(y), np.zeros_like(y)),
            ROW["scale"]: (scale, LD(rtol) * by + 3 * U * scale)}


def ref_accept(D, d, order):
    """OracleBDF.step after acceptance: D[order + 2] = d - D[order + 1]; D[order + 1] = d; D[j] += D[j + 1] downwards, i.e.
    D[j] = d + sum_{i = j .. order} D[i]: order - j + 1 additions -> (order - j + 2) u (|d| + sum |D_i|); the top row one
    subtraction -> 2 u (|d| + |D[order + 1]|)."""
    D = D.astype(LD); d = d.astype(LD)
    out = {order + 2: (d - D[order + 1], 2 * U * (np.abs(d) + np.abs(D[order + 1]))), order + 1: (d, np.zeros_like(d))}
    carry, mag = d.copy(), np.abs(d)
    for j in range(order, -1, -1):
        carry = carry + D[j]; mag = mag + np.abs(D[j])
        out[j] = (carry, (order - j + 2) * U * mag)
    return out


def ru_matrix(order, factor):
    """(R(factor) R(1), |R(factor)| |R(1)|) of SciPy's change_D, in extended precision"""
    def R(f):
        I = np.arange(1, order + 1, dtype=LD)[:, None]
        J = np.arange(1, order + 1, dtype=LD)
        M = np.zeros((order + 1, order + 1), LD)
        M[1:, 1:] = (I - 1 - LD(f) * J) / I
        M[0] = 1
        return np.cumprod(M, axis=0)
    return R(factor).dot(R(1)), np.abs(R(factor)).dot(np.abs(R(1)))


def ref_change_D(D, order, factor):
    """D[:order + 1] <- (R(factor) R(1))^T D[:order + 1]. The matrix is built on the host in double (bdf_change_D_matrix) from
    a dyadic factor: an entry of M is one rounding (the quotient), R[i][j] a product of i such entries (<= 2 i roundings), an
    entry of R U a sum of order + 1 products of two such (<= 4 order + order + 1); the kernel adds order + 1 products and
    additions. In all at most 7 order + 3 operations on sums of magnitudes (|R| |U|)^T |D|, i.e. (7 order + 4) u by the
    module's (k + 1) u rule.
    The resident kernel builds the same matrix ON THE DEVICE (ResidentBdf::change_D: bdf_change_D_matrix compiled for gfx950, where
    the compiler may contract a product and the addition behind it into one fused multiply-add): the operations and their order are
    the host's, a contraction removes a rounding and adds none, and the numerators i - 1 - factor j stay exact for a dyadic factor
    either way - the count above covers it unchanged. The kernel's sum runs over all six columns with zeros beyond `order`
    (ph_change_D): adding an exact zero rounds nothing."""
    D = D.astype(LD)
    RU, A = ru_matrix(order, factor)
    new = RU.T.dot(D[:order + 1])
    bound = (7 * order + 4) * U * A.T.dot(np.abs(D[:order + 1]))
    return {j: (new[j], bound[j]) for j in range(order + 1)}


def ref_init_D(y0, f0, h):
    """OracleBDF.restart: D[0] = y0, D[1] = h f0 (one product -> 2 u |h f0|), the rest 0"""
    z = np.zeros(len(y0), LD)
    out = {j: (z, z) for j in range(2, D_ROWS)}
    out[0] = (y0.astype(LD), z)
    out[1] = (f0.astype(LD) * LD(h), 2 * U * np.abs(f0.astype(LD) * LD(h)))
    return out


def interp_weights(order, ts, t, h_abs):
    j = np.arange(order, dtype=LD)
    return np.cumprod((LD(ts) - (LD(t) - LD(h_abs) * j)) / (LD(h_abs) * (1 + j)))


def ref_interp(D, order, ts, t, h_abs):
    """OracleBDF.interpolate (Newton form): D[0] + sum_j p_j D[j], p = cumprod((ts - (t - h (j - 1))) / (h j)). Weights on the
    host from dyadic times: a quotient and a product each -> p_j within 2 j u; the kernel: order products and additions. At
    most 4 order operations."""
    D = D.astype(LD)
    p = interp_weights(order, ts, t, h_abs)[:, None]
    v = D[0] + (p * D[1:order + 1]).sum(axis=0)
    return {ROW["out"]: (v, (4 * order + 1) * U * (np.abs(D[0]) + np.abs(p * D[1:order + 1]).sum(axis=0)))}


def ref_clipped(v):
    """y <- chunk_start with the negative entries replaced by 0 (`v < 0 ? 0 : v`): a copy, so -0.0 (not below zero) and NaN (no
    comparison holds) come back as they are, bit for bit"""
    v = np.asarray(v, np.float64)
    return np.where(v < 0, 0.0, v)


def ref_axpy(y, f0, h0):
    """ytmp = y + h0 f0: a product and a sum (fused or not) -> 3 u (|y| + |h0 f0|)"""
    y = y.astype(LD); t = LD(h0) * f0.astype(LD)
    return y + t, 3 * U * (np.abs(y) + np.abs(t))


def ref_rk_combine(y, K, w, stages):
    """out = y + sum_{j < stages} w_j K_j: stages products, stages additions (the sum starts at 0, the state comes last)"""
    y = y.astype(LD); K = K.astype(LD); w = np.asarray(w, LD)[:, None]
    v = (w[:stages] * K[:stages]).sum(axis=0)
    return {ROW["out"]: (y + v, (2 * stages + 1) * U * (np.abs(y) + np.abs(w[:stages] * K[:stages]).sum(axis=0)))}


# --------------------------------------------------------------------------------------------------------------- reductions
def norm_with_bound(terms, errs, n):
    """sqrt(sum terms / n) and its bound from the per-term absolute errors (module docstring: reduced quantities)"""
    S = terms.sum()
    norm = np.sqrt(S / n)
    if not np.isfinite(S):
        return norm, LD(0)
    if S == 0:
        return norm, np.sqrt(errs.sum() / n)
    return norm, (errs.sum() + (n + 1) * U * S) / (2 * np.sqrt(S * n)) + 3 * U * norm


def sum_with_bound(terms, errs, n):
    """the raw sum S of n non-negative terms and its bound sum e_i + (n + 1) u S (module docstring: reduced quantities, before
    the division and the square root); a non-finite sum is compared as it is"""
    S = terms.sum()
    if not np.isfinite(S):
        return S, LD(0)
    return S, errs.sum() + (n + 1) * U * S


def sq_term(num, num_err, den, den_err, k):
    """t = (num / den)^2 and its absolute error: num, den computed with absolute errors num_err, den_err; k further operations
    on the quotient before squaring (the quotient itself, a constant factor), then the square."""
    inf_den = np.isinf(den) & np.isfinite(num)      # a finite numerator over an infinite weight: exactly 0
    den = np.where(inf_den, 1, den); den_err = np.where(inf_den, 0, den_err)
    num = np.where(inf_den, 0, num); num_err = np.where(inf_den, 0, num_err)
    q = num / den
    qe = np.abs(q) * (den_err / np.abs(den) + (k + 1) * U) + num_err / np.abs(den)
    return q * q, 2 * np.abs(q) * qe + qe * qe + U * q * q


def ref_norms(y, f0, f1, atol, rtol):
    """first-step norms (OracleBDF.restart / CVODE's cvHin): rms(y / w), rms(f0 / w), rms((f1 - f0) / w), max |f0| / (0.1 |y| + w),
    w = atol + rtol |y|; nonfinite when f0 or f1 has a NaN / Inf. w: a product and a sum -> 3 u w; every term then a quotient and
    a square; f1 - f0 one subtraction of exact inputs (2 u |f1 - f0|). The maximum: 0.1 |y| + w is three operations on positive
    terms, then a quotient: 6 u relative; taking the maximum is exact. Entries whose f0 is NaN do not enter the maximum
    (block_max_1024: fmax drops them); the sums they enter are NaN."""
    n = len(y)
    y = y.astype(LD); g0 = f0.astype(LD)
    w = LD(atol) + LD(rtol) * np.abs(y)
    we = 3 * U * w
    z = np.zeros(n, LD)
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        out["scratch0"] = norm_with_bound(*sq_term(y, z, w, we, 1), n)
        out["scratch1"] = norm_with_bound(*sq_term(g0, z, w, we, 1), n)
        if f1 is None:
            out["scratch2"] = (LD(0), LD(0))
        else:
            df = f1.astype(LD) - g0
            out["scratch2"] = norm_with_bound(*sq_term(df, 2 * U * np.abs(df), w, we, 1), n)
        m = np.abs(g0) / (LD(0.1) * np.abs(y) + w)
        vm = np.max(m[~np.isnan(m)]) if np.any(~np.isnan(m)) else LD(0)
    out["scratch3"] = (vm, 6 * U * vm if np.isfinite(vm) else LD(0))
    bad = not np.all(np.isfinite(f0)) or (f1 is not None and not np.all(np.isfinite(f1)))
    out["nonfinite"] = (float(bad), None)
    return out


def ref_newton_sums(x, scale, y, d, D, order, upd, atol, rtol, x_err=None, scale_err=None, y_err=None, d_err=None):
    """One corrector update (OracleBDF._newton: dy = upd x, y += dy, d += dy) and the five sums the decision needs:
      s  = sum (dy / scale)^2                                  (update norm, scale of the predictor)
      se = sum (ec[order] d / w)^2, w = atol + rtol |y_new|     (error test, OracleBDF.step; + inf when y_new is not finite)
      sm = sum (ec[order - 1] (D[order] + d) / w)^2, order > 1  (the order - 1 test: D[order] after the accept)
      sp = sum (ec[order + 1] (d - D[order + 1]) / w)^2, order < 5
      negative entries of y_new: any, and any below -NEG_DEEP w.
    dy: one product (2 u); y_new, d_new: one more addition -> 3 u (|.| + |dy|); w: a product and a sum on the computed y_new;
    numerators of sm, sp: one more addition. Returns dict(y, d: (ref, bound); s, se, sm, sp: (terms, errs); neg, deep: bool).
    Non-finite inputs: s is Inf or NaN as its terms are. se of a non-finite y_new is given as +inf here; the kernels add +inf to the
    term ec d_new / w squared, which is 0 for an infinite y_new under a finite update (w is infinite) - se is then exactly +inf -
    and Inf / Inf or a NaN otherwise: there, and for sm and sp, only `not finite` is specified (the attempt reads !isfinite(se), and
    nothing but the flag once s is non-finite).
    x_err, scale_err, y_err, d_err: absolute error bounds of inputs that are computed values themselves (an attempt's later
    iterations: tests/resident_step_cases.py); they enter where the input enters, |upd| x_err next to dy's own rounding."""
    x = x.astype(LD); scale = scale.astype(LD); y = y.astype(LD); d = d.astype(LD); D = D.astype(LD)
    z = np.zeros(len(x), LD)
    x_err, scale_err, y_err, d_err = (z if e is None else np.asarray(e, LD) for e in (x_err, scale_err, y_err, d_err))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dy = LD(upd) * x
        dye = 2 * U * np.abs(dy) + abs(LD(upd)) * x_err
        yn, dn = y + dy, d + dy
        yne = dye + y_err + 2 * U * (np.abs(y) + np.abs(dy))
        dne = dye + d_err + 2 * U * (np.abs(d) + np.abs(dy))
        out = dict(y=(yn, yne + U * np.abs(yn)), d=(dn, dne + U * np.abs(dn)))
        out["s"] = sq_term(dy, dye, scale, scale_err, 1)
        w = LD(atol) + LD(rtol) * np.abs(yn)
        we = LD(rtol) * yne + 3 * U * w
        ec = [LD(v) for v in ERRC]
        t, e = sq_term(ec[order] * dn, np.abs(ec[order]) * dne, w, we, 2)
        fin = np.isfinite(yn)
        out["se"] = (np.where(fin, t, np.inf), np.where(fin, e, 0))
        if order > 1:
            num = D[order] + dn
            out["sm"] = sq_term(ec[order - 1] * num, np.abs(ec[order - 1]) * (dne + 2 * U * (np.abs(D[order]) + np.abs(dn))), w, we, 2)
        else:
            out["sm"] = (z, z)
        if order < 5:
            num = dn - D[order + 1]
            out["sp"] = sq_term(ec[order + 1] * num, np.abs(ec[order + 1]) * (dne + 2 * U * (np.abs(D[order + 1]) + np.abs(dn))), w, we, 2)
        else:
            out["sp"] = (z, z)
        out["neg"] = bool(np.any(yn < 0))
        out["deep"] = bool(np.any(yn < -LD(NEG_DEEP) * w))
        # how far the sign tests are from flipping, in units of the compared magnitudes
        out["neg_margin"] = float(np.min(np.abs(yn[fin]) / (np.abs(y[fin]) + np.abs(dy[fin]) + LD(1e-300)))) if np.any(fin) else 1.0
    return out


def ref_decide(sums, n, ctrl, iter=0, maxit=MAXIT, tol=TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0, dy_first_max=0.2,
               crate_from_ctrl=0, ban_negatives=0, **_):
    """The decision of one corrector iteration as a function of the sums - OracleBDF._newton's tests in its order (rate from the
    previous update norm; diverged by rate >= rate_max or by the estimate rate^(maxit - iter) / (1 - rate) dy > tol; converged
    by dy == 0, by rate / (1 - rate) dy < tol, on the first iteration by dy < tol or by the carried rate: crate0 < 1,
    dy <= dy_first_max, crate0 / (1 - crate0) dy < tol_first), CVODE's carried rate crate <- max(0.3 crate, rate), and the
    verdict `spec_go` = what OracleBDF.step concludes from an attempt: accepted, nothing that makes the next step more than a
    continuation. Returns (control block after: {field: (value, bound or None = exact)}, branch, published: bool-without-
    publish_always, margins: [(name, quantity, threshold)])."""
    c = {f: (LD(ctrl[f]), None) for f in FIELDS}
    if ctrl["newton_done"]:
        return c, "behind", False, []
    margins = []
    S = sums["s"][0].sum()
    dy, dyb = norm_with_bound(*sums["s"], n)
    nonfinite = not np.isfinite(S)
    have_rate = iter > 0
    cr0 = LD(ctrl["crate"]) if (crate_from_ctrl and iter == 0) else LD(crate0)
    crate = cr0 if iter == 0 else LD(ctrl["crate"])
    crate_b = None
    rate = rel = LD(0)
    if have_rate and not nonfinite:
        rate = dy / LD(ctrl["dy_norm_old"])
        rel = dyb / dy + U if dy > 0 else LD(0)      # relative error of the rate (dy_norm_old is an exact input)
        if rate > LD(0.3) * crate:
            crate, crate_b = rate, rate * rel
        else:
            crate = LD(0.3) * crate
            crate_b = U * crate
        margins.append(("rate vs 0.3 crate", rate, LD(0.3) * LD(ctrl["crate"])))
    c["crate"] = (crate, crate_b)
    c["n_iter"] = (LD(iter + 1), None)
    c["dy_norm"] = (dy, dyb)
    diverged, branch = nonfinite, "nonfinite" if nonfinite else None
    if not diverged and have_rate:
        est = rate ** (maxit - iter) / (1 - rate) * dy
        margins += [("rate vs rate_max", rate, LD(rate_max)), ("divergence estimate vs tol", est, LD(tol))]
        if rate >= rate_max:
            diverged, branch = True, "diverged_rate_max"
        elif est > tol:
            diverged, branch = True, "diverged_estimate"
    done, converged = True, False
    if diverged:
        c["nonfinite"] = (LD(nonfinite), None)
    else:
        if dy == 0:
            converged, branch = True, "zero_update"
        elif have_rate:
            est1 = rate / (1 - rate) * dy
            margins.append(("convergence estimate vs tol", est1, LD(tol)))
            if est1 < tol:
                converged, branch = True, "converged_rate"
        else:
            margins.append(("dy_norm vs tol", dy, LD(tol)))
            if dy < tol:
                converged, branch = True, "converged_first_tol"
            else:
                ok = [cr0 < 1, dy <= dy_first_max, cr0 / (1 - cr0) * dy < tol_first if cr0 < 1 else False]
                margins.append(("dy_norm vs dy_first_max", dy, LD(dy_first_max)))      # (crate0 < 1 tests an exact input)
                if cr0 < 1:
                    margins.append(("carried estimate vs tol_first", cr0 / (1 - cr0) * dy, LD(tol_first)))
                if all(ok):
                    converged, branch = True, "converged_carried_rate"
                else:
                    branch = "refused_" + "_".join(nm for nm, v in zip(("crate", "dymax", "estimate"), ok) if not v)
        if not converged:
            c["dy_norm_old"] = (dy, dyb)
            done = iter == maxit - 1
            branch = (branch + "_" if branch else "") + ("exhausted" if done else "continue")
    if converged:
        for f, q in (("err_norm", "se"), ("err_m_norm", "sm"), ("err_p_norm", "sp")):
            c[f] = norm_with_bound(*sums[q], n)
        c["any_negative"] = (LD(3 if sums["deep"] else 1 if sums["neg"] else 0), None)
        if not np.isfinite(sums["se"][0].sum()):
            c["nonfinite"] = (LD(1), None)
        else:
            margins.append(("err_norm vs 1", c["err_norm"][0], LD(1)))
    c["converged"] = (LD(converged), None)
    c["newton_done"] = (LD(done), None)
    neg = int(c["any_negative"][0])
    go = (done and converged and not c["nonfinite"][0] and not ctrl["lu_bad"] and not (ban_negatives and neg) and not (neg & 2)
          and not (c["err_norm"][0] > 1) and iter + 1 < maxit)
    c["spec_go"] = (LD(bool(go)), None)
    return c, branch, done, margins


def margins_ok(margins, rel=1e-6):
    """every tested quantity at least `rel` (relative to the threshold's magnitude, or absolutely when that is 0) away from
    its threshold - orders above any reduction bound, so device and reference take the same branch"""
    bad = [(nm, float(q), float(t)) for nm, q, t in margins if not abs(q - t) >= rel * max(abs(t), abs(q) if t == 0 else 0, 1e-300)]
    return bad


def ref_rk_error(y, y_new, K, e, atol, rtol):
    """err_norm = rms((sum_j e_j K_j) / (atol + rtol max(|y|, |y_new|))) (SciPy's RK45 error norm); any_negative: y_new < 0
    somewhere; nonfinite: y_new has a NaN / Inf (a NaN drops out of fmax, so the norm itself stays finite then) or the norm
    is not finite. Numerator: 7 products, 6 additions -> 14 u sum |e_j K_j|; denominator: a product and a sum -> 3 u."""
    n = len(y)
    y = y.astype(LD); yn = y_new.astype(LD); K = K.astype(LD); e = np.asarray(e, LD)[:, None]
    with np.errstate(invalid="ignore"):
        num = (e * K).sum(axis=0)
        w = LD(atol) + LD(rtol) * np.fmax(np.abs(y), np.abs(yn))
        norm = norm_with_bound(*sq_term(num, 14 * U * np.abs(e * K).sum(axis=0), w, 3 * U * w, 1), n)
        neg = bool(np.any(yn < 0))
    bad = (not np.all(np.isfinite(y_new))) or not np.isfinite(norm[0])
    return dict(err_norm=norm, any_negative=(LD(neg), None), nonfinite=(LD(bad), None))


# ------------------------------------------------------------------------------------------------------- corrector cases
def unit_rms(rng, n):
    z = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)
    return z * np.sqrt(n / np.sum(z * z))


def newton_inputs(n, seed, order, g, upd=1.0, d_weights=0.05, negative=None, x_bad=None, y_inf=False, y_hook=None):
    """state for one corrector update whose norm is g error weights: y >= 1e-12 (positive: the sign of y_new is under the case's
    control), scale = ATOL + RTOL |y|, d of d_weights error weights, D[order], D[order + 1] of about a weight, rows of D above
    order + 1 the sentinel (at order 5 row 6 too: the order + 1 sum has nothing to read there); x = g z scale / upd, rms(z) = 1.
    negative: None | 'shallow' (the LAST element ends at -3 weights) | 'deep' (element n // 2 at -1e4 weights);
    x_bad: a non-finite value for x[n // 3]; y_inf: y[n // 3] = inf with a finite update; y_hook: y <- y_hook(y) before anything
    is derived from it (tests/resident_step_cases.py ties the two species of a pair together)."""
    rng = np.random.default_rng(seed)
    st = make_state(n, seed, d_rows=min(order + 2, D_ROWS) if order < 5 else 6)
    y = 10.0 ** rng.uniform(-12, 0, n)
    if negative == "shallow":
        y[n - 1] = -3.0 * ATOL
    elif negative == "deep":
        y[n // 2] = -1e4 * ATOL
    if y_inf:
        y[n // 3] = np.inf
    if y_hook is not None:
        y = y_hook(y)
    scale = ATOL + RTOL * np.abs(y)
    scale[~np.isfinite(scale)] = 1.0
    st[ROW["y"]] = y
    st[ROW["scale"]] = scale
    st[ROW["d"]] = d_weights * scale * unit_rms(rng, n) / ERRC[order]
    st[order] = scale * signed_decades(rng, n, -2, 0)
    if order < 5:
        st[order + 1] = scale * signed_decades(rng, n, -2, 0)
    x = g * unit_rms(rng, n) * scale / upd
    if x_bad is not None:
        x[n // 3] = x_bad
    st[ROW["x"]] = x
    return st, rng.permutation(n).astype(np.int32)


# name -> (inputs: keyword arguments of newton_inputs, entry: arguments of the launch, ctrl: fields over clean_ctrl(),
#          expected branch of ref_decide, expected spec_go). g is the update norm in error weights; TOL = 0.03.
DECISION_CASES = {
    # first iteration
    "first_converged_by_tol": (dict(g=0.01), dict(), dict(), "converged_first_tol", 1),
    "first_converged_by_carried_rate": (dict(g=0.1), dict(crate0=0.1, tol_first=TOL), dict(), "converged_carried_rate", 1),
    "first_refused_rate_unknown": (dict(g=0.1), dict(crate0=1.0, tol_first=TOL), dict(), "refused_crate_estimate_continue", 0),
    "first_refused_test_off": (dict(g=0.1), dict(crate0=0.1, tol_first=-1.0), dict(), "refused_estimate_continue", 0),
    "first_refused_update_too_large": (dict(g=0.25), dict(crate0=0.05, tol_first=TOL), dict(), "refused_dymax_continue", 0),
    "first_refused_estimate_too_large": (dict(g=0.1), dict(crate0=0.5, tol_first=TOL), dict(), "refused_estimate_continue", 0),
    "first_rate_from_ctrl": (dict(g=0.1), dict(crate0=1.0, tol_first=TOL, crate_from_ctrl=1), dict(crate=0.1), "converged_carried_rate", 1),
    "first_rate_from_ctrl_unknown": (dict(g=0.1), dict(crate0=0.1, tol_first=TOL, crate_from_ctrl=1), dict(crate=1.0),
                                     "refused_crate_estimate_continue", 0),
    "zero_update": (dict(g=0.0), dict(), dict(), "zero_update", 1),
    "only_iteration_exhausted": (dict(g=0.1), dict(maxit=1), dict(), "refused_crate_estimate_exhausted", 0),
    # second and later iterations (dy_norm_old = the norm of the update before)
    "second_converged": (dict(g=0.01), dict(iter=1, rate_max=0.15), dict(dy_norm_old=0.1, n_iter=1, crate=0.2), "converged_rate", 1),
    "second_converged_crate_decays": (dict(g=0.01), dict(iter=1, rate_max=0.15), dict(dy_norm_old=0.1, n_iter=1, crate=0.5), "converged_rate", 1),
    "second_diverged_rate_max": (dict(g=0.02), dict(iter=1, rate_max=0.15), dict(dy_norm_old=0.1, n_iter=1), "diverged_rate_max", 0),
    "second_diverged_estimate": (dict(g=0.09), dict(iter=1), dict(dy_norm_old=0.1, n_iter=1), "diverged_estimate", 0),
    "second_continues": (dict(g=0.2), dict(iter=1), dict(dy_norm_old=1.0, n_iter=1), "continue", 0),
    "last_converged_no_go": (dict(g=0.001), dict(iter=3), dict(dy_norm_old=0.1, n_iter=3), "converged_rate", 0),
    # non-finite
    "nonfinite_update_inf": (dict(g=0.01, x_bad=np.inf), dict(), dict(), "nonfinite", 0),
    "nonfinite_update_nan": (dict(g=0.01, x_bad=np.nan), dict(iter=1), dict(dy_norm_old=0.1, n_iter=1, crate=0.4), "nonfinite", 0),
    "nonfinite_state_converged": (dict(g=0.01, y_inf=True), dict(), dict(), "converged_first_tol", 0),
    # the terms of spec_go, one at a time on a converged first iteration
    "go_lu_bad": (dict(g=0.01), dict(), dict(lu_bad=1), "converged_first_tol", 0),
    "go_shallow_negative_allowed": (dict(g=0.01, negative="shallow"), dict(), dict(), "converged_first_tol", 1),
    "go_shallow_negative_banned": (dict(g=0.01, negative="shallow"), dict(ban_negatives=1), dict(), "converged_first_tol", 0),
    "go_deep_negative": (dict(g=0.01, negative="deep"), dict(), dict(), "converged_first_tol", 0),
    "go_error_test_fails": (dict(g=0.01, d_weights=30.0), dict(), dict(), "converged_first_tol", 0),
    # a launch behind the decision
    "behind_a_decision": (dict(g=0.01), dict(publish_always=1), dict(newton_done=1, converged=1, n_iter=2, spec_go=1), "behind", 1),
}


def decision_case(name, n=257, order=3, seed=0):
    """(state, xloc, entry, ctrl dict) of a decision case"""
    inp, ent, ct, _, _ = DECISION_CASES[name]
    st, xloc = newton_inputs(n, 1000 + seed, order, **inp)
    entry = dict(order=order, atol=ATOL, rtol=RTOL, upd=1.0, tol=TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0, dy_first_max=0.2,
                 iter=0, maxit=MAXIT, seq=7)
    entry.update(ent)
    return st, xloc, entry, clean_ctrl(**ct)


def newton_reference(st, entry, ctrl):
    """reference of a corrector launch on the block `st` (x in its row): (sums, control block after, branch, decided, margins)"""
    n = st.shape[1]
    sums = ref_newton_sums(st[ROW["x"]], st[ROW["scale"]], st[ROW["y"]], st[ROW["d"]], st[:D_ROWS], entry["order"],
                           entry.get("upd", 1.0), entry["atol"], entry["rtol"])
    c, branch, done, margins = ref_decide(sums, n, ctrl, **{k: v for k, v in entry.items() if k not in ("order", "atol", "rtol", "upd")})
    return sums, c, branch, done, margins


# the sums across the reduction sizes: (order, upd, negative); every one converges on its first iteration (g = 0.01)
SUM_CASES = [(1, 1.0, None), (3, 0.8, "shallow"), (5, 1.0, "deep"), (3, 1.0, None), (5, 0.8, None)]

# Dormand-Prince weights as the solver passes them (h times the tableau's row): values only matter as mixed-sign weights
RK_B = np.array([35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0])
RK_E = np.array([-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40])


def newton_case_list():
    """every corrector launch the GPU file runs on paths 0 and 2 whose decision is compared: (id, builder) with builder() ->
    (state, xloc, entry, ctrl dict). tests/test_step_cases.py checks the threshold margins of each one."""
    out = []
    for name in DECISION_CASES:
        for n in (257, 1025):
            out.append((f"{name}-n{n}", lambda name=name, n=n: decision_case(name, n=n, order=3, seed=n)))
    for order, upd, negative in SUM_CASES:
        for n in SIZES_RED:
            def build(order=order, upd=upd, negative=negative, n=n):
                st, xloc = newton_inputs(n, 5000 + 10 * n + order, order, g=0.01, upd=upd, negative=negative)
                entry = dict(order=order, atol=ATOL, rtol=RTOL, upd=upd, tol=TOL, rate_max=1.0, crate0=1.0, tol_first=-1.0,
                             dy_first_max=0.2, iter=0, maxit=MAXIT, seq=3)
                return st, xloc, entry, clean_ctrl()
            out.append((f"sums-o{order}-upd{upd}-{negative}-n{n}", build))
    return out
