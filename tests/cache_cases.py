"""Shared by tests/test_cache_cases.py (no GPU) and tests/test_gpu_lu_cache.py: references of the LU cache's drift guard and of its
slot rules, written from their definitions (never from bdf_rules.hpp, the kernels or oracle/), the bound a computed drift is
judged with, and the cases. A plain module: no fixtures, no test collection.

Drift reference. Slot s was factorised at c_s with diag(J) = jd_s; today's diagonal is jd_now. Per element
    M_old = 1 - c_s jd_s[i],   M_new = 1 - c_s jd_now[i],   Q = M_old / M_new,   DEV_i = max(Q, 1 / Q),
the slot's drift is max_i DEV_i - 1, never below 0. A Q that is not positive (a sign change, a vanished M_old) or not a number
counts as unbounded, and so does M_new = 0: the reference reports inf there, an implementation at least 1e299. A slot is dropped
when its drift is not <= max_drift; an invalid slot reports 0 and stays as it is. Everything in np.longdouble (64-bit mantissa),
the exact cases in rationals.

Bound (u = 2^-53; derived, nothing here is fitted to what a device returned). fl(1 - fl(c jd)) is M (1 + e) with
|e| <= kappa u, kappa = 1 + |c jd| / |M| (the product's rounding is amplified by |c jd| / |M|, the subtraction adds one; a fused
multiply-add only removes a rounding). The quotient of two such values, its rounding, the reciprocal's and the final
subtraction's give |DEV_i(computed) - DEV_i| <= DEV_i (kappa_old,i + kappa_new,i + 3) u to first order, and with
|max a - max b| <= max |a - b|
    |out_s - ref_s| <= max_i [DEV_i (kappa_old,i + kappa_new,i + 3)] u + u |ref_s|.
(the last term covers the reference's own 2^-64 roundings with room to spare). The generator asserts |M| >= 2^-40 (1 + |c jd|)
wherever a finite drift is expected, so no sign is left open (the sign-change cases place M far from 0), and that no case's
drop decision lies within its bound of max_drift - except the exact cases, which sit at the threshold on purpose.

Exact cases. c a power of two, every jd an integer (or 3 + 2^-50), every Q a power of two (or 2 + 2^-51): M, Q, 1 / Q and the
result carry no rounding, so every correct evaluation returns the reference bit for bit. Q = 2 and Q = 1 / 2 give drift 1.0
exactly: kept at max_drift = 1.0 (the rule is <=); jd_old = -(3 + 2^-50), jd_new = -1, c = 1 gives 1 + 2^-51: dropped.

Slot rules (the statement the table's expectations come from):
  nearest(c)   among the slots i < n_slots that are valid, whose Jacobian is at most max_age restarts old
               (n_restarts - jac_stamp <= max_age) and - with step_age >= 0 - at most step_age accepted steps old, and whose
               c_fact is within the band (|c / c_fact - 1| <= band): the one with the smallest |log(c / c_fact)|, the lowest
               index among equals; -1 when there is none.
  victim       the lowest i < n_slots that is not valid or whose Jacobian is more than max_age restarts old; when there is none,
               the slot with the smallest last_use, the lowest index among equals. (n_slots = 0 names no slot.)"""
import math
from fractions import Fraction

import numpy as np

from kinetica_jl_amd.synth import from_lists
from tests.linalg_cases import core_net, with_special_stoichiometries

LD = np.longdouble
U = LD(2.0) ** -53
UNBOUNDED = 1e299                           # what every implementation reports at least for an unbounded drift
LU_MAX_SLOTS, RES_MAX_SLOTS = 128, 64       # solver_kernels.hpp, resident_core.hpp
HOST_N = (2, 63, 64, 65, 1023, 1024, 1025, 2049)
RES_N = (2, 63, 64, 65, 128, 129, 400)
HOST_SLOTS = (1, 2, 127, 128)
RES_SLOTS = (1, 2, 8, 9, 63, 64)
SPIKES = (0, 63, 64, 1023, 1024, -1)        # -1: N - 1
SENTINEL = -7.0                             # what the resident probe leaves where ph_drift wrote nothing


# ------------------------------------------------------------------------------------------------------------ networks
def chain_net(n):
    """reversible first-order chain 0 <-> 1 <-> ... <-> n - 1 (every species a reactant: every diagonal entry has terms)"""
    reacs, prods = [], []
    for i in range(n - 1):
        reacs += [[(i, 1)], [(i + 1, 1)]]; prods += [[(i + 1, 1)], [(i, 1)]]
    return from_lists(n, reacs, prods)


def special_net():
    """2A -> B, A -> 2B, an inert collider and a product that is also a reactant, on a small dense core with chains"""
    return with_special_stoichiometries(core_net(12))


# ------------------------------------------------------------------------------------------------------------ drift reference
def drift_reference(c, valid, jd_old, jd_now):
    """(drift[ns] as float64 with inf for unbounded, bound[ns]) of the slots (c[ns], valid[ns], jd_old[ns][N]) against jd_now[N]"""
    ns = len(c)
    drift = np.zeros(ns); bound = np.zeros(ns)
    now = np.asarray(jd_now, np.float64).astype(LD)
    for s in range(ns):
        if not valid[s]:
            continue
        cs = LD(c[s])
        old = np.asarray(jd_old[s], np.float64).astype(LD)
        with np.errstate(all="ignore"):
            m_old, m_new = LD(1) - cs * old, LD(1) - cs * now
            q = m_old / m_new
            fin = (q > 0) & np.isfinite(q)
            dev = np.where(fin, np.maximum(q, LD(1) / q), LD(1))
            k_old = LD(1) + np.abs(cs * old) / np.abs(m_old)
            k_new = LD(1) + np.abs(cs * now) / np.abs(m_new)
            if not fin.all():
                drift[s], bound[s] = np.inf, 0.0
                continue
            assert np.all(np.abs(m_old) >= LD(2.0) ** -40 * (1 + np.abs(cs * old))) and np.all(np.abs(m_new) >= LD(2.0) ** -40 * (1 + np.abs(cs * now)))
            ref = dev.max() - LD(1)
            drift[s] = float(ref)
            bound[s] = float((dev * (k_old + k_new + 3)).max() * U + U * abs(ref))
    return drift, bound


def drift_exact(c, jd_old, jd_now):
    """one slot's drift in rationals (every input a dyadic rational, no special values); Fraction"""
    cs = Fraction(float(c))
    worst = Fraction(1)
    for a, b in zip(jd_old, jd_now):
        q = (1 - cs * Fraction(float(a))) / (1 - cs * Fraction(float(b)))
        assert q > 0
        worst = max(worst, q, 1 / q)
    return worst - 1


def drift_float64(c, valid, jd_old, jd_now):
    """the formula in plain float64 NumPy, operation by operation (what the bound is tried on without a device)"""
    out = np.zeros(len(c))
    for s in range(len(c)):
        if not valid[s]:
            continue
        with np.errstate(all="ignore"):
            q = (1.0 - c[s] * np.asarray(jd_old[s])) / (1.0 - c[s] * np.asarray(jd_now))
            dev = np.where(q > 0.0, np.maximum(q, 1.0 / q), 1e300)
            dev = np.where(np.isnan(dev), 1e300, dev)
        out[s] = max(1.0, dev.max()) - 1.0
    return out


def decisions(drift, valid, max_drift):
    """dropped[ns]: valid and not drift <= max_drift"""
    return np.array([bool(v) and not (d <= max_drift) for d, v in zip(drift, valid)])


# ------------------------------------------------------------------------------------------------------------ drift cases
class DriftCase:
    """name, N, c[ns], valid[ns], jd_old[ns][N], jd_now[N], max_drift; exact: results bit for bit; poison: NaN in every
    off-diagonal Jacobian value; ref / bound / dropped from the reference"""

    def __init__(self, name, c, valid, jd_old, jd_now, max_drift=1.0, exact=False, poison=False, check=True):
        self.name = name
        self.c = np.asarray(c, np.float64); self.valid = np.asarray(valid, np.int32)
        self.jd_old = np.asarray(jd_old, np.float64); self.jd_now = np.asarray(jd_now, np.float64)
        self.ns, self.N = self.jd_old.shape
        assert self.c.shape == (self.ns,) and self.valid.shape == (self.ns,) and self.jd_now.shape == (self.N,)
        self.max_drift, self.exact, self.poison = max_drift, exact, poison
        self.ref, self.bound = drift_reference(self.c, self.valid, self.jd_old, self.jd_now)
        self.dropped = decisions(self.ref, self.valid, max_drift)
        if exact:
            for s in range(self.ns):
                if self.valid[s]:
                    assert Fraction(float(self.ref[s])) == drift_exact(self.c[s], self.jd_old[s], self.jd_now), name
        elif check:
            fin = np.isfinite(self.ref) & (self.valid != 0)
            # no decision within its bound of the threshold
            assert np.all(np.abs(self.ref[fin] - max_drift) > 4 * self.bound[fin] + 1e-9), name

    def __repr__(self):
        return self.name


def spike_positions(N):
    return sorted({p if p >= 0 else N - 1 for p in SPIKES if p < N})


def _spiked(rng, N, ns, positions, valid=None, name="", max_drift=1.0, poison=False, zero_at=()):
    """ns slots with a c of their own each; slot s differs from today's diagonal at positions[s % len] only, by a magnitude of
    its own: growth and shrinkage alternate, drifts on either side of max_drift"""
    c = 1e-3 * 100.0 ** ((np.arange(ns) * 0.6180339887) % 1.0) * rng.uniform(0.9, 1.1, ns)
    jd_now = -(10.0 ** rng.uniform(1.0, 2.0, N))
    for z in zero_at:
        jd_now[z] = 0.0
    jd_old = np.tile(jd_now, (ns, 1))
    mags = (1.4, 0.55, 7.0, 0.08, 2.6, 0.3, 30.0, 0.02)
    for s in range(ns):
        p = positions[s % len(positions)]
        if jd_now[p] == 0.0:
            jd_now[p] = -33.0; jd_old[:, p] = -33.0
        jd_old[s, p] = jd_now[p] * mags[s % len(mags)] * (1.0 + 0.01 * (s // len(mags)))
    valid = np.ones(ns, np.int32) if valid is None else np.asarray(valid, np.int32)
    case = DriftCase(name, c, valid, jd_old, jd_now, max_drift, poison=poison)
    # another slot's c or jd row changes the answer by more than the bounds
    for s in range(ns):
        o = (s + 1) % ns
        if ns > 1 and valid[s] and valid[o]:
            alt_c, _ = drift_reference([c[o]], [1], [jd_old[s]], jd_now)
            alt_r, _ = drift_reference([c[s]], [1], [jd_old[o]], jd_now)
            for alt in (alt_c[0], alt_r[0]):
                assert abs(alt - case.ref[s]) > 8 * case.bound[s] + 1e-9, (name, s)
    return case


def placement_case(N, seed=0):
    """one slot per spike position of SPIKES that exists at N"""
    pos = spike_positions(N)
    return _spiked(np.random.default_rng(1000 + N + seed), N, len(pos), pos, name=f"placement N={N}")


def slots_case(N, ns, seed=0):
    """ns slots, valid and invalid mixed (every third invalid; the last slot always valid), spikes cycling over the positions"""
    valid = np.array([0 if s % 3 == 1 else 1 for s in range(ns)], np.int32)
    valid[-1] = 1
    pos = spike_positions(N) + [N // 2, N // 3]
    return _spiked(np.random.default_rng(2000 + 7 * N + ns + seed), N, ns, pos, valid, name=f"slots N={N} ns={ns}",
                   zero_at=(1,) if N > 2 else ())


def exact_cases(N):
    """the threshold cases, bit for bit (module docstring)"""
    base = -np.arange(1.0, N + 1.0)
    # c = 1/4, jd_now[p] = -4: M_new = 2; jd_old = -12, 0, -28, 3: M_old = 4, 1, 8, 1/4, so Q = 2, 1/2, 4, 1/8
    p = N - 1
    now = base.copy(); now[p] = -4.0
    rows = []
    for old in (-12.0, 0.0, -28.0, 3.0):
        r = now.copy(); r[p] = old; rows.append(r)
    a = DriftCase(f"exact powers of two N={N}", [0.25] * 4, [1] * 4, rows, now, 1.0, exact=True)
    assert list(a.ref) == [1.0, 1.0, 3.0, 7.0] and list(a.dropped) == [False, False, True, True]
    now2 = base.copy(); now2[0] = -1.0
    r2 = now2.copy(); r2[0] = -(3.0 + 2.0 ** -50)
    b = DriftCase(f"exact one ulp above N={N}", [1.0], [1], [r2], now2, 1.0, exact=True)
    assert b.ref[0] == 1.0 + 2.0 ** -51 and b.dropped[0]
    return [a, b]


def special_cases(N):
    """each special value in a case of its own (3 slots, slot 1 the one concerned where it is a slot's matter)"""
    rng = np.random.default_rng(3000 + N)
    out = []
    g = _spiked(rng, N, 3, [0, N - 1, N // 2], name="template")
    q = N // 3                                    # the element the special value sits at (no slot's spike)

    def variant(name, edit, **kw):
        c, jd_old, jd_now = edit(g.c.copy(), g.jd_old.copy(), g.jd_now.copy())
        return DriftCase(f"{name} N={N}", c, [1, 1, 1], jd_old, jd_now, check=False, **kw)

    def nan_today(c, o, n):
        n[q] = np.nan; return c, o, n
    def nan_saved(c, o, n):
        o[1, q] = np.nan; return c, o, n
    def sign_change(c, o, n):
        n[q] = 4.0 / c[1]; o[:, q] = n[q]; o[1, q] = -1.0 / c[1]; return c, o, n      # slot 1: M_new = -3, M_old = 2
    def m_new_zero(c, o, n):
        c[1] = 0.5; n[q] = 2.0; o[:, q] = 2.0; o[1, q] = -2.0; return c, o, n         # slot 1: M_new = 0 exactly, M_old = 2
    def positive_diag(c, o, n):
        n[q] = 0.75 / c[1]; o[:, q] = n[q]; o[1, q] = 0.4 / c[1]; return c, o, n      # autocatalytic: c jd = 0.75 today, 0.4 then
    def never_reactant(c, o, n):
        n[q] = 0.0; o[:, q] = 0.0; return c, o, n
    out.append(variant("NaN today", nan_today))
    out.append(variant("NaN saved", nan_saved))
    sc = variant("sign change", sign_change)
    out.append(sc)
    out.append(variant("M_new zero", m_new_zero))
    pd = variant("positive diagonal", positive_diag)
    out.append(pd)
    out.append(variant("never a reactant", never_reactant))
    out.append(variant("poisoned off-diagonals", lambda c, o, n: (c, o, n), poison=True))
    assert np.all(np.isinf(out[0].ref)) and out[0].dropped.all()
    assert np.isinf(out[1].ref[1]) and np.isfinite(out[1].ref[[0, 2]]).all()
    assert np.isinf(sc.ref[1]) and sc.dropped[1] and np.isinf(out[3].ref[1]) and out[3].dropped[1]
    # the other slots of the sign-change / M_new = 0 / positive-diagonal cases see a positive c jd of their own at q
    for case in out:
        fin = np.isfinite(case.ref)
        assert np.all(np.abs(case.ref[fin] - case.max_drift) > 4 * case.bound[fin] + 1e-9), case.name
    assert np.isfinite(pd.ref).all() and pd.ref[1] >= 1.39                           # 0.6 / 0.25 - 1
    return out


def host_cases():
    """(N, [cases]) of the host-driven path"""
    out = []
    for N in HOST_N:
        cs = [placement_case(N)] + exact_cases(N)
        if N == 65:
            cs += [slots_case(N, ns) for ns in HOST_SLOTS] + special_cases(N)
        if N == 1025:
            cs += [slots_case(N, 3)]
        out.append((N, cs))
    return out


def resident_cases():
    """(N, [cases]) of the resident kernel"""
    out = []
    for N in RES_N:
        cs = [placement_case(N)] + exact_cases(N)
        if N == 65:
            cs += [slots_case(N, ns) for ns in RES_SLOTS] + special_cases(N)
        if N == 400:
            cs += [slots_case(N, 9)]
        out.append((N, cs))
    return out


def special_net_cases(N):
    """the cases of the network with special stoichiometries (N its species count)"""
    return [placement_case(N, seed=5), slots_case(N, 9, seed=5)] + exact_cases(N)


def jac_values(case, rowptr, col, seed=0):
    """(jv_slots[ns][nnz], jv_now[nnz]) in the pattern's order: the case's diagonals, everything else random (or NaN)"""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    rows = np.repeat(np.arange(case.N), np.diff(rowptr))
    diag = np.flatnonzero(rows == col)
    assert len(diag) == case.N and np.array_equal(col[diag], np.arange(case.N))
    rng = np.random.default_rng(seed)
    def fill(d):
        v = np.full(len(col), np.nan) if case.poison else rng.uniform(-1.0, 1.0, len(col))
        v[diag] = d
        return v
    return np.stack([fill(case.jd_old[s]) for s in range(case.ns)]), fill(case.jd_now)


# ------------------------------------------------------------------------------------------------------------ slot rules
FIELDS = ("valid", "c_fact", "jac_stamp", "step_stamp", "last_use")


def ref_nearest(t, c, band, n_restarts, max_age, n_steps, step_age, n_slots):
    best, bd = -1, None
    for i in range(min(n_slots, len(t["valid"]))):
        if not t["valid"][i] or n_restarts - t["jac_stamp"][i] > max_age:
            continue
        if step_age >= 0 and n_steps - t["step_stamp"][i] > step_age:
            continue
        ratio = Fraction(float(c)) / Fraction(float(t["c_fact"][i]))
        if abs(np.float64(c) / np.float64(t["c_fact"][i]) - 1.0) > band:       # the band is a float64 statement (one division)
            continue
        r = abs(math.log(ratio))
        if bd is None or r < bd:
            best, bd = i, r
    return best


def ref_victim(t, n_restarts, max_age, n_slots):
    n = min(n_slots, len(t["valid"]))
    if n_slots == 0:
        return None
    for i in range(n):
        if not t["valid"][i] or n_restarts - t["jac_stamp"][i] > max_age:
            return i
    if n < n_slots:
        return n                                                               # beyond the table: unused slots
    return min(range(n), key=lambda i: (t["last_use"][i], i))


def table(valid, c_fact, jac_stamp=None, step_stamp=None, last_use=None):
    n = len(valid)
    z = lambda v: np.zeros(n, np.int64) if v is None else np.asarray(v, np.int64)
    return dict(valid=np.asarray(valid, np.int32), c_fact=np.asarray(c_fact, np.float64), jac_stamp=z(jac_stamp),
                step_stamp=z(step_stamp), last_use=z(last_use))


def query(c, band=0.35, n_restarts=0, max_age=50, n_steps=0, step_age=-1, n_slots=None):
    return dict(c=float(c), band=float(band), n_restarts=n_restarts, max_age=max_age, n_steps=n_steps, step_age=step_age, n_slots=n_slots)


def slot_rule_rows():
    """[(name, table, [queries], [(nearest, victim)])]; every query's n_slots filled in (default: the table's length)"""
    up = float(np.nextafter(1.25, 2.0))
    rows = [
        ("empty", table([], []), [query(1.0, n_slots=0)]),
        ("all invalid", table([0, 0, 0], [1.0, 1.0, 1.0], last_use=[5, 1, 3]), [query(1.0)]),
        ("single", table([1], [1.0], last_use=[4]), [query(1.0), query(1.3), query(1.36), query(0.7), query(0.5)]),
        ("exact tie", table([1, 1, 1, 1], [2.0, 1.0, 1.0, 3.0], last_use=[9, 8, 7, 6]), [query(1.1), query(0.9)]),
        ("band edge", table([1], [1.0]), [query(1.25, band=0.25), query(up, band=0.25), query(0.75, band=0.25),
                                           query(float(np.nextafter(0.75, 0.0)), band=0.25)]),
        ("restart age", table([1, 1], [1.0, 1.1], jac_stamp=[10, 9], last_use=[2, 1]),
         [query(1.04, n_restarts=60, max_age=50), query(1.0, n_restarts=60, max_age=50), query(1.0, n_restarts=61, max_age=50),
          query(1.08, n_restarts=59, max_age=50), query(1.0, n_restarts=10, max_age=0), query(1.0, n_restarts=11, max_age=0)]),
        ("step age", table([1, 1], [1.0, 1.1], step_stamp=[100, 90], last_use=[2, 1]),
         [query(1.04, n_steps=150, step_age=50), query(1.08, n_steps=140, step_age=50), query(1.08, n_steps=141, step_age=50),
          query(1.0, n_steps=151, step_age=50), query(1.08, n_steps=100000, step_age=-1), query(1.0, n_steps=100, step_age=0),
          query(1.0, n_steps=101, step_age=0)]),
        # c = 1: slot 0 (0.78) is nearer in log ratio (0.248) but 1 / 0.78 - 1 = 0.282 is outside the band; slot 1 (1.3) is
        # farther (0.262) and inside (0.231)
        ("nearest outside the band", table([1, 1], [0.78, 1.3]), [query(1.0, band=0.25), query(1.0, band=0.3)]),
        ("first free", table([1, 0, 1, 0, 1], [1.0, 2.0, 3.0, 4.0, 5.0], jac_stamp=[5, 0, 1, 0, 5], last_use=[1, 2, 3, 4, 5]),
         [query(9.0, n_restarts=5, max_age=50), query(9.0, n_restarts=5, max_age=3), query(9.0, n_restarts=5, max_age=3, n_slots=2),
          query(9.0, n_restarts=5, max_age=50, n_slots=1)]),
        ("first expired", table([1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0], jac_stamp=[5, 5, 1, 0], last_use=[1, 2, 3, 4]),
         [query(9.0, n_restarts=5, max_age=3), query(9.0, n_restarts=5, max_age=4), query(9.0, n_restarts=5, max_age=5)]),
        ("lru", table([1, 1, 1, 1], [1.0, 2.0, 3.0, 4.0], last_use=[7, 3, 9, 3]), [query(9.0), query(9.0, n_slots=1), query(9.0, n_slots=3)]),
        ("lru large clocks", table([1, 1, 1], [1.0, 2.0, 3.0], last_use=[2 ** 40 + 1, 2 ** 40, 2 ** 33]), [query(9.0), query(9.0, n_slots=2)]),
        # entries beyond n_slots: an exact match, a free slot and the oldest use - all to be ignored
        ("beyond n_slots", table([1, 1, 1, 0, 1], [1.2, 0.9, 1.0, 1.0, 1.0], last_use=[5, 4, 0, 0, -3]),
         [query(1.0, n_slots=2), query(1.0, n_slots=3), query(1.0, n_slots=5), query(1.0, n_slots=1)]),
    ]
    # the widest table of each implementation, every slot valid: lane 63 / slot 127 is looked at, ties between far-apart lanes
    for n in (RES_MAX_SLOTS, LU_MAX_SLOTS):
        cf = 1.0 + 0.004 * ((np.arange(n) * 37) % n)
        cf[n - 1] = cf[3] = 0.97
        lu = 1000 + ((np.arange(n) * 29) % n); lu[n - 1] = lu[17] = 5
        rows.append((f"full {n}", table(np.ones(n, np.int32), cf, last_use=lu),
                     [query(0.97), query(float(cf[n // 2])), query(1.001), query(3.0), query(0.968, n_slots=n - 1)]))
    out = []
    for name, t, qs in rows:
        exp = []
        for q in qs:
            if q["n_slots"] is None:
                q["n_slots"] = len(t["valid"])
            a = (q["c"], q["band"], q["n_restarts"], q["max_age"], q["n_steps"], q["step_age"], q["n_slots"])
            exp.append((ref_nearest(t, *a), ref_victim(t, q["n_restarts"], q["max_age"], q["n_slots"])))
            _assert_log_separation(name, t, q)
        out.append((name, t, qs, exp))
    return out


def _assert_log_separation(name, t, q):
    """host and device log may differ in the last bit: two admitted candidates either share c_fact or are 1e-12 apart"""
    adm = []
    for i in range(min(q["n_slots"], len(t["valid"]))):
        if ref_nearest({k: v[i:i + 1] for k, v in t.items()}, q["c"], q["band"], q["n_restarts"], q["max_age"], q["n_steps"], q["step_age"], 1) == 0:
            adm.append((abs(math.log(Fraction(q["c"]) / Fraction(float(t["c_fact"][i])))), float(t["c_fact"][i])))
    for i, (r1, c1) in enumerate(adm):
        for r2, c2 in adm[i + 1:]:
            assert c1 == c2 or abs(r1 - r2) > 1e-12 * max(r1, r2), (name, q)


# ------------------------------------------------------------------------------------------------------------ solve level
def star_net(L=40):
    """centre 0 <-> leaf i, i = 1 .. L: first order and reversible, so J depends on the rate constants alone; the centre has L
    neighbours (a hub: the dense block of the factorisation, which the lockstep ensemble needs)"""
    reacs, prods = [], []
    for i in range(1, L + 1):
        reacs += [[(0, 1)], [(i, 1)]]; prods += [[(i, 1)], [(0, 1)]]
    return from_lists(L + 1, reacs, prods)


GUARD_SCHEDULES = dict(same=(1.0, 1.0, 1.0, 1.0), up=(1.0, 1.0, 16.0, 16.0), down=(1.0, 1.0, 1.0 / 16, 1.0 / 16))
GUARD_TSTOPS = np.array([0.0, 1.0, 2.0, 3.0])
GUARD_T1, GUARD_SAVE = 4.0, 0.5


def guard_problem(L=40):
    """(net, k, u0): rate constants over 4.5 decades (the slow modes are still relaxing in every segment, so every restart climbs
    through the step sizes again; the fast ones make c max|J_ii| >> 1 at the end of a segment), start within a factor 1.5 of the
    equilibrium u_i / u_0 = kf_i / kr_i. The schedules scale EVERY rate constant by the same power of two from one stop on: the
    equilibrium stays, J is scaled exactly."""
    net = star_net(L)
    rng = np.random.default_rng(1)
    k = 10.0 ** rng.uniform(-1.5, 3.0, net.n_reactions)
    ueq = np.concatenate([[1.0], k[0::2] / k[1::2]])
    u0 = ueq / ueq.sum()
    u0[1:] *= rng.uniform(0.5, 1.5, L)
    return net, k, u0 / u0.sum()


def guard_table(k, name):
    return np.stack([k * f for f in GUARD_SCHEDULES[name]])
