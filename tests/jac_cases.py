"""Shared by tests/test_jac_cases.py (no GPU) and tests/test_gpu_jacobian.py: an extended-precision reference of the mass-action
right-hand side, its Jacobian and the Newton residual of a BDF step, written from the network's reaction lists
(net.reaction(r)), never from the kernels or the compiled tables; the error bounds every value is judged with, entry by entry;
the case lists and the states. A plain module: no fixtures, no test collection.

Reference. Reaction r with operands a (and b) and net stoichiometry nu_ir contributes
    nu_ir rate_r                to the right-hand side of species i       (rate_r = k_r u_a [u_b]),
    nu_ir d rate_r / d u_j      to the Jacobian entry (i, j), j an operand of r,
with the derivative conventions of mass_action_drates (step_dev.hpp): 2A has ONE operand column with 2 k u; a species on both
sides multiplies the rate, and its net-zero row gets no term. From these term lists: per entry / species the value, the scale
S = sum of the absolute terms and the term count L; the pattern (sorted columns, diagonal always present) comes from the same
lists. Everything in np.longdouble (64-bit mantissa).

Bounds (u = 2^-53; derived, nothing here is fitted to what a device returned). A term is a product chain on exact inputs: p
roundings make it (1 + delta)^p of the exact term, |delta| <= u. A sum of L computed terms in ANY order (sequential, pairwise,
lanes then a butterfly, passes of a long row) carries at most L - 1 further roundings on every term's path: the computed value
is within gamma(L - 1 + p) S of the exact one, gamma(n) = n u / (1 - n u) <= n u (1 + 3e-12) for the n <= 24 600 used here. The
reference's own error is at most (520 + p) 2^-64 S < 0.3 u S (terms: p roundings of 2^-64; rows of more than 512 terms are
summed pairwise - blocks of 128 and a tree -, shorter ones in sequence). So |device - reference| <= (L - 1 + p + 1) u S; the
Jacobian and the RHS leave one more unit as slack:
    Jacobian entry   p <= 2 (2 k u is exact, k u one rounding, the coefficient times it one more)    (L + 3) u S_ij
    RHS component    p  = 3 (k u_a, times u_b, times the coefficient)                                (L + 4) u S_i
    residual         c f_i - psi_i - d_i: the sum above (L + 2 roundings), one product and two subtractions, each a
                     rounding of a value bounded by the scale |c| S_i + |psi_i| + |d_i|: L + 5, and the unit
                     for the second-order terms and the reference                                     (L + 6) u scale
A fused multiply-add only removes a rounding; a coefficient of +-1 or +-2 and an absent second operand remove theirs.
Where S = 0 (an empty row, a row whose terms all vanish) the bound is 0: the value must be WRITTEN as 0.0.

Exact inputs. With u in {1/2, 1, 2} and integer k in 1 .. 8 every term is a multiple of 1/4 below 2^8 and every partial sum of
every order is far below 2^53 (the largest entry of hub_net(24577) sums |terms| to less than 2^20): any correct evaluation
returns the reference bit for bit, and a missing, doubled or misplaced term changes the result whatever its size. The same holds
for the residual with c, psi, d multiples of 1/4 of modest size."""
import numpy as np

from kinetica_jl_amd.synth import from_lists, synthetic_crn
from tests.linalg_cases import hub_net, with_special_stoichiometries

LD = np.longdouble
U = LD(2.0) ** -53
P_JAC, P_RHS = 2, 3                         # roundings of a term before the sum
C_JAC, C_RHS, C_RESID = P_JAC - 1 + 2, P_RHS - 1 + 2, P_RHS - 1 + 3 + 1    # (L + 3), (L + 4), (L + 6): module docstring
assert (C_JAC, C_RHS, C_RESID) == (3, 4, 6)
PAIRWISE_FROM = 512                         # reference rows longer than this are summed pairwise
SENTINEL = -3.5e200                         # fills what an operation must not touch

# seg plan classes (network.hpp: SegPlanHost)
SHORT_MAX, SEG_LEN, BLK_PASS = 8, 256, 12288


# ------------------------------------------------------------------------------------------------------------ reference
class Reference:
    """term lists and pattern of a network, from its reaction lists alone"""

    def __init__(self, net):
        self.net = net
        N, R = net.n_species, net.n_reactions
        self.N, self.R = N, R
        a = np.zeros(R, np.int64); b = np.full(R, -1, np.int64)
        t_sp, t_rx, t_nu = [], [], []
        j_row, j_col, j_rx, j_w, j_nu = [], [], [], [], []
        for r in range(R):
            reac, prod = net.reaction(r)
            ops = [int(s) for s, c in reac for _ in range(int(c))]
            assert 1 <= len(ops) <= 2
            nu = {}
            for s, c in reac:
                nu[int(s)] = nu.get(int(s), 0) - int(c)
            for s, c in prod:
                nu[int(s)] = nu.get(int(s), 0) + int(c)
            a[r] = ops[0]
            if len(ops) == 2:
                b[r] = ops[1]
            cols = (0, 1) if len(ops) == 2 and ops[0] != ops[1] else (0,)
            for s, v in nu.items():
                if v == 0:
                    continue
                t_sp.append(s); t_rx.append(r); t_nu.append(v)
                for w in cols:
                    j_row.append(s); j_col.append(ops[w]); j_rx.append(r); j_w.append(w); j_nu.append(v)
        ai = lambda v: np.array(v, dtype=np.int64)
        self.a, self.b = a, b
        self.t_sp, self.t_rx, self.t_nu = ai(t_sp), ai(t_rx), ai(t_nu)
        self.j_row, self.j_col, self.j_rx, self.j_w, self.j_nu = ai(j_row), ai(j_col), ai(j_rx), ai(j_w), ai(j_nu)
        # pattern: the term positions and the diagonal, sorted by (row, column)
        keys = np.unique(np.concatenate([self.j_row * N + self.j_col, np.arange(N, dtype=np.int64) * (N + 1)]))
        self.nnz = len(keys)
        self.rows, self.cols = keys // N, keys % N
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(self.rows, minlength=N))]).astype(np.int64)
        self.j_ent = np.searchsorted(keys, self.j_row * N + self.j_col)
        self.diag = np.searchsorted(keys, np.arange(N, dtype=np.int64) * (N + 1))
        self.L_rhs = np.bincount(self.t_sp, minlength=N)
        self.L_jac = np.bincount(self.j_ent, minlength=self.nnz)

    # per-reaction rate and operand derivatives in the given type, rounded operation by operation in the kernels' order
    def rates(self, k, u, dtype=LD):
        k = np.asarray(k).astype(dtype); u = np.asarray(u).astype(dtype)
        two = self.b >= 0
        ub = np.where(two, u[np.where(two, self.b, 0)], dtype(1))
        return k * u[self.a] * ub

    def drates(self, k, u, dtype=LD):
        k = np.asarray(k).astype(dtype); u = np.asarray(u).astype(dtype)
        two = self.b >= 0; same = self.b == self.a
        ub = u[np.where(two, self.b, 0)]
        d0 = np.where(two, np.where(same, dtype(2) * k * u[self.a], k * ub), k)
        d1 = np.where(two & ~same, k * u[self.a], dtype(0))
        return np.stack([d0, d1], axis=1)

    def rhs_terms(self, k, u, dtype=LD, r_lo=0, r_hi=None):
        """(species, nu_ir rate_r) of the reactions [r_lo, r_hi)"""
        v = self.t_nu.astype(dtype) * self.rates(k, u, dtype)[self.t_rx]
        if r_lo == 0 and r_hi is None:
            return self.t_sp, v
        m = (self.t_rx >= r_lo) & (self.t_rx < (self.R if r_hi is None else r_hi))
        return self.t_sp[m], v[m]

    def jac_terms(self, k, u, dtype=LD):
        """(entry, nu_ir d rate_r / d u_j); entry e is (rows[e], cols[e])"""
        return self.j_ent, self.j_nu.astype(dtype) * self.drates(k, u, dtype)[self.j_rx, self.j_w]

    def rhs(self, k, u, r_lo=0, r_hi=None):
        """(value, S, L) per species"""
        return accumulate(*self.rhs_terms(k, u, LD, r_lo, r_hi), self.N)

    def jac(self, k, u):
        """(value, S, L) per stored entry"""
        return accumulate(*self.jac_terms(k, u), self.nnz)

    def resid(self, k, u, c, psi, d):
        """(value, scale, L) of c f(u) - psi - d per species"""
        f, S, L = self.rhs(k, u)
        psi = np.asarray(psi).astype(LD); d = np.asarray(d).astype(LD)
        return LD(c) * f - psi - d, abs(LD(c)) * S + np.abs(psi) + np.abs(d), L


def accumulate(idx, vals, n):
    """per index: (sum of the terms, sum of their magnitudes, their number); longdouble, long rows pairwise"""
    order = np.argsort(idx, kind="stable")
    idx, vals = idx[order], vals[order].astype(LD)
    L = np.bincount(idx, minlength=n)
    val = np.zeros(n, LD); S = np.zeros(n, LD)
    np.add.at(val, idx, vals)
    np.add.at(S, idx, np.abs(vals))
    beg = np.concatenate([[0], np.cumsum(L)])
    for i in np.nonzero(L > PAIRWISE_FROM)[0]:
        seg = np.ascontiguousarray(vals[beg[i]:beg[i + 1]])
        val[i] = seg.sum(); S[i] = np.abs(seg).sum()
    return val, S, L


def sum64(idx, vals, n, reverse=False):
    """float64 sequential sums of the terms per index, in list order or reversed (np.add.at adds one element at a time)"""
    out = np.zeros(n)
    v = np.asarray(vals, dtype=np.float64)
    if reverse:
        idx, v = idx[::-1], v[::-1]
    np.add.at(out, idx, v)
    return out


def bound_jac(S, L):
    return (L + C_JAC) * U * S


def bound_rhs(S, L):
    return (L + C_RHS) * U * S


def bound_resid(scale, L):
    return (L + C_RESID) * U * scale


def compare(dev, ref, bound):
    """(all inside, largest error / bound over the entries with a bound > 0). Where the bound is 0 the value must equal the
    reference exactly; a NaN is outside every bound."""
    dev = np.asarray(dev)
    err = np.abs(dev.astype(LD) - ref)
    ok = bool(np.all(err <= bound))
    pos = bound > 0
    ratio = float(np.max(err[pos] / bound[pos])) if np.any(pos) and not np.any(np.isnan(err[pos])) else (0.0 if not np.any(pos) else np.inf)
    return ok, ratio


def worst(dev, ref, bound):
    """the entry furthest outside, for an assertion message"""
    err = np.abs(np.asarray(dev).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    i = int(np.argmax(q))
    return dict(entry=i, dev=float(np.asarray(dev)[i]), ref=float(ref[i]), bound=float(bound[i]), ratio=float(q[i]))


def assert_jac_entrywise(net, k, u, vals, rowptr=None, col=None, what=None):
    """every stored Jacobian value inside its own bound (L + 3) u S_ij (and the pattern the reference's, when given); returns the
    largest error / bound. For tests that compare a Jacobian normwise: the entrywise bound next to it."""
    ref = Reference(net)
    if rowptr is not None:
        assert np.array_equal(rowptr, ref.rowptr) and np.array_equal(col, ref.cols), (what, "pattern")
    J, S, L = ref.jac(k, u)
    ok, ratio = compare(vals, J, bound_jac(S, L))
    assert ok, (what, worst(vals, J, bound_jac(S, L)))
    return ratio


def plan_class(L):
    """(G, S, B, max_row, short rows) of the gather plan over rows of these lengths (build_seg_plan: rows up to 8 entries
    64 to an ELL group, 9 .. 256 one wavefront each, longer ones one workgroup each; empty rows are scheduled)"""
    L = np.asarray(L)
    short = int(np.sum(L <= SHORT_MAX))
    return dict(G=(short + 63) // 64, S=int(np.sum((L > SHORT_MAX) & (L <= SEG_LEN))), B=int(np.sum(L > SEG_LEN)),
                max_row=int(L.max()) if len(L) else 0, short=short)


# ------------------------------------------------------------------------------------------------------------- networks
def short_rows_net(n_chain, n_iso, long_pair=False):
    """a chain 0 -> 1 -> ... of n_chain species, n_iso species in no reaction at all, and (long_pair) two more species P, Q with
    257 copies of P -> Q. Rows of the RHS plan: n_chain + n_iso short ones (1 or 2 entries; the isolated ones empty) and with
    long_pair two whole-workgroup rows of 257; rows of the Jacobian plan: 2 n_chain - 1 + n_iso short ones (the diagonal of the
    chain's last species and of every isolated species empty) and with long_pair one more empty one, (Q, Q), and the two
    whole-workgroup rows (P, P) and (Q, P)."""
    reacs = [[(i, 1)] for i in range(n_chain - 1)]
    prods = [[(i + 1, 1)] for i in range(n_chain - 1)]
    n = n_chain + n_iso
    if long_pair:
        reacs += [[(n, 1)]] * 257; prods += [[(n + 1, 1)]] * 257
        n += 2
    return from_lists(n, reacs, prods)


def rhs_rows_case(t, long_pair):
    """t short rows in the RHS / residual plan"""
    return short_rows_net(t - 1, 1, long_pair)


def jac_rows_case(t, long_pair):
    """t short rows in the Jacobian plan"""
    lp = 1 if long_pair else 0
    iso = 1 if (t - lp) % 2 == 0 else 2                      # 2 n - 1 + iso + lp = t, at least one isolated species
    n = (t + 1 - iso - lp) // 2
    assert 2 * n - 1 + iso + lp == t
    return short_rows_net(n, iso, long_pair)


def empty_rows_net():
    """species 3 is in no reaction; species 2 only ever an inert collider (A + C -> B + C, B + C -> A + C); species 4 is
    produced only: their rows of the RHS (2, 3) and their diagonal Jacobian entries (2, 3, 4) have no term"""
    return from_lists(5, [[(0, 1), (2, 1)], [(1, 1), (2, 1)], [(0, 2)]], [[(1, 1), (2, 1)], [(0, 1), (2, 1)], [(4, 1)]])


def triple_product_net():
    """A -> 3B (a coefficient that is no power of two), 2B -> A, A + B -> C, C -> A + B"""
    return from_lists(3, [[(0, 1)], [(1, 2)], [(0, 1), (1, 1)], [(2, 1)]], [[(1, 3)], [(0, 1)], [(2, 1)], [(0, 1), (1, 1)]])


HUB_LENGTHS = (1, 8, 9, 64, 65, 256, 257, 12288, 12289, 24577)
ROW_COUNTS = (63, 64, 65, 255, 256, 257)


def _hub_class(L):
    return "ell" if L <= SHORT_MAX else "wave" if L <= SEG_LEN else f"block{(L + BLK_PASS - 1) // BLK_PASS}"


def build_cases():
    """name -> (builder of the network, the class it is meant to reach: a dict of expectations on the plans' info:
    plan ('rhs' | 'jac' | 'both'), then any of G, S, B, max_row, short, wg)"""
    cases = {}
    for L in HUB_LENGTHS:
        cls = _hub_class(L)
        exp = dict(plan="both", max_row=L)
        if cls == "ell":
            exp.update(S=0, B=0, wg=256)
        elif cls == "wave":
            exp.update(S=2, B=0, wg=256)
        else:
            exp.update(S=0, B=2, wg=1024)
        cases[f"hub_{L}_{cls}"] = (lambda L=L: hub_net(L), exp)
    for t in ROW_COUNTS:
        for lp in (False, True):
            tag = "long" if lp else "short"
            cases[f"rhs_rows_{t}_{tag}"] = (lambda t=t, lp=lp: rhs_rows_case(t, lp),
                                            dict(plan="rhs", short=t, G=(t + 63) // 64, S=0, B=2 if lp else 0, wg=1024 if lp else 256))
            cases[f"jac_rows_{t}_{tag}"] = (lambda t=t, lp=lp: jac_rows_case(t, lp),
                                            dict(plan="jac", short=t, G=(t + 63) // 64, S=0, B=2 if lp else 0, wg=1024 if lp else 256))
    cases["empty_rows"] = (empty_rows_net, dict(plan="both", S=0, B=0, G=1))
    cases["triple_product"] = (triple_product_net, dict(plan="both", G=1))
    cases["special_stoichiometries_60"] = (lambda: with_special_stoichiometries(synthetic_crn(60, 300, seed=11)[0]), dict(plan="both", B=0))
    cases["synthetic_300"] = (lambda: synthetic_crn(300, 1500)[0], dict(plan="both"))
    cases["synthetic_1000"] = (lambda: synthetic_crn(1000, 5000)[0], dict(plan="both"))
    return cases


CASES = build_cases()
_CACHE = {}


def case(name):
    """(network, Reference) of a case, built once"""
    if name not in _CACHE:
        net = CASES[name][0]()
        _CACHE[name] = (net, Reference(net))
    return _CACHE[name]


def expected(name):
    return CASES[name][1]


def check_class(name, which, info):
    """assert from a plan's info (G, S, B, max_row, short, wg) that the case reached the class it is named after, and that the
    plan is the one the reference's row lengths predict"""
    net, ref = case(name)
    pred = plan_class(ref.L_rhs if which == "rhs" else ref.L_jac)
    pred["wg"] = 1024 if pred["B"] > 0 else 256
    got = {q: int(info[q]) for q in pred}
    assert got == pred, (name, which, got, pred)
    exp = expected(name)
    if exp["plan"] in (which, "both"):
        for q, v in exp.items():
            if q != "plan":
                assert got[q] == v, (name, which, q, got, exp)


# --------------------------------------------------------------------------------------------------------------- states
STATE_KINDS = ("loguniform", "one_hot", "zeros", "exact", "zero_operand")
EXACT_U = (0.5, 1.0, 2.0)


def _seed(name, kind, member=0):
    return [sum(name.encode()) * 1000 + len(name), STATE_KINDS.index(kind), member]


def state(name, kind, member=0):
    """(u, k) of a case: log-uniform 1e-12 .. 1 with k log-uniform over 12 decades; one-hot on the first operand of reaction 0;
    all zeros; the exact set (u in {1/2, 1, 2}, integer k in 1 .. 8); log-uniform with a zero at an operand of an A + B reaction
    and at the operand of a 2A reaction (where the network has them)"""
    net, ref = case(name)
    rng = np.random.default_rng(_seed(name, kind, member))
    N, R = ref.N, ref.R
    k = 10.0 ** rng.uniform(-3, 9, R)
    if kind == "exact":
        return rng.choice(EXACT_U, N), rng.integers(1, 9, R).astype(np.float64)
    if kind == "zeros":
        return np.zeros(N), k
    if kind == "one_hot":
        u = np.zeros(N); u[ref.a[0] if R else 0] = 1.0
        return u, k
    u = 10.0 ** rng.uniform(-12, 0, N)
    if kind == "zero_operand":
        ab = np.nonzero((ref.b >= 0) & (ref.b != ref.a))[0]
        aa = np.nonzero(ref.b == ref.a)[0]
        if len(ab):
            u[ref.b[ab[len(ab) // 2]]] = 0.0
        if len(aa):
            u[ref.a[aa[0]]] = 0.0
    return u, k


def resid_inputs(name, kind, member=0):
    """(c, psi, d) of a residual: on the exact inputs multiples of 1/4 (c = 1/2), else psi and d of mixed signs over 12 decades
    and c = 1e-3"""
    net, ref = case(name)
    rng = np.random.default_rng(_seed(name, kind, member) + [7])
    if kind == "exact":
        return 0.5, rng.integers(-16, 17, ref.N) / 4.0, rng.integers(-16, 17, ref.N) / 4.0
    sg = lambda: rng.choice([-1.0, 1.0], ref.N) * 10.0 ** rng.uniform(-12, 0, ref.N)
    return 1e-3, sg(), sg()
