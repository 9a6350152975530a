"""Path flux analysis written plainly in NumPy - the reference of the PFA tests - and the networks they share.

Definition (include/kinetica_hip.h, "path flux analysis"). Rates, records, pairing, nu_A and S are drg_cases.py's
(drg_cases.records gives the signed nu), E is DrgRef's pattern. For one state, with w = q_kf - q_kr (pairing) or q_r:
    P_A = sum of max(nu_A w, 0),  C_A = sum of max(-nu_A w, 0),  den_A = max(P_A, C_A)
    P_AB, C_AB = the parts of P_A, C_A whose records hold B (B in S, B != A)
    rp_AB = P_AB / den_A,  rc_AB = C_AB / den_A,  0.0 where den_A == 0
    r_AB = rp_AB + rc_AB + sum over M not in {A, B}, (A, M) and (M, B) in E, of (rp_AM rp_MB + rc_AM rc_MB)
on E2 = E and every two-hop pair (A, B), A != B; coef is the maximum of r over the states. Every sum here is math.fsum.

Bound of rp and rc (the terms are drgep_cases.py's), per (edge, state), eps = 2^-53: a term t = nu (q_f - q_r) carries
dt <= |nu| ((6 eps + ex_f) |q_f| + (6 eps + ex_r) |q_r|), and so do max(t, 0) and max(-t, 0), max being 1-Lipschitz. P_A and
C_A are sums of n non-negative numbers: dden <= sum dt + n eps (P_A + C_A), as there. P_AB is a sum of the n_e non-negative
numbers max(t, 0) of the edge's records: dP_AB <= sum dt + n_e eps P_AB, and C_AB likewise. The quotient, which is at most 1
(P_AB <= P_A <= den_A), is rounded once: |rp_got - rp_ref| <= (dP_AB + rp dden) / den + 2 eps, and the same for rc. Where
den_ref is 0 and every rate behind it is exactly 0 the bound is 0; where it is pure cancellation the bound is vacuous (inf).

Bound of the second stage GIVEN rp and rc: every term is non-negative. A product costs one rounding, a sum of n non-negative
terms in any order at most n - 1, the three closing additions three: with at most deg_A products in each of the two sums
that is deg_A + 3 roundings of relative size eps on any path from a term to the result, so
    |got - ref| <= (deg_A + 4) 2^-52 ref        (deg_A: the out-degree of A in E)
- twice the rounding count, the factor two covering the second-order terms. The reference rounds every product once as
well and sums exactly."""
import math

import numpy as np

import drg_cases as dc
import drgep_cases as ec
from kinetica_jl_amd.synth import from_lists

EPS = dc.EPS


class PfaRef:
    """E2 of one (network, pairing), the split coefficients of given per-state rates with their bounds, and the second stage.
    second=False leaves E2 and the second stage out (the split stage alone, where E2 would be millions of pairs)."""

    def __init__(self, net, pairing, second=True):
        self.s = s = ec.DrgepRef(net, pairing)          # the signed contribution lists on DrgRef's pattern
        self.g = g = s.g
        self.n, self.E, self.rows, self.cols, self.rowptr = g.n, g.E, g.rows, g.cols, g.rowptr
        n, deg = self.n, np.diff(g.rowptr)
        self.deg = deg
        if not second:
            return
        # every product: the edges e1 = (A, M) and e2 = (M, B), B != A
        cnt = deg[self.cols] if self.E else np.zeros(0, np.int64)
        e1 = np.repeat(np.arange(self.E, dtype=np.int64), cnt)
        start = np.repeat(g.rowptr[self.cols] if self.E else np.zeros(0, np.int64), cnt)
        within = np.arange(len(e1), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        e2 = start + within
        self.products = len(e1)                          # (A -> M -> A included: the count of the device's multiply-adds)
        ok = self.cols[e2] != self.rows[e1] if len(e1) else np.zeros(0, bool)
        e1, e2 = e1[ok], e2[ok]
        key1 = self.rows * n + self.cols
        key2 = self.rows[e1] * n + self.cols[e2]
        keys = np.unique(np.concatenate([key1, key2]))
        self.rows2, self.cols2 = keys // n, keys % n
        self.E2 = len(keys)
        self.rowptr2 = np.searchsorted(self.rows2, np.arange(n + 1)).astype(np.int64)
        self.colidx2 = self.cols2.astype(np.int64)
        self.z1 = np.searchsorted(keys, key1)           # where the first-generation edges sit in E2
        z2 = np.searchsorted(keys, key2)
        order = np.argsort(z2, kind="stable")           # (M in pattern order within a pair)
        self.e1, self.e2, self.z2 = e1[order], e2[order], z2[order]

    def info(self):
        """The sizes kin_pfa_pattern_host reports."""
        return dict(edges=self.E, pairs=self.E2, products=self.products, max_row=int(self.deg.max()) if self.n else 0)

    def split(self, q, ex=None):
        """(rp[E], rc[E], bound_p[E], bound_c[E]) of one state's rates q[R]; ex[R]: extra relative error of every rate."""
        s = self.s
        ex = np.zeros(len(q)) if ex is None else ex
        rowsum = dc.DrgRef._rowsum
        td, ed = s._terms(s.den, 1, q, ex)
        tn, en = s._terms(s.num, 2, q, ex)
        P, C = rowsum(np.maximum(td, 0.0), s.den_ptr), rowsum(np.maximum(-td, 0.0), s.den_ptr)
        den = np.maximum(P, C)
        dden = rowsum(ed, s.den_ptr) + np.diff(s.den_ptr) * EPS * (P + C)
        Pe, Ce = rowsum(np.maximum(tn, 0.0), s.edge_ptr), rowsum(np.maximum(-tn, 0.0), s.edge_ptr)
        de = rowsum(en, s.edge_ptr)
        ne = np.diff(s.edge_ptr)
        dA, ddA = den[self.rows], dden[self.rows]
        pos = dA > 0
        safe = np.where(pos, dA, 1.0)
        out = []
        for num in (Pe, Ce):
            r = np.where(pos, num / safe, 0.0)
            bound = np.where(pos, (de + ne * EPS * num + r * ddA) / safe + 2 * EPS, np.where(ddA > 0, np.inf, 0.0))
            out.append((r, bound))
        return out[0][0], out[1][0], out[0][1], out[1][1]

    def split_all(self, rates, ex=None):
        """(rp[B][E], rc[B][E], bound_p[B][E], bound_c[B][E]) of rates[B][R]."""
        rates = np.atleast_2d(rates)
        cols = zip(*[self.split(rates[b], None if ex is None else ex[b]) for b in range(len(rates))])
        return tuple(np.stack(c) for c in cols)

    def second(self, rp, rc):
        """r[E2] of one state's rp[E], rc[E]: every product rounded once, every sum exact."""
        z = np.concatenate([self.z1, self.z1, self.z2, self.z2])
        v = np.concatenate([rp, rc, rp[self.e1] * rp[self.e2], rc[self.e1] * rc[self.e2]])
        keep = v != 0.0
        z, v = z[keep], v[keep]
        order = np.argsort(z, kind="stable")
        z, v = z[order], v[order]
        ptr = np.searchsorted(z, np.arange(self.E2 + 1))
        cnt = np.diff(ptr)
        r = np.zeros(self.E2)
        one, two = cnt == 1, cnt == 2
        r[one] = v[ptr[:-1][one]]
        r[two] = v[ptr[:-1][two]] + v[ptr[:-1][two] + 1]          # (a single addition is correctly rounded, as fsum is)
        vl = v.tolist()
        for i in np.flatnonzero(cnt > 2):
            r[i] = math.fsum(vl[ptr[i]:ptr[i + 1]])
        return r

    def second_all(self, rp, rc):
        return np.stack([self.second(rp[b], rc[b]) for b in range(len(rp))]) if len(rp) else np.zeros((0, self.E2))

    def second_bound(self, ref):
        """The relative bound of the second stage on ref[...][E2]."""
        return (self.deg[self.rows2] + 4) * 2.0 ** -52 * ref

    def coefficients(self, rates):
        """(coef[E2], r[B][E2]) of rates[B][R]."""
        rp, rc, _, _ = self.split_all(rates)
        r = self.second_all(rp, rc)
        return (r.max(axis=0) if len(r) else np.zeros(self.E2)), r


# ---- networks ------------------------------------------------------------------------------------------------------------
def hand_networks():
    """name -> (net, k[R], U[B][N], {pairing: {(A, B): r}}): every pair of E2 with its hand value in the first state (dyadic
    numbers: exact in binary). The last state of every U is all zeros, where r is exactly 0.0."""
    out = {}
    z = lambda U: np.vstack([np.array(U, float), np.zeros((1, len(U[0])))])
    both = lambda v: {0: v, 1: v}
    A, M, B = 0, 1, 2
    # chain A -> M -> B, q = (2, 1). A: C = 2, rc_AM = 1. M: P = 2, C = 1, den = 2: rp_MA = 1, rc_MB = 0.5. B: P = 1, rp_BM = 1.
    # (A, B) is no DRG edge: r_AB = rc_AM rc_MB = 0.5 (consumption alone), r_BA = rp_BM rp_MA = 1 (production alone)
    out["chain"] = (from_lists(3, [[(A, 1)], [(M, 1)]], [[(M, 1)], [(B, 1)]]), np.array([4.0, 4.0]), z([[0.5, 0.25, 0.0]]),
                    both({(A, M): 1.0, (A, B): 0.5, (M, A): 1.0, (M, B): 0.5, (B, A): 1.0, (B, M): 1.0}))
    # fork M -> A, M -> B, q = (2, 2). M: C = 4, rc_MA = rc_MB = 0.5. A: rp_AM = 1, B: rp_BM = 1. (A, B): rp_AM meets rc_MB only
    out["fork"] = (from_lists(3, [[(M, 1)], [(M, 1)]], [[(A, 1)], [(B, 1)]]), np.array([4.0, 4.0]), z([[0.0, 0.5, 0.0]]),
                   both({(A, M): 1.0, (A, B): 0.0, (M, A): 0.5, (M, B): 0.5, (B, A): 0.0, (B, M): 1.0}))
    # reversible A -> M (q = 2), M -> A (q = 1). Unpaired: A has C = 2, P = 1: rc_AM = 1, rp_AM = 0.5; M has P = 2, C = 1.
    # Paired: w = 1, C_A = P_M = 1. A -> M -> A is no pair: E2 has no diagonal
    out["reversible"] = (from_lists(2, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(0, 1)]]), np.array([4.0, 4.0]), z([[0.5, 0.25]]),
                         {0: {(0, 1): 1.5, (1, 0): 1.5}, 1: {(0, 1): 1.0, (1, 0): 1.0}})
    # balanced A <=> M -> B, q = (3, 3, 1). Paired: w = 0 for the pair, den_A = 0: row A is 0.0; M: C = 1: rc_MB = 1, nothing
    # towards A; B: rp_BM = 1, r_BA = rp_BM rp_MA = 0. Unpaired: A: P = C = 3: rp_AM = rc_AM = 1; M: P = 3, C = 4, den = 4:
    # rp_MA = rc_MA = 0.75, rc_MB = 0.25; r_AB = rc_AM rc_MB = 0.25, r_BA = rp_BM rp_MA = 0.75
    out["balanced"] = (from_lists(3, [[(A, 1)], [(M, 1)], [(M, 1)]], [[(M, 1)], [(A, 1)], [(B, 1)]]), np.array([6.0, 12.0, 4.0]),
                       z([[0.5, 0.25, 0.0]]),
                       {1: {(A, M): 0.0, (A, B): 0.0, (M, A): 0.0, (M, B): 1.0, (B, A): 0.0, (B, M): 1.0},
                        0: {(A, M): 2.0, (A, B): 0.25, (M, A): 1.5, (M, B): 0.25, (B, A): 0.75, (B, M): 1.0}})
    # collider A + X -> B + X (species A, B, X = 0, 1, 2), q = 2 * 0.5 * 4 = 4. A: C = 4: rc_AB = rc_AX = 1; B: P = 4: rp_BA = rp_BX = 1;
    # X has no row. Second generation: A -> B -> X adds rp_AB rp_BX + rc_AB rc_BX = 0 * 1 + 1 * 0, and B -> A -> X likewise
    out["collider"] = (from_lists(3, [[(0, 1), (2, 1)]], [[(1, 1), (2, 1)]]), np.array([2.0]), z([[0.5, 0.25, 4.0]]),
                       both({(0, 1): 1.0, (0, 2): 1.0, (1, 0): 1.0, (1, 2): 1.0}))
    return out


def side_branch_network():
    """The chain A -> M -> B with an inert side branch M -> C -> D (species A, M, B, C, D = 0 .. 4; reactions in that order)."""
    return from_lists(5, [[(0, 1)], [(1, 1)], [(1, 1)], [(3, 1)]], [[(1, 1)], [(2, 1)], [(3, 1)], [(4, 1)]])


# ---- the synthetic cases of drg_cases.py -----------------------------------------------------------------------------------
B_GPU = 7
GPU_CASES = [("300x1500", m) for m in dc.MODES] + [("300x1500_cut", "per_state"), ("1000x5000", "per_state"), ("1000x5000", "T")]
_graphs, _refs = {}, {}


def graph(name, pairing):
    if (name, pairing) not in _graphs:
        _graphs[(name, pairing)] = PfaRef(dc.synth_case(name).net, pairing)
    return _graphs[(name, pairing)]


def ref(name, mode, pairing, B=B_GPU):
    """(rp[B][E], rc[B][E], bound_p[B][E], bound_c[B][E]) of a synthetic case, computed once."""
    key = (name, mode, pairing, B)
    if key not in _refs:
        _refs[key] = graph(name, pairing).split_all(ec.rates(name, mode, B), dc.synth_case(name).ex(mode, B))
    return _refs[key]
