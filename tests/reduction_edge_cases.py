"""Shared by tests/test_reduction_edge_cases.py (no GPU), tests/test_gpu_reduction_edges.py and
tests/test_gpu_reduction_trips.py: networks that put a chosen row of the reduction passes' gather plans, of the PFA second
stage and of the DRGEP path stage at every class limit, with inputs on which every sum is exact. A plain module: no fixtures,
no test collection. The references are those of drg_cases, drgep_cases, pfa_cases and reaction_importance_cases.

Gather families. A hub h of length n has the species A_h, B_h, C_h, D_h; the colliders X_i (and the partners Y_i of the
paired family) are shared by the hubs of a network.
    collider hub   A + X_i -> B + X_i, i < n                        records that never pair (b = -1)
    paired hub     A + X_i -> B + Y_i and B + Y_i -> A + X_i, i < n  n pair records with pairing (b >= 0), 2 n without
Both get SIDE = 2 records of A that do not hold B, A -> C and D -> A. The denominator row of B and the edge rows (A, B),
(B, A) then carry n contributions (2 n for the paired hub without pairing), the denominator row of A two more: at n = 8, 256
and 1024 the edge row and the denominator row of A fall into different classes, num_AB != den_A, and A is produced (by D) as
well as consumed, so that P_A and C_A are both non-zero and |s_AB| < den_A.

Exact inputs: u in {1/2, 1, 2}, integer k in 1 .. 8. A rate is a multiple of 1/4 up to 32, so every sum of at most
2 (2049 + 2) of them, signed or not, is exact in any order; the references (math.fsum, then one float64 division) are then
what a correct device returns bit for bit. State ZERO_STATE of every batch is all zeros.

PFA families (all reactions unimolecular, directions alternating; no reaction has a reverse, so both pairings see one pattern).
    double star DS(d, m)   A with d - 1 leaves and M, M with m - 1 leaves and A: row A has out-degree d, one neighbour of degree
                           m and d + m - 1 columns in E2; every leaf of A has the single neighbour A of degree d
    broom BR(d, l)         A with d neighbours of l private leaves each: row A has out-degree d and d (l + 1) columns in E2
A network is a disjoint union of them. The path family is the double stars again: the in-degree of A is d."""
import math

import numpy as np

import drg_cases as dc
import drgep_cases as ec
import pfa_cases as pc
import reaction_importance_cases as rc
from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists

EPS = dc.EPS
RGAS = dc.RGAS
LENGTHS = (1, 8, 9, 64, 65, 256, 257, 1024, 1025, 2049)
SIDE = 2
EXACT_U = (0.5, 1.0, 2.0)
B_EXACT = 7
ZERO_STATE = 4
# class limits of the gather plans (drg.hpp: SegPlanHost::SHORT_MAX, SEG_LEN) and the entries of a long row per pass
# (drg_kernels.hip: DRG_WG * DRG_LONG_NX)
SHORT_MAX, SEG_LEN, LONG_PASS = capi.DRG_SHORT_MAX, capi.DRG_SEG_LEN, capi.DRG_LONG_PASS


def row_class(n):
    return "short" if n <= SHORT_MAX else "medium" if n <= SEG_LEN else "long"


def passes(n):
    return -(-n // LONG_PASS)


# ---- gather families -------------------------------------------------------------------------------------------------------
def hub_network(family, lengths):
    """(net, hubs): hubs[h] = dict(n, A, B, C, D) of the family "collider" or "paired"."""
    H, nmax = len(lengths), max(lengths)
    X = lambda i: 4 * H + i
    Y = lambda i: 4 * H + nmax + i
    reacs, prods, hubs = [], [], []
    for h, n in enumerate(lengths):
        A, B, C, D = 4 * h, 4 * h + 1, 4 * h + 2, 4 * h + 3
        hubs.append(dict(n=n, A=A, B=B, C=C, D=D))
        for i in range(n):
            if family == "collider":
                reacs.append([(A, 1), (X(i), 1)]); prods.append([(B, 1), (X(i), 1)])
            else:
                reacs.append([(A, 1), (X(i), 1)]); prods.append([(B, 1), (Y(i), 1)])
                reacs.append([(B, 1), (Y(i), 1)]); prods.append([(A, 1), (X(i), 1)])
        reacs.append([(A, 1)]); prods.append([(C, 1)])
        reacs.append([(D, 1)]); prods.append([(A, 1)])
    return from_lists(4 * H + nmax * (1 if family == "collider" else 2), reacs, prods), hubs


def exact_states(n_species, n_reactions, B, seed):
    """(U[B][N], K[B][R]) of the exact set, all different, state ZERO_STATE all zeros"""
    rng = np.random.default_rng(seed)
    U = rng.choice(EXACT_U, (B, n_species))
    K = rng.integers(1, 9, (B, n_reactions)).astype(np.float64)
    if B > ZERO_STATE:
        U[ZERO_STATE] = 0.0
    return U, K


def edge_of(g, A, B):
    """index of the edge (A, B) in DrgRef's pattern"""
    e = g.rowptr[A] + int(np.searchsorted(g.colidx[g.rowptr[A]:g.rowptr[A + 1]], B))
    assert g.rows[e] == A and g.cols[e] == B
    return int(e)


class GatherCase:
    """One hub network with its exact states, their oracle rates and the references of every pass (built once, left unchanged)."""

    def __init__(self, family, lengths, B=B_EXACT, second=True):
        from oracle import oracle as orc
        self.family, self.lengths, self.B, self.second = family, tuple(lengths), B, second
        self.net, self.hubs = hub_network(family, lengths)
        self.U, self.K = exact_states(self.net.n_species, self.net.n_reactions, B, seed=len(lengths) + max(lengths))
        self.on = orc.OracleNetwork.from_flat(self.net)
        self.rates = np.stack([self.on.rates(self.K[b], self.U[b]) for b in range(B)])
        self._pfa, self._ri, self._ref = {}, {}, {}
        # the temperature form: the same states, Arrhenius parameters of the synthetic networks' ranges
        rng = np.random.default_rng(17)
        R = self.net.n_reactions
        self.Ea, self.A = rng.uniform(1e4, 8e4, R), 10.0 ** rng.uniform(6, 10, R)
        self.T = rng.uniform(600.0, 1200.0, B)

    def pfa(self, pairing):
        if pairing not in self._pfa:
            self._pfa[pairing] = pc.PfaRef(self.net, pairing, second=self.second)
        return self._pfa[pairing]

    def drgep(self, pairing):
        return self.pfa(pairing).s

    def drg(self, pairing):
        return self.pfa(pairing).g

    def ri(self, pairing):
        if pairing not in self._ri:
            self._ri[pairing] = rc.RiRef(self.net, pairing)
        return self._ri[pairing]

    def factor(self, pairing):
        """contributions per pair record of the hub rows: 2 for the paired family without pairing"""
        return 2 if self.family == "paired" and not pairing else 1

    def ref(self, what, pairing):
        """"drg": (coef[E], r[B][E]); "drgep": r[B][E]; "pfa": (rp[B][E], rc[B][E]); "ri": (importance[R], I[B][R])"""
        key = (what, pairing)
        if key not in self._ref:
            if what == "drg":
                coef, _, r, _ = self.drg(pairing).coefficients(self.rates)
                self._ref[key] = (coef, r)
            elif what == "drgep":
                self._ref[key] = self.drgep(pairing).coefficients(self.rates)[0]
            elif what == "pfa":
                self._ref[key] = self.pfa(pairing).split_all(self.rates)[:2]
            else:
                imp, _, I, _ = self.ri(pairing).importance(self.rates)
                self._ref[key] = (imp, I)
        return self._ref[key]

    # -- the temperature form ------------------------------------------------------------------------------------------------
    def t_rates(self):
        if "t_rates" not in self._ref:
            k = [self.on_arrhenius(b) for b in range(self.B)]
            self._ref["t_rates"] = np.stack([self.on.rates(k[b], self.U[b]) for b in range(self.B)])
        return self._ref["t_rates"]

    def on_arrhenius(self, b):
        from oracle import oracle as orc
        return orc.arrhenius(self.Ea, self.A, self.T[b])

    def ex(self):
        """extra relative error of every rate in the temperature form, [B][R] (drg_cases.SynthCase.ex)"""
        return (2.0 * np.abs(self.Ea[None, :] / (RGAS * self.T[:, None])) + 16.0) * EPS

    def t_ref(self, what, pairing):
        """(reference, bound) per (entry, state) of the temperature form, by the modules' own derived bounds"""
        key = ("T", what, pairing)
        if key not in self._ref:
            q, ex = self.t_rates(), self.ex()
            if what == "drg":
                coef, bound, _, bounds = self.drg(pairing).coefficients(q, ex)
                self._ref[key] = (coef, bound, bounds)
            elif what == "drgep":
                self._ref[key] = self.drgep(pairing).coefficients(q, ex)
            elif what == "pfa":
                self._ref[key] = self.pfa(pairing).split_all(q, ex)
            else:
                imp, bound, _, bounds = self.ri(pairing).importance(q, ex)
                self._ref[key] = (imp, bound, bounds)
        return self._ref[key]


# name -> (family, lengths, states, second stage in the reference). The paired hubs' colliders have rows of their own, so E2
# of a paired network grows with 4 n^2: PFA takes the paired family up to 257 in one network and 1025 alone on three states.
GATHER = {
    "collider": ("collider", LENGTHS, B_EXACT, True),
    "paired": ("paired", LENGTHS, B_EXACT, False),
    "paired_small": ("paired", LENGTHS[:7], B_EXACT, True),
    "paired_1025": ("paired", (1025,), 3, False),
}
PFA_GATHER = ("collider", "paired_small", "paired_1025")       # the gather cases the PFA pass runs on
TRIP_LENGTHS = (9, 257, 1025)
_gather = {}


def gather_case(name):
    if name not in _gather:
        family, lengths, B, second = GATHER[name]
        _gather[name] = GatherCase(family, lengths, B, second)
    return _gather[name]


def order_sums(terms):
    """(forward, reverse, fsum) of a list of terms in float64"""
    fwd = rev = 0.0
    for t in terms:
        fwd += t
    for t in terms[::-1]:
        rev += t
    return fwd, rev, math.fsum(terms)


# ---- PFA and path families -------------------------------------------------------------------------------------------------
def double_star(d, m):
    """(n_species, reacs, prods, A, M): A = 0, M = 1, the leaves of A 2 .. d, those of M d + 1 .. d + m - 1"""
    reacs, prods = [[(0, 1)]], [[(1, 1)]]
    for i, leaf in enumerate(range(2, d + 1)):
        a, b = (0, leaf) if i % 2 == 0 else (leaf, 0)
        reacs.append([(a, 1)]); prods.append([(b, 1)])
    for i, leaf in enumerate(range(d + 1, d + m)):
        a, b = (1, leaf) if i % 2 == 0 else (leaf, 1)
        reacs.append([(a, 1)]); prods.append([(b, 1)])
    return d + m, reacs, prods, 0, 1


def broom(d, l):
    """(n_species, reacs, prods, A, M): A = 0, its neighbours 1 .. d, the leaves of neighbour i at 1 + d + i l .."""
    reacs, prods = [], []
    for i in range(d):
        M = 1 + i
        reacs.append([(0, 1)] if i % 2 == 0 else [(M, 1)]); prods.append([(M, 1)] if i % 2 == 0 else [(0, 1)])
        for j in range(l):
            leaf = 1 + d + i * l + j
            reacs.append([(M, 1)] if j % 2 == 0 else [(leaf, 1)]); prods.append([(leaf, 1)] if j % 2 == 0 else [(M, 1)])
    return 1 + d + d * l, reacs, prods, 0, 1


def union(parts):
    """(net, [(kind, p, q, A, M)]) of the disjoint union of parts [(kind, p, q)], kind "ds" or "br" """
    n, reacs, prods, where = 0, [], [], []
    for kind, p, q in parts:
        ns, re, pr, A, M = (double_star if kind == "ds" else broom)(p, q)
        reacs += [[(s + n, c) for s, c in x] for x in re]
        prods += [[(s + n, c) for s, c in x] for x in pr]
        where.append((kind, p, q, A + n, M + n))
        n += ns
    return from_lists(n, reacs, prods), where


OUT_DEGREES = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129)          # chunk (PFA_CHUNK = 64) and look-ahead (PFA_AHEAD = 4) edges
M_DEGREES = (64, 65, 256, 257)                               # deg(M) = WG and WG + 1 at either width
E2_ROWS = (64, 65, 384, 385, 1536, 1537)                     # PFA_KEEP * WG register columns at either width, and the spill
IN_DEGREES = (32, 33, 256, 257, 512, 513)                    # DRGEP_IN_SHORT_MAX, DRGEP_IN_WAVE_MAX, the workgroup's stride
PFA_PARTS = {
    "stars": [("ds", d, 3) for d in OUT_DEGREES] + [("ds", 63, 64), ("ds", 64, 65), ("ds", 5, 256), ("ds", 65, 257)],
    "brooms": [("br", 8, 7), ("br", 13, 4), ("br", 64, 5), ("br", 55, 6), ("br", 128, 11), ("br", 29, 52)],
}
PATH_PARTS = [("ds", d, 3) for d in IN_DEGREES] + [("ds", 513, 257)]
DS_SIZES = ((64, 65), (65, 257), (129, 1408), (3, 1535))     # double stars whose sizes the host test checks


class PfaCase:
    """A union of double stars and brooms, exact first-generation coefficients and the second stage's reference."""

    def __init__(self, name, B=B_EXACT):
        self.net, self.where = union(PFA_PARTS[name])
        self.g = pc.PfaRef(self.net, 1)
        rng = np.random.default_rng(len(name))
        self.rp, self.rc = (rng.choice([0.0, 0.25, 0.5, 1.0], (B, self.g.E)) for _ in range(2))
        self.rp[ZERO_STATE] = 0.0; self.rc[ZERO_STATE] = 0.0
        self._r = None

    def r(self):
        if self._r is None:
            self._r = self.g.second_all(self.rp, self.rc)
        return self._r

    def row_cost(self):
        g = self.g
        return np.array([g.deg[g.cols[g.rowptr[a]:g.rowptr[a + 1]]].sum() for a in range(g.n)])


_pfa = {}


def pfa_case(name):
    if name not in _pfa:
        _pfa[name] = PfaCase(name)
    return _pfa[name]


class PathCase:
    """The double stars of IN_DEGREES as one network, DRGEP's pattern of it and coefficients for the path search."""

    def __init__(self):
        self.net, self.where = union(PATH_PARTS)
        self.g = ec.DrgepRef(self.net, 1)
        self.in_deg = np.bincount(self.g.cols, minlength=self.g.n)
        rng = np.random.default_rng(7)
        r = rng.random((B_EXACT, self.g.E)) ** 3              # the random r of test_gpu_drgep.py
        r[rng.random(r.shape) < 0.3] = 0.0
        r[rng.random(r.shape) < 0.05] = 1.0
        self.r = r
        # every hub and every M: 0.25 on the incoming edges, the winner 0.5 on the LAST of them
        self.planted = np.zeros((1, self.g.E))
        self.centres = [A for _, _, _, A, _ in self.where] + [M for _, _, _, _, M in self.where]
        for c in self.centres:
            e_in = np.flatnonzero(self.g.cols == c)
            self.planted[0, e_in] = 0.25
            self.planted[0, e_in[-1]] = 0.5
        self.leaves = [s for s in range(self.g.n) if s not in set(self.centres)]


_path = []


def path_case():
    if not _path:
        _path.append(PathCase())
    return _path[0]
