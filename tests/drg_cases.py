"""The directed relation graph written plainly in NumPy - the reference of the DRG tests - and the networks they share.

Definition (include/kinetica_hip.h, "directed relation graph"). Reaction rates q_r are the oracle's (OracleNetwork.rates).
Records: with pairing a reaction and its exact reverse, paired by the network compiler's rule - reactions in order; a
PLAIN reaction (no species on both sides, at most two product molecules) whose reverse is an earlier, still unpaired plain
reaction joins the LATEST such reaction, which becomes the record's forward; everything else is a record of its own - and
w = q_kf - q_kr; without pairing every reaction is a record and w = q_r. nu_A: net coefficient of A in the forward reaction,
S: the species on either side of it.
    den_A  = sum over records with nu_A != 0                   of |nu_A| |w|
    num_AB = sum over records with nu_A != 0, B in S, B != A   of |nu_A| |w|
    r_AB   = num_AB / den_A (0.0 where den_A == 0),  coef_AB = max over the states of r_AB
An edge (A, B) exists when some record contributes to num_AB. Every sum here is math.fsum."""
import math

import numpy as np

from kinetica_jl_amd.synth import from_lists, synthetic_crn

EPS = 2.0 ** -53
RGAS = 8.314462618


def records(net, pairing):
    """[(kf, kr, {species: nu}, [species of S])] in record order."""
    R = net.n_reactions
    nets, sets = [], []
    for r in range(R):
        re, pr = net.reaction(r)
        nu = {}
        for s, c in re:
            nu[int(s)] = nu.get(int(s), 0) - int(c)
        for s, c in pr:
            nu[int(s)] = nu.get(int(s), 0) + int(c)
        sets.append(sorted(nu))
        nets.append({s: c for s, c in nu.items() if c != 0})
    if not pairing:
        return [(r, -1, nets[r], sets[r]) for r in range(R)]
    partner = [-1] * R
    waiting = {}
    for r in range(R):
        re, _ = net.reaction(r)
        nu = nets[r]
        plain = all(nu.get(int(s), 0) == -int(c) for s, c in re) and 1 <= sum(c for c in nu.values() if c > 0) <= 2
        if not plain:
            continue
        fwd = tuple(sorted(nu.items()))
        rev = tuple(sorted((s, -c) for s, c in nu.items()))
        if waiting.get(rev):
            q = waiting[rev].pop()
            partner[r], partner[q] = q, r
        else:
            waiting.setdefault(fwd, []).append(r)
    return [(r, partner[r], nets[r], sets[r]) for r in range(R) if not (0 <= partner[r] < r)]


class DrgRef:
    """Pattern and contribution lists of one (network, pairing), and the coefficients of given per-state rates."""

    def __init__(self, net, pairing):
        self.net, self.pairing, self.n = net, bool(pairing), net.n_species
        den, num = [], []         # (A, kf, kr, |nu|), (A, B, kf, kr, |nu|)
        for kf, kr, nu, S in records(net, pairing):
            for A, c in nu.items():
                den.append((A, kf, kr, abs(c)))
                num.extend((A, B, kf, kr, abs(c)) for B in S if B != A)
        den.sort(key=lambda x: x[0])
        num.sort(key=lambda x: (x[0], x[1]))
        self.den = np.array(den, np.int64).reshape(-1, 4)
        self.num = np.array(num, np.int64).reshape(-1, 5)
        self.den_ptr = np.searchsorted(self.den[:, 0], np.arange(self.n + 1)).astype(np.int64)
        key = self.num[:, 0] * self.n + self.num[:, 1]
        ekey, first = np.unique(key, return_index=True)
        self.edge_ptr = np.append(first, len(key)).astype(np.int64)
        self.rows, self.cols = ekey // self.n, ekey % self.n
        self.rowptr = np.searchsorted(self.rows, np.arange(self.n + 1)).astype(np.int64)
        self.colidx = self.cols.astype(np.int64)
        self.E = len(ekey)

    def info(self):
        """The sizes kin_drg_pattern_host reports."""
        cls = lambda ptr: [int(np.sum(m)) for L in [np.diff(ptr)] for m in (L <= 8, (L > 8) & (L <= 256), L > 256)]
        d, e = cls(self.den_ptr), cls(self.edge_ptr)
        return dict(edges=self.E, den_contributions=len(self.den), edge_contributions=len(self.num), den_short=d[0], den_medium=d[1],
                    den_long=d[2], edge_short=e[0], edge_medium=e[1], edge_long=e[2])

    @staticmethod
    def _terms(tab, col, q, ex):
        """Per contribution: the term |nu| |q_f - q_r| and the bound of its absolute error (see test_gpu_drg.py)."""
        kf, kr, c = tab[:, col], tab[:, col + 1], tab[:, col + 2].astype(float)
        qf = q[kf]
        qr = np.where(kr >= 0, q[np.maximum(kr, 0)], 0.0)
        exf = ex[kf]
        exr = np.where(kr >= 0, ex[np.maximum(kr, 0)], 0.0)
        return c * np.abs(qf - qr), c * ((6 * EPS + exf) * np.abs(qf) + (6 * EPS + exr) * np.abs(qr))

    @staticmethod
    def _rowsum(v, ptr):
        return np.array([math.fsum(v[ptr[i]:ptr[i + 1]]) for i in range(len(ptr) - 1)])

    def state(self, q, ex=None):
        """(r[E], bound[E]) of one state's rates q[R]; ex[R]: extra relative error of every rate (temperature form)."""
        ex = np.zeros(len(q)) if ex is None else ex
        td, ed = self._terms(self.den, 1, q, ex)
        tn, en = self._terms(self.num, 2, q, ex)
        den, dden = self._rowsum(td, self.den_ptr), self._rowsum(ed, self.den_ptr)
        num, dnum = self._rowsum(tn, self.edge_ptr), self._rowsum(en, self.edge_ptr)
        dden = dden + np.diff(self.den_ptr) * EPS * den
        dnum = dnum + np.diff(self.edge_ptr) * EPS * num
        dA, ddA = den[self.rows], dden[self.rows]
        pos = dA > 0
        r = np.where(pos, num / np.where(pos, dA, 1.0), 0.0)
        bound = np.where(pos, (dnum + r * ddA) / np.where(pos, dA, 1.0) + 2 * EPS, np.where(ddA > 0, np.inf, 0.0))
        return r, bound

    def coefficients(self, rates, ex=None):
        """(coef[E], bound[E], r[B][E], bounds[B][E]) of rates[B][R]: the maximum over the states and the largest per-state bound."""
        rates = np.atleast_2d(rates)
        rs, bs = zip(*[self.state(rates[b], None if ex is None else ex[b]) for b in range(len(rates))]) if len(rates) else ((), ())
        if not rs:
            z = np.zeros(self.E)
            return z, z.copy(), np.zeros((0, self.E)), np.zeros((0, self.E))
        r, b = np.stack(rs), np.stack(bs)
        return r.max(axis=0), b.max(axis=0), r, b


def select(rowptr, colidx, coef, targets, eps):
    """Species reachable from `targets` over edges with coef >= eps (plain breadth-first search): sorted ids."""
    seen = set(int(t) for t in targets)
    todo = list(seen)
    while todo:
        a = todo.pop()
        for e in range(rowptr[a], rowptr[a + 1]):
            b = int(colidx[e])
            if coef[e] >= eps and b not in seen:
                seen.add(b); todo.append(b)
    return np.array(sorted(seen), np.int64)


# ---- networks ------------------------------------------------------------------------------------------------------------
def hand_networks():
    """name -> (net, k[R], U[B][N], {pairing: {(A, B): coef}}): every edge of the graph with its hand value (dyadic numbers:
    exact in binary). The last state of every U is all zeros."""
    out = {}
    z = lambda U: np.vstack([np.array(U, float), np.zeros((1, len(U[0])))])
    # A -> B
    out["A_to_B"] = (from_lists(2, [[(0, 1)]], [[(1, 1)]]), np.array([2.0]), z([[0.5, 0.25]]),
                     {p: {(0, 1): 1.0, (1, 0): 1.0} for p in (0, 1)})
    # A <=> B with kf uA == kr uB exactly: paired den = 0 -> 0.0, unpaired 1
    out["A_eq_B_balanced"] = (from_lists(2, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(0, 1)]]), np.array([2.0, 4.0]), z([[0.5, 0.25]]),
                              {1: {(0, 1): 0.0, (1, 0): 0.0}, 0: {(0, 1): 1.0, (1, 0): 1.0}})
    # 2A -> B
    out["2A_to_B"] = (from_lists(2, [[(0, 2)]], [[(1, 1)]]), np.array([3.0]), z([[0.5, 4.0]]),
                      {p: {(0, 1): 1.0, (1, 0): 1.0} for p in (0, 1)})
    # A + M -> B + M: M has no denominator term, but the edges A -> M and B -> M exist
    out["A_M_to_B_M"] = (from_lists(3, [[(0, 1), (2, 1)]], [[(1, 1), (2, 1)]]), np.array([2.0]), z([[0.5, 0.25, 4.0]]),
                         {p: {(0, 1): 1.0, (0, 2): 1.0, (1, 0): 1.0, (1, 2): 1.0} for p in (0, 1)})
    # A + B -> 2B beside A -> C: q = (2 * 0.5 * 0.25, 0.5 * 0.5) = (0.25, 0.25); den_A = 0.5, num_AB = 0.25
    out["A_B_to_2B"] = (from_lists(3, [[(0, 1), (1, 1)], [(0, 1)]], [[(1, 2)], [(2, 1)]]), np.array([2.0, 0.5]), z([[0.5, 0.25, 0.0]]),
                        {p: {(0, 1): 0.5, (0, 2): 0.5, (1, 0): 1.0, (2, 0): 1.0} for p in (0, 1)})
    return out


def hub_network(n_long=300, n_mid=20):
    """A + X_i -> B + X_i for i < n_long and C + X_i -> D + X_i for i < n_mid (colliders: never paired): the rows A, B and the
    edges (A, B), (B, A) carry n_long contributions (long), C, D and (C, D), (D, C) n_mid (medium), every other edge one."""
    n = 4 + n_long
    reacs = [[(0, 1), (4 + i, 1)] for i in range(n_long)] + [[(2, 1), (4 + i, 1)] for i in range(n_mid)]
    prods = [[(1, 1), (4 + i, 1)] for i in range(n_long)] + [[(3, 1), (4 + i, 1)] for i in range(n_mid)]
    return from_lists(n, reacs, prods)


def post_cutoff(net, Ea, A, seed=11):
    """About 30 % of the reactions removed, R odd: records that lost their reverse (kr = -1) and a half-filled last pair."""
    keep = np.flatnonzero(np.random.default_rng(seed).random(net.n_reactions) >= 0.3)
    if len(keep) % 2 == 0:
        keep = keep[:-1]
    return net.subset(keep), Ea[keep], A[keep]


def states(n, B, seed=0):
    """The states of test_gpu_flux.py: 10^U(-12, 0), a one-hot row, a row with exact zeros, entries of -1e-14."""
    rng = np.random.default_rng(seed)
    U = 10.0 ** rng.uniform(-12, 0, (B, n))
    U[0] = 0.0; U[0, 0] = 1.0
    if B > 1:
        U[1, rng.random(n) < 0.3] = 0.0
    if B > 2:
        U[2, rng.choice(n, 5, replace=False)] = -1e-14
    return U


_synth = {}


def synth(n, r):
    if (n, r) not in _synth:
        _synth[(n, r)] = synthetic_crn(n, r)
    return _synth[(n, r)]


MODES = ("shared", "per_state", "k_row", "T", "T_kmax")
BMAX = 130


class SynthCase:
    """One network with BMAX states, every rate-constant source of test_gpu_flux.py and the reference coefficients (cached)."""

    def __init__(self, net, Ea, A):
        from oracle import oracle as orc
        self.orc, self.net, self.Ea, self.A = orc, net, Ea, A
        self.on = orc.OracleNetwork.from_flat(net)
        self.U = states(net.n_species, BMAX)
        rng = np.random.default_rng(2)
        self.k0 = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
        self.K = self.k0[None, :] * rng.uniform(0.5, 2.0, (BMAX, 1)) * rng.uniform(0.9, 1.1, (BMAX, net.n_reactions))
        self.K3 = self.K[:3].copy()
        self.row3 = rng.integers(0, 3, BMAX).astype(np.int64)
        self.T = rng.uniform(600.0, 1200.0, BMAX)
        self._graph, self._rates, self._ref = {}, {}, {}

    def graph(self, pairing):
        if pairing not in self._graph:
            self._graph[pairing] = DrgRef(self.net, pairing)
        return self._graph[pairing]

    def k_of(self, mode, b):
        if mode == "shared":
            return self.k0
        if mode == "per_state":
            return self.K[b]
        if mode == "k_row":
            return self.K3[self.row3[b]]
        return self.orc.arrhenius(self.Ea, self.A, self.T[b], k_max=1e12 if mode == "T_kmax" else None)

    def source(self, mode, B):
        """Keywords of HipNetwork.drg_batched for the first B states (mode "shared": the caller sets the handle's rates to k0)."""
        if mode == "per_state":
            return dict(k=self.K[:B])
        if mode == "k_row":
            return dict(k=self.K3, k_row=self.row3[:B])
        if mode.startswith("T"):
            return dict(T=self.T[:B])
        return {}

    def ex(self, mode, B):
        """Extra relative error of every rate in the temperature form, [B][R]; None with rate constants given."""
        if not mode.startswith("T"):
            return None
        return (2.0 * np.abs(self.Ea[None, :] / (RGAS * self.T[:B, None])) + 16.0) * EPS

    def ref(self, mode, pairing, B):
        """(coef[E], bound[E], bounds[B][E]) over the first B states; the per-state rows are computed once for the largest B asked."""
        key = (mode, pairing)
        have = self._ref.get(key)
        if have is None or have[0].shape[0] < B:
            if mode not in self._rates or self._rates[mode].shape[0] < B:
                self._rates[mode] = np.stack([self.on.rates(self.k_of(mode, b), self.U[b]) for b in range(B)])
            _, _, r, bd = self.graph(pairing).coefficients(self._rates[mode][:B], self.ex(mode, B))
            have = self._ref[key] = (r, bd)
        r, bd = have[0][:B], have[1][:B]
        return r.max(axis=0), bd.max(axis=0), bd


_cases = {}


def synth_case(name):
    """"300x1500", "1000x5000" or "300x1500_cut" (post_cutoff of the first)."""
    if name not in _cases:
        if name == "300x1500_cut":
            _cases[name] = SynthCase(*post_cutoff(*synth(300, 1500)))
        else:
            n, r = (int(x) for x in name.split("x"))
            _cases[name] = SynthCase(*synth(n, r))
    return _cases[name]
