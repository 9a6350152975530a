"""Shared by tests/test_timescale_host.py (no GPU) and tests/test_gpu_timescale.py: the extended-precision reference of the
timescale analysis (kin_jac_batched, kin_timescale_*; definitions: include/kinetica_hip.h) built on jac_cases.Reference, the
bounds every output is judged with, and the networks of the row-pass classes. A plain module: no fixtures, no test collection.

Reference (np.longdouble). Per state: the Jacobian entries J and the right-hand side f of jac_cases.Reference with their
scales S and term counts L; d_i = J_ii, g_i = sum_j |J_ij| over the stored entries of row i, norm = max_i g_i,
e_i = |f_i| / |d_i| (0 where f_i = 0, +Inf where d_i = 0 and f_i != 0).

Bounds (u = 2^-53; derived, nothing here is fitted to what a device returned).
    a Jacobian entry      bound_jac(S, L)                                              (jac_cases)
    f_i                   bound_rhs(S, L)                                              (jac_cases)
    g_i over n entries    sum_j bound_ij + n u g_ref: the entries' own bounds plus at most n - 1 roundings of a sum of
                          non-negative terms, one unit of slack
    norm                  the largest bound of a g_i (|max a - max b| <= max |a - b|)
    e_i                   an INTERVAL: with bf, bd the bounds of f_i, d_i
                              lower end (|f| - bf) / (|d| + bd) (1 - 2u), or 0 if bf >= |f|
                              upper end (|f| + bf) / (|d| - bd) (1 + 2u), or +Inf if bd >= |d|
                          (the quotient of two values inside their bounds, one rounding of the division, one unit of slack).
                          Where f = 0 with bf = 0 the value must be WRITTEN as 0.0; where d = 0 with bd = 0 and |f| > bf it must
                          be +Inf (both ends of the interval are).
    extrema over states   the extrema of the interval ends: max and min are monotone in every argument.
Rate constants formed on the device from a temperature differ from the oracle's by a relative (2 |Ea / (R T)| + 16) u (the
bound tests/test_gpu_flux.py derives for the device's Arrhenius law); every term of reaction r then carries that much more,
`ex`[R] below: the bounds of J and f grow by sum |term| ex_r.

Exact inputs (jac_cases: u in {1/2, 1, 2}, integer k in 1 .. 8): every sum is exact in any order, so vals, diag, norm and
the summary rows 0 and 1 equal the reference bit for bit, and err / qss_err equal float64(|f|) / float64(|d|) bit for bit."""
import numpy as np

from kinetica_jl_amd.synth import from_lists
from tests import jac_cases as jc
from tests.jac_cases import LD, U

INF = LD(np.inf)


def fan_in_net(L):
    """X_j -> H for j = 1 .. L (H = species 0): row H of the Jacobian stores L + 1 entries (its empty diagonal and one column per
    X_j), every row X_j one; H is produced only, so d_H = 0."""
    return from_lists(L + 1, [[(j, 1)] for j in range(1, L + 1)], [[(0, 1)] for _ in range(L)])


def chain_net():
    """A -> X -> B (species 0, 1, 2; reactions 0: A -> X, 1: X -> B)"""
    return from_lists(3, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(2, 1)]])


class StateRef:
    """everything of one state: values, bounds and intervals (longdouble)"""

    def __init__(self, ref, k, u, ex=None):
        self.J, SJ, LJ = ref.jac(k, u)
        self.f, Sf, Lf = ref.rhs(k, u)
        self.bJ, self.bf = jc.bound_jac(SJ, LJ), jc.bound_rhs(Sf, Lf)
        if ex is not None:
            exl = np.asarray(ex).astype(LD)
            je, jv = ref.jac_terms(k, u)
            self.bJ = self.bJ + jc.accumulate(je, np.abs(jv) * exl[ref.j_rx], ref.nnz)[0]
            ts, tv = ref.rhs_terms(k, u)
            self.bf = self.bf + jc.accumulate(ts, np.abs(tv) * exl[ref.t_rx], ref.N)[0]
        self.d, self.bd = self.J[ref.diag], self.bJ[ref.diag]
        n = np.diff(ref.rowptr)
        self.g = np.zeros(ref.N, LD); bsum = np.zeros(ref.N, LD)
        np.add.at(self.g, ref.rows, np.abs(self.J))
        np.add.at(bsum, ref.rows, self.bJ)
        self.bg = bsum + n.astype(LD) * U * self.g
        self.norm, self.bnorm = self.g.max(), self.bg.max()
        af, ad = np.abs(self.f), np.abs(self.d)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.e = np.where(af == 0, LD(0), np.where(ad == 0, INF, af / np.where(ad == 0, LD(1), ad)))
            lo = np.where(self.bf >= af, LD(0), (af - self.bf) / (ad + self.bd) * (1 - 2 * U))
            hi = np.where(self.bd >= ad, INF, (af + self.bf) / np.where(self.bd >= ad, LD(1), ad - self.bd) * (1 + 2 * U))
        zero = (af == 0) & (self.bf == 0)
        self.e_lo, self.e_hi = np.where(zero, LD(0), lo), np.where(zero, LD(0), hi)
        assert not np.any(np.isnan(self.e_lo)) and not np.any(np.isnan(self.e_hi)) and np.all(self.e_lo <= self.e_hi)


class BatchRef:
    """the states of a batch and the summary over them; `count` masks the states that take part (None: all)"""

    def __init__(self, ref, K, Us, ex=None, count=None):
        B = len(Us)
        self.states = [StateRef(ref, K[b], Us[b], None if ex is None else ex[b]) for b in range(B)]
        on = [s for b, s in enumerate(self.states) if count is None or count[b]]
        N = ref.N
        if on:
            nd, bd = np.stack([-s.d for s in on]), np.stack([s.bd for s in on])
            self.summary = np.stack([nd.max(0), nd.min(0), np.stack([s.e for s in on]).max(0)])
            self.lo = np.stack([(nd - bd).max(0), (nd - bd).min(0), np.stack([s.e_lo for s in on]).max(0)])
            self.hi = np.stack([(nd + bd).max(0), (nd + bd).min(0), np.stack([s.e_hi for s in on]).max(0)])
        else:
            self.summary = self.lo = self.hi = identity(N).astype(LD)


def identity(N):
    """summary over no state"""
    return np.stack([np.full(N, -np.inf), np.full(N, np.inf), np.zeros(N)])


def inside(dev, lo, hi):
    """(all inside, index of the first entry outside or None); a NaN is outside every interval"""
    dev = np.asarray(dev).astype(LD)
    ok = (dev >= lo) & (dev <= hi)
    bad = np.flatnonzero(~ok.ravel())
    return bool(ok.all()), (int(bad[0]) if len(bad) else None)


def ratio(dev, ref, bound):
    """largest error / bound over the entries with a positive finite bound"""
    err = np.abs(np.asarray(dev).astype(LD) - ref)
    pos = (bound > 0) & np.isfinite(bound) & np.isfinite(ref)
    return float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0


def err_exact(f, d):
    """e of exact inputs in float64: |f| / |d|, 0.0 where f == 0, +Inf where d == 0 and f != 0"""
    f, d = np.abs(np.asarray(f, dtype=np.float64)), np.abs(np.asarray(d, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f == 0, 0.0, np.where(d == 0, np.inf, f / np.where(d == 0, 1.0, d)))


def exact_expectation(ref, K, Us):
    """what a correct evaluation returns for exact inputs, in float64: dict of vals[B][nnz], diag[B][N], err[B][N], norm[B],
    summary[3][N]; asserts that the reference values are float64 numbers (the inputs were exact)"""
    sts = [StateRef(ref, K[b], Us[b]) for b in range(len(Us))]
    f64 = lambda a: np.asarray(a).astype(np.float64)
    for s in sts:
        for a in (s.J, s.f, s.g):
            assert np.array_equal(f64(a).astype(LD), a)
    vals, diag = np.stack([f64(s.J) for s in sts]), np.stack([f64(s.d) for s in sts])
    err = np.stack([err_exact(f64(s.f), f64(s.d)) for s in sts])
    norm = np.array([float(s.norm) for s in sts])
    return dict(vals=vals, diag=diag, err=err, norm=norm, summary=np.stack([(-diag).max(0), (-diag).min(0), err.max(0)]))


def exact_states(ref, B, seed):
    """B states of the exact set and their rate constants: (U[B][N], K[B][R])"""
    rng = np.random.default_rng(seed)
    return rng.choice(jc.EXACT_U, (B, ref.N)), rng.integers(1, 9, (B, ref.R)).astype(np.float64)
