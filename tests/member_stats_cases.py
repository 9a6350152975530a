"""Seeded blocks of states for the cross-member statistics (kin_members_* / kin_ensemble_*) and the NumPy restatement of every
rule of include/kinetica_hip.h: participants in member order, exact sums (math.fsum) for moments and correlations, the
quantile rule with a separately rounded multiply and add (NumPy's elementwise operations never fuse), scipy.stats.rankdata for
the average-tie ranks. Shared by test_member_stats_host.py (no device) and the two GPU files."""
import functools
import math
from fractions import Fraction

import numpy as np
from scipy.stats import rankdata

EPS = 2.0 ** -53

# the special columns of a block (species ids; a block has at least 5 species)
SP_EQUAL, SP_SUBNORMAL, SP_NAN, SP_INF, SP_PLAIN = 0, 1, 2, 3, 4


def chain_network(N, index_base=0):
    """The arguments of capi.HipNetwork for the chain 0 -> 1 -> ... -> N - 1, species ids in `index_base` (the statistics never
    look at the reactions: any network with N species serves)."""
    ptr = np.arange(N, dtype=np.int64)
    one = np.ones(N - 1, dtype=np.int64)
    return N, ptr, np.arange(N - 1, dtype=np.int64) + index_base, one, ptr, np.arange(1, N, dtype=np.int64) + index_base, one


@functools.lru_cache(maxsize=None)
def block(K, L, N, seed=0):
    """u[K][L][N]: log-uniform over 30 decades with signs, 40 % exact zeros (of both signs); species 0 all equal, species 1
    subnormal, species 2 a NaN at (member 0, row 0), species 3 a +Inf at (member 0, last row). Read-only."""
    rng = np.random.default_rng([seed, K, L, N])
    u = rng.choice([-1.0, 1.0], (K, L, N)) * 10.0 ** rng.uniform(-15, 15, (K, L, N))
    u[rng.random((K, L, N)) < 0.4] = 0.0
    u[rng.random((K, L, N)) < 0.05] = -0.0
    u[:, :, SP_EQUAL] = 3.25
    u[:, :, SP_SUBNORMAL] = rng.integers(-40, 40, (K, L)) * 5e-324
    u[0, 0, SP_NAN] = np.nan
    u[0, L - 1, SP_INF] = np.inf
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def inputs(K, seed=0):
    """X[K][4]: normal draws, a heavily tied column (four levels), a monotone function of the block-independent draw with
    noise, a constant column."""
    rng = np.random.default_rng([seed, K, 77])
    z = rng.standard_normal(K)
    X = np.stack([z, rng.integers(0, 4, K).astype(float), np.exp(z) + 0.1 * rng.standard_normal(K), np.full(K, 2.5)], axis=1)
    X.setflags(write=False)
    return X


def masks(K):
    """The participant masks of a block of K members: (label, use or None), giving n = 0, 1, 2 and K (those that exist)."""
    out = [("none", np.zeros(K, np.int32))]
    one = np.zeros(K, np.int32); one[0] = 1
    out.append(("one", one))
    if K >= 2:
        two = one.copy(); two[K - 1] = 7      # (any non-zero value takes part)
        out.append(("two", two))
    if K >= 3:
        out.append(("all", None))
    return out


def participants(K, use):
    return np.arange(K) if use is None else np.flatnonzero(np.asarray(use) != 0)


def _fsum_cols(a):
    """math.fsum along axis 0 of a 2-D array (non-finite columns: what IEEE addition gives)."""
    out = np.empty(a.shape[1])
    for c in range(a.shape[1]):
        col = a[:, c]
        out[c] = math.fsum(col) if np.all(np.isfinite(col)) else np.sum(col)
    return out


def ref_moments(u, use=None):
    """dict(count, mean, var, min, max, abs_mean, S): mean from the exact sum, S the exact sum of squared deviations from it,
    abs_mean = sum |x| / n (the bounds' scale). n == 0: zeros. NaN columns: NaN."""
    K, L, N = u.shape
    idx = participants(K, use)
    n = len(idx)
    if n == 0:
        z = np.zeros((L, N))
        return dict(count=0, mean=z, var=z, min=z, max=z, abs_mean=z, S=z)
    x = u[idx].reshape(n, L * N)
    with np.errstate(all="ignore"):
        mean = _fsum_cols(x) / n
        S = _fsum_cols((x - mean) ** 2)
        var = S / (n - 1) if n > 1 else S
        out = dict(count=n, mean=mean, var=var, min=x.min(axis=0), max=x.max(axis=0), abs_mean=_fsum_cols(np.abs(x)) / n, S=S)
    return {k: (v.reshape(L, N) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def quantile_rule(xs, p):
    """The header's rule over sorted values xs[n] (or xs[n][columns]) for one probability p: h = (n - 1) p, lo = floor(h),
    g = h - lo; xs[lo] when g == 0, else xs[lo] + (xs[lo + 1] - xs[lo]) * g with the product and the sum rounded separately."""
    n = xs.shape[0]
    h = (n - 1) * float(p)
    lo = int(math.floor(h))
    g = h - lo
    if g == 0.0 or lo + 1 >= n:
        return xs[lo].copy() if isinstance(xs[lo], np.ndarray) else xs[lo]
    with np.errstate(all="ignore"):
        prod = (xs[lo + 1] - xs[lo]) * g
        return xs[lo] + prod


def ref_quantiles(u, p, species=None, use=None):
    """out[Q][L][n_sel] (species: 0-based ids; None: all). n == 0: zeros. A column holding a NaN: NaN."""
    K, L, N = u.shape
    sp = np.arange(N) if species is None else np.asarray(species, dtype=int)
    idx = participants(K, use)
    p = np.atleast_1d(np.asarray(p, dtype=float))
    if len(idx) == 0:
        return np.zeros((len(p), L, len(sp)))
    x = u[idx][:, :, sp].reshape(len(idx), L * len(sp))
    nan = np.isnan(x).any(axis=0)
    xs = np.sort(x, axis=0)
    out = np.stack([quantile_rule(xs, q) for q in p])
    out[:, nan] = np.nan
    return out.reshape(len(p), L, len(sp))


def ranks(v):
    """1-based average-tie ranks along axis 0 (-0.0 and +0.0 tie)."""
    return rankdata(v, method="average", axis=0)


def normalised(v):
    """(v - mean) / sqrt(sum (v - mean)^2) of a vector from exact sums; zeros without spread or for n < 2; NaN with a NaN."""
    v = np.asarray(v, dtype=float)
    if np.isnan(v).any():
        return np.full(len(v), np.nan)
    if len(v) < 2 or v.min() == v.max():
        return np.zeros(len(v))
    # rational arithmetic: the mean, the deviations and their squares are exact; three roundings at the end (under 2 ulp)
    f = [Fraction(float(x)) for x in v]
    m = sum(f) / len(f)
    d = [x - m for x in f]
    root = math.sqrt(float(sum(x * x for x in d)))
    return np.array([float(x) for x in d]) / root


def ref_inputs(X, use=None, rank=True):
    """(n, Xhat[n][P]) of kin_members_inputs_host."""
    X = np.asarray(X, dtype=float)
    idx = participants(X.shape[0], use)
    x = X[idx]
    out = np.zeros(x.shape)
    for p in range(x.shape[1]):
        col = x[:, p]
        if rank and len(col) and not np.isnan(col).any():
            col = ranks(col)
        out[:, p] = normalised(col)
    return len(idx), out


def pearson_exact(x, y):
    """(r, bound_factor): r = sum (x - xbar)(y - ybar) / sqrt(Sxx Syy) from exact sums - exactly 0.0 where a sum of squares is 0
    or n < 2, NaN with a NaN or where the deviations are not finite - and 1 + sqrt(n) (|xbar| / sqrt(Sxx) + |ybar| / sqrt(Syy)),
    the factor of the gate (inf where r is 0.0 by rule)."""
    n = len(x)
    if np.isnan(x).any() or np.isnan(y).any():
        return np.nan, np.inf
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        return np.nan, np.inf      # (values only: an infinite value has a finite rank)
    if n < 2 or x.min() == x.max() or y.min() == y.max():
        return 0.0, np.inf
    mx, my = math.fsum(x) / n, math.fsum(y) / n
    dx, dy = x - mx, y - my
    Sxx, Syy = math.fsum(dx * dx), math.fsum(dy * dy)
    if Sxx == 0.0 or Syy == 0.0:
        return 0.0, np.inf
    r = math.fsum(dx * dy) / math.sqrt(Sxx) / math.sqrt(Syy)
    return r, 1.0 + math.sqrt(n) * (abs(mx) / math.sqrt(Sxx) + abs(my) / math.sqrt(Syy))


# The gate of a correlation: |got - ref| <= CORR_C (n + 16) EPS (1 + sqrt(n) (|xbar| / sqrt(Sxx) + |ybar| / sqrt(Syy))).
# Derivation (unit roundoff EPS; xhat, yhat the exact normalised vectors, sum |xhat yhat| <= 1 by Cauchy-Schwarz):
#   the product sum     one fma chain over the n participants: n EPS sum |xhat yhat| <= n EPS
#   Xhat from the host  within 4 ulp = 8 EPS of exact (test_member_stats_host.py checks it): 8 EPS
#   Yhat on the device  d = y - mean rounds once; S is 32 chains of ceil(n / 32) fma and 31 additions, its d's carry 2 EPS:
#                       (n / 32 + 34) EPS on S, half of it through the root, one rounding each for root and quotient:
#                       (n / 64 + 20) EPS. For ranks d and S are exact: 3 EPS.
#   the mean's error    e = mean - ybar shifts every d by the same e: the product sum changes by e sum xhat / sqrt(Syy), and
#                       sum xhat is 0 up to 8 EPS sqrt(n); S grows by n e^2. With |e| <= n EPS sum |y| / n <=
#                       n EPS (|ybar| + sqrt(Syy / n)) the relative change of r is rho^2 / 2, rho = n EPS (1 + sqrt(n) |ybar| /
#                       sqrt(Syy)): second order, below EPS times the gate's factor whenever the gate is below 1e-9.
#   the restatement     rounds the deviations and the three quotients: 8 EPS
# Together (1.02 n + 36) EPS (1 + ...): c = 3 covers it for every n >= 1 (3 n + 48), c = 2 does not at n = 2 (36 against 38).
# CORR_C = 4 leaves one (n + 16) EPS for the second-order terms named above.
CORR_C = 4.0


def ref_correlate(u, X, species=None, rank=True, use=None):
    """(r[L][n_sel][P], bound[L][n_sel][P]): the exact-sum restatement and the gate of every entry (inf where the entry is 0.0
    or NaN by rule, to be compared exactly)."""
    K, L, N = u.shape
    sp = np.arange(N) if species is None else np.asarray(species, dtype=int)
    idx = participants(K, use)
    n, P = len(idx), X.shape[1]
    r = np.zeros((L, len(sp), P))
    bound = np.full((L, len(sp), P), np.inf)
    if n == 0:
        return r, bound
    xs = X[idx]
    for p in range(P):
        x = xs[:, p]
        if rank and not np.isnan(x).any():
            x = ranks(x)
        for j in range(L):
            for s, i in enumerate(sp):
                y = u[idx, j, i]
                if rank and not np.isnan(y).any():
                    y = ranks(y)
                r[j, s, p], f = pearson_exact(x, y)
                bound[j, s, p] = CORR_C * (n + 16) * EPS * f
    return r, bound


def same_bits_or_zero(a, b):
    """Equal bit for bit, zeros compared by value, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def mismatches(a, b, limit=6):
    """The first entries at which same_bits_or_zero fails, for an assertion's message."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    at = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return "; ".join(f"{tuple(int(i) for i in ix)}: {a[tuple(ix)]!r} against {b[tuple(ix)]!r}" for ix in at[:limit]) + f" ({len(at)} in all)"
