"""The documented sum orders of the cross-member statistics (member_stats.hpp), replayed operation by operation in
NumPy and `fractions`: what the kernels must give bit for bit on finite columns, whatever their blocking. The two constants
below are the header's; a tuning change that moves one of them moves it here as well.

NumPy's elementwise +, -, /, sqrt are the correctly rounded IEEE operations and never fuse; the one fused operation the orders
name is fma() below. The replays assume that division and square root are correctly rounded on the device too."""
from fractions import Fraction

import numpy as np

import member_stats_cases as mc

MOM_WAVES = 8      # member_stats.hpp: MS_MOM_WAVES, the wavefronts of the moments' workgroup the participants are split over
VAL_LANES = 32     # the participant lanes of the value column pass (256 threads / 8 columns)


def fma(a, b, c):
    """a * b + c rounded once (float() of a Fraction rounds correctly, subnormal results included)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _ordered_sum(x, lanes):
    """x[n][C] -> [C]: lane l adds q = l, l + lanes, ... in that order into one accumulator that starts at 0.0; the `lanes`
    partial sums are added in the order of l (a lane without a participant contributes its 0.0)."""
    part = np.zeros((lanes, x.shape[1]))
    for q0 in range(0, x.shape[0], lanes):
        blk = x[q0:q0 + lanes]
        part[:len(blk)] += blk
    tot = part[0].copy()
    for l in range(1, lanes):
        tot += part[l]
    return tot


def _ordered_sumsq(d, lanes):
    """d[n][C] -> [C]: S = fma(d, d, S) per lane in the order of _ordered_sum, the partials added in the order of the lanes."""
    n, C = d.shape
    out = np.empty(C)
    for c in range(C):
        part = [0.0] * lanes
        for q, v in enumerate(d[:, c].tolist()):
            part[q % lanes] = fma(v, v, part[q % lanes])
        t = part[0]
        for l in range(1, lanes):
            t += part[l]
        out[c] = t
    return out


def _finite(x):
    x = np.asarray(x, dtype=float)
    assert x.ndim == 2 and x.shape[0] >= 1 and np.all(np.isfinite(x)), "the replays take finite columns x[n][C], n >= 1"
    return x


def replay_moments(x):
    """(mean[C], var[C]) of the finite columns x[n][C] in the order of ms_moments_kernel."""
    x = _finite(x)
    n = x.shape[0]
    mean = _ordered_sum(x, MOM_WAVES) / float(n)
    S = _ordered_sumsq(x - mean, MOM_WAVES)
    return mean, (S / float(n - 1) if n > 1 else S)


def replay_values(y, flat_rule=True, want_S=False):
    """Yhat[n][C] of ms_values_kernel over the finite columns y[n][C]: 32 lanes, d = y - mean, S as above, d / sqrt(S); zeros
    where the column's minimum equals its maximum (flat_rule) or S == 0. want_S: (Yhat, S) with the S the quotient used."""
    y = _finite(y)
    n = y.shape[0]
    d = y - _ordered_sum(y, VAL_LANES) / float(n)
    S = _ordered_sumsq(d, VAL_LANES)
    if flat_rule:
        S = np.where(y.min(axis=0) == y.max(axis=0), 0.0, S)
    with np.errstate(all="ignore"):
        yhat = np.where(S > 0.0, d / np.sqrt(S), 0.0)
    return (yhat, S) if want_S else yhat


def replay_ranks(y):
    """Yhat[n][C] of the sorted pass over columns y[n][C] without a NaN: average-tie ranks, d = rank - (n + 1) / 2 and
    S = sum d^2 exact (multiples of 1/4 far below 2^53: any order), d / sqrt(S), zeros where S == 0."""
    y = np.asarray(y, dtype=float)
    assert y.ndim == 2 and not np.isnan(y).any()
    n = y.shape[0]
    d = mc.ranks(y) - 0.5 * (n + 1)
    S = np.sum(d * d, axis=0)
    assert np.all(4.0 * S == np.floor(4.0 * S)) and np.all(S < 2.0 ** 51)
    with np.errstate(all="ignore"):
        return np.where(S > 0.0, d / np.sqrt(S), 0.0)


def replay_corr(xhat, yhat):
    """r[C][P] of ms_corr_kernel: acc = fma(xhat[q][p], yhat[q][c], acc) over q = 0 .. n - 1, from 0.0 (finite operands)."""
    xhat, yhat = np.asarray(xhat, dtype=float), np.asarray(yhat, dtype=float)
    n, P = xhat.shape
    C = yhat.shape[1]
    assert yhat.shape[0] == n and np.all(np.isfinite(xhat)) and np.all(np.isfinite(yhat))
    out = np.empty((C, P))
    fx = [[Fraction(v) for v in xhat[:, p].tolist()] for p in range(P)]
    for c in range(C):
        fy = [Fraction(v) for v in yhat[:, c].tolist()]
        for p in range(P):
            acc = 0.0
            for a, b in zip(fx[p], fy):
                acc = float(a * b + Fraction(acc)) if a and b else acc + 0.0
            out[c, p] = acc
    return out
