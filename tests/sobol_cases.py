"""Seeded Saltelli blocks for the Sobol pass (kin_members_sobol / kin_ensemble_sobol), the restatement of the definition of
include/kinetica_hip.h in extended arithmetic (ref_sobol), the documented sum order replayed operation by operation
(replay_sobol; member_stats.hpp has the order, the constants are restated here) and the derived error gates. Shared by
test_sobol_host.py (no device) and the two GPU files."""
import functools
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "ref_sobol needs an extended type (x87 long double: 64-bit significand)"

SB_WAVES = 8      # member_stats.hpp: SB_WAVES, the wavefronts of a workgroup the participants are split over
SB_CHUNK = 8      # member_stats.hpp: SB_CHUNK, the inputs one workgroup takes (no result depends on it)

# the special columns of a block (species ids; a block has at least 5 species)
SP_CONST, SP_NAN_A, SP_NAN_AB, SP_BIG, SP_PLAIN = 0, 1, 2, 3, 4
BIG_MEAN = 1.0e3      # the large-mean column: mean BIG_MEAN times its spread


def nan_input(P):
    """The input whose block AB_p holds the NaN of species SP_NAN_AB: 1, or 0 for a design with one input."""
    return min(1, P - 1)


@functools.lru_cache(maxsize=None)
def block(M, P, L, N, seed=0):
    """u[M (P + 2)][L][N] in the design layout: every column is scale * g(x) of the design's inputs (linear terms, a product
    and a sine, coefficients per column), the scales log-uniform over 24 decades, so that the AB_p blocks differ from A the
    way a design's do. Species 0 is constant, species 1 holds a NaN in block A (sample 0, row 0), species 2 a NaN only in
    block AB_1 (sample 0, last row), species 3 has a mean 1000 times its spread. Read-only."""
    assert N >= 5
    rng = np.random.default_rng([seed, M, P, L, N])
    A, B = rng.random((M, P)), rng.random((M, P))
    X = np.empty((P + 2, M, P))
    X[0], X[1] = A, B
    for p in range(P):
        X[2 + p] = A
        X[2 + p][:, p] = B[:, p]
    coef = rng.uniform(-1.0, 1.0, (L, N, P)) * (rng.random((L, N, P)) < 0.7)
    inter, wave = rng.uniform(-2.0, 2.0, (L, N)), rng.uniform(-1.0, 1.0, (L, N))
    scale = rng.choice([-1.0, 1.0], (L, N)) * 10.0 ** rng.uniform(-12, 12, (L, N))
    g = np.einsum("bmp,jip->bmji", X, coef) + inter * (X[..., 0] * X[..., P - 1])[..., None, None] \
        + wave * np.sin(6.0 * X.sum(axis=-1))[..., None, None] + rng.uniform(-1.0, 1.0, (L, N))
    u = (scale * g).reshape((P + 2) * M, L, N)
    u[:, :, SP_CONST] = 3.25e-3 / 7.0
    u[:, :, SP_BIG] = BIG_MEAN + g.reshape(-1, L, N)[:, :, SP_BIG] / 4.0
    u[0, 0, SP_NAN_A] = np.nan
    u[(2 + nan_input(P)) * M, L - 1, SP_NAN_AB] = np.nan
    u.setflags(write=False)
    return u


def compacted(u, M, P, keep):
    """The design with only the samples keep[M] (a boolean mask): (u', M')."""
    keep = np.asarray(keep, dtype=bool)
    v = u.reshape(P + 2, M, *u.shape[1:])[:, keep]
    return np.ascontiguousarray(v.reshape(-1, *u.shape[1:])), int(keep.sum())


def _participants(M, w):
    wt = np.ones(M, np.int64) if w is None else np.asarray(w, dtype=np.int64)
    assert wt.shape == (M,) and (wt >= 0).all()
    idx = np.flatnonzero(wt > 0)
    return idx, wt[idx], int(wt[idx].sum())


def _columns(u, M, P, idx, species):
    K, L, N = u.shape
    assert K == M * (P + 2)
    sp = np.arange(N) if species is None else np.asarray(species, dtype=int)
    return u[:, :, sp].reshape(P + 2, M, L * len(sp))[:, idx], (L, len(sp))


# The gates. Unit roundoff EPS, n = sum w, g = (n + 16) EPS; starred quantities are the exact ones. The kernel's chains hold at
# most ceil(np / 8) <= n terms per wave and 7 additions of partials, so a sum of terms t carries at most (n / 8 + 8) EPS sum |t|
# from the additions, plus what each term carries itself.
#   mu      chain n / 8 + 8, the weight's product 1, TA + TB 1, the division 1, the restatement 1: (n / 8 + 12) EPS absmean with
#           absmean = (sum w |a| + sum w |b|) / (2 n) >= |mu*|. n / 8 + 12 <= n + 16:   |mu - mu*| <= d_mu = g absmean.
#   V       with delta = mu - mu*: sum w (a - mu)^2 + sum w (b - mu)^2 = 2 n (V* + delta^2) exactly, because the deviations
#           from mu* add up to zero over A and B together. Terms are >= 0, so the rest is relative: chain n / 8 + 9, d rounds
#           once and enters squared 2, the weight's product 1, the division 1, the restatement 1: (n / 8 + 14) EPS <= g.
#           |V - V*| <= 2 g V* + d_mu^2   (one g of room for the second-order terms).
#   S1_p    C1 = sum w (b - mu)(c - a) / n moves by delta sum w (c - a) / n <= d_mu D1, D1 = sum w |c - a| / n; its terms carry
#           3 EPS (two differences, the weight's product), the chain n / 8 + 8, two divisions 2, the restatement 3, all times
#           T1 = sum w |b - mu*| |c - a| / n; V's relative error g + delta^2 / V* multiplies |S1*| <= T1 / V*:
#           (n / 4 + 30) EPS <= 2 g.   |S1 - S1*| <= (4 g T1 + d_mu D1) / V* + (T1 / V*) d_mu^2 / V*.
#   ST_p    no mu in the numerator, terms >= 0: chain n / 8 + 8, terms 3, two divisions, the restatement 3, V's g + delta^2 / V*:
#           |ST - ST*| <= ST* (4 g + d_mu^2 / V*).
# Where the rules give an exact 0.0 (n < 2, V* == 0, n == 0) or a NaN the gate is 0: compared exactly.
GATE_C = 4.0


def ref_sobol(u, M, P, w=None, species=None):
    """dict(first, total [L][n_sel][P], mean, var [L][n_sel], count) from the definition in extended arithmetic over the same
    doubles (mu first, deviations and products formed in long double: errors 2^-11 of the gates'), with the rules: zeros for
    n == 0, S1 = ST = 0.0 for n < 2 or V == 0, V == 0.0 for a column whose participating a and b are all equal, NaN by IEEE.
    gate_first, gate_total, gate_mean, gate_var: the bounds derived above."""
    idx, wt, n = _participants(M, w)
    x, (L, ns) = _columns(u, M, P, idx, species)
    shape1, shapeP = (L, ns), (L, ns, P)
    if n == 0:
        z1, zP = np.zeros(shape1), np.zeros(shapeP)
        return dict(first=zP, total=zP, mean=z1, var=z1, count=0, gate_first=zP, gate_total=zP, gate_mean=z1, gate_var=z1)
    with np.errstate(all="ignore"):
        x = x.astype(LD)
        ww, nl = wt.astype(LD)[:, None], LD(n)
        a, b, c = x[0], x[1], x[2:]
        mu = ((ww * a).sum(0) + (ww * b).sum(0)) / (2 * nl)
        V = ((ww * (a - mu) ** 2).sum(0) + (ww * (b - mu) ** 2).sum(0)) / (2 * nl)
        ab = np.concatenate([a, b])
        V = np.where((ab.max(0) - ab.min(0) == 0) & ~np.isnan(mu), LD(0), V)
        C1 = (ww * (b - mu) * (c - a)).sum(1) / nl
        C2 = (ww * (a - c) ** 2).sum(1) / (2 * nl)
        zero = (V == 0) | (n < 2)
        S1, ST = np.where(zero, LD(0), C1 / V), np.where(zero, LD(0), C2 / V)
        g = (n + 16) * EPS
        d_mu = g * ((ww * np.abs(a)).sum(0) + (ww * np.abs(b)).sum(0)) / (2 * nl)
        T1 = (ww * np.abs(b - mu) * np.abs(c - a)).sum(1) / nl
        D1 = (ww * np.abs(c - a)).sum(1) / nl
        g_first = (GATE_C * g * T1 + d_mu * D1) / V + (T1 / V) * d_mu ** 2 / V
        g_total = ST * (GATE_C * g + d_mu ** 2 / V)
        g_var = 2 * g * V + d_mu ** 2
        exact = zero | np.isnan(S1) | np.isnan(g_first)
        g_first, g_total = np.where(exact, 0, g_first), np.where(zero | np.isnan(ST) | np.isnan(g_total), 0, g_total)
        g_mean, g_var = np.where(np.isnan(mu), 0, d_mu), np.where(np.isnan(V), 0, g_var)
    f = lambda v, shape: np.ascontiguousarray(np.moveaxis(np.asarray(v, dtype=float), 0, -1)).reshape(shape) if v.ndim == 2 \
        else np.asarray(v, dtype=float).reshape(shape)
    return dict(first=f(S1, shapeP), total=f(ST, shapeP), mean=f(mu, shape1), var=f(V, shape1), count=n,
                gate_first=f(g_first, shapeP), gate_total=f(g_total, shapeP), gate_mean=f(g_mean, shape1), gate_var=f(g_var, shape1))


def fma(a, b, c):
    """a * b + c rounded once (float() of a Fraction rounds correctly)."""
    if a == 0.0 or b == 0.0:
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _ordered(part):
    t = part[0]
    for v in part[1:]:
        t = t + v
    return t


def replay_sobol(u, M, P, w=None, species=None, columns=None):
    """The order of member_stats.hpp operation by operation over the finite columns `columns` (indices into the L n_sel selected
    columns; None: all): dict(first, total [len(columns)][P], mean, var [len(columns)]). Python's float +, -, *, / are the
    correctly rounded IEEE operations and never fuse; the fused operations of the order are fma() above."""
    idx, wt, n = _participants(M, w)
    x, (L, ns) = _columns(u, M, P, idx, species)
    cols = np.arange(L * ns) if columns is None else np.asarray(columns, dtype=int)
    x = x[:, :, cols]
    assert n >= 1 and np.all(np.isfinite(x)), "the replay takes finite columns and n >= 1"
    W, dn, dn2 = SB_WAVES, float(n), 2.0 * float(n)
    wq = [float(v) for v in wt]
    out = dict(first=np.empty((len(cols), P)), total=np.empty((len(cols), P)), mean=np.empty(len(cols)), var=np.empty(len(cols)))
    for ci in range(len(cols)):
        a, b = x[0, :, ci].tolist(), x[1, :, ci].tolist()
        cs = [x[2 + p, :, ci].tolist() for p in range(P)]
        ta, tb = [0.0] * W, [0.0] * W
        for q in range(len(a)):
            ta[q % W] = ta[q % W] + wq[q] * a[q]
            tb[q % W] = tb[q % W] + wq[q] * b[q]
        mu = (_ordered(ta) + _ordered(tb)) / dn2
        flat = max(a + b) - min(a + b) == 0.0
        SA, SB = [0.0] * W, [0.0] * W
        C1, C2 = [[0.0] * W for _ in range(P)], [[0.0] * W for _ in range(P)]
        for q in range(len(a)):
            k = q % W
            da, db = a[q] - mu, b[q] - mu
            wda, wdb = wq[q] * da, wq[q] * db
            SA[k], SB[k] = fma(wda, da, SA[k]), fma(wdb, db, SB[k])
            for p in range(P):
                C1[p][k] = fma(wdb, cs[p][q] - a[q], C1[p][k])
                e = a[q] - cs[p][q]
                C2[p][k] = fma(wq[q] * e, e, C2[p][k])
        V = 0.0 if flat else (_ordered(SA) + _ordered(SB)) / dn2
        zero = n < 2 or V == 0.0
        out["mean"][ci], out["var"][ci] = mu, V
        for p in range(P):
            out["first"][ci, p] = 0.0 if zero else (_ordered(C1[p]) / dn) / V
            out["total"][ci, p] = 0.0 if zero else (_ordered(C2[p]) / dn2) / V
    return out


def finite_columns(u, M, P, w=None, species=None):
    """The selected columns (indices into L n_sel) whose participating values are all finite."""
    idx, _, _ = _participants(M, w)
    x, _ = _columns(u, M, P, idx, species)
    return np.flatnonzero(np.isfinite(x).all(axis=(0, 1)))


def within(got, ref, gate):
    """|got - ref| <= gate entry by entry; NaN only where ref is NaN, and there always."""
    got, ref, gate = np.asarray(got), np.asarray(ref), np.asarray(gate)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isnan(got) == nan) and np.all((np.abs(got - ref) <= gate) | nan))


def worst(got, ref, gate):
    """The largest |got - ref| / gate over the entries with a gate > 0, for an assertion's message."""
    got, ref, gate = np.asarray(got), np.asarray(ref), np.asarray(gate)
    with np.errstate(all="ignore"):
        r = np.where(gate > 0, np.abs(got - ref) / gate, np.where((got == ref) | (np.isnan(got) & np.isnan(ref)), 0.0, np.inf))
    at = np.unravel_index(np.argmax(r), r.shape)
    return f"worst |got - ref| / gate = {r[at]:.3g} at {tuple(int(i) for i in at)}: {got[at]!r} against {ref[at]!r}, gate {gate[at]:.3g}"


def same_bits_or_zero(a, b):
    """Equal bit for bit, zeros compared by value, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def ishigami(x, a=7.0, b=0.1):
    """The Ishigami function of x[..][3] on the unit cube scaled to [-pi, pi]^3."""
    z = np.pi * (2.0 * np.asarray(x) - 1.0)
    return np.sin(z[..., 0]) + a * np.sin(z[..., 1]) ** 2 + b * z[..., 2] ** 4 * np.sin(z[..., 0])


ISHIGAMI_S1 = (0.3139, 0.4424, 0.0)
ISHIGAMI_ST = (0.5576, 0.4424, 0.2437)
