"""Seeded edge cases of the cross-member statistics, read-only and cached like member_stats_cases.block: participant lists that
leave out the first and last member, every participant count at which a kernel of member_stats_kernels.hip changes its path,
special values by participant POSITION, columns whose statistics are exact integers, constant columns whose mean rounds, offset
columns (a large mean over a small spread), inputs of 1 to 33 columns and probability vectors of 1 to 70 entries.
test_member_stats_edge_cases.py proves on the CPU that the cases are what they claim; test_gpu_member_stats_edges.py runs them."""
import functools
import math

import numpy as np

import member_stats_cases as mc
import member_stats_order as mo

EPS = mc.EPS

# every n in 1 .. 40 (the moments' unrolled loop runs for q + 24 < n: 24 | 25 and 32 | 33 are its edges; 32 | 33 the value pass's
# lanes; P2 = 2 .. 64 of the sorted pass) and the edges of the 64-participant tile of the product and of P2 = 64 .. 512
SMALL_NS = tuple(range(1, 41)) + (63, 64, 65, 255, 256, 257)
# the sorted pass's padded sizes 512 .. 4 096 from both sides, and the step from the 8-column tile to the 4-column one
SORTED_NS = (511, 512, 513, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
POSITIONS = (0, 1, 7, 8, -1)                     # participant positions of a special value (-1: the last, n - 1)
KINDS = ("nan", "+inf", "-inf", "both")          # "both": +Inf at the position, -Inf at the next participant (cyclically)
# species of the mixed block
SP_EXACT, SP_OFFSET, SP_FIRST_RANDOM = 0, 1, 2
OFFSET_RATIOS = (1e3, 1e2, 1e1)                  # c / s of the offset column in row 0, 1, 2
WIDE_SPECIES = (0, 1, 2, 3, 4, 63, 64, 65, 69)   # the correlation columns of a 70-species block (an 8-column tile and a ragged one)
CONSTANT_CASES = ((3, 0.1), (6, 0.1), (3, 0.7))  # (n, value): the mean of n such values is not the value
INPUT_PS = (1, 15, 16, 17, 33)
QS = (1, 32, 33, 70)

_BIG = {63: (5, 3, 33), 64: (5, 1, 16), 65: (70, 2, 17), 255: (5, 2, 15), 256: (5, 3, 1), 257: (70, 1, 17)}


def shape(n):
    """(N, L, P) of the mixed case of n participants: 70 species at the path edges, 1 to 3 rows, the five input counts in turn."""
    if n in _BIG:
        return _BIG[n]
    if n in SORTED_NS:
        return 5, 2, 1 + (n % 2)
    return (70 if n in (1, 8, 9, 24, 25, 32, 33, 40) else 5), 1 + n % 3, INPUT_PS[n % 5]


@functools.lru_cache(maxsize=None)
def mask(n):
    """use[K] of K = n + 5 members selecting n of them; for odd n neither member 0 nor member K - 1 takes part, for even n
    both do. The values are any non-zero int32."""
    K = n + 5
    rng = np.random.default_rng([11, n])
    use = np.zeros(K, np.int32)
    if n % 2:
        pick = 1 + rng.permutation(K - 2)[:n]
    else:
        pick = np.r_[0, K - 1, 1 + rng.permutation(K - 2)[:n - 2]]
    use[pick] = rng.integers(1, 9, len(pick)) * rng.choice([-1, 1], len(pick))
    use.setflags(write=False)
    assert int((use != 0).sum()) == n
    return use


def _random(rng, shape):
    """The mixture of member_stats_cases.block: log-uniform over 30 decades with signs, zeros of both signs."""
    u = rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-15, 15, shape)
    u[rng.random(shape) < 0.4] = 0.0
    u[rng.random(shape) < 0.05] = -0.0
    return u


def _exact_column(rng, n):
    """n integers in [-2000, 2000] whose sum is a multiple of n (mean, deviations and their squares are then exact)."""
    v = rng.integers(-1000, 1001, n)
    v[-1] -= int(v.sum()) % n      # (at most n - 1 <= 4 095 below -1000 ... the squares stay far below 2^53)
    assert int(v.sum()) % n == 0
    return v.astype(float)


def _unit(rng, n):
    """n normal draws shifted and scaled to mean 0 and mean square 1 (n = 1: 0.0), so that c + s z has spread s."""
    z = rng.standard_normal(n)
    z = z - z.mean()
    r = math.sqrt(float(np.mean(z * z))) if n > 1 else 0.0
    return z / r if r > 0.0 else z


@functools.lru_cache(maxsize=None)
def mixed_block(n):
    """u[K = n + 5][L][N] of shape(n): species 0 an exact-integer column, species 1 the offset column 1 + s z with
    1 / s = OFFSET_RATIOS[row], the others the random mixture. All finite. Only the participants' entries follow the column
    rules; the other members hold the random mixture, so a kernel that read them would be seen. Read-only."""
    N, L, _ = shape(n)
    K, idx = n + 5, mc.participants(n + 5, mask(n))
    rng = np.random.default_rng([12, n])
    u = _random(rng, (K, L, N))
    for j in range(L):
        u[idx, j, SP_EXACT] = _exact_column(rng, n)
        u[idx, j, SP_OFFSET] = 1.0 + _unit(rng, n) / OFFSET_RATIOS[j]
    u.setflags(write=False)
    return u


def special_columns():
    """[(species, kind, position)] of special_block: one column per kind and position."""
    return [(len(KINDS) * a + b, kind, pos) for a, pos in enumerate(POSITIONS) for b, kind in enumerate(KINDS)]


@functools.lru_cache(maxsize=None)
def special_block(n):
    """u[K = n + 5][1][70]: species 4 a + b holds kind KINDS[b] at participant position POSITIONS[a] where that position exists
    (and, for "both", n >= 2); the rest of the block is the random mixture. Read-only."""
    K, idx = n + 5, mc.participants(n + 5, mask(n))
    u = _random(np.random.default_rng([13, n]), (K, 1, 70))
    for sp, kind, pos in special_columns():
        q = special_position(n, pos)
        if q is None or (kind == "both" and n < 2):
            continue
        u[idx[q], 0, sp] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "both": np.inf}[kind]
        if kind == "both":
            u[idx[(q + 1) % n], 0, sp] = -np.inf
    u.setflags(write=False)
    return u


def special_position(n, pos):
    """The participant position a POSITIONS entry means at n participants, None where it does not exist."""
    q = n - 1 if pos < 0 else pos
    return q if q < n else None


@functools.lru_cache(maxsize=None)
def constant_block(n, value):
    """u[n + 5][1][5] whose species 1 is `value` at every participant (other members differ), the rest the random mixture."""
    K, idx = n + 5, mc.participants(n + 5, mask(n))
    u = _random(np.random.default_rng([14, n]), (K, 1, 5))
    u[:, 0, 1] = -value
    u[idx, 0, 1] = value
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def sorted_block(n):
    """u[n + 5][2][5] of a sorted size: the mixed block's columns, and in species 3 a +Inf and a -Inf (row 0) and in species 2 a
    NaN (row 1) among the participants. Species 4, 0 and 1 stay finite."""
    idx = mc.participants(n + 5, mask(n))
    u = mixed_block(n).copy()
    u[idx[n // 3], 0, 3] = np.inf
    u[idx[n - 1], 0, 3] = -np.inf
    u[idx[n // 2], 1, 2] = np.nan
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def inputs(n, P):
    """X[K = n + 5][P]: in turn normal draws, a heavily tied column (four levels) and a monotone function of normal draws with
    noise; for P > 1 the last column is constant. Read-only."""
    K = n + 5
    rng = np.random.default_rng([15, n, P])
    cols = []
    for p in range(P):
        z = rng.standard_normal(K)
        cols.append([z, rng.integers(0, 4, K).astype(float), np.exp(z) + 0.1 * rng.standard_normal(K)][p % 3])
    if P > 1:
        cols[-1] = np.full(K, 2.5)
    X = np.stack(cols, axis=1)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def probabilities(n, Q):
    """p[Q] for n participants. Q >= 32: 0, 1, 1/3, 2/3, the k / (n - 1) (whose (n - 1) p lands on or next to an integer) and
    uniform draws, shuffled. Q = 1 has room for one value: probabilities(n, 1) is 1/3, and the callers add [0] and [1]."""
    if Q == 1:
        return np.array([1.0 / 3.0])
    rng = np.random.default_rng([16, n, Q])
    fixed = [0.0, 1.0, 1.0 / 3.0, 2.0 / 3.0]
    if n > 1:
        fixed += [k / (n - 1) for k in rng.choice(np.arange(1, n), min(n - 1, (Q - 4) // 2), replace=False)]
    p = np.array(fixed + list(rng.random(Q - len(fixed))))
    rng.shuffle(p)
    p.setflags(write=False)
    assert len(p) == Q and p.min() == 0.0 and p.max() == 1.0
    return p


def probability_vectors(n):
    return [np.array([0.0]), np.array([1.0])] + [probabilities(n, Q) for Q in QS]


def sorted_layout(n):
    """(P2, T) of the sorted pass at n participants. Restated from the library (member_stats_api.cpp, ms_sorted_tile): P2 is the
    power of two >= max(n, 2); T = 8 columns per workgroup, halved while T (P2 + 2) 8 B exceeds the 132 KiB of dynamic LDS."""
    P2 = 2
    while P2 < n:
        P2 *= 2
    T = 8
    while T > 1 and T * (P2 + 2) * 8 > 132 * 1024:
        T //= 2
    return P2, T


def correlation_species(n, rank):
    """The species list of the mixed case's correlation call (None: all 5)."""
    return list(WIDE_SPECIES) if shape(n)[0] == 70 else None


# --- expectations shared by the CPU and the GPU file (computed once per process) --------------------------------------------

def columns_of(u, use, species=None):
    """x[n][L n_sel]: the participants' values, column c = j n_sel + s as the column passes number them."""
    K, L, N = u.shape
    sp = np.arange(N) if species is None else np.asarray(species, dtype=int)
    idx = mc.participants(K, use)
    return u[idx][:, :, sp].reshape(len(idx), L * len(sp))


@functools.lru_cache(maxsize=None)
def expected_moments(n):
    """(mean[L][N], var[L][N]) of the mixed block in the documented order."""
    u = mixed_block(n)
    mean, var = mo.replay_moments(columns_of(u, mask(n)))
    return mean.reshape(u.shape[1:]), var.reshape(u.shape[1:])


def exact_moments(n):
    """(mean[L], var[L]) of the exact column of the mixed block from Python integers: the mean is an integer, the variance one
    correctly rounded quotient of two integers."""
    u = mixed_block(n)
    idx = mc.participants(n + 5, mask(n))
    mean, var = [], []
    for j in range(u.shape[1]):
        v = [int(x) for x in u[idx, j, SP_EXACT]]
        assert sum(v) % n == 0
        m = sum(v) // n
        S = sum((x - m) ** 2 for x in v)
        mean.append(float(m))
        var.append(S / (n - 1) if n > 1 else float(S))
    return np.array(mean), np.array(var)


@functools.lru_cache(maxsize=None)
def expected_correlation(n, rank, block="mixed", species=None):
    """(r[L][n_sel][P] in the documented order with NaN where the replay does not apply (a column that is not finite), the
    columns' mask of where it applies [L][n_sel], ref r, gate) of a case's correlation call."""
    from kinetica_jl_amd import capi
    u = {"mixed": mixed_block, "sorted": sorted_block}[block](n)
    _, L, P = shape(n)
    sp = correlation_species(n, rank) if species is None else list(species)
    X, use = inputs(n, P), mask(n)
    y = columns_of(u, use, sp)
    ok = np.all(np.isfinite(y), axis=0)
    nx, xhat = capi.members_inputs(X, use=use, rank=rank)
    assert nx == n
    r = np.full((y.shape[1], P), np.nan)
    if ok.any():
        yhat = mo.replay_ranks(y[:, ok]) if rank else mo.replay_values(y[:, ok])
        r[ok] = mo.replay_corr(xhat, yhat)
    ref, gate = mc.ref_correlate(u, X, sp, rank, use)
    return r.reshape(ref.shape), ok.reshape(ref.shape[:2]), ref, gate
