"""The resampling pass restated in plain Python, and the cases its tests run (no device here).

ref_resample is the definition of include/kinetica_hip.h in plain loops over Python floats - IEEE doubles, every operation
rounded on its own, the bracket found by walking the rows, the chord in the documented order - so the device results are
compared with it bit for bit.

The cases are built at the smallest shapes at which the kernel can go wrong: species counts at the edges of a 64-species wave
row, query counts below, at and above the tile of TILE queries the GPU tests force (so that a workgroup holds a partial tile and
a wavefront takes several queries), segments of L, 0, 1 and about L / 2 rows with poison behind them, and a query for every
situation the definition names. SLICE_CASES reach the second and third species slice of a workgroup's 1024, PLAN_CASE with
PLANS the tiles and wavefront counts the launcher chooses for large calls."""
import numpy as np

from event_cases import same_bits  # noqa: F401  (the comparison the resampling tests use as well)

MODES = ("fill", "hold")
BELOW, ABOVE, NONE = -1, -2, -3
TILE = 4                 # the tile the GPU tests force (KIN_RESAMPLE_TILE_QUERIES)
FORCED = dict(KIN_RESAMPLE_TILE_QUERIES=str(TILE), KIN_RESAMPLE_WAVES="2")      # 9 queries: tiles of 4, 4 and 1, two per wavefront
# what a call is asked with besides its row_begin: both modes, fill NaN and a finite fill
REQUESTS = [dict(mode="fill", fill=float("nan")), dict(mode="fill", fill=-7.5), dict(mode="hold", fill=float("nan")),
            dict(mode="hold", fill=0.125)]


def ref_bracket(xs, row_begin, n, v):
    """(jc, w) of the query v on the axis rows xs[row_begin .. n - 1] (a list of Python floats)."""
    if n <= row_begin or v != v:
        return NONE, 0.0
    if v < xs[row_begin]:
        return BELOW, 0.0
    if v > xs[n - 1]:
        return ABOVE, 0.0
    jc = next(j for j in range(row_begin, n) if xs[j] >= v)
    if xs[jc] == v:
        return jc, 0.0
    return jc, (v - xs[jc - 1]) / (xs[jc] - xs[jc - 1])


def ref_resample(u, x, xq, seg_n=None, mode="fill", fill=float("nan"), row_begin=0):
    """(u_q[S][Q][N], jc[S][Q] int32, w[S][Q]) of u[S][L][N] with the axis x[L] or x[S][L] and the queries xq[Q] or xq[S][Q].
    Rows at or past seg_n[s] are never looked at."""
    u = np.asarray(u, dtype=float)
    S, L, N = u.shape
    x, xq = np.asarray(x, dtype=float), np.asarray(xq, dtype=float)
    Q = xq.shape[-1]
    out, jcs, ws = np.empty((S, Q, N)), np.empty((S, Q), np.int32), np.empty((S, Q))
    for s in range(S):
        n = L if seg_n is None else int(seg_n[s])
        xs = (x[s] if x.ndim == 2 else x)[:n].tolist()
        rows = u[s, :n].tolist()
        for q, v in enumerate((xq[s] if xq.ndim == 2 else xq).tolist()):
            jc, w = ref_bracket(xs, row_begin, n, v)
            jcs[s, q], ws[s, q] = jc, w
            if jc >= 0 and xs[jc] == v:
                row = rows[jc]
            elif jc >= 0:
                row = [a + w * (b - a) for a, b in zip(rows[jc - 1], rows[jc])]
            elif mode == "hold" and jc != NONE:
                row = rows[row_begin] if jc == BELOW else rows[n - 1]
            else:
                row = [fill] * N
            out[s, q] = row
    return out, jcs, ws


def covered_run(jc, mode):
    """n_saved' of a stored resampled record: per segment the length of the leading run of covered queries of jc[S][Q]."""
    cov = (jc >= 0) | ((jc != NONE) if mode == "hold" else False)
    return np.array([len(c) if c.all() else int(np.argmin(c)) for c in cov], dtype=np.int64)


# ---- generated blocks: every kind of column at every shape ---------------------------------------------------------------
COLUMN_KINDS = 8      # species i holds a column of kind i % 8


def _column(kind, L, rng):
    v = rng.random(L) + 0.0625
    if kind == 0:
        return (v - 0.5) * 1e-12                          # small values of both signs
    if kind == 1:
        return np.full(L, -0.0)                           # a copy keeps the sign of zero
    if kind == 2:
        return rng.integers(0, 9, L) * 5e-324             # subnormals
    if kind == 3:
        return np.full(L, 0.75)                           # every sample equals every other
    if kind == 5:
        v[int(rng.integers(0, L))] = np.inf               # an Inf in a bracketing row
        return v
    if kind == 6:
        return np.sort(v)
    if kind == 7:
        return -v * 1e3
    return v * 10.0 ** int(rng.integers(-6, 3))


def _axis(L, rng):
    """A non-decreasing axis with a plateau inside (L >= 4) and the last two rows equal (L >= 3): a ramp that holds."""
    x = np.cumsum(rng.random(L) + 0.125) + 900.0
    if L >= 4:
        x[L // 2] = x[L // 2 - 1]
    if L >= 3:
        x[-1] = x[-2]
    return x


def _queries(x, n, Q, offset):
    """Q queries from the pool of every situation on the axis rows x[:n] (n >= 1), unsorted, starting at `offset`."""
    lo, hi = x[0], x[n - 1]
    rising = [j for j in range(1, n) if x[j] > x[j - 1]]
    between = [0.5 * (x[j - 1] + x[j]) for j in rising] or [lo]
    plateau = x[(n // 2 - 1) if n >= 4 else n - 1]
    pool = [between[len(between) // 2], lo - 1.0, lo, x[n // 2], hi, hi + 1.0, np.inf, np.nan, plateau, -np.inf,
            between[len(between) // 2], between[0] if len(between) < 2 else 0.25 * x[rising[0] - 1] + 0.75 * x[rising[0]]]
    return np.array([pool[(offset + q) % len(pool)] for q in range(Q)])


PAYLOADS = np.array([0x7FF8000000001234, 0xFFF80000DEADBEEF], dtype=np.uint64).view(np.float64)      # NaNs a copy has to keep


def make_case(S, L, N, Q, seed, x_per=False, q_per=False, offset=0, seg_rows=None, row_begins=None, payloads=False):
    """Segments of L, 0, 1 and about L / 2 rows (then L again), or of seg_rows; the states past a segment's own rows are NaN and
    1e300, and its own axis past them NaN. payloads: the species i % 64 == 12 hold NaNs with a payload in every third row."""
    rng = np.random.default_rng(seed)
    u = np.empty((S, L, N))
    for s in range(S):
        for i in range(N):
            u[s, :, i] = _column(i % COLUMN_KINDS, L, rng)
    if payloads:
        for k, j in enumerate(range(0, L, 3)):
            u[:, j, 12::64] = PAYLOADS[k % 2]
    seg_n = np.array([(L, 0, min(1, L), (L + 1) // 2)[s % 4] if s < 4 else L for s in range(S)] if seg_rows is None else seg_rows,
                     dtype=np.int64)
    x = np.stack([_axis(L, rng) + 0.375 * s for s in range(S)]) if x_per else _axis(L, rng)
    xq = np.stack([_queries(x[s] if x_per else x, max(int(seg_n[s]), 1), Q, offset + s) for s in range(S)]) if q_per \
        else _queries(x[0] if x_per else x, L, Q, offset)
    for s in range(S):
        n = int(seg_n[s])
        u[s, n:, 0::2], u[s, n:, 1::2] = np.nan, 1e300
        if x_per:
            x[s, n:] = np.nan
    half = (L + 1) // 2
    if row_begins is None:
        row_begins = tuple(sorted({0, 1, max(half - 1, 0), half, max(L - 1, 0), L}))
    name = f"S{S}-L{L}-N{N}-Q{Q}" + ("-xper" if x_per else "") + ("-qper" if q_per else "")
    return dict(id=name, u=u, x=x, xq=xq, seg_n=seg_n, row_begins=row_begins)


CASES = [
    make_case(4, 1, 1, 1, 1, offset=2),
    make_case(4, 2, 63, 3, 2),
    make_case(4, 3, 64, 4, 3, x_per=True, offset=1),
    make_case(5, 9, 65, 5, 4, x_per=True, q_per=True),
    make_case(4, 9, 257, 9, 5),
    make_case(5, 37, 64, 9, 6, x_per=True, q_per=True, offset=3),
    make_case(4, 37, 1, 0, 7),
    make_case(4, 3, 65, 9, 8, q_per=True, offset=3),
    make_case(2, 37, 257, 5, 9, x_per=True, offset=7),
]

# More than one species slice of SLICE species (blockIdx.y of the kernel): exactly one slice, a second slice of one species, of a
# wave row and one species, and a third slice of one species. Segments of L and about L / 2 rows; three row_begins - every
# row, one row of the short segment, none of it - keep the plain-Python restatement short. -0.0 (kind 1), subnormals (kind 2)
# and NaN payloads sit on every slice: a copied row keeps them.
SLICE = 1024
_SLICED = dict(seg_rows=(9, 5), row_begins=(0, 4, 5), payloads=True)
SLICE_CASES = [
    make_case(2, 9, SLICE, 5, 21, q_per=True, offset=2, **_SLICED),
    make_case(2, 9, SLICE + 1, 5, 22, x_per=True, q_per=True, **_SLICED),
    make_case(2, 9, SLICE + 64 + 1, 5, 23, x_per=True, offset=8, **_SLICED),
    make_case(2, 9, 2 * SLICE + 1, 5, 24, offset=1, **_SLICED),
]

# One case for the launcher's plans: 70 queries of 65 species over axes of 37, 19 and 1 rows. PLANS are (tile, wavefronts) pairs:
# every tile resample_plan chooses (8, 16, 32 - 4 is FORCED's), one query per workgroup, a tile that is no power of two, and
# the largest tile on one wavefront - 64 threads search 70 queries: the search loop's second trip - and on sixteen. A tile of
# 32 leaves a last tile of 6 queries and gives each of 4 wavefronts 8 queries.
PLAN_CASE = make_case(3, 37, 65, 70, 25, x_per=True, q_per=True, offset=5, seg_rows=(37, 19, 1), row_begins=(0, 18, 36), payloads=True)
PLANS = [(1, 1), (8, 4), (16, 4), (32, 4), (33, 3), (256, 1), (256, 16)]
GPU_CASES = CASES + SLICE_CASES + [PLAN_CASE]      # what the GPU tests run under FORCED and the launcher's own plan
