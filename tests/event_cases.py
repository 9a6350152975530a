"""The event-time pass restated in NumPy, and the cases its tests run (no device here).

ref_events is the definition of include/kinetica_hip.h in plain loops over Python floats - IEEE doubles, every operation
rounded on its own, the chord in the documented order - so the device results are compared with it bit for bit.

The cases are built at the smallest shapes at which the kernel can go wrong: species counts at the edges of a 64-species
slice, segments shorter than, equal to and just longer than a part of PART_ROWS rows (the size the GPU tests force), segments
with 0, 1 and L rows, and columns for every situation the definition names."""
import itertools

import numpy as np

KINDS = ("abs", "of_peak", "of_start")
DIRECTIONS = ("rise", "fall")
STARTS = ("begin", "peak")
COMBOS = list(itertools.product(KINDS, DIRECTIONS, STARTS))
OUTPUTS = ("u_peak", "t_peak", "t_cross")
PART_ROWS = 4            # the part size C the GPU tests force (KIN_EVENT_PART_ROWS)
FORCED = dict(KIN_EVENT_PART_ROWS=str(PART_ROWS), KIN_EVENT_WAVES="2")      # 2C+1 rows: wavefront 0 walks parts 0 and 2


def ref_events(u, t, level, kind="abs", direction="rise", start="begin", row_begin=0, never=float("nan"), seg_n=None):
    """dict of u_peak, t_peak, t_cross [S][N] of u[S][L][N] with times t[L] or t[S][L]; level [N], a number, or None (no
    t_cross). Rows at or past seg_n[s] are never looked at."""
    u = np.asarray(u, dtype=float)
    S, L, N = u.shape
    t = np.asarray(t, dtype=float)
    lev = None if level is None else np.broadcast_to(np.asarray(level, dtype=float), (N,))
    out = {q: np.empty((S, N)) for q in OUTPUTS}
    for s in range(S):
        n = L if seg_n is None else int(seg_n[s])
        if row_begin >= n:
            out["u_peak"][s], out["t_peak"][s], out["t_cross"][s] = 0.0, never, never
            continue
        ts = (t[s] if t.ndim == 2 else t)[:n].tolist()
        for i in range(N):
            col = u[s, :n, i].tolist()
            peak, jp = col[row_begin], row_begin
            for j in range(row_begin + 1, n):
                if col[j] > peak:
                    peak, jp = col[j], j
            out["u_peak"][s, i], out["t_peak"][s, i] = peak, ts[jp]
            if lev is None:
                out["t_cross"][s, i] = never
                continue
            l = float(lev[i])
            if kind == "of_peak":
                l = l * peak
            elif kind == "of_start":
                l = l * col[row_begin]
            j0 = row_begin if start == "begin" else jp
            jc = None
            for j in range(j0, n):
                if (col[j] >= l) if direction == "rise" else (col[j] <= l):
                    jc = j
                    break
            if jc is None:
                tc = never
            elif jc == j0:
                tc = ts[j0]
            else:
                a, b = col[jc - 1], col[jc]
                tc = ts[jc - 1] + ((l - a) / (b - a)) * (ts[jc] - ts[jc - 1])
            out["t_cross"][s, i] = tc
    if lev is None:
        del out["t_cross"]
    return out


def same_bits(a, b):
    """a and b agree bit for bit; NaN (a `never`) only has to sit in the same places."""
    a, b = np.ascontiguousarray(a, dtype=float), np.ascontiguousarray(b, dtype=float)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)))


# ---- generated blocks: every kind of column at every shape ---------------------------------------------------------------
COLUMN_KINDS = 8      # species i holds a column of kind i % 8


def _column(kind, L, rng):
    v = rng.random(L) + 0.0625
    if kind == 1:
        v = np.sort(v)                                 # rising
    elif kind == 2:
        v = np.sort(v)[::-1]                           # falling
    elif kind == 3 and L >= 2:                         # a plateau at the peak: two rows hold it, the first wins
        a, b = sorted(rng.choice(L, 2, replace=False))
        v[a] = v[b] = 2.0
    elif kind == 4:
        v = np.zeros(L)                                # of_peak: l = 0, rising gives t[j0]
    elif kind == 5:
        v = (v - 0.5) * 1e-12                          # small values of both signs
    elif kind == 6:
        v = np.sort(v); v[-1] = 4.0                    # the peak at the last row
    elif kind == 7:
        v = np.full(L, 0.75)                           # every sample equals every other
    return v * (1.0 if kind in (4, 7) else 10.0 ** int(rng.integers(-6, 3)))


def make_block(S, L, N, seed):
    """(u[S][L][N], t[L], t_per[S][L], seg_n[S]): segments of L, 0, 1 and about L / 2 rows (then L again); the rows past a
    segment's own are NaN and 1e300, and its own times past them NaN."""
    rng = np.random.default_rng(seed)
    u = np.empty((S, L, N))
    for s in range(S):
        for i in range(N):
            u[s, :, i] = _column(i % COLUMN_KINDS, L, rng)
    t = np.cumsum(rng.random(L) + 0.125) - 0.5
    t_per = np.stack([np.cumsum(rng.random(L) + 0.125) * (s + 1) for s in range(S)])
    seg_n = np.array([(L, 0, min(1, L), (L + 1) // 2)[s % 4] if s < 4 else L for s in range(S)], dtype=np.int64)
    for s in range(S):
        n = int(seg_n[s])
        u[s, n:, 0::2], u[s, n:, 1::2] = np.nan, 1e300
        t_per[s, n:] = np.nan
    return u, t, t_per, seg_n


def make_levels(u, seg_n):
    """level[N] per kind. abs: by species i % 4 a sample of segment 0 bit for bit, the midpoint of segment 0's range, a level
    above everything (never met rising, met at j0 falling), one below everything. Relative kinds: fractions around 1."""
    S, L, N = u.shape
    n0 = max(int(seg_n[0]), 1)
    col = u[0, :n0]
    absolute = np.empty(N)
    for i in range(N):
        absolute[i] = (col[n0 // 2, i], 0.5 * (col[:, i].min() + col[:, i].max()), 1e300, -1e300)[i % 4]
    frac = np.array([0.5, 1.0, 0.1, 2.0, 0.0, 0.999, -1.0])[np.arange(N) % 7]
    return dict(abs=absolute, of_peak=frac, of_start=frac)


def _generated(S, L, N, seed, row_begins, per_segment=False, never=float("nan")):
    u, t, t_per, seg_n = make_block(S, L, N, seed)
    return dict(id=f"S{S}-L{L}-N{N}" + ("-tper" if per_segment else "") + ("" if np.isnan(never) else "-censor"), u=u,
                t=t_per if per_segment else t, seg_n=seg_n, levels=make_levels(u, seg_n), row_begins=row_begins, never=never)


C = PART_ROWS
CASES = [
    _generated(4, 1, 1, 1, (0, 1)),
    _generated(4, 2, 63, 2, (0, 1, 2)),
    _generated(4, 3, 64, 3, (0, 1, 2, 3), per_segment=True),
    _generated(4, C - 1, 65, 4, (0, C - 2)),
    _generated(4, C, 257, 5, (0, 1, C - 1, C)),
    _generated(5, C + 1, 65, 6, (0, 1, C), per_segment=True),
    _generated(5, 2 * C + 1, 64, 7, (0, 1, C, 2 * C, 2 * C + 1)),
    _generated(4, 2 * C + 1, 257, 8, (0, C - 1), never=-1.0),
    _generated(2, 37, 130, 9, (0, 5), per_segment=True),
]


def _hand_built():
    """One segment, one idea per column, at L = 2C + 1 rows with parts of C: the interval (C - 1, C) spans two parts."""
    L = 2 * C + 1
    j = np.arange(L, dtype=float)
    t = 0.5 * j + 0.25
    ramp = j.copy()                                   # 0, 1, .., 8
    tri = np.minimum(j, (L - 1) - j) * 0.25           # a triangle pulse, peak 1.0 at row C
    cols = [
        (ramp, C - 0.5),        # rising crossing inside (C - 1, C): the row before the crossing is another part's last
        (ramp, 2 * C - 0.75),   # ... and inside (2C - 1, 2C)
        (ramp, float(C)),       # a level equal to a sample bit for bit
        (ramp, -1.0),           # already met at j0
        (ramp, 100.0),          # never met
        (tri, 0.375),           # both flanks of a pulse
        (np.where((j == 2) | (j == 6), 3.0, 1.0), 2.0),      # a plateau of the peak over two parts: row 2 wins
        (np.zeros(L), 0.0),     # all zero
        (-1e-15 * (1.0 + j), -4.5e-15),                      # small negative values, falling
        (ramp, 1.0),            # the peak at the last row: from the peak, falling, of_peak level 1.0 gives t[L - 1]
    ]
    u = np.stack([c for c, _ in cols], axis=1)[None]
    level = np.array([l for _, l in cols])
    frac = np.array([0.5, 0.9, 1.0, 0.0, 2.0, 0.375, 0.5, 0.5, 2.0, 1.0])
    return dict(id="hand-built", u=u, t=t, seg_n=None, levels=dict(abs=level, of_peak=frac, of_start=frac), row_begins=(0, 1, C),
                never=float("nan"))


CASES.append(_hand_built())
