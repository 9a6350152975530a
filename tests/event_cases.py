"""The event-time pass restated in NumPy, and the cases its tests run (no device here).

ref_events is the definition of include/kinetica_hip.h in plain loops over Python floats - IEEE doubles, every operation
rounded on its own, the chord in the documented order - so the device results are compared with it bit for bit.

The cases are built at the smallest shapes at which the kernel can go wrong: species counts at the edges of a 64-species
slice, segments shorter than, equal to and just longer than a part of PART_ROWS rows (the size the GPU tests force), segments
with 0, 1 and L rows, and columns for every situation the definition names. Three more cases are built by hand for what the
generated columns reach only by chance: NaN rows inside a segment (the header's fmax rule), zeros of both signs, and peaks
late enough that the second walk skips whole parts (LATE_PEAK).

replay_events is the kernel's decomposition in NumPy - parts of C rows dealt to W wavefronts, the part skipping of the second
walk, the two combines - and reports how many parts the second walk skipped and walked: tests/test_event_cases.py asserts with
it, without a device, that the cases reach the paths they are named after, and that the decomposition does not change a
result. KNOBS is the matrix of launcher settings the GPU tests run the longest cases under."""
import itertools

import numpy as np

KINDS = ("abs", "of_peak", "of_start")
DIRECTIONS = ("rise", "fall")
STARTS = ("begin", "peak")
COMBOS = list(itertools.product(KINDS, DIRECTIONS, STARTS))
OUTPUTS = ("u_peak", "t_peak", "t_cross")
PART_ROWS = 4            # the part size C the GPU tests force (KIN_EVENT_PART_ROWS)
FORCED = dict(KIN_EVENT_PART_ROWS=str(PART_ROWS), KIN_EVENT_WAVES="2")      # 2C+1 rows: wavefront 0 walks parts 0 and 2
LANES = 64               # species of a workgroup (EVENT_LANES)
ROWS_IN_FLIGHT = 4       # EVENT_ROWS_IN_FLIGHT: the launcher's own part sizes are multiples of it
# every wavefront count the launcher chooses (4, 8, 16) and one wavefront alone, with parts of 1 row, of sizes that are no
# multiple of the rows in flight (3, 5, 6: the guarded tail of an in-flight group inside a segment) and of the launcher's own
# size (unset); and the setting every case is run under
KNOBS = [FORCED] + [dict(KIN_EVENT_WAVES=str(w), **({} if c is None else dict(KIN_EVENT_PART_ROWS=str(c))))
                    for w in (1, 4, 8, 16) for c in (1, 3, 5, 6, None)]


def knob_plan(knobs, L, default_waves=16):
    """(waves, part_rows) of a launch over segments of L rows under these settings, by the rule of event_plan (at the sizes of
    these cases the launcher's own choice is 16 wavefronts)."""
    W = int(knobs.get("KIN_EVENT_WAVES", default_waves))
    rows = max(ROWS_IN_FLIGHT, -(-(-(-max(L, 1) // W)) // ROWS_IN_FLIGHT) * ROWS_IN_FLIGHT)
    if "KIN_EVENT_PART_ROWS" in knobs:
        rows = min(rows, int(knobs["KIN_EVENT_PART_ROWS"]))
    return W, rows


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
            peak, jp = col[row_begin], row_begin      # the header's fmax chain: a NaN row is passed over, NaN only if every row is
            for j in range(row_begin + 1, n):
                if col[j] > peak or (peak != peak and col[j] == col[j]):
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


def _nan_rows():
    """L = 2C + 1 rows; under FORCED part 0 (rows 0 .. C - 1) and part 2 (row 2C) are wavefront 0's, part 1 wavefront 1's. Every
    third column holds NaN rows - `nan_cols`: only u_peak is specified there - the others stay as generated."""
    L, N = 2 * C + 1, 30
    u, t, _, seg_n = make_block(1, L, N, 11)
    levels = make_levels(u, seg_n)
    j = np.arange(L)
    ramp = 1.0 + np.minimum(j, 2 * (C + 1) - j)       # the peak at row C + 1
    rows = [
        [0],                                          # at row_begin 0
        [1],                                          # at row_begin 1
        [C],                                          # the peak's neighbour before it ...
        [C + 2],                                      # ... and after it
        list(range(C, 2 * C)),                        # the whole of part 1: everything wavefront 1 sees
        list(range(C)) + [2 * C],                     # parts 0 and 2: everything wavefront 0 sees
        list(range(C + 1, L)),                        # the parts from row 1 on: with row_begin 1, everything wavefront 1 sees
        list(range(L)),                               # every row
        list(range(1, L)),                            # every row but the first
        list(range(L - 1)),                           # every row but the last
    ]
    nan_cols = [3 * k + 1 for k in range(len(rows))]
    for col, rr in zip(nan_cols, rows):
        u[0, :, col] = ramp * (1.0 + col)
        u[0, rr, col] = np.nan
    return dict(id="nan-rows", u=u, t=t, seg_n=seg_n, levels=levels, row_begins=(0, 1), never=float("nan"), nan_cols=nan_cols)


def _signed_zeros():
    """Zeros of both signs: the peak is 0.0 by value, first held by the first row, whatever the decomposition. (`zeros`: u_peak
    is compared with the restatement by value - its `>` chain keeps the first row's sign, an fmax that orders the zeros gives
    +0.0 - and byte for byte between the decompositions.)"""
    L = 2 * C + 1
    u = np.full((1, L, 6), -0.0)
    u[0, 1, 0] = 0.0                                  # -0, +0, -0 ...
    u[0, 0, 1] = 0.0                                  # +0, -0, -0 ...
    u[0, L - 1, 2] = 0.0                              # -0 everywhere but one +0 in the last part
    u[0, :, 3] = 0.0                                  # +0 everywhere
    u[0, C, 5] = 0.0                                  # (column 4: -0 everywhere) one +0 at the first row of part 1
    t = 0.25 * np.arange(L) + 0.125
    lev = np.array([0.0, -0.0, 0.5, 1.0, 2.0, -1.0])
    return dict(id="signed-zeros", u=u, t=t, seg_n=None, levels=dict(abs=lev * 0.0, of_peak=lev, of_start=lev), row_begins=(0, 1),
                never=float("nan"), zeros=True)


def _late_peak():
    """S = 2, N = 65, L = 4C + 1. Species 0 .. 63 peak (1.0) at rows 2C .. 3C - 1, the earliest exactly at 2C: from the peak, the
    second walk of two wavefronts skips parts 0 and 1 of the first species group. Species 64, alone in the second group, falls from
    its first row: nothing is skipped there. Before its peak a column is the ramp (j + 1) / 32, after it 0.75 down to the row `fr`
    and 0.25 from there on; with the level of its kind (species i % 7) the crossing lands, from the peak and falling,
      0 at j0 itself (level 1.0), 1 at j0 + 1, 2 at the first row of part 3, 3 at row L - 1, 4 nowhere,
    and from the beginning and rising (abs and of_peak are the same level: the peak is 1.0)
      5 at the last row of part 1 (row 2C - 1), 6 at the first row of part 2 (row 2C).
    Segment 1 has 3C + 1 rows (poison behind them): its row L - 1 is not there."""
    L, N = 4 * C + 1, 65
    j = np.arange(L)
    u = np.empty((2, L, N))
    level = np.empty(N)
    for i in range(N - 1):
        pk = 2 * C + (i // 7) % C
        fr = (L, pk + 1, 3 * C, L - 1, L, L, L)[i % 7]
        u[:, :, i] = np.where(j < pk, (j + 1) / 32.0, np.where(j == pk, 1.0, np.where(j < fr, 0.75, 0.25)))[None, :]
        level[i] = (1.0, 0.5, 0.5, 0.5, 0.0625, (2 * C - 0.5) / 32.0, (2 * C + 0.5) / 32.0)[i % 7]
    u[:, :, N - 1] = (2.0 - j / 16.0)[None, :]
    level[N - 1] = 0.75
    seg_n = np.array([L, 3 * C + 1], dtype=np.int64)
    u[1, 3 * C + 1:, 0::2], u[1, 3 * C + 1:, 1::2] = np.nan, 1e300
    t = np.cumsum(np.random.default_rng(12).random(L) + 0.125) - 0.5
    return dict(id="late-peak", u=u, t=t, seg_n=seg_n, levels=dict(abs=level, of_peak=level, of_start=level * 16.0), row_begins=(0, 1),
                never=float("nan"))


LATE_PEAK = _late_peak()
CASES += [_nan_rows(), _signed_zeros(), LATE_PEAK]
MATRIX_CASES = [next(c for c in CASES if c["id"] == "S2-L37-N130-tper"), LATE_PEAK, CASES[-2]]      # the cases run under every KNOBS
MATRIX_ROW_BEGINS = {"S2-L37-N130-tper": (0, 5), "late-peak": (0, 1), "signed-zeros": (0, 1)}


def judged(case, q, a):
    """The columns of output q[S][N] that the header specifies for this case: all of them, but on the case's `nan_cols` only u_peak."""
    a = np.asarray(a, dtype=float)
    if q == "u_peak" or not case.get("nan_cols"):
        return a
    keep = np.ones(a.shape[-1], dtype=bool)
    keep[case["nan_cols"]] = False
    return np.ascontiguousarray(a[..., keep])


def agree(case, q, got, ref):
    """Output q of a case as it is judged: bit for bit (a NaN by its place) - on the columns of the case's `nan_cols` only in
    u_peak, the header specifies nothing else there; u_peak of a case with `zeros` by value."""
    got, ref = judged(case, q, got), judged(case, q, ref)
    if q == "u_peak" and case.get("zeros"):
        return bool(np.array_equal(got, ref))
    return same_bits(got, ref)


# ---- the kernel's decomposition -------------------------------------------------------------------------------------------
NO_ROW = np.iinfo(np.int32).max


def fmax_ordered(a, b):
    """fmax as the device instruction forms it: a NaN is passed over, and of two zeros +0.0 is the larger."""
    r = np.fmax(a, b)
    return np.where((a == 0.0) & (b == 0.0), np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), r)


def replay_events(u, t, level, kind="abs", direction="rise", start="begin", row_begin=0, never=float("nan"), seg_n=None, waves=2,
                  part_rows=PART_ROWS):
    """event_kernel's decomposition, the lanes (and segments) as NumPy arrays: the rows from row_begin on in parts of part_rows,
    part p walked by wavefront p % waves; the peak combined as "larger value, then smaller row"; a level or a start that
    depends on the peak searched in a second walk that passes over a part ending at or before the earliest search start of the
    workgroup's 64 species; the crossing row the smallest of the wavefronts'. Returns (the dict of ref_events, skipped[G],
    walked[G]): per species group the parts of the second walk that were passed over and walked, over all segments."""
    u, t = np.asarray(u, dtype=float), np.asarray(t, dtype=float)
    S, L, N = u.shape
    W, Cp, jb = int(waves), int(part_rows), int(row_begin)
    G = -(-N // LANES)
    n = np.full(S, L) if seg_n is None else np.clip(np.asarray(seg_n, dtype=np.int64), 0, L)
    live = n > jb
    T2 = np.broadcast_to(t, (S, L)) if t.ndim == 1 else t
    want_cross = level is not None
    second = want_cross and (kind == "of_peak" or start == "peak")
    met = (lambda x, l: x >= l) if direction == "rise" else (lambda x, l: x <= l)
    lev = np.broadcast_to(np.asarray(0.0 if level is None else level, dtype=float), (N,))
    l = np.broadcast_to(lev, (S, N)).copy()
    if want_cross and kind == "of_start" and L > 0:
        l = l * u[:, min(jb, L - 1), :]
    pv, pr, cr = np.full((W, S, N), np.nan), np.full((W, S, N), NO_ROW), np.full((W, S, N), NO_ROW)
    nparts = int(max(0, -(-(int(n.max(initial=0)) - jb) // Cp)))
    skipped, walked = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)

    def walk(peak, search, l, j0, lo):
        for p in range(nparts):
            w, p0 = p % W, jb + p * Cp
            p1 = np.minimum(p0 + Cp, n)
            has = live & (p0 < n)                                            # the segments that have this part
            act = np.repeat(has[:, None], N, axis=1)
            if lo is not None:
                sk = has[:, None] & (p1[:, None] <= lo)                     # (the same in every lane of a group)
                skipped[:] += sk.sum(axis=0)
                walked[:] += (has[:, None] & ~sk).sum(axis=0)
                act &= ~np.repeat(sk, LANES, axis=1)[:, :N]
            for j in range(p0, min(p0 + Cp, L)):
                m = act & (j < p1)[:, None]
                x = u[:, j, :]
                if peak:
                    take = m & ((pr[w] == NO_ROW) | (x > pv[w]))
                    pr[w] = np.where(take, j, pr[w])
                    pv[w] = np.where(m, fmax_ordered(pv[w], x), pv[w])
                if search:
                    hit = m & (cr[w] == NO_ROW) & (j >= j0) & met(x, l)
                    cr[w] = np.where(hit, j, cr[w])

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        j0 = np.full((S, N), jb)
        walk(True, want_cross and not second, l, j0, None)
        bv, br = np.zeros((S, N)), np.full((S, N), NO_ROW)
        for ww in range(W):                                                  # larger value, then smaller row
            r, v = pr[ww], pv[ww]
            has, first = r != NO_ROW, br == NO_ROW
            upd = has & (first | (v > bv) | ((v == bv) & (r < br)))
            bv = np.where(has, np.where(first, v, fmax_ordered(bv, v)), bv)
            br = np.where(upd, r, br)
        if second:
            if kind == "of_peak":
                l = lev[None, :] * bv
            if start == "peak":
                j0 = br
            lo = np.minimum.reduceat(np.where(live[:, None], j0, NO_ROW), np.arange(0, N, LANES), axis=1)
            cr[:] = NO_ROW
            walk(False, True, l, j0, lo)
        jc = cr.min(axis=0)
        si, ii = np.arange(S)[:, None], np.arange(N)[None, :]
        at = lambda rows: np.clip(rows, 0, max(L - 1, 0))
        out = dict(u_peak=np.where(live[:, None], bv, 0.0))
        if L == 0:
            out["t_peak"] = np.full((S, N), never)
            out["t_cross"] = np.full((S, N), never)
        else:
            out["t_peak"] = np.where(live[:, None], T2[si, at(br)], never)
            ua, ub, ta, tb = u[si, at(jc - 1), ii], u[si, at(jc), ii], T2[si, at(jc - 1)], T2[si, at(jc)]
            chord = ta + ((l - ua) / (ub - ua)) * (tb - ta)
            out["t_cross"] = np.where(live[:, None] & (jc != NO_ROW), np.where(jc == j0, T2[si, at(j0)], chord), never)
    if not want_cross:
        del out["t_cross"]
    return out, skipped, walked
