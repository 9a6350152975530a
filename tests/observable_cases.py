"""The observables pass restated in plain Python, and the cases its tests run (no device here).

ref_observables is the definition of include/kinetica_hip.h in plain loops over Python floats - IEEE doubles, every product and
every sum rounded on its own, a short form summed in entry order, a long one as 64 chains folded by the butterfly - so the host
restatement and the device results are compared with it bit for bit.

The cases sit at the smallest shapes at which the kernel can go wrong: species counts around a wavefront's 64 lanes and past
1024 (odd counts: every second row starts 8 bytes off a 16-byte boundary), 8 193 and 16 385 species in two rows (a staged row of
more than 64 KiB; a row that does not fit LDS), form lengths around the short / long threshold of 64
terms and around 128 (a chain's second entry), states of magnitudes 1e16, 1 and -1e16 spread over the chains so that the order
of the sum decides the bits, -0.0 in states and weights, ratios with a zero denominator, segments of L, 0, 1 and about L / 2
rows with NaN rows behind them, and more than 64 distinct denominators (a second phase of the workgroup's table)."""
import numpy as np

from event_cases import same_bits  # noqa: F401  (the comparison the observables tests use as well)

SHORT_MAX = 64
FORM_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129)
ROWS = (None, "1", "3", "16")      # KIN_OBSERVABLES_ROWS of the GPU tests (None: unset)
LDS = (None, "0")                  # KIN_OBSERVABLES_LDS


def ref_form(idx, w, row):
    """The value of the form with the entries (idx[e], w[e]) at the state `row` (lists of Python floats and ints)."""
    n = len(idx)
    if n == 0:
        return 0.0

    def chain(entries):
        acc = w[entries[0]] * row[idx[entries[0]]]
        for e in entries[1:]:
            t = w[e] * row[idx[e]]
            acc = acc + t
        return acc

    if n <= SHORT_MAX:
        return chain(list(range(n)))
    v = [chain(list(range(l, n, 64))) for l in range(64)]
    off = 32
    while off >= 1:
        for l in range(off):
            v[l] = v[l] + v[l + off]
        off //= 2
    return v[0]


def ref_divide(a, b):
    """a / b as IEEE double division gives it (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def ref_observables(u, seg_n, forms, num, den, pitch):
    """out[S][L][pitch] of u[S][L][N]; forms = (form_ptr, form_idx, form_w) with 0-based species. Rows at or past seg_n[s] are
    never looked at."""
    u = np.asarray(u, dtype=float)
    S, L, N = u.shape
    ptr, idx, w = (np.asarray(a).tolist() for a in forms)
    H, G = max(len(ptr) - 1, 0), len(num)
    out = np.zeros((S, L, pitch))
    for s in range(S):
        n = L if seg_n is None else int(seg_n[s])
        for j in range(n):
            row = u[s, j].tolist()
            F = [ref_form(idx[ptr[f]:ptr[f + 1]], w[ptr[f]:ptr[f + 1]], row) for f in range(H)]
            for g in range(G):
                out[s, j, g] = F[num[g]] if den[g] < 0 else ref_divide(F[num[g]], F[den[g]])
    return out


def sequential_form(idx, w, row):
    """One sequential sum over all entries, whatever their number: what a long form is NOT."""
    acc = w[0] * row[idx[0]]
    for e in range(1, len(idx)):
        acc = acc + w[e] * row[idx[e]]
    return acc


# ---- the cases -------------------------------------------------------------------------------------------------------------
_MAGNITUDES = (1e16, 1.0, -1e16, 3.0, -0.0, 1e-3, 0.75, -2.5e-7)
_WEIGHTS = (1.0, -1.0, 0.5, -0.0, 2.0, 1.0, -3.0, 0.25)


def make_states(S, L, N, seg_n, seed):
    """u[S][L][N]: the magnitudes above in a pattern that shifts with the row, each scaled by a random factor in [1, 2) where it
    is not a zero, species 5 mod 11 an exact -0.0; NaN in every row at or past a segment's end."""
    rng = np.random.default_rng([seed, S, L, N])
    u = np.empty((S, L, N))
    for s in range(S):
        for j in range(L):
            shift = 3 * s + j
            u[s, j] = [_MAGNITUDES[(i + shift) % len(_MAGNITUDES)] for i in range(N)]
    u *= 1.0 + rng.integers(0, 8, u.shape) / 8.0
    u[:, :, 5::11] = -0.0
    for s in range(S):
        u[s, (L if seg_n is None else int(seg_n[s])):] = np.nan
    return u


def make_forms(N, seed, many_denominators=False):
    """(forms, num, den, names): forms of every length of FORM_LENGTHS that N allows and of N itself over distinct species, a
    singleton of weight 1.0 on a species that holds -0.0 (when there is one), a form with a repeated species - of 70 terms when
    N == 1, a long form over one species - and the observables: every form as it is, then ratios - by the empty form (a zero
    denominator: Inf and NaN by place), of a form by itself, of short by long and long by short. many_denominators adds 70
    singleton forms, each the denominator of one more observable: a second phase of the table of 64."""
    rng = np.random.default_rng([seed, N])
    ptr, idx, w, names = [0], [], [], []

    def add(name, ids, weights):
        idx.extend(int(i) for i in ids)
        w.extend(float(x) for x in weights)
        ptr.append(len(idx))
        names.append(name)
        return len(ptr) - 2

    by_len = {}
    for n in sorted(set(FORM_LENGTHS) | {N}):
        if n <= N:
            ids = rng.permutation(N)[:n]
            by_len[n] = add(f"len{n}", ids, [_WEIGHTS[(k + n) % len(_WEIGHTS)] for k in range(n)])
    negzero = add("copy", [5 if N > 5 else 0], [1.0])
    rep = add("repeat", [0, min(1, N - 1), 0, 0] if N > 1 else [0] * 70, [1.0, -2.0, 0.5, 1.0] if N > 1 else [1.0 + k / 64.0 for k in range(70)])
    H = len(ptr) - 1
    num, den = list(range(H)), [-1] * H
    longest, shortest = by_len[max(by_len)], by_len[1]
    for a, b in ((shortest, by_len[0]), (by_len[0], by_len[0]), (longest, by_len[0]), (longest, longest), (shortest, longest),
                 (longest, shortest), (rep, negzero), (negzero, rep)):
        num.append(a); den.append(b)
    if many_denominators:
        for k in range(70):
            f = add(f"single{k}", [k % N], [1.0 + k])
            num.append(by_len[sorted(by_len)[k % len(by_len)]]); den.append(f)
    forms = (np.array(ptr, np.int64), np.array(idx, np.int64), np.array(w))
    return forms, np.array(num, np.int64), np.array(den, np.int64), names


def make_case(N, S, L, seg_n, seed, many_denominators=False):
    seg = None if seg_n is None else np.array(seg_n, dtype=np.int64)
    forms, num, den, names = make_forms(N, seed, many_denominators)
    G = len(num)
    pitches = [G, G + 3] + ([N] if N >= G else [])
    name = f"N{N}-S{S}-L{L}-" + ("full" if seg is None else "n" + "_".join(str(int(x)) for x in seg)) + ("-dens" if many_denominators else "")
    return dict(id=name, u=make_states(S, L, N, seg, seed), seg_n=seg, forms=forms, num=num, den=den, pitches=pitches, names=names)


def empty_spec_case(N, S, L, H0):
    """G = 0, with H = 0 (no form_ptr worth the name) or with forms nobody asks for: every column is a zero."""
    forms = (np.array([0], np.int64), np.zeros(0, np.int64), np.zeros(0)) if H0 else make_forms(N, 3)[0]
    return dict(id=f"N{N}-S{S}-L{L}-G0" + ("-H0" if H0 else ""), u=make_states(S, L, N, None, 5), seg_n=None, forms=forms,
                num=np.zeros(0, np.int64), den=np.zeros(0, np.int64), pitches=[0, 3, N], names=[])


CASES = [
    make_case(1, 3, 5, (5, 0, 3), 1),
    make_case(1, 1, 1, None, 2),
    make_case(63, 3, 5, (1, 5, 2), 3),
    make_case(63, 1, 5, (3,), 4),
    make_case(64, 3, 1, (1, 0, 1), 5),
    make_case(64, 1, 5, None, 6),
    make_case(65, 3, 5, (5, 0, 3), 7),
    make_case(65, 1, 1, (0,), 8),
    make_case(129, 3, 5, (2, 5, 0), 9, many_denominators=True),
    make_case(129, 1, 5, (1,), 10),
    make_case(1025, 3, 5, (5, 1, 3), 11),
    make_case(1025, 1, 1, None, 12),
    # one staged row beyond 64 KiB of LDS (the kernel's opt-in to more dynamic LDS, one workgroup per compute unit), and a row
    # beyond the 16 384 species that fit LDS at all: the launcher's own switch to the gather path, no knob set
    make_case(8193, 1, 2, None, 13),
    make_case(16385, 1, 2, (1,), 14),
    empty_spec_case(65, 3, 5, True),
    empty_spec_case(65, 1, 5, False),
]

_REFS = {}


def reference(case):
    """ref_observables of a case at its compact pitch, computed once and shared (read-only); at(case, pitch) widens it."""
    if case["id"] not in _REFS:
        r = ref_observables(case["u"], case["seg_n"], case["forms"], case["num"], case["den"], len(case["num"]))
        r.setflags(write=False)
        _REFS[case["id"]] = r
    return _REFS[case["id"]]


def at(case, pitch):
    r = reference(case)
    out = np.zeros(r.shape[:2] + (pitch,))
    out[:, :, :r.shape[2]] = r
    return out

