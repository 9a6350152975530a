"""Host-side tests (no device) of the event-time pass: the NumPy restatement against closed forms and against a replay of the
kernel's decomposition under every launcher setting the GPU tests use (which also shows that the cases reach the paths they are
named after: the parts the second walk passes over, NaN rows, zeros of both signs), the argument checks of the
Python layers (ValueError before anything touches a device) and how `solving` hands event times to the statistics entries,
on a stand-in for capi.HipNetwork."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest

import event_cases as ec
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S


# ---- the restatement against closed forms ----------------------------------------------------------------------------------------
def test_half_life_of_an_exponential_decay_within_the_chord_bound():
    """u = exp(-k t) is convex: the chord lies above it by at most dt^2 max|u''| / 8 = k^2 dt^2 u / 8, which the slope k u turns
    into at most k dt^2 / 8 in time. The grid puts ln 2 / k inside an interval, not on a sample."""
    k, dt = 3.0, 0.01
    t = dt * np.arange(101)
    u = np.exp(-k * t)[None, :, None]
    r = ec.ref_events(u, t, 0.5, kind="of_start", direction="fall")
    tc = r["t_cross"][0, 0]
    assert 0.0 <= tc - math.log(2.0) / k <= k * dt * dt / 8.0
    assert r["u_peak"][0, 0] == 1.0 and r["t_peak"][0, 0] == 0.0


def test_triangle_pulse_is_exact():
    t = np.arange(7, dtype=float)
    u = np.array([0.0, 0.25, 0.5, 0.75, 0.5, 0.25, 0.0])[None, :, None]
    rise = ec.ref_events(u, t, 0.5, kind="of_peak", direction="rise")
    fall = ec.ref_events(u, t, 0.5, kind="of_peak", direction="fall", start="peak")
    assert rise["u_peak"][0, 0] == 0.75 and rise["t_peak"][0, 0] == 3.0
    assert rise["t_cross"][0, 0] == 1.5 and fall["t_cross"][0, 0] == 4.5      # the pulse is 3.0 wide at half of its maximum
    # falling from the beginning: the first row is already below the level
    assert ec.ref_events(u, t, 0.5, kind="of_peak", direction="fall")["t_cross"][0, 0] == 0.0


def test_edge_rules_of_the_restatement():
    t = np.array([1.0, 2.0, 4.0])
    u = np.array([[1.0, 0.0, -1.0], [3.0, 0.0, -2.0], [3.0, 0.0, -0.5]])[None]
    r = ec.ref_events(u, t, [3.0, 0.0, 10.0], kind="abs")
    assert r["u_peak"].tolist() == [[3.0, 0.0, -0.5]] and r["t_peak"].tolist() == [[2.0, 1.0, 4.0]]      # a plateau: the first row
    assert r["t_cross"][0, :2].tolist() == [2.0, 1.0] and np.isnan(r["t_cross"][0, 2])      # equal to a sample; met at j0; never
    # an empty segment; rows past n_s are not looked at; never is the caller's
    bad = np.concatenate([u, np.full((1, 2, 3), np.nan)], axis=1)
    r2 = ec.ref_events(bad, np.append(t, [np.nan, np.nan]), [3.0, 0.0, 10.0], seg_n=[3])
    assert all(ec.same_bits(r[q], r2[q]) for q in ec.OUTPUTS)
    e = ec.ref_events(u, t, 1.0, row_begin=3, never=-7.0)
    assert np.all(e["u_peak"] == 0.0) and np.all(e["t_peak"] == -7.0) and np.all(e["t_cross"] == -7.0)
    # all zero under of_peak: l = 0, rising, gives t[j0]; from row 1 on
    assert ec.ref_events(u, t, 0.5, kind="of_peak", row_begin=1)["t_cross"][0, 1] == 2.0
    assert "t_cross" not in ec.ref_events(u, t, None)


def test_cases_cover_what_they_claim():
    C = ec.PART_ROWS
    assert {c["u"].shape[2] for c in ec.CASES} >= {1, 63, 64, 65, 257}
    assert {c["u"].shape[1] for c in ec.CASES} >= {1, 2, 3, C - 1, C, C + 1, 2 * C + 1}
    assert any(c["t"].ndim == 2 for c in ec.CASES) and any(c["t"].ndim == 1 for c in ec.CASES)
    assert any(not np.isnan(c["never"]) for c in ec.CASES)
    for c in ec.CASES:
        if c["seg_n"] is not None and c["u"].shape[0] >= 4:
            L = c["u"].shape[1]
            assert {0, min(1, L), L} <= set(c["seg_n"].tolist())
            for s, n in enumerate(c["seg_n"]):
                assert np.all(~np.isfinite(c["u"][s, n:]) | (c["u"][s, n:] == 1e300))
    hb = next(c for c in ec.CASES if c["id"] == "hand-built")
    r = ec.ref_events(hb["u"], hb["t"], hb["levels"]["abs"])
    t = hb["t"]
    assert r["t_cross"][0, 0] == t[C - 1] + 0.5 * (t[C] - t[C - 1]) and r["t_cross"][0, 2] == t[C]      # the halo; a sample
    assert r["t_cross"][0, 3] == t[0] and np.isnan(r["t_cross"][0, 4]) and r["t_peak"][0, 6] == t[2]
    last = ec.ref_events(hb["u"], t, hb["levels"]["of_peak"], kind="of_peak", direction="fall", start="peak")
    assert last["t_cross"][0, 9] == t[-1] and last["t_peak"][0, 9] == t[-1]
    # the late-peak case: where its peaks and crossings land (a chord's time lies in the interval that ends at the crossing row)
    lp, W = ec.LATE_PEAK, 2
    u, t, lev = lp["u"], lp["t"], lp["levels"]["of_peak"]
    L, i = u.shape[1], np.arange(64)
    assert (u.shape, L) == ((2, L, 65), 4 * C + 1) and lp["seg_n"].tolist() == [L, 3 * C + 1]
    peak_row = u[0, :, :64].argmax(axis=0)
    assert peak_row.min() == 2 * C and peak_row[0] == 2 * C and peak_row.max() < 3 * C and u[0, :, 64].argmax() == 0
    fall = ec.ref_events(u, t, lev, kind="of_peak", direction="fall", start="peak", seg_n=lp["seg_n"])["t_cross"][0]
    rise = ec.ref_events(u, t, lev, kind="of_peak", direction="rise", start="begin", seg_n=lp["seg_n"])["t_cross"][0]
    lands = lambda tc, rows: np.all((t[rows - 1] < tc) & (tc <= t[rows]))
    k = i % 7
    assert np.array_equal(fall[:64][k == 0], t[peak_row[k == 0]]) and lands(fall[:64][k == 1], peak_row[k == 1] + 1)
    assert lands(fall[:64][k == 2], np.full((k == 2).sum(), 3 * C)) and lands(fall[:64][k == 3], np.full((k == 3).sum(), L - 1))
    assert np.isnan(fall[:64][k == 4]).all()
    assert lands(rise[:64][k == 5], np.full((k == 5).sum(), 2 * C - 1)) and lands(rise[:64][k == 6], np.full((k == 6).sum(), 2 * C))
    # ... and what the second walk of the kernel's decomposition passes over: with two wavefronts and parts of C rows, parts 0
    # and 1 of both segments in the first species group, nothing in the second (species 64 peaks at its first row)
    for kind in ("abs", "of_peak"):
        _, skipped, walked = ec.replay_events(u, t, lp["levels"][kind], kind=kind, direction="fall", start="peak", seg_n=lp["seg_n"],
                                              waves=W, part_rows=C)
        assert skipped.tolist() == [4, 0] and walked.tolist() == [5 + 4 - 4, 5 + 4], (kind, skipped, walked)
    _, skipped, walked = ec.replay_events(u, t, lev, kind="of_peak", direction="rise", start="begin", seg_n=lp["seg_n"], waves=W, part_rows=C)
    assert skipped.tolist() == [0, 0] and walked.tolist() == [9, 9]          # from the beginning: every part is walked
    # the NaN and signed-zero cases hold what they are named after
    nr = next(c for c in ec.CASES if c["id"] == "nan-rows")
    held = np.isnan(nr["u"][0]).any(axis=0)
    assert np.flatnonzero(held).tolist() == nr["nan_cols"] and np.isnan(nr["u"][0, :, nr["nan_cols"][7]]).all()
    assert all(np.isnan(nr["u"][0, rb, nr["nan_cols"][rb]]) for rb in (0, 1))
    sz = next(c for c in ec.CASES if c["id"] == "signed-zeros")
    assert np.all(sz["u"] == 0.0) and np.signbit(sz["u"][0, :2, 0]).tolist() == [True, False] and np.signbit(sz["u"][0, :2, 1]).tolist() == [False, True]
    assert np.signbit(sz["u"][0, :, 2]).tolist() == [True] * (2 * C) + [False]
    # the matrix of launcher settings: every wavefront count the launcher chooses, a part of one row, parts that are no multiple of
    # the rows in flight, and the launcher's own size
    plans = {ec.knob_plan(kn, 37) for kn in ec.KNOBS}
    assert {w for w, _ in plans} == {1, 2, 4, 8, 16} and {c for _, c in plans} >= {1, 3, 5, 6, 4, 8, 12, 40} and len(ec.KNOBS) == 21
    assert [c["id"] for c in ec.MATRIX_CASES] == ["S2-L37-N130-tper", "late-peak", "signed-zeros"]
    assert all(set(ec.MATRIX_ROW_BEGINS[c["id"]]) <= set(c["row_begins"]) for c in ec.MATRIX_CASES)


def _peak_by_greater_than(u, row_begin, seg_n):
    """(u_peak, row of the peak) by the chain the restatement had before it took up the header's NaN rule: from the first row,
    a later row only if it compares greater."""
    S, L, N = u.shape
    peak, row = np.zeros((S, N)), np.full((S, N), -1)
    for s in range(S):
        n = L if seg_n is None else int(seg_n[s])
        for i in range(N):
            if row_begin < n:
                col = u[s, :n, i].tolist()
                peak[s, i], row[s, i] = col[row_begin], row_begin
                for j in range(row_begin + 1, n):
                    if col[j] > peak[s, i]:
                        peak[s, i], row[s, i] = col[j], j
    return peak, row


def test_the_nan_rule_changes_no_case_without_a_nan_inside_a_segment():
    for c in ec.CASES:
        u, t, seg_n = c["u"], c["t"], c["seg_n"]
        S, L, N = u.shape
        inside = np.arange(L)[None, :] < (np.full(S, L) if seg_n is None else seg_n)[:, None]
        clean = ~np.isnan(np.where(inside[:, :, None], u, 0.0)).any(axis=1)          # [S][N]: no NaN among the segment's rows
        assert clean.all() == ("nan_cols" not in c), c["id"]
        for rb in c["row_begins"]:
            r = ec.ref_events(u, t, None, row_begin=rb, never=-1.0, seg_n=seg_n)
            peak, row = _peak_by_greater_than(u, rb, seg_n)
            T2 = np.broadcast_to(t, (S, L)) if t.ndim == 1 else t
            t_peak = np.where(row >= 0, T2[np.arange(S)[:, None], np.maximum(row, 0)], -1.0)
            assert r["u_peak"][clean].tobytes() == peak[clean].tobytes() and r["t_peak"][clean].tobytes() == t_peak[clean].tobytes(), (c["id"], rb)
    # on the NaN columns: the maximum of the rows that are numbers, NaN only where every row is NaN
    c = next(c for c in ec.CASES if c["id"] == "nan-rows")
    for rb in c["row_begins"]:
        got = ec.ref_events(c["u"], c["t"], None, row_begin=rb)["u_peak"][0, c["nan_cols"]]
        rows = c["u"][0, rb:, c["nan_cols"]].T
        every = np.isnan(rows).all(axis=0)
        assert every.sum() == (1 if rb == 0 else 2) and np.isnan(got[every]).all()
        assert np.array_equal(got[~every], np.nanmax(rows[:, ~every], axis=0))


@pytest.mark.parametrize("case", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_the_kernels_decomposition_gives_the_restatement(case):
    """The replay under every setting of the matrix, every combination and every row_begin of the case: the bits of ref_events
    (as the case is judged) and the same bytes under every setting."""
    u, t, seg_n, never = case["u"], case["t"], case["seg_n"], case["never"]
    checked = 0
    for kind, direction, start in ec.COMBOS:
        level = case["levels"][kind]
        for rb in case["row_begins"]:
            kw = dict(kind=kind, direction=direction, start=start, row_begin=rb, never=never, seg_n=seg_n)
            ref = ec.ref_events(u, t, level, **kw)
            first = None
            for plan in sorted({ec.knob_plan(kn, u.shape[1]) for kn in ec.KNOBS} | {ec.knob_plan({}, u.shape[1])}):
                got = ec.replay_events(u, t, level, waves=plan[0], part_rows=plan[1], **kw)[0]
                first = first or got
                for q in ec.OUTPUTS:
                    assert ec.agree(case, q, got[q], ref[q]), (case["id"], kw, plan, q)
                    assert ec.judged(case, q, got[q]).tobytes() == ec.judged(case, q, first[q]).tobytes(), (case["id"], kw, plan, q)
                checked += 1
    assert checked >= len(ec.COMBOS) * len(case["row_begins"]) * 5


# ---- argument checks: ValueError, and no device -------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    monkeypatch.setattr(capi.HipNetwork, "__init__", boom)


def _handle(n=3):
    h = object.__new__(capi.HipNetwork)
    h._h, h.n, h.nr, h.index_base = None, n, 2, 0
    return h


@pytest.mark.parametrize("kw", [
    dict(kind="relative"), dict(direction="up"), dict(start="end"), dict(level=[1.0, 2.0]), dict(level=1.0, want=("t_first",)),
    dict(want=()), dict(want=("t_cross",)), dict(seg_n=[1, 2, 3])])
def test_binding_refuses_malformed_arguments(no_library, kw):
    u, t = np.zeros((2, 4, 3)), np.arange(4.0)
    with pytest.raises(ValueError):
        _handle().events_segmented(u, t, **kw)


def test_binding_refuses_malformed_blocks_and_times(no_library):
    h = _handle()
    with pytest.raises(ValueError):
        h.events_segmented(np.zeros((4, 3)), np.arange(4.0), level=1.0)
    with pytest.raises(ValueError):
        h.events_segmented(np.zeros((2, 4, 5)), np.arange(4.0), level=1.0)
    for t in (np.arange(5.0), np.zeros((3, 4)), np.zeros((2, 4, 1))):
        with pytest.raises(ValueError):
            h.events_segmented(np.zeros((2, 4, 3)), t, level=1.0)


def test_binding_hands_over_what_the_entry_takes(monkeypatch):
    """On a stand-in for the library: the arguments of kin_events_segmented in the header's order, a number as level[N]."""
    calls = []

    class Lib:
        def kin_events_segmented(self, *a):
            calls.append(a)
            return capi.KIN_OK

    monkeypatch.setattr(capi, "lib", lambda: Lib())
    u, t = np.arange(24.0).reshape(2, 4, 3), np.arange(8.0).reshape(2, 4)
    r = _handle().events_segmented(u, t, level=0.25, kind="of_start", direction="fall", start="peak", row_begin=1, never=9.0, seg_n=[4, 2])
    (a,) = calls
    read = lambda p, shape, ty=np.float64: np.ctypeslib.as_array(p, shape=shape).astype(ty)
    assert len(a) == 16 and a[1:3] == (2, 4) and a[6] == 1 and a[8:13] == (2, -1, 1, 1, 9.0)
    assert read(a[3], (2,)).tolist() == [4, 2] and np.array_equal(read(a[4], u.shape), u) and np.array_equal(read(a[5], t.shape), t)
    assert read(a[7], (3,)).tolist() == [0.25] * 3
    assert sorted(r) == sorted(ec.OUTPUTS) and all(v.shape == (2, 3) for v in r.values())
    assert all(ctypes.addressof(a[13 + i].contents) == r[q].ctypes.data for i, q in enumerate(ec.OUTPUTS))
    _handle().events_segmented(u, t[0], want=("u_peak",))
    a = calls[-1]
    assert a[3] is None and a[6] == 0 and a[7] is None and a[8:12] == (0, 1, 0, 0) and a[13] is not None and a[14] is None and a[15] is None


def _out(with_states=True):
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])
    t = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    sol = S.ODESolution(t, np.arange(15.0).reshape(5, 3) if with_states else None, "Success")
    return S.ODESolveOutput(sd, rd, sol, None, None, None, None)


@pytest.mark.parametrize("kw", [
    dict(kind="relative"), dict(kind=1), dict(direction=1), dict(start="end"), dict(level="high"), dict(level=[[1.0]]), dict(level=True),
    dict(level=[1.0, 2.0]), dict(t_min="soon"), dict(t_min=float("nan")), dict(never=None), dict(never="never"), dict(species=["D"]),
    dict(species=[3]), dict(species=[0.5]), dict(t=[0.0, 1.0])])
def test_event_times_refuses_malformed_arguments_before_any_handle(no_library, kw):
    with pytest.raises(ValueError):
        S.event_times(_out(), **dict(dict(level=1.0), **kw))


def test_event_times_refuses_what_it_cannot_read(no_library):
    with pytest.raises(ValueError, match="no saved states"):
        S.event_times(_out(with_states=False), level=1.0)
    h = _handle()
    with pytest.raises(ValueError, match="needs t"):
        S.event_times(h, level=1.0)
    with pytest.raises(ValueError, match="one save grid"):
        S.event_times(h, level=1.0, t=np.zeros((2, 4)), t_min=0.5)
    with pytest.raises(ValueError):
        S.event_times(h, level=1.0, t=np.zeros((2, 4, 1)))
    with pytest.raises(ValueError, match="species ids"):
        S.event_times(h, level=1.0, t=np.arange(4.0), species=[3])


@pytest.mark.parametrize("events", [7, dict(colour=1), dict(kind="x"), dict(level=[[1.0]]), dict(never="x"), dict(species=[-1])])
def test_solve_network_ensemble_refuses_malformed_events_before_the_device(no_library, events):
    with pytest.raises(ValueError):
        S.solve_network_ensemble([object()], None, None, events=events)


@pytest.mark.parametrize("statistics", [
    dict(of="t_first"), dict(of="max"), dict(of="t_cross"), dict(of="t_cross", events=dict(kind="abs")), dict(events=dict(level=1.0)),
    dict(of="t_peak", events=dict(species=[0])), dict(of="t_peak", events=dict(colour=1)),
    dict(sobol=dict(M=2, P=1, of="t_cross")), dict(sobol=dict(M=2, P=1, of="max", events=dict(level=1.0))),
    dict(sobol=dict(M=2, P=1, of="t_peak", events=dict(start="end")))])
def test_statistics_arguments_refuse_malformed_of_and_events(statistics):
    with pytest.raises(ValueError):
        S._statistics_arguments(statistics, 6)


def test_statistics_arguments_carry_of_and_events():
    kw = S._statistics_arguments(dict(of="t_cross", events=dict(level=0.5, kind="of_start", direction="fall")), 6)
    assert kw["of"] == "t_cross" and kw["events"]["level"] == 0.5 and kw["events"]["kind"] == "of_start" and kw["events"]["start"] == "begin"
    kw = S._statistics_arguments(dict(sobol=dict(M=2, P=1, of="t_peak")), 6)
    assert "of" not in kw and "events" not in kw and kw["sobol"]["of"] == "t_peak" and kw["sobol"]["events"]["level"] is None
    assert "events" not in S._statistics_arguments(dict(sobol=dict(M=2, P=1)), 6)["sobol"]      # the default: the keywords as they were


# ---- the of= plumbing, on a stand-in for the handle --------------------------------------------------------------------------------
K, ROWS, N = 6, 5, 3
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0])
T_PEAK, T_CROSS, U_PEAK = (np.arange(K * N, dtype=float).reshape(K, N) + off for off in (0.0, 100.0, 200.0))


class _Recorder:
    """Stands in for a capi.HipNetwork that holds a stored ensemble of K members: records every call."""
    n, index_base = N, 1

    def __init__(self, n_saved=(ROWS,) * K):
        self.calls, self.n_saved = [], np.array(n_saved, dtype=np.int64)

    def ensemble_size(self):
        return K, ROWS, N, self.n_saved

    def ensemble_events(self, t, **kw):
        self.calls.append(("ensemble_events", (t,), kw))
        r = dict(u_peak=U_PEAK.copy(), t_peak=T_PEAK.copy())
        if kw.get("level") is not None:
            r["t_cross"] = T_CROSS.copy()
        return r

    def ensemble_sobol_weights(self, M, P):
        return np.ones(M, np.int32)

    def _members(self, name, u, a, kw, result):
        self.calls.append((name, (u,) + a, kw))
        return result

    def members_sobol(self, u, *a, **kw):
        z = np.zeros((1, N, 1))
        return self._members("members_sobol", u, a, kw, dict(first=z, total=z, mean=z[..., 0], var=z[..., 0], count=2))

    def members_moments(self, u, *a, **kw):
        z = np.zeros((1, N))
        return self._members("members_moments", u, a, kw, dict(count=K, mean=z, var=z, min=z, max=z))

    def members_quantiles(self, u, *a, **kw):
        return self._members("members_quantiles", u, a, kw, np.zeros((len(a[0]), 1, N)))

    def members_correlate(self, u, *a, **kw):
        return self._members("members_correlate", u, a, kw, np.zeros((1, N, 2)))


def test_event_times_on_a_handle_reads_the_stored_ensemble():
    h = _Recorder()
    ev = S.event_times(h, level=0.5, kind="of_peak", direction="fall", start="peak", t_min=0.75, never=2.0, species=[3, 1], t=GRID)
    ((name, (t,), kw),) = h.calls
    assert name == "ensemble_events" and np.array_equal(t, GRID)
    assert kw == dict(row_begin=2, level=0.5, kind="of_peak", direction="fall", start="peak", never=2.0)      # t >= 0.75: from row 2
    assert isinstance(ev, S.EventTimes) and [f.name for f in dataclasses.fields(ev)][:4] == ["t", "u_peak", "t_peak", "t_cross"]
    assert np.array_equal(ev.t_cross, T_CROSS[:, [2, 0]]) and np.array_equal(ev.u_peak, U_PEAK[:, [2, 0]])      # (the handle's base is 1)
    assert ev.species.tolist() == [3, 1] and ev.level.tolist() == [0.5] * N and (ev.kind, ev.never, ev.t_min) == ("of_peak", 2.0, 0.75)
    ev = S.event_times(h, t=GRID)
    assert ev.t_cross is None and ev.level is None and h.calls[-1][2]["row_begin"] == 0 and np.array_equal(ev.t_peak, T_PEAK)
    assert S.event_times(h, t=GRID, t_min=2.5).t_min == 2.5 and h.calls[-1][2]["row_begin"] == ROWS


@pytest.mark.parametrize("of, block", [("t_peak", T_PEAK), ("t_cross", T_CROSS)])
def test_sobol_indices_hands_the_event_array_to_members_sobol(of, block):
    h = _Recorder()
    si = S.sobol_indices(h, GRID, 2, 1, species=[2], of=of, events=dict(level=0.25, direction="fall"))
    assert [c[0] for c in h.calls] == ["ensemble_events", "members_sobol"]
    assert h.calls[0][2] == dict(row_begin=0, level=0.25, kind="abs", direction="fall", start="begin", never=h.calls[0][2]["never"])
    name, a, kw = h.calls[1]
    assert a[0].shape == (K, 1, N) and np.array_equal(a[0][:, 0], block) and a[0].flags.c_contiguous and a[1:] == (2, 1)
    assert kw["species"] == [2] and np.array_equal(kw["w"], np.ones(2, np.int32))
    assert isinstance(si, S.SobolIndices) and si.count == 2
    with pytest.raises(ValueError):
        S.sobol_indices(h, GRID, 2, 1, of="t_cross")
    with pytest.raises(ValueError):
        S.sobol_indices(h, GRID, 2, 1, of="max", events=dict(level=1.0))


def test_ensemble_statistics_hands_the_event_array_to_the_members_entries():
    h = _Recorder(n_saved=(ROWS, ROWS, 2, ROWS, ROWS, ROWS))
    X = np.ones((K, 2))
    st = S.ensemble_statistics(h, GRID, quantiles=(0.5,), species=[1], inputs=X, of="t_cross", events=dict(level=0.5, kind="of_start"))
    assert [c[0] for c in h.calls] == ["ensemble_events", "members_moments", "members_quantiles", "members_correlate"]
    done = np.array([True, True, False, True, True, True])       # the default participants: the members that completed the grid
    for name, a, kw in h.calls[1:]:
        assert a[0].shape == (K, 1, N) and np.array_equal(a[0][:, 0], T_CROSS) and np.array_equal(kw["use"], done)
    assert h.calls[2][2]["species"].tolist() == [1] and h.calls[3][1][1] is X and h.calls[3][2]["rank"] is True
    assert st.count == K and st.mean.shape == (1, N) and st.quantiles.shape == (1, 1, N) and st.corr.shape == (1, N, 2)
    use = np.array([1, 0, 0, 1, 1, 1])
    S.ensemble_statistics(h, GRID, quantiles=None, use=use, of="t_peak")
    assert np.array_equal(h.calls[-1][1][0][:, 0], T_PEAK) and h.calls[-1][2]["use"] is use and h.calls[-1][0] == "members_moments"
