"""Host tests of the resampling pass (no device): the symbols, kin_resample_bracket_host against the restatement of
resample_cases.py bit for bit - on the cases and on axes of up to 1000 rows with plateaus of every kind, queried at, next to
and between their values -, what the slice and plan cases hold, the statuses of the host-checkable arguments, the refusal of every malformed resample= dict
before a handle exists, and the restatement's own self-check."""
import os
import re

import numpy as np
import pytest

import resample_cases as rc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kin_resample_bracket_host", "kin_resample_segmented", "kin_resample_segmented_dev", "kin_solution_resample",
         "kin_ensemble_resample"]


def test_symbols_are_declared_listed_and_exported_under_abi_6():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kinetica_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kin_[A-Za-z0-9_]+)\s*\(", text))
    L = capi.lib()
    for name in NAMES:
        assert name in declared and name in capi.SYMBOLS and name in capi.ARGTYPES, name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"#define KIN_ABI_VERSION 6\b", text) and L.kin_abi_version() == 6 and capi.ABI_VERSION == 6
    assert "KIN_RESAMPLE_FILL = 0" in text and "KIN_RESAMPLE_HOLD = 1" in text and capi.RESAMPLE_MODES == dict(fill=0, hold=1)


@pytest.mark.parametrize("case", rc.CASES, ids=[c["id"] for c in rc.CASES])
def test_bracket_host_is_the_restatement_bit_for_bit(case):
    u, x, xq, seg_n = case["u"], case["x"], case["xq"], case["seg_n"]
    S_ = u.shape[0]
    for rb in case["row_begins"]:
        _, jc_ref, w_ref = rc.ref_resample(u[:, :, :1], x, xq, seg_n=seg_n, row_begin=rb)
        jc, w = capi.resample_brackets(x if x.ndim == 2 else np.tile(x, (S_, 1)), xq, seg_n=seg_n, row_begin=rb)
        assert jc.dtype == np.int32 and jc.shape == jc_ref.shape == (S_, xq.shape[-1])
        assert np.array_equal(jc, jc_ref), (case["id"], rb, jc, jc_ref)
        assert w.tobytes() == w_ref.tobytes(), (case["id"], rb)
        assert np.all(w[jc < 0] == 0.0) and np.all((w >= 0.0) & (w < 1.0))


def test_cases_cover_what_they_claim():
    assert {c["u"].shape[2] for c in rc.CASES} == {1, 63, 64, 65, 257}
    assert {c["u"].shape[1] for c in rc.CASES} == {1, 2, 3, 9, 37}
    assert {c["xq"].shape[-1] for c in rc.CASES} == {0, 1, 3, 4, 5, 9}
    assert {c["x"].ndim for c in rc.CASES} == {1, 2} and {c["xq"].ndim for c in rc.CASES} == {1, 2}
    seen = set()
    for c in rc.CASES:
        L = c["u"].shape[1]
        assert {0, 1, L - 1, L} <= set(c["row_begins"])
        if len(c["seg_n"]) >= 4:
            assert set(c["seg_n"].tolist()) == {L, 0, min(1, L), (L + 1) // 2}
        xq = c["xq"]
        seen |= {k for k, hit in (("nan", np.isnan(xq).any()), ("+inf", (xq == np.inf).any()), ("-inf", (xq == -np.inf).any())) if hit}
        out, jc, w = rc.ref_resample(c["u"], c["x"], xq, seg_n=c["seg_n"])
        seen |= {("jc", int(v)) for v in np.unique(jc[jc < 0])}
        if (jc >= 0).any():
            seen |= {"copy"} if ((jc >= 0) & (w == 0.0)).any() else set()
            seen |= {"chord"} if (w > 0.0).any() else set()
        s0 = xq[0] if xq.ndim == 2 else xq
        if len(s0) != len(set(s0[~np.isnan(s0)].tolist())) + int(np.isnan(s0).sum()):
            seen.add("repeat")
        if len(s0) > 2 and np.any(np.diff(s0[~np.isnan(s0)]) < 0):
            seen.add("unsorted")
        x0 = c["x"][0] if c["x"].ndim == 2 else c["x"]
        inner = x0[:-1][np.diff(x0) == 0]
        if len(inner) and np.isin(s0, inner).any():
            seen.add("plateau")
    assert seen >= {"nan", "+inf", "-inf", ("jc", -1), ("jc", -2), ("jc", -3), "copy", "chord", "repeat", "unsorted", "plateau"}, seen


def test_slice_and_plan_cases_cover_what_they_claim():
    S1 = rc.SLICE
    assert [c["u"].shape for c in rc.SLICE_CASES] == [(2, 9, n) for n in (S1, S1 + 1, S1 + 65, 2 * S1 + 1)]
    assert any(c["x"].ndim == 2 and c["xq"].ndim == 2 for c in rc.SLICE_CASES) and {c["x"].ndim for c in rc.SLICE_CASES} == {1, 2}
    for c in rc.SLICE_CASES + [rc.PLAN_CASE]:
        u, L = c["u"], c["u"].shape[1]
        assert len(c["row_begins"]) == 3 and c["seg_n"].tolist()[:2] == [L, (L + 1) // 2]
        # on the last slice as on the first: -0.0, subnormals and a NaN with a payload among the rows a query copies
        out, jc, w = rc.ref_resample(u, c["x"], c["xq"], seg_n=c["seg_n"])
        copied = out[(jc >= 0) & (w == 0.0)]
        assert len(copied)
        for i0 in (0, S1) if u.shape[2] > S1 + 64 else (0,):
            assert np.signbit(copied[:, i0 + 1]).all() and np.all(copied[:, i0 + 1] == 0.0)
            assert np.all(np.abs(copied[:, i0 + 2]) < 2.3e-308) and np.any(copied[:, i0 + 2] != 0.0)
            assert set(np.unique(np.ascontiguousarray(copied[:, i0 + 12]).view(np.uint64)).tolist()) & set(rc.PAYLOADS.view(np.uint64).tolist())
    assert sum(c["u"].shape[2] > S1 + 64 for c in rc.SLICE_CASES) == 2
    pc = rc.PLAN_CASE
    assert pc["u"].shape == (3, 37, 65) and pc["xq"].shape == (3, 70) and pc["x"].shape == (3, 37)
    assert rc.PLANS == [(1, 1), (8, 4), (16, 4), (32, 4), (33, 3), (256, 1), (256, 16)]
    assert 70 % 32 == 6 and 32 // 4 == 8 and 70 > 64 * 1          # the partial tile; queries per wavefront; the search's second trip


def _long_axes(L, rng):
    """[4][L]: strictly increasing; one plateau over all rows but the first; over all but the last; plateaus of random length."""
    inc = np.cumsum(rng.random(L) + 0.125) + 900.0
    late, early = inc.copy(), inc.copy()
    late[1:] = inc[1]
    early[:-1] = inc[0]
    steps = np.cumsum(np.where(rng.random(L) < 0.4, rng.random(L) + 0.125, 0.0)) + 900.0
    return np.stack([inc, late, early, steps])


@pytest.mark.parametrize("L", [2, 3, 64, 65, 1000])
def test_bisection_is_the_row_walk_on_long_axes_and_plateaus(L):
    """kin_resample_bracket_host's bisection against ref_bracket's walk over the rows: a query at every axis value, at its two
    neighbours among the doubles, at the midpoint of every rising interval, at +-Inf and at NaN."""
    x = _long_axes(L, np.random.default_rng(L))
    qs = []
    for xs in x:
        rising = np.flatnonzero(np.diff(xs) > 0)
        qs.append(np.concatenate([xs, np.nextafter(xs, -np.inf), np.nextafter(xs, np.inf), 0.5 * (xs[rising] + xs[rising + 1]),
                                  [np.inf, -np.inf, np.nan]]))
    Q = max(len(q) for q in qs)
    xq = np.stack([np.concatenate([q, np.full(Q - len(q), np.nan)]) for q in qs])
    assert len(np.flatnonzero(np.diff(x[3]) == 0)) > 0 or L < 4
    for rb in sorted({0, 1, L - 1, L}):
        jc, w = capi.resample_brackets(x, xq, row_begin=rb)
        ref = [[rc.ref_bracket(xs, rb, L, v) for v in q] for xs, q in zip(x.tolist(), xq.tolist())]
        jc_ref, w_ref = np.array([[r[0] for r in row] for row in ref], np.int32), np.array([[r[1] for r in row] for row in ref])
        assert np.array_equal(jc, jc_ref), (L, rb)
        assert w.tobytes() == w_ref.tobytes(), (L, rb)
        if rb < L - 1:
            assert {rc.BELOW, rc.ABOVE, rc.NONE} <= set(jc.ravel().tolist()) and (jc >= 0).any() and (w > 0.0).any()


def test_restatement_at_a_segments_own_axis_returns_its_rows():
    """The yardstick's self-check: -0.0, subnormals, Inf and the first row of a plateau included."""
    rng = np.random.default_rng(3)
    L, N = 9, 16
    u = np.stack([np.stack([rc._column(i % rc.COLUMN_KINDS, L, rng) for i in range(N)], axis=1)])
    x = np.cumsum(rng.random(L) + 0.125)
    out, jc, w = rc.ref_resample(u, x, x)
    assert out.tobytes() == u.tobytes() and jc.tolist() == [list(range(L))] and np.all(w == 0.0)
    x[4] = x[3]      # a plateau: both queries give the first row that holds the value
    out, jc, _ = rc.ref_resample(u, x, x)
    assert jc[0].tolist() == [0, 1, 2, 3, 3, 5, 6, 7, 8] and out[0, 4].tobytes() == u[0, 3].tobytes()
    mid, _, w = rc.ref_resample(u[:, :, 6:7], np.arange(9.0), np.array([2.5]))
    assert w[0, 0] == 0.5 and mid[0, 0, 0] == u[0, 2, 6] + 0.5 * (u[0, 3, 6] - u[0, 2, 6])
    assert rc.covered_run(np.array([[0, 1, -2, 3], [-1, 0, 0, 0], [1, 1, 1, 1]]), "fill").tolist() == [2, 0, 4]
    assert rc.covered_run(np.array([[0, -1, -2, -3], [-3, 0, 0, 0]]), "hold").tolist() == [3, 0]


def test_statuses_of_the_host_checkable_arguments():
    lib = capi.lib()
    pd, p64, p32 = capi._pd, capi._p64, capi._p32
    S_, L, Q = 2, 4, 3
    x, xq = np.arange(float(L)), np.array([0.5, 7.0, 2.0])
    seg = np.array([L, 2], np.int64)
    jc, w = np.full((S_, Q), 99, np.int32), np.full((S_, Q), 99.0)

    def call(S=S_, L_=L, seg_n=seg, x_=x, per=0, Q_=Q, xq_=xq, qper=0, rb=0, outs=(0, 1)):
        return lib.kin_resample_bracket_host(S, L_, p64(seg_n), pd(x_), per, Q_, pd(xq_), qper, rb, p32(jc) if 0 in outs else None,
                                             pd(w) if 1 in outs else None)

    assert call() == capi.KIN_OK
    assert jc.tolist() == [[1, -2, 2], [1, -2, -2]] and w.tolist() == [[0.5, 0.0, 0.0], [0.5, 0.0, 0.0]]
    good = (jc.copy(), w.copy())
    nan = float("nan")
    late = np.array([0.0, 1.0, 3.0, 2.0])      # decreasing in rows 2, 3: segment 0 reads them, segment 1 does not
    refused = [dict(S=-1), dict(L_=-1), dict(Q_=-1), dict(rb=-1), dict(x_=None), dict(xq_=None), dict(outs=()),
               dict(seg_n=np.array([L + 1, 0], np.int64)), dict(seg_n=np.array([-1, 0], np.int64)), dict(x_=late),
               dict(x_=np.stack([late, x]), per=1), dict(x_=np.array([0.0, nan, 2.0, 3.0])), dict(x_=np.array([nan, 1.0, 2.0, 3.0]))]
    for kw in refused:
        assert call(**kw) == capi.KIN_ERR_INVALID_ARG, kw
    for kw in (dict(S=1 << 31, L_=0, x_=None, seg_n=None, Q_=0), dict(L_=1 << 31, S=0, seg_n=None), dict(Q_=1 << 31, S=0, seg_n=None)):
        assert call(**kw) == capi.KIN_ERR_UNSUPPORTED, kw
    assert jc.tobytes() == good[0].tobytes() and w.tobytes() == good[1].tobytes()      # a refused call writes nothing
    # what is allowed: an axis that is bad only where no row is read, plateaus, one output alone, nothing to do
    assert call(x_=np.stack([x, late]), per=1) == capi.KIN_OK
    assert call(x_=late, rb=3) == capi.KIN_OK and call(x_=np.array([nan, 1.0, 2.0, 3.0]), rb=1) == capi.KIN_OK
    assert call(x_=np.array([0.0, 1.0, 1.0, 1.0])) == capi.KIN_OK and call(rb=L + 5) == capi.KIN_OK
    assert call(outs=(0,)) == capi.KIN_OK and call(outs=(1,)) == capi.KIN_OK
    assert call(S=0, x_=None, xq_=None, seg_n=None) == capi.KIN_OK and call(Q_=0, xq_=None) == capi.KIN_OK
    assert call(L_=0, x_=None, seg_n=None) == capi.KIN_OK
    # the entries that take a handle refuse a null one before anything else
    out = np.zeros((S_, Q, 1))
    assert lib.kin_resample_segmented(None, S_, L, None, pd(out), pd(x), 0, Q, pd(xq), 0, 0, nan, 0, pd(out), None, None) == capi.KIN_ERR_INVALID_ARG
    assert lib.kin_ensemble_resample(None, pd(x), 0, Q, pd(xq), 0, 0, nan, 0, 0, pd(out)) == capi.KIN_ERR_INVALID_ARG
    assert lib.kin_solution_resample(None, None, Q, pd(xq), 0, nan, 0, pd(out)) == capi.KIN_ERR_INVALID_ARG
    with pytest.raises(capi.KineticaHipError) as e:
        capi.resample_brackets(late, xq)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG


# ---- argument checks: ValueError, and no device ---------------------------------------------------------------------------------
@pytest.fixture
def no_handle(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("a handle was constructed")
    monkeypatch.setattr(capi.HipNetwork, "__init__", boom)


def _methods(rate=1e5, K=3):
    from kinetica_jl_amd import conditions as C
    from kinetica_jl_amd.synth import synthetic_crn
    n = 12
    net, Ea, A = synthetic_crn(n, 4 * n)
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(n)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    methods = []
    for m in range(K):
        u0 = np.zeros(n); u0[0] = 1.0
        pars = S.ODESimulationParams(tspan=(0.0, 2e-3), u0=u0, save_interval=2.5e-4, low_k_cutoff="none")
        start, end = (900.0, 1300.0) if rate > 0 else (1300.0, 900.0)
        methods.append(S.VariableODESolve(pars, C.ConditionSet({"T": C.LinearGradientProfile(rate=rate * (1 + m), X_start=start, X_end=end)}),
                                          calc))
    return methods, sd, rd


MALFORMED = [
    7, [900.0, 1000.0], dict(), dict(axis="T"), dict(at=[900.0], colour=1), dict(at="hot"), dict(at=[["a"]]), dict(at=900.0),
    dict(at=np.zeros((2, 2, 2))), dict(at=np.zeros((2, 4))), dict(at=[900.0], axis="temperature"), dict(at=[900.0], axis=3),
    dict(at=[900.0], axis=np.zeros((2, 9))), dict(at=[900.0], axis=np.zeros((3, 9, 1))), dict(at=[900.0], axis=["a", "b"]),
    dict(at=[900.0], mode="clamp"), dict(at=[900.0], mode=1), dict(at=[900.0], fill="x"), dict(at=[900.0], fill=None),
    dict(at=[900.0], t_min="soon"), dict(at=[900.0], t_min=float("nan")), dict(at=[True, False]),
]


@pytest.mark.parametrize("resample", MALFORMED, ids=range(len(MALFORMED)))
def test_solve_network_ensemble_refuses_a_malformed_resample_before_the_device(no_handle, resample):
    methods, sd, rd = _methods()
    with pytest.raises(ValueError):
        S.solve_network_ensemble(methods, sd, rd, resample=resample)


def test_solve_network_ensemble_refuses_cooling_and_unordered_event_axes_before_the_device(no_handle):
    methods, sd, rd = _methods(rate=-1e5)
    with pytest.raises(ValueError, match="negate"):
        S.solve_network_ensemble(methods, sd, rd, resample=dict(axis="T", at=[1000.0, 1100.0]))
    methods, sd, rd = _methods()
    with pytest.raises(ValueError, match="increase strictly"):
        S.solve_network_ensemble(methods, sd, rd, resample=dict(axis="T", at=[1100.0, 1000.0]), events=dict(level=0.5))
    # a well-formed dict gets as far as the handle
    with pytest.raises(AssertionError, match="a handle was constructed"):
        S.solve_network_ensemble(methods, sd, rd, resample=dict(axis="T", at=[1000.0, 1100.0], mode="hold", fill=0.0, t_min=0.0))


def test_binding_refuses_malformed_blocks(no_handle):
    h = object.__new__(capi.HipNetwork)
    h._h, h.n, h.nr, h.index_base = None, 3, 2, 0
    u, x, xq = np.zeros((2, 4, 3)), np.arange(4.0), np.array([0.5])
    for kw in (dict(u=np.zeros((4, 3))), dict(u=np.zeros((2, 4, 5))), dict(x=np.arange(5.0)), dict(x=np.zeros((3, 4))),
               dict(xq=np.zeros((3, 2))), dict(xq=np.zeros((2, 2, 1))), dict(seg_n=[1, 2, 3]), dict(mode="clamp")):
        a = dict(dict(u=u, x=x, xq=xq), **kw)
        with pytest.raises(ValueError):
            h.resample_segmented(a.pop("u"), a.pop("x"), a.pop("xq"), **a)
    with pytest.raises(ValueError, match="store"):
        h.ensemble_resample(x, xq, store=False, download=False)


class _Stored:
    """Stands in for a capi.HipNetwork that holds a stored ensemble of 3 members on a 5-row grid: records every call."""
    n, index_base = 2, 0

    def __init__(self):
        self.calls = []

    def ensemble_size(self):
        return 3, 5, self.n, np.array([5, 3, 0], np.int64)

    def ensemble_resample(self, x, xq, **kw):
        self.calls.append((np.array(x), np.array(xq), kw))
        return np.zeros((3, np.shape(xq)[-1], self.n)) if kw["download"] else None


def test_resample_ensemble_on_a_handle_hands_over_axis_queries_and_row_begin():
    t = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    h = _Stored()
    rs = S.resample_ensemble(h, t, [0.5, 0.1, 2.0], axis="t", mode="hold", fill=1.5, t_min=0.2)
    (x, xq, kw), = h.calls
    assert np.array_equal(x, t) and xq.tolist() == [0.5, 0.1, 2.0] and kw == dict(mode="hold", fill=1.5, row_begin=1, store=True, download=False)
    assert rs.u is None and rs.jc.tolist() == [[2, -1, -2], [2, -1, -2], [-3, -3, -3]]
    assert rs.covered.tolist() == [[True] * 3, [True] * 3, [False] * 3] and rs.n_covered.tolist() == [3, 3, 0] and rs.t_min == 0.2
    rs = S.resample_ensemble(h, t, [0.0, 0.5, 1.0, 1.5], axis="t_rel", store=False)
    x, xq, kw = h.calls[-1]
    assert x.shape == (3, 5) and np.array_equal(x[0], t) and np.array_equal(x[1], t / 0.5) and kw["download"] and not kw["store"]
    assert rs.u.shape == (3, 4, 2) and rs.jc.tolist() == [[0, 2, 4, -2], [0, 1, 2, -2], [-3] * 4] and rs.n_covered.tolist() == [3, 3, 0]
    ax = np.stack([t, t[::-1], t])      # member 1's axis decreases over its saved rows
    with pytest.raises(ValueError, match="negate"):
        S.resample_ensemble(h, t, [0.5], axis=ax)
    ax[1] = [0.0, 1.0, 2.0, 1.0, 0.0]   # ... and here only past them
    assert S.resample_ensemble(h, t, [0.5], axis=ax).jc.tolist() == [[2], [1], [-3]]
    for bad in (dict(axis="T"), dict(axis=np.zeros(4)), dict(axis=np.zeros((2, 5))), dict(mode="x"), dict(t_min="x")):
        with pytest.raises(ValueError):
            S.resample_ensemble(h, t, [0.5], **bad)
    with pytest.raises(ValueError, match="save grid"):
        S.resample_ensemble(h, t[:4], [0.5])


def test_resample_solution_refuses_what_it_cannot_read(no_handle):
    sd = S.SpeciesData.from_names(["A", "B", "C"])
    rd = S.RxData(2, [[1], [1]], [[2], [3]], [[1], [1]], [[1], [1]])
    t = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    out = lambda u: S.ODESolveOutput(sd, rd, S.ODESolution(t, u, "Success"), None, None, None, None)
    with pytest.raises(ValueError, match="no saved states"):
        S.resample_solution(out(None), [0.5])
    full = out(np.arange(15.0).reshape(5, 3))
    for kw in (dict(axis="T"), dict(axis="t_rel"), dict(axis=np.zeros(4)), dict(axis=t[::-1]), dict(mode="x"), dict(at=[[0.5]])):
        with pytest.raises(ValueError):
            S.resample_solution(full, **dict(dict(at=[0.5]), **kw))
    with pytest.raises(AssertionError, match="a handle was constructed"):
        S.resample_solution(full, [0.5])
