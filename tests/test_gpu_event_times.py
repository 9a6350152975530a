"""GPU tests of the event-time pass on caller-given blocks: kin_events_segmented (host arrays) and kin_events_segmented_dev
(buffers made by torch) over every case of event_cases.py, every (kind, direction, start) combination and every row_begin of
the case, bit for bit against event_cases.ref_events (a NaN `never` by its place). The launcher's knobs are forced to parts of
PART_ROWS rows on two wavefronts - so that a wavefront walks several parts and a crossing's interval spans two of them - and
left at their defaults: the bytes are the same. Then the status of every refused argument.

Beyond the first cases (event_cases.py): NaN rows inside a segment, where only u_peak is specified and is compared - the
header's fmax rule, which ref_events restates; zeros of both signs, whose peak is compared with the restatement by value, byte
for byte between the decompositions, and with the header's rule (+0.0 if any row holds it); and LATE_PEAK, whose second walk
passes over whole parts (tests/test_event_cases.py shows on a replay of the decomposition that it does). The longest generated
case, LATE_PEAK and the zeros run under ec.KNOBS: 1, 4, 8 and 16 wavefronts with parts of 1, 3, 5 and 6 rows and of the
launcher's own size. tests/test_pass_plans_host.py has event_plan itself.

Measured on an MI355X: u_peak of the zero columns -0 +0 -0.., +0 -0 -0.., -0.. +0, +0.., -0.., -0.. +0 -0.. is +0.0 in all
but the all-negative one under every setting; from row_begin 1 the second column is all -0.0 and gives -0.0.

Mutation check (value-only changes on a scratch build, one at a time, nothing of it kept): which tests of this file fail, and
what the four modules that launch these kernels did before this change (test_gpu_event_times, test_gpu_resample,
test_gpu_ensemble_event_times, test_gpu_ensemble_resample: 38 tests; no other module reaches event_kernels.hip).
  d the combine of the wavefronts' peaks uses bv = first ? v : (v > bv ? v : bv): 4 of the 20 tests fail -
    every_case_bit_for_bit on nan-rows and signed-zeros, every_knob_setting on signed-zeros, and
    signed_zeros_and_nan_rows_follow_the_stated_rules.
    Before: MISSED - all 38 passed.
  e the second walk passes over a part with p1 <= skip_below + 1: 13 fail - every_case_bit_for_bit on the nine generated cases
    and on late-peak, every_knob_setting on its three.
    Before: 9 of the 13 tests of test_gpu_event_times failed (every generated case); the other three modules passed.
  f event_walk leaves out the guarded tail of an in-flight group (the rows of a part past its last whole group of
    EVENT_ROWS_IN_FLIGHT; the part's first group is kept whole, so that the mutated kernel still has a peak row to read the
    time of): 3 fail - every_knob_setting on its three cases, each first under one wavefront with parts of 5 rows.
    Before: MISSED - all 38 passed (every part of the forced and of the default plan is a multiple of four rows or the
    segment's last).
  The mutations of resample_kernels.hip (a, b, c: test_gpu_resample.py) leave every test of this file passing."""
import numpy as np
import pytest

import event_cases as ec
import member_stats_cases as mc
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
SENTINEL = -9.75e99      # what the device entry's outputs hold before the call: every entry must be written


def network(N):
    """A handle with N species (the pass never looks at the reactions)."""
    return capi.HipNetwork(*(mc.chain_network(N) if N > 1 else (1, [0, 1], [0], [1], [0, 1], [0], [1])))


def events_dev(h, u, t, level, seg_n=None, want=ec.OUTPUTS, **kw):
    """kin_events_segmented_dev on torch buffers; returns the dict of the host entry."""
    import torch
    dev = torch.device("cuda")
    S, L, N = u.shape
    dt = lambda a, ty: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=ty, device=dev)
    d_u, d_t, d_l, d_n = dt(u, torch.float64), dt(t, torch.float64), dt(level, torch.float64), dt(seg_n, torch.int64)
    out = {q: torch.full((S, N), SENTINEL, dtype=torch.float64, device=dev) for q in want}
    p = lambda x: 0 if x is None or x.numel() == 0 else x.data_ptr()
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the stream it is handed
    h.events_segmented_dev(S, L, p(d_u), p(d_t), d_level=p(d_l), d_seg_n=p(d_n), t_per_segment=t.ndim == 2,
                           **{"d_" + q: p(out[q]) for q in want}, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return {q: v.cpu().numpy() for q, v in out.items()}


def _force(monkeypatch, on):
    for name, value in ec.FORCED.items():
        if on:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("case", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_every_case_bit_for_bit(case, monkeypatch):
    u, t, seg_n, never = case["u"], case["t"], case["seg_n"], case["never"]
    h = network(u.shape[2])
    checked = 0
    for kind, direction, start in ec.COMBOS:
        level = case["levels"][kind]
        for rb in case["row_begins"]:
            kw = dict(kind=kind, direction=direction, start=start, row_begin=rb, never=never)
            ref = ec.ref_events(u, t, level, seg_n=seg_n, **kw)
            _force(monkeypatch, True)
            host = h.events_segmented(u, t, level=level, seg_n=seg_n, **kw)
            dev = events_dev(h, u, t, level, seg_n=seg_n, **kw)
            _force(monkeypatch, False)
            plain = h.events_segmented(u, t, level=level, seg_n=seg_n, **kw)
            for q in ec.OUTPUTS:
                for name, got in (("host", host), ("device", dev), ("default plan", plain)):
                    assert ec.agree(case, q, got[q], ref[q]), (case["id"], kw, q, name, got[q], ref[q])
                    # forced and default knobs, host and device entry: the same bytes, the sign of a zero included
                    assert ec.judged(case, q, got[q]).tobytes() == ec.judged(case, q, host[q]).tobytes(), (case["id"], kw, q, name)
            checked += 1
    assert checked == len(ec.COMBOS) * len(case["row_begins"])
    # a second call repeats the bits; outputs that are not asked for are not needed
    kw = dict(kind="of_peak", direction="fall", start="peak", row_begin=case["row_begins"][0], never=never)
    a = h.events_segmented(u, t, level=case["levels"]["of_peak"], seg_n=seg_n, **kw)
    b = h.events_segmented(u, t, level=case["levels"]["of_peak"], seg_n=seg_n, **kw)
    assert all(a[q].tobytes() == b[q].tobytes() for q in ec.OUTPUTS)
    only = h.events_segmented(u, t, seg_n=seg_n, row_begin=kw["row_begin"], never=never, want=("t_peak",))
    assert list(only) == ["t_peak"] and only["t_peak"].tobytes() == a["t_peak"].tobytes()
    peaks = events_dev(h, u, t, None, seg_n=seg_n, want=("u_peak",), row_begin=kw["row_begin"], never=never)
    assert peaks["u_peak"].tobytes() == a["u_peak"].tobytes()
    h.close()


@pytest.mark.parametrize("case", ec.MATRIX_CASES, ids=[c["id"] for c in ec.MATRIX_CASES])
def test_every_knob_setting_gives_the_same_bytes(case, monkeypatch):
    """ec.KNOBS - 1, 4, 8 and 16 wavefronts with parts of 1, 3, 5 and 6 rows and of the launcher's own size, and the forced
    setting - over every combination at a row_begin of 0 and one inside the segment, through the host and the device entry:
    the restatement's bits, and the same bytes under every setting."""
    u, t, seg_n, never = case["u"], case["t"], case["seg_n"], case["never"]
    h = network(u.shape[2])
    checked = 0
    for kind, direction, start in ec.COMBOS:
        level = case["levels"][kind]
        for rb in ec.MATRIX_ROW_BEGINS[case["id"]]:
            kw = dict(kind=kind, direction=direction, start=start, row_begin=rb, never=never)
            ref = ec.ref_events(u, t, level, seg_n=seg_n, **kw)
            first = None
            for knobs in ec.KNOBS:
                for name in ("KIN_EVENT_WAVES", "KIN_EVENT_PART_ROWS"):
                    monkeypatch.delenv(name, raising=False)
                for name, value in knobs.items():
                    monkeypatch.setenv(name, value)
                host = h.events_segmented(u, t, level=level, seg_n=seg_n, **kw)
                dev = events_dev(h, u, t, level, seg_n=seg_n, **kw)
                first = first or host
                for q in ec.OUTPUTS:
                    for name, got in (("host", host), ("device", dev)):
                        assert ec.agree(case, q, got[q], ref[q]), (case["id"], kw, knobs, q, name, got[q], ref[q])
                        assert ec.judged(case, q, got[q]).tobytes() == ec.judged(case, q, first[q]).tobytes(), (case["id"], kw, knobs, q, name)
                checked += 1
    assert checked == len(ec.COMBOS) * 2 * len(ec.KNOBS)
    h.close()


def test_signed_zeros_and_nan_rows_follow_the_stated_rules():
    """What the header says of a peak among zeros of both signs and of NaN rows, on the device under the forced knobs: +0.0 if any
    row holds +0.0, its first row's time; the maximum of the rows that are numbers, NaN only where every row is NaN."""
    by_id = {c["id"]: c for c in ec.CASES}
    for case in (by_id["signed-zeros"], by_id["nan-rows"]):
        u, t = case["u"], case["t"]
        h = network(u.shape[2])
        for rb in case["row_begins"]:
            got = h.events_segmented(u, t, row_begin=rb)
            rows = u[0, rb:]
            with np.errstate(invalid="ignore"):
                expect = np.fmax.reduce(rows, axis=0)
            if case.get("zeros"):
                expect = np.where(np.signbit(rows).all(axis=0), -0.0, 0.0)
                assert np.all(got["t_peak"] == t[rb])
                print("signed zeros, row_begin", rb, "u_peak sign bits", np.signbit(got["u_peak"][0]).tolist())
            assert ec.same_bits(got["u_peak"][0], expect), (case["id"], rb, got["u_peak"], expect)
        h.close()


def test_a_segment_does_not_depend_on_its_neighbours():
    case = ec.CASES[6]
    u, t, seg_n = case["u"], case["t"], case["seg_n"]
    h = network(u.shape[2])
    kw = dict(level=case["levels"]["of_peak"], kind="of_peak", direction="fall", start="peak")
    full = h.events_segmented(u, t, seg_n=seg_n, **kw)
    for s in (0, 3, 4):
        alone = h.events_segmented(u[s:s + 1], t, seg_n=seg_n[s:s + 1], **kw)
        assert all(ec.same_bits(alone[q][0], full[q][s]) for q in ec.OUTPUTS), s
    h.close()


def test_empty_calls_write_the_empty_segment_values():
    h = network(5)
    r = h.events_segmented(np.zeros((3, 0, 5)), np.zeros(0), level=1.0, never=-2.0)
    assert np.all(r["u_peak"] == 0.0) and np.all(r["t_peak"] == -2.0) and np.all(r["t_cross"] == -2.0) and r["u_peak"].shape == (3, 5)
    r = h.events_segmented(np.zeros((0, 4, 5)), np.arange(4.0), level=1.0)
    assert all(r[q].shape == (0, 5) for q in ec.OUTPUTS)
    r = events_dev(h, np.zeros((2, 0, 5)), np.zeros(0), np.ones(5), never=7.0)
    assert np.all(r["u_peak"] == 0.0) and np.all(r["t_peak"] == 7.0) and np.all(r["t_cross"] == 7.0)
    h.close()


def test_statuses_of_refused_arguments():
    N, S, L = 5, 2, 4
    h = network(N)
    lib = capi.lib()
    u, t, level = np.ones((S, L, N)), np.arange(float(L)), np.ones(N)
    seg = np.array([L, 2], np.int64)
    out = [np.full((S, N), SENTINEL) for _ in range(3)]
    pd, p64 = capi._pd, capi._p64
    nan = float("nan")

    def call(S_=S, L_=L, seg_n=seg, u_=u, t_=t, per=0, lev=level, kind=0, direction=1, start=0, rb=0, outs=(0, 1, 2)):
        o = [pd(out[i]) if i in outs else None for i in range(3)]
        return lib.kin_events_segmented(h.handle, S_, L_, p64(seg_n), pd(u_), pd(t_), per, pd(lev), kind, direction, start, rb, nan, *o)

    assert call() == capi.KIN_OK
    good = [o.copy() for o in out]
    bad_t = np.array([0.0, 1.0, 1.0, 2.0])
    late = np.array([0.0, 1.0, 3.0, 2.0])          # not increasing in rows 2, 3: segment 0 reads them, segment 1 does not
    per_t = np.stack([t, late])
    refused = [
        dict(S_=-1), dict(L_=-1), dict(u_=None), dict(t_=None), dict(outs=()), dict(lev=None), dict(direction=0), dict(kind=3),
        dict(kind=-1), dict(start=2), dict(start=-1), dict(rb=-1), dict(seg_n=np.array([L + 1, 0], np.int64)),
        dict(seg_n=np.array([-1, 0], np.int64)), dict(t_=bad_t), dict(t_=late), dict(t_=np.stack([late, t]), per=1),
        dict(t_=np.array([0.0, nan, 2.0, 3.0])),
    ]
    for kw in refused:
        assert call(**kw) == capi.KIN_ERR_INVALID_ARG, kw
        assert lib.kin_last_error(h.handle)
    for o, g in zip(out, good):
        assert o.tobytes() == g.tobytes()            # a refused call writes nothing
    # what is allowed: no level without t_cross, times that are bad only where no row is read, a direction by its sign alone
    assert call(lev=None, outs=(0, 1)) == capi.KIN_OK
    assert call(t_=per_t, per=1) == capi.KIN_OK
    assert call(t_=late, rb=3, seg_n=np.array([L, 2], np.int64)) == capi.KIN_OK
    assert call(direction=-7) == capi.KIN_OK and call(rb=L + 5) == capi.KIN_OK
    # the device entry: the same argument rules (it reads neither seg_n nor t)
    dev = lambda **kw: events_dev(h, u, t, level, **kw)
    for kw in (dict(direction=0), dict(kind=5), dict(start=7), dict(row_begin=-1), dict(want=())):
        with pytest.raises(capi.KineticaHipError) as e:
            dev(**kw)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG, kw
    # the stored forms without a stored ensemble / solution
    for name, args in (("kin_ensemble_events", (pd(t), 0)), ("kin_solution_events", ())):
        st = getattr(lib, name)(h.handle, *args, pd(level), 0, 1, 0, 0, nan, pd(out[0]), pd(out[1]), pd(out[2]))
        assert st == capi.KIN_ERR_STATE, name
    assert lib.kin_events_segmented(None, S, L, None, pd(u), pd(t), 0, pd(level), 0, 1, 0, 0, nan, pd(out[0]), None, None) == capi.KIN_ERR_INVALID_ARG
    # the handle is as it was: the next call gives the first call's bits
    assert call() == capi.KIN_OK and all(o.tobytes() == g.tobytes() for o, g in zip(out, good))
    h.close()
