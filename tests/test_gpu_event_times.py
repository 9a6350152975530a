"""GPU tests of the event-time pass on caller-given blocks: kin_events_segmented (host arrays) and kin_events_segmented_dev
(buffers made by torch) over every case of event_cases.py, every (kind, direction, start) combination and every row_begin of
the case, bit for bit against event_cases.ref_events (a NaN `never` by its place). The launcher's knobs are forced to parts of
PART_ROWS rows on two wavefronts - so that a wavefront walks several parts and a crossing's interval spans two of them - and
left at their defaults: the bytes are the same. Then the status of every refused argument."""
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
                    assert ec.same_bits(got[q], ref[q]), (case["id"], kw, q, name, got[q], ref[q])
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
