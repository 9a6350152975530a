"""GPU tests of the resampling pass on caller-given blocks: kin_resample_segmented (host arrays) and kin_resample_segmented_dev
(buffers made by torch) over every case of resample_cases.py, both modes with a NaN and a finite fill and every row_begin of
the case, bit for bit against resample_cases.ref_resample in u_q, jc and w (a NaN by its place). The launcher's knobs are
forced to tiles of TILE queries on two wavefronts - a partial tile, several queries per wavefront - and left at their defaults:
the bytes are the same. A repeat gives the same bytes, nothing outside the written range is touched, and every refused
argument has its status.

Beyond the first cases: rc.SLICE_CASES have 1024, 1025, 1089 and 2049 species - one, two and three species slices
(blockIdx.y), whose brackets must be those of a call over one slice alone; rc.PLAN_CASE runs under every (tile, wavefronts)
pair of rc.PLANS, the tiles resample_plan chooses for large calls and a tile larger than its workgroup among them. Every row
that is no chord is compared byte for byte: -0.0 and NaN payloads as stored. tests/test_pass_plans_host.py has resample_plan
itself, tests/test_resample_host.py the bisection on long axes.

Mutation check (value-only changes on a scratch build, one at a time, nothing of it kept): which tests of this file fail, and
what the four modules that launch these kernels did before this change (test_gpu_resample, test_gpu_event_times,
test_gpu_ensemble_resample, test_gpu_ensemble_event_times: 38 tests; no other module reaches resample_kernels.hip).
  a launch_resample launches ceil_div(N, 2 * RESAMPLE_SLICE) slices: 6 of the 22 tests fail - every_case_bit_for_bit and
    brackets_of_a_sliced_call on the cases of 1025, 1089 and 2049 species (the sentinel is still there).
    Before: MISSED - all 38 passed.
  b the search loop of resample_kernel runs once (if (threadIdx.x < nq); the tile's later queries are left as `fill`, so that
    the mutated kernel reads no row index it has not written): 1 fails - every_plan_gives_the_same_bytes, at (256, 1).
    Before: MISSED - all 38 passed.
  c a slice >= 1 also writes jc and w, from a search that starts at row_begin + 1: 4 fail - every_case_bit_for_bit on the
    cases of 1025, 1089 and 2049 species, brackets_of_a_sliced_call on that of 2049 (which slice's write lands last is a race).
    Before: MISSED - all 38 passed.
  The mutations of event_kernels.hip (d, e, f: test_gpu_event_times.py) leave every test of this file passing."""
import numpy as np
import pytest

import member_stats_cases as mc
import resample_cases as rc
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
SENTINEL = -9.75e99      # what the device entry's outputs hold before the call: every entry must be written
GUARD = 67               # entries behind every device output that must keep the sentinel


def network(N):
    """A handle with N species (the pass never looks at the reactions)."""
    return capi.HipNetwork(*(mc.chain_network(N) if N > 1 else (1, [0, 1], [0], [1], [0, 1], [0], [1])))


def resample_dev(h, u, x, xq, seg_n=None, brackets=True, **kw):
    """kin_resample_segmented_dev on torch buffers; returns (u_q, jc, w) and checks the guards behind them."""
    import torch
    dev = torch.device("cuda")
    S, L, N = u.shape
    Q = xq.shape[-1]
    dt = lambda a, ty: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=ty, device=dev)
    d_u, d_x, d_q, d_n = dt(u, torch.float64), dt(x, torch.float64), dt(xq, torch.float64), dt(seg_n, torch.int64)
    out = torch.full((S * Q * N + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    jc = torch.full((S * Q + GUARD,), -77, dtype=torch.int32, device=dev)
    w = torch.full((S * Q + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    p = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the stream it is handed
    h.resample_segmented_dev(S, L, p(d_u), p(d_x), Q, p(d_q), p(out), d_seg_n=p(d_n), x_per_segment=x.ndim == 2,
                             xq_per_segment=xq.ndim == 2, d_jc=p(jc) if brackets else 0, d_w=p(w) if brackets else 0,
                             stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    out, jc, w = out.cpu().numpy(), jc.cpu().numpy(), w.cpu().numpy()
    assert np.all(out[S * Q * N:] == SENTINEL) and np.all(jc[S * Q:] == -77) and np.all(w[S * Q:] == SENTINEL)
    assert not np.any(out[:S * Q * N] == SENTINEL)      # every species of every slice, query and segment was written
    if brackets:
        assert not np.any(jc[:S * Q] == -77) and not np.any(w[:S * Q] == SENTINEL)
    if not brackets:
        assert np.all(jc == -77) and np.all(w == SENTINEL)
    return out[:S * Q * N].reshape(S, Q, N), jc[:S * Q].reshape(S, Q), w[:S * Q].reshape(S, Q)


def _force(monkeypatch, on):
    for name, value in rc.FORCED.items():
        if on:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)


def _same(got, ref):
    """u_q bit for bit (a NaN by its place), jc equal, w byte for byte; and every row that is no chord (w == 0: a copy, a held
    row, the fill) byte for byte: -0.0 and NaN payloads as they were stored."""
    plain = ref[2] == 0.0
    return rc.same_bits(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2].tobytes() == ref[2].tobytes() and \
        got[0][plain].tobytes() == ref[0][plain].tobytes()


@pytest.mark.parametrize("case", rc.GPU_CASES, ids=[c["id"] for c in rc.GPU_CASES])
def test_every_case_bit_for_bit(case, monkeypatch):
    u, x, xq, seg_n = case["u"], case["x"], case["xq"], case["seg_n"]
    h = network(u.shape[2])
    checked = 0
    for rb in case["row_begins"]:
        for req in rc.REQUESTS:
            kw = dict(req, row_begin=rb)
            ref = rc.ref_resample(u, x, xq, seg_n=seg_n, **kw)
            _force(monkeypatch, True)
            host = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True, **kw)
            dev = resample_dev(h, u, x, xq, seg_n=seg_n, **kw)
            _force(monkeypatch, False)
            plain = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True, **kw)
            for name, got in (("host", host), ("device", dev), ("default plan", plain)):
                assert _same(got, ref), (case["id"], kw, name)
            # default and forced knobs: the same bytes, NaN payloads included
            assert all(a.tobytes() == b.tobytes() for a, b in zip(host, plain)) and all(a.tobytes() == b.tobytes() for a, b in zip(host, dev))
            checked += 1
    assert checked == len(rc.REQUESTS) * len(case["row_begins"])
    # a second call repeats the bytes; the brackets are optional
    kw = dict(mode="hold", fill=-7.5, row_begin=case["row_begins"][1])
    a = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True, **kw)
    b = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True, **kw)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    only = h.resample_segmented(u, x, xq, seg_n=seg_n, **kw)
    assert only.tobytes() == a[0].tobytes()
    bare = resample_dev(h, u, x, xq, seg_n=seg_n, brackets=False, **kw)
    assert bare[0].tobytes() == a[0].tobytes()
    h.close()


@pytest.mark.parametrize("case", rc.SLICE_CASES, ids=[c["id"] for c in rc.SLICE_CASES])
def test_brackets_of_a_sliced_call_are_those_of_a_single_slice_call(case, monkeypatch):
    """jc and w are written once, by slice 0: a call over the first 64 species alone, on the same axes, gives the same bytes;
    and its u_q is the sliced call's first 64 columns."""
    u, x, xq, seg_n = case["u"], case["x"], case["xq"], case["seg_n"]
    h, h64 = network(u.shape[2]), network(64)
    for on in (True, False):
        _force(monkeypatch, on)
        for rb in case["row_begins"]:
            kw = dict(mode="hold", fill=0.125, row_begin=rb, seg_n=seg_n)
            full = h.resample_segmented(u, x, xq, want_brackets=True, **kw)
            dev = resample_dev(h, u, x, xq, **kw)
            one = h64.resample_segmented(u[:, :, :64], x, xq, want_brackets=True, **kw)
            ref = rc.ref_resample(u[:, :, :64], x, xq, **kw)
            assert _same(one, ref), (case["id"], rb)
            for got in (full, dev):
                assert np.array_equal(got[1], one[1]) and got[2].tobytes() == one[2].tobytes(), (case["id"], rb, on)
                assert got[0][:, :, :64].tobytes() == one[0].tobytes(), (case["id"], rb, on)
    h.close(); h64.close()


def test_every_plan_gives_the_same_bytes(monkeypatch):
    """rc.PLAN_CASE under every (tile, wavefronts) pair of rc.PLANS: the restatement's bits in u_q, jc and w, and the same bytes
    under every plan, through the host and the device entry."""
    case = rc.PLAN_CASE
    u, x, xq, seg_n = case["u"], case["x"], case["xq"], case["seg_n"]
    assert xq.shape[-1] == 70 and u.shape[2] == 65
    h = network(u.shape[2])
    checked = 0
    for rb in case["row_begins"]:
        for req in rc.REQUESTS:
            kw = dict(req, row_begin=rb)
            ref = rc.ref_resample(u, x, xq, seg_n=seg_n, **kw)
            first = None
            for tile, waves in rc.PLANS:
                monkeypatch.setenv("KIN_RESAMPLE_TILE_QUERIES", str(tile))
                monkeypatch.setenv("KIN_RESAMPLE_WAVES", str(waves))
                host = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True, **kw)
                dev = resample_dev(h, u, x, xq, seg_n=seg_n, **kw)
                first = first or host
                for name, got in (("host", host), ("device", dev)):
                    assert _same(got, ref), (kw, tile, waves, name)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, first)), (kw, tile, waves, name)
                checked += 1
    assert checked == len(case["row_begins"]) * len(rc.REQUESTS) * len(rc.PLANS)
    h.close()


def test_resampling_at_the_own_axis_returns_the_rows_and_a_segment_does_not_depend_on_its_neighbours():
    case = rc.CASES[5]
    u, x, xq, seg_n = case["u"], case["x"], case["xq"], case["seg_n"]
    h = network(u.shape[2])
    s = 4                                            # a segment of L rows with its own axis (a plateau inside, the last two rows equal)
    own = h.resample_segmented(u[s:s + 1], x[s], x[s])
    first = [int(np.argmax(x[s] == v)) for v in x[s]]      # on a plateau the first row that holds the value
    assert own[0].tobytes() == u[s, first].tobytes()
    full = h.resample_segmented(u, x, xq, seg_n=seg_n, want_brackets=True)
    for s in (0, 3, 4):
        alone = h.resample_segmented(u[s:s + 1], x[s:s + 1], xq[s:s + 1], seg_n=seg_n[s:s + 1], want_brackets=True)
        assert all(rc.same_bits(a[0], f[s]) for a, f in zip(alone, full)), s
    h.close()


def test_empty_calls_write_nothing():
    h = network(5)
    r = h.resample_segmented(np.zeros((3, 0, 5)), np.zeros(0), np.array([1.0, 2.0]), fill=-2.0, want_brackets=True)
    assert r[0].shape == (3, 2, 5) and np.all(r[0] == -2.0) and np.all(r[1] == rc.NONE) and np.all(r[2] == 0.0)      # (empty segments)
    assert h.resample_segmented(np.zeros((0, 4, 5)), np.arange(4.0), np.array([1.0])).shape == (0, 1, 5)
    assert h.resample_segmented(np.zeros((2, 4, 5)), np.arange(4.0), np.zeros(0)).shape == (2, 0, 5)
    out, jc, w = resample_dev(h, np.zeros((2, 4, 5)), np.arange(4.0), np.zeros(0))
    assert out.size == 0 and jc.size == 0 and w.size == 0
    h.close()


def test_statuses_of_refused_arguments():
    N, S, L, Q = 5, 2, 4, 3
    h = network(N)
    lib = capi.lib()
    u, x, xq = np.arange(float(S * L * N)).reshape(S, L, N), np.arange(float(L)), np.array([0.5, 7.0, 2.0])
    seg = np.array([L, 2], np.int64)
    out, jc, w = np.full((S, Q, N), SENTINEL), np.full((S, Q), -77, np.int32), np.full((S, Q), SENTINEL)
    pd, p64, p32 = capi._pd, capi._p64, capi._p32
    nan = float("nan")

    def call(S_=S, L_=L, seg_n=seg, u_=u, x_=x, per=0, Q_=Q, xq_=xq, qper=0, mode=0, rb=0, out_=out):
        return lib.kin_resample_segmented(h.handle, S_, L_, p64(seg_n), pd(u_), pd(x_), per, Q_, pd(xq_), qper, mode, nan, rb, pd(out_),
                                          p32(jc), pd(w))

    assert call() == capi.KIN_OK
    good = [a.copy() for a in (out, jc, w)]
    assert jc.tolist() == [[1, -2, 2], [1, -2, -2]]
    late = np.array([0.0, 1.0, 3.0, 2.0])          # decreasing in rows 2, 3: segment 0 reads them, segment 1 does not
    refused = [dict(S_=-1), dict(L_=-1), dict(Q_=-1), dict(rb=-1), dict(u_=None), dict(x_=None), dict(xq_=None), dict(out_=None),
               dict(mode=2), dict(mode=-1), dict(seg_n=np.array([L + 1, 0], np.int64)), dict(seg_n=np.array([-1, 0], np.int64)),
               dict(x_=late), dict(x_=np.stack([late, x]), per=1), dict(x_=np.array([0.0, nan, 2.0, 3.0]))]
    for kw in refused:
        assert call(**kw) == capi.KIN_ERR_INVALID_ARG, kw
        assert lib.kin_last_error(h.handle)
    for kw in (dict(S_=1 << 31, L_=0, Q_=0, seg_n=None), dict(L_=1 << 31, S_=0, seg_n=None), dict(Q_=1 << 31, S_=0, seg_n=None)):
        assert call(**kw) == capi.KIN_ERR_UNSUPPORTED, kw
    for a, g in zip((out, jc, w), good):
        assert a.tobytes() == g.tobytes()            # a refused call writes nothing
    # what is allowed: an axis that is bad only where no row is read, a plateau, a row_begin past every row
    assert call(x_=np.stack([x, late]), per=1) == capi.KIN_OK and call(x_=late, rb=3) == capi.KIN_OK
    assert call(x_=np.array([0.0, 1.0, 1.0, 1.0])) == capi.KIN_OK and call(rb=L + 5) == capi.KIN_OK and call(mode=1) == capi.KIN_OK
    # the device entry: the same argument rules (it reads neither seg_n nor the axis)
    for kw in (dict(mode=5), dict(row_begin=-1)):
        with pytest.raises(capi.KineticaHipError) as e:
            resample_dev(h, u, x, xq, **kw)
        assert e.value.code == capi.KIN_ERR_INVALID_ARG, kw
    with pytest.raises(capi.KineticaHipError) as e:
        h.resample_segmented_dev(S, L, 0, 0, Q, 0, 0)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG
    # the stored forms without a stored ensemble / solution
    assert lib.kin_ensemble_resample(h.handle, pd(x), 0, Q, pd(xq), 0, 0, nan, 0, 0, pd(out)) == capi.KIN_ERR_STATE
    assert lib.kin_ensemble_resample(h.handle, pd(x), 0, Q, pd(xq), 0, 0, nan, 0, 1, None) == capi.KIN_ERR_STATE
    assert lib.kin_solution_resample(h.handle, None, Q, pd(xq), 0, nan, 0, pd(out)) == capi.KIN_ERR_STATE
    # the handle is as it was: the next call gives the first call's bytes
    assert call() == capi.KIN_OK and all(a.tobytes() == g.tobytes() for a, g in zip((out, jc, w), good))
    h.close()
