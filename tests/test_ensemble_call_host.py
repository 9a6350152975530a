"""CPU tests of the ensemble call layer's host parts (kinetica_jl_amd/csrc/solver.hpp through tests/native/ensemble_call_host.cpp):
EnsembleCall::block, the thread route's member assignment, the finishing layer's host part (finish_members) and the member-thread
runner. tests/test_gpu_ensemble*.py run the routes that are built on them."""
import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64

import numpy as np
import pytest

from kinetica_jl_amd import capi
from tests import res_host

P64, P32, PD = POINTER(c_int64), POINTER(c_int32), POINTER(c_double)
BLOCK_OUT = ("K", "u0", "k", "T", "stop_ptr", "node_ptr", "tstops", "T_stops", "t_nodes", "T_nodes", "Ea", "A", "out_t", "out_u", "n_saved",
             "retcodes", "stats", "cap", "m_tstops", "m_T_stops", "m_n", "m_dEa", "m_dA", "m_t_nodes")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _block(K, N, R, m0, n, j, stop_ptr=None, node_ptr=None):
    pars = capi.KinParams(tspan0=0.0, tspan1=1.0, abstol=1e-10, reltol=1e-8, solve_chunks=1, solve_chunkstep=0.5, maxiters=1000, save_interval=0.25)
    out = np.zeros(len(BLOCK_OUT), np.int64)
    res_host.lib().ens_host_block(ctypes.byref(pars), K, N, R, _p(stop_ptr, P64), _p(node_ptr, P64), m0, n, j, _p(out, P64))
    return dict(zip(BLOCK_OUT, (int(v) for v in out)))


K, N, R, BLOCK = 5, 3, 4, 2
PTR = np.concatenate([[0], np.cumsum([1, 3, 2, 1, 4])]).astype(np.int64)   # per-member counts 1, 3, 2, 1, 4


@pytest.mark.parametrize("form", ["stops", "nodes", "static"])
def test_block_advances_every_per_member_pointer_and_leaves_the_shared_ones(form):
    ptrs = dict(stops=dict(stop_ptr=PTR), nodes=dict(node_ptr=PTR), static={})[form]
    cap = _block(K, N, R, 0, K, 0, **ptrs)["cap"]
    assert cap == 5   # 0 : 0.25 : 0.5 per chunk, two chunks
    for m0 in range(0, K, BLOCK):
        n = min(BLOCK, K - m0)   # (the last block is ragged: one member)
        for j in range(n):
            b, whole = _block(K, N, R, m0, n, j, **ptrs), _block(K, N, R, 0, K, m0 + j, **ptrs)
            assert b["K"] == n
            # every per-member input and output: base + m0 * its stride
            strides = dict(u0=N, out_u=cap * N, n_saved=1, retcodes=1, stats=1)
            strides.update(dict(stops=dict(stop_ptr=1, Ea=R, A=R), nodes=dict(node_ptr=1, Ea=R, A=R), static=dict(k=R, T=1))[form])
            for name in ("u0", "k", "T", "stop_ptr", "node_ptr", "Ea", "A", "out_u", "n_saved", "retcodes", "stats"):
                assert b[name] == (m0 * strides[name] if name in strides else -1), name
            # the shared inputs and the call-wide output stay where they are (-1: the form has none)
            for name in ("tstops", "T_stops", "t_nodes", "T_nodes", "out_t"):
                assert b[name] == whole[name] and b[name] in (0, -1), name
            # the member's own stops, parameters and profile are those of the same absolute member of the whole call
            for name in ("m_tstops", "m_T_stops", "m_n", "m_dEa", "m_dA", "m_t_nodes"):
                assert b[name] == whole[name], name
            if form == "stops":
                assert (b["m_tstops"], b["m_T_stops"], b["m_n"]) == (PTR[m0 + j], PTR[m0 + j], PTR[m0 + j + 1] - PTR[m0 + j])
            if form == "nodes":
                assert b["m_t_nodes"] == PTR[m0 + j]
            if form != "static":
                assert b["m_dEa"] == b["m_dA"] == (m0 + j) * R


@pytest.mark.parametrize("K,limit", [(1, 12), (12, 12), (13, 12), (5, 2), (25, 12)])
def test_thread_share_assigns_every_member_once_and_evenly(K, limit):
    out, thread_of = np.zeros(2, np.int64), np.full(K, -1, np.int64)
    res_host.lib().ens_host_thread_share(K, limit, _p(out, P64), _p(thread_of, P64))
    per, threads = int(out[0]), int(out[1])
    assert per == -(-K // limit) and threads == -(-K // per) and 1 <= threads <= limit
    assert np.array_equal(thread_of, np.arange(K) % threads)    # member m on thread m mod threads: each member exactly once
    loads = np.bincount(thread_of, minlength=threads)
    assert loads.sum() == K and loads.min() >= 1 and loads.max() - loads.min() <= 1 and loads.max() == per


def _finish(n_saved, cap, host_times=True, outputs=True):
    K = len(n_saved)
    ns_in = np.array(n_saved, np.int64); rc_in = np.arange(10, 10 + K, dtype=np.int32); steps = np.arange(100, 100 + K, dtype=np.int64)
    times = (np.arange(K)[:, None] * 1000.0 + np.arange(cap)[None, :] + 1.0).copy()   # member m's times: 1000 m + 1, + 2, ...
    out_t = np.full(cap, np.nan)
    ns, rc, st = np.full(K, -7, np.int64), np.full(K, -7, np.int32), (capi.KinStats * K)()
    rows = np.zeros(K, np.int64)
    best = res_host.lib().ens_host_finish(K, cap, _p(ns_in, P64), _p(rc_in, P32), _p(steps, P64), _p(times if host_times else None, PD),
                                          _p(out_t, PD), *((_p(ns, P64), _p(rc, P32), st) if outputs else (None, None, None)), _p(rows, P64))
    return dict(best=best, rows=rows, out_t=out_t, n_saved=ns, retcodes=rc, steps=np.array([s.n_steps for s in st]), times=times)


def test_finish_fills_the_members_outputs_and_picks_the_first_of_the_furthest():
    f = _finish([2, 4, 4, 1], cap=5)
    assert f["best"] == 1                                   # members 1 and 2 tie: the first
    assert np.array_equal(f["rows"], [2, 4, 4, 1]) and np.array_equal(f["n_saved"], [2, 4, 4, 1])
    assert np.array_equal(f["retcodes"], [10, 11, 12, 13]) and np.array_equal(f["steps"], [100, 101, 102, 103])
    assert np.array_equal(f["out_t"], np.concatenate([f["times"][1, :4], [0.0]]))   # the NaN prefill is gone: zeros past n_saved


def test_finish_clamps_n_saved_to_the_grid():
    f = _finish([3, 9, 5], cap=5)
    assert np.array_equal(f["rows"], [3, 5, 5]) and np.array_equal(f["n_saved"], [3, 5, 5]) and f["best"] == 1
    assert np.array_equal(f["out_t"], f["times"][1])


def test_finish_zeroes_the_whole_of_out_t_when_nobody_saved_a_row():
    f = _finish([0, 0], cap=4)
    assert f["best"] == 0 and np.array_equal(f["out_t"], np.zeros(4))


def test_finish_without_host_times_writes_the_tail_only():
    """the resident route's times are on the device: the head is left for finish_ensemble's download"""
    f = _finish([1, 3, 2], cap=5, host_times=False)
    assert f["best"] == 1 and np.isnan(f["out_t"][:3]).all() and np.array_equal(f["out_t"][3:], [0.0, 0.0])


def test_finish_skips_null_outputs():
    f = _finish([2, 3], cap=4, outputs=False)
    assert f["best"] == 1 and np.array_equal(f["rows"], [2, 3])
    assert (f["n_saved"] == -7).all() and (f["retcodes"] == -7).all()   # (the arrays the call was not given: untouched)
    best = res_host.lib().ens_host_finish(2, 4, _p(np.array([2, 3], np.int64), P64), _p(np.zeros(2, np.int32), P32), _p(np.zeros(2, np.int64), P64),
                                          None, None, None, None, None, _p(np.zeros(2, np.int64), P64))   # ... and no out_t either
    assert best == 1


@pytest.mark.parametrize("throw_at", [-1, 0, 2])
def test_runner_joins_every_thread_and_rethrows_the_first_member_error(throw_at):
    n = 6
    ran, never = np.zeros(n, np.int32), np.zeros(1, np.int64)
    msg = ctypes.create_string_buffer(256)
    code = res_host.lib().ens_host_runner(n, throw_at, _p(ran, P32), _p(never, P64), msg, len(msg))
    expect = np.ones(n, np.int32)
    if throw_at >= 0:
        expect[throw_at] = 0
    assert np.array_equal(ran, expect)          # every other member ran, those after the failing one included, on threads of their own
    assert never[0] == 0
    if throw_at < 0:
        assert code == 0
    else:
        assert code == capi.KIN_ERR_DEVICE and msg.value == b"ensemble member failed: boom"
