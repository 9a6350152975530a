"""GPU tests of the caller-layout batched sweep (kin_rhs_batched_dev; kernels.hip: sweep_reg_kernel, sweep_gen_kernel,
sweep_lds_kernel, sweep_big_kernel and the per-state path at N >= 65535) in every instantiation and on every trip of the state
loop. Cases, inputs, references and bounds: tests/sweep_cases.py (checked without a GPU by tests/test_sweep_cases.py).

For every case: kin_sweep_plan on the live handle and the real pointers reports the instantiation the case is named after; du
starts as NaN; on the exact inputs EVERY state of every batch equals the float64 reference bit for bit (by value); on the random
inputs every entry of the sampled states (first, last, one per trip) is inside (L + 4) u S against the longdouble reference.
Batches: B = 1, grid, grid + 1, 2 grid + 3 with `grid` from the query - every state has its own u and its own k; the largest
batch shares one k row where per-state rows would exceed 150 MB (B = grid + 1 always has per-state rows). A case that reaches
its instantiation through an 8-byte offset of u, du or k is also compared with the aligned run of the same network.

Measured on one MI355X (printed at the end of the module, pytest -s; 50 tests, 30 s): largest error / bound on the random
inputs against the longdouble reference - sweep_reg_kernel 0.44, sweep_gen_kernel 0.51, sweep_lds_kernel 0.31,
sweep_big_kernel 0.44, the per-state path 0.32. Every exact-input run equals the reference bit for bit; no kernel was found
wrong. What the case list showed about the dispatch: a network with a species on both sides of a reaction is never
`adjacent` (such a reaction has no partner record), so the explicit-operand branch of sweep_big_kernel<true> and of
sweep_lds_kernel<*, true> cannot be reached; the colliders run in the <false> instantiations.

Mutation check (value-only changes, one at a time on a scratch build selected through KIN_LIB_PATH, nothing of them kept):
failing tests of this file (of 50), and what test_gpu_sweep_batches.py + the sweep tests of test_gpu_parity.py (24 tests) - the
suite's view of these kernels before - did. (a) - (c), (h) and the tiled kernel's (d): test_gpu_tiled_exact.py.
  d sweep_reg_kernel's fold of the split accumulators adds 0 for the last copy entry: 10 fail - every reg_stream_* case (the
    synthetic CRNs: n_copy > 0); the 18 pair_net cases have n_copy = 0 and pass. Before: 16 of 24 failed.
  e sweep_reg_kernel does not refresh k0 for the next state: 21 fail - every TR = 4 / 8 case (12 reg_bs*_tr4/8_*, 9 reg_stream_*);
    TR = 0 has no prefetch and passes. Before: 10 failed.
  f the ILP + 1 batch applies only ILP rows: 3 fail - reg_stream_bs256_R6500, _R8392, reg_stream_bs1024_R25576: exactly the
    cases whose plan has n_b > 0. Before: 3 failed.
  g sweep_gen_kernel does not zero a missing reverse's kr: all 5 gen_* cases fail. Before: 4 failed."""
import numpy as np
import pytest
import torch

from kinetica_jl_amd import capi
from tests import sweep_cases as sc

pytestmark = pytest.mark.gpu

RATIOS = {}          # kernel -> largest error / bound seen on the random inputs


def _buf(a, off_bytes):
    """device copy of `a` whose first element sits `off_bytes` (0 or 8) past a 16-byte aligned address; returns (owner, view)"""
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    own = torch.empty(a.size + 2, dtype=torch.float64, device="cuda")
    o = off_bytes // 8
    if own.data_ptr() % 16:
        o += 1
    v = own[o:o + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == off_bytes
    return own, v


def _run(h, case, U_, K, B, bits=None):
    """du[B][N] of the first B states through kin_rhs_batched_dev (K[R]: shared, set on the handle), and the plan of that call"""
    ub, kb, db = case.bits if bits is None else bits
    N, R = h.n, h.nr
    shared = K.ndim == 1
    if shared:
        h.set_rates(K)
    _, d_u = _buf(U_[:B], ub)
    d_k = None if shared else _buf(K[:B], kb)[1]
    own, d_du = _buf(np.full((B, N), np.nan), db)
    own.fill_(float("nan"))
    torch.cuda.synchronize()
    kp = 0 if shared else d_k.data_ptr()
    plan = h.sweep_plan(B, d_u.data_ptr(), kp, d_du.data_ptr())
    h.rhs_batched_dev(B, d_u.data_ptr(), kp, d_du.data_ptr())
    torch.cuda.synchronize()
    out = own.cpu().numpy()
    o = (d_du.data_ptr() - own.data_ptr()) // 8
    assert np.isnan(out[:o]).all() and np.isnan(out[o + B * N:]).all(), "wrote outside du"
    return out[o:o + B * N].reshape(B, N), plan


def _expect(case, plan, shared):
    e = dict(case.expect)
    if shared and case.bits[1]:          # the handle's own k row is aligned: an offset of the per-state k does not apply
        return
    assert {q: plan[q] for q in e} == e, (case.name, plan)


@pytest.mark.parametrize("name", list(sc.SWEEP_CASES))
def test_every_state_of_every_trip(name):
    case = sc.SWEEP_CASES[name]
    net, ref = sc.built("sweep", name)
    N, R = ref.N, ref.R
    h = capi.HipNetwork.from_flat(net)
    try:
        # the grid of THIS case's instantiation (its own pointer bits), from the query
        Ux1, Kx1 = sc.exact_inputs(1, N, R, 3)
        _, p1 = _run(h, case, Ux1, Kx1, 1)
        _expect(case, p1, False)
        if case.batches:
            Bs, grid = list(case.batches), max(1, min(case.batches))
        else:
            _, d = _buf(np.zeros(2 * N + 2), case.bits[0])
            _, dk = _buf(np.zeros(2 * R + 2), case.bits[1])
            _, dd = _buf(np.zeros(2 * N + 2), case.bits[2])
            grid = h.sweep_plan(10 ** 6, d.data_ptr(), dk.data_ptr(), dd.data_ptr())["grid"]
            assert grid == h.compute_units() * p1["per_cu"]
            Bs = sc.trip_batches(grid)
        Bmax, Bper = max(Bs), max(b for b in Bs if b * R * 8 <= sc.K_BYTES_MAX or b <= grid + 1)
        assert Bper >= min(grid + 1, Bmax)
        for kind in ("exact", "random"):
            gen = sc.exact_inputs if kind == "exact" else sc.random_inputs
            U_, K = gen(Bmax, N, R, 5)[0], gen(Bper, N, R, 5)[1]
            Ks = gen(1, N, R, 6, shared_k=True)[1]
            ex_per = sc.exact_rhs(ref, U_[:Bper], K) if kind == "exact" else None
            ex_sh = sc.exact_rhs(ref, U_, Ks) if kind == "exact" and Bper < Bmax else None
            for B in Bs:
                shared = B > Bper
                du, plan = _run(h, case, U_, Ks if shared else K, B)
                _expect(case, plan, shared)
                assert plan["grid"] == min(B, grid) or plan["kernel"] == "per_state"
                g = max(1, plan["grid"]) if plan["kernel"] != "per_state" else B
                if kind == "exact":
                    want = (ex_sh if shared else ex_per)[:B]
                    if not np.array_equal(du, want):
                        b, i = np.argwhere(du != want)[0]
                        raise AssertionError((name, f"B={B} state {b} (trip {b // g}) species {i}: {du[b, i]} != {want[b, i]}",
                                              f"{int((du != want).sum())} entries differ"))
                    assert np.abs(du).max() > 0
                else:
                    for b in sc.sample_states(B, g):
                        ok, ratio, worst = sc.judge_rhs(ref, Ks if shared else K[b], U_[b], du[b])
                        assert ok, (name, B, b, worst)
                        RATIOS[plan["kernel"]] = max(RATIOS.get(plan["kernel"], 0.0), ratio)
                if case.against and B == min(grid + 1, Bmax):
                    # the aligned run of the same network: another instantiation, the same values on exact inputs
                    du0, plan0 = _run(h, case, U_, K, B, bits=(0, 0, 0))
                    assert {q: plan0[q] for q in sc.SWEEP_CASES[case.against].expect} == sc.SWEEP_CASES[case.against].expect
                    if kind == "exact":
                        assert np.array_equal(du, du0)
    finally:
        h.close()


def test_doubling_k_doubles_du_exactly_in_the_general_and_large_kernels():
    """du(2 K) == 2 du(K) bit for bit on the exact inputs (test_gpu_sweep_batches has this for one register-resident case)"""
    for name in ("gen_colliders_odd_R", "big_10242_colliders", "lds_odd_N_blk"):
        case = sc.SWEEP_CASES[name]
        net, ref = sc.built("sweep", name)
        h = capi.HipNetwork.from_flat(net)
        try:
            U_, K = sc.exact_inputs(259, ref.N, ref.R, 9)
            du, _ = _run(h, case, U_, K, 259)
            du2, _ = _run(h, case, U_, 2.0 * K, 259)
            assert np.array_equal(du2, 2.0 * du) and np.abs(du).max() > 0
        finally:
            h.close()


def test_zz_report():
    """(last in the file) the largest error / bound per kernel on the random inputs, against the longdouble reference"""
    print("\nsweep error / bound:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    assert all(v <= 1.0 for v in RATIOS.values())
