"""GPU tests of the Sobol pass over synthetic Saltelli blocks (kin_members_sobol and its device form; no solve is needed)
against sobol_cases.py: every column within the derived gates of the extended-precision restatement, chosen columns bit for
bit against the replayed sum order, the exact zeros and the NaN placement of the edge rules, weights, species selections,
repeats and every status code.

Shapes: N = 5 (below one wavefront's lanes) and 70 (across 64); M around the split over the eight wavefronts and its
multiples; P = 1, 3, the kernel's chunk of inputs and one more (a second workgroup row)."""
import ctypes

import numpy as np
import pytest

import member_stats_cases as mc
import sobol_cases as sc
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu
CHUNK = sc.SB_CHUNK
MS = (1, 2, 7, 8, 9, 63, 64, 65, 257)
DESIGNS = [(M, 3) for M in MS] + [(M, P) for M in (9, 65) for P in (1, CHUNK, CHUNK + 1)]
SHAPES = [(N, L, M, P) for N in (5, 70) for L in (1, 3) for (M, P) in DESIGNS]
OUTPUTS = ("first", "total", "mean", "var")

_handles = {}


def handle(N):
    if N not in _handles:
        _handles[N] = capi.HipNetwork(*mc.chain_network(N))
    return _handles[N]


def check_against_reference(got, ref, label=""):
    assert got["count"] == ref["count"], label
    for k in OUTPUTS:
        assert sc.within(got[k], ref[k], ref["gate_" + k]), (label, k, sc.worst(got[k], ref[k], ref["gate_" + k]))


def replay_columns(u, M, P, L, N, w=None):
    """At most 16 columns for the bit-for-bit replay: first, last, the lanes around 64, each row's large-mean and plain column."""
    want = {0, sc.SP_PLAIN, 63, 64, 65, N - 1, N, L * N - 1, L * N - 2} | {j * N + s for j in range(L) for s in (sc.SP_BIG, sc.SP_PLAIN)}
    fin = set(sc.finite_columns(u, M, P, w).tolist())
    return sorted(c for c in want if c in fin)[:16]


def check_against_replay(got, u, M, P, L, N, w=None, label=""):
    cols = replay_columns(u, M, P, L, N, w)
    assert len(cols) >= 3
    rep = sc.replay_sobol(u, M, P, w=w, columns=cols)
    for k in ("first", "total"):
        assert sc.same_bits_or_zero(got[k].reshape(L * N, P)[cols], rep[k]), (label, k, mc.mismatches(got[k].reshape(L * N, P)[cols], rep[k]))
    for k in ("mean", "var"):
        assert sc.same_bits_or_zero(got[k].ravel()[cols], rep[k]), (label, k, mc.mismatches(got[k].ravel()[cols], rep[k]))


@pytest.mark.parametrize("N,L,M,P", SHAPES)
def test_indices(N, L, M, P):
    h, u = handle(N), sc.block(M, P, L, N)
    got, ref = h.members_sobol(u, M, P), sc.ref_sobol(u, M, P)
    assert got["first"].shape == got["total"].shape == (L, N, P) and got["mean"].shape == got["var"].shape == (L, N)
    check_against_reference(got, ref)
    check_against_replay(got, u, M, P, L, N)
    # the constant column: exact zeros, V itself exactly 0.0
    assert all(np.all(got[k][:, sc.SP_CONST] == 0.0) for k in ("first", "total", "var"))
    if M < 2:
        assert np.all(got["first"] == 0.0) and np.all(got["total"] == 0.0)
    else:
        # NaN exactly where the rule says: the whole column for a NaN in A, the one input for a NaN in AB_p
        nan = np.zeros((L, N, P), bool)
        nan[0, sc.SP_NAN_A] = True
        nan[L - 1, sc.SP_NAN_AB, sc.nan_input(P)] = True
        assert np.array_equal(np.isnan(got["first"]), nan) and np.array_equal(np.isnan(got["total"]), nan)
        finite = got["first"][~nan]
        assert np.all(np.isfinite(finite)) and np.all(np.isfinite(got["total"][~nan]))
    nan0 = np.zeros((L, N), bool)
    nan0[0, sc.SP_NAN_A] = True
    assert np.array_equal(np.isnan(got["mean"]), nan0) and np.array_equal(np.isnan(got["var"]), nan0)
    # every finite gate is small: the comparison above is not about centring
    fin = sc.finite_columns(u, M, P)
    assert ref["gate_first"].reshape(L * N, P)[fin].max() < 1e-9 and ref["gate_total"].reshape(L * N, P)[fin].max() < 1e-9


@pytest.mark.parametrize("M,P", [(9, 3), (65, 3), (65, CHUNK + 1)])
def test_weights(M, P):
    N, L = 70, 3
    h, u = handle(N), sc.block(M, P, L, N)
    got = h.members_sobol(u, M, P, w=np.zeros(M, np.int32))
    assert got["count"] == 0 and all(np.all(got[k] == 0.0) for k in OUTPUTS)
    # a 0/1 mask: the bits of the compacted block (sample 0, which holds the NaNs, is among the dropped)
    keep = np.arange(M) % 3 != 0
    uc, Mc = sc.compacted(u, M, P, keep)
    masked, packed = h.members_sobol(u, M, P, w=keep.astype(np.int32)), h.members_sobol(uc, Mc, P)
    assert masked["count"] == packed["count"] == Mc
    for k in OUTPUTS:
        assert masked[k].tobytes() == packed[k].tobytes(), k
    assert not np.isnan(masked["first"]).any()
    check_against_replay(masked, u, M, P, L, N, w=keep.astype(np.int32), label="mask")
    # one participant: n < 2
    one = np.zeros(M, np.int32); one[M - 1] = 1
    got = h.members_sobol(u, M, P, w=one)
    assert got["count"] == 1 and np.all(got["first"] == 0.0) and np.all(got["total"] == 0.0)
    check_against_reference(got, sc.ref_sobol(u, M, P, w=one), "one")
    # multiplicities 0, 1, 3 (a bootstrap replicate's shape), NaN sample in and out
    for first in (0, 3):
        w = np.array([0, 1, 3], np.int32)[(np.arange(M) * 7 + 1) % 3]
        w[0] = first
        got = h.members_sobol(u, M, P, w=w)
        check_against_reference(got, sc.ref_sobol(u, M, P, w=w), f"multiplicities, w[0] = {first}")
        check_against_replay(got, u, M, P, L, N, w=w, label="multiplicities")
    # one sample of weight 2 alone: n = 2, the indices are no longer zero by rule
    two = np.zeros(M, np.int32); two[1] = 2
    check_against_reference(h.members_sobol(u, M, P, w=two), sc.ref_sobol(u, M, P, w=two), "two")
    bad = np.ones(M, np.int32); bad[M // 2] = -1
    with pytest.raises(capi.KineticaHipError) as e:
        h.members_sobol(u, M, P, w=bad)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG


@pytest.mark.parametrize("M,P", [(9, 3), (65, CHUNK + 1)])
def test_species_selection_equals_the_columns_of_the_full_call(M, P):
    N, L = 70, 3
    h, u = handle(N), sc.block(M, P, L, N)
    full = h.members_sobol(u, M, P)
    for sp in ([0, 1, 2, 3, 4, 63, 64, 65, 69], [69, 4, 64, 0, 4], [63]):
        got = h.members_sobol(u, M, P, species=sp)
        assert got["first"].shape == (L, len(sp), P) and got["mean"].shape == (L, len(sp))
        for k in OUTPUTS:
            assert sc.same_bits_or_zero(got[k], full[k][:, sp]), (sp, k)
    assert h.members_sobol(u, M, P, species=[])["first"].shape == (L, 0, P)
    one = capi.HipNetwork(*mc.chain_network(N, index_base=1), index_base=1)      # ids in the base the handle was created with
    got = one.members_sobol(u, M, P, species=[70, 1, 65])
    one.close()
    for k in OUTPUTS:
        assert sc.same_bits_or_zero(got[k], full[k][:, [69, 0, 64]]), k


def test_repeated_calls_are_bit_identical():
    N, L, M, P = 70, 3, 65, CHUNK + 1
    h, u = handle(N), sc.block(M, P, L, N)
    w = np.array([0, 1, 3], np.int32)[np.arange(M) % 3]
    base = h.members_sobol(u, M, P, w=w)
    h.members_sobol(sc.block(9, 3, 1, N), 9, 3)      # another shape in between: the staging buffers are reused
    for _ in range(3):
        again = h.members_sobol(u, M, P, w=w)
        assert all(base[k].tobytes() == again[k].tobytes() for k in OUTPUTS)


def test_device_entry_equals_the_host_entry():
    import torch
    N, L, M, P = 70, 3, 65, CHUNK + 1
    h, u = handle(N), sc.block(M, P, L, N)
    w = np.array([0, 1, 3], np.int32)[np.arange(M) % 3]
    sp = [4, 63, 2, 0]
    d_u = torch.tensor(u, dtype=torch.float64, device="cuda:0")
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda:0")
    d = dict(first=new(L, N, P), total=new(L, N, P), mean=new(L, N), var=new(L, N))
    ds = dict(first=new(L, len(sp), P), total=new(L, len(sp), P), mean=new(L, len(sp)), var=new(L, len(sp)))
    d_only = new(L, N, P)
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    h.members_sobol_dev(M, P, L, d_u.data_ptr(), **{"d_" + k: v.data_ptr() for k, v in d.items()}, w=w)
    h.members_sobol_dev(M, P, L, d_u.data_ptr(), **{"d_" + k: v.data_ptr() for k, v in ds.items()}, species=sp)
    h.members_sobol_dev(M, P, L, d_u.data_ptr(), d_total=d_only.data_ptr())      # one output wanted: nothing else is written
    torch.cuda.synchronize()
    host, host_sp = h.members_sobol(u, M, P, w=w), h.members_sobol(u, M, P, species=sp)
    for k in OUTPUTS:
        assert d[k].cpu().numpy().tobytes() == host[k].tobytes(), k
        assert ds[k].cpu().numpy().tobytes() == host_sp[k].tobytes(), k
    assert d_only.cpu().numpy().tobytes() == h.members_sobol(u, M, P)["total"].tobytes()


def test_status_codes():
    N, L, M, P = 5, 3, 4, 2
    h, u = handle(N), np.ascontiguousarray(sc.block(M, P, L, N))
    L_ = capi.lib()
    PD, pd = ctypes.POINTER(ctypes.c_double), lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    p32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    null = PD()
    S1, ST, mu, V = np.empty((L, N, P)), np.empty((L, N, P)), np.empty((L, N)), np.empty((L, N))
    call = lambda M_=M, P_=P, L_n=L, u_=pd(u), w=None, sp=None, ns=0, outs=(pd(S1), pd(ST), pd(mu), pd(V)): \
        L_.kin_members_sobol(h.handle, M_, P_, L_n, u_, w, sp, ns, *outs)
    assert call() == capi.KIN_OK
    assert call(outs=(null, null, null, pd(V))) == capi.KIN_OK and V.tobytes() == h.members_sobol(u, M, P)["var"].tobytes()
    INV = capi.KIN_ERR_INVALID_ARG
    assert call(M_=0) == INV and call(M_=-3) == INV and call(P_=0) == INV and call(P_=-1) == INV and call(L_n=-1) == INV
    assert call(u_=null) == INV and call(outs=(null, null, null, null)) == INV
    assert call(w=p32(np.array([1, 1, -2, 1], np.int32))) == INV
    for bad in ([5], [-1], [0, 7]):
        assert call(sp=p64(np.array(bad, np.int64)), ns=len(bad)) == INV
    assert call(sp=p64(np.array([0], np.int64)), ns=-1) == INV
    assert L_.kin_members_sobol(None, M, P, L, pd(u), None, None, 0, pd(S1), pd(ST), pd(mu), pd(V)) == INV
    # M (P + 2) members beyond 32-bit member indices (nothing is read: L = 0)
    assert call(M_=1 << 30, P_=2, L_n=0, u_=null) == capi.KIN_ERR_UNSUPPORTED
    assert call(L_n=0, u_=null) == capi.KIN_OK      # an empty block is an empty result
    # the device entry: the same checks before anything is enqueued
    assert L_.kin_members_sobol_dev(h.handle, M, P, L, None, None, None, 0, None, None, None, None, None) == INV
    assert L_.kin_members_sobol_dev(h.handle, 0, P, L, None, None, None, 0, None, None, None, 1, None) == INV
    # no stored ensemble
    assert L_.kin_ensemble_sobol(h.handle, M, P, None, None, 0, pd(S1), pd(ST), pd(mu), pd(V)) == capi.KIN_ERR_STATE
    with pytest.raises(capi.KineticaHipError) as e:
        h.ensemble_sobol(M, P)
    assert e.value.code == capi.KIN_ERR_STATE
    # the binding's own checks
    with pytest.raises(ValueError):
        h.members_sobol(u, M, P + 1)
    with pytest.raises(ValueError):
        h.members_sobol(u, M, P, w=np.ones(M))
    with pytest.raises(ValueError):
        h.members_sobol(u, M, P, w=np.ones(M + 1, np.int32))
