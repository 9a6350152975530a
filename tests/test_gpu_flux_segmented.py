"""GPU tests of the segmented flux pass (kin_flux_segmented_dev / kin_flux_segmented): S segments of up to L states,
flux[s][r] = sum over j < seg_n[s] of w[s][j] rate_r(u[s][j]), against math.fsum of the CPU oracle's per-state rates. The device
entry runs on buffers made by torch, as in test_gpu_flux.py. Rows j >= seg_n[s] hold NaN everywhere (states, weights,
temperatures) and out-of-range row indices: they must never be read.

Bounds (derived, not measured; EPS = 2^-53):
  flux, k given     |got - ref| <= (L + 8) EPS sum_j |w_j rate_j| + 1e-300   (<= 4 roundings per term on either side, <= L - 1
                                                                              additions)
  temperature form  + (2 |Ea_r / (R T)| + 16) EPS per term against oracle.arrhenius; none against capi.arrhenius_eval, the
                    device's own function: there the bits must agree
  two finite sums   twice the bound (LDS paths against the gather path)"""
import math

import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
RGAS = 8.314462618
S_, L_ = 5, 7
SEG_N = np.array([7, 0, 3, 1, 5], np.int64)
MODES = ["shared", "per_state", "k_row", "T", "T_kmax"]


def _states(n, S, L, seg_n, seed=0):
    rng = np.random.default_rng(seed)
    U = 10.0 ** rng.uniform(-12, 0, (S, L, n))
    U[0, 0] = 0.0; U[0, 0, 0] = 1.0                             # the solve's one-hot u0
    if L > 1:
        U[0, 1, rng.random(n) < 0.3] = 0.0                      # exact zeros
    if L > 2:
        U[0, 2, rng.choice(n, min(5, n), replace=False)] = -1e-14   # what an implicit solve leaves behind
    for s in range(S):
        U[s, seg_n[s]:] = np.nan                                # never read
    return U


def _weights(S, L, seg_n, seed=1):
    w = np.random.default_rng(seed).normal(size=(S, L))
    w[:, ::5] = 0.0
    w[:, 1::3] = -np.abs(w[:, 1::3])
    for s in range(S):
        w[s, seg_n[s]:] = np.nan
    return w


def seg_dev(h, U, seg_n=None, k=None, k_row=None, T=None, w=None):
    """kin_flux_segmented_dev on torch buffers; the output starts as NaN."""
    import torch
    dev = "cuda:0"
    S, L = U.shape[:2]
    t = lambda a, dt: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    d_u, d_k, d_T, d_w = t(U, torch.float64), t(k, torch.float64), t(T, torch.float64), t(w, torch.float64)
    d_n, d_row = t(seg_n, torch.int64), t(k_row, torch.int64)
    d_f = torch.full((S, h.nr), float("nan"), dtype=torch.float64, device=dev)
    p = lambda x: 0 if x is None else x.data_ptr()
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    h.flux_segmented_dev(S, L, p(d_u), p(d_f), d_seg_n=p(d_n), d_k=p(d_k), d_k_row=p(d_row), d_T=p(d_T), d_w=p(d_w),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_f.cpu().numpy()


class Case:
    """One network: handle, oracle, S x L states (NaN past seg_n), the inputs of every rate-constant source and the
    oracle's per-state rates of each (computed once)."""

    def __init__(self, net, Ea, A, S=S_, L=L_, seg_n=SEG_N):
        self.net, self.Ea, self.A, self.S, self.L, self.seg_n = net, Ea, A, S, L, np.asarray(seg_n, np.int64)
        self.h = capi.HipNetwork.from_flat(net)
        self.on = orc.OracleNetwork.from_flat(net)
        self.U = _states(net.n_species, S, L, self.seg_n)
        self.w = _weights(S, L, self.seg_n)
        rng = np.random.default_rng(2)
        R = net.n_reactions
        self.k0 = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
        self.K = self.k0[None, None, :] * rng.uniform(0.5, 2.0, (S, L, 1)) * rng.uniform(0.9, 1.1, (S, L, R))
        self.K3 = self.K[0, :3].copy()
        self.row3 = rng.integers(0, 3, (S, L)).astype(np.int64)
        self.T = rng.uniform(600.0, 1200.0, (S, L))
        for s in range(S):                                       # what lies past a segment's rows is never looked at
            self.row3[s, self.seg_n[s]:] = 1 << 40
            self.T[s, self.seg_n[s]:] = np.nan
        self._ref = {}

    def k_of(self, mode, s, j):
        if mode == "shared":
            return self.k0
        if mode == "per_state":
            return self.K[s, j]
        if mode == "k_row":
            return self.K3[self.row3[s, j]]
        return orc.arrhenius(self.Ea, self.A, self.T[s, j], k_max=1e12 if mode == "T_kmax" else None)

    def ref_rates(self, mode):
        """rates[S][L][R] of the oracle (zeros past seg_n: those rows do not exist)."""
        if mode not in self._ref:
            r = np.zeros((self.S, self.L, self.net.n_reactions))
            for s in range(self.S):
                for j in range(self.seg_n[s]):
                    r[s, j] = self.on.rates(self.k_of(mode, s, j), self.U[s, j])
            self._ref[mode] = r
        return self._ref[mode]

    def source(self, mode):
        h = self.h
        if mode == "shared":
            h.set_rates(self.k0)
            return {}
        if mode == "per_state":
            return dict(k=self.K.reshape(self.S * self.L, -1))
        if mode == "k_row":
            return dict(k=self.K3, k_row=self.row3)
        h.set_arrhenius(self.Ea, self.A, k_max=1e12 if mode == "T_kmax" else None)
        return dict(T=self.T)

    def call(self, mode, w=None):
        return seg_dev(self.h, self.U, self.seg_n, w=w, **self.source(mode))

    def bound(self, mode, w):
        """(fsum reference [S][R], bound [S][R])"""
        ref = self.ref_rates(mode)
        fref, bound = np.zeros((self.S, ref.shape[2])), np.zeros((self.S, ref.shape[2]))
        for s in range(self.S):
            n = self.seg_n[s]
            terms = (np.ones(n) if w is None else w[s, :n])[:, None] * ref[s, :n]
            fref[s] = [math.fsum(terms[:, r]) for r in range(ref.shape[2])]
            ex = 0.0
            if mode.startswith("T") and n:
                ex = (2.0 * np.abs(self.Ea[None, :] / (RGAS * self.T[s, :n, None])) + 16.0) * EPS
            bound[s] = (self.L + 8) * EPS * np.abs(terms).sum(axis=0) + (ex * np.abs(terms)).sum(axis=0) + 1e-300
        return fref, bound

    def check(self, mode, flux, w, what=""):
        fref, bound = self.bound(mode, w)
        err = np.abs(flux - fref)
        print(f"segmented flux {what}{mode}: max err/bound {np.max(err / bound):.3f}")
        assert np.all(np.isfinite(flux))
        assert np.all(err <= bound)
        for s in np.nonzero(self.seg_n == 0)[0]:
            assert np.all(flux[s] == 0.0)


_cases = {}


def _case(key):
    if key not in _cases:
        _cases[key] = Case(*synthetic_crn(*key))
    return _cases[key]


@pytest.fixture(scope="module")
def small():
    return _case((300, 1500))


@pytest.fixture(scope="module")
def odd():
    return _case((301, 1500))          # N odd: rows are not all 16-byte aligned - the staging without prefetch (path 1)


@pytest.fixture(scope="module")
def mid():
    return _case((1000, 5000))


@pytest.mark.parametrize("lds", ["1", "0"])
def test_a_to_b_hand_values(lds, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_LDS", lds)
    h = capi.HipNetwork.from_flat(from_lists(2, [[(0, 1)]], [[(1, 1)]]))        # R = 1: a half-filled pair
    nan = np.nan
    U = np.array([[[1.0, 0.0], [0.5, 0.5], [0.25, 0.75], [0.125, 0.875]],
                  [[nan, nan]] * 4,
                  [[2.0, 0.0], [4.0, 1.0], [nan, nan], [nan, nan]]])
    w = np.array([[1.0, 2.0, -4.0, 8.0], [nan] * 4, [0.5, 0.25, nan, nan]])
    seg_n = np.array([4, 0, 2], np.int64)
    k = np.array([[0.5]])
    hand = np.array([[0.5 * (1.0 * 1.0 + 2.0 * 0.5 - 4.0 * 0.25 + 8.0 * 0.125)], [0.0], [0.5 * (0.5 * 2.0 + 0.25 * 4.0)]])
    row = np.zeros((3, 4), np.int64)
    assert np.array_equal(seg_dev(h, U, seg_n, k=k, k_row=row, w=w), hand)
    h.set_rates(k[0])
    assert np.array_equal(seg_dev(h, U, seg_n, w=w), hand)
    assert np.array_equal(h.flux_segmented(U, seg_n=seg_n, w=w), hand)
    # no weights: plain sums; no seg_n: every segment has L rows (the NaN rows then show, as they must)
    plain = np.array([[0.5 * 1.875], [0.0], [0.5 * 6.0]])
    assert np.array_equal(seg_dev(h, U, seg_n), plain)
    full = seg_dev(h, U)
    assert full[0, 0] == plain[0, 0] and np.isnan(full[1, 0]) and np.isnan(full[2, 0])
    h.close()


@pytest.mark.parametrize("lds", ["1", "0"])
def test_special_stoichiometries_hand_values(lds, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_LDS", lds)
    # 2A -> B (no 1/2!), A -> 2B, inert collider A + M -> B + M, product = reactant species (N = 3: odd, path 1)
    reacs = [[(0, 2)], [(0, 1)], [(0, 1), (2, 1)], [(1, 1)]]
    prods = [[(1, 1)], [(1, 2)], [(1, 1), (2, 1)], [(0, 1), (1, 1)]]
    h = capi.HipNetwork.from_flat(from_lists(3, reacs, prods))
    k = np.array([3.0, 0.5, 2.0, 0.25])
    rows = np.array([[0.5, 0.25, 4.0], [2.0, 0.0, 1.0], [0.125, 8.0, 0.5]])
    hand = np.array([[3.0 * 0.25, 0.5 * 0.5, 2.0 * 0.5 * 4.0, 0.25 * 0.25],
                     [3.0 * 4.0, 0.5 * 2.0, 2.0 * 2.0 * 1.0, 0.0],
                     [3.0 * 0.015625, 0.5 * 0.125, 2.0 * 0.125 * 0.5, 0.25 * 8.0]])
    U = np.stack([rows, rows[::-1]])                       # S = 2, L = 3
    U[1, 2] = np.nan
    w = np.array([[1.0, 2.0, -4.0], [0.5, -1.0, np.nan]])
    seg_n = np.array([3, 2], np.int64)
    h.set_rates(k)
    want = np.stack([(w[0][:, None] * hand).sum(axis=0), 0.5 * hand[2] - 1.0 * hand[1]])
    assert np.array_equal(seg_dev(h, U, seg_n, w=w), want)
    h.close()


@pytest.mark.parametrize("mode", MODES)
def test_every_source_matches_oracle(small, mode):
    small.check(mode, small.call(mode, w=small.w), small.w)


@pytest.mark.parametrize("mode", ["per_state", "T_kmax"])
def test_null_weights_are_ones(small, mode):
    small.check(mode, small.call(mode), None, "w = NULL ")


@pytest.mark.parametrize("mode", MODES)
def test_odd_species_count(odd, mode):
    odd.check(mode, odd.call(mode, w=odd.w), odd.w, "N = 301 ")


@pytest.mark.parametrize("mode", MODES)
def test_gather_path_matches_oracle_and_lds_path(small, mode, monkeypatch):
    f_lds = small.call(mode, w=small.w)
    monkeypatch.setenv("KIN_FLUX_LDS", "0")
    f_g = small.call(mode, w=small.w)
    small.check(mode, f_g, small.w, "gather ")
    # both paths sit within the bound of the same reference: they agree within twice the bound
    _, bound = small.bound(mode, small.w)
    print("gather == lds bit for bit:", np.array_equal(f_g, f_lds))
    assert np.all(np.abs(f_g - f_lds) <= 2 * bound)


def test_three_parts_ragged_last(mid, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_ROWS", "1")      # 2 500 pairs over 1 024 threads: parts of 1 024, 1 024 and 452 pairs
    for mode in ("per_state", "T_kmax"):
        mid.check(mode, mid.call(mode, w=mid.w), mid.w, "3 parts ")


def test_one_part_of_four_rows(mid):
    for mode in ("per_state", "k_row", "shared", "T"):       # 2 500 pairs: 4 rows (k given: 1 part), 2 rows (T: 2 parts)
        mid.check(mode, mid.call(mode, w=mid.w), mid.w)


def test_odd_reaction_count_half_filled_pair(small, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_ROWS", "2")
    R = small.net.n_reactions - 1
    c = Case(small.net.subset(np.arange(R)), small.Ea[:R], small.A[:R], S=3, L=4, seg_n=[4, 2, 3])
    for mode in MODES:
        c.check(mode, c.call(mode, w=c.w), c.w, "R odd ")
    c.h.close()


def test_reuse_changes_no_bit(small):
    """One temperature per segment, handed over three ways: the kernel evaluates the law once per segment (T_rows), loads one
    row once per segment (k_row = s), or loads a row for every state (one k row per state: every key differs)."""
    h, S, L = small.h, small.S, small.L
    h.set_arrhenius(small.Ea, small.A, k_max=1e12)
    Ts = np.array([900.0, 950.0, 950.0, 1100.0, 733.25])        # segments 1 and 2: equal keys in adjacent segments
    krows = np.stack([capi.arrhenius_eval(small.Ea, small.A, float(T), k_max=1e12) for T in Ts])
    U, w = small.U, small.w
    f_T = seg_dev(h, U, small.seg_n, T=np.repeat(Ts[:, None], L, axis=1), w=w)
    f_row = seg_dev(h, U, small.seg_n, k=krows, k_row=np.repeat(np.arange(S)[:, None], L, axis=1), w=w)
    f_each = seg_dev(h, U, small.seg_n, k=np.repeat(krows, L, axis=0), w=w)
    assert np.array_equal(f_T, f_row) and np.array_equal(f_row, f_each)
    assert np.any(f_T[0] != 0.0)
    # a key that changes in the middle of a segment (rows 0-2 at one temperature, 3-6 at another), again three ways
    T2 = np.repeat(Ts[:, None], L, axis=1); T2[:, 3:] += 125.0
    k2 = np.stack([capi.arrhenius_eval(small.Ea, small.A, float(T) + 125.0, k_max=1e12) for T in Ts])
    both = np.concatenate([krows, k2])                                          # rows 0 .. S-1 and S .. 2S-1
    row2 = np.repeat(np.arange(S)[:, None], L, axis=1); row2[:, 3:] += S
    g_T = seg_dev(h, U, small.seg_n, T=T2, w=w)
    g_row = seg_dev(h, U, small.seg_n, k=both, k_row=row2, w=w)
    g_each = seg_dev(h, U, small.seg_n, k=both[row2.ravel()], w=w)
    assert np.array_equal(g_T, g_row) and np.array_equal(g_row, g_each)
    assert not np.array_equal(g_T[0], f_T[0])                                   # (segment 0 has rows past the change)
    assert np.array_equal(g_T[3], f_T[3])                                       # (segment 3 has one row: before the change)
    # equal keys in adjacent segments: segment 2 loads for itself - it is what it is alone
    alone = seg_dev(h, U[2:3], small.seg_n[2:3], T=np.full((1, L), Ts[2]), w=w[2:3])
    assert np.array_equal(alone[0], f_T[2])
    # against the oracle: the temperature form's bound
    small.T, keep = np.repeat(Ts[:, None], L, axis=1), small.T
    small._ref.pop("T_kmax", None)
    try:
        small.check("T_kmax", f_T, w, "one T per segment ")
    finally:
        small.T = keep
        small._ref.pop("T_kmax", None)


@pytest.mark.parametrize("mode", ["per_state", "k_row", "T_kmax"])
def test_segments_are_independent_and_repeatable(mid, mode):
    src = mid.source(mode)
    L = mid.L
    full = seg_dev(mid.h, mid.U, mid.seg_n, w=mid.w, **src)
    assert np.array_equal(full, seg_dev(mid.h, mid.U, mid.seg_n, w=mid.w, **src))
    for s in range(mid.S):
        one = {}
        if "T" in src:
            one["T"] = src["T"][s:s + 1]
        if "k_row" in src:
            one["k"], one["k_row"] = src["k"], src["k_row"][s:s + 1]
        elif "k" in src:
            one["k"] = src["k"][s * L:(s + 1) * L]
        alone = seg_dev(mid.h, mid.U[s:s + 1], mid.seg_n[s:s + 1], w=mid.w[s:s + 1], **one)
        assert np.array_equal(alone[0], full[s]), s
    # another order of the segments: every segment keeps its bits
    perm = np.array([3, 0, 4, 2, 1])
    srcp = {}
    if "T" in src:
        srcp["T"] = src["T"][perm]
    if "k_row" in src:
        srcp["k"], srcp["k_row"] = src["k"], src["k_row"][perm]
    elif "k" in src:
        srcp["k"] = src["k"].reshape(mid.S, L, -1)[perm].reshape(mid.S * L, -1)
    assert np.array_equal(seg_dev(mid.h, mid.U[perm], mid.seg_n[perm], w=mid.w[perm], **srcp), full[perm])


@pytest.mark.parametrize("mode", MODES)
def test_host_entry_equals_device_entry(small, mode):
    src = small.source(mode)
    dev = seg_dev(small.h, small.U, small.seg_n, w=small.w, **src)
    # the host entry validates the row indices of the rows a segment has - and only those (the others hold 2^40 here)
    host = small.h.flux_segmented(small.U, seg_n=small.seg_n, w=small.w, **src)
    assert np.array_equal(host, dev)


def test_zero_sizes_write_zeros(small):
    h, n, R = small.h, small.net.n_species, small.net.n_reactions
    h.set_rates(small.k0)
    f = h.flux_segmented(np.empty((3, 0, n)))                    # L = 0
    assert f.shape == (3, R) and np.all(f == 0.0)
    f = h.flux_segmented(np.empty((0, 4, n)))                    # S = 0: nothing to write
    assert f.shape == (0, R)
    f = seg_dev(h, np.empty((2, 0, n)))                          # the device entry overwrites the NaN fill
    assert f.shape == (2, R) and np.all(f == 0.0)
    f = h.flux_segmented(np.full((2, 3, n), np.nan), seg_n=np.zeros(2, np.int64))      # every segment empty
    assert np.all(f == 0.0)


def test_error_statuses():
    net, Ea, A = synthetic_crn(50, 200, seed=3)
    h = capi.HipNetwork.from_flat(net)
    Lb = capi.lib()
    U = np.ones((2, 3, 50)); K = np.ones((6, 200)); T = np.full((2, 3), 800.0)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    INV, STATE = capi.KIN_ERR_INVALID_ARG, capi.KIN_ERR_STATE
    assert code(lambda: h.flux_segmented(U)) == STATE                                       # no rates at all
    assert code(lambda: h.flux_segmented(U, T=T)) == STATE                                  # T without Arrhenius parameters
    for fn in (h.ensemble_size, h.ensemble_max, lambda: h.ensemble_dot(np.ones(50)), h.ensemble_flux):
        assert code(fn) == STATE                                                            # no stored ensemble
    h.set_arrhenius(Ea, A)
    assert code(lambda: h.flux_segmented(U, k=K, T=T)) == INV                               # both k and T
    assert code(lambda: h.flux_segmented(U, k_row=np.zeros((2, 3), np.int64))) == INV       # k_row without k
    assert code(lambda: h.flux_segmented(U, k=K, k_row=np.array([[0, 1, 6], [2, 3, 4]]))) == INV      # row index out of range
    assert code(lambda: h.flux_segmented(U, k=K, k_row=np.array([[0, -1, 1], [2, 3, 4]]))) == INV
    # ... but not in a row the segment does not have
    f = h.flux_segmented(U, seg_n=np.array([2, 3]), k=K, k_row=np.array([[0, 1, 6], [2, 3, 4]]))
    assert f.shape == (2, 200) and np.all(f[0] == 2.0) and np.all(f[1] == 3.0)
    assert code(lambda: h.flux_segmented(U, k=K[:5])) == INV                                # k_row == NULL needs n_k_rows == S L
    assert code(lambda: h.flux_segmented(U, seg_n=np.array([4, 0]), k=K)) == INV            # seg_n outside [0, L]
    assert code(lambda: h.flux_segmented(U, seg_n=np.array([0, -1]), k=K)) == INV
    PD, P64 = capi._pd, capi._p64
    out = np.empty((2, 200))
    assert Lb.kin_flux_segmented(h.handle, -1, 3, None, PD(U), PD(K), 6, None, None, None, PD(out)) == INV       # S < 0
    assert Lb.kin_flux_segmented(h.handle, 2, -1, None, PD(U), PD(K), 6, None, None, None, PD(out)) == INV       # L < 0
    assert Lb.kin_flux_segmented(h.handle, 2, 3, None, PD(U), PD(K), 6, None, None, None, None) == INV           # null output
    assert Lb.kin_flux_segmented_dev(h.handle, -1, 3, None, None, None, None, None, None, None, None) == INV
    assert Lb.kin_flux_segmented_dev(h.handle, 2, -1, None, None, None, None, None, None, None, None) == INV
    assert Lb.kin_flux_segmented_dev(h.handle, 2, 3, None, None, None, None, None, None, None, None) == INV      # null output
    assert Lb.kin_ensemble_max(h.handle, None) == INV and Lb.kin_ensemble_flux(h.handle, None, None, 0, None, None, None) == INV
    assert Lb.kin_ensemble_dot(h.handle, None, None) == INV
    h.close()
