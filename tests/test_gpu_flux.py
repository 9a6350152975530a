"""GPU tests of the reaction-flux pass (kin_flux_batched / kin_flux_batched_dev) against the CPU oracle's per-state rates in
float64; flux is compared against math.fsum of w_b rate_b.

Bounds (derived, not measured):
  per-state rates   |got - ref| <= 4 2^-53 |ref| + 1e-300                      (a rate is two products, on either side)
  flux, k given     |got - ref| <= (B + 8) 2^-53 sum_b |w_b rate_b| + 1e-300   (<= 4 roundings per term on either side, B - 1
                                                                                additions in any order)
  temperature form  + (2 |Ea_r / (R T_b)| + 16) 2^-53 per term                 (device-side Arrhenius: the bound smoke() and
                                                                                test_rate_table_matches_oracle apply)"""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists, synthetic_crn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
TOL = 1e-13          # the sweep tolerance of test_gpu_parity.py
RGAS = 8.314462618
BMAX = 600
BS = [1, 7, 130, 600]


def _states(n, B, seed=0):
    rng = np.random.default_rng(seed)
    U = 10.0 ** rng.uniform(-12, 0, (B, n))
    U[0] = 0.0; U[0, 0] = 1.0                                  # the solve's one-hot u0
    if B > 1:
        U[1, rng.random(n) < 0.3] = 0.0                        # exact zeros
    if B > 2:
        U[2, rng.choice(n, 5, replace=False)] = -1e-14          # what an implicit solve leaves behind
    return U


def _weights(B, seed=1):
    w = np.random.default_rng(seed).normal(size=B)
    w[::5] = 0.0
    w[1::7] = -np.abs(w[1::7])
    return w


class Case:
    """One network with its handle, oracle, BMAX states and the references of every rate-constant source (computed once)."""

    def __init__(self, net, Ea, A):
        self.net, self.Ea, self.A = net, Ea, A
        self.h = capi.HipNetwork.from_flat(net)
        self.on = orc.OracleNetwork.from_flat(net)
        self.U = _states(net.n_species, BMAX)
        self.w = _weights(BMAX)
        rng = np.random.default_rng(2)
        self.k0 = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
        self.K = self.k0[None, :] * rng.uniform(0.5, 2.0, (BMAX, 1)) * rng.uniform(0.9, 1.1, (BMAX, net.n_reactions))
        self.K3 = self.K[:3].copy()
        self.row3 = rng.integers(0, 3, BMAX).astype(np.int64)
        self.T = rng.uniform(600.0, 1200.0, BMAX)
        self._ref = {}

    def k_of(self, mode, b):
        if mode == "shared":
            return self.k0
        if mode == "per_state":
            return self.K[b]
        if mode == "k_row":
            return self.K3[self.row3[b]]
        return orc.arrhenius(self.Ea, self.A, self.T[b], k_max=1e12 if mode == "T_kmax" else None)

    def ref_rates(self, mode):
        if mode not in self._ref:
            self._ref[mode] = np.stack([self.on.rates(self.k_of(mode, b), self.U[b]) for b in range(BMAX)])
        return self._ref[mode]

    def call(self, mode, B, w=None, **kw):
        h, U = self.h, self.U[:B]
        if mode == "shared":
            h.set_rates(self.k0)
            return h.flux_batched(U, w=w, **kw)
        if mode == "per_state":
            return h.flux_batched(U, k=self.K[:B], w=w, **kw)
        if mode == "k_row":
            return h.flux_batched(U, k=self.K3, k_row=self.row3[:B], w=w, **kw)
        h.set_arrhenius(self.Ea, self.A, k_max=1e12 if mode == "T_kmax" else None)
        return h.flux_batched(U, T=self.T[:B], w=w, **kw)

    def extra(self, mode, B):
        """Per-term relative slack of the temperature form, [B][R] (0 with rate constants given)."""
        if not mode.startswith("T"):
            return np.zeros((B, self.net.n_reactions))
        return (2.0 * np.abs(self.Ea[None, :] / (RGAS * self.T[:B, None])) + 16.0) * EPS

    def check(self, mode, B, flux, rates, w):
        ref = self.ref_rates(mode)[:B]
        ex = self.extra(mode, B)
        if rates is not None:
            err = np.abs(rates - ref)
            bound = (4 * EPS + ex) * np.abs(ref) + 1e-300
            print(f"rates {mode} B={B}: max err/bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)
        if flux is not None:
            terms = w[:B, None] * ref
            fref = np.array([math.fsum(terms[:, r]) for r in range(ref.shape[1])])
            bound = (B + 8) * EPS * np.abs(terms).sum(axis=0) + (ex * np.abs(terms)).sum(axis=0) + 1e-300
            err = np.abs(flux - fref)
            print(f"flux {mode} B={B}: max err/bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)


_cases = {}


@pytest.fixture(scope="module", params=[(300, 1500), (1000, 5000)], ids=["300x1500", "1000x5000"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(*synthetic_crn(*request.param))
    return _cases[request.param]


@pytest.fixture(scope="module")
def small():
    if (300, 1500) not in _cases:
        _cases[(300, 1500)] = Case(*synthetic_crn(300, 1500))
    return _cases[(300, 1500)]


@pytest.fixture(scope="module")
def mid():
    if (1000, 5000) not in _cases:
        _cases[(1000, 5000)] = Case(*synthetic_crn(1000, 5000))
    return _cases[(1000, 5000)]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("mode", ["shared", "per_state", "k_row", "T", "T_kmax"])
def test_flux_and_rates_match_oracle(case, mode, B):
    flux, rates = case.call(mode, B, w=case.w[:B], want_rates=True)
    case.check(mode, B, flux, rates, case.w)


def test_null_weights_are_ones(small):
    flux = small.call("per_state", 130)
    small.check("per_state", 130, flux, None, np.ones(BMAX))


def test_three_parts_ragged_last(mid, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_ROWS", "1")      # 2 500 pairs over 1 024 threads: parts of 1 024, 1 024 and 452 pairs
    for mode in ("per_state", "T_kmax"):
        flux, rates = mid.call(mode, 130, w=mid.w[:130], want_rates=True)
        mid.check(mode, 130, flux, rates, mid.w)


def test_odd_reaction_count_half_filled_pair(small, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_ROWS", "2")
    R = small.net.n_reactions - 1
    net = small.net.subset(np.arange(R))
    h = capi.HipNetwork.from_flat(net)
    on = orc.OracleNetwork.from_flat(net)
    B = 7
    U, K, w = small.U[:B], small.K[:B, :R].copy(), small.w[:B]
    ref = np.stack([on.rates(K[b], U[b]) for b in range(B)])
    terms = w[:, None] * ref
    fref = np.array([math.fsum(terms[:, r]) for r in range(R)])
    fbound = (B + 8) * EPS * np.abs(terms).sum(axis=0) + 1e-300
    flux, rates = h.flux_batched(U, k=K, w=w, want_rates=True)
    assert np.all(np.abs(rates - ref) <= 4 * EPS * np.abs(ref) + 1e-300)
    assert np.all(np.abs(flux - fref) <= fbound)
    h.set_rates(K[0])                                          # ... and the shared row
    ref0 = np.stack([on.rates(K[0], U[b]) for b in range(B)])
    _, rates0 = h.flux_batched(U, w=w, want_rates=True)
    assert np.all(np.abs(rates0 - ref0) <= 4 * EPS * np.abs(ref0) + 1e-300)
    h.set_arrhenius(small.Ea[:R], small.A[:R], k_max=1e12)
    T = small.T[:B]
    refT = np.stack([on.rates(orc.arrhenius(small.Ea[:R], small.A[:R], T[b], k_max=1e12), U[b]) for b in range(B)])
    _, ratesT = h.flux_batched(U, T=T, want_rates=True)
    ex = (2.0 * np.abs(small.Ea[None, :R] / (RGAS * T[:, None])) + 16.0) * EPS
    assert np.all(np.abs(ratesT - refT) <= (4 * EPS + ex) * np.abs(refT) + 1e-300)
    h.close()


@pytest.mark.parametrize("mode", ["shared", "per_state", "k_row", "T_kmax"])
def test_gather_path_matches_oracle_and_lds_path(small, mode, monkeypatch):
    B = 130
    f_lds, r_lds = small.call(mode, B, w=small.w[:B], want_rates=True)
    monkeypatch.setenv("KIN_FLUX_LDS", "0")
    flux, rates = small.call(mode, B, w=small.w[:B], want_rates=True)
    small.check(mode, B, flux, rates, small.w)
    # both paths sit within the bound of the same reference: they agree within twice the bound
    ref = small.ref_rates(mode)[:B]
    assert np.all(np.abs(rates - r_lds) <= 2 * (4 * EPS + small.extra(mode, B)) * np.abs(ref) + 1e-300)


def test_species_ids_above_65535():
    N, R, B = 70000, 200, 2
    rng = np.random.default_rng(5)
    reacs, prods = [], []
    for r in range(R):
        a, b, c = (int(x) for x in rng.integers(65536, N, 3)) if r % 2 == 0 else (int(x) for x in rng.integers(0, N, 3))
        if r % 3 == 0:
            reacs.append([(a, 1)]); prods.append([(c, 1)])
        elif r % 3 == 1:
            reacs.append([(a, 2)]); prods.append([(c, 1)])
        else:
            reacs.append([(a, 1), (b, 1)] if a != b else [(a, 2)]); prods.append([(c, 1)])
    net = from_lists(N, reacs, prods)
    h = capi.HipNetwork.from_flat(net)
    on = orc.OracleNetwork.from_flat(net)
    U = 10.0 ** rng.uniform(-6, 0, (B, N))
    K = 10.0 ** rng.uniform(-3, 3, (B, R))
    w = np.array([0.25, -3.0])
    flux, rates = h.flux_batched(U, k=K, w=w, want_rates=True)
    ref = np.stack([on.rates(K[b], U[b]) for b in range(B)])
    assert np.all(ref != 0.0)
    assert np.all(np.abs(rates - ref) <= 4 * EPS * np.abs(ref) + 1e-300)
    terms = w[:, None] * ref
    fref = np.array([math.fsum(terms[:, r]) for r in range(R)])
    assert np.all(np.abs(flux - fref) <= (B + 8) * EPS * np.abs(terms).sum(axis=0) + 1e-300)
    h.close()


@pytest.mark.parametrize("lds", ["1", "0"])
def test_special_stoichiometries_hand_values(lds, monkeypatch):
    monkeypatch.setenv("KIN_FLUX_LDS", lds)
    # 2A -> B (no 1/2!), A -> 2B, inert collider A + M -> B + M, product = reactant species
    reacs = [[(0, 2)], [(0, 1)], [(0, 1), (2, 1)], [(1, 1)]]
    prods = [[(1, 1)], [(1, 2)], [(1, 1), (2, 1)], [(0, 1), (1, 1)]]
    h = capi.HipNetwork.from_flat(from_lists(3, reacs, prods))
    k = np.array([3.0, 0.5, 2.0, 0.25])
    U = np.array([[0.5, 0.25, 4.0], [2.0, 0.0, 1.0], [0.125, 8.0, 0.5]])
    w = np.array([1.0, 2.0, -4.0])
    # exact in binary: every factor is a small dyadic number
    hand = np.array([[3.0 * 0.25, 0.5 * 0.5, 2.0 * 0.5 * 4.0, 0.25 * 0.25],
                     [3.0 * 4.0, 0.5 * 2.0, 2.0 * 2.0 * 1.0, 0.0],
                     [3.0 * 0.015625, 0.5 * 0.125, 2.0 * 0.125 * 0.5, 0.25 * 8.0]])
    h.set_rates(k)
    flux, rates = h.flux_batched(U, w=w, want_rates=True)
    assert np.array_equal(rates, hand)
    assert np.array_equal(flux, (w[:, None] * hand).sum(axis=0))
    h.close()


def test_output_selection_gives_identical_bits(mid):
    B = 130
    both_f, both_r = mid.call("per_state", B, w=mid.w[:B], want_rates=True)
    only_f = mid.call("per_state", B, w=mid.w[:B])
    none_f, only_r = mid.call("per_state", B, w=mid.w[:B], want_rates=True, want_flux=False)
    assert none_f is None
    assert np.array_equal(both_f, only_f) and np.array_equal(both_r, only_r)


def test_deterministic_and_host_equals_device(mid):
    import torch
    B = 600
    h, U, K, w = mid.h, mid.U[:B], mid.K[:B], mid.w[:B]
    f1 = h.flux_batched(U, k=K, w=w)
    f2 = h.flux_batched(U, k=K, w=w)
    assert np.array_equal(f1, f2)
    dev = "cuda:0"
    d_u, d_k, d_w = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (U, K, w))
    d_f = torch.full((mid.net.n_reactions,), float("nan"), dtype=torch.float64, device=dev)
    d_r = torch.full((B, mid.net.n_reactions), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    h.flux_batched_dev(B, d_u.data_ptr(), d_k=d_k.data_ptr(), d_w=d_w.data_ptr(), d_flux=d_f.data_ptr(), d_rates=d_r.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_f.cpu().numpy(), f1)
    _, r1 = h.flux_batched(U, k=K, w=w, want_rates=True)
    assert np.array_equal(d_r.cpu().numpy(), r1)
    # k_row on the device: int64 indices into a 3-row array
    d_k3 = torch.tensor(mid.K3, dtype=torch.float64, device=dev)
    d_row = torch.tensor(mid.row3[:B], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    h.flux_batched_dev(B, d_u.data_ptr(), d_k=d_k3.data_ptr(), d_k_row=d_row.data_ptr(), d_w=d_w.data_ptr(), d_flux=d_f.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_f.cpu().numpy(), h.flux_batched(U, k=mid.K3, k_row=mid.row3[:B], w=w))


def test_stoichiometric_matrix_times_rates_is_the_sweep(case):
    net, B = case.net, 7
    rr = np.repeat(np.arange(net.n_reactions), np.diff(net.reac_ptr))
    pr = np.repeat(np.arange(net.n_reactions), np.diff(net.prod_ptr))
    shape = (net.n_species, net.n_reactions)
    S = sp.csr_matrix((net.prod_sto.astype(float), (net.prod_idx, pr)), shape=shape) - \
        sp.csr_matrix((net.reac_sto.astype(float), (net.reac_idx, rr)), shape=shape)
    U, K = case.U[:B], case.K[:B]
    _, rates = case.h.flux_batched(U, k=K, want_rates=True)
    DU = case.h.rhs_batched(U, K)
    for b in range(B):
        assert np.all(np.abs(S @ rates[b] - DU[b]) <= TOL * case.on.abs_rhs(K[b], U[b]) + 1e-300)


def test_zero_states_write_zeros(small):
    small.h.set_rates(small.k0)
    flux = small.h.flux_batched(np.empty((0, small.net.n_species)))
    assert flux.shape == (small.net.n_reactions,) and np.all(flux == 0.0)


def test_error_statuses():
    net, Ea, A = synthetic_crn(50, 200, seed=3)
    h = capi.HipNetwork.from_flat(net)
    L = capi.lib()
    U = np.ones((4, 50)); K = np.ones((4, 200)); T = np.full(4, 800.0)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    INV, STATE = capi.KIN_ERR_INVALID_ARG, capi.KIN_ERR_STATE
    assert code(lambda: h.flux_batched(U)) == STATE                                        # no rates at all
    assert code(lambda: h.flux_batched(U, T=T)) == STATE                                   # T without Arrhenius parameters
    assert code(lambda: h.solution_flux(k=K[:1], k_row=np.zeros(0, np.int64))) == STATE    # no stored solution
    h.set_arrhenius(Ea, A)
    assert code(lambda: h.flux_batched(U, k=K, T=T)) == INV                                # both k and T
    assert code(lambda: h.flux_batched(U, k_row=np.zeros(4, np.int64))) == INV             # k_row without a k source
    assert code(lambda: h.flux_batched(U, k=K, k_row=np.array([0, 1, 4, 2]))) == INV       # row index out of range
    assert code(lambda: h.flux_batched(U, k=K, k_row=np.array([0, -1, 1, 2]))) == INV
    assert code(lambda: h.flux_batched(U, k=K[:3])) == INV                                 # k_row == NULL needs n_k_rows == B
    assert code(lambda: h.flux_batched(U, k=K, want_flux=False)) == INV                    # neither output
    PD = capi._pd
    out = np.empty(200)
    assert L.kin_flux_batched(h.handle, -1, PD(U), PD(K), 4, None, None, None, PD(out), None) == INV          # B < 0
    assert L.kin_flux_batched_dev(h.handle, -1, None, None, None, None, None, None, None, None) == INV
    assert L.kin_flux_batched_dev(h.handle, 4, None, None, None, None, None, None, None, None) == INV          # neither output
    # table rows asked for with no resident table: needs a stored solution first
    h.set_rates(np.ones(200))
    pars = capi.KinParams(tspan0=0.0, tspan1=2e-3, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1,
                          ban_negatives=0, solve_chunkstep=1e-3, maxiters=100000, save_interval=-1.0)
    u0 = np.zeros(50); u0[0] = 1.0
    t, us, rc, st, status = h.solve(pars, u0)
    assert rc == 0 and len(t) >= 2
    assert code(lambda: h.solution_flux(k_row=np.zeros(len(t), np.int64))) == STATE
    assert code(lambda: h.solution_flux(k=K[:2], k_row=np.full(len(t), 2, np.int64))) == INV
    assert code(lambda: h.solution_flux(want_flux=False)) == INV
    h.close()
