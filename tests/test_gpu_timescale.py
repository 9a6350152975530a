"""GPU tests of the timescale analysis (kin_jac_batched, kin_timescale_batched and the solution / ensemble forms) against the
extended-precision reference and the derived bounds of tests/timescale_cases.py (its docstring has the derivations): exact
inputs bit for bit, random states inside the bounds and intervals entry by entry."""
import numpy as np
import pytest

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from oracle import oracle as orc
from tests import jac_cases as jc
from tests import timescale_cases as tc
from tests.linalg_cases import hub_net

pytestmark = pytest.mark.gpu

LD = jc.LD
# One length past a single pass of a workgroup: a long contribution list and a long row are both taken TS_WG * TS_LONG_NX =
# 1024 entries per pass (timescale.hpp), so 1025 needs a second pass with one live entry in it.
PAST_ONE_PASS = capi.TIMESCALE_LONG_PASS + 1
assert PAST_ONE_PASS == 1025
OUTPUTS = ("diag", "err", "norm", "summary")


def all_outputs(h, U, **src):
    out = h.timescale_batched(U, want_diag=True, want_err=True, **src)
    out["vals"] = h.jac_batched(U, **{q: v for q, v in src.items() if q != "summary"})
    return out


def assert_exact(net, ref, seed, B=3):
    """every output of the exact inputs equals the reference bit for bit (by value: -0.0 equals 0.0)"""
    Us, K = tc.exact_states(ref, B, seed)
    want = tc.exact_expectation(ref, K, Us)
    h = capi.HipNetwork.from_flat(net)
    try:
        rowptr, col = h.jac_pattern()
        assert np.array_equal(rowptr, ref.rowptr) and np.array_equal(col, ref.cols)
        got = all_outputs(h, Us, k=K)
    finally:
        h.close()
    for q in ("vals",) + OUTPUTS:
        assert got[q].shape == want[q].shape and np.array_equal(got[q], want[q]), (q, got[q], want[q])
    return got, want


# ------------------------------------------------------------------------------------- 1. values and derived quantities, exact
CASE_NAMES = [f"{plan}_rows_{t}_{tag}" for plan in ("jac", "rhs") for t in jc.ROW_COUNTS for tag in ("short", "long")] + \
             ["empty_rows", "triple_product"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_exact_inputs_bit_for_bit_on_the_case_list(name):
    net, ref = jc.case(name)
    got, want = assert_exact(net, ref, seed=len(name))
    if name == "empty_rows":
        assert got["diag"][:, 2:].tolist() == [[0.0] * 3] * 3
        assert got["err"][:, 2:4].tolist() == [[0.0] * 2] * 3 and np.all(got["err"][:, 4] == np.inf)


@pytest.mark.parametrize("L", [1, 8, 9, 64, 65, 256, 257, PAST_ONE_PASS])
def test_exact_inputs_bit_for_bit_on_hub_lengths(L):
    """hub_net(L): the entries J[hub, hub] and J[sink, hub] gather L contributions each"""
    net = hub_net(L)
    ref = jc.Reference(net)
    assert int(ref.L_jac.max()) == L
    assert_exact(net, ref, seed=L)


# ----------------------------------------------------------------------------------------------------- 2. row-pass classes
@pytest.mark.parametrize("entries", [1, 8, 9, 64, 65, 256, 257, PAST_ONE_PASS])
def test_row_pass_classes_on_fan_in_rows(entries):
    """row H of X_j -> H stores L + 1 entries; H is produced only: d = 0 and e = +Inf there"""
    L = entries - 1
    net = tc.fan_in_net(L)                                # (L = 0: H alone, no reaction)
    ref = jc.Reference(net)
    info = capi.timescale_plan_host(net)
    cls = "rows_short" if entries <= 8 else "rows_medium" if entries <= 256 else "rows_long"
    assert int(np.diff(ref.rowptr)[0]) == entries and info[cls] == (L + 1 if cls == "rows_short" else 1)
    got, want = assert_exact(net, ref, seed=entries)
    e_H = np.inf if L else 0.0                            # f_H = sum k_j X_j > 0 over a diagonal of 0; without a reaction 0 / 0
    assert np.all(got["diag"][:, 0] == 0.0) and np.all(got["err"][:, 0] == e_H)
    assert got["summary"][:, 0].tolist() == [0.0, 0.0, e_H]


# ----------------------------------------------------------------------------------- 3. random states inside the derived bounds
MODES = ("shared", "per_state", "k_row", "T", "T_kmax")
BMAX = 64
RGAS = 8.314462618


class Synth:
    """a synthetic network with BMAX random states - positive over 12 decades, a few exact zeros, a few entries at -1e-12 - and
    every rate-constant source of tests/test_gpu_flux.py; the per-state references are built once per source"""

    def __init__(self, n, r):
        self.net, self.Ea, self.A = synthetic_crn(n, r)
        self.ref = jc.Reference(self.net)
        rng = np.random.default_rng(n + r)
        self.U = 10.0 ** rng.uniform(-12, 0, (BMAX, n))
        self.U[rng.random((BMAX, n)) < 0.01] = 0.0
        self.U[rng.random((BMAX, n)) < 0.01] = -1e-12
        self.k0 = orc.arrhenius(self.Ea, self.A, 1000.0, k_max=1e12)
        self.K = self.k0[None, :] * rng.uniform(0.5, 2.0, (BMAX, 1)) * rng.uniform(0.9, 1.1, (BMAX, r))
        self.K3 = self.K[:3].copy()
        self.row3 = rng.integers(0, 3, BMAX).astype(np.int64)
        self.T = rng.uniform(600.0, 1200.0, BMAX)
        self.h = capi.HipNetwork.from_flat(self.net)
        self._states = {}

    def k_of(self, mode, b):
        if mode == "shared":
            return self.k0
        if mode == "per_state":
            return self.K[b]
        if mode == "k_row":
            return self.K3[self.row3[b]]
        return orc.arrhenius(self.Ea, self.A, self.T[b], k_max=1e12 if mode == "T_kmax" else None)

    def source(self, mode, lo, hi):
        """keywords of the first states lo .. hi - 1, the handle prepared for them"""
        if mode == "shared":
            self.h.set_rates(self.k0)
        elif mode.startswith("T"):
            self.h.set_arrhenius(self.Ea, self.A, k_max=1e12 if mode == "T_kmax" else None)
        if mode == "per_state":
            return dict(k=self.K[lo:hi])
        if mode == "k_row":
            return dict(k=self.K3, k_row=self.row3[lo:hi])
        if mode.startswith("T"):
            return dict(T=self.T[lo:hi])
        return {}

    def states(self, mode, B):
        have = self._states.setdefault(mode, [])
        for b in range(len(have), B):
            ex = (2.0 * np.abs(self.Ea / (RGAS * self.T[b])) + 16.0) * 2.0 ** -53 if mode.startswith("T") else None
            have.append(tc.StateRef(self.ref, self.k_of(mode, b), self.U[b], ex))
        return have[:B]


_synth = {}


def synth(n, r):
    if (n, r) not in _synth:
        _synth[(n, r)] = Synth(n, r)
    return _synth[(n, r)]


def check_bounds(what, got, sts):
    """every entry of every output inside its bound or interval; prints the largest error / bound"""
    B = len(sts)
    nd, bd = np.stack([-s.d for s in sts]), np.stack([s.bd for s in sts])
    e_lo, e_hi = np.stack([s.e_lo for s in sts]), np.stack([s.e_hi for s in sts])
    J, bJ = np.stack([s.J for s in sts]), np.stack([s.bJ for s in sts])
    norm, bnorm = np.array([s.norm for s in sts]), np.array([s.bnorm for s in sts])
    lo = np.stack([(nd - bd).max(0), (nd - bd).min(0), e_lo.max(0)])
    hi = np.stack([(nd + bd).max(0), (nd + bd).min(0), e_hi.max(0)])
    e_ref = np.stack([s.e for s in sts])
    fin = np.isfinite(e_hi)
    half = (np.where(fin, e_hi, 0) - np.where(fin, e_lo, 0)) / 2
    print(f"{what} B={B}: max err/bound vals {tc.ratio(got['vals'], J, bJ):.3f}, diag {tc.ratio(got['diag'], -nd, bd):.3f}, "
          f"norm {tc.ratio(got['norm'], norm, bnorm):.3f}, err (of the half width) "
          f"{tc.ratio(np.where(fin, got['err'], 0.0), np.where(fin, e_ref, 0), half):.3f}, {100 * np.mean(~fin):.2f} % of the err intervals open")
    assert np.all(np.abs(got["vals"].astype(LD) - J) <= bJ), (what, "vals")
    assert np.all(np.abs(got["diag"].astype(LD) + nd) <= bd), (what, "diag")
    assert np.all(np.abs(got["norm"].astype(LD) - norm) <= bnorm), (what, "norm")
    assert tc.inside(got["err"], e_lo, e_hi)[0], (what, "err", tc.inside(got["err"], e_lo, e_hi))
    assert tc.inside(got["summary"], lo, hi)[0], (what, "summary", tc.inside(got["summary"], lo, hi))
    assert not np.any(np.isnan(got["err"])) and not np.any(np.isnan(got["summary"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,r,B", [(300, 1500, 1), (300, 1500, 5), (300, 1500, 64), (1000, 5000, 8)])
def test_random_states_inside_the_bounds(n, r, B, mode):
    c = synth(n, r)
    got = all_outputs(c.h, c.U[:B], **c.source(mode, 0, B))
    check_bounds(f"{n}x{r} {mode}", got, c.states(mode, B))
    if mode == "shared":       # the batched values next to kin_jac_values, both inside the entrywise bound
        for b in range(min(B, 5)):
            ra = jc.assert_jac_entrywise(c.net, c.k0, c.U[b], got["vals"][b], what=("jac_batched", b))
            rb = jc.assert_jac_entrywise(c.net, c.k0, c.U[b], c.h.jac_values(c.U[b]), what=("jac_values", b))
            print(f"state {b}: jac_batched err/bound {ra:.3f}, jac_values {rb:.3f}")


# ------------------------------------------------------------------------------------------------------------ 4. blocking
@pytest.mark.parametrize("mode", ["per_state", "k_row", "T"])
def test_blocks_of_three_states_change_nothing(mode, monkeypatch):
    c, B = synth(300, 1500), 8
    whole = all_outputs(c.h, c.U[:B], **c.source(mode, 0, B))
    again = all_outputs(c.h, c.U[:B], **c.source(mode, 0, B))
    monkeypatch.setenv("KIN_TS_BLOCK_STATES", "3")
    blocks = all_outputs(c.h, c.U[:B], **c.source(mode, 0, B))
    for q in ("vals",) + OUTPUTS:
        assert np.array_equal(again[q], whole[q]), q
        assert np.array_equal(blocks[q], whole[q]), q
    check_bounds(f"blocks {mode}", blocks, c.states(mode, B))


# ---------------------------------------------------------------------------------------------------------- 5. accumulate
def test_accumulate_folds_two_halves_bit_for_bit():
    c, B = synth(300, 1500), 64
    whole = c.h.timescale_batched(c.U[:B], **c.source("per_state", 0, B))
    first = c.h.timescale_batched(c.U[:30], **c.source("per_state", 0, 30))
    both = c.h.timescale_batched(c.U[30:B], summary=first["summary"], **c.source("per_state", 30, B))
    assert np.array_equal(both["summary"], whole["summary"])
    assert np.array_equal(np.concatenate([first["norm"], both["norm"]]), whole["norm"])
    assert not np.array_equal(first["summary"], whole["summary"])
    # no states: the identities, or summary left alone when accumulating
    n, r = c.net.n_species, c.net.n_reactions
    none = c.h.timescale_batched(np.empty((0, n)), k=np.empty((0, r)))
    assert np.array_equal(none["summary"], tc.identity(n)) and none["norm"].shape == (0,)
    kept = c.h.timescale_batched(np.empty((0, n)), k=np.empty((0, r)), summary=whole["summary"])
    assert np.array_equal(kept["summary"], whole["summary"])
    # folding the identities into a call changes nothing
    ident = c.h.timescale_batched(c.U[:B], summary=tc.identity(n), **c.source("per_state", 0, B))
    assert np.array_equal(ident["summary"], whole["summary"])


# ------------------------------------------------------------------------------------------------------ 6. device pointers
def test_device_pointers_equal_host_arrays_on_another_stream():
    import torch
    c, B = synth(1000, 5000), 8
    want = all_outputs(c.h, c.U[:B], **c.source("per_state", 0, B))
    n, nnz = c.net.n_species, want["vals"].shape[1]
    dev = "cuda:0"
    d_u, d_k = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (c.U[:B], c.K[:B]))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    d_s, d_d, d_e, d_n, d_v = nan(3, n), nan(B, n), nan(B, n), nan(B), nan(B, nnz)
    torch.cuda.synchronize()      # torch's fills run on torch's stream
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    c.h.timescale_batched_dev(B, d_u.data_ptr(), d_summary=d_s.data_ptr(), d_diag=d_d.data_ptr(), d_err=d_e.data_ptr(), d_norm=d_n.data_ptr(),
                              d_k=d_k.data_ptr(), stream=stream.cuda_stream)
    c.h.jac_batched_dev(B, d_u.data_ptr(), d_v.data_ptr(), d_k=d_k.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    for q, t in (("summary", d_s), ("diag", d_d), ("err", d_e), ("norm", d_n), ("vals", d_v)):
        assert np.array_equal(t.cpu().numpy(), want[q]), q
    c.h.timescale_batched_dev(3, d_u.data_ptr(), d_summary=d_s.data_ptr(), d_k=d_k.data_ptr(), accumulate=True, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_s.cpu().numpy(), want["summary"])


# ------------------------------------------------------------------------------------------ 7. solution and ensemble forms
def _pars(t1, chunks, save=-1.0, maxiters=100000):
    return capi.KinParams(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
                          ban_negatives=0, solve_chunkstep=t1 / max(chunks, 1), maxiters=maxiters, save_interval=save, dtmin=0.0)


def test_solution_and_ensemble_forms_equal_the_batched_call():
    solution_and_ensemble_forms()


def test_solution_and_ensemble_forms_equal_the_batched_call_in_two_slices(monkeypatch):
    """KIN_SLICES_MAX = 2: a task walks every other row of the record and skips, inside its walk, the rows below row_begin and
    those a short member has not saved"""
    monkeypatch.setenv("KIN_SLICES_MAX", "2")
    solution_and_ensemble_forms()


def solution_and_ensemble_forms():
    c = synth(300, 1500)
    h = capi.HipNetwork.from_flat(c.net)
    u0 = np.zeros(300); u0[0] = 1.0
    h.set_rates(c.k0)
    t, us, rc, st, status = h.solve(_pars(2e-3, 2), u0)
    n_saved = len(t)
    assert rc == 0 and n_saved >= 3
    for rb in (0, 1, n_saved):
        want = h.timescale_batched(us[rb:])
        summary, norm = h.solution_timescale(row_begin=rb)
        assert np.array_equal(summary, want["summary"]), rb
        assert np.all(norm[:rb] == 0.0) and np.array_equal(norm[rb:], want["norm"]), rb
    assert np.array_equal(h.solution_timescale(row_begin=n_saved)[0], tc.identity(300))
    whole = h.timescale_batched(us)["summary"]
    krow = np.zeros(n_saved, np.int64)
    assert np.array_equal(h.solution_timescale(k=c.k0[None, :], k_row=krow)[0], whole)
    tail = h.solution_timescale(row_begin=1)[0]
    assert np.array_equal(h.solution_timescale(row_begin=n_saved, summary=tail)[0], tail)      # nothing counts: left alone
    head = h.timescale_batched(us[:1])["summary"]
    assert np.array_equal(h.solution_timescale(row_begin=1, summary=head)[0], whole)           # the two parts fold to the whole
    # an ensemble of three members with their own rate constants; member 1 fails early (rate constants beyond any step size) and
    # has fewer saved rows: the rows past n_saved take no part and their norm is 0.0
    K = 3
    k = c.K[:K].copy()
    k[1] *= 1e40
    u0s = np.repeat(u0[None, :], K, axis=0)
    res = h.solve_ensemble(_pars(2e-3, 2, save=2.5e-4, maxiters=3000), u0s, k=k)
    Ke, rows, n, ns = h.ensemble_size()
    assert Ke == K and rows == 9 and ns[0] == 9 and ns[2] == 9 and ns[1] < 9
    us_e = np.asarray(res[1]).reshape(K, -1, n)
    k_row = np.repeat(np.arange(K, dtype=np.int64)[:, None], rows, axis=1)
    for m in range(K):
        k_row[m, ns[m]:] = 10 ** 9            # keys of rows that do not exist are ignored
    for rb in (0, 1, int(ns[1]), rows):
        cnt = [max(int(ns[m]) - rb, 0) for m in range(K)]
        flat = np.concatenate([us_e[m, rb:ns[m]] for m in range(K)])
        flat_row = np.concatenate([np.full(cnt[m], m, np.int64) for m in range(K)])
        want = h.timescale_batched(flat, k=k, k_row=flat_row)
        summary, norm = h.ensemble_timescale(k=k, k_row=k_row, row_begin=rb)
        assert np.array_equal(summary, want["summary"]), rb
        assert norm.shape == (K, rows)
        for m in range(K):
            assert np.all(norm[m, :rb] == 0.0) and np.all(norm[m, ns[m]:] == 0.0), (rb, m)
        assert np.array_equal(np.concatenate([norm[m, rb:ns[m]] for m in range(K)]), want["norm"]), rb
    assert np.array_equal(h.ensemble_timescale(k=k, k_row=k_row, row_begin=rows)[0], tc.identity(300))
    h.close()


# ------------------------------------------------------------------------------------------------------ 8. Python end to end
def test_python_end_to_end_finds_the_quasi_steady_intermediate():
    from kinetica_jl_amd import conditions as C
    from kinetica_jl_amd import solving as S
    k1, k2 = 1.0, 1e4
    sd = S.SpeciesData.from_names(["A", "X", "B"])
    rd = S.RxData.from_flat(tc.chain_net())
    calc = S.DummyKineticCalculator([k1, k2])
    pars = S.ODESimulationParams(tspan=(0.0, 1.0), u0={"A": 1.0}, solve_chunkstep=0.1, abstol=1e-12, reltol=1e-8, low_k_cutoff="none")
    out = S.solve_network(S.StaticODESolve(pars, C.ConditionSet({"T": 300.0}), calc), sd, rd)
    assert out.sol.retcode == "Success"
    t = np.asarray(out.sol.t)
    scale = np.asarray(out.sol.u).reshape(len(t), 3).max(axis=0)
    # the initial layer of X lasts a few 1 / k2 = 1e-4: t_min = 0.05 is 500 of them, and leaves out t = 0 only
    ts = S.species_timescales(out, calc, t_min=0.05)
    assert np.array_equal(ts.t, t[t >= 0.05]) and len(ts.t) == len(t) - 1 and len(ts.norm) == len(ts.t)
    print("qss_err / scale", ts.qss_err / scale, "decay", ts.decay_min, ts.decay_max, "stiffness", ts.stiffness())
    assert S.qss_candidates(ts, tol=1e-2, scale=scale).tolist() == [1]
    assert ts.decay_max.tolist() == [k1, k2, 0.0] and ts.decay_min.tolist() == [k1, k2, 0.0]
    assert ts.lifetime_min().tolist() == [1.0 / k1, 1.0 / k2, np.inf]
    # with t = 0 in, e_X = k1 A0 / k2 there is the whole of X's scale
    full = S.species_timescales(out, calc)
    assert len(full.t) == len(t) and 1 not in S.qss_candidates(full, tol=1e-2, scale=scale).tolist()
    assert full.qss_err[1] == k1 * 1.0 / k2
    assert k2 <= ts.stiffness() <= 2 * k2                       # row X holds k1 + k2, row B holds k2
    # an earlier result folds in
    folded = S.species_timescales(out, calc, t_min=0.05, summary=full)
    assert np.array_equal(folded.qss_err, full.qss_err)


# ----------------------------------------------------------------------------------------------------------- 9. statuses
def test_error_statuses():
    net, Ea, A = synthetic_crn(50, 200, seed=3)
    h = capi.HipNetwork.from_flat(net)
    U = np.ones((4, 50)); K = np.ones((4, 200)); T = np.full(4, 800.0)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    INV, STATE = capi.KIN_ERR_INVALID_ARG, capi.KIN_ERR_STATE
    for fn in (h.timescale_batched, h.jac_batched):
        assert code(lambda: fn(U)) == STATE                                               # no rates at all
        assert code(lambda: fn(U, T=T)) == STATE                                          # T without Arrhenius parameters
    assert code(lambda: h.solution_timescale(k=K[:1], k_row=np.zeros(0, np.int64))) == STATE   # no stored solution
    assert code(lambda: h.ensemble_timescale()) == STATE                                  # no stored ensemble
    h.set_arrhenius(Ea, A)
    for fn in (h.timescale_batched, h.jac_batched):
        assert code(lambda: fn(U, k=K, T=T)) == INV                                       # both k and T
        assert code(lambda: fn(U, k_row=np.zeros(4, np.int64))) == INV                    # k_row without a k source
        assert code(lambda: fn(U, k=K, k_row=np.array([0, 1, 4, 2]))) == INV              # row index out of range
        assert code(lambda: fn(U, k=K[:3])) == INV                                        # k_row == NULL needs n_k_rows == B
    assert code(lambda: h.timescale_batched(U, k=K, want_summary=False, want_norm=False)) == INV   # no output
    L = capi.lib()
    assert L.kin_jac_batched(h.handle, 4, capi._pd(U), capi._pd(K), 4, None, None, None) == INV               # null output
    assert L.kin_timescale_batched_dev(h.handle, -1, None, None, None, None, 0, None, None, None, None, None) == INV   # B < 0
    assert L.kin_jac_batched_dev(h.handle, -1, None, None, None, None, None, None) == INV
    assert L.kin_solution_timescale(h.handle, None, 0, None, None, -1, 0, capi._pd(np.empty((3, 50))), None) == INV    # row_begin < 0
    assert L.kin_ensemble_timescale(h.handle, None, 0, None, None, -1, 0, capi._pd(np.empty((3, 50))), None) == INV
    h.set_rates(np.ones(200))
    assert h.timescale_batched(U)["norm"].shape == (4,)
    h.close()
