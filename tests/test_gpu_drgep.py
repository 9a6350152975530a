"""GPU tests of DRG with error propagation (kin_drgep_batched, kin_drgep_paths and the solution / ensemble forms) against the
NumPy reference of drgep_cases.py.

Stage 2 (r) is compared within the bound derived in drgep_cases.py, per (edge, state); test_drgep_host.py checks on the CPU
that at most 1 % of those bounds are above 1e-9, and the tests here repeat that on what they compare. The path stage is
compared BIT FOR BIT: multiplication by a number in [0, 1] is monotone in floating point, so the fixed point is the maximum
over the paths of the left-to-right product whatever the order of relaxation, and the NumPy search on the device's own r
does the same multiplications."""
import numpy as np
import pytest

import drg_cases as dc
import drgep_cases as ec
from kinetica_jl_amd import capi

pytestmark = pytest.mark.gpu

TG = ec.TARGETS
B = ec.B_GPU
_handles, _stages = {}, {}


def handle(name):
    if name not in _handles:
        _handles[name] = capi.HipNetwork.from_flat(dc.synth_case(name).net)
    return _handles[name]


def device(name, mode, pairing, hi=B, lo=0, importance=None, stages=False):
    """drgep_batched of states lo .. hi - 1 of a synthetic case, targets 0, 1, 2."""
    case, h = dc.synth_case(name), handle(name)
    if mode == "shared":
        h.set_rates(case.k0)
    elif mode.startswith("T"):
        h.set_arrhenius(case.Ea, case.A, k_max=1e12 if mode == "T_kmax" else None)
    src = {k: (v[lo:] if k != "k" or mode == "per_state" else v) for k, v in case.source(mode, hi).items()}
    return h.drgep_batched(case.U[lo:hi], TG, pairing=pairing, importance=importance, stages=stages, **src)


def staged(name, mode, pairing):
    """(importance, r, R, rounds) of the first B states, computed once and left unchanged."""
    key = (name, mode, pairing)
    if key not in _stages:
        _stages[key] = device(name, mode, pairing, stages=True)
    return _stages[key]


def check_paths(g, r, targets, imp, R, rounds):
    """The device's search against NumPy's on the same r: bit for bit, the rounds too (Jacobi on both sides)."""
    imp_ref, R_ref, rounds_ref = g.importance(r, targets)
    assert np.array_equal(R, R_ref) and np.array_equal(imp, imp_ref)
    assert np.all(rounds <= g.n) and np.array_equal(rounds, np.minimum(rounds_ref, g.n))
    assert np.all(imp[np.asarray(targets)] == 1.0) and np.all((R >= 0.0) & (R <= 1.0))


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(ec.hand_networks()))
def test_hand_networks(name, pairing):
    net, k, U, targets, want = ec.hand_networks()[name]
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    imp, r, R, rounds = h.drgep_batched(U, targets, pairing=pairing, stages=True)
    assert imp.tolist() == want[pairing] and R[0].tolist() == want[pairing]          # dyadic inputs: exact
    zero = [1.0 if i in targets else 0.0 for i in range(net.n_species)]
    assert R[-1].tolist() == zero and np.all(r[-1] == 0.0)                          # den = 0 everywhere: exactly 0.0, never NaN
    assert h.drgep_batched(np.zeros((1, net.n_species)), targets, pairing=pairing).tolist() == zero
    assert np.all(rounds >= 1) and np.all(rounds <= net.n_species)
    h.close()


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name,mode", ec.GPU_CASES)
def test_stage_two_within_the_derived_bound(name, mode, pairing):
    _, r, _, _ = staged(name, mode, pairing)
    ref, bounds = ec.ref(name, mode, pairing)
    frac = float(np.mean(bounds > 1e-9))
    err = np.abs(r - ref)
    print(f"{name} {mode} pairing={pairing}: edges {ref.shape[1]}, max err {err.max():.3e}, max err/bound "
          f"{np.max(err / np.maximum(bounds, 1e-300)):.3f}, {100 * frac:.3f} % of the bounds above 1e-9")
    assert frac <= 0.01
    assert np.all(np.isfinite(r)) and np.all((r >= 0.0) & (r <= 1.0))
    assert np.all(err <= bounds)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name,mode", [("300x1500", "per_state"), ("300x1500", "T"), ("300x1500_cut", "per_state"), ("1000x5000", "per_state")])
def test_path_stage_bit_exact_on_the_device_coefficients(name, mode, pairing):
    imp, r, R, rounds = staged(name, mode, pairing)
    check_paths(ec.graph(name, pairing), r, TG, imp, R, rounds)
    print(f"{name} {mode} pairing={pairing}: rounds {rounds.min()}..{rounds.max()}, median importance {np.median(imp):.2e}")


@pytest.mark.parametrize("name", ["300x1500", "1000x5000"])
def test_paths_entry_on_random_coefficients(name):
    g, h = ec.graph(name, 1), handle(name)
    rng = np.random.default_rng(7)
    r = rng.random((5, g.E)) ** 3
    r[rng.random(r.shape) < 0.3] = 0.0
    r[rng.random(r.shape) < 0.05] = 1.0
    r[4] = 1.0                                   # every edge at 1: whatever can be reached is exactly 1
    targets = [g.n - 1, 3, 3]                    # (a target named twice)
    imp, R, rounds = h.drgep_paths(r, targets, pairing=1, stages=True)
    check_paths(g, r, targets, imp, R, rounds)
    assert set(np.unique(R[4])) <= {0.0, 1.0}
    # accumulation: the given importance takes part, values above every R survive
    assert np.array_equal(h.drgep_paths(r[:2], targets, importance=h.drgep_paths(r[2:], targets)), imp)
    assert np.array_equal(h.drgep_paths(r, targets, importance=np.full(g.n, 2.0)), np.full(g.n, 2.0))


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("n", [300, 20])
def test_collider_in_degree_of_a_workgroup_and_of_a_wavefront(n, pairing):
    from oracle import oracle as orc
    net = ec.collider_network(n)
    g = ec.DrgepRef(net, pairing)
    deg = np.bincount(g.cols, minlength=g.n)
    assert deg[0] == 2 * n + 1                    # every X_i and Y_i, and Z
    assert deg[0] > capi.DRGEP_IN_WAVE_MAX if n == 300 else capi.DRGEP_IN_SHORT_MAX < deg[0] <= capi.DRGEP_IN_WAVE_MAX
    rng = np.random.default_rng(5)
    nB = 6
    U = dc.states(net.n_species, nB, seed=3)
    K = 10.0 ** rng.uniform(-2, 2, (nB, net.n_reactions))
    on = orc.OracleNetwork.from_flat(net)
    ref, bounds = g.coefficients(np.stack([on.rates(K[b], U[b]) for b in range(nB)]))
    targets = [2, 2 + n + 1]                      # X_0 and Y_1: Z is reached over M alone
    h = capi.HipNetwork.from_flat(net)
    imp, r, R, rounds = h.drgep_batched(U, targets, k=K, pairing=pairing, stages=True)
    assert np.all(np.abs(r - ref) <= bounds)
    check_paths(g, r, targets, imp, R, rounds)
    assert imp[0] > 0.0 and imp[1] > 0.0          # M and, through it, Z
    # the search alone: M takes the maximum over all of its 2 n + 1 incoming edges - plant the winner on the last of them
    rr = np.zeros((1, g.E))
    e_in = np.flatnonzero(g.cols == 0)
    rr[0, e_in] = 0.25
    rr[0, e_in[-1]] = 0.5
    rr[0, np.flatnonzero((g.rows == 0) & (g.cols == 1))] = 0.5
    all_xy = list(range(2, g.n))
    imp2, R2, rounds2 = h.drgep_paths(rr, all_xy, pairing=pairing, stages=True)
    assert imp2[0] == 0.5 and imp2[1] == 0.25
    check_paths(g, rr, all_xy, imp2, R2, rounds2)
    h.close()


def test_global_memory_form_equals_the_lds_form(monkeypatch):
    want = staged("300x1500", "per_state", 1)
    monkeypatch.setenv("KIN_DRGEP_LDS_SPECIES", "100")
    got = device("300x1500", "per_state", 1, stages=True)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # ... with the long and the medium class as well
    for n in (300, 20):
        net = ec.collider_network(n)
        g = ec.DrgepRef(net, 1)
        r = np.random.default_rng(n).random((3, g.E))
        h = capi.HipNetwork.from_flat(net)
        glob = h.drgep_paths(r, [2, 5], stages=True)
        monkeypatch.delenv("KIN_DRGEP_LDS_SPECIES")
        lds = h.drgep_paths(r, [2, 5], stages=True)
        monkeypatch.setenv("KIN_DRGEP_LDS_SPECIES", "100")
        for a, b in zip(glob, lds):
            assert np.array_equal(a, b)
        check_paths(g, r, [2, 5], *glob)
        h.close()


@pytest.mark.parametrize("mode", ["per_state", "k_row", "T"])
def test_result_does_not_depend_on_the_blocks(mode, monkeypatch):
    whole = staged("300x1500", mode, 1)
    monkeypatch.setenv("KIN_DRG_BLOCK_STATES", "5")
    blocks = device("300x1500", mode, 1, stages=True)
    for a, b in zip(blocks, whole):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("pairing", [1, 0])
def test_repeat_and_accumulate_bit_for_bit(pairing):
    whole = staged("300x1500", "per_state", pairing)[0]
    assert np.array_equal(device("300x1500", "per_state", pairing), whole)            # two identical calls
    first = device("300x1500", "per_state", pairing, hi=6)
    both = device("300x1500", "per_state", pairing, hi=B, lo=6, importance=first)
    assert np.array_equal(both, whole)
    # accumulating over no states leaves importance alone; without accumulation no states give zeros
    h, n = handle("300x1500"), dc.synth_case("300x1500").net.n_species
    none = dict(k=np.empty((0, 1500)), pairing=pairing)
    assert np.array_equal(h.drgep_batched(np.empty((0, n)), TG, importance=whole, **none), whole)
    assert np.all(h.drgep_batched(np.empty((0, n)), TG, **none) == 0.0)


def test_device_pointers_equal_host_arrays():
    import torch
    case, h = dc.synth_case("1000x5000"), handle("1000x5000")
    want = staged("1000x5000", "per_state", 1)[0]
    dev = "cuda:0"
    d_u, d_k = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (case.U[:B], case.K[:B]))
    d_t = torch.tensor(TG, dtype=torch.int64, device=dev)
    d_i = torch.full((len(want),), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    stream = torch.cuda.current_stream().cuda_stream
    h.drgep_batched_dev(B, d_u.data_ptr(), d_t.data_ptr(), len(TG), d_i.data_ptr(), d_k=d_k.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_i.cpu().numpy(), want)
    h.drgep_batched_dev(3, d_u.data_ptr(), d_t.data_ptr(), len(TG), d_i.data_ptr(), d_k=d_k.data_ptr(), accumulate=True, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_i.cpu().numpy(), want)


def _pars(t1, chunks, save=-1.0, maxiters=100000):
    return capi.KinParams(tspan0=0.0, tspan1=t1, abstol=1e-10, reltol=1e-8, adaptive_tols=1, update_tols=0, solve_chunks=1 if chunks else 0,
                          ban_negatives=0, solve_chunkstep=t1 / max(chunks, 1), maxiters=maxiters, save_interval=save, dtmin=0.0)


# cap 2: KIN_SLICES_MAX = 2, so that a task walks every other row of the record and skips, inside its walk, the rows a short
# member has not saved
@pytest.mark.parametrize("pairing,cap", [(1, None), (0, None), (1, 2), (0, 2)], ids=["1", "0", "1-cap2", "0-cap2"])
def test_solution_and_ensemble_forms_equal_the_batched_call(pairing, cap, monkeypatch):
    if cap:
        monkeypatch.setenv("KIN_SLICES_MAX", str(cap))
    net, Ea, A = dc.synth(300, 1500)
    case = dc.synth_case("300x1500")
    h = capi.HipNetwork.from_flat(net)
    u0 = np.zeros(300); u0[0] = 1.0
    h.set_rates(case.k0)
    t, us, rc, st, status = h.solve(_pars(2e-3, 2), u0)
    assert rc == 0 and len(t) >= 3
    want = h.drgep_batched(us, TG, pairing=pairing)
    assert want[0] == 1.0 and np.sum(want > 0) > 3
    assert np.array_equal(h.solution_drgep(TG, pairing=pairing), want)
    krow = np.zeros(len(t), np.int64)
    assert np.array_equal(h.solution_drgep(TG, k=case.k0[None, :], k_row=krow, pairing=pairing), want)
    assert np.array_equal(h.solution_drgep(TG, pairing=pairing, importance=want), want)
    # an ensemble of three members with their own rate constants; member 1 fails early (rate constants beyond any step size) and
    # has fewer saved rows: the rows past n_saved take no part
    K = 3
    k = case.K[:K].copy()
    k[1] *= 1e40
    u0s = np.repeat(u0[None, :], K, axis=0)
    res = h.solve_ensemble(_pars(2e-3, 2, save=2.5e-4, maxiters=3000), u0s, k=k)
    Ke, rows, n, n_saved = h.ensemble_size()
    assert Ke == K and rows == 9 and n_saved[0] == 9 and n_saved[2] == 9 and n_saved[1] < 9
    us_e = np.asarray(res[1]).reshape(K, -1, n)
    k_row = np.repeat(np.arange(K, dtype=np.int64)[:, None], rows, axis=1)
    for m in range(K):
        k_row[m, n_saved[m]:] = 10 ** 9           # keys of rows that do not exist are ignored
    got = h.ensemble_drgep(TG, k=k, k_row=k_row, pairing=pairing)
    flat = np.concatenate([us_e[m, :n_saved[m]] for m in range(K)])
    flat_row = np.concatenate([np.full(n_saved[m], m, np.int64) for m in range(K)])
    assert np.all(np.isfinite(got)) and got[0] == 1.0
    assert np.array_equal(got, h.drgep_batched(flat, TG, k=k, k_row=flat_row, pairing=pairing))
    h.close()


def test_error_statuses():
    from kinetica_jl_amd.synth import synthetic_crn
    net, Ea, A = synthetic_crn(50, 200, seed=3)
    h = capi.HipNetwork.from_flat(net)
    U = np.ones((4, 50)); K = np.ones((4, 200)); T = np.full(4, 800.0)

    def code(fn):
        with pytest.raises(capi.KineticaHipError) as e:
            fn()
        return e.value.code

    INV, STATE = capi.KIN_ERR_INVALID_ARG, capi.KIN_ERR_STATE
    E = len(h.drg_pattern(1)[1])
    assert code(lambda: h.drgep_batched(U, [0])) == STATE                                    # no rates at all
    assert code(lambda: h.drgep_batched(U, [0], T=T)) == STATE                               # T without Arrhenius parameters
    assert code(lambda: h.solution_drgep([0], k=K[:1], k_row=np.zeros(0, np.int64))) == STATE    # no stored solution
    assert code(lambda: h.ensemble_drgep([0])) == STATE                                      # no stored ensemble
    h.set_arrhenius(Ea, A)
    assert code(lambda: h.drgep_batched(U, [0], k=K, T=T)) == INV                            # both k and T
    assert code(lambda: h.drgep_batched(U, [50], k=K)) == INV                                # target out of range
    assert code(lambda: h.drgep_batched(U, [-1], k=K)) == INV
    assert code(lambda: h.drgep_batched(U, [], k=K)) == INV                                  # n_targets = 0
    assert code(lambda: h.drgep_paths(np.zeros((2, E)), [])) == INV
    assert code(lambda: h.drgep_paths(np.zeros((2, E)), [50])) == INV
    for bad in (1.5, -0.25, np.nan, np.inf):                                                 # r outside [0, 1] or not finite
        r = np.full((2, E), 0.5); r[1, E // 2] = bad
        assert code(lambda: h.drgep_paths(r, [0])) == INV
    assert code(lambda: h.drgep_batched(U, [0], k=K[:3])) == INV                             # k_row == NULL needs n_k_rows == B
    L = capi.lib()
    tg = np.zeros(1, np.int64)
    assert L.kin_drgep_batched(h.handle, 1, 4, capi._pd(U), capi._pd(K), 4, None, None, capi._p64(tg), 1, 0, 0, None, None, None, None) == INV
    assert L.kin_drgep_batched_dev(h.handle, 1, -1, None, None, None, None, None, 1, 0, None, None) == INV
    # a valid call still works afterwards
    imp = h.drgep_batched(U, [0], k=K)
    assert imp[0] == 1.0 and np.all((imp >= 0.0) & (imp <= 1.0))
    h.close()
