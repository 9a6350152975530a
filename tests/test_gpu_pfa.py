"""GPU tests of path flux analysis (kin_pfa_batched, kin_pfa_paths and the solution / ensemble forms) against the NumPy
reference of pfa_cases.py.

The split stage (rp, rc) is compared within the bound derived in pfa_cases.py, per (edge, state); test_pfa_host.py checks on
the CPU that at most 1 % of those bounds are above 1e-9, and the tests here repeat that on what they compare. The second
stage is compared on the device's own rp and rc within its relative bound (deg_A + 4) 2^-52 ref, and the coefficients are the
exact maximum of the staged per-state r. Everything that only rearranges the states - blocks, halves folded with accumulate,
a second call, device pointers, the stored solution and ensemble, the row classes - is compared bit for bit.

Largest error / bound ratios printed on an MI355X when this was written: split stage 0.146, second stage 0.250 (0.246 on the
random coefficients of the paths entry)."""
import numpy as np
import pytest

import drg_cases as dc
import pfa_cases as pc
from kinetica_jl_amd import capi
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S

pytestmark = pytest.mark.gpu

B = pc.B_GPU
_handles, _stages = {}, {}


def handle(name):
    if name not in _handles:
        _handles[name] = capi.HipNetwork.from_flat(dc.synth_case(name).net)
    return _handles[name]


def device(name, mode, pairing, hi=B, lo=0, coef=None, stages=False):
    """pfa_batched of states lo .. hi - 1 of a synthetic case."""
    case, h = dc.synth_case(name), handle(name)
    if mode == "shared":
        h.set_rates(case.k0)
    elif mode.startswith("T"):
        h.set_arrhenius(case.Ea, case.A, k_max=1e12 if mode == "T_kmax" else None)
    src = {k: (v[lo:] if k != "k" or mode == "per_state" else v) for k, v in case.source(mode, hi).items()}
    return h.pfa_batched(case.U[lo:hi], pairing=pairing, coef=coef, stages=stages, **src)


def staged(name, mode, pairing):
    """(coef, rp, rc, r) of the first B states, computed once and left unchanged."""
    key = (name, mode, pairing)
    if key not in _stages:
        _stages[key] = device(name, mode, pairing, stages=True)
    return _stages[key]


def check_second(g, rp, rc, r, what):
    ref = g.second_all(rp, rc)
    bound = g.second_bound(ref)
    err = np.abs(r - ref)
    print(f"{what}: pairs {g.E2}, largest row of E {g.deg.max()}, max err {err.max():.3e}, max err/bound "
          f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.isfinite(r)) and np.all(r >= 0.0)
    assert np.all(r[ref == 0.0] == 0.0)
    assert np.all(err <= bound)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(pc.hand_networks()))
def test_hand_networks(name, pairing):
    net, k, U, want = pc.hand_networks()[name]
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    rowptr, colidx = h.pfa_pattern(pairing)
    pairs = [(a, int(b)) for a in range(net.n_species) for b in colidx[rowptr[a]:rowptr[a + 1]]]
    assert pairs == sorted(want[pairing])
    coef, rp, rc, r = h.pfa_batched(U, pairing=pairing, stages=True)
    values = [want[pairing][p] for p in pairs]
    assert coef.tolist() == values and r[0].tolist() == values                          # dyadic inputs: exact
    assert r[-1].tolist() == [0.0] * len(pairs) and np.all(rp[-1] == 0.0) and np.all(rc[-1] == 0.0)    # den = 0: 0.0, never NaN
    assert h.pfa_batched(np.zeros((1, net.n_species)), pairing=pairing).tolist() == [0.0] * len(pairs)
    if name == "chain":
        drg = h.drg_pattern(pairing)
        assert 2 not in drg[1][drg[0][0]:drg[0][1]]                                     # kin_drg_pattern has no edge (A, B)
    h.close()


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name,mode", pc.GPU_CASES)
def test_split_stage_within_the_derived_bound(name, mode, pairing):
    _, rp, rc, _ = staged(name, mode, pairing)
    rp_ref, rc_ref, bp, bc = pc.ref(name, mode, pairing)
    for what, got, ref, bound in (("rp", rp, rp_ref, bp), ("rc", rc, rc_ref, bc)):
        frac = float(np.mean(bound > 1e-9))
        err = np.abs(got - ref)
        print(f"{name} {mode} pairing={pairing} {what}: edges {ref.shape[1]}, max err {err.max():.3e}, max err/bound "
              f"{np.max(err / np.maximum(bound, 1e-300)):.3f}, {100 * frac:.3f} % of the bounds above 1e-9")
        assert frac <= 0.01
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        assert np.all(err <= bound)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name,mode", [("300x1500", "per_state"), ("300x1500", "T"), ("300x1500_cut", "per_state"), ("1000x5000", "per_state")])
def test_second_stage_on_the_device_coefficients(name, mode, pairing):
    coef, rp, rc, r = staged(name, mode, pairing)
    g = pc.graph(name, pairing)
    if name == "1000x5000":
        assert g.deg.max() > 256                       # rows with more than 256 out-edges (484 with pairing)
    if name == "300x1500_cut":
        assert np.any(g.s.num[:, 3] < 0)               # records without a reverse
    check_second(g, rp, rc, r, f"{name} {mode} pairing={pairing}")
    assert np.array_equal(coef, r.max(axis=0))         # the maximum over the states is exact


@pytest.mark.parametrize("name", ["300x1500", "1000x5000"])
def test_paths_entry_on_random_coefficients(name):
    g, h = pc.graph(name, 1), handle(name)
    rng = np.random.default_rng(7)
    rp, rc = rng.random((5, g.E)) ** 3, rng.random((5, g.E)) ** 3
    for x in (rp, rc):
        x[rng.random(x.shape) < 0.3] = 0.0
        x[rng.random(x.shape) < 0.05] = 1.0
    rc[3] = 0.0                                        # production alone
    coef, r = h.pfa_paths(rp, rc, pairing=1, stages=True)
    check_second(g, rp, rc, r, f"{name} random")
    assert np.array_equal(coef, r.max(axis=0))
    # accumulation: the given coefficients take part, values above every r survive
    assert np.array_equal(h.pfa_paths(rp[:2], rc[:2], coef=h.pfa_paths(rp[2:], rc[2:])), coef)
    top = np.full(g.E2, 1e6)
    assert np.array_equal(h.pfa_paths(rp, rc, coef=top), top)
    assert np.array_equal(h.pfa_paths(rp[:0], rc[:0], coef=coef), coef) and np.all(h.pfa_paths(rp[:0], rc[:0]) == 0.0)


@pytest.mark.parametrize("mode", ["per_state", "T"])
def test_blocks_halves_and_repeats_bit_for_bit(mode, monkeypatch):
    whole = staged("300x1500", mode, 1)
    assert np.array_equal(device("300x1500", mode, 1), whole[0])                         # two identical calls
    first = device("300x1500", mode, 1, hi=3)
    assert np.array_equal(device("300x1500", mode, 1, hi=B, lo=3, coef=first), whole[0])   # two halves folded with accumulate
    monkeypatch.setenv("KIN_DRG_BLOCK_STATES", "3")                                      # blocks of 3, 3 and 1 states
    for a, b in zip(device("300x1500", mode, 1, stages=True), whole):
        assert np.array_equal(a, b)
    # accumulating over no states leaves coef alone; without accumulation no states give zeros
    h, n = handle("300x1500"), dc.synth_case("300x1500").net.n_species
    none = dict(k=np.empty((0, 1500)), pairing=1)
    assert np.array_equal(h.pfa_batched(np.empty((0, n)), coef=whole[0], **none), whole[0])
    assert np.all(h.pfa_batched(np.empty((0, n)), **none) == 0.0)


@pytest.mark.parametrize("name", ["300x1500", "1000x5000"])
def test_row_classes_bit_for_bit(name, monkeypatch):
    """Every row by a workgroup, every row by a wavefront, the rows above the median cost by a workgroup, and the default: the
    same bits."""
    whole = staged(name, "per_state", 1)
    g = pc.graph(name, 1)
    cost = np.array([g.deg[g.cols[g.rowptr[a]:g.rowptr[a + 1]]].sum() for a in range(g.n)])
    median = int(np.median(cost[cost > 0]))
    assert np.any(cost > median) and np.any((cost > 0) & (cost <= median))
    for wg_cost in ("0", str(10 ** 9), str(median)):
        monkeypatch.setenv("KIN_PFA_WG_COST", wg_cost)
        for a, b in zip(device(name, "per_state", 1, stages=True), whole):
            assert np.array_equal(a, b)


def test_device_pointers_equal_host_arrays():
    import torch
    case, h = dc.synth_case("1000x5000"), handle("1000x5000")
    want = staged("1000x5000", "per_state", 1)[0]
    dev = "cuda:0"
    d_u, d_k = (torch.tensor(x, dtype=torch.float64, device=dev) for x in (case.U[:B], case.K[:B]))
    d_c = torch.full((len(want),), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()      # torch's fills run on torch's stream, the library on the handle's own
    stream = torch.cuda.current_stream().cuda_stream
    h.pfa_batched_dev(B, d_u.data_ptr(), d_c.data_ptr(), d_k=d_k.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_c.cpu().numpy(), want)
    h.pfa_batched_dev(3, d_u.data_ptr(), d_c.data_ptr(), d_k=d_k.data_ptr(), accumulate=True, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_c.cpu().numpy(), want)


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
    want = h.pfa_batched(us, pairing=pairing)
    assert np.sum(want > 0) > 3
    assert np.array_equal(h.solution_pfa(pairing=pairing), want)
    krow = np.zeros(len(t), np.int64)
    assert np.array_equal(h.solution_pfa(k=case.k0[None, :], k_row=krow, pairing=pairing), want)
    assert np.array_equal(h.solution_pfa(pairing=pairing, coef=want), want)
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
    got = h.ensemble_pfa(k=k, k_row=k_row, pairing=pairing)
    flat = np.concatenate([us_e[m, :n_saved[m]] for m in range(K)])
    flat_row = np.concatenate([np.full(n_saved[m], m, np.int64) for m in range(K)])
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, h.pfa_batched(flat, k=k, k_row=flat_row, pairing=pairing))
    h.close()


CHAIN_K = np.array([1.0, 1.0, 1e-3, 1e-3])      # A -> M, M -> B, and the inert side branch M -> C -> D
CHAIN_EPS, CHAIN_T1 = 0.6, 0.8


def test_reduce_network_pfa_keeps_what_drg_drops():
    """A -> M -> B with k = (1, 1) from A alone: q_MB / q_AM = t. Up to t = 0.8 the DRG edge (M, B) carries at most
    q_MB / (q_AM + q_MB + q_MC) < 0.8 / 1.8 = 0.45 and (A, B) is no DRG edge, while PFA's r_AB = rc_AM rc_MB reaches 0.8:
    at eps = 0.6 DRG from target A drops B, PFA keeps it. Both drop the side branch (coefficients of 1e-3)."""
    from oracle import oracle as orc
    net = pc.side_branch_network()
    names = ["A", "M", "B", "C", "D"]
    sd = S.SpeciesData.from_names(names)
    rd = S.RxData.from_flat(net)
    calc = S.DummyKineticCalculator(CHAIN_K)
    cond = C.ConditionSet({"T": 300.0})
    pars = S.ODESimulationParams(tspan=(0.0, CHAIN_T1), u0={"A": 1.0}, solve_chunkstep=0.1, abstol=1e-12, reltol=1e-10, low_k_cutoff="none")
    full = S.solve_network(S.StaticODESolve(pars, cond, calc), sd, rd)
    assert full.sol.retcode == "Success" and len(full.sol.t) == 9
    # the reference first, on the exact solution of the chain at the saved times (k_MB + k_MC = 1.001 = 1 + d)
    t = np.asarray(full.sol.t)
    d = 1e-3
    u_ref = np.zeros((len(t), 5))
    u_ref[:, 0] = np.exp(-t)
    u_ref[:, 1] = np.exp(-t) * -np.expm1(-d * t) / d
    on = orc.OracleNetwork.from_flat(net)
    rates = np.stack([on.rates(CHAIN_K, x) for x in u_ref])
    g, dg = pc.PfaRef(net, 1), dc.DrgRef(net, 1)
    pcoef = g.coefficients(rates)[0]
    dcoef = dg.coefficients(rates)[0]
    assert dc.select(g.rowptr2, g.colidx2, pcoef, [0], CHAIN_EPS).tolist() == [0, 1, 2]
    assert dc.select(dg.rowptr, dg.colidx, dcoef, [0], CHAIN_EPS).tolist() == [0, 1]
    pair = {(int(a), int(b)): v for a, b, v in zip(g.rows2, g.cols2, pcoef)}
    assert 0.79 < pair[(0, 2)] < 0.8 and abs(pair[(0, 2)] - CHAIN_EPS) > 0.1
    # the device pipeline
    red = S.reduce_network(full, calc, ["A"], CHAIN_EPS, method="pfa")
    assert np.array_equal(red.rowptr, g.rowptr2) and np.array_equal(red.colidx, g.colidx2)
    # (the saved A and M agree with the exact ones to the solve's tolerances; the reference states leave C and D at zero)
    main = [i for i, p in enumerate(zip(g.rows2, g.cols2)) if p in ((0, 1), (0, 2), (1, 0), (1, 2))]
    print(f"coefficients of A and M towards A, M, B, device against reference: max |difference| {np.max(np.abs(red.coef - pcoef)[main]):.3e}")
    assert np.max(np.abs(red.coef - pcoef)[main]) < 1e-6
    assert red.species_kept.tolist() == [0, 1, 2] and red.reactions_kept.tolist() == [0, 1]
    assert red.sd.toInt == {"A": 1, "M": 2, "B": 3} and red.rd.nr == 2
    drg = S.reduce_network(full, calc, ["A"], CHAIN_EPS, method="drg")
    assert drg.species_kept.tolist() == [0, 1] and drg.reactions_kept.tolist() == [0]


def test_size_limit_status_and_message():
    from kinetica_jl_amd.synth import from_lists
    n = capi.PFA_MAX_SPECIES + 1
    h = capi.HipNetwork.from_flat(from_lists(n, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(n - 1, 1)]]))
    h.set_rates(np.ones(2))
    rowptr, colidx = h.pfa_pattern(1)                   # the pattern alone has no limit
    assert len(colidx) == 6
    for call in (lambda: h.pfa_batched(np.ones((1, n))), lambda: h.pfa_paths(np.ones((1, 4)), np.ones((1, 4)))):
        with pytest.raises(capi.KineticaHipError) as e:
            call()
        assert e.value.code == capi.KIN_ERR_UNSUPPORTED and f"at most {capi.PFA_MAX_SPECIES} species" in str(e.value)
    h.close()
    # one species below: taken
    h = capi.HipNetwork.from_flat(from_lists(n - 1, [[(0, 1)], [(1, 1)]], [[(1, 1)], [(n - 2, 1)]]))
    h.set_rates(np.array([4.0, 4.0]))
    u = np.zeros((1, n - 1)); u[0, 0] = 0.5; u[0, 1] = 0.25
    assert h.pfa_batched(u).tolist() == [1.0, 0.5, 1.0, 0.5, 1.0, 1.0]      # the chain's values, rows A, M, B = 0, 1, n - 2
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
    E, E2 = len(h.drg_pattern(1)[1]), len(h.pfa_pattern(1)[1])
    assert E2 > E
    assert code(lambda: h.pfa_batched(U)) == STATE                                          # no rates at all
    assert code(lambda: h.pfa_batched(U, T=T)) == STATE                                     # T without Arrhenius parameters
    assert code(lambda: h.solution_pfa(k=K[:1], k_row=np.zeros(0, np.int64))) == STATE      # no stored solution
    assert code(lambda: h.ensemble_pfa()) == STATE                                          # no stored ensemble
    h.set_arrhenius(Ea, A)
    assert code(lambda: h.pfa_batched(U, k=K, T=T)) == INV                                  # both k and T
    assert code(lambda: h.pfa_batched(U, k=K[:3])) == INV                                   # k_row == NULL needs n_k_rows == B
    for bad in (-0.25, np.nan, np.inf):                                                     # negative or not finite
        for which in (0, 1):
            r = [np.full((2, E), 0.5), np.full((2, E), 0.5)]
            r[which][1, E // 2] = bad
            assert code(lambda: h.pfa_paths(r[0], r[1])) == INV
    assert code(lambda: h.pfa_batched(U, k=K, coef=np.zeros(E))) == INV                     # a coef of the DRG pattern's size
    assert code(lambda: h.pfa_paths(np.zeros((1, E)), np.zeros((1, E)), coef=np.zeros(E2 + 1))) == INV
    L = capi.lib()
    z = np.zeros((2, E))
    out = np.zeros(E2)
    assert L.kin_pfa_batched(h.handle, 1, 4, capi._pd(U), capi._pd(K), 4, None, None, 0, None, None, None, None) == INV
    assert L.kin_pfa_batched(h.handle, 1, 4, None, capi._pd(K), 4, None, None, 0, capi._pd(out), None, None, None) == INV
    assert L.kin_pfa_batched_dev(h.handle, 1, -1, None, None, None, None, 0, None, None) == INV
    assert L.kin_pfa_paths(h.handle, 1, 2, capi._pd(z), None, 0, capi._pd(out), None) == INV
    assert L.kin_pfa_paths(h.handle, 1, 2, capi._pd(z), capi._pd(z), 0, None, None) == INV
    assert L.kin_pfa_paths(None, 1, 2, capi._pd(z), capi._pd(z), 0, capi._pd(out), None) == INV
    assert L.kin_pfa_pattern(None, 1, 0, None, None, None) == INV
    # a valid call still works afterwards (without pairing: with it, equal rates cancel in every pair); r is not clipped at 1
    assert np.all(h.pfa_batched(U, k=K) == 0.0)
    coef = h.pfa_batched(U, k=K, pairing=0)
    assert np.all(np.isfinite(coef)) and np.all(coef >= 0.0) and coef.max() > 0.0
    assert h.pfa_paths(np.ones((1, E)), np.ones((1, E))).max() > 2.0
    h.close()
