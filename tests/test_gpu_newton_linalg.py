"""GPU tests of the host-driven Newton-matrix linear algebra (kinetica_jl_amd/csrc/lu.cpp, solver_kernels.hip, the gather
traversal seg_traverse of segsum_dev.hpp and gemv_row of step_dev.hpp: every solve above the resident kernel's size, the thread and lockstep ensembles) through kin_newton_probe: the scatter of I - c J with the identity on
the dense block's padding rows, the sparse elimination rounds and their gather plans, the monomial kernel and the LZ / NVU
products, the blocked Gauss-Jordan inverse on the FP64 matrix cores (single-matrix and batched chains, the look-ahead workgroup,
the vanished-pivot flag), the one-wavefront-per-row GEMV and the three solve forms. Every member of every case is compared with
two independent references - the residual M x - b summed in extended precision (backward error < 1e-13) and SuperLU with
pivoting (forward error <= 1e-9 of max|x| where cond(M) <= 1e10) - with M from the oracle's Jacobian; never with another device
path. Every case asserts from the probe's `info` that it reached the structure it is named after, and before touching the device
that capi.lu_analyze_host predicts that structure (tests/test_linalg_cases.py checks the predictions on machines without a GPU).

The forward bound is left out only for members of the synthetic networks with cond(M) > 1e10; they are counted, and the last test
fails when they exceed a tenth of all members checked. Every constructed case has a member with max|c J| >= 1 (at c <= 1e-8 the
matrix is the identity to 1e-4 and a wrong off-diagonal tile would hardly show).

Not covered: the limits at which the analysis gives up the explicit inverses (4 M monomials) or the fused products (16 M terms) -
no network of a size this suite can afford reaches them. (The corrector update fused into the solve's last launch -
stagec_newton_kernel - and the lockstep ensemble's batched vector kernels: tests/test_gpu_step_kernels.py, through kin_step_probe.)
The largest errors each case measured are printed at the end of the module (pytest -s).

Mutation check (value-only changes to the product kernels on a scratch build, one at a time, this file without the 3 000- and
10 000-species cases; nothing of it is kept): which tests here fail, and what the suite before this file did.
  1 gj_update_body stores +acc in the pivot columns: 43 fail - dense_block_sweep m >= 33, deep_sparse_chains, the_three_solve_forms,
    every vanished_pivot_in_the_dense_block, batched_inverse_* K = 1 / 16 / 17, pivot_inside_a_full_batched_chain, both slot
    reuse tests, newton_solve_is_the_probe, synthetic 1000. Before: the first failure was a trajectory comparison
    (test_synchronising_hand_over_gives_the_same_trajectory).
  2 the GEMV's (now gemv_row's) final add drops acc3: 17 fail - dense_block_sweep m = 193 .. 1025, vanished_pivot_in_the_dense_block q = 200, both
    slot reuse tests, newton_solve_is_the_probe, synthetic 1000. Before: test_newton_matrix_solve_against_sparse_direct (m = 501).
  3 gj_update_batched_kernel reads B.pinv[0]: 15 fail - every batched case with more than one member (vanished pivots, the pair,
    m = 0 / ns = 0, batched_inverse_* K = 16 / 17, pivot_inside_a_full_batched_chain, slot reuse, synthetic 1000); K = 1 and all
    single-matrix cases pass. Before: test_lockstep_ensemble_of_a_large_network, whose chains depend on thread timing.
  4 segsum_kernel (now seg_traverse, which it wraps) skips the second pass of a whole-workgroup row: 3 fail - gather_row_lengths L = 12289 in the three forms
    (L = 12288 passes). Before: no failure in the 68 tests that ran before a time limit ended that run; not determined further.
  5 lu_assemble_kernel writes the padding identity one row off: 62 fail - everything with padding rows (m % 64 != 0);
    dense_block_sweep m = 64, 128, 192, 256 and vanished_pivot q = 64 pass. Before: the same trajectory comparison as 1."""
import time

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import synthetic_crn
from oracle import oracle as orc
from tests import linalg_cases as lc
from tests.linalg_cases import C_VALUES, SYNTH_COND, SYNTH_U, core_net, dense_pivot_net, static_handle

pytestmark = pytest.mark.gpu

MEASURED = {}
COUNT = {"members": 0, "fwd_skipped": 0}
FORMS = {"fused": 0, "explicit": 1, "rounds": 2}
FORM_ENV = {"fused": {}, "explicit": {"KIN_LU_FUSED": "0"}, "rounds": {"KIN_LU_EXPLICIT": "0"}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    if MEASURED:
        print("\nnewton linalg probe: largest errors per case (backward: extended-precision residual; forward: vs SuperLU)")
        for case, v in sorted(MEASURED.items()):
            print(f"  {case:44s} bwd {v[0]:.2e}  fwd {v[1]:.2e}")
        print(f"  overall: bwd {max(v[0] for v in MEASURED.values()):.2e}  fwd (cond <= 1e10) {max(v[2] for v in MEASURED.values()):.2e}  "
              f"members {COUNT['members']}  forward checks skipped {COUNT['fwd_skipped']}  wall {time.time() - t0:.0f} s")


def set_form(monkeypatch, mode):
    """the switches are read when a handle's analysis runs: set them before the handle's first probe"""
    for q, v in FORM_ENV[mode].items():
        monkeypatch.setenv(q, v)


def predicted(net):
    return capi.lu_analyze_host(net, **lc.host_lu_options(net.n_species))


def assert_structure(net, info, ns, m, rounds, form=None):
    assert (info["ns"], info["m"], info["rounds"]) == (ns, m, rounds), info
    assert info["mpad"] == (0 if m == 0 else (m + 63) // 64 * 64) and info["gj_steps"] == info["mpad"] // 32, info
    assert ns + m == net.n_species
    if form is not None:
        assert info["solve_form"] == form, info


def check_members(on, k, U, cs, B, outs, case, synthetic=False, members=None):
    """every member of `members` (default: all) of every probe result in `outs` (same inputs) against the references"""
    K = len(cs)
    for i in (range(K) if members is None else members):
        M = lc.newton_matrix(on, k, U[i], cs[i])
        lu = spl.splu(M.tocsc())
        cond = lc.cond_of(M, lu=lu)
        for out in outs:
            assert out["bad"][i] == 0, (case, i, out["bad"])
            e_bwd, e_fwd = lc.solve_errors(M, out["x"][i], B[i], lu=lu)
            COUNT["members"] += 1
            lc.record(MEASURED, case, (e_bwd, e_fwd, e_fwd if cond <= SYNTH_COND else 0.0))
            assert e_bwd < lc.BWD_MAX, (case, i, cs[i], e_bwd)
            if cond <= SYNTH_COND:
                assert e_fwd <= lc.FWD_MAX, (case, i, cs[i], e_fwd, cond)
            else:
                assert synthetic, (case, i, cs[i], "cond(M) above 1e10 in a constructed case", cond)
                COUNT["fwd_skipped"] += 1


def inputs(on, k, rng, n, cs, u_decades=(-4, 0), need_big=True):
    """one member per c with u and b of its own; need_big: some member has max|c J| >= 1"""
    K = len(cs)
    U = 10.0 ** rng.uniform(*u_decades, (K, n))
    B = rng.standard_normal((K, n))
    if need_big:
        assert max(cs[i] * abs(on.jac(k, U[i])).max() for i in range(K)) >= 1.0
    return U, np.array(cs, dtype=np.float64), B


def probe_case(h, on, k, rng, n, case, cs=C_VALUES, u_decades=(-4, 0), batched=False):
    U, cs, B = inputs(on, k, rng, n, cs, u_decades)
    out = h.newton_probe(U, cs, B, batched=batched)
    check_members(on, k, U, cs, B, [out], case)
    return out


# ---- (a) dense-block sweep

@pytest.mark.parametrize("m", lc.NEWTON_DENSE_SWEEP, ids=lambda m: f"m{m}")
def test_dense_block_sweep(m):
    net, ns, rounds = lc.dense_sweep_net(m)
    p = predicted(net)
    assert (p["ns"], p["m"], p["rounds"]) == (ns, m, rounds)
    n = net.n_species
    if m == 1:      # A + B -> 2A with B first: the members keep A > B, where det(I - c J) = 1 + c k (A - B) >= 1
        k = np.array([2.0])
        h = capi.HipNetwork.from_flat(net)
        h.set_rates(k)
        on = orc.OracleNetwork.from_flat(net)
        rng = np.random.default_rng(100 + m)
        cs = np.array(C_VALUES + (1.0,))
        U = np.stack([rng.uniform(0.1, 0.5, 5), rng.uniform(1.0, 2.0, 5)], axis=1)      # species 0 is B, species 1 is A
        B = rng.standard_normal((5, 2))
        assert max(cs[i] * abs(on.jac(k, U[i])).max() for i in range(5)) >= 1.0
        out = h.newton_probe(U, cs, B)
        check_members(on, k, U, cs, B, [out], f"dense m={m}")
    elif m == 2:
        h, on, k = static_handle(net, m, -1.0, 2.0)
        out = probe_case(h, on, k, np.random.default_rng(100 + m), n, f"dense m={m}", cs=C_VALUES + (1.0,), u_decades=(-2, 0))
    else:
        h, on, k = static_handle(net, m)
        out = probe_case(h, on, k, np.random.default_rng(100 + m), n, f"dense m={m}")
    assert_structure(net, out["info"], ns, m, rounds, form=0)
    if m > 2:
        assert list(out["info"]["dense_species"]) == list(range(m))
    h.close()


def test_dense_sweep_reaches_every_branch():
    ms = lc.NEWTON_DENSE_SWEEP
    steps = {(m + 63) // 64 * 2 for m in ms}
    assert {m % 64 for m in ms} >= {0, 1, 63}
    assert {2, 4, 6, 8} <= steps and any(s >= 16 for s in steps)
    # the GEMV: lane 0 takes the unrolled trip when m > 192, lane 63 when m > 255, lane 0 a second trip when m > 448
    for lo, edge, hi in ((128, 192, 255), (192, 256, 448), (256, 448, 704)):
        assert any(lo < m <= edge for m in ms) and any(edge < m <= hi for m in ms), edge
    assert {191, 192, 193, 255, 256, 257, 449} <= set(ms)
    assert max(ms) > 1024      # a tile grid beyond 16 x 16, pivot blocks off the grid's diagonal


@pytest.mark.parametrize("n_chain,rounds,nnzZ", [(8, 4, 169), (16, 5, 494)], ids=["chain8", "chain16"])
def test_deep_sparse_chains(n_chain, rounds, nnzZ):
    """chains of 8 and 16 species off the core: 4 and 5 elimination rounds, monomials of several factors in Z and V, a plan
    per round"""
    net = core_net(129, n_chain=n_chain)
    p = predicted(net)
    assert (p["m"], p["rounds"], p["nnzZ"]) == (129, rounds, nnzZ)
    h, on, k = static_handle(net, 129 + n_chain)
    out = probe_case(h, on, k, np.random.default_rng(n_chain), net.n_species, f"chains n_chain={n_chain}")
    assert_structure(net, out["info"], p["ns"], 129, rounds, form=0)
    h.close()


# ---- (b) degenerate structures

def test_no_dense_block_no_sparse_rows_and_a_single_dense_entry():
    """m = 0 (20 disjoint pairs: two sparse rounds eliminate everything; explicit form, no Gauss-Jordan, no GEMV), ns = 0 (a
    clique of 12: no sparse round; round-by-round form, which is then the GEMV alone) and m = 1, ns = 1 (the autocatalytic pair
    with B first: a 1 x 1 Schur complement in a padded 64 x 64 block)"""
    for net, case, m, ns, rounds, form in ((lc.pairs_net(), "pairs m=0", 0, 40, 2, 1), (core_net(12, n_chain=0), "clique ns=0", 12, 0, 0, 2)):
        p = predicted(net)
        assert (p["ns"], p["m"], p["rounds"]) == (ns, m, rounds)
        h, on, k = static_handle(net, m)
        for batched in (False, True):
            out = probe_case(h, on, k, np.random.default_rng(m), net.n_species, case, batched=batched)
            assert_structure(net, out["info"], ns, m, rounds, form=form)
        h.close()
    net, a, b = lc.autocatalytic((1, 0))
    p = predicted(net)
    assert (p["ns"], p["m"], p["rounds"]) == (1, 1, 1)
    h = capi.HipNetwork.from_flat(net)
    k = np.array([2.0])
    h.set_rates(k)
    on = orc.OracleNetwork.from_flat(net)
    u = np.zeros(2); u[a] = 2.0; u[b] = 0.5     # det(I - c J) = 1 + 1.5 k c: regular for every c > 0
    cs = np.array(C_VALUES + (1.0,))
    B = np.random.default_rng(1).standard_normal((5, 2))
    out = h.newton_probe(np.tile(u, (5, 1)), cs, B)
    assert_structure(net, out["info"], 1, 1, 1, form=0)
    check_members(on, k, np.tile(u, (5, 1)), cs, B, [out], "pair m=1 ns=1")
    h.close()


# ---- (c) the three solve forms

@pytest.mark.parametrize("mode", list(FORMS))
def test_the_three_solve_forms(mode, monkeypatch):
    """KIN_LU_FUSED=0 / KIN_LU_EXPLICIT=0 (a fresh handle per setting) on deep chains (4 rounds, m = 129) and on the pairs
    network, where the fused form falls back to the explicit one (no dense block); the hub rows of
    test_gather_row_lengths run in all three forms too"""
    set_form(monkeypatch, mode)
    net = core_net(129, n_chain=8)
    h, on, k = static_handle(net, 137)
    out = probe_case(h, on, k, np.random.default_rng(137), net.n_species, f"form {mode} chains m=129")
    assert_structure(net, out["info"], 104, 129, 4, form=FORMS[mode])
    h.close()
    net = lc.pairs_net()
    h, on, k = static_handle(net, 0)
    out = probe_case(h, on, k, np.random.default_rng(0), net.n_species, f"form {mode} pairs m=0")
    assert_structure(net, out["info"], 40, 0, 2, form=max(FORMS[mode], 1))
    h.close()


# ---- (d) gather-row lengths

@pytest.mark.parametrize("L,mode", [(L, mode) for L in lc.NEWTON_HUB_LENGTHS for mode in FORMS
                                    if mode == "fused" or L in lc.NEWTON_HUB_ALL_FORMS], ids=lambda v: str(v))
def test_gather_row_lengths(L, mode, monkeypatch):
    """a hub in L reactions hub + s_i -> sink: one sparse round of L pivots, hub and sink dense (m = 2). Every entry of the 2 x 2
    Schur update gathers L products, the two dense rows of stage A (fused) / of the dense forward plan (explicit, rounds) gather L
    terms, and the two dense columns feed every sparse row. 8 / 9: ELL group to one wavefront; 256 / 257: one wavefront to a whole
    workgroup; 12288 / 12289: a whole-workgroup row's second pass. The fused plans are value-ordered, the others are not."""
    set_form(monkeypatch, mode)
    net = lc.hub_net(L)
    p = predicted(net)
    assert (p["ns"], p["m"], p["rounds"], p["nnzLZ"]) == (L, 2, 1, 2 * L if mode == "fused" else 0)
    h, on, k = static_handle(net, L, -1.0, 2.0)
    out = probe_case(h, on, k, np.random.default_rng(L), L + 2, f"hub row L={L} {mode}", cs=C_VALUES + (1.0,), u_decades=(-2, 0))
    inf = out["info"]
    assert_structure(net, inf, L, 2, 1, form=FORMS[mode])
    assert sorted(inf["dense_species"]) == [0, L + 1]
    assert inf["max_row"] == L, inf
    assert (inf["long_rows"] > 0) == (L > 256), inf
    h.close()


# ---- (e) vanished pivots

@pytest.mark.parametrize("q,p", lc.NEWTON_DENSE_PIVOTS, ids=lambda v: str(v))
@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
def test_vanished_pivot_in_the_dense_block(q, p, batched):
    """the flag rises when the pivot at dense position p vanishes and not at a c 10 % away. Pivot blocks are 32 x 32, inverted
    as two 16 x 16 halves with a Schur step between them: q = 48: p = 5 / 21 (block 0, inverted by the pivot kernel: first /
    second half), p = 37 (block 1, inverted by the look-ahead workgroup); q = 64: p = 53 (block 1, second half, no padding rows);
    q = 200: p = 133 / 183 (blocks 4 and 5 of a 4 x 4 tile grid), p = 199 (the last real row before 56 padding rows)"""
    net, k, u, c_star = dense_pivot_net(q, p)
    pr = predicted(net)
    assert pr["m"] == q and pr["ns"] == net.n_species - q and pr["rounds"] == 2
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    rng = np.random.default_rng(p)
    cs = np.array([c_star, 0.9 * c_star, 1.1 * c_star])
    U = np.tile(u, (3, 1))
    B = rng.standard_normal((3, net.n_species))
    out = h.newton_probe(U, cs, B, batched=batched)
    inf = out["info"]
    assert_structure(net, inf, net.n_species - q, q, 2, form=0)
    assert inf["dense_species"][p] == p
    assert list(out["bad"]) == [1, 0, 0]
    on = orc.OracleNetwork.from_flat(net)
    assert max(c * abs(on.jac(k, u)).max() for c in cs[1:]) >= 1.0
    check_members(on, k, U, cs, B, [out], f"dense pivot q={q} p={p}", members=(1, 2))
    h.close()


@pytest.mark.parametrize("order,c_sing,where", [((0, 1), 0.25, "sparse"), ((1, 0), 1.0 / 3.0, "schur1x1")], ids=["sparse_pivot", "schur_1x1"])
def test_vanished_pivot_of_the_autocatalytic_pair(order, c_sing, where):
    """A + B -> 2A, k = 2, A = 0.5, B = 2: with A first the sparse pivot 1 - c k B vanishes at c = 1/4 (lu_scale_kernel's flag),
    with B first the 1 x 1 Schur complement 1 - 3 c at c = 1/3 (the pivot kernel's); at c = 0.125 and at c = 1 the flag stays down
    and x is right"""
    net, a, b = lc.autocatalytic(order)
    h = capi.HipNetwork.from_flat(net)
    k = np.array([2.0])
    h.set_rates(k)
    u = np.zeros(2); u[a] = 0.5; u[b] = 2.0
    rhs = np.array([1.0, -1.0])
    cs = np.array([0.125, c_sing, 1.0])
    U, B = np.tile(u, (3, 1)), np.tile(rhs, (3, 1))
    on = orc.OracleNetwork.from_flat(net)
    for batched in (False, True):
        out = h.newton_probe(U, cs, B, batched=batched)
        assert_structure(net, out["info"], 1, 1, 1, form=0)
        assert list(out["bad"]) == [0, 1, 0]
        check_members(on, k, U, cs, B, [out], f"pair {where}", members=(0, 2))
    h.close()


# ---- (f) the batched inverse

def _mixed_members(on, k, rng, n, K):
    cs = np.array([((1e-3, 1.0, 1e-2, 1e-1) + C_VALUES[:3])[i % 7] for i in range(K)])
    return inputs(on, k, rng, n, cs)


@pytest.mark.parametrize("K", [1, 16, 17])
def test_batched_inverse_is_the_single_matrix_inverse(K):
    """K members of core_net(129) with u, c and b of their own (K = 16: a full chain, blockIdx.z up to 15; K = 17: two chains):
    the batched chain gives x and the flags bit for bit as the single-matrix chain does, each member is bit for bit its K = 1
    call, and every member meets the references"""
    net = core_net(129)
    h, on, k = static_handle(net, 129)
    U, cs, B = _mixed_members(on, k, np.random.default_rng(1000 + K), net.n_species, K)
    single = h.newton_probe(U, cs, B, batched=False)
    batch = h.newton_probe(U, cs, B, batched=True)
    assert_structure(net, batch["info"], 39, 129, 2, form=0)
    assert np.array_equal(batch["x"], single["x"]) and np.array_equal(batch["bad"], single["bad"])
    for i in range(K):
        solo = h.newton_probe(U[i], cs[i], B[i], batched=bool(i % 2))
        assert np.array_equal(solo["x"][0], batch["x"][i]) and solo["bad"][0] == batch["bad"][i], i
    check_members(on, k, U, cs, B, [batch], f"batched K={K} m=129")
    h.close()


def test_batched_inverse_of_the_10k_network():
    """4 members of the 10 000-species synthetic network (m = 981, a 16 x 16 tile grid) in one chain"""
    net, Ea, A = synthetic_crn(10000, 50000)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    k = h.rates_at(1000.0)
    on = orc.OracleNetwork.from_flat(net)
    U, cs, B = inputs(on, k, np.random.default_rng(10000), 10000, C_VALUES, u_decades=SYNTH_U, need_big=False)
    single = h.newton_probe(U, cs, B, batched=False)
    batch = h.newton_probe(U, cs, B, batched=True)
    assert batch["info"]["m"] > 512 and batch["info"]["solve_form"] == 0
    assert np.array_equal(batch["x"], single["x"]) and np.array_equal(batch["bad"], single["bad"])
    for i in range(4):
        solo = h.newton_probe(U[i], cs[i], B[i])
        assert np.array_equal(solo["x"][0], batch["x"][i]) and solo["bad"][0] == batch["bad"][i], i
    check_members(on, k, U, cs, B, [batch], "batched K=4 synth 10000", synthetic=True)
    h.close()


def test_vanished_pivot_inside_a_full_batched_chain():
    """16 members in one chain, member 7 with a vanishing dense pivot (block 1: found by the look-ahead workgroup of its own
    matrix): it flags itself and no other, and every other member is bit for bit its solo call"""
    net, k, u, c_star = dense_pivot_net(48, 37)
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    rng = np.random.default_rng(7)
    K = 16
    exact = np.isin(np.arange(K), (6, 7, 8))[:, None]          # members 6 and 8: 10 % either side of the singular c
    U = np.tile(u, (K, 1)) * np.where(exact, 1.0, rng.uniform(0.5, 2.0, (K, net.n_species)))
    cs = np.array([(1e-12, 1e-8, 1e-5, 1e-3, 0.05, 0.1)[i % 6] for i in range(K)])
    cs[6:9] = (0.9 * c_star, c_star, 1.1 * c_star)
    B = rng.standard_normal((K, net.n_species))
    out = h.newton_probe(U, cs, B, batched=True)
    assert out["info"]["m"] == 48
    assert list(out["bad"]) == [int(i == 7) for i in range(K)]
    for i in range(K):
        solo = h.newton_probe(U[i], cs[i], B[i])
        assert solo["bad"][0] == out["bad"][i]
        if i != 7:
            assert np.array_equal(solo["x"][0], out["x"][i]), i
    on = orc.OracleNetwork.from_flat(net)
    check_members(on, k, U, cs, B, [out], "pivot inside a batched chain", members=[i for i in range(K) if i != 7])
    h.close()


# ---- (g) slot reuse

@pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
def test_a_slot_that_flagged_a_pivot_is_reused_cleanly(batched):
    """the probe factorises into the solver's slots 0 .. K-1: after a probe whose first member met a vanished dense pivot (NaN and
    Inf all over its slot), a regular probe on the same handle is bit for bit the same probe on a fresh handle"""
    net, k, u, c_star = dense_pivot_net(200, 183)
    rng = np.random.default_rng(183)
    n = net.n_species
    on = orc.OracleNetwork.from_flat(net)
    U = np.tile(u, (3, 1)) * rng.uniform(0.5, 1.0, (3, n))
    U[:, 183] = 2.0; U[:, n - 1] = 0.5                         # A above B: regular at every c
    cs = np.array([1e-3, 0.3, 1.0])
    B = rng.standard_normal((3, n))
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    first = h.newton_probe(np.tile(u, (3, 1)), np.array([c_star, 0.9 * c_star, 1.1 * c_star]), B, batched=batched)
    assert list(first["bad"]) == [1, 0, 0]
    again = h.newton_probe(U, cs, B, batched=batched)
    h.close()
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    fresh = h.newton_probe(U, cs, B, batched=batched)
    h.close()
    assert np.array_equal(again["x"], fresh["x"]) and not again["bad"].any() and not fresh["bad"].any()
    assert max(c * abs(on.jac(k, uu)).max() for c, uu in zip(cs, U)) >= 1.0
    check_members(on, k, U, cs, B, [again], "slot reuse after a flag")


def test_newton_solve_is_the_probe_of_one_member():
    """kin_newton_solve(c, u, b) is bit for bit kin_newton_probe at K = 1 through the single-matrix chain, on either side of a
    multi-member probe that used the same slots"""
    net = core_net(193, n_chain=8)
    h, on, k = static_handle(net, 193)
    U, cs, B = inputs(on, k, np.random.default_rng(193), net.n_species, C_VALUES)
    x_before = [h.newton_solve(cs[i], U[i], B[i]) for i in range(4)]
    out = h.newton_probe(U, cs, B)
    x_after = [h.newton_solve(cs[i], U[i], B[i]) for i in range(4)]
    for i in range(4):
        solo = h.newton_probe(U[i], cs[i], B[i])
        assert np.array_equal(x_before[i], solo["x"][0]) and np.array_equal(x_after[i], solo["x"][0]), i
        assert np.array_equal(out["x"][i], solo["x"][0]), i
    check_members(on, k, U, cs, B, [out], "newton_solve = probe K=1")
    h.close()


# ---- (h) the trajectory networks

@pytest.mark.parametrize("n", [1000, 3000, 10000])
def test_synthetic_networks_with_special_stoichiometries(n):
    """the networks the headline solves and the ensembles send through these kernels, at 1000 K, plus 2A -> B, A -> 2B, an inert
    collider and a product that is also a reactant; single-matrix and batched chains"""
    net, Ea, A = synthetic_crn(n, 5 * n)
    for special in (False, True):
        nt = lc.with_special_stoichiometries(net) if special else net
        h = capi.HipNetwork.from_flat(nt)
        k = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
        if special:
            k = np.concatenate([k, [3.0, 2.0, 5.0, 7.0]])
        h.set_rates(k)
        on = orc.OracleNetwork.from_flat(nt)
        p = predicted(nt)
        U, cs, B = inputs(on, k, np.random.default_rng(n), n, C_VALUES, u_decades=SYNTH_U, need_big=False)
        outs = [h.newton_probe(U, cs, B, batched=batched) for batched in (False, True)]
        for out in outs:
            assert_structure(nt, out["info"], p["ns"], p["m"], p["rounds"], form=0)
        assert np.array_equal(outs[0]["x"], outs[1]["x"])
        check_members(on, k, U, cs, B, outs, f"synth {n}{' special' if special else ''}", synthetic=True)
        h.close()


# ---- errors, and the share of forward checks left out

def test_probe_refuses_bad_arguments():
    """KIN_ERR_STATE without rates; KIN_ERR_INVALID_ARG for a null buffer"""
    import ctypes
    net = core_net(30)
    h = capi.HipNetwork.from_flat(net)
    with pytest.raises(capi.KineticaHipError) as e:
        h.newton_probe(np.ones(net.n_species), 1e-3, np.ones(net.n_species))
    assert e.value.code == capi.KIN_ERR_STATE
    h.set_rates(np.ones(net.n_reactions))
    v = np.ones(net.n_species)
    bad = np.zeros(1, np.int32)
    info = np.zeros(8 + net.n_species, np.int64)
    P32 = ctypes.POINTER(ctypes.c_int32)
    for K, x in ((0, v), (1, None)):
        st = capi.lib().kin_newton_probe(h._h, K, 0, capi._pd(v), capi._pd(v), capi._pd(v), capi._pd(x), bad.ctypes.data_as(P32), capi._p64(info))
        assert st == capi.KIN_ERR_INVALID_ARG, (K, st)
    h.close()


def test_forward_checks_left_out_stay_below_a_tenth():
    """runs last: the forward bound was left out for synthetic-network members with cond(M) > 1e10 only (check_members), and for
    at most 10 % of all members this module checked"""
    assert COUNT["fwd_skipped"] <= 0.1 * COUNT["members"], COUNT
