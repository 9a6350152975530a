"""GPU tests of the resident kernel's own linear algebra (kinetica_jl_amd/csrc/resident.hip) through kin_resident_probe: the
right-hand side gather (ph_rhs), the analytic Jacobian (ph_jac), the factorisation of M = I - c J (ph_factor: sparse rounds, the
blocked Gauss-Jordan inverse of the dense Schur block, its vanished-pivot flag) and the solve (fused / explicit / plain forms,
the dense GEMV), each run once on given inputs and compared with an independent reference: the oracle's RHS and Jacobian, the
residual of M x - b summed in extended precision, and SuperLU (pivoted) for the forward error. Every case asserts from the probe's
`info` that it reached the structure it is named after (dense block size m, nb = ceil(m / 16) block steps, solve form,
descriptors in LDS), so coverage cannot shrink unnoticed. The largest errors each case measured are printed at the end of the
module (pytest -s)."""
import numpy as np
import pytest
import scipy.sparse as sp

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import FlatNetwork, from_lists, synthetic_crn
from oracle import oracle as orc
from tests.jac_cases import Reference, bound_jac, compare, worst
from tests.linalg_cases import (C_VALUES, SYNTH_COND, SYNTH_U, core_net, dense_pivot_net as _dense_pivot_net, record, solve_errors,
                                static_handle, with_special_stoichiometries)

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nresident linalg probe: largest errors per case (rhs / jac relative to the oracle scale, backward, forward vs SuperLU)")
        for case, v in sorted(MEASURED.items()):
            print(f"  {case:40s} rhs {v[0]:.2e}  jac {v[1]:.2e}  bwd {v[2]:.2e}  fwd {v[3]:.2e}")


_REFS = {}


def reference_of(on):
    """the term-list reference of tests/jac_cases.py for the network behind an oracle handle, built once per handle"""
    if id(on) not in _REFS:
        _REFS[id(on)] = (on, Reference(FlatNetwork(on.n, on.nr, on.rp, on.ri, on.rs, on.pp, on.pi, on.ps)))
    return _REFS[id(on)][1]


def check_member(h, on, k, u, c, b, out, i, case, fwd_cond_max=None):
    """member i of a probe against the references; returns (rhs, jac, backward, forward) errors. fwd_cond_max: the forward error
    is bounded only where cond(M) is at most this (the backward error always)."""
    n = len(u)
    e_rhs = float(np.max(np.abs(out["du"][i] - on.rhs(k, u)) / (on.abs_rhs(k, u) + 1e-300)))
    rowptr, col = h.jac_pattern()
    Jd = sp.csr_matrix((out["jac"][i], col, rowptr), shape=(n, n))
    Jo = on.jac(k, u)
    e_jac = float(abs(Jd - Jo).max() / abs(Jo).max())
    ref = reference_of(on)     # entry by entry as well (tests/jac_cases.py): the normwise measure misses entries small against the largest
    J, S, L = ref.jac(k, u)
    ok, _ = compare(out["jac"][i], J, bound_jac(S, L))
    assert ok, (case, c, worst(out["jac"][i], J, bound_jac(S, L)))
    M = (sp.identity(n, format="csr") - c * Jo).tocsr()
    e_bwd, e_fwd = solve_errors(M, out["x"][i], b)
    record(MEASURED, case, (e_rhs, e_jac, e_bwd, e_fwd))
    assert e_rhs < 1e-13, (case, c, e_rhs)
    assert e_jac < 1e-13, (case, c, e_jac)
    assert e_bwd < 1e-13, (case, c, e_bwd)
    if fwd_cond_max is None or np.linalg.cond(M.toarray()) <= fwd_cond_max:
        assert e_fwd <= 1e-9, (case, c, e_fwd)
    return e_rhs, e_jac, e_bwd, e_fwd


def probe_all_c(h, on, k, u_rng, n, case, cs=C_VALUES, u_decades=(-4, 0), fwd_cond_max=None):
    """one launch, one member per c (own u and b each), every member against the references"""
    K = len(cs)
    U = 10.0 ** u_rng.uniform(*u_decades, (K, n))
    B = u_rng.standard_normal((K, n))
    out = h.resident_probe(U, np.array(cs), B)
    assert (out["bad"] == 0).all(), (case, out["bad"])
    for i, c in enumerate(cs):
        check_member(h, on, k, U[i], c, B[i], out, i, case, fwd_cond_max)
    return out


def look_ahead(nb):
    """gj_blocked: the last wavefront forms and inverts the next pivot block when the strips spread over 7 wavefronts in as many
    rounds as over 8"""
    return (nb + 6) // 7 == (nb + 7) // 8


# m: every nb from 1 to 9, nb = 15, 16, 17, 23 and the RES_MAX_DENSE end; m % 16 in {0, 1, 15} throughout. nb = 8, 15, 16, 23, 32
# run the Gauss-Jordan without look-ahead, odd nb copy the inverse back from the scratch block, m > 128 takes the 16-lane GEMV.
DENSE_SWEEP = (15, 16, 17, 32, 47, 64, 65, 95, 97, 113, 128, 129, 240, 241, 271, 368, 497, 511, 512)


@pytest.mark.parametrize("m", DENSE_SWEEP, ids=lambda m: f"m{m}_nb{(m + 15) // 16}")
def test_dense_block_sweep(m):
    net = core_net(m)
    assert capi.lu_analyze_host(net, min_round=2)["m"] == m
    h, on, k = static_handle(net, m)
    out = probe_all_c(h, on, k, np.random.default_rng(100 + m), net.n_species, f"dense m={m}")
    inf = out["info"]
    assert inf["m"] == m and inf["ns"] == net.n_species - m and inf["solve_form"] == 0
    assert list(inf["dense_species"]) == list(range(m))
    h.close()


def test_dense_sweep_reaches_every_branch():
    nbs = [(m + 15) // 16 for m in DENSE_SWEEP]
    assert set(range(1, 10)) <= set(nbs) and {15, 16, 17, 23, 32} <= set(nbs)
    assert {m % 16 for m in DENSE_SWEEP} >= {0, 1, 15}
    assert any(not look_ahead(nb) for nb in nbs) and any(look_ahead(nb) and nb > 8 for nb in nbs)
    assert any(nb % 2 == 1 for nb in nbs) and any(m > 128 for m in DENSE_SWEEP) and max(DENSE_SWEEP) == 512
    assert [look_ahead(nb) for nb in (7, 8, 9, 14, 15, 16, 17, 21, 22, 24, 28, 29, 32)] == \
        [True, False, True, True, False, False, True, True, False, False, True, False, False]


def test_no_dense_block_all_dense_and_single_pivot_block():
    """m = 0 (20 disjoint pairs: two sparse rounds eliminate everything; explicit triangular form, no GEMV), ns = 0 (a clique of
    12: no sparse round; plain form) and m = 1 (the autocatalytic pair with B first: a 1 x 1 Schur complement)"""
    n = 40
    pairs = from_lists(n, [[(2 * i, 1)] for i in range(20)] + [[(2 * i + 1, 2)] for i in range(20)],
                       [[(2 * i + 1, 1)] for i in range(20)] + [[(2 * i, 1)] for i in range(20)])
    for net, case, m, ns, form in ((pairs, "pairs m=0", 0, 40, 1), (core_net(12, n_chain=0), "clique ns=0", 12, 0, 2),
                                   (from_lists(2, [[(1, 1), (0, 1)]], [[(1, 2)]]), "pair m=1", 1, 1, 0)):
        h, on, k = static_handle(net, m, 0.0, 0.5 if m == 1 else 4.0)
        out = probe_all_c(h, on, k, np.random.default_rng(m), net.n_species, case)
        assert (out["info"]["m"], out["info"]["ns"], out["info"]["solve_form"]) == (m, ns, form), (case, out["info"])
        h.close()


@pytest.mark.parametrize("mode", ["fused", "explicit", "plain"])
def test_the_three_solve_forms(mode, monkeypatch):
    """KIN_LU_FUSED=0 / KIN_LU_EXPLICIT=0 (a fresh handle per setting: the analysis runs once per handle), at m = 129 (16-lane
    GEMV, nb = 9 with look-ahead) and on the 300-species synthetic network (m = 108)"""
    env = {"fused": {}, "explicit": {"KIN_LU_FUSED": "0"}, "plain": {"KIN_LU_EXPLICIT": "0"}}[mode]
    for q, v in env.items():
        monkeypatch.setenv(q, v)
    form = {"fused": 0, "explicit": 1, "plain": 2}[mode]
    net = core_net(129)
    h, on, k = static_handle(net, 129)
    out = probe_all_c(h, on, k, np.random.default_rng(129), net.n_species, f"form {mode} m=129")
    assert out["info"]["solve_form"] == form and out["info"]["m"] == 129
    h.close()
    net, Ea, A = synthetic_crn(300, 1500)
    h = capi.HipNetwork.from_flat(net)
    h.set_arrhenius(Ea, A, k_max=1e12)
    k = h.rates_at(1000.0)
    out = probe_all_c(h, orc.OracleNetwork.from_flat(net), k, np.random.default_rng(300), 300, f"form {mode} synth 300",
                      u_decades=SYNTH_U, fwd_cond_max=SYNTH_COND)
    assert out["info"]["solve_form"] == form and out["info"]["m"] == 108
    h.close()


def test_descriptors_in_lds_and_not():
    """The corrector plans' task descriptors go to LDS where that costs no second workgroup per compute unit: both decisions,
    each against the references"""
    seen = {}
    for n in (300, 500, 600, 700, 800):
        net, Ea, A = synthetic_crn(n, 5 * n)
        h = capi.HipNetwork.from_flat(net)
        h.set_arrhenius(Ea, A, k_max=1e12)
        k = h.rates_at(1000.0)
        out = probe_all_c(h, orc.OracleNetwork.from_flat(net), k, np.random.default_rng(n), n, f"descriptors synth {n}", cs=(1e-8, 1e-3),
                          u_decades=SYNTH_U, fwd_cond_max=SYNTH_COND)
        seen.setdefault(out["info"]["desc_in_lds"], n)
        h.close()
    assert set(seen) == {0, 1}, seen


@pytest.mark.parametrize("n,r,seed,m", [(60, 300, 11, 31), (100, 500, None, 55), (300, 1500, None, 108), (1000, 5000, None, 237)],
                         ids=["synth60", "synth100", "synth300", "synth1000"])
def test_synthetic_networks_with_special_stoichiometries(n, r, seed, m):
    """the networks the trajectory tests send through the kernel, at 1000 K, plus 2A -> B, A -> 2B, an inert collider and a
    product that is also a reactant"""
    net, Ea, A = synthetic_crn(n, r) if seed is None else synthetic_crn(n, r, seed=seed)
    for special in (False, True):
        nt = with_special_stoichiometries(net) if special else net
        h = capi.HipNetwork.from_flat(nt)
        k = orc.arrhenius(Ea, A, 1000.0, k_max=1e12)
        if special:
            k = np.concatenate([k, [3.0, 2.0, 5.0, 7.0]])
        h.set_rates(k)
        out = probe_all_c(h, orc.OracleNetwork.from_flat(nt), k, np.random.default_rng(n), n, f"synth {n}{' special' if special else ''}",
                          u_decades=SYNTH_U, fwd_cond_max=SYNTH_COND)
        if not special:
            assert out["info"]["m"] == m
        h.close()


@pytest.mark.parametrize("L", [8, 9, 32, 33, 64, 65, 256, 257, 512, 513])
def test_gather_row_length_edges(L):
    """a hub in L reactions (hub + s_i -> sink): its RHS row and its Jacobian entries J[hub, hub], J[sink, hub] gather L terms -
    ELL to segment, 8 to 16 to 64 lanes, segment to long row, a long row's second pass"""
    n = L + 2
    net = from_lists(n, [[(0, 1), (i, 1)] for i in range(1, L + 1)], [[(L + 1, 1)] for _ in range(L)])
    h, on, k = static_handle(net, L, -1.0, 2.0)
    probe_all_c(h, on, k, np.random.default_rng(L), n, f"hub row L={L}")
    h.close()


def _autocatalytic(order):
    a, b = order
    return from_lists(2, [[(a, 1), (b, 1)]], [[(a, 2)]]), a, b


@pytest.mark.parametrize("order,c_sing,where", [((0, 1), 0.25, "sparse"), ((1, 0), 1.0 / 3.0, "schur1x1")], ids=["sparse_pivot", "schur_1x1"])
def test_vanished_pivot_of_the_autocatalytic_pair(order, c_sing, where):
    """A + B -> 2A, k = 2, A = 0.5, B = 2: with A first the sparse pivot 1 - c k B vanishes at c = 1/4, with B first the 1 x 1
    Schur complement 1 - 3 c at c = 1/3; at c = 0.125 the flag stays down and x is right"""
    net, a, b = _autocatalytic(order)
    h = capi.HipNetwork.from_flat(net)
    k = np.array([2.0])
    h.set_rates(k)
    u = np.zeros(2); u[a] = 0.5; u[b] = 2.0
    rhs = np.array([1.0, -1.0])
    out = h.resident_probe(np.tile(u, (2, 1)), np.array([c_sing, 0.125]), np.tile(rhs, (2, 1)))
    assert out["info"]["m"] == 1 and out["info"]["ns"] == 1
    assert out["bad"][0] == 1 and out["bad"][1] == 0
    check_member(h, orc.OracleNetwork.from_flat(net), k, u, 0.125, rhs, out, 1, f"pair {where} c=0.125")
    h.close()


@pytest.mark.parametrize("q,p", [(48, 37), (128, 117)], ids=["look_ahead_nb3", "no_look_ahead_nb8"])
def test_vanished_pivot_inside_a_later_dense_block(q, p):
    """the flag rises when the pivot at dense position p (block p // 16 > 0, row p % 16 of that block) vanishes - inverted by the
    look-ahead wavefront at nb = 3, by wavefront 0 at nb = 8 - and not at a c 10 % away"""
    nb = (q + 15) // 16
    net, k, u, c_star = _dense_pivot_net(q, p)
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    rng = np.random.default_rng(p)
    cs = np.array([c_star, 0.9 * c_star, 1.1 * c_star])
    B = rng.standard_normal((3, net.n_species))
    out = h.resident_probe(np.tile(u, (3, 1)), cs, B)
    inf = out["info"]
    assert inf["m"] == q and inf["dense_species"][p] == p and p // 16 > 0 and look_ahead(nb) == (q == 48)
    assert list(out["bad"]) == [1, 0, 0]
    on = orc.OracleNetwork.from_flat(net)
    for i in (1, 2):
        check_member(h, on, k, u, cs[i], B[i], out, i, f"dense pivot q={q} p={p}")
    h.close()


def test_members_of_one_launch_are_their_solo_launches():
    """K members with their own u, c and b in one launch, one of them with a vanishing dense pivot: each member is bit for bit its
    K = 1 launch, and the failing member flags no other"""
    net, k, u, c_star = _dense_pivot_net(48, 37)
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    rng = np.random.default_rng(7)
    K = 6
    U = np.tile(u, (K, 1)) * np.where(np.arange(K)[:, None] == 2, 1.0, rng.uniform(0.5, 2.0, (K, net.n_species)))
    cs = np.array([1e-12, 1e-5, c_star, 0.5, 1e-3, 0.9 * c_star])
    B = rng.standard_normal((K, net.n_species))
    out = h.resident_probe(U, cs, B)
    assert out["bad"][2] == 1 and out["bad"].sum() == 1
    for i in range(K):
        o1 = h.resident_probe(U[i], cs[i], B[i])
        assert o1["bad"][0] == out["bad"][i]
        for key in ("du", "jac", "x"):
            assert np.array_equal(o1[key][0], out[key][i], equal_nan=True), (i, key)
    on = orc.OracleNetwork.from_flat(net)
    for i in (0, 1, 4):
        check_member(h, on, k, U[i], cs[i], B[i], out, i, "members of one launch")
    h.close()


def test_probe_refuses_what_the_kernel_does_not_take():
    """KIN_ERR_STATE without rates; KIN_ERR_UNSUPPORTED beyond the kernel (dense block > 512)"""
    net = core_net(30)
    h = capi.HipNetwork.from_flat(net)
    with pytest.raises(capi.KineticaHipError) as e:
        h.resident_probe(np.ones(net.n_species), 1e-3, np.ones(net.n_species))
    assert e.value.code == capi.KIN_ERR_STATE
    h.close()
    net = core_net(520)
    assert capi.lu_analyze_host(net, min_round=2)["m"] == 520
    h, _, _ = static_handle(net, 5)
    with pytest.raises(capi.KineticaHipError) as e:
        h.resident_probe(np.ones(net.n_species), 1e-3, np.ones(net.n_species))
    assert e.value.code == capi.KIN_ERR_UNSUPPORTED and "dense" in str(e.value)
    h.close()
