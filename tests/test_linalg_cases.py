"""CPU tests of tests/linalg_cases.py: the structures the GPU tests of the host-driven Newton linear algebra
(tests/test_gpu_newton_linalg.py) are named after, predicted by the symbolic analysis alone (capi.lu_analyze_host with the
elimination parameters the host-driven solver uses), and the references themselves on a matrix with a known solution."""
import numpy as np
import pytest
import scipy.sparse as sp

from kinetica_jl_amd import capi
from oracle import oracle as orc
from tests import linalg_cases as lc


def predicted(net):
    p = capi.lu_analyze_host(net, **lc.host_lu_options(net.n_species))
    return p["ns"], p["m"], p["rounds"]


@pytest.mark.parametrize("m", lc.NEWTON_DENSE_SWEEP)
def test_dense_sweep_structures(m):
    net, ns, rounds = lc.dense_sweep_net(m)
    assert predicted(net) == (ns, m, rounds) and ns + m == net.n_species
    if m >= 15:
        assert 36 <= ns <= 51


def test_dense_sweep_reaches_every_branch():
    ms = lc.NEWTON_DENSE_SWEEP
    steps = {(m + 63) // 64 * 2 for m in ms}                  # Gauss-Jordan block steps = mpad / 32
    assert {m % 64 for m in ms} >= {0, 1, 63}
    assert {2, 4, 6, 8} <= steps and any(s >= 16 for s in steps)
    # the GEMV: lane 0 takes the unrolled trip when m > 192, lane 63 when m > 255, lane 0 a second trip when m > 448
    for lo, edge, hi in ((128, 192, 255), (192, 256, 448), (256, 448, 704)):
        assert any(lo < m <= edge for m in ms) and any(edge < m <= hi for m in ms), edge
    assert {191, 192, 193, 255, 256, 257, 449} <= set(ms)


def test_chain_and_degenerate_structures():
    for n_chain, rounds, nnzZ in ((8, 4, 169), (16, 5, 494)):
        p = capi.lu_analyze_host(lc.core_net(129, n_chain=n_chain))
        assert (p["m"], p["rounds"], p["nnzZ"]) == (129, rounds, nnzZ)
    assert predicted(lc.pairs_net()) == (40, 0, 2)
    assert predicted(lc.core_net(12, n_chain=0)) == (0, 12, 0)
    assert predicted(lc.autocatalytic((1, 0))[0]) == (1, 1, 1)
    assert predicted(lc.autocatalytic((0, 1))[0]) == (1, 1, 1)


@pytest.mark.parametrize("L", lc.NEWTON_HUB_LENGTHS)
def test_hub_structures(L):
    """12288 / 12289 cross the size at which the solver eliminates with its looser parameters; still m = 2"""
    net = lc.hub_net(L)
    p = capi.lu_analyze_host(net, **lc.host_lu_options(net.n_species))
    assert (p["ns"], p["m"], p["rounds"], p["nnzLZ"]) == (L, 2, 1, 2 * L)
    assert set(lc.NEWTON_HUB_ALL_FORMS) <= set(lc.NEWTON_HUB_LENGTHS)


@pytest.mark.parametrize("q,p", lc.NEWTON_DENSE_PIVOTS)
def test_dense_pivot_structures(q, p):
    """the species with the vanishing pivot sits at dense position p, and the matrix is singular at c* to rounding"""
    net, k, u, c_star = lc.dense_pivot_net(q, p)
    assert predicted(net) == (net.n_species - q, q, 2)
    on = orc.OracleNetwork.from_flat(net)
    assert abs(np.linalg.det(lc.newton_matrix(on, k, u, c_star).toarray())) < 1e-10
    for c in (0.9 * c_star, 1.1 * c_star):
        assert lc.cond_of(lc.newton_matrix(on, k, u, c)) < 1e3 and c * abs(on.jac(k, u)).max() >= 1.0
    blocks = {(pp // 32, pp % 32 >= 16) for _, pp in lc.NEWTON_DENSE_PIVOTS}
    assert {(0, False), (0, True), (1, False), (1, True), (4, False), (5, True)} <= blocks


def test_references_on_a_known_solution():
    rng = np.random.default_rng(0)
    M = (sp.identity(50) + 0.1 * sp.random(50, 50, 0.2, random_state=1)).tocsr()
    x = rng.standard_normal(50)
    b = M @ x
    e_bwd, e_fwd = lc.solve_errors(M, x, b)
    assert e_bwd < 1e-15 and e_fwd < 1e-14
    x2 = x.copy(); x2[7] *= 1.0 + 1e-9
    e_bwd, e_fwd = lc.solve_errors(M, x2, b)
    assert e_bwd > 1e-11 and e_fwd > 1e-10
    assert abs(lc.cond_of(M) / np.linalg.cond(M.toarray()) - 1.0) < 1e-12
    c1 = np.linalg.cond(M.toarray(), 1)
    assert 0.3 * c1 <= lc.cond_of(M, dense_max=0) <= 1.0001 * c1
