"""Shared by tests/test_gpu_resident_linalg.py and tests/test_gpu_newton_linalg.py: the constructed networks whose Newton matrices
have a known structure (dense Schur block size, sparse rows, gather-row lengths, a pivot that vanishes at a known c), the
references a device solve of (I - c J) x = b is compared with (the residual summed in extended precision, SuperLU with pivoting),
and the bookkeeping of the largest errors each case measured. A plain module: no fixtures, no test collection."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from kinetica_jl_amd import capi
from kinetica_jl_amd.synth import from_lists
from oracle import oracle as orc

C_VALUES = (1e-12, 1e-8, 1e-5, 1e-3)

# Synthetic networks at 1000 K (rate constants up to k_max = 1e12) take the states of the host path's test
# (test_gpu_boundary_r2.py: test_newton_matrix_solve_against_sparse_direct), 1e-8 .. 1e-2. At c = 1e-3 their Newton matrices
# have condition numbers of 1e11 .. 5e12: there the kernel (static diagonal pivoting, explicit inverses) differed from SuperLU by
# up to 5.7e-8 of max|x| at backward errors below 1e-13 (LAPACK's pivoted dense solve differs from SuperLU by up to 6e-10 on the
# same matrices). The forward bound of 1e-9 holds for these networks where cond(M) <= 1e10; the backward bound everywhere.
SYNTH_U = (-8, -2)
SYNTH_COND = 1e10

BWD_MAX = 1e-13     # the project's bounds for a Newton-matrix solve (both existing Newton tests use them)
FWD_MAX = 1e-9


def core_net(q, n_chain=3):
    """A core of q species that the symbolic analysis never eliminates (each has more than 8 non-hub neighbours: all pairs for
    q <= 20, else neighbours i +- 1 .. 5), reversible unimolecular reactions between neighbours, and sparse chains hanging off it
    (prev -> c, 2 c -> prev: the 2A Jacobian term). The dense Schur block is the core in ascending species order (m = q)."""
    reacs, prods = [], []
    pairs = [(i, j) for i in range(q) for j in range(i + 1, q)] if q <= 20 else [(i, (i + o) % q) for i in range(q) for o in range(1, 6)]
    for i, j in pairs:
        reacs += [[(i, 1)], [(j, 1)]]; prods += [[(j, 1)], [(i, 1)]]
    n = q
    for i in range(0, q, max(1, q // 12)):
        prev = i
        for _ in range(n_chain):
            reacs += [[(prev, 1)], [(n, 2)]]; prods += [[(n, 1)], [(prev, 1)]]
            prev = n; n += 1
    return from_lists(n, reacs, prods)


def with_special_stoichiometries(net):
    """net plus 2A -> B, A -> 2B, A + C -> B + C (inert collider C) and B -> A + B (a product that is also a reactant)."""
    rs = [net.reaction(r) for r in range(net.n_reactions)]
    extra = [([(0, 2)], [(1, 1)]), ([(0, 1)], [(1, 2)]), ([(0, 1), (2, 1)], [(1, 1), (2, 1)]), ([(1, 1)], [(0, 1), (1, 1)])]
    return from_lists(net.n_species, [r for r, _ in rs] + [r for r, _ in extra], [p for _, p in rs] + [p for _, p in extra])


def pairs_net(n_pairs=20):
    """n_pairs disjoint pairs A -> B, 2B -> A: two sparse rounds eliminate everything (m = 0)"""
    return from_lists(2 * n_pairs, [[(2 * i, 1)] for i in range(n_pairs)] + [[(2 * i + 1, 2)] for i in range(n_pairs)],
                      [[(2 * i + 1, 1)] for i in range(n_pairs)] + [[(2 * i, 1)] for i in range(n_pairs)])


def hub_net(L):
    """a hub in L reactions hub + s_i -> sink (hub = species 0, sink = species L + 1): the hub's RHS row and the Jacobian entries
    J[hub, hub], J[sink, hub] gather L terms; in the factorisation the L species s_i are one sparse round, hub and sink the dense
    block (m = 2), and every entry of its Schur update gathers L terms"""
    return from_lists(L + 2, [[(0, 1), (i, 1)] for i in range(1, L + 1)], [[(L + 1, 1)] for _ in range(L)])


def autocatalytic(order):
    """A + B -> 2A with A = species order[0], B = species order[1]; returns (net, a, b)"""
    a, b = order
    return from_lists(2, [[(a, 1), (b, 1)]], [[(a, 2)]]), a, b


def dense_pivot_net(q, p):
    """core_net(q) with weak coupling everywhere and A_p + B -> 2 A_p on the species at dense position p (B: a new species): the
    Schur pivot of A_p is (1 + c k (u_A - u_B)) / (1 + c k u_A) up to the weak terms, zero at c* = 1 / (k (u_B - u_A))"""
    base = core_net(q)
    B = base.n_species
    rs = [base.reaction(r) for r in range(base.n_reactions)]
    net = from_lists(B + 1, [r for r, _ in rs] + [[(p, 1), (B, 1)]], [pp for _, pp in rs] + [[(p, 2)]])
    k = np.full(net.n_reactions, 1e-12); k[-1] = 1.0
    u = np.full(net.n_species, 0.1); u[p] = 0.5; u[B] = 2.0
    return net, k, u, 1.0 / (1.0 * (2.0 - 0.5))


def static_handle(net, seed, lo=0.0, hi=4.0):
    k = 10.0 ** np.random.default_rng(seed).uniform(lo, hi, net.n_reactions)
    h = capi.HipNetwork.from_flat(net)
    h.set_rates(k)
    return h, orc.OracleNetwork.from_flat(net), k


def residual_ld(M, x, b):
    """M x - b with every product and sum in extended precision (np.longdouble)."""
    M = M.tocsr()
    prod = M.data.astype(np.longdouble) * x[M.indices].astype(np.longdouble)
    r = np.zeros(M.shape[0], np.longdouble)
    np.add.at(r, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), prod)
    return r - b.astype(np.longdouble)


def newton_matrix(on, k, u, c):
    """I - c J(u) from the oracle's Jacobian (CSR)"""
    n = len(u)
    return (sp.identity(n, format="csr") - c * on.jac(k, u)).tocsr()


def solve_errors(M, x, b, lu=None):
    """(backward, forward) error of x as a solution of M x = b: max|M x - b| in extended precision relative to
    max(|M||x|) + max|b|, and max|x - x_SuperLU| relative to max|x_SuperLU| (lu: splu(M), when the caller has it already)"""
    r = residual_ld(M, x, b)
    e_bwd = float(np.max(np.abs(r))) / (float(np.max(abs(M) @ np.abs(x))) + float(np.max(np.abs(b))))
    xr = (lu or spl.splu(M.tocsc())).solve(b)
    e_fwd = float(np.max(np.abs(x - xr)) / np.max(np.abs(xr)))
    return e_bwd, e_fwd


def cond_of(M, dense_max=3000, lu=None):
    """cond(M): the 2-norm condition number from the dense matrix up to dense_max rows; beyond, where that is too slow, the
    1-norm estimate ||M||_1 ||M^-1||_1 (Hager / Higham, M^-1 applied through SuperLU; lu: splu(M), when the caller has it)"""
    n = M.shape[0]
    if n <= dense_max:
        return float(np.linalg.cond(M.toarray()))
    lu = lu or spl.splu(M.tocsc())
    inv = spl.LinearOperator((n, n), matvec=lu.solve, rmatvec=lambda v: lu.solve(v, "T"), dtype=np.float64)
    return float(spl.onenormest(M.tocsc()) * spl.onenormest(inv))


def record(measured, case, errs):
    """keep the largest of each error measured under `case`"""
    prev = measured.get(case, (0.0,) * len(errs))
    measured[case] = tuple(max(a, bb) for a, bb in zip(prev, errs))


def host_lu_options(n_species):
    """the elimination parameters the host-driven solver analyses with (lu.hpp: lu_options_for), as arguments of capi.lu_analyze_host"""
    return dict(max_tail_degree=32, max_rounds=16, max_degree=400) if n_species >= 4000 else {}


# ---- the host-driven path's cases (tests/test_gpu_newton_linalg.py); their structure is predicted without a device in
# tests/test_linalg_cases.py

# dense block sizes: m % 64 in {0, 1, 63}; mpad / 32 = 2, 4, 6, 8, 10, 16, 18, 34; both sides of the GEMV's trip boundaries
# (lane 0 takes the unrolled trip from m = 193, a second one from 449; 256 / 257 is where a lane's fourth column starts)
NEWTON_DENSE_SWEEP = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 449, 513, 1025)

# hub row lengths: ELL group / one wavefront at 8 / 9, one wavefront / whole workgroup at 256 / 257, one pass / two passes of a
# whole-workgroup row at 12288 / 12289 (SegPlanHost::BLK_PASS)
NEWTON_HUB_LENGTHS = (8, 9, 64, 65, 256, 257, 1024, 1025, 12288, 12289)
NEWTON_HUB_ALL_FORMS = (256, 257, 12288, 12289)

# (q, p): a pivot vanishing at dense position p of dense_pivot_net(q, p). Pivot blocks are 32 x 32, inverted as two 16 x 16
# halves; block 0 by gj_pivot_kernel, every later one by the look-ahead workgroup of the update before it
NEWTON_DENSE_PIVOTS = ((48, 5), (48, 21), (48, 37), (64, 53), (200, 133), (200, 183), (200, 199))


def dense_sweep_net(m):
    """the network of dense-sweep entry m: (net, expected ns, expected rounds)"""
    if m == 1:
        return autocatalytic((1, 0))[0], 1, 1
    if m == 2:
        return hub_net(40), 40, 1
    net = core_net(m)
    return net, net.n_species - m, 2
