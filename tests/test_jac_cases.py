"""CPU checks of tests/jac_cases.py (no GPU, no oracle library): the reference on networks worked out by hand, the pattern, the
plan class every case is named after, the derived bounds against a float64 evaluation of the same terms in reversed order, and
bit-for-bit exactness of float64 sums of the exact inputs in two orders. tests/test_gpu_jacobian.py judges the kernels with the
same references and bounds."""
import numpy as np
import pytest

from tests import jac_cases as jc
from tests.jac_cases import LD

F64 = np.float64
ALL = list(jc.CASES)


def test_reference_by_hand():
    """A -> 3B (k0), 2B -> A (k1), A + B -> C (k2), C -> A + B (k3) at u = (a, b, c)"""
    net, ref = jc.case("triple_product")
    k = np.array([2.0, 3.0, 5.0, 7.0]); a, b, c = 0.5, 2.0, 1.0
    u = np.array([a, b, c])
    f, S, L = ref.rhs(k, u)
    r0, r1, r2, r3 = 2 * a, 3 * b * b, 5 * a * b, 7 * c
    assert list(f) == [-r0 + r1 - r2 + r3, 3 * r0 - 2 * r1 - r2 + r3, r2 - r3]
    assert list(S) == [r0 + r1 + r2 + r3, 3 * r0 + 2 * r1 + r2 + r3, r2 + r3] and list(L) == [4, 4, 2]
    assert list(ref.rowptr) == [0, 3, 6, 9] and list(ref.cols) == [0, 1, 2] * 3
    J, SJ, LJ = ref.jac(k, u)
    want = [[-2 - 5 * b, 2 * 3 * b - 5 * a, 7], [6 - 5 * b, -2 * 2 * 3 * b - 5 * a, 7], [5 * b, 5 * a, -7]]
    assert np.array_equal(J.reshape(3, 3), np.array(want, dtype=LD))
    assert list(LJ) == [2, 2, 1, 2, 2, 1, 1, 1, 1]


def test_conventions_collider_and_self_product():
    """A + C -> B + C: C multiplies the rate and has no row term, but column C exists in rows A and B; B -> A + B: row B gets no
    term; 2A -> B: one column with 2 k u"""
    net, ref = jc.case("empty_rows")
    k = np.array([3.0, 5.0, 7.0]); u = np.array([0.5, 2.0, 4.0, 1.0, 1.0])
    f, S, L = ref.rhs(k, u)
    ra, rb, rc = 3 * 0.5 * 4, 5 * 2 * 4, 7 * 0.25
    assert list(f) == [-ra + rb - 2 * rc, ra - rb, 0, 0, rc] and list(L) == [3, 2, 0, 0, 1]
    J, SJ, LJ = ref.jac(k, u)
    dense = np.zeros((5, 5), LD); dense[ref.rows, ref.cols] = J
    assert dense[0, 0] == -3 * 4 - 2 * (2 * 7 * 0.5) and dense[0, 2] == -3 * 0.5 + 5 * 2 and dense[4, 0] == 2 * 7 * 0.5
    for i in (2, 3, 4):                                      # diagonal present, without a term
        assert LJ[ref.diag[i]] == 0 and J[ref.diag[i]] == 0
    assert not np.any(ref.rows == 2) or list(ref.cols[ref.rows == 2]) == [2]


@pytest.mark.parametrize("name", ALL)
def test_pattern_and_class(name):
    net, ref = jc.case(name)
    assert ref.rowptr[0] == 0 and ref.rowptr[-1] == ref.nnz
    for i in range(min(ref.N, 300)):
        c = ref.cols[ref.rowptr[i]:ref.rowptr[i + 1]]
        assert np.all(np.diff(c) > 0) and i in c
    assert np.array_equal(ref.rows[ref.diag], np.arange(ref.N)) and np.array_equal(ref.cols[ref.diag], np.arange(ref.N))
    # the class the case is named after, predicted from the reference's row lengths
    exp = jc.expected(name)
    for which, L in (("rhs", ref.L_rhs), ("jac", ref.L_jac)):
        if exp["plan"] not in (which, "both"):
            continue
        pred = jc.plan_class(L)
        pred["wg"] = 1024 if pred["B"] else 256
        for q, v in exp.items():
            if q != "plan":
                assert pred[q] == v, (name, which, q, pred, exp)


def test_case_list_covers_the_classes():
    names = " ".join(ALL)
    for L in jc.HUB_LENGTHS:
        assert f"hub_{L}_" in names
    assert {jc._hub_class(L) for L in jc.HUB_LENGTHS} == {"ell", "wave", "block1", "block2", "block3"}
    for t in jc.ROW_COUNTS:
        for tag in ("short", "long"):
            assert f"rhs_rows_{t}_{tag}" in jc.CASES and f"jac_rows_{t}_{tag}" in jc.CASES
    net, ref = jc.case("hub_24577_block3")
    assert (ref.N, ref.R) == (24579, 24577)
    # the zero_operand state does zero an A + B operand and a 2A operand where the network has both
    net, ref = jc.case("special_stoichiometries_60")
    u, k = jc.state("special_stoichiometries_60", "zero_operand")
    r = ref.rates(k, u)
    assert np.any((r == 0) & (ref.b >= 0) & (ref.b != ref.a)) and np.any((r == 0) & (ref.b == ref.a))


@pytest.mark.parametrize("name", ALL)
def test_reversed_order_float64_stays_inside_every_bound(name):
    """the same terms, formed in float64 operation by operation and summed in sequence in reversed order"""
    net, ref = jc.case(name)
    for kind in jc.STATE_KINDS:
        u, k = jc.state(name, kind)
        f, S, L = ref.rhs(k, u)
        idx, v = ref.rhs_terms(k, u, F64)
        f64 = jc.sum64(idx, v, ref.N, reverse=True)
        ok, ratio = jc.compare(f64, f, jc.bound_rhs(S, L))
        assert ok, (name, kind, "rhs", jc.worst(f64, f, jc.bound_rhs(S, L)))
        J, SJ, LJ = ref.jac(k, u)
        idx, v = ref.jac_terms(k, u, F64)
        j64 = jc.sum64(idx, v, ref.nnz, reverse=True)
        okj, ratio_j = jc.compare(j64, J, jc.bound_jac(SJ, LJ))
        assert okj, (name, kind, "jac", jc.worst(j64, J, jc.bound_jac(SJ, LJ)))
        c, psi, d = jc.resid_inputs(name, kind)
        g, scale, Lr = ref.resid(k, u, c, psi, d)
        g64 = F64(c) * f64 - psi - d
        okr, ratio_r = jc.compare(g64, g, jc.bound_resid(scale, Lr))
        assert okr, (name, kind, "resid", jc.worst(g64, g, jc.bound_resid(scale, Lr)))
        assert max(ratio, ratio_j, ratio_r) < 1.0


@pytest.mark.parametrize("name", ALL)
def test_exact_inputs_are_exact_in_any_order(name):
    net, ref = jc.case(name)
    u, k = jc.state(name, "exact")
    assert set(np.unique(u)) <= set(jc.EXACT_U) and np.all(k == np.round(k)) and k.min() >= 1 and k.max() <= 8
    f, S, L = ref.rhs(k, u)
    J, SJ, LJ = ref.jac(k, u)
    assert float(max(S.max(), SJ.max())) < 2.0 ** 20
    idx, v = ref.rhs_terms(k, u, F64)
    jdx, w = ref.jac_terms(k, u, F64)
    c, psi, d = jc.resid_inputs(name, "exact")
    g, scale, _ = ref.resid(k, u, c, psi, d)
    for rev in (False, True):
        f64 = jc.sum64(idx, v, ref.N, reverse=rev)
        assert np.array_equal(f64.astype(LD), f), (name, rev)
        assert np.array_equal(jc.sum64(jdx, w, ref.nnz, reverse=rev).astype(LD), J), (name, rev)
        assert np.array_equal((F64(c) * f64 - psi - d).astype(LD), g), (name, rev)
    # a shuffled order too (what a gather plan does to the list order)
    p = np.random.default_rng(1).permutation(len(idx))
    assert np.array_equal(jc.sum64(idx[p], v[p], ref.N).astype(LD), f)


@pytest.mark.parametrize("name", ("synthetic_300", "synthetic_1000"))
def test_entrywise_bound_sees_what_the_normwise_measure_misses(name):
    """the tenth of the Jacobian entries with the smallest scale set to zero: invisible to max|Jd - Jo| <= 1e-13 max|Jo|,
    far outside the entrywise bound; and one dropped term of an exact evaluation is a bitwise difference"""
    net, ref = jc.case(name)
    u, k = jc.state(name, "loguniform")
    J, SJ, LJ = ref.jac(k, u)
    idx, v = ref.jac_terms(k, u, F64)
    j64 = jc.sum64(idx, v, ref.nnz)
    cut = np.sort(SJ[SJ > 0])[len(SJ[SJ > 0]) // 10]
    mut = np.where(SJ <= cut, 0.0, j64)
    assert float(np.max(np.abs(mut.astype(LD) - J)) / np.max(np.abs(J))) <= 1e-13
    ok, ratio = jc.compare(mut, J, jc.bound_jac(SJ, LJ))
    assert not ok and ratio > 1e3
    u, k = jc.state(name, "exact")
    J, SJ, LJ = ref.jac(k, u)
    idx, v = ref.jac_terms(k, u, F64)
    drop = np.ones(len(idx), bool); drop[len(idx) // 2] = False
    assert not np.array_equal(jc.sum64(idx[drop], v[drop], ref.nnz).astype(LD), J)
