"""CPU tests of the timescale analysis: the reference of tests/timescale_cases.py against closed forms, the classes of the row
pass (kin_timescale_plan_host needs no device), and the NumPy side of solving.species_timescales (Timescales, qss_candidates)."""
import numpy as np
import pytest

from kinetica_jl_amd import capi, solving
from kinetica_jl_amd.synth import from_lists
from tests import jac_cases as jc
from tests import timescale_cases as tc

F = lambda a: np.asarray(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ reference
def test_reference_a_to_b():
    ref = jc.Reference(from_lists(2, [[(0, 1)]], [[(1, 1)]]))
    k, A = 4.0, 0.5
    s = tc.StateRef(ref, [k], [A, 2.0])
    assert F(s.d).tolist() == [-k, 0.0]
    assert F(s.f).tolist() == [-k * A, k * A]
    assert F(s.g).tolist() == [k, k] and float(s.norm) == k
    assert F(s.e).tolist() == [A, np.inf]
    assert F(s.e_lo)[1] == np.inf and F(s.e_hi)[1] == np.inf              # nothing consumes B: exactly +Inf
    assert s.e_lo[0] <= A <= s.e_hi[0] and float(s.e_hi[0] - s.e_lo[0]) < 1e-14


def test_reference_a_plus_b_reversible():
    ref = jc.Reference(from_lists(3, [[(0, 1), (1, 1)], [(2, 1)]], [[(2, 1)], [(0, 1), (1, 1)]]))
    k1, k2, A, B, C = 2.0, 8.0, 0.5, 2.0, 1.0
    s = tc.StateRef(ref, [k1, k2], [A, B, C])
    assert F(s.d).tolist() == [-k1 * B, -k1 * A, -k2]
    fA = -k1 * A * B + k2 * C
    assert F(s.f).tolist() == [fA, fA, -fA]
    row = k1 * B + k1 * A + k2
    assert F(s.g).tolist() == [row, row, row] and float(s.norm) == row
    assert F(s.e).tolist() == [abs(fA) / (k1 * B), abs(fA) / (k1 * A), abs(fA) / k2]
    # at equilibrium f = 0 with a bound above 0 (cancellation): the interval starts at 0 and is finite
    q = tc.StateRef(ref, [k1, k2], [2.0, 2.0, 1.0])
    assert F(q.f).tolist() == [0.0, 0.0, 0.0] and F(q.e).tolist() == [0.0, 0.0, 0.0]
    assert np.all(q.e_lo == 0) and np.all(q.e_hi > 0) and np.all(np.isfinite(F(q.e_hi)))


def test_reference_two_a():
    ref = jc.Reference(from_lists(2, [[(0, 2)]], [[(1, 1)]]))
    k, A = 3.0, 2.0
    s = tc.StateRef(ref, [k], [A, 1.0])
    assert F(s.d).tolist() == [-4 * k * A, 0.0]                            # nu = -2 times the single column 2 k u
    assert F(s.f).tolist() == [-2 * k * A * A, k * A * A]
    assert F(s.g).tolist() == [4 * k * A, 2 * k * A]
    assert F(s.e).tolist() == [A / 2, np.inf]


def test_reference_empty_rows():
    net = jc.empty_rows_net()
    ref = jc.Reference(net)
    u, k = np.array([2.0, 1.0, 0.5, 1.0, 2.0]), np.array([1.0, 2.0, 4.0])
    s = tc.StateRef(ref, k, u)
    assert F(s.d)[2:].tolist() == [0.0, 0.0, 0.0] and F(s.bd)[2:].tolist() == [0.0, 0.0, 0.0]
    assert F(s.f)[2:].tolist() == [0.0, 0.0, 4.0 * 2.0 * 2.0]
    assert F(s.e)[2:].tolist() == [0.0, 0.0, np.inf]                       # 0 / 0 is 0.0, f / 0 is +Inf
    assert F(s.e_lo)[2:].tolist() == [0.0, 0.0, np.inf] and F(s.e_hi)[2:].tolist() == [0.0, 0.0, np.inf]
    want = tc.exact_expectation(ref, k[None, :], u[None, :])
    assert want["err"][0, 2:].tolist() == [0.0, 0.0, np.inf]
    assert want["summary"][0, 2:].tolist() == [0.0, 0.0, 0.0] and want["summary"][1, 2:].tolist() == [0.0, 0.0, 0.0]


def test_batch_reference_extrema_and_identity():
    ref = jc.Reference(tc.chain_net())
    Us, K = tc.exact_states(ref, 4, seed=1)
    b = tc.BatchRef(ref, K, Us)
    nd = np.stack([-F(s.d) for s in b.states])
    assert np.array_equal(F(b.summary[0]), nd.max(0)) and np.array_equal(F(b.summary[1]), nd.min(0))
    assert np.all(b.lo <= b.summary) and np.all(b.summary <= b.hi)
    none = tc.BatchRef(ref, K, Us, count=[False] * 4)
    assert np.array_equal(F(none.summary), tc.identity(3))
    half = tc.BatchRef(ref, K, Us, count=[False, False, True, True])
    assert np.array_equal(F(half.summary[0]), nd[2:].max(0))


# ------------------------------------------------------------------------------------------------------- row-pass classes
@pytest.mark.parametrize("entries,cls", [(1, "short"), (8, "short"), (9, "medium"), (256, "medium"), (257, "long")])
def test_plan_classes_of_a_fan_in_row(entries, cls):
    """row H of X_j -> H, j = 1 .. L, stores L + 1 entries; every other row one"""
    L = entries - 1
    net = tc.fan_in_net(L) if L else from_lists(1, [], [])
    info = capi.timescale_plan_host(net)
    ref = jc.Reference(net)
    assert info["nnz"] == ref.nnz == 2 * L + 1
    assert int(np.diff(ref.rowptr)[0]) == entries
    want = dict(rows_short=L, rows_medium=0, rows_long=0)
    want["rows_" + cls] += 1
    assert {q: info[q] for q in want} == want
    assert (capi.TIMESCALE_SHORT_MAX, capi.TIMESCALE_WAVE_MAX) == (8, 256)


def test_plan_of_the_synthetic_case_matches_the_reference_pattern():
    net, ref = jc.case("synthetic_300")
    info = capi.timescale_plan_host(net)
    n = np.diff(ref.rowptr)
    assert info == dict(nnz=ref.nnz, rows_short=int(np.sum(n <= 8)), rows_medium=int(np.sum((n > 8) & (n <= 256))),
                        rows_long=int(np.sum(n > 256)))


# --------------------------------------------------------------------------------------------------------- NumPy side
def _ts(decay_max, decay_min, qss_err):
    a = lambda v: np.asarray(v, dtype=float)
    return solving.Timescales(np.zeros(1), a(decay_max), a(decay_min), a(qss_err), np.array([3.0, 7.0, 5.0]))


def test_lifetimes_with_zero_negative_and_positive_decay():
    ts = _ts([4.0, 0.0, -2.0, np.inf], [0.5, 0.0, -3.0, 2.0], [0, 0, 0, 0])
    assert ts.lifetime_min().tolist() == [0.25, np.inf, np.inf, 0.0]
    assert ts.lifetime_max().tolist() == [2.0, np.inf, np.inf, 0.5]
    assert ts.stiffness() == 7.0
    assert solving.Timescales(np.zeros(0), np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(0)).stiffness() == 0.0
    assert np.array_equal(ts.summary, np.stack([ts.decay_max, ts.decay_min, ts.qss_err]))


def test_qss_candidates_branches():
    #            0: in      1: error   2: produced   3: d == 0   4: Inf     5: slow
    ts = _ts([10.0, 10.0, 10.0, 0.0, 10.0, 10.0], [5.0, 5.0, -1.0, 0.0, 5.0, 0.01], [1e-3, 0.5, 1e-3, 0.0, np.inf, 1e-3])
    assert solving.qss_candidates(ts, 1e-2).tolist() == [0, 5]
    assert solving.qss_candidates(ts, 1.0).tolist() == [0, 1, 5]                       # tol
    assert solving.qss_candidates(ts, 1e-2, max_lifetime=1.0).tolist() == [0]          # 1 / 0.01 = 100 > 1
    assert solving.qss_candidates(ts, 1e-2, max_lifetime=100.0).tolist() == [0, 5]     # <= is inclusive
    scale = np.array([1.0, 100.0, 1.0, 1.0, 1e300, 0.01])
    assert solving.qss_candidates(ts, 1e-2, scale=scale).tolist() == [0, 1]            # 0.5 / 100 in, 1e-3 / 0.01 out, Inf out
    assert solving.qss_candidates(ts, 1e-2).dtype == np.int64
    for bad in (0.0, -1.0):
        sc = np.ones(6); sc[3] = bad
        with pytest.raises(ValueError):
            solving.qss_candidates(ts, 1e-2, scale=sc)
    with pytest.raises(ValueError):
        solving.qss_candidates(ts, 1e-2, scale=np.ones(5))
