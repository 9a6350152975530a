"""CPU tests of the Sobol indices' host side: the symbols, sobol_design, the restatement of sobol_cases.py on the Ishigami
function and against its own replayed order, the edge rules, solve_network_ensemble's argument checks and the SobolIndices
container. No device is touched."""
import ctypes
import os

import numpy as np
import pytest

import sobol_cases as sc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S

NEW_SYMBOLS = ["kin_members_sobol", "kin_members_sobol_dev", "kin_ensemble_sobol"]


def test_symbols_in_binding_header_and_library():
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
    assert os.path.exists(capi.LIB_PATH)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "include", "kinetica_hip.h")
    text = open(header).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(kin_network* h" in text, name
    assert "#define KIN_ABI_VERSION 6" in text and capi.ABI_VERSION == 6


def test_sobol_design_layout():
    M, P = 5, 3
    X = S.sobol_design(M, P, seed=11)
    assert X.shape == (M * (P + 2), P) and X.min() >= 0.0 and X.max() < 1.0
    A, B = X[:M], X[M:2 * M]
    for p in range(P):
        AB = X[(2 + p) * M:(3 + p) * M]
        other = [c for c in range(P) if c != p]
        assert np.array_equal(AB[:, other], A[:, other]) and np.array_equal(AB[:, p], B[:, p])
        assert not np.array_equal(AB[:, p], A[:, p])
    A2, B2 = np.arange(6.0).reshape(3, 2), -np.arange(6.0).reshape(3, 2)
    X2 = S.sobol_design(3, 2, A=A2, B=B2)
    assert np.array_equal(X2[:3], A2) and np.array_equal(X2[3:6], B2)
    assert X2[6:9].tolist() == [[-0.0, 1.0], [-2.0, 3.0], [-4.0, 5.0]] and X2[9:].tolist() == [[0.0, -1.0], [2.0, -3.0], [4.0, -5.0]]
    X1 = S.sobol_design(1, 1, seed=0)
    assert X1.shape == (3, 1) and X1[2, 0] == X1[1, 0]


def test_sobol_design_generator_recipe_bit_for_bit():
    for seed, M, P in ((0, 7, 3), (5, 1, 1), (19, 64, 4)):
        rng = np.random.default_rng(seed)
        A = rng.random((M, P))
        B = rng.random((M, P))
        X = S.sobol_design(M, P, seed=seed)
        assert np.array_equal(X[:M], A) and np.array_equal(X[M:2 * M], B)
    assert np.array_equal(S.sobol_design(4, 2), S.sobol_design(4, 2, seed=0))


@pytest.mark.parametrize("args, kw", [((0, 3), {}), ((4, 0), {}), ((2.5, 3), {}), ((4, 2), dict(A=np.zeros((4, 2)))),
                                      ((4, 2), dict(A=np.zeros((4, 2)), B=np.zeros((4, 3)))),
                                      ((4, 2), dict(A=np.zeros((3, 2)), B=np.zeros((3, 2))))])
def test_sobol_design_value_errors(args, kw):
    with pytest.raises(ValueError):
        S.sobol_design(*args, **kw)


def test_restatement_on_ishigami():
    """M = 4096, P = 3, seeds 0-19 of the design recipe: every S1 and ST within 0.05 of the analytic values."""
    M, P = 4096, 3
    worst1 = worstT = 0.0
    for seed in range(20):
        y = sc.ishigami(S.sobol_design(M, P, seed=seed))
        r = sc.ref_sobol(y[:, None, None], M, P)
        assert r["count"] == M
        worst1 = max(worst1, np.abs(r["first"][0, 0] - sc.ISHIGAMI_S1).max())
        worstT = max(worstT, np.abs(r["total"][0, 0] - sc.ISHIGAMI_ST).max())
    print(f"worst |S1 - analytic| = {worst1:.4f}, worst |ST - analytic| = {worstT:.4f}")
    assert worst1 <= 0.05 and worstT <= 0.05


@pytest.mark.parametrize("M, P, L, N", [(9, 3, 2, 6), (65, 2, 1, 5), (257, 1, 1, 5), (2, 9, 1, 5)])
def test_gates_test_something_and_replay_within_them(M, P, L, N):
    u = sc.block(M, P, L, N)
    ref = sc.ref_sobol(u, M, P)
    fin = sc.finite_columns(u, M, P)
    const = fin[(fin % N) == sc.SP_CONST]
    assert len(fin) >= L * (N - 2) and len(const) == L
    for k in ("first", "total"):
        gate = ref["gate_" + k].reshape(L * N, P)[fin]
        assert gate.max() < 1e-9, (k, gate.max())
        plain = np.setdiff1d(fin, const)
        assert (ref["gate_" + k].reshape(L * N, P)[plain] > 0).all()
    with np.errstate(all="ignore"):
        rel = ref["gate_var"].ravel()[fin] / np.where(ref["var"].ravel()[fin] > 0, ref["var"].ravel()[fin], 1.0)
    assert rel.max() < 1e-9
    rep = sc.replay_sobol(u, M, P, columns=fin)
    for k, width in (("first", P), ("total", P), ("mean", 1), ("var", 1)):
        want, gate = ref[k].reshape(L * N, width)[fin], ref["gate_" + k].reshape(L * N, width)[fin]
        assert sc.within(rep[k].reshape(len(fin), width), want, gate), (k, sc.worst(rep[k].reshape(len(fin), width), want, gate))


def test_edge_rules_of_the_restatement():
    M, P, L, N = 9, 3, 2, 6
    u = sc.block(M, P, L, N)
    ref = sc.ref_sobol(u, M, P)
    # V == 0: exact zeros, and V itself exactly 0.0
    assert np.all(ref["first"][:, sc.SP_CONST] == 0.0) and np.all(ref["total"][:, sc.SP_CONST] == 0.0) and np.all(ref["var"][:, sc.SP_CONST] == 0.0)
    assert np.all(ref["mean"][:, sc.SP_CONST] == u[0, 0, sc.SP_CONST])
    # NaN placement: a NaN in A takes the whole column, a NaN in AB_p only that p
    nan1 = np.zeros((L, N, P), bool); nan1[0, sc.SP_NAN_A] = True; nan1[L - 1, sc.SP_NAN_AB, sc.nan_input(P)] = True
    assert np.array_equal(np.isnan(ref["first"]), nan1) and np.array_equal(np.isnan(ref["total"]), nan1)
    nan0 = np.zeros((L, N), bool); nan0[0, sc.SP_NAN_A] = True
    assert np.array_equal(np.isnan(ref["mean"]), nan0) and np.array_equal(np.isnan(ref["var"]), nan0)
    # n == 0: zeros everywhere; n == 1: S1 = ST = 0.0, mu and V as defined
    r0 = sc.ref_sobol(u, M, P, w=np.zeros(M, int))
    assert r0["count"] == 0 and all(np.all(r0[k] == 0.0) for k in ("first", "total", "mean", "var"))
    w1 = np.zeros(M, int); w1[3] = 1
    r1 = sc.ref_sobol(u, M, P, w=w1)
    assert r1["count"] == 1 and np.all(r1["first"] == 0.0) and np.all(r1["total"] == 0.0)
    a, b = u[3], u[M + 3]
    assert np.allclose(r1["mean"], 0.5 * (a + b), rtol=1e-15, atol=0.0) and np.allclose(r1["var"], 0.25 * (a - b) ** 2, rtol=1e-14, atol=0.0)
    # a 0/1 mask equals the compacted block (restatement and replayed order alike); a multiplicity equals a repeated sample
    keep = np.arange(M) % 3 != 0
    uc, Mc = sc.compacted(u, M, P, keep)
    rm, rc = sc.ref_sobol(u, M, P, w=keep.astype(int)), sc.ref_sobol(uc, Mc, P)
    assert all(sc.same_bits_or_zero(rm[k], rc[k]) for k in ("first", "total", "mean", "var")) and rm["count"] == Mc == 6
    fin = sc.finite_columns(uc, Mc, P)
    pm, pc = sc.replay_sobol(u, M, P, w=keep.astype(int), columns=fin), sc.replay_sobol(uc, Mc, P, columns=fin)
    assert all(np.array_equal(pm[k], pc[k]) for k in pm)
    w3 = np.ones(M, int); w3[4] = 3
    rep = np.ones(M + 2, bool)
    ur = np.concatenate([u.reshape(P + 2, M, L, N), u.reshape(P + 2, M, L, N)[:, [4, 4]]], axis=1).reshape(-1, L, N)
    r3, rr = sc.ref_sobol(u, M, P, w=w3), sc.ref_sobol(ur, M + 2, P)
    assert r3["count"] == rr["count"] == M + 2 and rep.all()
    for k in ("first", "total", "mean", "var"):
        assert sc.within(r3[k], rr[k], rr["gate_" + k]), k


def test_statistics_arguments_with_a_sobol_key():
    kw = S._statistics_arguments(dict(sobol=dict(M=4, P=1)), 12)
    assert kw["sobol"] == dict(M=4, P=1, species=None, w=None, of="states", n_boot=0, seed=0, level=0.95)
    assert kw["quantiles"].tolist() == [0.05, 0.5, 0.95]
    kw = S._statistics_arguments(dict(sobol=dict(M=np.int64(2), P=2, species=[3, 0], w=[1, 2], of="max", n_boot=5, seed=3, level=0.9)), 8)
    sb = kw["sobol"]
    assert sb["M"] == 2 and sb["species"].tolist() == [3, 0] and sb["w"].dtype == np.int32 and sb["w"].tolist() == [1, 2]
    assert (sb["of"], sb["n_boot"], sb["seed"], sb["level"]) == ("max", 5, 3, 0.9)
    assert "sobol" not in S._statistics_arguments(True, 4) and "sobol" not in S._statistics_arguments(dict(sobol=None), 4)


@pytest.mark.parametrize("sobol", [
    7, dict(P=1), dict(M=4), dict(M=0, P=1), dict(M=4, P=0), dict(M=4.0, P=1), dict(M=True, P=1), dict(M=4, P=2),
    dict(M=4, P=1, colour=1), dict(M=4, P=1, species=[-1]), dict(M=4, P=1, species=[0.5]), dict(M=4, P=1, w=[1, 1, 1]),
    dict(M=4, P=1, w=[1, -1, 1, 1]), dict(M=4, P=1, w=[1.0, 1.0, 1.0, 1.0]), dict(M=4, P=1, of="min"), dict(M=4, P=1, n_boot=-1),
    dict(M=4, P=1, n_boot=1.5), dict(M=4, P=1, level=1.0), dict(M=4, P=1, level="x")])
def test_statistics_arguments_malformed_sobol(sobol):
    with pytest.raises(ValueError):
        S._statistics_arguments(dict(sobol=sobol), 12)


def test_solve_network_ensemble_rejects_a_design_that_does_not_match_before_the_device():
    with pytest.raises(ValueError, match="members"):
        S.solve_network_ensemble([object()] * 5, None, None, statistics=dict(sobol=dict(M=2, P=1)))


def test_sobol_indices_container_and_ranking():
    total = np.array([[[0.1, 0.7, 0.2], [0.5, 0.0, 0.5]],
                      [[0.3, 0.3, 0.9], [np.nan, 0.2, 0.1]]])
    si = S.SobolIndices(t=np.array([0.0, 1.0]), count=8, first=total * 0.5, total=total, mean=np.zeros((2, 2)), var=np.ones((2, 2)),
                        species=np.array([7, 2]))
    assert si.first_ci is None and si.total_ci is None
    assert si.ranking().tolist() == [2, 0, 1]                    # last row, mean over the species with a value: (0.3, 0.25, 0.5)
    assert si.ranking(row=0).tolist() == [1, 2, 0]               # (0.3, 0.35, 0.35): the tie keeps the inputs' order
    assert si.ranking(row=0, species=7).tolist() == [1, 2, 0]
    assert si.ranking(row=0, species=2).tolist() == [0, 2, 1]
    assert si.ranking(row=1, species=2).tolist() == [1, 2, 0]    # NaN last
    with pytest.raises(ValueError):
        si.ranking(species=3)
    si.species = None
    assert si.ranking(row=0, species=1).tolist() == [0, 2, 1]    # without a selection the id is the position
    assert S.EnsembleStatistics(np.zeros(1), 0, *[np.zeros((1, 1))] * 4).sobol is None
