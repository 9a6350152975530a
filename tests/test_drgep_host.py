"""CPU tests of DRG with error propagation: the NumPy reference of drgep_cases.py on networks worked by hand, the conditions
the GPU tests' bound rests on, the selection, reduce_network(method="drgep") and the binding's symbol list."""
from types import SimpleNamespace

import numpy as np
import pytest

import drg_cases as dc
import drgep_cases as ec
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S

NEW_SYMBOLS = ["kin_drgep_batched", "kin_drgep_batched_dev", "kin_drgep_paths", "kin_solution_drgep", "kin_ensemble_drgep"]


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(ec.hand_networks()))
def test_reference_on_hand_networks(name, pairing):
    from oracle import oracle as orc
    net, k, U, targets, want = ec.hand_networks()[name]
    g = ec.DrgepRef(net, pairing)
    on = orc.OracleNetwork.from_flat(net)
    r, bound = g.coefficients(np.stack([on.rates(k, u) for u in U]))
    imp, R, rounds = g.importance(r, targets)
    assert imp.tolist() == want[pairing]                          # dyadic inputs: exact
    zero = [1.0 if i in targets else 0.0 for i in range(net.n_species)]
    assert R[-1].tolist() == zero and np.all(r[-1] == 0.0)        # the all-zero state: the targets alone
    assert np.all(rounds <= net.n_species)


def test_binding_lists_the_new_symbols_and_the_library_exports_them():
    assert all(s in capi.SYMBOLS for s in NEW_SYMBOLS)
    assert all(hasattr(capi.lib(), s) for s in NEW_SYMBOLS)
    assert all(hasattr(capi.HipNetwork, m) for m in ("drgep_batched", "drgep_batched_dev", "drgep_paths", "solution_drgep", "ensemble_drgep"))


def test_case_list_reaches_every_in_degree_class():
    """The path kernel takes a species by a lane, a wavefront or the workgroup according to its in-degree: the networks of
    test_gpu_drgep.py reach all three."""
    short, wave = capi.DRGEP_IN_SHORT_MAX, capi.DRGEP_IN_WAVE_MAX
    nets = {"collider300": ec.collider_network(300), "collider20": ec.collider_network(20)}
    nets.update({n: dc.synth_case(n).net for n in ("300x1500", "300x1500_cut", "1000x5000")})
    cls = {}
    for name, net in nets.items():
        for pairing in (0, 1):
            _, colidx, _ = capi.drg_pattern_host(net, pairing)
            cls[(name, pairing)] = ec.in_degree_classes(colidx, net.n_species, short, wave)
    assert cls[("collider300", 1)] == [601, 0, 1] and cls[("collider20", 1)] == [41, 1, 0]     # M: 601 and 41 incoming edges
    assert all(sum(c[i] for c in cls.values()) > 0 for i in range(3)), cls
    assert any(c[0] > 0 and c[1] > 0 for c in cls.values())           # a network that mixes lanes and wavefronts


@pytest.mark.parametrize("name,mode", ec.GPU_CASES)
def test_states_keep_the_derived_bound_meaningful(name, mode):
    """The conditions under test_gpu_drgep.py's checks: at most 1 % of the (edge, state) bounds of r are above 1e-9, and at
    most 1 % of the species have an importance interval (the searches on r + bound and r - bound) wider than 1e-9."""
    for pairing in (1, 0):
        g = ec.graph(name, pairing)
        r, bounds = ec.ref(name, mode, pairing)
        frac = float(np.mean(bounds > 1e-9))
        b = np.where(np.isfinite(bounds), bounds, 1.0)
        lo = g.importance(np.clip(r - b, 0.0, 1.0), ec.TARGETS)[0]
        hi = g.importance(np.clip(r + b, 0.0, 1.0), ec.TARGETS)[0]
        mid, _, rounds = g.importance(r, ec.TARGETS)
        wide = float(np.mean(hi - lo > 1e-9))
        print(f"{name} {mode} pairing={pairing}: {100 * frac:.3f} % of the bounds above 1e-9, {100 * wide:.3f} % of the species wider than "
              f"1e-9, rounds {rounds.min()}..{rounds.max()}, median importance {np.median(mid):.2e}")
        assert frac <= 0.01 and wide <= 0.01
        assert np.all(lo <= mid) and np.all(mid <= hi)
        assert np.all(mid[ec.TARGETS] == 1.0) and np.all((mid >= 0.0) & (mid <= 1.0))


def test_select_threshold_and_targets():
    imp = np.array([1.0, 0.25, 0.0, 0.125, 0.5])
    assert S.drgep_select(imp, [0], 0.25).tolist() == [0, 1, 4]                       # 0.25 >= 0.25 is kept
    assert S.drgep_select(imp, [0], np.nextafter(0.25, 1.0)).tolist() == [0, 4]
    assert S.drgep_select(imp, [2, 0], 0.5).tolist() == [0, 2, 4]                     # a target below the threshold stays
    assert S.drgep_select(imp, [3], 2.0).tolist() == [3]                              # nothing reaches eps: the targets alone
    assert S.drgep_select(imp, [], 0.0).tolist() == [0, 1, 2, 3, 4]
    assert S.drgep_select(imp, [], 2.0).tolist() == []
    with pytest.raises(ValueError):
        S.drgep_select(imp, [5], 0.1)
    assert imp.tolist() == [1.0, 0.25, 0.0, 0.125, 0.5]                               # the argument is left alone


def _fixture():
    # species a..e (ids 1..5); reactions: a -> b, b -> c, c + d -> e, a + e -> b, b -> a (the fixture of test_drg_host.py)
    sd = S.SpeciesData.from_names(["a", "b", "c", "d", "e"], n_atoms=[1, 2, 3, 4, 5])
    rd = S.RxData(5, [[1], [2], [3, 4], [1, 5], [2]], [[2], [3], [5], [2], [1]], [[1], [1], [1, 1], [1, 1], [1]],
                  [[1], [1], [1], [1], [1]], dH=[1.0, 2.0, 3.0, 4.0, 5.0])
    calc = S.PrecalculatedArrheniusCalculator(Ea=[10.0, 20.0, 30.0, 40.0, 50.0], A=[1.0, 2.0, 3.0, 4.0, 5.0])
    u = np.zeros((2, 5)); u[0, 0] = 1.0; u[1] = 0.2
    return sd, rd, calc, SimpleNamespace(sd=sd, rd=rd, sol=SimpleNamespace(t=np.array([0.0, 1.0]), u=u))


def test_reduce_network_drgep_with_a_given_importance():
    sd, rd, calc, out = _fixture()
    imp = np.array([0.5, 0.75, 1.0, 0.1, 0.0])
    red = S.reduce_network(out, calc, ["c"], 0.5, method="drgep", importance=imp)
    assert red.targets.tolist() == [0, 2]                       # a is non-zero in the first saved state
    assert red.species_kept.tolist() == [0, 1, 2]
    assert red.reactions_kept.tolist() == [0, 1, 4]             # c + d -> e and a + e -> b touch dropped species
    assert red.sd.toInt == {"a": 1, "b": 2, "c": 3} and red.rd.nr == 3 and red.rd.id_prods == [[2], [3], [1]]
    assert red.calculator.Ea.tolist() == [10.0, 20.0, 50.0] and len(calc.Ea) == 5
    assert red.importance.tolist() == imp.tolist() and red.eps == 0.5 and len(red.coef) == 0
    # a is kept as a target although its importance is below eps
    red2 = S.reduce_network(out, calc, ["c"], 0.9, method="drgep", importance=imp)
    assert red2.species_kept.tolist() == [0, 2] and red2.rd.nr == 0
    with pytest.raises(ValueError):
        S.reduce_network(out, calc, ["c"], 0.5, method="drgep", importance=imp[:4])
    with pytest.raises(ValueError):
        S.reduce_network(out, calc, ["c"], 0.5, method="lu")


def test_reduce_network_drg_is_unchanged():
    """method="drg", the default: the result of test_drg_host.py's fixture field by field, and no importance."""
    from kinetica_jl_amd.synth import from_lists
    sd, rd, calc, out = _fixture()
    rowptr, colidx, _ = capi.drg_pattern_host(from_lists(5, *[[[(i - 1, c) for i, c in zip(ids[r], st[r])] for r in range(5)]
                                                              for ids, st in ((rd.id_reacs, rd.stoic_reacs), (rd.id_prods, rd.stoic_prods))]), 1)
    coef = np.zeros(len(colidx))
    edge = lambda a, b: rowptr[a] + list(colidx[rowptr[a]:rowptr[a + 1]]).index(b)
    coef[edge(2, 1)] = 0.75
    coef[edge(1, 0)] = 0.5
    coef[edge(2, 3)] = 0.1
    for kw in ({}, {"method": "drg"}):
        red = S.reduce_network(out, calc, ["c"], 0.5, coef=(rowptr, colidx, coef), **kw)
        assert red.targets.tolist() == [0, 2] and red.species_kept.tolist() == [0, 1, 2] and red.reactions_kept.tolist() == [0, 1, 4]
        assert np.array_equal(red.rowptr, rowptr) and np.array_equal(red.colidx, colidx) and np.array_equal(red.coef, coef)
        assert red.eps == 0.5 and red.importance is None
        assert red.calculator.Ea.tolist() == [10.0, 20.0, 50.0]
    import dataclasses
    assert [f.name for f in dataclasses.fields(S.DRGReduction)][-1] == "importance"
