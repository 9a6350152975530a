"""CPU tests of the directed-relation-graph reduction: the host pattern (kin_drg_pattern_host) against the NumPy reference of
drg_cases.py, the selection and the renumbering of reduce_network, and the condition the GPU tests' bound rests on."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import drg_cases as dc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import from_lists

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _networks():
    d = json.load(open(os.path.join(GOLDEN, "doc_crn.json")))
    nets = {"doc_crn": from_lists(5, d["reacs"], d["prods"]), "hub": dc.hub_network()}
    nets.update({name: v[0] for name, v in dc.hand_networks().items()})
    net, Ea, A = dc.synth(300, 1500)
    nets["300x1500"] = net
    nets["300x1500_cut"] = dc.post_cutoff(net, Ea, A)[0]
    return nets


NETS = _networks()


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(NETS))
def test_pattern_host_equals_numpy(name, pairing):
    net = NETS[name]
    ref = dc.DrgRef(net, pairing)
    rowptr, colidx, info = capi.drg_pattern_host(net, pairing)
    assert np.array_equal(rowptr, ref.rowptr) and np.array_equal(colidx, ref.colidx)
    assert info == ref.info()
    # sorted columns, no diagonal
    for a in range(net.n_species):
        cols = colidx[rowptr[a]:rowptr[a + 1]]
        assert np.all(np.diff(cols) > 0) and a not in cols


def test_pattern_of_the_collider_and_of_pairing():
    net = dc.hand_networks()["A_M_to_B_M"][0]
    rowptr, colidx, info = capi.drg_pattern_host(net, 1)
    assert rowptr.tolist() == [0, 2, 4, 4] and colidx.tolist() == [1, 2, 0, 2]      # M heads A -> M, B -> M and is the tail of none
    assert info["den_contributions"] == 2 and info["edge_contributions"] == 4
    # pairing halves the contributions of a reversible pair and leaves the edges alone
    net = dc.hand_networks()["A_eq_B_balanced"][0]
    i1, i0 = capi.drg_pattern_host(net, 1)[2], capi.drg_pattern_host(net, 0)[2]
    assert i1["edges"] == i0["edges"] == 2 and i1["edge_contributions"] == 2 and i0["edge_contributions"] == 4


def test_case_list_covers_every_row_class():
    seen = {k: 0 for k in capi.DRG_INFO[3:]}
    for name in ("hub", "300x1500", "300x1500_cut"):
        for pairing in (0, 1):
            info = capi.drg_pattern_host(NETS[name], pairing)[2]
            for k in seen:
                seen[k] += info[k]
    assert all(v > 0 for v in seen.values()), seen


def test_select_threshold_unreachable_and_cycles():
    # 0 -> 1 (0.5), 1 -> 2 (0.25), 2 -> 0 (1.0: a cycle), 3 -> 0 (1.0: 3 reaches the others, nothing reaches 3), 1 -> 4 (0.125)
    rowptr = np.array([0, 1, 3, 4, 5, 5])
    colidx = np.array([1, 2, 4, 0, 0])
    coef = np.array([0.5, 0.25, 0.125, 1.0, 1.0])
    assert S.drg_select(rowptr, colidx, coef, [0], 0.25).tolist() == [0, 1, 2]        # 0.25 >= 0.25 keeps 1 -> 2; 3 and 4 dropped
    assert S.drg_select(rowptr, colidx, coef, [0], np.nextafter(0.25, 1.0)).tolist() == [0, 1]
    assert S.drg_select(rowptr, colidx, coef, [0], 0.125).tolist() == [0, 1, 2, 4]
    assert S.drg_select(rowptr, colidx, coef, [3], 0.5).tolist() == [0, 1, 3]
    assert S.drg_select(rowptr, colidx, coef, [2, 4], 2.0).tolist() == [2, 4]          # no edge survives: the targets alone
    assert S.drg_select(rowptr, colidx, coef, [], 0.0).tolist() == []
    for tg, eps in (([0], 0.25), ([3], 0.5), ([1], 0.0)):
        assert S.drg_select(rowptr, colidx, coef, tg, eps).tolist() == dc.select(rowptr, colidx, coef, tg, eps).tolist()
    with pytest.raises(ValueError):
        S.drg_select(rowptr, colidx, coef, [5], 0.1)


def test_reduce_network_renumbers_species_reactions_calculator_and_u0():
    # species a..e (ids 1..5); reactions: a -> b, b -> c, c + d -> e, a + e -> b, b -> a
    names = ["a", "b", "c", "d", "e"]
    sd = S.SpeciesData.from_names(names, n_atoms=[1, 2, 3, 4, 5])
    rd = S.RxData(5, [[1], [2], [3, 4], [1, 5], [2]], [[2], [3], [5], [2], [1]], [[1], [1], [1, 1], [1, 1], [1]],
                  [[1], [1], [1], [1], [1]], dH=[1.0, 2.0, 3.0, 4.0, 5.0])
    calc = S.PrecalculatedArrheniusCalculator(Ea=[10.0, 20.0, 30.0, 40.0, 50.0], A=[1.0, 2.0, 3.0, 4.0, 5.0])
    u = np.zeros((2, 5)); u[0, 0] = 1.0; u[1] = 0.2
    out = SimpleNamespace(sd=sd, rd=rd, sol=SimpleNamespace(t=np.array([0.0, 1.0]), u=u))
    rowptr, colidx, _ = capi.drg_pattern_host(from_lists(5, *[[[(i - 1, c) for i, c in zip(ids[r], st[r])] for r in range(5)]
                                                              for ids, st in ((rd.id_reacs, rd.stoic_reacs), (rd.id_prods, rd.stoic_prods))]), 1)
    coef = np.zeros(len(colidx))
    edge = lambda a, b: rowptr[a] + list(colidx[rowptr[a]:rowptr[a + 1]]).index(b)
    coef[edge(2, 1)] = 0.75       # c -> b
    coef[edge(1, 0)] = 0.5        # b -> a
    coef[edge(2, 3)] = 0.1        # c -> d: below the threshold
    red = S.reduce_network(out, calc, ["c"], 0.5, coef=(rowptr, colidx, coef))
    assert red.targets.tolist() == [0, 2]                       # a is non-zero in the first saved state
    assert red.species_kept.tolist() == [0, 1, 2]
    assert red.reactions_kept.tolist() == [0, 1, 4]             # c + d -> e and a + e -> b touch dropped species
    assert red.sd.n == 3 and red.sd.toInt == {"a": 1, "b": 2, "c": 3} and red.sd.toStr == {1: "a", 2: "b", 3: "c"}
    assert red.sd.xyz == {1: {"N_atoms": 1}, 2: {"N_atoms": 2}, 3: {"N_atoms": 3}}
    assert red.rd.nr == 3 and red.rd.id_reacs == [[1], [2], [2]] and red.rd.id_prods == [[2], [3], [1]]
    assert red.rd.stoic_reacs == [[1], [1], [1]] and red.rd.dH == [1.0, 2.0, 5.0]
    assert red.calculator.Ea.tolist() == [10.0, 20.0, 50.0] and red.calculator.A.tolist() == [1.0, 2.0, 5.0]
    assert len(calc.Ea) == 5 and rd.nr == 5 and sd.n == 5       # the inputs are left alone
    S.setup_network(red.sd, red.rd, red.calculator)
    assert red.map_u0({"a": 1.0, "c": 0.5, "e": 0.0}) == {"a": 1.0, "c": 0.5}
    assert red.map_u0([1.0, 0.0, 0.5, 0.0, 0.0]).tolist() == [1.0, 0.0, 0.5]
    assert red.map_u0([1.0]).tolist() == [1.0, 0.0, 0.0]        # a short u0 stays a prefix
    with pytest.raises(ValueError):
        red.map_u0({"d": 0.1})
    with pytest.raises(ValueError):
        red.map_u0([0.0, 0.0, 0.0, 0.1, 0.0])
    # a dropped species in the middle: ids close up
    red2 = S.reduce_network(out, calc, ["e"], 2.0, coef=(rowptr, colidx, coef))
    assert red2.species_kept.tolist() == [0, 4] and red2.sd.toInt == {"a": 1, "e": 2} and red2.rd.nr == 0
    assert len(red2.calculator.Ea) == 0


def test_species_subset_operations():
    sd = S.SpeciesData.from_names(["a", "b", "c"])
    sub, new_id = sd.subset([3, 1])
    assert new_id == {1: 1, 3: 2} and sub.toInt == {"a": 1, "c": 2} and sub.n == 2 and sub.xyz is None
    with pytest.raises(ValueError):
        sd.subset([4])
    rd = S.RxData(2, [[1, 3], [2]], [[3], [1]], [[1, 1], [2]], [[2], [1]])
    sub_rd, kept = rd.subset_species(new_id)
    assert kept == [0] and sub_rd.id_reacs == [[1, 2]] and sub_rd.id_prods == [[2]] and sub_rd.stoic_prods == [[2]] and sub_rd.dH is None
    assert rd.id_reacs == [[1, 3], [2]]


@pytest.mark.parametrize("name,mode,B", [("300x1500", "per_state", dc.BMAX), ("300x1500", "T", 7), ("300x1500_cut", "per_state", 7),
                                         ("300x1500_cut", "T_kmax", 7), ("1000x5000", "per_state", 7)])
def test_states_keep_the_derived_bound_meaningful(name, mode, B):
    """The condition under test_gpu_drg.py's bound: at most 1 % of the (edge, state) entries have a bound above 1e-9."""
    case = dc.synth_case(name)
    for pairing in (1, 0):
        _, _, bounds = case.ref(mode, pairing, B)
        frac = float(np.mean(bounds > 1e-9))
        print(f"{name} {mode} pairing={pairing} B={B}: {100 * frac:.3f} % of the entries above 1e-9, median {np.median(bounds):.2e}")
        assert frac <= 0.01
