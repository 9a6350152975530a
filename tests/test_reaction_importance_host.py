"""CPU tests of reaction elimination: the per-reaction table (kin_reaction_importance_plan_host) against records() of
drg_cases.py, reaction_select, the reaction step of reduce_network (graph and importance supplied: no device is touched), and
the NumPy reference of reaction_importance_cases.py on the hand values."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import drg_cases as dc
import reaction_importance_cases as rc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S
from kinetica_jl_amd.synth import from_lists


def _networks():
    nets = {name: v[0] for name, v in dc.hand_networks().items()}
    nets["hub"] = dc.hub_network(300, 20)
    net, Ea, A = dc.synth(300, 1500)
    nets["300x1500"] = net
    nets["300x1500_cut"] = dc.post_cutoff(net, Ea, A)[0]
    return nets


NETS = _networks()


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(NETS))
def test_plan_host_equals_records(name, pairing):
    net = NETS[name]
    ref = rc.RiRef(net, pairing)
    partner, species, nu, info = capi.reaction_importance_plan_host(net, pairing)
    assert partner.shape == (net.n_reactions,) and species.shape == nu.shape == (net.n_reactions, 4)
    assert np.array_equal(partner, ref.partner)
    assert info == ref.info()
    if not pairing:
        assert np.all(partner == -1) and info["records"] == net.n_reactions and info["paired_reactions"] == 0
    for r in range(net.n_reactions):
        got = {int(s): int(c) for s, c in zip(species[r], nu[r]) if s >= 0}
        assert got == ref.slots[r], r
        assert np.all(nu[r][species[r] < 0] == 0) and np.all(nu[r][species[r] >= 0] != 0)
        if partner[r] >= 0:       # the reverse member: the same species in the same slots, every sign flipped
            assert partner[partner[r]] == r
            assert np.array_equal(species[partner[r]], species[r]) and np.array_equal(nu[partner[r]], -nu[r])


def test_plan_host_of_odd_reaction_count_and_lost_reverses():
    net = NETS["300x1500_cut"]
    assert net.n_reactions % 2 == 1
    partner = capi.reaction_importance_plan_host(net, 1)[0]
    assert np.any(partner < 0) and np.any(partner >= 0)


def test_plan_host_takes_either_index_base():
    """The same network handed over 1-based gives the same 0-based table."""
    net = NETS["300x1500_cut"]
    L = capi.lib()
    for pairing in (1, 0):
        want = capi.reaction_importance_plan_host(net, pairing)
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (net.reac_ptr, net.reac_idx + 1, net.reac_sto, net.prod_ptr,
                                                                  net.prod_idx + 1, net.prod_sto)]
        R = net.n_reactions
        info, partner, species, nu = np.zeros(3, np.int64), np.empty(R, np.int64), np.empty((R, 4), np.int64), np.empty((R, 4), np.int64)
        st = L.kin_reaction_importance_plan_host(net.n_species, R, *[capi._p64(a) for a in arrs], 1, pairing, capi._p64(info),
                                                 capi._p64(partner), capi._p64(species), capi._p64(nu))
        assert st == capi.KIN_OK
        assert np.array_equal(partner, want[0]) and np.array_equal(species, want[1]) and np.array_equal(nu, want[2])
        assert info.tolist() == list(want[3].values())
        # sizes only
        info2 = np.zeros(3, np.int64)
        assert L.kin_reaction_importance_plan_host(net.n_species, R, *[capi._p64(a) for a in arrs], 1, pairing, capi._p64(info2),
                                                   None, None, None) == capi.KIN_OK
        assert np.array_equal(info2, info)


def test_plan_host_rejects_a_bad_network():
    with pytest.raises(capi.KineticaHipError) as e:
        capi.reaction_importance_plan_host(SimpleNamespace(n_species=3, n_reactions=1, reac_ptr=[0, 1], reac_idx=[7], reac_sto=[1],
                                                           prod_ptr=[0, 1], prod_idx=[1], prod_sto=[1]), 1)
    assert e.value.code == capi.KIN_ERR_INVALID_ARG


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(rc.HAND))
def test_reference_on_the_hand_values(name, pairing):
    from oracle import oracle as orc
    net, k, U, _ = dc.hand_networks()[name]
    on = orc.OracleNetwork.from_flat(net)
    rates = np.stack([on.rates(k, u) for u in U])
    ref = rc.RiRef(net, pairing)
    for selected, want in rc.HAND[name]:
        imp, bound, I, _ = ref.importance(rates, selected=selected)
        assert imp.tolist() == want[pairing]
        assert I[-1].tolist() == [0.0] * net.n_reactions          # the all-zero last state
        if name == "A_eq_B_balanced" and pairing:
            assert np.all(np.isinf(bound))           # den = 0 by cancellation of non-zero rates: the bound says so
        else:
            assert np.all(bound < 1e-14)


def test_reference_bound_is_meaningful_on_the_synthetic_case():
    """The condition under test_gpu_reaction_importance.py's bound: at most 1 % of the (reaction, state) entries above 1e-9."""
    for pairing in (1, 0):
        _, _, I, bounds = rc.ref_of("300x1500", pairing).importance(rc.case_rates("300x1500", "per_state", 7))
        frac = float(np.mean(bounds > 1e-9))
        print(f"pairing={pairing}: {100 * frac:.3f} % of the entries above 1e-9, median {np.median(bounds):.2e}")
        assert frac <= 0.01
        assert np.all(I >= 0.0) and np.all(I <= 1.0 + 1e-15)


def test_reaction_select_threshold_and_candidates():
    imp = np.array([0.5, 0.02, 0.0199, 1.0, 0.0, 0.02])
    assert S.reaction_select(imp, 0.02).tolist() == [0, 1, 3, 5]                   # >= keeps the threshold itself
    assert S.reaction_select(imp, np.nextafter(0.02, 1.0)).tolist() == [0, 3]
    assert S.reaction_select(imp, 0.0).tolist() == [0, 1, 2, 3, 4, 5]
    assert S.reaction_select(imp, 2.0).tolist() == []
    assert S.reaction_select(imp, 0.02, candidates=[5, 2, 3, 3]).tolist() == [3, 5]    # unsorted, duplicates
    assert S.reaction_select(imp, 0.02, candidates=[]).tolist() == []
    assert S.reaction_select(imp, 0.02).dtype == np.int64
    with pytest.raises(ValueError):
        S.reaction_select(imp, 0.02, candidates=[6])


def _small_case():
    # species a..e (ids 1..5); reactions: a -> b, b -> c, c + d -> e, a + e -> b, b -> a, a -> c
    sd = S.SpeciesData.from_names(["a", "b", "c", "d", "e"], n_atoms=[1, 2, 3, 4, 5])
    rd = S.RxData(6, [[1], [2], [3, 4], [1, 5], [2], [1]], [[2], [3], [5], [2], [1], [3]], [[1], [1], [1, 1], [1, 1], [1], [1]],
                  [[1], [1], [1], [1], [1], [1]], dH=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    calc = S.PrecalculatedArrheniusCalculator(Ea=[10.0, 20.0, 30.0, 40.0, 50.0, 60.0], A=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    u = np.zeros((2, 5)); u[0, 0] = 1.0; u[1] = 0.2
    out = SimpleNamespace(sd=sd, rd=rd, sol=SimpleNamespace(t=np.array([0.0, 1.0]), u=u))
    net = from_lists(5, *[[[(i - 1, c) for i, c in zip(ids[r], st[r])] for r in range(6)]
                          for ids, st in ((rd.id_reacs, rd.stoic_reacs), (rd.id_prods, rd.stoic_prods))])
    rowptr, colidx, _ = capi.drg_pattern_host(net, 1)
    coef = np.zeros(len(colidx))
    edge = lambda a, b: rowptr[a] + list(colidx[rowptr[a]:rowptr[a + 1]]).index(b)
    coef[edge(2, 1)] = 0.75       # c -> b
    coef[edge(1, 0)] = 0.5        # b -> a
    return sd, rd, calc, out, (rowptr, colidx, coef)


def test_reduce_network_combines_the_species_rule_and_the_threshold():
    sd, rd, calc, out, graph = _small_case()
    base = S.reduce_network(out, calc, ["c"], 0.5, coef=graph)
    assert base.species_kept.tolist() == [0, 1, 2] and base.reactions_kept.tolist() == [0, 1, 4, 5]
    assert base.reaction_eps is None and base.reaction_importance is None
    # reaction 2 is important but touches dropped species; reaction 4 passes the species rule but not the threshold;
    # reaction 1 sits exactly on the threshold and stays
    imp = np.array([0.9, 0.25, 1.0, 1.0, 0.1, 0.3])
    red = S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=0.25, reaction_importance=imp)
    assert red.species_kept.tolist() == [0, 1, 2] and red.reactions_kept.tolist() == [0, 1, 5]
    assert red.reactions_kept.dtype == np.int64
    assert red.reaction_eps == 0.25 and np.array_equal(red.reaction_importance, imp)
    assert red.sd.n == 3 and red.sd.toInt == {"a": 1, "b": 2, "c": 3}
    assert red.rd.nr == 3 and red.rd.id_reacs == [[1], [2], [1]] and red.rd.id_prods == [[2], [3], [3]] and red.rd.dH == [1.0, 2.0, 6.0]
    assert red.calculator.Ea.tolist() == [10.0, 20.0, 60.0] and red.calculator.A.tolist() == [1.0, 2.0, 6.0]
    S.setup_network(red.sd, red.rd, red.calculator)
    assert len(calc.Ea) == 6 and rd.nr == 6 and sd.n == 5       # the inputs are left alone
    # no species leaves in this step: b loses every reaction and stays as an inert entry, u0 maps as before
    lone = S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=0.5, reaction_importance=np.array([0.0, 0.0, 1.0, 1.0, 0.0, 0.5]))
    assert lone.species_kept.tolist() == [0, 1, 2] and lone.reactions_kept.tolist() == [5] and lone.sd.n == 3
    assert lone.rd.id_reacs == [[1]] and lone.rd.id_prods == [[3]] and lone.calculator.Ea.tolist() == [60.0]
    assert lone.map_u0({"a": 1.0, "b": 0.5}) == {"a": 1.0, "b": 0.5}
    # every reaction below the threshold: an empty rd, a spliced-empty calculator
    none = S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=2.0, reaction_importance=imp)
    assert none.reactions_kept.tolist() == [] and none.rd.nr == 0 and len(none.calculator.Ea) == 0 and none.sd.n == 3
    # the same step behind the DRGEP selection
    ep = S.reduce_network(out, calc, ["c"], 0.5, method="drgep", importance=np.array([1.0, 0.6, 1.0, 0.1, 0.2]), reaction_eps=0.25,
                          reaction_importance=imp)
    assert ep.species_kept.tolist() == [0, 1, 2] and ep.reactions_kept.tolist() == [0, 1, 5]


def test_reduce_network_without_reaction_eps_is_unchanged():
    sd, rd, calc, out, graph = _small_case()
    a = S.reduce_network(out, calc, ["c"], 0.5, coef=graph)
    b = S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=None, reaction_importance=np.zeros(6))    # ignored without eps
    c = S.reduce_network(out, calc, ["c"], 0.5, True, graph, "drg", None)                 # the positional form of before
    for x in (b, c):
        for f in dataclasses.fields(S.DRGReduction):
            va, vx = getattr(a, f.name), getattr(x, f.name)
            if isinstance(va, np.ndarray):
                assert np.array_equal(va, vx) and va.dtype == vx.dtype, f.name
            elif f.name == "calculator":
                assert va.Ea.tolist() == vx.Ea.tolist() and va.A.tolist() == vx.A.tolist()
            else:
                assert va == vx, f.name
        assert x.reaction_eps is None and x.reaction_importance is None
    # the two results of reaction elimination are attributes with defaults behind the dataclass fields, which stay as they were
    names = [f.name for f in dataclasses.fields(S.DRGReduction)]
    assert names[-1] == "importance" and "reaction_eps" not in names and "reaction_importance" not in names
    assert S.DRGReduction.reaction_eps is None and S.DRGReduction.reaction_importance is None
    assert a.reactions_kept.tolist() == [0, 1, 4, 5] and a.reactions_kept.dtype == np.int64


def test_reduce_network_rejects_a_vector_of_the_wrong_length():
    sd, rd, calc, out, graph = _small_case()
    with pytest.raises(ValueError):
        S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=0.1, reaction_importance=np.ones(5))
    with pytest.raises(ValueError):
        S.reduce_network(out, calc, ["c"], 0.5, coef=graph, reaction_eps=0.1, reaction_importance=np.ones((6, 1)))
