"""CPU tests of path flux analysis: the reference of pfa_cases.py on its hand networks, the host pattern
(kin_pfa_pattern_host) against it, reduce_network(method="pfa") on coefficients the reference supplies, the condition the
GPU test's bound of the split stage rests on, and the binding's symbol list."""
from types import SimpleNamespace

import numpy as np
import pytest

import drg_cases as dc
import drgep_cases as ec
import pfa_cases as pc
from kinetica_jl_amd import capi
from kinetica_jl_amd import solving as S

NEW_SYMBOLS = ["kin_pfa_pattern_host", "kin_pfa_pattern", "kin_pfa_batched", "kin_pfa_batched_dev", "kin_pfa_paths", "kin_solution_pfa",
               "kin_ensemble_pfa"]


def _networks():
    nets = {name: v[0] for name, v in pc.hand_networks().items()}
    nets["side_branch"] = pc.side_branch_network()
    nets["hub"] = dc.hub_network()
    for name in ("300x1500", "300x1500_cut", "1000x5000"):
        nets[name] = dc.synth_case(name).net
    return nets


NETS = _networks()


def _pairs(g, r):
    return {(int(a), int(b)): float(v) for a, b, v in zip(g.rows2, g.cols2, r)}


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(pc.hand_networks()))
def test_reference_on_hand_networks(name, pairing):
    from oracle import oracle as orc
    net, k, U, want = pc.hand_networks()[name]
    on = orc.OracleNetwork.from_flat(net)
    g = pc.PfaRef(net, pairing)
    coef, r = g.coefficients(np.stack([on.rates(k, u) for u in U]))
    assert _pairs(g, r[0]) == want[pairing] and _pairs(g, coef) == want[pairing]       # dyadic inputs: exact
    assert np.all(r[-1] == 0.0)                                                      # the all-zero state
    assert not any(a == b for a, b in want[pairing])


def test_chain_pair_is_no_drg_edge():
    net = pc.hand_networks()["chain"][0]
    for pairing in (0, 1):
        rowptr, colidx = capi.drg_pattern_host(net, pairing)[:2]
        assert 2 not in colidx[rowptr[0]:rowptr[1]] and 0 not in colidx[rowptr[2]:rowptr[3]]
        rowptr2, colidx2, info = capi.pfa_pattern_host(net, pairing)
        assert colidx2[rowptr2[0]:rowptr2[1]].tolist() == [1, 2] and colidx2[rowptr2[2]:rowptr2[3]].tolist() == [0, 1]
        assert info == dict(edges=4, pairs=6, products=6, max_row=2)


@pytest.mark.parametrize("pairing", [1, 0])
@pytest.mark.parametrize("name", sorted(NETS))
def test_pattern_host_equals_numpy(name, pairing):
    net = NETS[name]
    g = pc.PfaRef(net, pairing)
    rowptr, colidx, info = capi.pfa_pattern_host(net, pairing)
    assert np.array_equal(rowptr, g.rowptr2) and np.array_equal(colidx, g.colidx2)
    assert info == g.info()
    print(f"{name} pairing={pairing}: {info}")
    # sorted columns, no diagonal, E inside E2
    for a in range(net.n_species):
        cols = colidx[rowptr[a]:rowptr[a + 1]]
        assert np.all(np.diff(cols) > 0) and a not in cols
        assert np.all(np.isin(g.cols[g.rowptr[a]:g.rowptr[a + 1]], cols))


def test_sizes_of_the_synthetic_networks():
    """The figures the second-generation kernel was designed for (pairing on)."""
    i300, i1000 = (capi.pfa_pattern_host(NETS[n], 1)[2] for n in ("300x1500", "1000x5000"))
    assert (i300["edges"], i300["pairs"], i300["max_row"]) == (3704, 57792, 169)
    assert (i1000["edges"], i1000["pairs"], i1000["max_row"]) == (12398, 489132, 484)
    assert i1000["max_row"] > 256                                                    # rows with more than 256 out-edges
    assert 0.1e6 < i300["products"] < 0.2e6 and 0.9e6 < i1000["products"] < 1.2e6


def test_binding_lists_the_new_symbols_and_the_library_exports_them():
    assert all(s in capi.SYMBOLS for s in NEW_SYMBOLS)
    assert all(hasattr(capi.lib(), s) for s in NEW_SYMBOLS)
    assert all(hasattr(capi.HipNetwork, m) for m in ("pfa_pattern", "pfa_batched", "pfa_batched_dev", "pfa_paths", "solution_pfa", "ensemble_pfa"))
    assert capi.ABI_VERSION == 6 and capi.lib().kin_abi_version() == 6


def test_second_stage_keeps_production_and_consumption_apart():
    g = pc.PfaRef(pc.hand_networks()["chain"][0], 1)
    edge = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(g.rows, g.cols))}
    rp, rc = np.zeros(g.E), np.zeros(g.E)
    rp[edge[(0, 1)]] = 0.5      # A -> M by production only,
    rc[edge[(1, 2)]] = 0.25     # M -> B by consumption only: nothing reaches (A, B)
    assert _pairs(g, g.second(rp, rc)) == {(0, 1): 0.5, (0, 2): 0.0, (1, 0): 0.0, (1, 2): 0.25, (2, 0): 0.0, (2, 1): 0.0}
    rp[edge[(1, 2)]] = 0.125    # ... and now 0.5 * 0.125
    assert g.second(rp, rc)[list(zip(g.rows2, g.cols2)).index((0, 2))] == 0.0625


def test_reduce_network_pfa_on_reference_coefficients():
    """The chain with its side branch: A reaches B over the pair (A, B) of E2 alone, which the DRG graph does not have."""
    from oracle import oracle as orc
    net = pc.side_branch_network()
    names = ["A", "M", "B", "C", "D"]
    sd = S.SpeciesData.from_names(names, n_atoms=[1, 2, 3, 4, 5])
    rd = S.RxData(4, [[1], [2], [2], [4]], [[2], [3], [4], [5]], [[1]] * 4, [[1]] * 4, dH=[1.0, 2.0, 3.0, 4.0])
    calc = S.PrecalculatedArrheniusCalculator(Ea=[10.0, 20.0, 30.0, 40.0], A=[1.0, 2.0, 3.0, 4.0])
    u = np.zeros((2, 5)); u[0, 0] = 1.0; u[1] = [0.5, 0.25, 0.1, 0.0, 0.0]
    out = SimpleNamespace(sd=sd, rd=rd, sol=SimpleNamespace(t=np.array([0.0, 1.0]), u=u))
    k = np.array([4.0, 4.0, 0.5, 1.0])               # q = (2, 1, 0.125, 0) in the second state
    on = orc.OracleNetwork.from_flat(net)
    rates = np.stack([on.rates(k, x) for x in u])
    g = pc.PfaRef(net, 1)
    coef, _ = g.coefficients(rates)
    pairs = _pairs(g, coef)
    assert pairs[(0, 1)] == 1.0 and pairs[(0, 2)] == 0.5 and pairs[(0, 3)] == 0.0625 and (0, 4) not in pairs
    red = S.reduce_network(out, calc, ["A"], 0.4, method="pfa", coef=(g.rowptr2, g.colidx2, coef))
    assert red.targets.tolist() == [0]
    assert red.species_kept.tolist() == [0, 1, 2]                # M over (A, M), B over (A, B); C at 0.0625 and D are dropped
    assert red.reactions_kept.tolist() == [0, 1]
    assert red.sd.toInt == {"A": 1, "M": 2, "B": 3} and red.rd.nr == 2 and red.rd.id_prods == [[2], [3]]
    assert red.calculator.Ea.tolist() == [10.0, 20.0] and len(calc.Ea) == 4
    assert np.array_equal(red.rowptr, g.rowptr2) and np.array_equal(red.colidx, g.colidx2) and np.array_equal(red.coef, coef)
    assert red.importance is None and red.eps == 0.4
    assert red.map_u0({"A": 1.0, "D": 0.0}) == {"A": 1.0}
    # the DRG graph of the same states: M -> B carries 1 / (2 + 1 + 0.125) only, and there is no edge (A, B)
    d = dc.DrgRef(net, 1)
    dcoef = d.coefficients(rates)[0]
    red_drg = S.reduce_network(out, calc, ["A"], 0.4, coef=(d.rowptr, d.colidx, dcoef))
    assert red_drg.species_kept.tolist() == [0, 1]
    with pytest.raises(ValueError):
        S.reduce_network(out, calc, ["A"], 0.4, method="pfa2")


@pytest.mark.parametrize("name,mode", pc.GPU_CASES)
def test_states_keep_the_derived_bound_meaningful(name, mode):
    """The condition under test_gpu_pfa.py's bound of the split stage: at most 1 % of the (edge, state) entries of rp and of rc
    have a bound above 1e-9 - the cap test_drg_host.py uses for the same states."""
    for pairing in (1, 0):
        rp, rc, bp, bc = pc.ref(name, mode, pairing)
        for what, r, b in (("rp", rp, bp), ("rc", rc, bc)):
            frac = float(np.mean(b > 1e-9))
            print(f"{name} {mode} pairing={pairing} {what}: {100 * frac:.3f} % of the bounds above 1e-9, median {np.median(b):.2e}")
            assert frac <= 0.01
            assert np.all(np.isfinite(r)) and np.all(r >= 0.0) and np.all(r <= 1.0 + 1e-12)
        # what the split stage has to agree with: the DRGEP denominators and |rp den - rc den| = |s|
        r_ep = ec.ref(name, mode, pairing, pc.B_GPU)[0]
        ok = r_ep < 1.0
        assert np.allclose(np.abs(rp - rc)[ok], r_ep[ok], rtol=0, atol=1e-9)
