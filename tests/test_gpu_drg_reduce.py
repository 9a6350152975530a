"""End to end: a solve, its directed relation graph, the reduced network, the reduced solve - on the device through the public
interface, against the same pipeline on the CPU (oracle BDF, the NumPy graph of drg_cases.py).

Setup: synthetic_crn(300, 1500), static 1000 K (Arrhenius, k_max = 1e12), tspan (0, 0.02) in 20 chunks of 1e-3 (21 saved
states), u0 = species 0 alone, no low-k cutoff. Targets: the five species of greatest maximum concentration (0, 44, 191, 211,
252 in the oracle's solve; species 0 is also the one non-zero in the first saved state).

Chosen on the CPU: pairing off, eps = 0.2.
  * The reduced network keeps 143 of 300 species and 628 of 1500 reactions.
  * The reference coefficient nearest to eps is 5.3e-3 of eps away (the condition: none within 1e-6), and without pairing the
    derived bound of every coefficient of these states is below 4e-14 - the selection cannot flip on rounding, and the
    device's own saved states, which agree with the oracle's to the solve's tolerances only, moved no coefficient by more than
    8.4e-7 when this was written. (With pairing the near-equilibrium states of this solve make 5 % of the (edge, state)
    entries pure cancellation, bounds up to 0.08: a selection made on them could flip, so the test does not use it. There
    eps = 0.3 keeps 142 species at a deviation of 6.8e7.)
  * Largest deviation of the five targets' trajectories, reduced against full, both by the oracle BDF, in tolerance units
    |u_red - u_full| / (abstol + reltol |u_full|) with abstol = 1e-10, reltol = 1e-8:  7.486e7  (species 44; the others
    7.9, 3.1e7, 5.8e7 and 3.1e7). A random network has no structure for the graph to find: halving it costs a relative
    error of the order of one in its main products. The figure is recorded, not judged.
The device pipeline has to select exactly the reference's sets, its reduced solve has to succeed and its targets have to stay
within 2 x 7.486e7 units of the full device solve (2: the step sequences of device and oracle differ)."""
import dataclasses

import numpy as np
import pytest

import drg_cases as dc
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S
from oracle import bdf as obdf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS_DRG, PAIRING, T_K = 0.2, False, 1000.0
CPU_DEVIATION = 7.486e7          # measured once on the CPU (docstring); never re-fitted to the device
ABSTOL, RELTOL = 1e-10, 1e-8


@pytest.fixture(scope="module")
def reference():
    """The CPU pipeline up to the selection: oracle solve, NumPy graph, kept species and reactions."""
    net, Ea, A = dc.synth(300, 1500)
    k = orc.arrhenius(Ea, A, T_K, k_max=1e12)
    on = orc.OracleNetwork.from_flat(net)
    u0 = np.zeros(300); u0[0] = 1.0
    t, u, rc, _ = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), 300,
                                            dict(tspan=(0.0, 0.02), solve_chunks=True, solve_chunkstep=1e-3, abstol=ABSTOL, reltol=RELTOL),
                                            u0, k0=k)
    assert rc == 0 and len(t) == 21
    targets = np.sort(np.argsort(-u.max(axis=0), kind="stable")[:5])
    g = dc.DrgRef(net, PAIRING)
    coef, bound, _, _ = g.coefficients(np.stack([on.rates(k, u[b]) for b in range(len(t))]))
    kept = dc.select(g.rowptr, g.colidx, coef, np.union1d(targets, np.flatnonzero(u[0] != 0)), EPS_DRG)
    inside = np.zeros(300, bool); inside[kept] = True
    rx = [r for r in range(net.n_reactions) if all(inside[s] for s, _ in net.reaction(r)[0]) and all(inside[s] for s, _ in net.reaction(r)[1])]
    return dict(net=net, Ea=Ea, A=A, targets=targets, graph=g, coef=coef, bound=bound, kept=kept, rx=np.array(rx, np.int64))


def test_reference_choice_of_eps_holds(reference):
    coef, kept = reference["coef"], reference["kept"]
    assert len(kept) < 150 and len(kept) == 143 and len(reference["rx"]) == 628
    assert reference["targets"].tolist() == [0, 44, 191, 211, 252]
    assert np.min(np.abs(coef - EPS_DRG)) > 1e-6 * EPS_DRG
    assert np.max(reference["bound"]) < 1e-6 * EPS_DRG          # the device's coefficients cannot cross eps either


def test_device_pipeline_selects_the_reference_sets_and_solves_the_reduced_network(reference):
    net, Ea, A = reference["net"], reference["Ea"], reference["A"]
    sd = S.SpeciesData.from_names([f"S{i}" for i in range(300)])
    rd = S.RxData.from_flat(net)
    calc = S.PrecalculatedArrheniusCalculator(Ea, A, k_max=1e12)
    cond = C.ConditionSet({"T": T_K})
    pars = S.ODESimulationParams(tspan=(0.0, 0.02), u0={"S0": 1.0}, solve_chunkstep=1e-3, abstol=ABSTOL, reltol=RELTOL, low_k_cutoff="none")
    full = S.solve_network(S.StaticODESolve(pars, cond, calc), sd, rd)
    assert full.sol.retcode == "Success" and len(full.sol.t) == 21 and full.rd.nr == 1500
    targets = np.sort(np.argsort(-np.asarray(full.sol.u).max(axis=0), kind="stable")[:5])
    assert targets.tolist() == reference["targets"].tolist()
    red = S.reduce_network(full, calc, [f"S{i}" for i in targets], EPS_DRG, pairing=PAIRING)
    g = reference["graph"]
    assert np.array_equal(red.rowptr, g.rowptr) and np.array_equal(red.colidx, g.colidx)
    # the states of device and oracle agree to the solve's tolerances, not to rounding: reported, the sets are what is asserted
    print(f"coefficients, device against reference: max |difference| {np.max(np.abs(red.coef - reference['coef'])):.3e}")
    assert red.species_kept.tolist() == reference["kept"].tolist()
    assert red.reactions_kept.tolist() == reference["rx"].tolist()
    assert red.sd.n == 143 and red.rd.nr == 628 and len(red.calculator.Ea) == 628
    pars_red = dataclasses.replace(pars, u0=red.map_u0(pars.u0))
    small = S.solve_network(S.StaticODESolve(pars_red, cond, red.calculator), red.sd, red.rd)
    assert small.sol.retcode == "Success" and len(small.sol.t) == 21
    new = {int(old): i for i, old in enumerate(red.species_kept)}
    u_full = np.asarray(full.sol.u)[:, targets]
    u_red = np.asarray(small.sol.u)[:, [new[int(s)] for s in targets]]
    dev = np.abs(u_red - u_full) / (ABSTOL + RELTOL * np.abs(u_full))
    print(f"targets, reduced against full on the device: {dev.max():.4e} tolerance units (per target {dev.max(axis=0)}); the CPU's {CPU_DEVIATION:.4e}")
    assert dev.max() <= 2.0 * CPU_DEVIATION
