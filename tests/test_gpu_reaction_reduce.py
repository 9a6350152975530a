"""End to end: a solve, its directed relation graph, the reaction importance over the kept species, the network reduced in
species AND reactions, the reduced solve - on the device through the public interface, against the same pipeline on the CPU
(oracle BDF, the NumPy graph of drg_cases.py, the NumPy importance of reaction_importance_cases.py).

Setup: that of test_gpu_drg_reduce.py - synthetic_crn(300, 1500), static 1000 K (Arrhenius, k_max = 1e12), tspan (0, 0.02) in
20 chunks of 1e-3 (21 saved states), u0 = species 0 alone, no low-k cutoff, the five species of greatest maximum concentration
as targets (0, 44, 191, 211, 252), pairing off, eps = 0.2 - plus reaction_eps = 0.02.

Chosen on the CPU:
  * The species step keeps 143 of 300 species and 628 of 1500 reactions; of those 628, 522 have an importance >= 0.02 judged
    by the 143 kept species (536 at 0.01, 463 at 0.05, 398 at 0.1, 238 at 0.2).
  * The importance nearest to the threshold is 4.9e-2 of it away (the condition: none within 1e-3) and the derived bound of every
    importance of these states is below 1.5e-14: the selection cannot flip on rounding.
  * Largest deviation of the five targets' trajectories against the full solve, all by the oracle BDF, in tolerance units
    |u_red - u_full| / (abstol + reltol |u_full|) with abstol = 1e-10, reltol = 1e-8:
        species-only reduction   7.4861e7
        reaction-reduced         7.4629e7   (species 44; the others 0.80, 3.1e7, 6.7e7 and 3.1e7) - no worse
    and the reaction-reduced solve against the species-only one: 5.6e6. Dropping 106 more reactions costs a fraction of what
    the species step cost. (0.05 and above cost more than the species step did.) The figures are recorded, not judged.
The device pipeline has to select exactly the reference's species and reactions, its reduced solve has to succeed and its
targets have to stay within 2 x 7.4629e7 units of the full device solve (2: the step sequences of device and oracle differ,
the factor of test_gpu_drg_reduce.py)."""
import dataclasses

import numpy as np
import pytest

import drg_cases as dc
import reaction_importance_cases as rc
from kinetica_jl_amd import conditions as C
from kinetica_jl_amd import solving as S
from oracle import bdf as obdf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

EPS_DRG, EPS_RX, PAIRING, T_K = 0.2, 0.02, False, 1000.0
CPU_DEVIATION = 7.4629e7         # measured once on the CPU (docstring); never re-fitted to the device
ABSTOL, RELTOL = 1e-10, 1e-8


def _oracle_solve(net, k):
    on = orc.OracleNetwork.from_flat(net)
    u0 = np.zeros(300); u0[0] = 1.0
    t, u, rcode, _ = obdf.solve_network_oracle(lambda kk: (lambda y: on.rhs(kk, y)), lambda kk: (lambda y: on.jac(kk, y)), 300,
                                               dict(tspan=(0.0, 0.02), solve_chunks=True, solve_chunkstep=1e-3, abstol=ABSTOL, reltol=RELTOL),
                                               u0, k0=k)
    assert rcode == 0 and len(t) == 21
    return on, u


@pytest.fixture(scope="module")
def reference():
    """The CPU pipeline: oracle solve, NumPy graph, kept species, NumPy importance over them, kept reactions, and the oracle
    solve of the reduced network (its reactions alone on the full species numbering: the same trajectories)."""
    net, Ea, A = dc.synth(300, 1500)
    k = orc.arrhenius(Ea, A, T_K, k_max=1e12)
    on, u = _oracle_solve(net, k)
    targets = np.sort(np.argsort(-u.max(axis=0), kind="stable")[:5])
    g = dc.DrgRef(net, PAIRING)
    rates = np.stack([on.rates(k, u[b]) for b in range(len(u))])
    coef, _, _, _ = g.coefficients(rates)
    kept = dc.select(g.rowptr, g.colidx, coef, np.union1d(targets, np.flatnonzero(u[0] != 0)), EPS_DRG)
    inside = np.zeros(300, bool); inside[kept] = True
    rx_species = np.array([r for r in range(net.n_reactions)
                           if all(inside[s] for s, _ in net.reaction(r)[0]) and all(inside[s] for s, _ in net.reaction(r)[1])], np.int64)
    imp, bound, _, _ = rc.RiRef(net, PAIRING).importance(rates, selected=kept)
    rx = rx_species[imp[rx_species] >= EPS_RX]
    _, u_red = _oracle_solve(net.subset(rx), k[rx])
    dev = np.abs(u_red[:, targets] - u[:, targets]) / (ABSTOL + RELTOL * np.abs(u[:, targets]))
    return dict(net=net, Ea=Ea, A=A, targets=targets, graph=g, kept=kept, rx_species=rx_species, imp=imp, bound=bound, rx=rx,
                cpu_deviation=float(dev.max()))


def test_reference_choice_of_the_thresholds_holds(reference):
    imp, rx_species = reference["imp"], reference["rx_species"]
    assert reference["targets"].tolist() == [0, 44, 191, 211, 252]
    assert len(reference["kept"]) == 143 and len(rx_species) == 628 and len(reference["rx"]) == 522
    nearest = np.min(np.abs(imp[rx_species] - EPS_RX)) / EPS_RX
    print(f"importance nearest to the threshold: {nearest:.3e} of it away; largest bound {np.max(reference['bound']):.3e}; "
          f"CPU deviation {reference['cpu_deviation']:.4e}")
    assert nearest > 1e-3
    assert np.max(reference["bound"]) < 1e-6 * EPS_RX           # the device's importance cannot cross the threshold either
    assert abs(reference["cpu_deviation"] - CPU_DEVIATION) <= 1e-3 * CPU_DEVIATION     # the constant is the fixture's figure


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
    red = S.reduce_network(full, calc, [f"S{i}" for i in targets], EPS_DRG, pairing=PAIRING, reaction_eps=EPS_RX)
    # the states of device and oracle agree to the solve's tolerances, not to rounding: reported, the sets are what is asserted
    inside = reference["rx_species"]
    print(f"importance of the {len(inside)} candidates, device against reference: max |difference| "
          f"{np.max(np.abs(red.reaction_importance - reference['imp'])[inside]):.3e}")
    assert red.reaction_eps == EPS_RX and red.reaction_importance.shape == (1500,)
    assert np.all(red.reaction_importance >= 0.0) and np.all(red.reaction_importance <= 1.0)
    assert red.species_kept.tolist() == reference["kept"].tolist()
    assert red.reactions_kept.tolist() == reference["rx"].tolist()
    assert red.sd.n == 143 and red.rd.nr == 522 == len(red.calculator.Ea)
    # the importance reduce_network computed is the public function's, and the species step alone is what it was
    again = S.reaction_importance(full, calc, species=red.species_kept, pairing=PAIRING)
    assert np.array_equal(again, red.reaction_importance)
    by_name = S.reaction_importance(full, calc, species=[f"S{i}" for i in red.species_kept], pairing=PAIRING, importance=again)
    assert np.array_equal(by_name, again)
    species_only = S.reduce_network(full, calc, [f"S{i}" for i in targets], EPS_DRG, pairing=PAIRING, coef=(red.rowptr, red.colidx, red.coef))
    assert species_only.reactions_kept.tolist() == reference["rx_species"].tolist() and species_only.reaction_importance is None
    pars_red = dataclasses.replace(pars, u0=red.map_u0(pars.u0))
    small = S.solve_network(S.StaticODESolve(pars_red, cond, red.calculator), red.sd, red.rd)
    assert small.sol.retcode == "Success" and len(small.sol.t) == 21
    new = {int(old): i for i, old in enumerate(red.species_kept)}
    u_full = np.asarray(full.sol.u)[:, targets]
    u_red = np.asarray(small.sol.u)[:, [new[int(s)] for s in targets]]
    dev = np.abs(u_red - u_full) / (ABSTOL + RELTOL * np.abs(u_full))
    print(f"targets, reaction-reduced against full on the device: {dev.max():.4e} tolerance units (per target {dev.max(axis=0)}); "
          f"the CPU's {CPU_DEVIATION:.4e}")
    assert dev.max() <= 2.0 * CPU_DEVIATION
