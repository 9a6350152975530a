"""Host-side mirror of the reference's solve interface (src/solving/*.jl, src/analysis/io.jl):
ODESimulationParams / StaticODESolve / VariableODESolve / solve_network / ODESolveOutput, the
kinetic calculators, RxFilter and the CRN containers the solve reads. Same names, argument
meaning and error behaviour as the reference; all numerics go through the C ABI
(include/kinetica_hip.h) into libkinetica_hip.so - there is no CPU path here.

A Julia user keeps the reference's own types and calls the same library through the `ccall`
shim in INTEGRATION.md; this module is the runnable twin used by the parity tests.
"""
from __future__ import annotations

import copy
import dataclasses
import math
from dataclasses import dataclass, field
from collections.abc import Mapping
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np

from . import capi
from .conditions import (ConditionSet, get_initial_conditions, get_static_conditions, get_tstops, isstatic,
                         isvariable, solve_variable_conditions)
from .synth import FlatNetwork, from_lists

__all__ = ["SpeciesData", "RxData", "RxFilter", "get_filter_mask", "DummyKineticCalculator",
           "PrecalculatedArrheniusCalculator", "PrecalculatedLindemannCalculator", "allows_continuous",
           "has_conditions", "setup_network", "ODESimulationParams", "StaticODESolve", "VariableODESolve",
           "HIPBDF", "HIPRK45", "ArrheniusRates", "solve_network", "sample_arrhenius", "identify_next_seeds", "insert_inert", "ODESolveOutput", "ODESolution", "tconvert", "make_u0", "apply_low_k_cutoff",
           "get_max_rates", "get_initial_rates", "calculate_discrete_rates",
           "solve_network_ensemble",   # EXTENSION: the reference has no ensemble call
           "flux_weights", "held_stop_index", "ReactionFluxes", "reaction_fluxes", "ensemble_flux_sources",   # EXTENSION: post-hoc flux analysis
           "EnsembleStatistics", "ensemble_statistics",   # EXTENSION: statistics across the members of an ensemble
           "SobolIndices", "sobol_design", "sobol_indices"]   # EXTENSION: variance-based sensitivity of a Saltelli design

_T_UNIT = {  # src/utils.jl:77-97
    "picoseconds": 1.0e-12, "ps": 1.0e-12, "nanoseconds": 1.0e-9, "ns": 1.0e-9, "microseconds": 1.0e-6, "us": 1.0e-6,
    "milliseconds": 1.0e-3, "ms": 1.0e-3, "seconds": 1.0, "s": 1.0, "minutes": 60.0, "mins": 60.0, "hours": 3600.0,
    "hrs": 3600.0, "days": 86400.0, "months": 2.6297368e06, "mts": 2.6297368e06, "years": 3.15576e07, "yrs": 3.15576e07,
}


def tconvert(*args):
    """tconvert(t, from, to) / tconvert(from, to) (src/utils.jl:21-43)."""
    t, fu, tu = (1.0, *args) if len(args) == 2 else args
    if fu not in _T_UNIT or tu not in _T_UNIT:
        raise RuntimeError("Unknown unit specified in time conversion!")
    return float(t) * _T_UNIT[fu] / _T_UNIT[tu]


# ---- CRN containers (src/exploration/network.jl:1-8, 193-203): only what the solve reads -------
@dataclass
class SpeciesData:
    toInt: Dict[str, int]      # SMILES -> species id (1-based, as in the reference)
    toStr: Dict[int, str]
    n: int
    xyz: Optional[Dict[int, dict]] = None     # per-species geometry frames; the solve side only reads "N_atoms"

    @classmethod
    def from_names(cls, names: Sequence[str], n_atoms: Optional[Sequence[int]] = None):
        xyz = None if n_atoms is None else {i + 1: {"N_atoms": int(a)} for i, a in enumerate(n_atoms)}
        return cls({s: i + 1 for i, s in enumerate(names)}, {i + 1: s for i, s in enumerate(names)}, len(names), xyz)

    def subset(self, ids):
        """(sd_new, new_id): the species `ids` (1-based) renumbered 1 .. len(ids) in ascending order of their old ids, and the
        dict old id -> new id. EXTENSION (the reference only ever grows a SpeciesData): what a reduced network is solved with."""
        ids = sorted(set(int(i) for i in ids))
        if ids and (ids[0] < 1 or ids[-1] > self.n):
            raise ValueError("species id out of range")
        new_id = {old: i + 1 for i, old in enumerate(ids)}
        xyz = None if self.xyz is None else {new_id[old]: self.xyz[old] for old in ids if old in self.xyz}
        return SpeciesData({self.toStr[old]: new for old, new in new_id.items()}, {new: self.toStr[old] for old, new in new_id.items()},
                           len(ids), xyz), new_id


@dataclass
class RxData:
    nr: int
    id_reacs: List[List[int]]      # 1-based species ids
    id_prods: List[List[int]]
    stoic_reacs: List[List[int]]
    stoic_prods: List[List[int]]
    dH: Optional[List[float]] = None

    @classmethod
    def from_flat(cls, net: FlatNetwork):
        ir, ip, sr, sp = [], [], [], []
        for r in range(net.n_reactions):
            re, pr = net.reaction(r)
            ir.append([int(s) + 1 for s, _ in re]); sr.append([int(c) for _, c in re])
            ip.append([int(s) + 1 for s, _ in pr]); sp.append([int(c) for _, c in pr])
        return cls(net.n_reactions, ir, ip, sr, sp)

    def __deepcopy__(self, memo):
        # deepcopy(rd) of solve_network's copy_network (methods.jl:107-111): rows are lists of ints, so a row-wise slice copy
        # is a full copy - 20x faster than the generic deepcopy on a 50k-reaction network (0.46 s -> 0.02 s)
        rows = lambda L: [r[:] for r in L]
        return RxData(self.nr, rows(self.id_reacs), rows(self.id_prods), rows(self.stoic_reacs), rows(self.stoic_prods),
                      None if self.dH is None else list(self.dH))

    def splice(self, rids):
        """splice!(rd, rids): removes the reactions at the (0-based here) positions `rids`
        (src/exploration/network.jl:514-529)."""
        if len(rids) == 0:
            return
        kill = set(int(i) for i in rids)
        keep = [i for i in range(self.nr) if i not in kill]
        for name in ("id_reacs", "id_prods", "stoic_reacs", "stoic_prods"):
            setattr(self, name, [getattr(self, name)[i] for i in keep])
        if self.dH is not None:
            self.dH = [self.dH[i] for i in keep]
        self.nr = len(keep)

    def subset_species(self, new_id):
        """(rd_new, kept): the reactions ALL of whose species, on both sides, are keys of `new_id` (old id -> new id, as
        SpeciesData.subset returns it), renumbered, and their 0-based positions in this RxData. EXTENSION next to splice,
        which only removes reactions."""
        kept = [r for r in range(self.nr) if all(i in new_id for i in self.id_reacs[r]) and all(i in new_id for i in self.id_prods[r])]
        ren = lambda L: [[new_id[i] for i in L[r]] for r in kept]
        cp = lambda L: [L[r][:] for r in kept]
        return RxData(len(kept), ren(self.id_reacs), ren(self.id_prods), cp(self.stoic_reacs), cp(self.stoic_prods),
                      None if self.dH is None else [self.dH[r] for r in kept]), kept

    def flat(self, n_species):
        """Flat arrays for kin_network_create (index_base = 1)."""
        rp, pp = [0], [0]
        for r in range(self.nr):
            rp.append(rp[-1] + len(self.id_reacs[r])); pp.append(pp[-1] + len(self.id_prods[r]))
        cat = lambda L: np.array([x for row in L for x in row], dtype=np.int64)
        return (n_species, np.array(rp, np.int64), cat(self.id_reacs), cat(self.stoic_reacs),
                np.array(pp, np.int64), cat(self.id_prods), cat(self.stoic_prods))


# ---- reaction filters (src/solving/filters.jl) ----------------------------------------------------
def insert_inert(rd: "RxData", sd: "SpeciesData", inert_species: Sequence[str]):
    """insert_inert!(rd, sd, inert_species) (src/solving/solve_utils.jl:126-192), topology part: every unimolecular
    reaction (one reactant with stoichiometry 1) becomes bimolecular with the inert species as a bystander on both
    sides; with several inert species the reaction is copied once per additional collision partner (new reactions
    appended, the original modified for the last partner). The reference also builds 3D geometries for new species
    and re-hashes the reactions (OpenBabel, stable_hash): chemistry metadata the solve path does not read."""
    ids = []
    for name in inert_species:
        if name not in sd.toInt:
            sd.n += 1
            sd.toInt[name] = sd.n
            sd.toStr[sd.n] = name
        ids.append(sd.toInt[name])
    uni = [i for i in range(rd.nr) if len(rd.id_reacs[i]) == 1 and rd.stoic_reacs[i][0] == 1]
    for pos, sid in enumerate(ids):
        if pos < len(ids) - 1:
            for rid in uni:
                rd.id_reacs.append(rd.id_reacs[rid] + [sid]); rd.id_prods.append(rd.id_prods[rid] + [sid])
                rd.stoic_reacs.append(rd.stoic_reacs[rid] + [1]); rd.stoic_prods.append(rd.stoic_prods[rid] + [1])
                if rd.dH is not None:
                    rd.dH.append(rd.dH[rid])
                rd.nr += 1
        else:
            for rid in uni:
                rd.id_reacs[rid] = rd.id_reacs[rid] + [sid]; rd.id_prods[rid] = rd.id_prods[rid] + [sid]
                rd.stoic_reacs[rid] = rd.stoic_reacs[rid] + [1]; rd.stoic_prods[rid] = rd.stoic_prods[rid] + [1]


class RxFilter:
    def __init__(self, filters: Optional[List[Callable]] = None, keep_filtered: bool = False):
        self.filters = [lambda sd, rd: [False] * rd.nr] if filters is None else filters
        self.keep_filtered = keep_filtered


def get_filter_mask(rf: RxFilter, sd, rd):
    """filters.jl:40-52"""
    if len(rf.filters) == 0:
        raise RuntimeError("RxFilter has not filter functions defined.")
    mask = np.zeros(rd.nr, bool)
    for f in rf.filters:
        mask |= np.asarray(f(sd, rd), dtype=bool)
    return ~mask if rf.keep_filtered else mask


# ---- kinetic calculators (src/solving/calculator.jl) ------------------------------------------------
class AbstractKineticCalculator:
    pass


class DummyKineticCalculator(AbstractKineticCalculator):
    """calculator.jl:72-158: always returns the stored rates (scaled to the time unit; note the
    cap is applied BEFORE t_mult here, calculator.jl:130-132)."""

    def __init__(self, rates, k_max=None, t_unit="s"):
        self.rates = np.asarray(rates, dtype=float).copy()
        self.k_max, self.t_unit, self.t_mult = k_max, t_unit, tconvert(t_unit, "s")

    def __call__(self, T=None, V=None):
        if T is None and V is None:
            raise TypeError("DummyKineticCalculator needs T and/or V")   # MethodError in the reference
        if self.k_max is None:
            return self.rates * self.t_mult
        return 1.0 / ((1.0 / self.k_max) + (1.0 / self.rates)) * self.t_mult

    def splice(self, rids):
        self.rates = np.delete(self.rates, np.asarray(rids, dtype=int))


class PrecalculatedArrheniusCalculator(AbstractKineticCalculator):
    """calculator.jl:164-238. k = A exp(-Ea/RT) N_A t_mult, optionally capped; evaluated on the device
    (kin_arrhenius_eval), so the cutoff decision and the solve see the same numbers."""

    def __init__(self, Ea, A, k_max=None, t_unit="s"):
        self.Ea = np.asarray(Ea, dtype=float).copy()
        self.A = np.asarray(A, dtype=float).copy()
        self.k_max, self.t_unit, self.t_mult = k_max, t_unit, tconvert(t_unit, "s")

    def __call__(self, T):
        return capi.arrhenius_eval(self.Ea, self.A, float(T), self.k_max, self.t_mult)

    def splice(self, rids):
        rids = np.asarray(rids, dtype=int)
        self.Ea = np.delete(self.Ea, rids)
        self.A = np.delete(self.A, rids)


class PrecalculatedLindemannCalculator(AbstractKineticCalculator):
    """calculator.jl:244-320: a stub in the reference (its functor throws), mirrored as such."""

    def __init__(self, Ea, A_0, A_inf, k_max=None, t_unit="s"):
        self.Ea, self.A_0, self.A_inf = map(lambda x: np.asarray(x, dtype=float), (Ea, A_0, A_inf))
        self.k_max, self.t_unit, self.t_mult = k_max, t_unit, tconvert(t_unit, "s")

    def __call__(self, **kw):
        raise RuntimeError("Lindemann calculator is not implemented yet.")   # calculator.jl:308, 313


def setup_network(sd, rd, calc):
    """setup_network! (calculator.jl:102-106, 200-204)"""
    if isinstance(calc, DummyKineticCalculator):
        if len(calc.rates) != rd.nr:
            raise ValueError(f"Number of rates ({len(calc.rates)}) does not match number of reactions in `RxData` ({rd.nr})")
    elif isinstance(calc, PrecalculatedArrheniusCalculator):
        if len(calc.Ea) != rd.nr or len(calc.A) != rd.nr:
            raise ValueError(f"Number of parameters (Ea: {len(calc.Ea)}, A: {len(calc.A)}) does not match number of reactions in `RxData` ({rd.nr})")


def has_conditions(calc, symbols):
    """calculator.jl:154-156, 234-236"""
    allowed = {"T", "V"} if isinstance(calc, DummyKineticCalculator) else {"T"}
    return all(str(s) in allowed for s in symbols)


def allows_continuous(calc):
    """calculator.jl:158, 238"""
    return isinstance(calc, (DummyKineticCalculator, PrecalculatedArrheniusCalculator))


def _call_calc(calc, conds: dict):
    if isinstance(calc, DummyKineticCalculator):
        return calc(T=conds.get("T"), V=conds.get("V"))
    return calc(T=conds["T"])


# ---- solver sentinels: what `pars.solver` holds to select this backend (HIPBDF / HIPRK45) -------------
@dataclass
class HIPBDF:
    """`ODESimulationParams(solver=HIPBDF(), ...)`: the library's variable-order BDF with the on-device sparse LU
    (kin_solve). The reference hands `pars.solver` to `init` together with `dtmin = eps(solve_chunkstep)` or
    `eps(tspan[end])` (methods.jl:164, 232, 694, 770) and `ODESimulationParams` has no field for it (params.jl:3-27):
    a solver-level option therefore lives on the solver object. `dtmin=None` keeps the reference's value.
    `warm_chunks=True` (extension): a chunkwise solve keeps difference history, order and step size across chunk starts whose
    rate constants did not change (kin_params.solve_chunks = 2) instead of re-initialising the integrator there as the
    reference does (`reinit!`, methods.jl:819): the same exact solution - chunk boundaries of a StaticODESolve are not events -
    in ~2/3 of the steps and closer to it (C3, 30 chunks: 58 against 170 tolerance units); rate updates still re-initialise."""
    dtmin: Optional[float] = None
    warm_chunks: bool = False


@dataclass
class HIPRK45:
    """`ODESimulationParams(solver=HIPRK45(), ...)`: the explicit Dormand-Prince 5(4) pair (kin_solve_explicit)."""
    dtmin: Optional[float] = None


# ---- ODESimulationParams (src/solving/params.jl) ---------------------------------------------------
@dataclass
class ODESimulationParams:
    tspan: tuple
    u0: Union[Dict[str, float], Sequence[float]]
    solver: object = None          # None / "BDF": the library's implicit BDF; "RK45" (or "DP5", "explicit"): its explicit
                                   # Dormand-Prince 5(4) pair (kin_solve_explicit); the reference takes any SciML algorithm here
    jac: bool = True
    sparse: bool = True
    abstol: float = 1.0e-10
    reltol: float = 1.0e-8
    adaptive_tols: bool = True
    update_tols: bool = False
    solve_chunks: bool = True
    solve_chunkstep: float = 1e-3
    maxiters: int = 100000
    ban_negatives: bool = False
    progress: bool = False
    save_interval: Optional[float] = None
    low_k_cutoff: Union[float, str] = "auto"     # :auto / :none / number
    low_k_maxconc: float = 2.0
    allow_short_u0: bool = False
    dtmin: Optional[float] = None   # EXTENSION kept for earlier callers (not a field of the reference's struct; prefer
                                    # `solver=HIPBDF(dtmin=...)`): None = what the reference hard-codes,
                                    # eps(solve_chunkstep) / eps(tspan[end]) (methods.jl:164, 232, 694, 770)

    def __post_init__(self):
        # validation of the keyword constructor (params.jl:77-104); ArgumentError -> ValueError
        if self.tspan[0] >= self.tspan[1]:
            raise ValueError(f"Invalid time span: Start = {self.tspan[0]}, End = {self.tspan[1]}")
        if isinstance(self.low_k_cutoff, str):
            if self.low_k_cutoff not in ("auto", "none"):
                raise ValueError("low_k_cutoff must be a numerical value or one of [:auto, :none]")
        elif self.low_k_cutoff < 0:
            raise ValueError("low_k_cutoff must be a positive number or one of [:auto, :none]")
        if self.solve_chunks:
            q = self.tspan[1] / self.solve_chunkstep
            if q != math.floor(q):
                raise ValueError("Simulation timespan is not divisible by requested chunkwise simulation step size")
        if self.solve_chunks and self.save_interval is not None and self.save_interval > self.solve_chunkstep:
            raise ValueError("Solution save interval must be less than chunkwise simulation step size")

    @property
    def explicit(self):
        """True when `solver` selects the explicit integrator."""
        if isinstance(self.solver, HIPRK45):
            return True
        if isinstance(self.solver, HIPBDF):
            return False
        if self.solver is None or (isinstance(self.solver, str) and self.solver.upper() in ("BDF", "CVODE_BDF", "IMPLICIT")):
            return False
        if isinstance(self.solver, str) and self.solver.upper() in ("RK45", "DP5", "EXPLICIT"):
            return True
        raise ValueError(f"solver must be None / 'BDF' / HIPBDF() or 'RK45' / 'DP5' / 'explicit' / HIPRK45(), got {self.solver!r}")

    @property
    def solver_dtmin(self):
        """dtmin of the solver sentinel, else the extension field, else None (the reference's own choice)."""
        d = getattr(self.solver, "dtmin", None)
        return self.dtmin if d is None else d

    def to_kin_params(self):
        return capi.KinParams(tspan0=self.tspan[0], tspan1=self.tspan[1], abstol=self.abstol, reltol=self.reltol,
                              adaptive_tols=int(self.adaptive_tols), update_tols=int(self.update_tols),
                              solve_chunks=(2 if getattr(self.solver, "warm_chunks", False) else 1) if self.solve_chunks else 0,
                              ban_negatives=int(self.ban_negatives),
                              solve_chunkstep=self.solve_chunkstep, maxiters=int(self.maxiters),
                              save_interval=-1.0 if self.save_interval is None else self.save_interval,
                              dtmin=0.0 if self.solver_dtmin is None else float(self.solver_dtmin))


# ---- solve methods (src/solving/methods.jl:7-58) -----------------------------------------------------
class StaticODESolve:
    def __init__(self, pars, conditions, calculator, filter=None):
        if not isstatic(conditions):
            raise ValueError("All conditions must be static to run a StaticODESolve.")
        if not has_conditions(calculator, conditions.symbols):
            raise ValueError("Calculator does not support all of the provided conditions.")
        self.pars, self.conditions, self.calculator = pars, conditions, calculator
        self.filter = RxFilter() if filter is None else filter


class VariableODESolve:
    def __init__(self, pars, conditions, calculator, filter=None):
        if not has_conditions(calculator, conditions.symbols):
            raise ValueError("Calculator does not support all of the provided conditions.")
        if not conditions.discrete_updates and not allows_continuous(calculator):
            raise ValueError("Calculator does not support continuous rate updates in simulations.")
        self.pars, self.conditions, self.calculator = pars, conditions, calculator
        self.filter = RxFilter() if filter is None else filter


# ---- pre-solve pipeline (src/solving/solve_utils.jl) ---------------------------------------------------
def get_max_rates(conditions, calculator):
    """solve_utils.jl:19-54: enumerate min/max corners of the variable conditions (binary order,
    minimum first), keep the corner with the greatest mean rate (first maximum)."""
    static = get_static_conditions(conditions)
    var = [(s, p.minimum(), p.maximum()) for s, p in zip(conditions.symbols, conditions.profiles) if not isstatic(p)]
    if not var:
        return _call_calc(calculator, static)
    best, best_mean = None, -math.inf
    for bits in range(2 ** len(var)):
        conds = dict(static)
        for j, (s, lo, hi) in enumerate(var):
            conds[s] = hi if (bits >> (len(var) - 1 - j)) & 1 else lo
        k = _call_calc(calculator, conds)
        if np.mean(k) > best_mean:
            best, best_mean = k, np.mean(k)
    return best


def get_initial_rates(conditions, calculator):
    """solve_utils.jl:62-73"""
    return _call_calc(calculator, get_initial_conditions(conditions))


def apply_low_k_cutoff(rd, calc, pars, conditions):
    """apply_low_k_cutoff! (solve_utils.jl:213-245). Mutates rd AND the calculator, as the
    reference does. Returns the number of removed reactions."""
    if pars.low_k_cutoff == "none":
        return 0
    k_cutoff = pars.reltol / pars.tspan[-1] if pars.low_k_cutoff == "auto" else float(pars.low_k_cutoff)
    max_rates = get_max_rates(conditions, calc) * pars.low_k_maxconc ** 2
    low = [i for i, rate in enumerate(max_rates) if rate < k_cutoff]
    rd.splice(low)
    calc.splice(low)
    return len(low)


def make_u0(sd, pars):
    """solve_utils.jl:262-297"""
    if not isinstance(pars.u0, dict):
        u0 = np.asarray(pars.u0, dtype=float)
        if len(u0) != sd.n:
            if pars.allow_short_u0:
                out = np.zeros(sd.n)
                out[:len(u0)] = u0
                return out
            raise RuntimeError("Length of supplied initial concentration vector does not match with number of species in system.")
        return u0.copy()
    out = np.zeros(sd.n)
    for spec, conc in pars.u0.items():
        if spec not in sd.toInt:
            raise RuntimeError(f"Species {spec} not in SpeciesData. Check pars.u0 is correct.")
        out[sd.toInt[spec] - 1] = conc
    return out


def discrete_stop_temperatures(conditions):
    """(tstops, T(tstops)): the condition-interpolation half of calculate_discrete_rates (solve_utils.jl:91-104) for a
    calculator that reads :T only - what kin_solve needs instead of a rate table."""
    if not conditions.discrete_updates:
        raise RuntimeError("Cannot calculate discrete rates for a continuous ConditionSet.")
    tstops = get_tstops(conditions)
    prof = conditions.profiles[conditions.symbols.index("T")]
    T = np.full(len(tstops), float(prof.value)) if isstatic(prof) else np.asarray(prof.sol(tstops), dtype=float)
    return tstops, T


def calculate_discrete_rates(conditions, calculator, nr, handle=None):
    """solve_utils.jl:91-109: k_precalc[s] = calculator(conditions interpolated at tstop_s).
    With the Arrhenius calculator and a live network handle the S x R table is generated by the
    device kernel (kin_rate_table); otherwise by S calculator calls. Returns (tstops, T or None, table)."""
    if not conditions.discrete_updates:
        raise RuntimeError("Cannot calculate discrete rates for a continuous ConditionSet.")
    tstops = get_tstops(conditions)
    static = get_static_conditions(conditions)
    var = {s: p.sol(tstops) for s, p in zip(conditions.symbols, conditions.profiles) if isvariable(p)}
    if isinstance(calculator, PrecalculatedArrheniusCalculator) and handle is not None:
        T = var["T"] if "T" in var else np.full(len(tstops), static["T"])
        return tstops, T, handle.rate_table(T)
    table = np.empty((len(tstops), nr))
    for i in range(len(tstops)):
        conds = dict(static)
        conds.update({s: v[i] for s, v in var.items()})
        table[i] = _call_calc(calculator, conds)
    return tstops, None, table


# ---- results (src/analysis/io.jl:3-48; SciMLBase solution fields the callers read) ----------------------
@dataclass
class ODESolution:
    t: np.ndarray
    u: np.ndarray            # [len(t)][n_species]
    retcode: str
    k: Optional[object] = None
    stats: dict = field(default_factory=dict)
    umax: Optional[np.ndarray] = None    # max over saved times per species, reduced on the device (kin_solution_max)
    fluxes: Optional[object] = None      # ReactionFluxes of the solve (solve_network_ensemble(fluxes=True)), else None
    ensemble_stats: Optional[object] = None   # the ensemble's one EnsembleStatistics (solve_network_ensemble(statistics=...)), else None
    events: Optional[object] = None      # the ensemble's one EventTimes (solve_network_ensemble(events=...)), else None
    resampled: Optional[object] = None   # the ensemble's one ResampledEnsemble (solve_network_ensemble(resample=...)), else None
    observables: Optional[object] = None   # the ensemble's one Observables (solve_network_ensemble(observables=...)), else None

    def __call__(self, tq):
        """Linear interpolation res.sol(t) (docs/src/getting-started.md:232-236)."""
        tq = np.atleast_1d(np.asarray(tq, dtype=float))
        i = np.clip(np.searchsorted(self.t, tq, side="left"), 1, len(self.t) - 1)
        th = ((tq - self.t[i - 1]) / (self.t[i] - self.t[i - 1]))[:, None]
        return (1 - th) * self.u[i - 1] + th * self.u[i]


@dataclass
class DiscreteRates:
    """sol_k: DiffEqArray(k_precalc, tstops) (methods.jl:739, io.jl:38)."""
    t: np.ndarray
    u: np.ndarray            # [S][R']


class ArrheniusRates:
    """sol_k of a discrete-update solve with the Arrhenius calculator: the same DiffEqArray(k_precalc, tstops) seen from
    outside (`t`, `u[s]`, `len`), but no S x R table exists anywhere - not on the host, not on the device (C4: 14 001 x
    50 000 doubles = 5.6 GB). The solve received the temperatures at the stops and formed each stop's rate constants on
    the device when it reached it (kin_solve with T_stops); a row asked for here is evaluated by the same device functor
    (kin_arrhenius_eval: calculator.jl:223-232 literally), so `u[s]` is bit for bit what the integrator used.
    `u` of the whole object (`np.asarray(sol_k.u)`, `save_output`) materialises all rows on demand."""

    def __init__(self, t, T, Ea, A, k_max, t_mult):
        self.t = np.asarray(t, dtype=float)
        self.T = np.asarray(T, dtype=float)
        self._Ea, self._A, self._k_max, self._t_mult = np.array(Ea, dtype=float), np.array(A, dtype=float), k_max, t_mult
        self._full = None

    def __len__(self):
        return len(self.t)

    def row(self, s):
        if self._full is not None:
            return self._full[s]
        return capi.arrhenius_eval(self._Ea, self._A, float(self.T[s]), self._k_max, self._t_mult)

    __getitem__ = row

    @property
    def u(self):
        return _LazyRows(self)

    def materialize(self):
        if self._full is None:
            self._full = np.stack([self.row(s) for s in range(len(self.t))]) if len(self.t) else np.empty((0, len(self._Ea)))
        return self._full


class _LazyRows:
    """`sol_k.u`: rows on demand (`u[s]`), the full [S][R'] array when converted (`np.asarray(u)`, `u.shape`)."""

    def __init__(self, owner):
        self._o = owner

    def __len__(self):
        return len(self._o)

    def __getitem__(self, s):
        if isinstance(s, (int, np.integer)):
            return self._o.row(int(s))
        return self._o.materialize()[s]

    def __array__(self, dtype=None, copy=None):
        a = self._o.materialize()
        return a if dtype is None else a.astype(dtype)

    @property
    def shape(self):
        return (len(self._o), len(self._o._Ea))


@dataclass
class ODESolveOutput:
    sd: SpeciesData
    rd: RxData
    sol: ODESolution
    sol_k: Optional[DiscreteRates]
    sol_vcs: Optional[object]
    pars: ODESimulationParams
    conditions: ConditionSet


# ---- solve_network (src/solving/methods.jl:105-130, 330-360) ----------------------------------------------
class HipIntegrator:
    """What `solve_network(...; return_integrator=true)` hands back (methods.jl:98-100, 175-178): the
    initialised integrator, living on the device. `step()` = step!(integ), `solve()` = solve!(integ),
    `t` / `u` = integ.t / integ.u. It spans the whole tspan (solve_chunks=false) or the first chunk
    (solve_chunks=true: "integrators for chunkwise solutions require significant work to fully solve
    outside of their intended solution methods", methods.jl:244). Close it (or use `with`) to free the GPU."""

    def __init__(self, handle, sd, rd, pars):
        self._h, self.sd, self.rd, self.pars = handle, sd, rd, pars

    def step(self, n=1):
        """n accepted steps; returns how many were taken (fewer at the end of the span / on failure)."""
        return self._h.integrator_step(max(int(n), 1))

    def solve(self):
        self._h.integrator_step(0)
        return self

    @property
    def t(self):
        return self._h.integrator_state(with_u=False)[0]

    @property
    def u(self):
        return self._h.integrator_state()[1]

    @property
    def retcode(self):
        return capi.RETCODE_NAMES[self._h.integrator_state(with_u=False)[2]]

    @property
    def stats(self):
        return self._h.integrator_state(with_u=False)[3]

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def solve_network(method, sd, rd, copy_network=True, return_integrator=False):
    """Solve a network with static or variable kinetics on the MI355X.

    Pipeline order as in the reference: deepcopy -> [variable: solve condition
    profiles] -> filter -> splice -> setup_network! -> low-k cutoff (mutates the copies AND the
    caller's calculator) -> rates -> u0 -> solve -> ODESolveOutput with the REDUCED network."""
    pars, conditions, calc = method.pars, method.conditions, method.calculator
    sd_a, rd_a = (copy.deepcopy(sd), copy.deepcopy(rd)) if copy_network else (sd, rd)
    variable = isinstance(method, VariableODESolve)
    if variable:
        solve_variable_conditions(conditions, pars)
    mask = get_filter_mask(method.filter, sd_a, rd_a)
    rd_a.splice(np.nonzero(mask)[0])
    setup_network(sd_a, rd_a, calc)
    apply_low_k_cutoff(rd_a, calc, pars, conditions)
    u0 = make_u0(sd_a, pars)

    h = capi.HipNetwork(*rd_a.flat(sd_a.n), index_base=1)
    try:
        arr = isinstance(calc, PrecalculatedArrheniusCalculator)
        if arr:
            h.set_arrhenius(calc.Ea, calc.A, calc.k_max, calc.t_mult)
        sol_k = None
        sol_vcs = None
        continuous = variable and not conditions.discrete_updates and arr
        if continuous:
            # continuous rate updates (methods.jl:363-653): T(t) = the profile solution, linearly interpolated
            # (src/utils.jl:135-139); a static T in the set is a constant trace
            prof = conditions.profiles[conditions.symbols.index("T")]
            if isstatic(prof):
                nodes_t, nodes_T = np.array([pars.tspan[0], pars.tspan[1]]), np.array([prof.value, prof.value], dtype=float)
            else:
                nodes_t, nodes_T = prof.sol.t, prof.sol.u
        if pars.explicit and (return_integrator or continuous):
            # the explicit pair exists behind kin_solve_explicit only (static / discrete-update solves)
            raise ValueError("solver='RK45' is not available with return_integrator=true or continuous rate updates; "
                             "use the default BDF there")
        if return_integrator:
            # methods.jl:175-178, 242-246, 445-449, 706-709: hand back the initialised integrator instead of solving
            if continuous:
                h.integrator_init_continuous(pars.to_kin_params(), u0, nodes_t, nodes_T)
            elif not variable or not conditions.discrete_updates:
                h.set_rates(get_initial_rates(conditions, calc))
                h.integrator_init(pars.to_kin_params(), u0)
            else:
                if arr:
                    tstops, T = discrete_stop_temperatures(conditions)
                    h.integrator_init(pars.to_kin_params(), u0, tstops=tstops, T_stops=T)
                else:
                    tstops, T, table = calculate_discrete_rates(conditions, calc, rd_a.nr, handle=None)
                    h.integrator_init(pars.to_kin_params(), u0, tstops=tstops, k_table=table)
            integ, h = HipIntegrator(h, sd_a, rd_a, pars), None      # the integrator owns the handle now
            return integ
        if not variable or (not conditions.discrete_updates and not arr):
            # static rates (a Dummy calculator is constant under continuous updates as well)
            k0 = get_initial_rates(conditions, calc)
            h.set_rates(k0)
            t, u, rc, st, status = h.solve(pars.to_kin_params(), u0, explicit=pars.explicit)
        elif not conditions.discrete_updates:
            # k(t) = calculator(T(t)) evaluated on the device at every step attempt
            t, u, rc, st, status = h.solve_continuous(pars.to_kin_params(), u0, nodes_t, nodes_T)
        else:
            if arr:
                # Arrhenius + discrete updates: only T(tstop) is evaluated here (calculate_discrete_rates' interpolation of
                # the profile solutions, solve_utils.jl:91-104); the rate constants of a stop are formed on the device when
                # the solve reaches it, and sol_k hands out rows on demand - no S x R table on either side
                tstops, T = discrete_stop_temperatures(conditions)
                sol_k = ArrheniusRates(tstops, T, calc.Ea, calc.A, calc.k_max, calc.t_mult)
                t, u, rc, st, status = h.solve(pars.to_kin_params(), u0, tstops=tstops, T_stops=T, explicit=pars.explicit)
            else:
                tstops, T, table = calculate_discrete_rates(conditions, calc, rd_a.nr, handle=None)
                sol_k = DiscreteRates(tstops, table)
                t, u, rc, st, status = h.solve(pars.to_kin_params(), u0, tstops=tstops, k_table=table, explicit=pars.explicit)
        if status == capi.KIN_ERR_SOLVE_FAILED:
            raise RuntimeError("ODE solution failed.")      # ErrorException (solve_utils.jl:405-411)
        if variable and not conditions.discrete_updates:
            # ODESolutionVC's condition traces (solutions.jl:1-21, rebuild_vc_solution): one per VARIABLE condition of
            # the set, whatever the calculator reads (a Dummy calculator accepts :T and :V, calculator.jl:154-156)
            sol_vcs = {}
            for sym, prof in zip(conditions.symbols, conditions.profiles):
                if not isstatic(prof):
                    sol_vcs[sym] = np.interp(t, prof.sol.t, prof.sol.u)
        if pars.update_tols and st["final_abstol"] != pars.abstol:
            pars.abstol, pars.reltol = st["final_abstol"], st["final_reltol"]   # solve_utils.jl:397-401
        umax = h.solution_max()      # what identify_next_seeds reads, reduced where the trajectory lives
    finally:
        if h is not None:
            h.close()
    sol = ODESolution(t, u, capi.RETCODE_NAMES[rc], k=sol_k, stats=st, umax=umax)
    return ODESolveOutput(sd_a, rd_a, sol, sol_k, sol_vcs, pars, conditions)


def _same_filter(a, b):
    """Do two RxFilters select the same reactions by construction (the same object, or the same filter functions -
    a default RxFilter() of each method counts as the same)?"""
    if a is b:
        return True
    if a.keep_filtered != b.keep_filtered or len(a.filters) != len(b.filters):
        return False
    for f, g in zip(a.filters, b.filters):
        code_f, code_g = getattr(f, "__code__", None), getattr(g, "__code__", None)
        if not (f is g or (code_f is not None and code_f is code_g and not f.__closure__ and not g.__closure__)):
            return False
    return True


def _same_calculator(a, b):
    return a is b or (type(a) is type(b) and np.array_equal(a.Ea, b.Ea) and np.array_equal(a.A, b.A) and a.k_max == b.k_max
                      and a.t_mult == b.t_mult)


def _calculator_mismatch(a, b):
    """What keeps two Arrhenius calculators out of one ensemble call (None: nothing; they may differ in the VALUES of Ea / A):
    the type, the number of reactions, k_max and t_mult are the handle's, one for all members."""
    if type(a) is not type(b):
        return "type"
    if len(a.Ea) != len(b.Ea) or len(a.A) != len(b.A):
        return "length"
    if a.k_max != b.k_max:
        return "k_max"
    if a.t_mult != b.t_mult:
        return "t_mult"
    return None


def apply_ensemble_low_k_cutoff(rd, calc, pars, condition_sets, calculators=None):
    """apply_low_k_cutoff! over an ensemble (EXTENSION, solve_network_ensemble): a reaction is removed only if every condition
    set's cutoff removes it. calculators: one per condition set when the members' Arrhenius parameters differ (each member's
    maximum rates are then its own calculator's); None: `calc` for all. Mutates rd and `calc` as apply_low_k_cutoff does;
    returns the removed positions."""
    if pars.low_k_cutoff == "none":
        return np.zeros(0, dtype=int)
    k_cutoff = pars.reltol / pars.tspan[-1] if pars.low_k_cutoff == "auto" else float(pars.low_k_cutoff)
    low = np.ones(rd.nr, bool)
    for i, cs in enumerate(condition_sets):
        low &= get_max_rates(cs, calc if calculators is None else calculators[i]) * pars.low_k_maxconc ** 2 < k_cutoff
    rids = np.nonzero(low)[0]
    rd.splice(rids)
    calc.splice(rids)
    return rids


def solve_network_ensemble(methods, sd, rd, copy_network=True, fluxes=False, trajectories=True, statistics=None,
                           member_calculators=False, events=None, resample=None, observables=None):
    """EXTENSION (the reference has no ensemble call: it solves member after member through solve_network): K
    `VariableODESolve`s with Arrhenius condition sets - one temperature profile each, e.g. a set of heating rates or start
    temperatures - on one network in ONE ensemble call: kin_solve_ensemble_continuous when every set is continuous,
    kin_solve_ensemble_discrete when every set has ts_update (discrete rate updates: each member its own stops and the
    temperatures at them, discrete_stop_temperatures - stop grids of different lengths included). Returns one ODESolveOutput
    per member.

    The methods must share the calculator, the filter and every ODESimulationParams field except u0, and all be continuous or
    all discrete-update sets (ValueError otherwise, before anything touches the GPU).

    member_calculators=True: the methods' calculators must agree in type, length, k_max and t_mult only (ValueError otherwise)
    and may differ in the VALUES of Ea / A - uncertain barriers and prefactors; sample_arrhenius builds such calculators from a
    design. Every member is then solved with its own parameters (kin_solve_ensemble_*_params), its low-k cutoff uses its own
    calculator's maximum rates, sol_k of a discrete member and fluxes=True (kin_ensemble_flux on the per-member record) use its
    own parameters too. With calculators equal in value the call is exactly the one made without the flag, no Ea / A passed.
    The default keeps the refusal: calculators that differ by mistake are not silently solved as a design. solve_network's pipeline runs once: every
    member's solve_variable_conditions, filter, splice, setup_network!, low-k cutoff, then the members' u0. The low-k cutoff
    removes a reaction only if EVERY member's cutoff (its own condition set's maximum rates, apply_low_k_cutoff) removes it:
    when the members agree, the network is exactly the one solve_network builds for each; otherwise a member may keep
    reactions its own solve_network would have dropped (rates below its cutoff, which is the cutoff's own criterion for
    negligible). Every member's calculator object is spliced as solve_network splices it (once per distinct object).
    Per member as solve_network fills them: continuous sets give sol_vcs (the variable conditions at the saved times) and
    sol_k = None, discrete-update sets sol_vcs = None and sol_k = sol.k = ArrheniusRates of the member's own stops; sol.umax;
    sol.retcode the member's own (a failed member does not raise: the others' results stand); update_tols writes the
    member's final tolerances into its own `pars`. Ensembles are BDF only (pars.explicit raises ValueError). Static and
    non-Arrhenius sets raise ValueError: use HipNetwork.solve_ensemble (kin_solve_ensemble) or solve_network for those.

    fluxes=True: every member's sol.fluxes is its ReactionFluxes - what reaction_fluxes(out, calculator) gives, trapezoid
    weights over the member's own saved times and the rate constants the solve held there - from ONE segmented pass over the
    members' states where they live on the device (kin_ensemble_flux), before the handle closes. trajectories=False: no
    state is downloaded; sol.u is None, sol.t the member's saved times, sol.umax kin_ensemble_max's. With the defaults the
    function does what it did before either existed.

    statistics=True or a dict of ensemble_statistics' keyword arguments (quantiles, species, inputs, rank, use; species are
    0-based ids of the network as it is solved, inputs[K][P] one row per method): every member's sol.ensemble_stats refers to
    ONE shared EnsembleStatistics over the members that completed the save grid, computed from the states where they live on
    the device before the handle closes (with trajectories=False no state is downloaded). The key sobol=dict(M=, P=, ...) -
    sobol_indices' keyword arguments, species again 0-based - declares the methods a Saltelli design in sobol_design's layout
    (len(methods) == M (P + 2)) and fills ensemble_stats.sobol with its SobolIndices. A malformed `statistics` raises
    ValueError before anything touches the GPU. None (the default): nothing is computed. The keys of="t_peak" | "t_cross" with
    events=dict(...) take the statistics of that event time instead of the states (ensemble_statistics), and the sobol dict has
    the same two keys (sobol_indices).

    events=dict of event_times' keyword arguments (level, kind, direction, start, t_min, never, species; species 0-based ids
    of the network as it is solved): every member's sol.events refers to ONE shared EventTimes - per member and species the
    peak, its time and the time a level is first crossed - computed from the states where they live on the device before the
    handle closes; it works with trajectories=False. A malformed dict raises ValueError before anything touches the GPU.

    resample=dict(axis="T" | "t" | "t_rel" | array, at=[...], mode=, fill=, t_min=) puts the members on a common axis before the
    statistics and the event times look at them: members of a heating-rate or start-temperature sweep sit at different
    temperatures at one saved time, and a mean "at row j" compares different stages of the programme. The order inside the call:
    the solve; whatever refers to the solve's own rows, as always (the trajectory download, sol.umax, fluxes=True); then
    resample_ensemble(store=True) - the stored ensemble becomes the states at the queries `at` of every member's axis; then
    statistics= and events= over that record with t = at: EnsembleStatistics.t and EventTimes.t are the query axis, and t_peak
    under axis="T" is the peak temperature. axis="T" is the member's own temperature programme at its saved times (the values
    sol_vcs["T"] holds; for discrete-update sets the set's profile interpolated the same way), "t" the save grid, "t_rel" the
    time over the member's last saved time, an array [n_rows] or [K][n_rows] anything else. The axis must not decrease: a
    cooling programme is a ValueError - negate the axis and the queries. Every member's sol.resampled refers to ONE shared
    ResampledEnsemble (its u the resampled block when trajectories=True, else None). A malformed dict raises ValueError
    before anything touches the GPU (an axis array's row count is compared with the save grid once that is known). None (the
    default): the function as it was.

    observables=an ObservableSpec or the mapping `observables()` takes (species by name or 0-based id of the network as it is
    solved) turns the stored ensemble into observables - mole fractions, lumped classes, ratios - before the statistics and the
    event times look at it. The order inside the call: the solve; whatever refers to the solve's own rows (the trajectory
    download, sol.umax, fluxes=True); resample= with store, if given; then ensemble_observables(store=True) - observable g takes
    column g of the record, the columns from G on are zeros; then statistics= and events= over that record, whose `species` now
    number the observables (ids below G; None: all G of them, and mean / var / min / max have G columns). A vector `level` of
    events still has one entry per column of the record, N of them, the first G for the observables. Every member's sol.observables refers to ONE shared Observables (its values
    [K][n_rows][G] when trajectories=True, else None). A malformed argument - an unknown species, more observables than species -
    raises ValueError before anything touches the GPU. None (the default): the function as it was."""
    methods = list(methods)
    if not methods:
        raise ValueError("solve_network_ensemble needs at least one method")
    stat_kw = _statistics_arguments(statistics, len(methods))
    ev_kw = None if events is None else _event_arguments(events)
    rs_kw = None if resample is None else _resample_arguments(resample, len(methods))
    if rs_kw is not None and ev_kw is not None and not np.all(np.diff(rs_kw["at"], axis=-1) > 0):
        raise ValueError("resample: events over the resampled record need queries `at` that increase strictly")
    if observables is not None and not isinstance(observables, (ObservableSpec, Mapping)):
        raise ValueError("observables must be None, an ObservableSpec or the mapping observables() takes")
    m0 = methods[0]
    for m in methods:
        if not isinstance(m, VariableODESolve) or not isinstance(m.calculator, PrecalculatedArrheniusCalculator):
            raise ValueError("solve_network_ensemble takes VariableODESolves with the Arrhenius calculator; for static solves or "
                             "other calculators use HipNetwork.solve_ensemble (kin_solve_ensemble) or solve_network")
        if m.conditions.discrete_updates != m0.conditions.discrete_updates:
            raise ValueError("the methods of an ensemble must all have continuous or all discrete-update condition sets (one "
                             "kin_solve_ensemble_continuous / _discrete call); solve the others with HipNetwork.solve_ensemble "
                             "(kin_solve_ensemble) or solve_network")
        if m.pars.explicit:
            raise ValueError("solver='RK45' is not available with continuous rate updates; use the default BDF"
                             if not m.conditions.discrete_updates else
                             "solver='RK45' is not available in an ensemble (BDF only); use the default BDF or solve_network")
        why = _calculator_mismatch(m.calculator, m0.calculator)
        if why is not None:
            raise ValueError(f"the calculators of an ensemble's methods may differ in the values of Ea / A only ({why} differs: the "
                             "handle has one k_max, one t_mult and one network for all members)")
        if not member_calculators and not _same_calculator(m.calculator, m0.calculator):
            raise ValueError("the methods of an ensemble must share the calculator; pass member_calculators=True to solve every "
                             "member with the Ea / A of its own calculator")
        if not _same_filter(m.filter, m0.filter):
            raise ValueError("the methods of an ensemble must share the filter")
        for f in dataclasses.fields(ODESimulationParams):
            if f.name != "u0" and getattr(m.pars, f.name) != getattr(m0.pars, f.name):
                raise ValueError(f"the methods of an ensemble must share every ODESimulationParams field except u0 ({f.name} differs)")
    discrete = m0.conditions.discrete_updates
    pars, calc = m0.pars, m0.calculator
    # calculators that differ in value: every member's own (Ea, A) goes to the call; all equal: the call as it always was
    per_member = member_calculators and not all(_same_calculator(m.calculator, calc) for m in methods)
    sd_a, rd_a = (copy.deepcopy(sd), copy.deepcopy(rd)) if copy_network else (sd, rd)
    for m in methods:
        solve_variable_conditions(m.conditions, m.pars)
    mask = get_filter_mask(m0.filter, sd_a, rd_a)
    rd_a.splice(np.nonzero(mask)[0])
    setup_network(sd_a, rd_a, calc)
    rids = apply_ensemble_low_k_cutoff(rd_a, calc, pars, [m.conditions for m in methods],
                                       calculators=[m.calculator for m in methods] if per_member else None)
    # members may carry distinct (equal) calculator objects: each is spliced, as its own solve_network would splice it
    spliced = [calc]
    for m in methods:
        if not any(m.calculator is c for c in spliced):
            m.calculator.splice(rids)
            spliced.append(m.calculator)
    U0 = np.array([make_u0(sd_a, m.pars) for m in methods])
    ob_spec = None if observables is None else _observable_spec(sd_a, observables, store=True)
    # the columns the statistics and the event times can select: the species, or the observables that take their place
    n_cols, cols = (sd_a.n, f"{sd_a.n} species of the network as it is solved") if ob_spec is None else (ob_spec.G, f"{ob_spec.G} observables")
    stat_kw, ev_kw = _select_observables(stat_kw, ob_spec), _select_observables(ev_kw, ob_spec)
    if stat_kw is not None and stat_kw["species"] is not None and stat_kw["species"].max(initial=-1) >= n_cols:
        raise ValueError(f"statistics: species ids must be below the {cols}")
    sob_kw = None if stat_kw is None else stat_kw.get("sobol")
    sob_kw = _select_observables(sob_kw, ob_spec)
    if sob_kw is not None and sob_kw["species"] is not None and sob_kw["species"].max(initial=-1) >= n_cols:
        raise ValueError(f"statistics: sobol species ids must be below the {cols}")
    if ev_kw is not None:
        if ev_kw["species"] is not None and ev_kw["species"].max(initial=-1) >= n_cols:
            raise ValueError(f"events: species ids must be below the {cols}")
        if np.ndim(ev_kw["level"]) == 1 and len(ev_kw["level"]) != sd_a.n:
            raise ValueError(f"events: level must be a number or one per species of the network as it is solved ({sd_a.n})")
    if discrete:
        # each member's (tstops, T(tstops)), as solve_network hands them to kin_solve
        stops = [discrete_stop_temperatures(m.conditions) for m in methods]
    else:
        nodes = []
        for m in methods:
            prof = m.conditions.profiles[m.conditions.symbols.index("T")]
            if isstatic(prof):
                nodes.append((np.array([pars.tspan[0], pars.tspan[1]]), np.array([prof.value, prof.value], dtype=float)))
            else:
                nodes.append((np.asarray(prof.sol.t, dtype=float), np.asarray(prof.sol.u, dtype=float)))
    if rs_kw is not None and isinstance(rs_kw["axis"], str) and rs_kw["axis"] == "T":
        for m in methods:
            prof = m.conditions.profiles[m.conditions.symbols.index("T")]
            if not isstatic(prof) and np.any(np.diff(np.asarray(prof.sol.u, dtype=float)) < 0):
                raise ValueError("resample: axis='T' needs temperature programmes that do not decrease; for a cooling programme "
                                 "negate the axis and the queries (axis=-T as an array, at=-at)")
    h = capi.HipNetwork(*rd_a.flat(sd_a.n), index_base=1)
    try:
        h.set_arrhenius(calc.Ea, calc.A, calc.k_max, calc.t_mult)
        kw = {} if trajectories else dict(trajectories=False)   # (the defaults: the call as it always was)
        if per_member:      # gathered after splicing: row i is member i's calculator as the network is solved
            kw.update(Ea=np.array([m.calculator.Ea for m in methods]), A=np.array([m.calculator.A for m in methods]))
        if discrete:
            t, u, ns, rcs, sts = h.solve_ensemble_discrete(pars.to_kin_params(), U0, stops, **kw)
        else:
            t, u, ns, rcs, sts = h.solve_ensemble_continuous(pars.to_kin_params(), U0, nodes, **kw)
        dev_umax = None if trajectories else h.ensemble_max()
        F = None
        if fluxes:
            src = ensemble_flux_sources("discrete_members", t, ns, stops=stops) if discrete else \
                ensemble_flux_sources("continuous", t, ns, nodes=nodes)
            F = h.ensemble_flux(w=src["w"], T_rows=src["T_rows"])
        rs, t_stat = None, t
        if rs_kw is not None:      # from here on the stored ensemble is the resampled one and its rows are the queries
            axis = rs_kw["axis"]
            if isinstance(axis, str) and axis == "T":
                axis = np.array([_member_temperatures(m.conditions, t) for m in methods])
            rs = resample_ensemble(h, t, rs_kw["at"], axis=axis, mode=rs_kw["mode"], fill=rs_kw["fill"], t_min=rs_kw["t_min"],
                                   store=True, download=trajectories)
            rs.axis = rs_kw["axis"]
            t_stat = rs_kw["at"]
        ob = None
        if ob_spec is not None:      # from here on the columns of the stored ensemble are the observables
            ob = ensemble_observables(h, ob_spec, store=True, download=trajectories)
        stats = None
        if stat_kw is not None:
            sp0 = stat_kw["species"]
            if sob_kw is not None:
                sb0 = sob_kw["species"]
                sob_kw = dict(sob_kw, species=None if sb0 is None else sb0 + 1)
            stats = ensemble_statistics(h, t_stat, **dict(stat_kw, species=None if sp0 is None else sp0 + 1, sobol=sob_kw))   # (the handle's base is 1)
            stats.species = sp0
            if ob_spec is not None:      # (the moments have no selection of their own: their first G columns are the observables)
                for name in ("mean", "var", "min", "max"):
                    setattr(stats, name, np.ascontiguousarray(getattr(stats, name)[:, :ob_spec.G]))
            if sob_kw is not None:
                stats.sobol.species = sb0
        ev = None
        if ev_kw is not None:
            ev0 = ev_kw["species"]
            ev = event_times(h, t=t_stat, **dict(ev_kw, species=None if ev0 is None else ev0 + 1))
            ev.species = ev0
    finally:
        h.close()
    out = []
    for i, m in enumerate(methods):
        n_i = int(ns[i])
        ti, ui = t[:n_i].copy(), (u[i, :n_i].copy() if trajectories else None)
        if discrete:
            sol_vcs = None
            sol_k = ArrheniusRates(stops[i][0], stops[i][1], m.calculator.Ea, m.calculator.A, m.calculator.k_max, m.calculator.t_mult)
        else:
            sol_vcs = {sym: np.interp(ti, prof.sol.t, prof.sol.u) for sym, prof in zip(m.conditions.symbols, m.conditions.profiles)
                       if not isstatic(prof)}
            sol_k = None
        st = sts[i]
        if m.pars.update_tols and st["final_abstol"] != m.pars.abstol:
            m.pars.abstol, m.pars.reltol = st["final_abstol"], st["final_reltol"]   # solve_utils.jl:397-401
        if trajectories:
            umax = ui.max(axis=0) if n_i else np.zeros(sd_a.n)
        else:
            umax = dev_umax[i]
        fl = None if F is None else ReactionFluxes.from_flux(F[i], rd_a, sd_a.n, src["w"][i, :n_i])
        sol = ODESolution(ti, ui, capi.RETCODE_NAMES[int(rcs[i])], k=sol_k, stats=st, umax=umax, fluxes=fl)
        if stat_kw is not None:
            sol.ensemble_stats = stats
        sol.events = ev
        sol.resampled = rs
        sol.observables = ob
        out.append(ODESolveOutput(sd_a, rd_a, sol, sol_k, sol_vcs, m.pars, m.conditions))
    return out


# ---- statistics across the members of an ensemble (EXTENSION) -------------------------------------------------------------
@dataclass
class EnsembleStatistics:
    """Result of ensemble_statistics: what the members of an ensemble say together. Over the n = count participants, per row j
    of the save grid t and species i: mean, var (unbiased), min, max [n_rows][N]; quantiles[Q][n_rows][n_sel] at the
    probabilities p[Q] for the selected `species` (None: all; ids as the caller gave them); corr[n_rows][n_sel][P], the
    correlation of each sampled input with each selected species - Spearman's coefficient when `rank`, else Pearson's - or
    None when no inputs were given (include/kinetica_hip.h has every definition)."""
    t: np.ndarray
    count: int
    mean: np.ndarray
    var: np.ndarray
    min: np.ndarray
    max: np.ndarray
    quantiles: Optional[np.ndarray] = None
    p: Optional[np.ndarray] = None
    species: Optional[np.ndarray] = None
    corr: Optional[np.ndarray] = None
    rank: bool = True
    # the design's SobolIndices (ensemble_statistics(sobol=...)), else None: a plain attribute set after construction, not a
    # dataclass field - the constructor and dataclasses.fields() stay as they were
    sobol = None

    @property
    def std(self):
        return np.sqrt(self.var)

    def envelope(self, lo=0.05, hi=0.95):
        """(quantiles at lo, at hi), both [n_rows][n_sel]; the probabilities must be among p (ValueError otherwise)."""
        out = []
        for q in (lo, hi):
            at = np.nonzero(self.p == q)[0] if self.p is not None else []
            if len(at) == 0:
                raise ValueError(f"probability {q} is not among the computed quantiles {None if self.p is None else list(self.p)}")
            out.append(self.quantiles[at[0]])
        return tuple(out)


def _statistics_arguments(statistics, K):
    """solve_network_ensemble's `statistics` as keyword arguments of ensemble_statistics (None: no statistics); ValueError for
    anything malformed - nothing here touches the device."""
    if statistics is None or statistics is False:
        return None
    if statistics is True:
        statistics = {}
    if not isinstance(statistics, dict):
        raise ValueError("statistics must be None, True or a dict of ensemble_statistics' keyword arguments")
    known = ("quantiles", "species", "inputs", "rank", "use", "sobol", "of", "events")
    bad = [k for k in statistics if k not in known]
    if bad:
        raise ValueError(f"statistics: unknown keys {bad}; choose among {known}")
    kw = dict(quantiles=(0.05, 0.5, 0.95), species=None, inputs=None, rank=True, use=None)
    kw.update(statistics)
    ev = _of_arguments("statistics", kw.pop("of", "states"), kw.pop("events", None), ("states", "t_peak", "t_cross"))
    if ev is not None:      # (of="states", the default: the keywords as they always were)
        kw.update(of=statistics["of"], events=ev)
    if kw.get("sobol") is not None:
        kw["sobol"] = _sobol_arguments(kw["sobol"], K)
    else:
        kw.pop("sobol", None)
    try:
        q = np.atleast_1d(np.asarray(() if kw["quantiles"] is None else kw["quantiles"], dtype=float))
    except (TypeError, ValueError):
        raise ValueError("statistics: quantiles must be numbers in [0, 1]") from None
    if q.ndim != 1 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("statistics: quantiles must be numbers in [0, 1]")
    kw["quantiles"] = q
    if kw["species"] is not None:
        sp = np.asarray(kw["species"])
        if sp.ndim != 1 or sp.dtype.kind not in "iu" or (sp < 0).any():
            raise ValueError("statistics: species must be a list of 0-based integer ids")
        kw["species"] = sp.astype(np.int64)
    if kw["inputs"] is not None:
        try:
            X = np.asarray(kw["inputs"], dtype=float)
        except (TypeError, ValueError):
            raise ValueError("statistics: inputs must be a [K][P] array of numbers") from None
        if X.ndim != 2 or X.shape[0] != K:
            raise ValueError(f"statistics: inputs must be [K][P] with one row per method ({K}); got {X.shape}")
        kw["inputs"] = X
    if kw["use"] is not None:
        use = np.asarray(kw["use"])
        if use.shape != (K,):
            raise ValueError(f"statistics: use must have one entry per method ({K})")
    kw["rank"] = bool(kw["rank"])
    return kw


def ensemble_statistics(h, t, quantiles=(0.05, 0.5, 0.95), species=None, inputs=None, rank=True, use=None, sobol=None, of="states",
                        events=None):
    """Statistics across the members of the ensemble stored in the handle `h` (a capi.HipNetwork after a solve_ensemble* call,
    trajectories downloaded or not), read where the states live on the device: kin_ensemble_moments, kin_ensemble_quantiles
    (quantiles: probabilities in [0, 1]; None or empty: none) and, with inputs[K][P] (one row per member: whatever was sampled -
    log-multipliers of rate constants, temperatures, heating rates, u0 entries), kin_ensemble_correlate. species: ids in the
    handle's index base, None for all. use: a mask over the members, None for those that completed the save grid `t`.
    sobol: a dict of sobol_indices' keyword arguments (M, P, ...) when the ensemble is a Saltelli design; fills `.sobol`.
    of="t_peak" | "t_cross" with events=dict of event_times' keyword arguments (no species: `species` selects): the statistics
    of that event time over the members instead of the states - the [K][1][N] array of kin_ensemble_events handed to
    kin_members_moments / _quantiles / _correlate, every result with one row; `never` entries go into them as they are, so a
    species some participant never crosses takes whatever the statistic does with that value (NaN spreads; a censoring
    value counts as a time)."""
    events = _of_arguments("ensemble_statistics", of, events, ("states", "t_peak", "t_cross"))
    p = np.atleast_1d(np.asarray(() if quantiles is None else quantiles, dtype=float))
    sp = None if species is None else np.asarray(species, dtype=np.int64)
    if of == "states":
        m = h.ensemble_moments(use=use)
        qv = h.ensemble_quantiles(p, species=sp, use=use) if len(p) else None
        corr = None if inputs is None else h.ensemble_correlate(inputs, species=sp, rank=rank, use=use)
    else:
        arr = _event_block(h, t, of, events)
        if use is None:      # (the stored forms' default: the members that completed the save grid)
            _, rows, _, n_saved = h.ensemble_size()
            use = n_saved == rows
        m = h.members_moments(arr, use=use)
        qv = h.members_quantiles(arr, p, species=sp, use=use) if len(p) else None
        corr = None if inputs is None else h.members_correlate(arr, inputs, species=sp, rank=rank, use=use)
    sob = None if sobol is None else sobol_indices(h, t, **sobol)
    st = EnsembleStatistics(np.asarray(t, dtype=float), m["count"], m["mean"], m["var"], m["min"], m["max"], quantiles=qv,
                            p=p if len(p) else None, species=sp, corr=corr, rank=bool(rank))
    st.sobol = sob
    return st


# ---- variance-based sensitivity: Sobol indices of a Saltelli design (EXTENSION) ---------------------------------------------
def sobol_design(M, P, seed=0, A=None, B=None):
    """The Saltelli design X[M (P + 2)][P] on the unit cube in the layout of kin_members_sobol / kin_ensemble_sobol: row
    b M + m is sample m of block b; block 0 is A, block 1 is B, block 2 + p is A with column p taken from B. Without A / B the
    base samples are A = rng.random((M, P)) and then B = rng.random((M, P)) of np.random.default_rng(seed); a caller with a
    sampler of their own (Latin hypercube, a low-discrepancy sequence) passes both as [M][P] arrays.

    Building the ensemble from it: map every column to its parameter with any per-column transform - a log-multiplier
    k[:, r] = k0[r] * exp(s * (X[:, p] - 0.5)), a temperature T = T_lo + (T_hi - T_lo) * X[:, p], a heating rate - and give the
    K rows to the ensemble call IN THIS ORDER: k[K][R] (and T[K]) to HipNetwork.solve_ensemble, or one VariableODESolve per
    row to solve_network_ensemble(methods, ..., statistics=dict(sobol=dict(M=M, P=P))). A design over RATE PARAMETERS under a
    temperature programme - barriers off by a few kJ/mol, prefactors by an order of magnitude - goes through
    sample_arrhenius(calc, X, spec): one calculator per row, one VariableODESolve each, one ensemble call
    (solve_network_ensemble(..., member_calculators=True))."""
    if int(M) != M or int(P) != P or M < 1 or P < 1:
        raise ValueError(f"sobol_design: M and P must be integers >= 1; got {M!r}, {P!r}")
    M, P = int(M), int(P)
    if (A is None) != (B is None):
        raise ValueError("sobol_design: give both A and B or neither")
    if A is None:
        rng = np.random.default_rng(seed)
        A = rng.random((M, P))
        B = rng.random((M, P))
    else:
        A, B = np.asarray(A, dtype=float), np.asarray(B, dtype=float)
        if A.shape != (M, P) or B.shape != (M, P):
            raise ValueError(f"sobol_design: A and B must be [M = {M}][P = {P}]; got {A.shape} and {B.shape}")
    X = np.empty((M * (P + 2), P))
    X[:M], X[M:2 * M] = A, B
    for p in range(P):
        blk = X[(2 + p) * M:(3 + p) * M]
        blk[:] = A
        blk[:, p] = B[:, p]
    return X


def sample_arrhenius(calc, X, spec):
    """K PrecalculatedArrheniusCalculators from samples X[K][P] on the unit cube, one per row, for solve_network_ensemble (a
    Saltelli design from sobol_design, or any other sample). spec[p] = (kind, reaction_ids, half_width) says what column p
    moves: kind "Ea" shifts the barriers of the listed reactions by half_width (2 x - 1) (the units of calc.Ea), kind "lnA"
    multiplies their prefactors by exp(half_width (2 x - 1)); x = 0.5 leaves them as they are. reaction_ids are 0-based
    positions in calc.Ea / calc.A - the reactions of `rd` as it is passed to solve_network_ensemble(member_calculators=True),
    before filter and cutoff -
    and may be empty (a dummy input: its indices measure the estimator's noise). A reaction listed under several columns
    gets every shift. `calc` is not modified; k_max and t_unit are its own."""
    if not isinstance(calc, PrecalculatedArrheniusCalculator):
        raise ValueError("sample_arrhenius needs a PrecalculatedArrheniusCalculator")
    X = np.asarray(X, dtype=float)
    if X.ndim != 2 or X.shape[1] != len(spec):
        raise ValueError(f"sample_arrhenius: X must be [K][P] with P = len(spec) = {len(spec)}; got {X.shape}")
    if not np.all((X >= 0.0) & (X <= 1.0)):
        raise ValueError("sample_arrhenius: X must lie on the unit cube")
    R = len(calc.Ea)
    cols = []
    for p, item in enumerate(spec):
        try:
            kind, ids, hw = item
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            hw = float(hw)
        except (TypeError, ValueError):
            raise ValueError(f"sample_arrhenius: spec[{p}] must be (kind, reaction_ids, half_width)") from None
        if kind not in ("Ea", "lnA"):
            raise ValueError(f"sample_arrhenius: spec[{p}]: kind must be 'Ea' or 'lnA', got {kind!r}")
        if len(ids) and (ids.min() < 0 or ids.max() >= R):
            raise ValueError(f"sample_arrhenius: spec[{p}]: reaction ids must be in [0, {R})")
        cols.append((kind, ids, hw))
    out = []
    for x in X:
        Ea, A = calc.Ea.copy(), calc.A.copy()
        for (kind, ids, hw), xp in zip(cols, x):
            s = hw * (2.0 * xp - 1.0)
            for r in ids:      # (one by one: an id listed twice is shifted twice)
                if kind == "Ea":
                    Ea[r] += s
                else:
                    A[r] *= np.exp(s)
        out.append(PrecalculatedArrheniusCalculator(Ea, A, k_max=calc.k_max, t_unit=calc.t_unit))
    return out


@dataclass
class SobolIndices:
    """Result of sobol_indices. Over the n = count base samples (sum of the weights), per row j of `t` (one row for of="max")
    and selected species: first[n_rows][n_sel][P] the first-order index S1 of every input, total[n_rows][n_sel][P] the
    total-effect index ST, mean and var [n_rows][n_sel] over the design's blocks A and B (include/kinetica_hip.h has the
    estimators). first_ci / total_ci [2][n_rows][n_sel][P]: bootstrap percentile interval (lower, upper), or None."""
    t: np.ndarray
    count: int
    first: np.ndarray
    total: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    species: Optional[np.ndarray] = None
    first_ci: Optional[np.ndarray] = None
    total_ci: Optional[np.ndarray] = None

    def ranking(self, row=-1, species=None):
        """The inputs ordered by their total-effect index at `row`, the most influential first (ties and NaN keep the inputs'
        order, NaN last). species: one of the selected ids (as the caller gave them), or None for the mean over the selected
        species that have a value."""
        st = self.total[row]
        if species is None:
            with np.errstate(all="ignore"):
                ok = ~np.isnan(st)
                v = np.where(ok.any(axis=0), np.where(ok, st, 0.0).sum(axis=0) / np.maximum(ok.sum(axis=0), 1), np.nan)
        else:
            ids = np.arange(st.shape[0]) if self.species is None else np.asarray(self.species)
            at = np.nonzero(ids == species)[0]
            if len(at) == 0:
                raise ValueError(f"species {species} is not among the selected species")
            v = st[at[0]]
        return np.argsort(np.where(np.isnan(v), -np.inf, v) * -1.0, kind="stable")


_SOBOL_KEYS = ("M", "P", "species", "w", "of", "n_boot", "seed", "level", "events")
_SOBOL_OF = ("states", "max", "t_peak", "t_cross")


def _sobol_arguments(sobol, K):
    """The `sobol` entry of solve_network_ensemble's statistics as keyword arguments of sobol_indices; ValueError for anything
    malformed, a design that does not match the K methods included - nothing here touches the device."""
    if not isinstance(sobol, dict):
        raise ValueError("statistics: sobol must be a dict of sobol_indices' keyword arguments (M, P, ...)")
    bad = [k for k in sobol if k not in _SOBOL_KEYS]
    if bad:
        raise ValueError(f"statistics: unknown sobol keys {bad}; choose among {_SOBOL_KEYS}")
    kw = dict(species=None, w=None, of="states", n_boot=0, seed=0, level=0.95)
    kw.update(sobol)
    ev = _of_arguments("statistics: sobol", kw["of"], kw.pop("events", None), _SOBOL_OF)
    if ev is not None:      # (an event time's indices: the one case with this key)
        kw["events"] = ev
    for name in ("M", "P"):
        v = kw.get(name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"statistics: sobol needs an integer {name} >= 1")
        kw[name] = int(v)
    if kw["M"] * (kw["P"] + 2) != K:
        raise ValueError(f"statistics: a sobol design with M = {kw['M']}, P = {kw['P']} has {kw['M'] * (kw['P'] + 2)} members; "
                         f"there are {K} methods")
    if kw["species"] is not None:
        sp = np.asarray(kw["species"])
        if sp.ndim != 1 or sp.dtype.kind not in "iu" or (sp < 0).any():
            raise ValueError("statistics: sobol species must be a list of 0-based integer ids")
        kw["species"] = sp.astype(np.int64)
    if kw["w"] is not None:
        w = np.asarray(kw["w"])
        if w.shape != (kw["M"],) or w.dtype.kind not in "iu" or (w < 0).any():
            raise ValueError(f"statistics: sobol w must be {kw['M']} integer multiplicities >= 0")
        kw["w"] = w.astype(np.int32)
    nb = kw["n_boot"]
    if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or nb < 0:
        raise ValueError("statistics: sobol n_boot must be an integer >= 0")
    kw["n_boot"] = int(nb)
    if not isinstance(kw["level"], (int, float)) or not 0.0 < kw["level"] < 1.0:
        raise ValueError("statistics: sobol level must lie in (0, 1)")
    return kw


def sobol_indices(h, t, M, P, species=None, w=None, of="states", n_boot=0, seed=0, level=0.95, events=None):
    """First-order and total-effect Sobol indices of the Saltelli design stored in the handle `h` (a capi.HipNetwork after a
    solve_ensemble* call over the K = M (P + 2) members of sobol_design, trajectories downloaded or not), read where the states
    live on the device (kin_ensemble_sobol). species: ids in the handle's index base, None for all. w: int multiplicities per
    base sample, None for 1 where all P + 2 members of a sample completed the save grid `t`, else 0.
    of="states": the indices of every species at every saved time; of="max": of every species' peak value over a member's own
    rows (kin_ensemble_max's [K][N] handed to kin_members_sobol as one row; `t` is kept as given); of="t_peak" | "t_cross" with
    events=dict of event_times' keyword arguments (no species: `species` selects): of that event time of every species -
    which input controls an induction time or a half-life - kin_ensemble_events' [K][N] handed over the same way (`never`
    entries of participating members go into the sums as they are).
    n_boot > 0: bootstrap percentile intervals at `level` - n_boot replicates, each the multinomial multiplicities of
    resampling the participants with replacement (np.random.default_rng(seed)), one device pass per replicate."""
    events = _of_arguments("sobol_indices", of, events, _SOBOL_OF)
    if of != "states":
        umax = h.ensemble_max()[:, None, :] if of == "max" else _event_block(h, t, of, events)
        base = h.ensemble_sobol_weights(M, P) if w is None else np.asarray(w)
        run = lambda wt: h.members_sobol(umax, M, P, species=species, w=wt)
        r = run(base)      # (a failed member's peak is no peak: its sample is dropped here as over the states)
    else:
        base = h.ensemble_sobol_weights(M, P) if w is None else np.asarray(w)
        run = lambda wt: h.ensemble_sobol(M, P, species=species, w=wt)
        r = run(w)
    ci = [None, None]
    if n_boot > 0:
        rng = np.random.default_rng(seed)
        at = np.flatnonzero(base > 0)
        prob = base[at] / base[at].sum() if len(at) else None
        reps = ([], [])
        for _ in range(int(n_boot)):
            wt = np.zeros(int(M), np.int32)
            if len(at):
                wt[at] = rng.multinomial(int(base[at].sum()), prob)
            b = run(wt)
            reps[0].append(b["first"]); reps[1].append(b["total"])
        q = [(1.0 - level) / 2.0, (1.0 + level) / 2.0]
        with np.errstate(all="ignore"):
            ci = [np.quantile(np.stack(x), q, axis=0) for x in reps]
    sp = None if species is None else np.asarray(species, dtype=np.int64)
    return SobolIndices(np.asarray(t, dtype=float), r["count"], r["first"], r["total"], r["mean"], r["var"], species=sp,
                        first_ci=ci[0], total_ci=ci[1])


# ---- event times: when a species peaks and when it crosses a level (EXTENSION) ------------------------------------------------
@dataclass
class EventTimes:
    """Result of event_times. Per segment - the members of an ensemble, [K][n_sel], or the one trajectory of a solve, [n_sel] -
    and selected species (`species` as the caller gave them; None: all): u_peak the maximum over the rows that take part,
    t_peak the time of the first row that holds it, t_cross the time at which the species first reaches the level, by the
    chord between the two saved rows around the crossing (None when no level was given); `never` where there is no such time
    (include/kinetica_hip.h has the definitions). t: the saved times; the other fields are the request."""
    t: np.ndarray
    u_peak: np.ndarray
    t_peak: np.ndarray
    t_cross: Optional[np.ndarray]
    level: Optional[np.ndarray] = None
    kind: str = "abs"
    direction: str = "rise"
    start: str = "begin"
    t_min: Optional[float] = None
    never: float = float("nan")
    species: Optional[np.ndarray] = None


_EVENT_KEYS = ("level", "kind", "direction", "start", "t_min", "never", "species")


def _event_arguments(events, what="events"):
    """A dict of event_times' keyword arguments, completed with the defaults; ValueError for anything malformed - nothing here
    touches the device. level comes back None, a float or a float array [N]; species None or int64 ids."""
    if not isinstance(events, dict):
        raise ValueError(f"{what} must be a dict of event_times' keyword arguments {_EVENT_KEYS}")
    bad = [k for k in events if k not in _EVENT_KEYS]
    if bad:
        raise ValueError(f"{what}: unknown keys {bad}; choose among {_EVENT_KEYS}")
    kw = dict(level=None, kind="abs", direction="rise", start="begin", t_min=None, never=float("nan"), species=None)
    kw.update(events)
    if kw["level"] is not None:
        try:
            lv = np.asarray(kw["level"], dtype=float)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: level must be a number or one number per species") from None
        if lv.ndim > 1 or isinstance(kw["level"], (bool, np.bool_)):
            raise ValueError(f"{what}: level must be a number or one number per species")
        kw["level"] = float(lv) if lv.ndim == 0 else lv
    for name, names in (("kind", capi.EVENT_KINDS), ("direction", capi.EVENT_DIRECTIONS), ("start", capi.EVENT_STARTS)):
        if not isinstance(kw[name], str) or kw[name] not in names:
            raise ValueError(f"{what}: {name} must be one of {tuple(names)}; got {kw[name]!r}")
    for name in ("t_min", "never"):
        v = kw[name]
        if v is None and name == "t_min":
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: {name} must be a number")
        kw[name] = float(v)
    if kw["t_min"] is not None and np.isnan(kw["t_min"]):
        raise ValueError(f"{what}: t_min must be a number")
    if kw["species"] is not None:
        sp = np.asarray(kw["species"])
        if sp.ndim != 1 or sp.dtype.kind not in "iu" or (sp < 0).any():
            raise ValueError(f"{what}: species must be a list of non-negative integer ids")
        kw["species"] = sp.astype(np.int64)
    return kw


def _of_arguments(what, of, events, choices):
    """The (of, events) pair of ensemble_statistics / sobol_indices: `of` among `choices`; of="t_peak" | "t_cross" needs
    events=dict(...) without species (and with a level for t_cross), the others take none. Returns the completed dict or None."""
    if of not in choices:
        raise ValueError(f"{what}: of must be one of {choices}; got {of!r}")
    if of not in ("t_peak", "t_cross"):
        if events is not None:
            raise ValueError(f"{what}: events goes with of='t_peak' or of='t_cross', not of={of!r}")
        return None
    kw = _event_arguments({} if events is None else events, what=f"{what}: events")
    if kw["species"] is not None:
        raise ValueError(f"{what}: events takes no species here; the species are selected beside `of`")
    if of == "t_cross" and kw["level"] is None:
        raise ValueError(f"{what}: of='t_cross' needs events=dict(level=...)")
    return kw


def _event_row_begin(t, t_min):
    """The first row of the increasing times t with t >= t_min (None: row 0)."""
    return 0 if t_min is None else int(np.searchsorted(np.asarray(t, dtype=float), float(t_min), side="left"))


def _event_block(h, t, of, events):
    """The event time `of` of every member and species of the handle's stored ensemble as the [K][1][N] block the
    kin_members_* entries take."""
    return np.ascontiguousarray(getattr(event_times(h, t=t, **events), of)[:, None, :])


def event_times(out_or_handle, level=None, kind="abs", direction="rise", start="begin", t_min=None, never=float("nan"), species=None,
                t=None):
    """When does every species peak, and when does it first cross a level - the induction time before a product reaches 10 % of
    its final value (level=0.1, kind="of_peak"), the half-life of the feed (level=0.5, kind="of_start", direction="fall"), the
    falling edge of a pulse at half of its maximum (level=0.5, kind="of_peak", direction="fall", start="peak"). One device pass
    (kin_events_segmented / kin_ensemble_events), no sum in it: the result is exact whatever the launch looks like.

    out_or_handle: an ODESolveOutput - its saved states are handed to a handle of out.rd as the other analysis passes hand them
    over, result arrays [n_sel] - or a capi.HipNetwork after a solve_ensemble* call (trajectories downloaded or not) with t=
    the save grid [n_rows] (or every member's own times [K][n_rows]): the stored ensemble is read where it lives, result arrays
    [K][n_sel], a member's rows past its n_saved taking no part.
    level: a number or one per species, None for the peaks alone (t_cross is None then); kind "abs" | "of_peak" | "of_start";
    direction "rise" | "fall"; start "begin" | "peak". t_min: only the rows with t >= t_min take part (turned into the pass's
    row_begin; with per-member times it is refused). never: what a time that does not exist is reported as - NaN, or e.g.
    t[-1] to censor. species: the columns returned - names or 0-based ids for an ODESolveOutput, ids in the handle's index base
    for a handle; None for all. Malformed arguments raise ValueError before anything touches the device."""
    is_out = isinstance(out_or_handle, ODESolveOutput)
    if is_out and species is not None:
        try:
            if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (str, int, np.integer)) for x in species):
                raise TypeError
            species = _species_ids(out_or_handle.sd, species)
        except (KeyError, TypeError, ValueError):
            raise ValueError("events: species must be names or 0-based ids of the solve's species") from None
    kw = _event_arguments(dict(level=level, kind=kind, direction=direction, start=start, t_min=t_min, never=never, species=species))
    opts = dict(level=kw["level"], kind=kw["kind"], direction=kw["direction"], start=kw["start"], never=kw["never"])
    cols = kw["species"]
    if is_out:
        out = out_or_handle
        if t is not None:
            raise ValueError("events: t goes with a handle's stored ensemble; an ODESolveOutput carries its own saved times")
        if out.sol.u is None:
            raise ValueError("events: the solve output holds no saved states (it was solved with trajectories=False)")
        n = out.sd.n
        ts = np.asarray(out.sol.t, dtype=float)
        u = np.ascontiguousarray(np.asarray(out.sol.u, dtype=float).reshape(1, len(ts), n))
    else:
        if t is None:
            raise ValueError("events: a handle needs t, the save grid of its stored ensemble")
        n = out_or_handle.n
        ts = np.asarray(t, dtype=float)
        if ts.ndim not in (1, 2):
            raise ValueError(f"events: t must be the save grid [n_rows] or every member's times [K][n_rows]; got {ts.shape}")
        if ts.ndim == 2 and kw["t_min"] is not None:
            raise ValueError("events: t_min needs one save grid for all members")
        cols = None if cols is None else cols - getattr(out_or_handle, "index_base", 0)
    if np.ndim(kw["level"]) == 1 and len(kw["level"]) != n:
        raise ValueError(f"events: level must be a number or one per species ({n}); got {len(kw['level'])}")
    if cols is not None and len(cols) and (cols.min() < 0 or cols.max() >= n):
        raise ValueError(f"events: species ids must be among the {n} species")
    row_begin = _event_row_begin(ts, kw["t_min"])
    if is_out:
        h = capi.HipNetwork(*out.rd.flat(n), index_base=1)
        try:
            r = h.events_segmented(u, ts, row_begin=row_begin, **opts)
        finally:
            h.close()
        r = {q: v[0] for q, v in r.items()}
    else:
        r = out_or_handle.ensemble_events(ts, row_begin=row_begin, **opts)
    if cols is not None:
        r = {q: np.ascontiguousarray(v[..., cols]) for q, v in r.items()}
    lv = None if kw["level"] is None else np.broadcast_to(np.asarray(kw["level"], dtype=float), (n,)).copy()
    return EventTimes(ts, r["u_peak"], r["t_peak"], r.get("t_cross"), level=lv, kind=kw["kind"], direction=kw["direction"],
                      start=kw["start"], t_min=kw["t_min"], never=kw["never"], species=kw["species"])


# ---- resampling: stored trajectories on a common axis (EXTENSION) -----------------------------------------------------------
@dataclass
class ResampledEnsemble:
    """Result of resample_ensemble / resample_solution: the stored trajectories at the queries `at` of the axis `axis`.
    axis: what the caller named ("t", "t_rel", "T") or gave; x: the axis as the pass read it, [n_rows] or [K][n_rows]; at: the
    queries [Q] or [K][Q]; u: the states at them [K][Q][N] ([Q][N] for one solve), None when not downloaded; jc[K][Q]: the row
    that closes the bracket of a query inside a member's range, -1 below it, -2 above it, -3 for a NaN query or a member
    without rows; covered[K][Q]: the query has a state (inside, or held under mode="hold"); n_covered[K]: the length of the
    leading run of covered queries - a member's n_saved in a stored resampled record (include/kinetica_hip.h has the
    definitions)."""
    axis: object
    at: np.ndarray
    u: Optional[np.ndarray]
    jc: np.ndarray
    covered: np.ndarray
    n_covered: np.ndarray
    x: Optional[np.ndarray] = None
    mode: str = "fill"
    fill: float = float("nan")
    t_min: Optional[float] = None


_RESAMPLE_KEYS = ("axis", "at", "mode", "fill", "t_min")
_RESAMPLE_AXES = ("T", "t", "t_rel")


def _resample_arguments(resample, K, what="resample", axes=_RESAMPLE_AXES):
    """A dict of resample_ensemble's keyword arguments, completed with the defaults; ValueError for anything malformed - nothing
    here touches the device. at comes back a float array [Q] or [K][Q], axis a name or a float array of 1 or 2 dimensions."""
    if not isinstance(resample, dict):
        raise ValueError(f"{what} must be a dict with the keys {_RESAMPLE_KEYS}")
    bad = [k for k in resample if k not in _RESAMPLE_KEYS]
    if bad:
        raise ValueError(f"{what}: unknown keys {bad}; choose among {_RESAMPLE_KEYS}")
    if "at" not in resample:
        raise ValueError(f"{what}: at, the queries, is missing")
    kw = dict(axis="t", mode="fill", fill=float("nan"), t_min=None)
    kw.update(resample)

    def numbers(v, name):
        try:
            a = np.asarray(v)
            if a.dtype.kind not in "iuf":
                raise TypeError
            if a.ndim == 0:      # (ascontiguousarray would make a number an array of one)
                raise TypeError
            return np.ascontiguousarray(a, dtype=float)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {name} must be an array of numbers") from None

    at = numbers(kw["at"], "at")
    if not (at.ndim == 1 or (at.ndim == 2 and at.shape[0] == K)):
        raise ValueError(f"{what}: at must be the queries [Q] or one set per member [{K}][Q]; got {at.shape}")
    kw["at"] = at
    if isinstance(kw["axis"], str):
        if kw["axis"] not in axes:
            raise ValueError(f"{what}: axis must be one of {axes} or an array; got {kw['axis']!r}")
    else:
        ax = numbers(kw["axis"], "axis")
        if not (ax.ndim == 1 or (ax.ndim == 2 and ax.shape[0] == K)):
            raise ValueError(f"{what}: an axis array must be [n_rows] or [{K}][n_rows]; got {ax.shape}")
        kw["axis"] = ax
    if not isinstance(kw["mode"], str) or kw["mode"] not in capi.RESAMPLE_MODES:
        raise ValueError(f"{what}: mode must be one of {tuple(capi.RESAMPLE_MODES)}; got {kw['mode']!r}")
    for name in ("fill", "t_min"):
        v = kw[name]
        if v is None and name == "t_min":
            continue
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: {name} must be a number")
        kw[name] = float(v)
    if kw["t_min"] is not None and np.isnan(kw["t_min"]):
        raise ValueError(f"{what}: t_min must be a number")
    return kw


def _member_temperatures(conditions, t):
    """A member's temperature programme at the save grid t: what sol_vcs["T"] holds at the member's saved times."""
    prof = conditions.profiles[conditions.symbols.index("T")]
    if isstatic(prof):
        return np.full(len(t), float(prof.value))
    return np.interp(t, prof.sol.t, prof.sol.u)


def _resample_axis(axis, t, K, n_saved, what="resample"):
    """The axis array [n_rows] or [K][n_rows] of a named or given axis over the save grid t; ValueError for a wrong shape or an
    axis that decreases over a member's saved rows."""
    L = len(t)
    if isinstance(axis, str):
        if axis == "t":
            x = np.asarray(t, dtype=float)
        elif axis == "t_rel":
            last = np.asarray(t, dtype=float)[np.maximum(np.asarray(n_saved) - 1, 0)]
            x = np.asarray(t, dtype=float)[None, :] / np.where(np.asarray(n_saved) > 0, last, 1.0)[:, None]
        else:
            raise ValueError(f"{what}: axis must be 't', 't_rel' or an array here; got {axis!r}")
    else:
        x = np.ascontiguousarray(axis, dtype=float)
    if x.shape not in ((L,), (K, L)):
        raise ValueError(f"{what}: the axis must be [{L}] or [{K}][{L}] (the save grid's rows); got {x.shape}")
    for m in range(K):
        rows = (x[m] if x.ndim == 2 else x)[:int(n_saved[m])]
        if np.any(np.diff(rows) < 0):
            raise ValueError(f"{what}: the axis decreases over member {m}'s saved rows; for a cooling programme negate the axis "
                             "and the queries")
    return np.ascontiguousarray(x)


def _covered(jc, mode):
    covered = (jc >= 0) | ((jc != capi.RESAMPLE_NONE) if mode == "hold" else False)
    n_cov = np.array([len(c) if c.all() else int(np.argmin(c)) for c in covered.reshape(-1, covered.shape[-1])], dtype=np.int64)
    return covered, n_cov


def resample_ensemble(h, t, at, axis="t", mode="fill", fill=float("nan"), t_min=None, store=True, download=False):
    """The ensemble stored in the handle `h` (a capi.HipNetwork after a solve_ensemble* call with the save grid `t`, trajectories
    downloaded or not) at the queries `at` ([Q], or [K][Q] one set per member) of a per-member axis, computed where the states
    live (kin_ensemble_resample): a saved row copied bit for bit where the axis holds the query, else the chord between the two
    rows around it. axis: "t" the save grid, "t_rel" t / t[n_saved[m] - 1], or an array [n_rows] / [K][n_rows] (e.g. every
    member's temperature at the saved times) that does not decrease over a member's saved rows. mode "fill": a query outside a
    member's range gets `fill`; "hold": the member's first / last row. t_min: only the rows with t >= t_min take part.
    store=True: the result becomes the stored ensemble - Q rows, a member's n_saved its n_covered - so that every ensemble_*
    method, ensemble_statistics, sobol_indices and event_times (with t=at) run on it. download: fill `.u`. Returns a
    ResampledEnsemble; its jc / covered / n_covered come from kin_resample_bracket_host."""
    K, L, _, n_saved = h.ensemble_size()
    kw = _resample_arguments(dict(at=at, axis=axis, mode=mode, fill=fill, t_min=t_min), K)
    t = np.asarray(t, dtype=float)
    if t.shape != (L,):
        raise ValueError(f"resample: t must be the save grid of the stored ensemble ({L} rows); got {t.shape}")
    x = _resample_axis(kw["axis"], t, K, n_saved)
    rb = _event_row_begin(t, kw["t_min"])
    jc, _ = capi.resample_brackets(x if x.ndim == 2 else np.broadcast_to(x, (K, L)), kw["at"], seg_n=n_saved, row_begin=rb)
    u = h.ensemble_resample(x, kw["at"], mode=kw["mode"], fill=kw["fill"], row_begin=rb, store=store, download=download or not store)
    covered, n_cov = _covered(jc, kw["mode"])
    return ResampledEnsemble(axis, kw["at"], u if download or not store else None, jc, covered, n_cov, x=x, mode=kw["mode"],
                             fill=kw["fill"], t_min=kw["t_min"])


def resample_solution(out_or_handle, at, axis=None, mode="fill", fill=float("nan"), t_min=None):
    """resample_ensemble for one solve: an ODESolveOutput - its saved states are handed to a handle of out.rd as the other
    analysis passes hand them over; axis None or "t" its saved times, "T" its sol_vcs["T"], or an array [n_saved] - or a
    capi.HipNetwork after a solve (kin_solution_resample, the states read where they live) with axis the array [n_saved] of its
    saved rows: the saved times, or anything else. Returns a ResampledEnsemble with u[Q][N], jc[Q], covered[Q] and n_covered a
    number."""
    is_out = isinstance(out_or_handle, ODESolveOutput)
    kw = _resample_arguments(dict(at=at, axis="t" if axis is None else axis, mode=mode, fill=fill, t_min=t_min), 1,
                             axes=("t", "T") if is_out else ("t",))
    if kw["at"].ndim != 1:
        raise ValueError("resample: one solve takes one set of queries [Q]")
    if is_out:
        out = out_or_handle
        if out.sol.u is None:
            raise ValueError("resample: the solve output holds no saved states (it was solved with trajectories=False)")
        ts = np.asarray(out.sol.t, dtype=float)
        x = kw["axis"]
        if isinstance(x, str) and x == "T":
            if not out.sol_vcs or "T" not in out.sol_vcs:
                raise ValueError("resample: axis='T' needs a solve with a temperature profile (sol_vcs['T'])")
            x = np.asarray(out.sol_vcs["T"], dtype=float)
        x = _resample_axis(x, ts, 1, [len(ts)])
        if x.ndim == 2:
            x = x[0]
        rb = _event_row_begin(ts, kw["t_min"])
        n = out.sd.n
        h = capi.HipNetwork(*out.rd.flat(n), index_base=1)
        try:
            u = h.resample_segmented(np.asarray(out.sol.u, dtype=float).reshape(1, len(ts), n), x, kw["at"], mode=kw["mode"],
                                     fill=kw["fill"], row_begin=rb)[0]
        finally:
            h.close()
    else:
        h = out_or_handle
        x = None if isinstance(kw["axis"], str) else np.ascontiguousarray(kw["axis"], dtype=float)
        if t_min is not None:
            raise ValueError("resample: t_min goes with an ODESolveOutput (a handle's saved times are not known here)")
        if x is None:
            raise ValueError("resample: a handle needs the axis array of its saved rows (its saved times, or anything else)")
        if x.ndim != 1 or np.any(np.diff(x) < 0):
            raise ValueError("resample: the axis must be [n_saved] and must not decrease; for a cooling programme negate the axis and the queries")
        rb = 0
        u = h.solution_resample(kw["at"], x=x, mode=kw["mode"], fill=kw["fill"])
    jc, _ = capi.resample_brackets(x, kw["at"], row_begin=rb)
    covered, n_cov = _covered(jc[0], kw["mode"])
    return ResampledEnsemble(axis, kw["at"], u, jc[0], covered, int(n_cov[0]), x=x, mode=kw["mode"], fill=kw["fill"], t_min=kw["t_min"])


# ---- observables: weighted species sums and ratios of stored states (EXTENSION) ---------------------------------------------
@dataclass
class ObservableSpec:
    """What observables() and mole_fractions() build: the names of the G observables, the H linear forms over the N species in
    CSR (form_ptr[H + 1], form_idx 0-based, form_w) and per observable the form num[g] and the form den[g] it is divided by, -1
    for none (include/kinetica_hip.h has the definitions)."""
    names: tuple
    N: int
    form_ptr: np.ndarray
    form_idx: np.ndarray
    form_w: np.ndarray
    num: np.ndarray
    den: np.ndarray

    @property
    def G(self):
        return len(self.num)

    @property
    def H(self):
        return len(self.form_ptr) - 1

    def arrays(self, index_base=0):
        """(form_ptr, form_idx, form_w, num, den) as the capi entries take them, the species in `index_base`."""
        return self.form_ptr, self.form_idx + int(index_base), self.form_w, self.num, self.den


@dataclass
class Observables:
    """Result of ensemble_observables / solution_observables: names[G]; values[K][n_rows][G] ([n_saved][G] for one solve), None
    when not downloaded; G; spec, the ObservableSpec they were computed from."""
    names: tuple
    values: Optional[np.ndarray]
    G: int
    spec: Optional[ObservableSpec] = None


def _observable_species(sd, N, x):
    """The 0-based id of a species given by name (with a SpeciesData) or by 0-based id; ValueError for anything else."""
    if isinstance(x, str):
        if sd is None or x not in sd.toInt:
            raise ValueError(f"observables: unknown species {x!r}")
        return sd.toInt[x] - 1
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < N:
        raise ValueError(f"observables: species must be names or 0-based ids below {N}; got {x!r}")
    return int(x)


def observables(sd_or_N, spec, store=False):
    """An ObservableSpec from a mapping name -> what the observable is: a species (name or 0-based id), a list of species (their
    sum, weights 1), a {species: weight} mapping (a weighted sum; a species may not repeat, a list may repeat one), or
    ("ratio", name_a, name_b), the quotient of two other entries of the mapping that are sums themselves. sd_or_N: the
    SpeciesData that resolves names, or the number of species (ids only). Every entry that is no ratio becomes one linear
    form, in the mapping's order; observable g is the mapping's g-th entry. store=True also asks for G <= N, what a stored
    record of observables needs. ValueError - nothing here touches the device - for an unknown species, an unknown or ratio
    name inside a ratio, an empty mapping or entry type, or G > N with store."""
    sd = sd_or_N if isinstance(sd_or_N, SpeciesData) else None
    if sd is None and (isinstance(sd_or_N, (bool, np.bool_)) or not isinstance(sd_or_N, (int, np.integer)) or sd_or_N < 1):
        raise ValueError("observables: the first argument must be a SpeciesData or the number of species")
    N = sd.n if sd is not None else int(sd_or_N)
    if not isinstance(spec, Mapping) or len(spec) == 0:
        raise ValueError("observables: the spec must be a non-empty mapping name -> species, list, {species: weight} or ('ratio', a, b)")
    ptr, idx, w, form_of = [0], [], [], {}
    for name, what in spec.items():
        if isinstance(what, tuple) and len(what) == 3 and what[0] == "ratio":
            continue
        if isinstance(what, Mapping):
            terms = [(_observable_species(sd, N, k), v) for k, v in what.items()]
        elif isinstance(what, (list, tuple, np.ndarray)):
            terms = [(_observable_species(sd, N, k), 1.0) for k in what]
        else:
            terms = [(_observable_species(sd, N, what), 1.0)]
        for i, v in terms:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"observables: the weights of {name!r} must be numbers")
            idx.append(i); w.append(float(v))
        form_of[name] = len(ptr) - 1
        ptr.append(len(idx))
    num, den = [], []
    for name, what in spec.items():
        if name in form_of:
            num.append(form_of[name]); den.append(-1)
            continue
        for operand in what[1:]:
            if operand not in form_of:
                raise ValueError(f"observables: the ratio {name!r} names {operand!r}, which is no sum of the spec")
        num.append(form_of[what[1]]); den.append(form_of[what[2]])
    if store and len(num) > N:
        raise ValueError(f"observables: a stored record holds at most as many observables as species ({N}); got {len(num)}")
    return ObservableSpec(tuple(spec), N, np.array(ptr, np.int64), np.array(idx, np.int64), np.array(w, float), np.array(num, np.int64),
                          np.array(den, np.int64))


def mole_fractions(sd_or_N, species=None):
    """The ObservableSpec of the mole fractions u_i / sum_k u_k of `species` (names or 0-based ids; None: all N): N singleton
    forms and the total over all species, H = N + 1; observable g is the g-th selected species over the total."""
    sd = sd_or_N if isinstance(sd_or_N, SpeciesData) else None
    if sd is None and (isinstance(sd_or_N, (bool, np.bool_)) or not isinstance(sd_or_N, (int, np.integer)) or sd_or_N < 1):
        raise ValueError("observables: the first argument must be a SpeciesData or the number of species")
    N = sd.n if sd is not None else int(sd_or_N)
    sel = list(range(N)) if species is None else [_observable_species(sd, N, x) for x in species]
    if not sel:
        raise ValueError("observables: mole fractions of no species")
    names = tuple(f"x[{sd.toStr[i + 1]}]" if sd is not None else f"x[{i}]" for i in sel)
    ptr = np.concatenate([np.arange(N + 1), [2 * N]]).astype(np.int64)
    idx = np.concatenate([np.arange(N), np.arange(N)]).astype(np.int64)
    return ObservableSpec(names, N, ptr, idx, np.ones(2 * N), np.array(sel, np.int64), np.full(len(sel), N, np.int64))


def _select_observables(kw, spec):
    """The keyword dict of a pass over a record of the observables `spec` (statistics, Sobol, events; None: no such pass, or no
    observables): without a selection of its own it selects the G observables, not the N - G zero columns behind them."""
    if kw is None or spec is None or kw["species"] is not None:
        return kw
    return dict(kw, species=np.arange(spec.G, dtype=np.int64))


def _observable_spec(sd_or_N, spec, store=False):
    """spec as an ObservableSpec for a network of sd_or_N species: one is checked against the network, a mapping built."""
    if isinstance(spec, ObservableSpec):
        N = sd_or_N.n if isinstance(sd_or_N, SpeciesData) else int(sd_or_N)
        if spec.N != N:
            raise ValueError(f"observables: the spec was built for {spec.N} species, the network has {N}")
        if store and spec.G > N:
            raise ValueError(f"observables: a stored record holds at most as many observables as species ({N}); got {spec.G}")
        return spec
    return observables(sd_or_N, spec, store=store)


def ensemble_observables(h, spec, store=False, download=True):
    """The observables `spec` (an ObservableSpec, or observables()' mapping with 0-based ids) of the ensemble stored in the handle
    `h` (a capi.HipNetwork after a solve_ensemble* call), computed where the states live (kin_ensemble_observables). store=True:
    the result becomes the stored ensemble - observable g in column g, zeros from column G on - so that ensemble_statistics,
    sobol_indices, event_times and resample_ensemble run on the observables; the passes that need species and reactions refuse
    such a record. Returns an Observables; values[K][n_rows][G], None with download=False (which needs store)."""
    spec = _observable_spec(h.n, spec, store=store)
    if not download and not store:
        raise ValueError("observables: download=False needs store=True: the result would go nowhere")
    v = h.ensemble_observables(*spec.arrays(h.index_base), pitch=h.n if store else spec.G, store=store, download=download)
    return Observables(spec.names, None if v is None else np.ascontiguousarray(v[:, :, :spec.G]), spec.G, spec)


def solution_observables(out_or_handle, spec):
    """ensemble_observables for one solve: an ODESolveOutput - its saved states are handed to a handle of out.rd as the other
    analysis passes hand them over, species by name or 0-based id - or a capi.HipNetwork after a solve (kin_solution_observables,
    the states read where they live). Returns an Observables with values[n_saved][G]."""
    if isinstance(out_or_handle, ODESolveOutput):
        out = out_or_handle
        spec = _observable_spec(out.sd, spec)
        if out.sol.u is None:
            raise ValueError("observables: the solve output holds no saved states (it was solved with trajectories=False)")
        n = out.sd.n
        u = np.ascontiguousarray(np.asarray(out.sol.u, dtype=float).reshape(1, -1, n))
        h = capi.HipNetwork(*out.rd.flat(n), index_base=1)
        try:
            v = h.observables_segmented(u, *spec.arrays(1))[0]
        finally:
            h.close()
    else:
        h = out_or_handle
        spec = _observable_spec(h.n, spec)
        v = h.solution_observables(*spec.arrays(h.index_base))
    return Observables(spec.names, v, spec.G, spec)


# ---- post-hoc reaction-flux analysis (EXTENSION, in the style of the reference's analysis/: works on an ODESolveOutput) ----
def flux_weights(t):
    """Trapezoid weights of the saved times t: sum_b w[b] f(t[b]) is the trapezoid rule for the integral of f over
    [t[0], t[-1]]; the weights sum to t[-1] - t[0]. One row gives [0.0]. t must be strictly increasing (ValueError)."""
    t = np.asarray(t, dtype=float).ravel()
    if len(t) == 0:
        raise ValueError("flux_weights needs at least one saved time")
    dt = np.diff(t)
    if np.any(dt <= 0):
        raise ValueError("saved times must be strictly increasing")
    w = np.zeros(len(t))
    w[:-1] += 0.5 * dt
    w[1:] += 0.5 * dt
    return w


def held_stop_index(t, tstops):
    """Index of the stop whose rate constants hold at each saved time under kin_solve's zero-order hold:
    searchsorted(tstops, t, side="right") - 1, clipped at 0 - a saved time equal to a stop takes that stop's rates, a time
    before the first stop the first stop's."""
    idx = np.searchsorted(np.asarray(tstops, dtype=float), np.asarray(t, dtype=float), side="right") - 1
    return np.clip(idx, 0, None).astype(np.int64)


def ensemble_flux_sources(kind, t, n_saved, T=None, tstops=None, T_stops=None, stops=None, nodes=None):
    """What kin_ensemble_flux needs per (member, row of the save grid) of an ensemble call, pure NumPy. t[M]: the call's save
    grid (its out_t), n_saved[K]: the members' saved rows. Returns dict(w=[K][M], and k_row=[K][M] (int64) or T_rows=[K][M]):
      w       flux_weights(t[:n_saved[m]]) in member m's first n_saved[m] entries, zeros beyond (no saved row: all zeros);
      the rate constants a member's solve held at each saved time, by `kind`:
        "static"            T=None: k_row = m (kin_solve_ensemble's per-member k[K][R] handed on as the table); T[K]: T_rows = T[m]
        "discrete"          stops shared by the members (tstops): held_stop_index(t, tstops), as T_rows = T_stops[held] or, without
                            T_stops, as k_row = held (rows of the k_table)
        "discrete_members"  stops: K pairs (tstops_m, T_stops_m): T_rows[m] = T_stops_m[held_stop_index(t, tstops_m)]
        "continuous"        nodes: K pairs (t_nodes_m, T_nodes_m): T_rows[m] = np.interp(t, t_nodes_m, T_nodes_m)
    Keys are formed for every row of the grid; the pass ignores those past a member's saved rows."""
    t = np.asarray(t, dtype=float).ravel()
    n_saved = np.asarray(n_saved, dtype=np.int64).ravel()
    K, M = len(n_saved), len(t)
    if np.any(n_saved < 0) or np.any(n_saved > M):
        raise ValueError("n_saved must lie in [0, len(t)]")
    w = np.zeros((K, M))
    for m in range(K):
        n = int(n_saved[m])
        if n >= 1:
            w[m, :n] = flux_weights(t[:n])
    out = dict(w=w)
    if kind == "static":
        if T is None:
            out["k_row"] = np.repeat(np.arange(K, dtype=np.int64)[:, None], M, axis=1)
        else:
            T = np.asarray(T, dtype=float).ravel()
            if len(T) != K:
                raise ValueError("T must have one entry per member")
            out["T_rows"] = np.repeat(T[:, None], M, axis=1)
    elif kind == "discrete":
        if tstops is None:
            raise ValueError('kind "discrete" needs tstops')
        held = held_stop_index(t, tstops)
        if T_stops is None:
            out["k_row"] = np.repeat(held[None, :], K, axis=0)
        else:
            out["T_rows"] = np.repeat(np.asarray(T_stops, dtype=float)[held][None, :], K, axis=0)
    elif kind == "discrete_members":
        if stops is None or len(stops) != K:
            raise ValueError('kind "discrete_members" needs one (tstops, T_stops) pair per member')
        out["T_rows"] = np.stack([np.asarray(Ts, dtype=float)[held_stop_index(t, ts)] for ts, Ts in stops]) if K else np.zeros((0, M))
    elif kind == "continuous":
        if nodes is None or len(nodes) != K:
            raise ValueError('kind "continuous" needs one (t_nodes, T_nodes) pair per member')
        out["T_rows"] = np.stack([np.interp(t, np.asarray(tn, dtype=float), np.asarray(Tn, dtype=float)) for tn, Tn in nodes]) if K else np.zeros((0, M))
    else:
        raise ValueError('kind must be "static", "discrete", "discrete_members" or "continuous"')
    return out


@dataclass
class ReactionFluxes:
    """Result of reaction_fluxes: flux[R] = sum_b weights[b] rate_r(u_b) (time-integrated rate of every reaction of
    `rd`), per species the gross production[N] = sum_r nu+_ir flux_r and consumption[N] = sum_r nu-_ir flux_r (their
    difference is the net change the RHS integrates), the weights used and, if asked for, rates[B][R]."""
    flux: np.ndarray
    production: np.ndarray
    consumption: np.ndarray
    weights: np.ndarray
    rates: Optional[np.ndarray] = None

    def top(self, n):
        """Ids (0-based positions in rd) of the n reactions of greatest |flux|, greatest first (ties: lower id first)."""
        return np.argsort(-np.abs(self.flux), kind="stable")[:int(n)]

    @classmethod
    def from_flux(cls, flux, rd, n_species, weights, rates=None):
        flux = np.asarray(flux, dtype=float)
        prod, cons = np.zeros(n_species), np.zeros(n_species)
        for r in range(rd.nr):
            for sid, st in zip(rd.id_prods[r], rd.stoic_prods[r]):
                prod[sid - 1] += st * flux[r]
            for sid, st in zip(rd.id_reacs[r], rd.stoic_reacs[r]):
                cons[sid - 1] += st * flux[r]
        return cls(flux, prod, cons, np.asarray(weights, dtype=float), rates)


def saved_state_rate_source(out, calculator, t):
    """The rate constants a solve held at each of its saved times t, as the keywords of HipNetwork.flux_batched /
    drg_batched: dict(k=, k_row=) or dict(T=) (reaction_fluxes documents the rules)."""
    conditions = out.conditions
    arr = isinstance(calculator, PrecalculatedArrheniusCalculator)
    src = {}
    if isstatic(conditions) or isinstance(calculator, DummyKineticCalculator):
        src = dict(k=np.asarray(get_initial_rates(conditions, calculator), dtype=float)[None, :], k_row=np.zeros(len(t), np.int64))
    elif conditions.discrete_updates:
        if out.sol_k is None:
            raise ValueError("a discrete-update solve output needs sol_k (the rate constants at the stops)")
        held = held_stop_index(t, out.sol_k.t)
        if arr and hasattr(out.sol_k, "T"):
            src = dict(T=np.asarray(out.sol_k.T, dtype=float)[held])
        else:
            src = dict(k=np.asarray(out.sol_k.u, dtype=float), k_row=held)
    elif arr:
        prof = conditions.profiles[conditions.symbols.index("T")]
        src = dict(T=np.full(len(t), float(prof.value)) if isstatic(prof) else np.asarray(out.sol_vcs["T"], dtype=float))
    else:
        raise ValueError("calculator does not support continuous rate updates")
    return src


def _saved_state_pass(out, calculator, run, t_min=None):
    """One analysis pass over the saved states of a solve, (t, run(h, u, src)): `calculator` is checked against out.rd as
    setup_network does; t, u[B][N] are the saved times and states, of t >= t_min alone when that is given; src the keywords of
    the rate constants the solve held at each of them (saved_state_rate_source); h a handle of out.rd (species ids in rd are
    1-based) that holds the calculator's Arrhenius law when temperatures are the source, closed whatever `run` does."""
    sd, rd = out.sd, out.rd
    setup_network(sd, rd, calculator)
    t = np.asarray(out.sol.t, dtype=float)
    u = np.ascontiguousarray(np.asarray(out.sol.u, dtype=float).reshape(len(t), sd.n))
    src = saved_state_rate_source(out, calculator, t)
    if t_min is not None:
        keep = t >= float(t_min)
        t, u = t[keep], np.ascontiguousarray(u[keep])
        for key in ("k_row", "T"):      # (one entry per saved time; k holds the rows k_row indexes)
            if key in src:
                src[key] = np.asarray(src[key])[keep]
    h = capi.HipNetwork(*rd.flat(sd.n), index_base=1)
    try:
        if "T" in src:
            h.set_arrhenius(calculator.Ea, calculator.A, calculator.k_max, calculator.t_mult)
        return t, run(h, u, src)
    finally:
        h.close()


def _species_ids(sd, species):
    """0-based ids of species given by name or by 0-based id."""
    return [sd.toInt[x] - 1 if isinstance(x, str) else int(x) for x in species]


def reaction_fluxes(out, calculator, weights="trapezoid", rates=False):
    """Time-integrated rate of every reaction over the saved states of a solve - which reactions carried the flux, the
    companion of identify_next_seeds' "which species matter". `out` is any ODESolveOutput (solve_network's, or one read
    back by load_output); `calculator` must be the one the solve used: the low-k cutoff has already spliced it to `out.rd`
    (lengths are checked as setup_network does, ValueError). `weights`: "trapezoid" (flux_weights(out.sol.t)), None
    (weights 1: a plain sum over the saved states) or an array of one weight per saved time. `rates=True` also returns the
    per-state rates[B][R].

    The rate constants of a saved state are the ones the solve held there: a static solve (or a Dummy calculator, which is
    constant) uses get_initial_rates; discrete updates use stop held_stop_index(t, tstops) - with the Arrhenius calculator
    its temperature, evaluated on the device inside the pass, otherwise row k_row of sol_k.u; continuous updates use
    T = sol_vcs["T"] at the saved times. One pass of the device's flux kernel (kin_flux_batched) over sol.u.

    The trapezoid rule is exact to O(dt^2) between rate updates and first order across a stop, where k jumps: callers who
    need more should save more often."""
    setup_network(out.sd, out.rd, calculator)      # (before the weights are looked at; the pass below checks again)
    t = np.asarray(out.sol.t, dtype=float)
    if isinstance(weights, str):
        if weights != "trapezoid":
            raise ValueError('weights must be "trapezoid", None or an array of one weight per saved time')
        w = flux_weights(t)
    elif weights is None:
        w = np.ones(len(t))
    else:
        w = np.asarray(weights, dtype=float).ravel()
        if len(w) != len(t):
            raise ValueError("weights must have one entry per saved time")
    _, res = _saved_state_pass(out, calculator, lambda h, u, src: h.flux_batched(u, w=w, want_rates=rates, **src))
    flux, rr = res if rates else (res, None)
    return ReactionFluxes.from_flux(flux, out.rd, out.sd.n, w, rr)


# ---- directed-relation-graph reduction (EXTENSION: Lu & Law's DRG over the saved states of a solve) ---------------------
def drg_coefficients(out, calculator, pairing=True):
    """(rowptr[N + 1], colidx[E], coef[E]): the directed relation graph of `out.rd` over the saved states of a solve - edge
    (A, B) in CSR form (0-based, sorted columns, no diagonal) with coef_AB = max over the saved states of num_AB / den_A, the
    share of species A's turnover that runs through records B takes part in (include/kinetica_hip.h has the definition;
    pairing: a reaction and its exact reverse are one record progressing at their net rate). `calculator` and the rate
    constants of every saved state are chosen as reaction_fluxes chooses them. One device pass (kin_drg_batched) over sol.u."""
    _, graph = _saved_state_pass(out, calculator, lambda h, u, src: h.drg_pattern(pairing) + (h.drg_batched(u, pairing=pairing, **src),))
    return graph


def drg_select(rowptr, colidx, coef, targets, eps):
    """Species (0-based, sorted) reachable from `targets` over the edges with coef >= eps: the targets themselves and, from
    every kept species A, every B with coef_AB >= eps. Pure NumPy."""
    rowptr, colidx, coef = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64), np.asarray(coef, dtype=float)
    n = len(rowptr) - 1
    keep = np.zeros(n, bool)
    front = np.unique(np.asarray(list(targets), dtype=np.int64))
    if len(front) and (front[0] < 0 or front[-1] >= n):
        raise ValueError("target species id out of range")
    keep[front] = True
    strong = coef >= float(eps)
    while len(front):
        idx = np.concatenate([np.arange(rowptr[a], rowptr[a + 1]) for a in front]) if len(front) else np.zeros(0, np.int64)
        nxt = np.unique(colidx[idx[strong[idx]]]) if len(idx) else np.zeros(0, np.int64)
        front = nxt[~keep[nxt]]
        keep[front] = True
    return np.flatnonzero(keep).astype(np.int64)


def pfa_coefficients(out, calculator, pairing=True):
    """(rowptr[N + 1], colidx[E2], coef[E2]): path flux analysis (Sun, Chen, Gou & Ju) of `out.rd` over the saved states of a
    solve - pair (A, B) in CSR form (0-based, sorted columns, no diagonal) on the pattern E2 of the DRG edges and every
    two-hop pair A -> M -> B, with coef_AB = max over the saved states of rp_AB + rc_AB + sum_M (rp_AM rp_MB + rc_AM rc_MB):
    the production and the consumption share of A's turnover that run through B, directly and over one intermediate
    (include/kinetica_hip.h has the definition; pairing as in drg_coefficients). `calculator` and the rate constants of every
    saved state are chosen as reaction_fluxes chooses them. One device pass (kin_pfa_batched) over sol.u."""
    _, graph = _saved_state_pass(out, calculator, lambda h, u, src: h.pfa_pattern(pairing) + (h.pfa_batched(u, pairing=pairing, **src),))
    return graph


def drgep_importance(out, calculator, targets, pairing=True, importance=None):
    """importance[N] of DRG with error propagation (Pepiot-Desjardins & Pitsch) over the saved states of a solve: R_B = the
    largest product, over any path from a target (names or 0-based ids) to B, of the signed net direct-interaction
    coefficients r_AB = |sum nu_A w| / max(P_A, C_A) of the state, maximised over the saved states (include/kinetica_hip.h has
    the definition; pairing as in drg_coefficients). `importance`: the result of an earlier call, which takes part in the
    maximum (several solves folded into one ranking). `calculator` and the rate constants of every saved state are chosen as
    reaction_fluxes chooses them. One device pass (kin_drgep_batched) over sol.u."""
    tg = _species_ids(out.sd, targets)
    _, imp = _saved_state_pass(out, calculator, lambda h, u, src: h.drgep_batched(u, tg, pairing=pairing, importance=importance, **src))
    return imp


def drgep_select(importance, targets, eps):
    """Species (0-based, sorted) with importance >= eps, the targets always among them. Pure NumPy."""
    importance = np.asarray(importance, dtype=float)
    n = len(importance)
    tg = np.unique(np.asarray(list(targets), dtype=np.int64))
    if len(tg) and (tg[0] < 0 or tg[-1] >= n):
        raise ValueError("target species id out of range")
    keep = importance >= float(eps)
    keep[tg] = True
    return np.flatnonzero(keep).astype(np.int64)


def reaction_importance(out, calculator, species=None, pairing=True, importance=None):
    """importance[R] of reaction elimination (Lu & Law 2008) over the saved states of a solve: per reaction of `out.rd` the
    largest share |nu_A| |w| / den_A its record holds of the turnover of any species A it changes, maximised over the saved
    states (include/kinetica_hip.h has the definition; pairing as in drg_coefficients; the two reactions of a pair carry the
    same value). `species` (names or 0-based ids; None: every species): the species a reaction is judged by - the
    denominators are always the whole network's. `importance`: the result of an earlier call, which takes part in the
    maximum (several solves folded into one ranking). `calculator` and the rate constants of every saved state are chosen as
    reaction_fluxes chooses them. One device pass (kin_reaction_importance_batched) over sol.u."""
    sp = None if species is None else _species_ids(out.sd, species)
    _, imp = _saved_state_pass(out, calculator, lambda h, u, src: h.reaction_importance_batched(u, species=sp, pairing=pairing,
                                                                                            importance=importance, **src))
    return imp


_reaction_importance = reaction_importance      # (reduce_network has a keyword of the same name)


def reaction_select(importance, eps, candidates=None):
    """Reactions (0-based, sorted) with importance >= eps, among `candidates` (0-based ids) when given. Pure NumPy."""
    importance = np.asarray(importance, dtype=float)
    keep = importance >= float(eps)
    if candidates is not None:
        cand = np.unique(np.asarray(list(candidates), dtype=np.int64))
        if len(cand) and (cand[0] < 0 or cand[-1] >= len(importance)):
            raise ValueError("candidate reaction id out of range")
        inside = np.zeros(len(importance), bool)
        inside[cand] = True
        keep &= inside
    return np.flatnonzero(keep).astype(np.int64)


@dataclass
class DRGReduction:
    """Result of reduce_network: the kept species / reactions (0-based positions in the full sd / rd, ascending), the
    renumbered sd and rd, the calculator spliced to rd, and the graph the selection was made on."""
    species_kept: np.ndarray
    reactions_kept: np.ndarray
    sd: SpeciesData
    rd: RxData
    calculator: object
    rowptr: np.ndarray
    colidx: np.ndarray
    coef: np.ndarray
    targets: np.ndarray
    eps: float
    importance: Optional[np.ndarray] = None       # method="drgep": the importance the selection was made on
    # Reaction elimination (None: the species rule alone): the threshold and the importance, one entry per reaction of the
    # FULL network. Plain attributes that reduce_network sets, not dataclass fields: `importance` stays the last field, as
    # callers that build or unpack a DRGReduction by position (and tests/test_drgep_host.py) expect.
    reaction_eps = None
    reaction_importance = None

    def map_u0(self, u0):
        """A u0 specification of the full network (ODESimulationParams.u0: dict name -> concentration, or a vector over the
        full species) in the reduced numbering. A non-zero concentration of a dropped species is an error."""
        if isinstance(u0, dict):
            lost = [sp for sp, c in u0.items() if sp not in self.sd.toInt and c != 0]
            if lost:
                raise ValueError(f"u0 gives a concentration to species the reduction dropped: {lost}")
            return {sp: c for sp, c in u0.items() if sp in self.sd.toInt}
        u0 = np.asarray(u0, dtype=float)
        dropped = np.ones(len(u0), bool)
        dropped[self.species_kept[self.species_kept < len(u0)]] = False
        if np.any(u0[dropped] != 0):
            raise ValueError("u0 gives a concentration to species the reduction dropped")
        out = np.zeros(len(self.species_kept))
        inside = self.species_kept < len(u0)
        out[inside] = u0[self.species_kept[inside]]
        return out


def reduce_network(out, calculator, targets, eps, pairing=True, coef=None, method="drg", importance=None, reaction_eps=None,
                   reaction_importance=None):
    """DRG reduction of the network of a solve: keeps the species reachable from `targets` (names or 0-based ids) over the
    edges with coefficient >= eps - the species non-zero in the first saved state always count as targets - and the
    reactions ALL of whose species, on both sides, are kept. `coef`: (rowptr, colidx, coef) of an earlier drg_coefficients
    call (or several solves folded into one graph), else computed here. `calculator` is left alone; the DRGReduction
    carries a copy spliced to the reduced rd, ready for solve_network / solve_network_ensemble.

    method="drgep" keeps instead the species whose DRGEP importance (drgep_importance, with the same targets) is >= eps;
    `importance`: the vector of an earlier drgep_importance call made with these targets (or several solves folded into one),
    else computed here. The reaction rule and the splicing are the same; the result carries `importance` and no graph.

    method="pfa" is the DRG form on the path-flux-analysis graph: `coef` is (rowptr, colidx, coef) of pfa_coefficients, else
    computed here, and the selection is drg_select's on it.

    reaction_eps (None: nothing below happens) adds reaction elimination as a second step: of the reactions the species rule
    keeps, only those with importance >= reaction_eps stay, the importance being that of the FULL network judged by the kept
    species (the function reaction_importance with species = the kept species and the same pairing); the argument
    `reaction_importance`: that vector from an earlier call, one entry per reaction of out.rd, used as it is. No species is
    dropped in this step: a kept species that loses all its reactions stays as an inert entry, so map_u0 and the numbering mean
    what they meant. The result carries reaction_eps and the vector."""
    if method not in ("drg", "drgep", "pfa"):
        raise ValueError('method must be "drg", "drgep" or "pfa"')
    sd, rd = out.sd, out.rd
    tg = [sd.toInt[x] - 1 if isinstance(x, str) else int(x) for x in targets]
    u_first = np.asarray(out.sol.u, dtype=float).reshape(len(out.sol.t), sd.n)[0]
    tg = np.unique(np.concatenate([np.asarray(tg, dtype=np.int64), np.flatnonzero(u_first != 0)]))
    imp = None
    if method == "drgep":
        imp = np.asarray(drgep_importance(out, calculator, tg, pairing) if importance is None else importance, dtype=float)
        if len(imp) != sd.n:
            raise ValueError("importance must have one entry per species")
        rowptr = colidx = cf = np.zeros(0)
        kept_sp = drgep_select(imp, tg, eps)
    else:
        graph = pfa_coefficients if method == "pfa" else drg_coefficients
        rowptr, colidx, cf = graph(out, calculator, pairing) if coef is None else coef
        kept_sp = drg_select(rowptr, colidx, cf, tg, eps)
    sd_new, new_id = sd.subset(kept_sp + 1)
    rd_new, kept_rx = rd.subset_species(new_id)
    kept_rx = np.asarray(kept_rx, dtype=np.int64)
    rx_imp = None
    if reaction_eps is not None:
        rx_imp = np.asarray(_reaction_importance(out, calculator, kept_sp, pairing) if reaction_importance is None
                            else reaction_importance, dtype=float)
        if rx_imp.shape != (rd.nr,):
            raise ValueError("reaction_importance must have one entry per reaction of the full network")
        strong = reaction_select(rx_imp, reaction_eps, kept_rx)
        rd_new.splice(np.flatnonzero(~np.isin(kept_rx, strong)))
        kept_rx = strong
    kill = np.setdiff1d(np.arange(rd.nr), kept_rx)
    calc = copy.deepcopy(calculator)
    if len(kill):
        calc.splice(kill)
    red = DRGReduction(kept_sp, kept_rx, sd_new, rd_new, calc, np.asarray(rowptr), np.asarray(colidx), np.asarray(cf), tg, float(eps), imp)
    if reaction_eps is not None:
        red.reaction_eps, red.reaction_importance = float(reaction_eps), rx_imp
    return red


# ---- timescale analysis (EXTENSION: species lifetimes, quasi-steady-state error and stiffness along a solve) ---------------
@dataclass
class Timescales:
    """Result of species_timescales: the saved times that count, per species decay_max[N] = max over them of -J_ii,
    decay_min[N] = min of -J_ii and qss_err[N] = max of |f_i| / |J_ii| (include/kinetica_hip.h has the definitions), and
    norm = the infinity norm of the Jacobian at every counting state."""
    t: np.ndarray
    decay_max: np.ndarray
    decay_min: np.ndarray
    qss_err: np.ndarray
    norm: np.ndarray

    def lifetime_min(self):
        """The shortest lifetime tau_i = -1 / J_ii of every species along the run: 1 / decay_max where that is positive, else inf."""
        return _inverse_where_positive(self.decay_max)

    def lifetime_max(self):
        """The longest lifetime of every species along the run: 1 / decay_min where that is positive, else inf."""
        return _inverse_where_positive(self.decay_min)

    def stiffness(self):
        """The largest ||J||_inf along the run, a bound of the spectral radius (0.0 without a counting state)."""
        return float(np.max(self.norm)) if len(self.norm) else 0.0

    @property
    def summary(self):
        return np.stack([self.decay_max, self.decay_min, self.qss_err])


def _inverse_where_positive(x):
    x = np.asarray(x, dtype=float)
    out = np.full(x.shape, np.inf)
    pos = x > 0
    out[pos] = 1.0 / x[pos]
    return out


def species_timescales(out, calculator, t_min=None, summary=None):
    """Timescales of `out.rd` over the saved states of a solve with t >= t_min (None: all of them; a t_min past the initial
    layer leaves out the induction period, where nothing is quasi-steady yet). `summary`: an earlier Timescales, whose three
    per-species arrays take part in the extrema (several solves folded into one). `calculator` and the rate constants of every
    saved state are chosen as reaction_fluxes chooses them. One device pass (kin_timescale_batched) over the counting states."""
    earlier = None if summary is None else summary.summary
    t, res = _saved_state_pass(out, calculator, lambda h, u, src: h.timescale_batched(u, summary=earlier, **src), t_min=t_min)
    s = res["summary"]
    return Timescales(t, s[0], s[1], s[2], res["norm"])


def qss_candidates(ts, tol, scale=None, max_lifetime=None):
    """Species (0-based, sorted) that stayed in quasi-steady state over the states `ts` covers: qss_err / scale <= tol, consumed
    at every state (decay_min > 0) and, with max_lifetime, never slower than it (1 / decay_min <= max_lifetime). `scale`: a
    positive array of one concentration per species, e.g. the per-species maximum of the solve (None: 1, the absolute error in
    concentration units); a non-positive entry raises ValueError. Pure NumPy."""
    err = np.asarray(ts.qss_err, dtype=float)
    dmin = np.asarray(ts.decay_min, dtype=float)
    sc = np.ones(len(err)) if scale is None else np.asarray(scale, dtype=float).ravel()
    if len(sc) != len(err):
        raise ValueError("scale must have one entry per species")
    if not np.all(sc > 0):
        raise ValueError("scale must be positive")
    keep = (err / sc <= float(tol)) & (dmin > 0)
    if max_lifetime is not None:
        keep &= _inverse_where_positive(dmin) <= float(max_lifetime)
    return np.flatnonzero(keep).astype(np.int64)


# ---- the consumer of a level's solve (src/exploration/explore_utils.jl:338-406) ---------------------------
def identify_next_seeds(sol, sd: SpeciesData, seed_conc: Optional[float] = None, *, elim_small_na: int = 0,
                        ignore: Optional[Sequence[str]] = (), saveto: Optional[str] = None) -> List[str]:
    """identify_next_seeds(sol, sd, seed_conc; elim_small_na, ignore, saveto) and the three-argument-less method
    without `seed_conc` (explore_utils.jl:338-374, 376-406): species whose maximum concentration over the saved
    trajectory reaches `seed_conc` (all species when it is None), minus `ignore`d SMILES and, with
    `elim_small_na > 0`, species of fewer atoms (`sd.xyz[i]["N_atoms"]`). `saveto` writes the reference's seeds.out
    table. The per-species maxima are `sol.umax` - reduced on the device by `kin_solution_max` when `sol` comes from
    `solve_network`, so the trajectory is never scanned on the host; a solution read back from disk (`load_output`)
    has no device side and its saved `u` is reduced here."""
    umax = getattr(sol, "umax", None)
    if umax is None:
        umax = np.max(np.asarray(sol.u, dtype=float), axis=0)
    if len(umax) != sd.n:
        raise ValueError("solution and SpeciesData disagree on the number of species")
    if elim_small_na > 0 and sd.xyz is None:
        raise ValueError("elim_small_na needs SpeciesData.xyz (N_atoms per species)")
    ignore = set(ignore or ())
    seeds, concs = [], []
    for sid in range(1, sd.n + 1):
        smi = sd.toStr[sid]
        if smi in ignore:
            continue
        c = float(umax[sid - 1])
        if seed_conc is not None and not c >= seed_conc:
            continue
        if elim_small_na > 0 and sd.xyz[sid]["N_atoms"] < elim_small_na:
            continue
        seeds.append(smi); concs.append(c)
    if saveto is not None:
        w = max(len(x) for x in seeds)      # an empty selection raises here as `maximum` of an empty list does there
        with open(saveto, "w") as f:
            f.write(f"{len(seeds)}\n")
            f.write(f"SID   {'SMILES'.ljust(w)}   Max. Conc.\n")
            for i, (smi, c) in enumerate(zip(seeds, concs), start=1):
                f.write(f"{str(i).ljust(5)} {smi.ljust(w)}   {_julia_float(c)}\n")
    return seeds


def _julia_float(x: float) -> str:
    """Julia's `print(::Float64)`: shortest round-trip digits, fixed notation for 1e-4 <= |x| < 1e6, else `d.ddde±x`."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Inf" if x > 0 else "-Inf"
    if x == 0:
        return "-0.0" if str(x).startswith("-") else "0.0"
    r = repr(float(x))
    mant, _, ex = r.partition("e")
    sign = "-" if mant.startswith("-") else ""
    mant = mant.lstrip("-")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0") or "0"
    # decimal exponent of the first significant digit
    if ex:
        e10 = int(ex) + len(ip) - 1 if ip.strip("0") else int(ex) - (len(fp) - len(fp.lstrip("0"))) - 1
    else:
        e10 = len(ip) - 1 if ip.strip("0") else -(len(fp) - len(fp.lstrip("0"))) - 1
    digits = digits.rstrip("0") or "0"
    if -5 < e10 < 6:
        if e10 >= 0:
            whole = digits[: e10 + 1].ljust(e10 + 1, "0")
            frac = digits[e10 + 1:] or "0"
        else:
            whole, frac = "0", "0" * (-e10 - 1) + digits
        return f"{sign}{whole}.{frac}"
    m = digits[0] + "." + (digits[1:] or "0")
    return f"{sign}{m}e{e10}"
