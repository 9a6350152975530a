"""ctypes binding of libkinetica_hip.so (C ABI: include/kinetica_hip.h).

This is the Python twin of the Julia `ccall` shim shown in INTEGRATION.md. There is no CPU
fallback: a missing library or a missing HIP device raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KIN_LIB_PATH", os.path.join(_HERE, "libkinetica_hip.so"))   # (override: A/B builds in tools/)

KIN_OK, KIN_ERR_INVALID_ARG, KIN_ERR_UNSUPPORTED, KIN_ERR_DEVICE, KIN_ERR_SOLVE_FAILED, KIN_ERR_CAPACITY, KIN_ERR_STATE = range(7)
RETCODE_NAMES = {0: "Success", 1: "MaxIters", 2: "DtLessThanMin", 3: "Unstable"}

# every symbol include/kinetica_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "kin_network_create", "kin_network_destroy", "kin_network_sizes", "kin_last_error",
    "kin_set_rates", "kin_get_rates", "kin_set_arrhenius", "kin_rates_at", "kin_arrhenius_eval",
    "kin_rate_table", "kin_rhs", "kin_rhs_batched", "kin_rhs_batched_dev",
    "kin_jac_nnz", "kin_jac_pattern", "kin_jac_values", "kin_solve", "kin_solve_explicit", "kin_solve_continuous", "kin_solution_size",
    "kin_solution_copy", "kin_solution_max", "kin_integrator_init", "kin_integrator_init_continuous", "kin_integrator_step",
    "kin_integrator_state",
    "kin_newton_solve", "kin_device_count", "kin_set_device", "kin_version", "kin_solution_dot", "kin_rate_table_rows",
    "kin_solution_max_dev", "kin_rate_table_dev", "kin_rhs_block_dev",
    "kin_lib_layout", "kin_lib_layout_host", "kin_states_to_lib_dev", "kin_states_from_lib_dev", "kin_rates_to_lib_dev", "kin_rate_table_lib_dev",
    "kin_rhs_tiled_dev", "kin_rhs_batched_T_dev", "kin_rhs_batched_klib_dev", "kin_abi_version", "kin_struct_size",
    "kin_solve_ensemble", "kin_lu_analyze_host", "kin_solve_ensemble_continuous", "kin_solve_ensemble_discrete",
    "kin_solve_ensemble_continuous_params", "kin_solve_ensemble_discrete_params",
    "kin_resident_probe", "kin_newton_probe", "kin_step_probe", "kin_eval_probe", "kin_cache_probe",
    "kin_flux_batched", "kin_flux_batched_dev", "kin_solution_flux",
    "kin_flux_segmented", "kin_flux_segmented_dev", "kin_ensemble_size", "kin_ensemble_max", "kin_ensemble_dot", "kin_ensemble_flux",
    "kin_drg_pattern_host", "kin_drg_pattern", "kin_drg_batched", "kin_drg_batched_dev", "kin_solution_drg", "kin_ensemble_drg",
    "kin_drgep_batched", "kin_drgep_batched_dev", "kin_drgep_paths", "kin_solution_drgep", "kin_ensemble_drgep",
    "kin_pfa_pattern_host", "kin_pfa_pattern", "kin_pfa_batched", "kin_pfa_batched_dev", "kin_pfa_paths", "kin_solution_pfa",
    "kin_ensemble_pfa",
    "kin_reaction_importance_plan_host", "kin_reaction_importance_batched", "kin_reaction_importance_batched_dev",
    "kin_solution_reaction_importance", "kin_ensemble_reaction_importance",
    "kin_jac_batched", "kin_jac_batched_dev", "kin_timescale_batched", "kin_timescale_batched_dev", "kin_solution_timescale",
    "kin_ensemble_timescale", "kin_timescale_plan_host",
    "kin_members_inputs_host", "kin_members_moments", "kin_members_moments_dev", "kin_members_quantiles", "kin_members_quantiles_dev",
    "kin_members_correlate", "kin_members_correlate_dev", "kin_ensemble_moments", "kin_ensemble_quantiles", "kin_ensemble_correlate",
    "kin_members_sobol", "kin_members_sobol_dev", "kin_ensemble_sobol",
    "kin_events_segmented", "kin_events_segmented_dev", "kin_ensemble_events", "kin_solution_events",
    "kin_resample_bracket_host", "kin_resample_segmented", "kin_resample_segmented_dev", "kin_solution_resample", "kin_ensemble_resample",
    "kin_observables_host", "kin_observables_segmented", "kin_observables_segmented_dev", "kin_solution_observables",
    "kin_ensemble_observables", "kin_ensemble_observable_count",
    "kin_flux_plan_host", "kin_network_compute_units",
    "kin_sweep_plan", "kin_sweep_plan_host", "kin_tiled_sweep_plan", "kin_tiled_sweep_plan_host",
]
# in-degree classes of the DRGEP path search (drg.hpp: IN_SHORT_MAX, IN_WAVE_MAX): a lane, a wavefront, the workgroup
DRGEP_IN_SHORT_MAX, DRGEP_IN_WAVE_MAX = 32, 256
MEMBERS_MAX_SORTED = 4096   # include/kinetica_hip.h: KIN_MEMBERS_MAX_SORTED, the participants quantiles and rank correlations take
ABI_VERSION = 6   # include/kinetica_hip.h: KIN_ABI_VERSION this binding was written against
# the event-time pass (include/kinetica_hip.h: KIN_LEVEL_*, the sign of `direction`, KIN_FROM_*) and the names of its results
EVENT_KINDS = dict(abs=0, of_peak=1, of_start=2)
EVENT_DIRECTIONS = dict(rise=1, fall=-1)
EVENT_STARTS = dict(begin=0, peak=1)
EVENT_OUTPUTS = ("u_peak", "t_peak", "t_cross")
# the resampling pass (include/kinetica_hip.h: KIN_RESAMPLE_*) and the jc codes of a query that is not inside
RESAMPLE_MODES = dict(fill=0, hold=1)
RESAMPLE_BELOW, RESAMPLE_ABOVE, RESAMPLE_NONE = -1, -2, -3


# kin_step_probe (include/kinetica_hip.h): rows of the state block, fields of the flattened control block, argument slots
STEP_ROWS, STEP_CTRL, STEP_IARGS, STEP_DARGS = 28, 18, 12, 24
STEP_ROW = dict(D=0, y=8, psi=9, d=10, scale=11, f0=12, f1=13, ytmp=14, cs=15, K=16, x=23, out=24, y_new=25, u=26, b=27)
STEP_CTRL_FIELDS = ("dy_norm_old", "dy_norm", "err_norm", "err_m_norm", "err_p_norm", "crate", "scratch0", "scratch1", "scratch2",
                    "scratch3", "newton_done", "converged", "n_iter", "nonfinite", "any_negative", "ticket", "lu_bad", "spec_go")
STEP_OPS = dict(init_D=0, predict=1, accept=2, accept_predict=3, change_D=4, interp=5, norms=6, newton=7, rk_combine=8, rk_error=9, vec=10,
                corrector=11)
STEP_VEC_OPS = dict(load_u0=0, cs_from_y=1, y_from_cs_clipped=2, y_from_d0=3, ytmp_from_d0=4, ytmp_axpy=5, save_y=6, interp=7,
                    set_time=8)      # (set_time: the resident kernel's paths only)
STEP_IARG_NAMES = ("member", "order", "aux", "copy_out", "go", "iter", "maxit", "publish_always", "crate_from_ctrl", "ban_negatives", "seq",
                   "row")
STEP_DARG_TAIL = dict(c_fact=20, ec=21, ec_m=22, ec_p=23)      # (paths 3 and 4)
STEP_DARG_NAMES = ("atol", "rtol", "h", "upd", "tol", "rate_max", "crate0", "tol_first", "dy_first_max", "c", "ts", "t", "h_abs")
STEP_DARG_W = 13


class KinParams(ctypes.Structure):
    """kin_params: mirror of ODESimulationParams (src/solving/params.jl:3-27)."""
    _fields_ = [("tspan0", c_double), ("tspan1", c_double), ("abstol", c_double), ("reltol", c_double),
                ("adaptive_tols", c_int32), ("update_tols", c_int32), ("solve_chunks", c_int32),
                ("ban_negatives", c_int32), ("solve_chunkstep", c_double), ("maxiters", c_int64),
                ("save_interval", c_double), ("dtmin", c_double)]


class KinStats(ctypes.Structure):
    _fields_ = [(n, c_int64) for n in ("n_steps", "n_rejected", "n_rhs", "n_jac", "n_factor", "n_linsolve",
                                        "n_newton_fail", "n_chunks", "n_restarts", "n_retries")] + \
               [("final_abstol", c_double), ("final_reltol", c_double), ("wall_seconds", c_double)] + \
               [(n, c_int64) for n in ("lu_dense_dim", "lu_sparse_rows", "lu_rounds", "lu_nnz", "n_lu_reused", "lu_slots", "n_bad_pivot", "n_lu_dropped")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KineticaHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[kin status {code}] {msg}")
        self.code = code


# ---- the argument types of every entry include/kinetica_hip.h declares that takes arguments, by name -----------------------------
P64, PD, P32, PV = POINTER(c_int64), POINTER(c_double), POINTER(c_int32), c_void_p
_NET = [c_int64, c_int64] + [P64] * 6 + [c_int]     # a *_host entry's leading arguments: sizes, the six index lists, index base
_SOLVED = [P64, POINTER(c_int32), POINTER(KinStats)]      # n_saved, retcode, stats of a solve
_MEMBERS = [P64, PD, PD, P64, POINTER(c_int32), POINTER(KinStats)]      # n_rows, out_t, out_u, n_saved, retcodes, stats of an ensemble
_KSRC = [PD, c_int64, P64, PD]      # the rate constants of a pass on host arrays: k, n_k_rows, k_row, T
_EVENT = [c_int, c_int, c_int, c_int64, c_double]      # what an event-time pass looks for: level_kind, direction, start, row_begin, never
_RESAMPLE = [c_int, c_double, c_int64]      # what a resampling pass does besides its axes: mode, fill, row_begin
_OBSERVABLES = [c_int64, P64, P64, PD, c_int64, P64, P64, c_int64]      # H, form_ptr, form_idx, form_w, G, num, den, pitch
ARGTYPES = {
    "kin_struct_size": [c_int], "kin_last_error": [PV],
    "kin_network_create": _NET + [POINTER(PV)], "kin_network_destroy": [PV], "kin_network_sizes": [PV, P64, P64],
    "kin_set_rates": [PV, PD], "kin_get_rates": [PV, PD], "kin_set_arrhenius": [PV, PD, PD, c_double, c_double],
    "kin_rates_at": [PV, c_double, PD], "kin_arrhenius_eval": [PD, PD, c_int64, c_double, c_double, c_double, PD],
    "kin_rate_table": [PV, PD, c_int64, PD], "kin_rate_table_rows": [PV, P64, c_int64, PD], "kin_rate_table_dev": [PV, PD, c_int64, PV],
    "kin_rhs": [PV, PD, PD], "kin_rhs_batched": [PV, c_int64, PD, PD, PD], "kin_rhs_batched_dev": [PV, c_int64] + [PV] * 4,
    "kin_rhs_block_dev": [PV, c_int64, c_int64, PV, PV, PV],
    "kin_jac_nnz": [PV, P64], "kin_jac_pattern": [PV, P64, P64, c_int], "kin_jac_values": [PV, PD, PD],
    "kin_solve": [PV, POINTER(KinParams), PD, PD, PD, PD, c_int64] + _SOLVED,
    "kin_solve_explicit": [PV, POINTER(KinParams), PD, PD, PD, PD, c_int64] + _SOLVED,
    "kin_solve_continuous": [PV, POINTER(KinParams), PD, PD, PD, c_int64] + _SOLVED,
    "kin_solve_ensemble": [PV, POINTER(KinParams), c_int64, PD, PD, PD, PD, PD, PD, c_int64] + _MEMBERS,
    "kin_solve_ensemble_continuous": [PV, POINTER(KinParams), c_int64, PD, P64, PD, PD] + _MEMBERS,
    "kin_solve_ensemble_discrete": [PV, POINTER(KinParams), c_int64, PD, P64, PD, PD] + _MEMBERS,
    "kin_solve_ensemble_continuous_params": [PV, POINTER(KinParams), c_int64, PD, PD, PD, P64, PD, PD] + _MEMBERS,
    "kin_solve_ensemble_discrete_params": [PV, POINTER(KinParams), c_int64, PD, PD, PD, P64, PD, PD] + _MEMBERS,
    "kin_integrator_init": [PV, POINTER(KinParams), PD, PD, PD, PD, c_int64],
    "kin_integrator_init_continuous": [PV, POINTER(KinParams), PD, PD, PD, c_int64],
    "kin_integrator_step": [PV, c_int64, P64], "kin_integrator_state": [PV, PD, PD, POINTER(c_int32), POINTER(KinStats)],
    "kin_solution_size": [PV, P64, P64], "kin_solution_copy": [PV, PD, PD], "kin_solution_max": [PV, PD],
    "kin_solution_max_dev": [PV, PV], "kin_solution_dot": [PV, PD, PD],
    "kin_newton_solve": [PV, c_double, PD, PD, PD], "kin_device_count": [POINTER(c_int)], "kin_set_device": [c_int],
    # diagnostics
    "kin_resident_probe": [PV, c_int64, PD, PD, PD, PD, PD, PD, P32, P64],
    "kin_newton_probe": [PV, c_int64, c_int32, PD, PD, PD, PD, P32, P64],
    "kin_step_probe": [PV, c_int32, c_int32, c_int64, c_int64, c_int64, P32, PD, P32, PD, PD, PD, P64],
    "kin_eval_probe": [PV, c_int32, c_int32, c_int32, c_int64, c_int64, P32, PD, PD, c_double, PD, PD, PD, P32, c_double, PD, c_int64, PD,
                       P32, P64],
    "kin_cache_probe": [PV, c_int32, c_int32, c_int64, PD, PD, P32, PD, c_double, P64, c_int64, PD, P64, PD, PD, P32, P64],
    "kin_lu_analyze_host": _NET + [c_int] * 5 + [P64],
    # library order (tiled sweep) and the plan queries of the two batched sweeps
    "kin_lib_layout": [PV, c_int, P64, P64, P64, P32, P64],
    "kin_lib_layout_host": _NET + [c_int, P64, P64, P64, POINTER(ctypes.c_uint64)] + [P32] * 6,
    "kin_states_to_lib_dev": [PV, c_int64, PV, PV, PV], "kin_states_from_lib_dev": [PV, c_int64, PV, PV, PV],
    "kin_rates_to_lib_dev": [PV, c_int64, PV, PV, PV], "kin_rate_table_lib_dev": [PV, PD, c_int64, PV],
    "kin_rhs_tiled_dev": [PV, c_int64] + [PV] * 5, "kin_rhs_batched_T_dev": [PV, c_int64] + [PV] * 4,
    "kin_rhs_batched_klib_dev": [PV, c_int64] + [PV] * 4,
    "kin_sweep_plan": [PV, c_int64, PV, PV, PV, P64], "kin_sweep_plan_host": _NET + [c_int, c_int64, c_int, c_int, c_int, P64],
    "kin_tiled_sweep_plan": [PV, c_int64, c_int, P64], "kin_tiled_sweep_plan_host": _NET + [c_int, c_int64, c_int, P64],
    # reaction fluxes, per state and segmented, and the stored ensemble
    "kin_flux_batched": [PV, c_int64, PD] + _KSRC + [PD, PD, PD], "kin_flux_batched_dev": [PV, c_int64] + [PV] * 8,
    "kin_solution_flux": [PV, PD] + _KSRC + [PD, PD],
    "kin_flux_plan_host": [c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int64, c_int, c_int, c_int, P64],
    "kin_network_compute_units": [PV, POINTER(c_int)],
    "kin_flux_segmented": [PV, c_int64, c_int64, P64, PD] + _KSRC + [PD, PD], "kin_flux_segmented_dev": [PV, c_int64, c_int64] + [PV] * 8,
    "kin_ensemble_size": [PV, P64, P64, P64, P64], "kin_ensemble_max": [PV, PD], "kin_ensemble_dot": [PV, PD, PD],
    "kin_ensemble_flux": [PV, PD] + _KSRC + [PD],
    # directed relation graph, DRGEP, reaction elimination, path flux analysis
    "kin_drg_pattern_host": _NET + [c_int, P64, P64, P64], "kin_drg_pattern": [PV, c_int, c_int, P64, P64, P64],
    "kin_drg_batched": [PV, c_int, c_int64, PD] + _KSRC + [c_int, PD],
    "kin_drg_batched_dev": [PV, c_int, c_int64, PV, PV, PV, PV, c_int, PV, PV],
    "kin_solution_drg": [PV, c_int] + _KSRC + [c_int, PD], "kin_ensemble_drg": [PV, c_int] + _KSRC + [c_int, PD],
    "kin_drgep_batched": [PV, c_int, c_int64, PD] + _KSRC + [P64, c_int64, c_int, c_int, PD, PD, PD, P32],
    "kin_drgep_batched_dev": [PV, c_int, c_int64] + [PV] * 5 + [c_int64, c_int, PV, PV],
    "kin_drgep_paths": [PV, c_int, c_int64, PD, P64, c_int64, c_int, c_int, PD, PD, P32],
    "kin_solution_drgep": [PV, c_int] + _KSRC + [P64, c_int64, c_int, c_int, PD],
    "kin_ensemble_drgep": [PV, c_int] + _KSRC + [P64, c_int64, c_int, c_int, PD],
    "kin_reaction_importance_plan_host": _NET + [c_int, P64, P64, P64, P64],
    "kin_reaction_importance_batched": [PV, c_int, c_int64, PD] + _KSRC + [P64, c_int64, c_int, c_int, PD, PD],
    "kin_reaction_importance_batched_dev": [PV, c_int, c_int64] + [PV] * 5 + [c_int64, c_int, PV, PV],
    "kin_solution_reaction_importance": [PV, c_int] + _KSRC + [P64, c_int64, c_int, c_int, PD],
    "kin_ensemble_reaction_importance": [PV, c_int] + _KSRC + [P64, c_int64, c_int, c_int, PD],
    "kin_pfa_pattern_host": _NET + [c_int, P64, P64, P64], "kin_pfa_pattern": [PV, c_int, c_int, P64, P64, P64],
    "kin_pfa_batched": [PV, c_int, c_int64, PD] + _KSRC + [c_int, PD, PD, PD, PD],
    "kin_pfa_batched_dev": [PV, c_int, c_int64, PV, PV, PV, PV, c_int, PV, PV],
    "kin_pfa_paths": [PV, c_int, c_int64, PD, PD, c_int, PD, PD],
    "kin_solution_pfa": [PV, c_int] + _KSRC + [c_int, PD], "kin_ensemble_pfa": [PV, c_int] + _KSRC + [c_int, PD],
    # timescale analysis
    "kin_jac_batched": [PV, c_int64, PD] + _KSRC + [PD], "kin_jac_batched_dev": [PV, c_int64] + [PV] * 6,
    "kin_timescale_batched": [PV, c_int64, PD] + _KSRC + [c_int, PD, PD, PD, PD],
    "kin_timescale_batched_dev": [PV, c_int64] + [PV] * 4 + [c_int] + [PV] * 5,
    "kin_solution_timescale": [PV] + _KSRC + [c_int64, c_int, PD, PD], "kin_ensemble_timescale": [PV] + _KSRC + [c_int64, c_int, PD, PD],
    "kin_timescale_plan_host": _NET + [P64],
    # cross-member statistics and the Sobol indices of a Saltelli design
    "kin_members_inputs_host": [c_int64, c_int64, PD, P32, c_int, P64, PD],
    "kin_members_moments": [PV, c_int64, c_int64, PD, P32, P64, PD, PD, PD, PD],
    "kin_members_moments_dev": [PV, c_int64, c_int64, PV, P32, P64] + [PV] * 5,
    "kin_members_quantiles": [PV, c_int64, c_int64, PD, P32, P64, c_int64, PD, c_int64, PD],
    "kin_members_quantiles_dev": [PV, c_int64, c_int64, PV, P32, P64, c_int64, PD, c_int64, PV, PV],
    "kin_members_correlate": [PV, c_int64, c_int64, PD, P32, P64, c_int64, PD, c_int64, c_int, PD],
    "kin_members_correlate_dev": [PV, c_int64, c_int64, PV, P32, P64, c_int64, PD, c_int64, c_int, PV, PV],
    "kin_ensemble_moments": [PV, P32, P64, PD, PD, PD, PD], "kin_ensemble_quantiles": [PV, P32, P64, c_int64, PD, c_int64, PD],
    "kin_ensemble_correlate": [PV, P32, P64, c_int64, PD, c_int64, c_int, PD],
    "kin_members_sobol": [PV, c_int64, c_int64, c_int64, PD, P32, P64, c_int64, PD, PD, PD, PD],
    "kin_members_sobol_dev": [PV, c_int64, c_int64, c_int64, PV, P32, P64, c_int64] + [PV] * 5,
    "kin_ensemble_sobol": [PV, c_int64, c_int64, P32, P64, c_int64, PD, PD, PD, PD],
    # event times
    "kin_events_segmented": [PV, c_int64, c_int64, P64, PD, PD, c_int, PD] + _EVENT + [PD, PD, PD],
    "kin_events_segmented_dev": [PV, c_int64, c_int64, PV, PV, PV, c_int, PV] + _EVENT + [PV] * 4,
    "kin_ensemble_events": [PV, PD, c_int, PD] + _EVENT + [PD, PD, PD], "kin_solution_events": [PV, PD] + _EVENT + [PD, PD, PD],
    # resampling
    "kin_resample_bracket_host": [c_int64, c_int64, P64, PD, c_int, c_int64, PD, c_int, c_int64, P32, PD],
    "kin_resample_segmented": [PV, c_int64, c_int64, P64, PD, PD, c_int, c_int64, PD, c_int] + _RESAMPLE + [PD, P32, PD],
    "kin_resample_segmented_dev": [PV, c_int64, c_int64, PV, PV, PV, c_int, c_int64, PV, c_int] + _RESAMPLE + [PV] * 4,
    "kin_solution_resample": [PV, PD, c_int64, PD] + _RESAMPLE + [PD],
    "kin_ensemble_resample": [PV, PD, c_int, c_int64, PD, c_int] + _RESAMPLE + [c_int, PD],
    # observables
    "kin_observables_host": [c_int64, c_int, c_int64, c_int64, P64, PD] + _OBSERVABLES + [PD],
    "kin_observables_segmented": [PV, c_int64, c_int64, P64, PD] + _OBSERVABLES + [PD],
    "kin_observables_segmented_dev": [PV, c_int64, c_int64, PV, PV] + _OBSERVABLES + [PV, PV],
    "kin_solution_observables": [PV] + _OBSERVABLES + [PD], "kin_ensemble_observables": [PV] + _OBSERVABLES + [c_int, PD],
    "kin_ensemble_observable_count": [PV, P64],
}

_lib = None


def lib():
    """Load libkinetica_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP extension is mandatory, there is no CPU fallback)")
        # PyTorch (device buffers, streams, torch.distributed in bench / tests) ships a HIP runtime of its own; a process that
        # loads this library first and torch second ends up with torch seeing no GPU. Loading torch first works both ways.
        import sys
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = ctypes.CDLL(LIB_PATH)
        for name, argtypes in ARGTYPES.items():
            fn = getattr(L, name, None)     # entries added under ABI 6 are found by symbol lookup: an earlier build lacks some
            if fn is not None:
                fn.argtypes = argtypes
        L.kin_struct_size.restype = c_int64
        if L.kin_abi_version() != ABI_VERSION or L.kin_struct_size(0) != ctypes.sizeof(KinParams) or \
                L.kin_struct_size(1) != ctypes.sizeof(KinStats):
            raise ImportError(f"{LIB_PATH}: ABI version {L.kin_abi_version()} / struct sizes do not match this binding "
                              f"(version {ABI_VERSION}); rebuild the library")
        L.kin_version.restype = c_char_p
        L.kin_last_error.restype = c_char_p
        _lib = L
    return _lib


def _pd(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _p64(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_int64))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p32(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_int32))


def _dp(x):
    """A device pointer or a stream given as an int: the c_void_p of it, NULL for 0."""
    return c_void_p(x) if x else None


def _nonempty(a):
    """a, or None for None and for an array without entries: an optional output the library is not handed."""
    return a if a is not None and a.size else None


def _net_head(net):
    """The leading C arguments of a *_host entry for a FlatNetwork: n_species, n_reactions, its six index lists as int64 and
    index base 0 (a pointer made by data_as keeps its array alive)."""
    return [int(net.n_species), int(net.n_reactions)] + \
        [_p64(np.ascontiguousarray(a, dtype=np.int64)) for a in (net.reac_ptr, net.reac_idx, net.reac_sto, net.prod_ptr, net.prod_idx,
                                                                 net.prod_sto)] + [0]


def _acc_buffer(length, given, what):
    """(buffer, accumulate) of an output the library can fold an earlier result into: max(length, 1) zeros and 0, or - `given`,
    the caller's `what` of `length` values - a copy of it, which then takes part, and 1. The caller's array is left alone; the
    result is the buffer's first `length` entries."""
    out = np.zeros(max(length, 1))
    if given is None:
        return out, 0
    c = _f64(given).ravel()
    assert len(c) == length, f"{what} has {len(c)} entries, not {length}"
    out[:length] = c
    return out, 1


def _use32(use, K):
    """A participant mask as the kin_members_* / kin_ensemble_* entries take it: int32[K] (truthy: takes part) or None."""
    if use is None:
        return None
    use = np.ascontiguousarray(np.asarray(use).ravel() != 0, dtype=np.int32)
    if len(use) != K:
        raise ValueError(f"use must have one entry per member ({K}); got {len(use)}")
    return use


def _axis(a, S, L, what):
    """(a as float64, the per-segment flag) of an axis or a set of queries: a[L] shared by the S segments, or a[S][L]."""
    a = np.ascontiguousarray(_f64(a))
    if a.shape == (L,):
        return a, 0
    if a.shape == (S, L):
        return a, 1
    raise ValueError(f"{what} must be [{L}] (shared) or [{S}][{L}] (one per segment); got {a.shape}")


def _queries(xq, S):
    """(xq as float64, Q, the per-segment flag): queries xq[Q] shared by the S segments, or xq[S][Q]."""
    xq = np.ascontiguousarray(_f64(xq))
    if xq.ndim == 1:
        return xq, len(xq), 0
    if xq.ndim == 2 and xq.shape[0] == S:
        return xq, xq.shape[1], 1
    raise ValueError(f"xq must be [Q] (shared) or [{S}][Q] (one set per segment); got {xq.shape}")


def _seg_n(seg_n, S):
    if seg_n is None:
        return None
    seg_n = np.ascontiguousarray(seg_n, dtype=np.int64).ravel()
    if len(seg_n) != S:
        raise ValueError(f"seg_n must have one entry per segment ({S}); got {len(seg_n)}")
    return seg_n


def resample_brackets(x, xq, seg_n=None, row_begin=0):
    """kin_resample_bracket_host (no handle, no device): the brackets of the resampling pass. x[L] or x[S][L] the axis (S = 1
    for x[L] unless seg_n or a two-dimensional xq says otherwise), xq[Q] or xq[S][Q] the queries, seg_n[S] the rows a segment
    really has (None: L each). Returns (jc[S][Q] int32, w[S][Q]): jc the first row from row_begin on with x[j] >= xq, or
    RESAMPLE_BELOW / _ABOVE / _NONE for a query below the segment's range, above it, or NaN / of an empty segment; w the
    chord's weight (xq - x[jc-1]) / (x[jc] - x[jc-1]), 0.0 where x[jc] == xq or the query is not inside."""
    x = np.ascontiguousarray(_f64(x))
    q = np.ascontiguousarray(_f64(xq))
    if x.ndim not in (1, 2):
        raise ValueError(f"x must be [L] or [S][L]; got {x.shape}")
    S = x.shape[0] if x.ndim == 2 else (q.shape[0] if q.ndim == 2 else (1 if seg_n is None else len(np.ravel(seg_n))))
    x, x_per = _axis(x, S, x.shape[-1], "x")
    q, Q, q_per = _queries(q, S)
    seg_n = _seg_n(seg_n, S)
    jc, w = np.zeros((S, Q), np.int32), np.zeros((S, Q))
    st = lib().kin_resample_bracket_host(S, x.shape[-1], _p64(seg_n), _pd(x), x_per, Q, _pd(q), q_per, int(row_begin), _p32(jc), _pd(w))
    if st != KIN_OK:
        raise KineticaHipError(st, "kin_resample_bracket_host: invalid argument (sizes, seg_n, or an axis that decreases or holds a NaN)")
    return jc, w


def _observable_args(form_ptr, form_idx, form_w, num, den, pitch):
    """The C arguments H, form_ptr, form_idx, form_w, G, num, den, pitch of an observables entry and (G, pitch) as integers
    (pitch None: G, the compact form). The arrays go to the library as they are given - it checks them; only their lengths
    are compared here. A pointer made by data_as keeps its array alive."""
    ptr = np.ascontiguousarray(form_ptr, dtype=np.int64).ravel()
    idx = np.ascontiguousarray(form_idx, dtype=np.int64).ravel()
    w = _f64(form_w).ravel()
    num = np.ascontiguousarray(num, dtype=np.int64).ravel()
    den = np.ascontiguousarray(den, dtype=np.int64).ravel()
    if len(idx) != len(w):
        raise ValueError(f"form_idx and form_w must have one entry per term; got {len(idx)} and {len(w)}")
    if len(num) != len(den):
        raise ValueError(f"num and den must have one entry per observable; got {len(num)} and {len(den)}")
    if len(ptr) and int(ptr[-1]) > len(idx):
        raise ValueError(f"form_ptr ends at {int(ptr[-1])} but the forms have {len(idx)} entries")
    H, G = max(len(ptr) - 1, 0), len(num)
    pitch = G if pitch is None else int(pitch)
    return [H, _p64(ptr) if len(ptr) else None, _p64(idx) if len(idx) else None, _pd(w) if len(w) else None, G,
            _p64(num) if G else None, _p64(den) if G else None, pitch], G, pitch


def observables_host(u, form_ptr, form_idx, form_w, num, den, pitch=None, seg_n=None, index_base=0):
    """kin_observables_host (no handle, no device): the observables pass in plain loops, the normative restatement. u[S][L][N]
    (S segments of up to L rows, seg_n[S] of them real; None: L each); the forms in CSR over the species (form_idx in
    index_base); observable g is form num[g], divided by form den[g] unless that is -1. Returns out[S][L][pitch] (pitch None:
    G): the observables in the columns below G, zeros in the others and in every row past a segment's end."""
    u = np.ascontiguousarray(_f64(u))
    if u.ndim != 3:
        raise ValueError(f"u must be [S][L][N]; got {u.shape}")
    S, L, N = u.shape
    seg_n = _seg_n(seg_n, S)
    args, G, pitch = _observable_args(form_ptr, form_idx, form_w, num, den, pitch)
    out = np.full((S, L, max(pitch, 0)), np.nan)
    st = lib().kin_observables_host(N, int(index_base), S, L, _p64(seg_n), _pd(u) if u.size else None, *args, _pd(out) if out.size else None)
    if st != KIN_OK:
        raise KineticaHipError(st, "kin_observables_host: invalid argument (sizes, seg_n, form_ptr, a species, num, den or pitch)")
    return out


def members_inputs(X, use=None, rank=True):
    """kin_members_inputs_host (no handle, no device): the inputs' side of a correlation. X[K][P], one row per member; returns
    (n, Xhat[n][P]): per input the participants' (x - mean) / sqrt(sum (x - mean)^2) in member order, of the average-tie ranks when
    rank; zeros for a column without spread or n < 2."""
    X = np.ascontiguousarray(_f64(X))
    if X.ndim != 2:
        raise ValueError(f"inputs must be [K][P] (one row per member); got {X.shape}")
    K, P = X.shape
    use = _use32(use, K)
    n = c_int64(0)
    out = np.zeros((max(K, 1), max(P, 1)))
    st = lib().kin_members_inputs_host(K, P, _pd(X), _p32(use), int(bool(rank)), ctypes.byref(n), _pd(out))
    if st != KIN_OK:
        raise KineticaHipError(st, "kin_members_inputs_host: invalid argument")
    return n.value, out.ravel()[:n.value * P].reshape(n.value, P).copy()


def device_count():
    n = c_int(0)
    lib().kin_device_count(ctypes.byref(n))
    return n.value


def lib_layout_host(net, hubs=0):
    """The tiled sweep's library order of a FlatNetwork, computed on the host (no device): dict of the layout tables."""
    L = lib()
    info = np.zeros(10, np.int64)
    head = _net_head(net) + [int(hubs), _p64(info)]
    st = L.kin_lib_layout_host(*head, None, None, None, None, None, None, None, None, None)
    if st != KIN_OK:
        raise KineticaHipError(st, "network has no tiled layout")
    h, T, P, E, n_copy, BS, wbase, Q, k_len, has_singles = [int(x) for x in info]
    sp = np.empty(net.n_species, np.int64); slot = np.empty(net.n_reactions, np.int64)
    rec = np.empty(max(P, 1), np.uint64); rowtab = np.empty(max(2 * Q, 1), np.int32); seg_q = np.empty(T + 1, np.int32)
    woff = np.empty(T, np.int32); wcnt = np.empty(T, np.int32); copy_src = np.empty(max(n_copy, 1), np.int32)
    seg_k = np.empty(2 * T, np.int32)
    st = L.kin_lib_layout_host(*head, _p64(sp), _p64(slot), rec.ctypes.data_as(POINTER(ctypes.c_uint64)), _p32(rowtab), _p32(seg_q),
                               _p32(woff), _p32(wcnt), _p32(copy_src), _p32(seg_k))
    assert st == KIN_OK
    return dict(k_len=k_len, has_singles=bool(has_singles), seg_k=seg_k.reshape(T, 2), h=h, T=T, P=P, E=E, n_copy=n_copy, BS=BS, wbase=wbase, Q=Q, species_of_lib=sp, slot_of_reaction=slot,
                rec=rec[:P], rowtab=rowtab[:2 * Q].reshape(Q, 2), seg_q=seg_q, win_off=woff, win_cnt=wcnt, copy_src=copy_src[:n_copy])


def lu_analyze_host(net, hub_degree=0, max_rounds=0, max_tail_degree=0, max_degree=0, min_round=0):
    """Sizes of the symbolic Newton-matrix factorisation of a FlatNetwork, computed on the host (no device). Arguments left at 0
    take the library's defaults (lu.hpp: LUOptions)."""
    info = np.zeros(12, np.int64)
    st = lib().kin_lu_analyze_host(*_net_head(net), int(hub_degree), int(max_rounds), int(max_tail_degree), int(max_degree),
                                   int(min_round), _p64(info))
    if st != KIN_OK:
        raise KineticaHipError(st, "symbolic LU analysis failed")
    keys = ("ns", "m", "rounds", "nnzU", "nnzZ", "nnzV", "nnzLZ", "nnzNVU", "w_size", "fused_products", "plan_entries", "plan_tasks")
    return {k: int(v) for k, v in zip(keys, info)}


# classes of the DRG gather plans by contributions of a row (drg.hpp: SegPlanHost::SHORT_MAX, SEG_LEN), and the entries a
# workgroup takes per pass of a long row (drg_kernels.hip: DRG_WG * DRG_LONG_NX)
DRG_SHORT_MAX, DRG_SEG_LEN, DRG_LONG_PASS = 8, 256, 1024
DRG_INFO = ("edges", "den_contributions", "edge_contributions", "den_short", "den_medium", "den_long", "edge_short", "edge_medium",
            "edge_long")


def drg_pattern_host(net, pairing=True):
    """kin_drg_pattern_host of a FlatNetwork, computed on the host (no device): (rowptr[N + 1], colidx[edges], info) - the edge
    CSR of the directed relation graph (0-based, sorted columns, no diagonal) and a dict of the DRG_INFO sizes: edges,
    contributions, and the rows / edges of the two gather plans by class (<= 8, 9 .. 256, > 256 contributions)."""
    return _pattern_host("kin_drg_pattern_host", DRG_INFO, 0, net, pairing)


def _pattern_host(entry, names, count, net, pairing):
    """(rowptr[N + 1], colidx[nnz], info) of a host pattern entry: the sizes `names` first (nnz is info[count]), then the arrays."""
    fn = getattr(lib(), entry)
    head = _net_head(net) + [1 if pairing else 0]
    info = np.zeros(len(names), np.int64)
    st = fn(*head, _p64(info), None, None)
    if st != KIN_OK:
        raise KineticaHipError(st, lib().kin_last_error(None).decode())
    nnz = int(info[count])
    rowptr, colidx = np.empty(net.n_species + 1, np.int64), np.empty(max(nnz, 1), np.int64)
    st = fn(*head, _p64(info), _p64(rowptr), _p64(colidx))
    assert st == KIN_OK
    return rowptr, colidx[:nnz], {k: int(v) for k, v in zip(names, info)}


REACTION_IMPORTANCE_INFO = ("records", "paired_reactions", "empty_reactions")


def reaction_importance_plan_host(net, pairing=True):
    """kin_reaction_importance_plan_host of a FlatNetwork, computed on the host (no device): (partner[R], species[R][4], nu[R][4],
    info) - per reaction the other reaction of its pair record (-1: none; always -1 without pairing) and the record's up to
    four slots (0-based species or -1, signed net coefficient: the forward reaction's, the sign flipped for the reverse member)
    - and a dict of the REACTION_IMPORTANCE_INFO sizes: records, reactions with a partner, reactions without a non-zero slot."""
    R = int(net.n_reactions)
    info = np.zeros(len(REACTION_IMPORTANCE_INFO), np.int64)
    partner, species, nu = np.empty(max(R, 1), np.int64), np.empty((max(R, 1), 4), np.int64), np.empty((max(R, 1), 4), np.int64)
    st = lib().kin_reaction_importance_plan_host(*_net_head(net), 1 if pairing else 0, _p64(info), _p64(partner), _p64(species), _p64(nu))
    if st != KIN_OK:
        raise KineticaHipError(st, lib().kin_last_error(None).decode())
    return partner[:R], species[:R], nu[:R], {k: int(v) for k, v in zip(REACTION_IMPORTANCE_INFO, info)}


PFA_INFO = ("edges", "pairs", "products", "max_row")
# the largest network the second-generation stage takes (pfa.hpp: PFA_LDS_SPECIES) and the cost sum over M in out(A) of deg(M)
# above which a workgroup, not a wavefront, takes row A (PFA_WG_COST)
PFA_MAX_SPECIES, PFA_WG_COST = 20286, 65536
# the second-generation stage (pfa.hpp, pfa_kernels.hip): out-edges of a row staged at a time, rows M whose loads are in flight
# together, and the columns of the E2 row per thread whose maximum lives in registers (of a wavefront of 64 or a workgroup of 256)
PFA_CHUNK, PFA_AHEAD, PFA_KEEP = 64, 4, 6


def pfa_pattern_host(net, pairing=True):
    """kin_pfa_pattern_host of a FlatNetwork, computed on the host (no device): (rowptr[N + 1], colidx[pairs], info) - the CSR of
    the path-flux-analysis pattern E2 (the DRG edges and every two-hop pair; 0-based, sorted columns, no diagonal) and a dict
    of the PFA_INFO sizes: the edges of E, the pairs of E2, the products per state and the largest row of E."""
    return _pattern_host("kin_pfa_pattern_host", PFA_INFO, 1, net, pairing)


TIMESCALE_INFO = ("nnz", "rows_short", "rows_medium", "rows_long")
# classes of the timescale row pass by stored entries of a Jacobian row (timescale.hpp: TS_SHORT_MAX, TS_WAVE_MAX), and the
# entries a workgroup takes per pass of a long row or a long contribution list (TS_WG * TS_LONG_NX)
TIMESCALE_SHORT_MAX, TIMESCALE_WAVE_MAX, TIMESCALE_LONG_PASS = 8, 256, 1024


def timescale_plan_host(net):
    """kin_timescale_plan_host of a FlatNetwork, computed on the host (no device): a dict of the TIMESCALE_INFO sizes - the
    stored entries of the Jacobian and its rows by class of the row pass (<= 8, 9 .. 256, > 256 stored entries)."""
    info = np.zeros(len(TIMESCALE_INFO), np.int64)
    st = lib().kin_timescale_plan_host(*_net_head(net), _p64(info))
    if st != KIN_OK:
        raise KineticaHipError(st, "network has no timescale plan")
    return {k: int(v) for k, v in zip(TIMESCALE_INFO, info)}


FLUX_PLAN_INFO = ("path", "rows", "parts", "G", "k_mode", "rates_mode")
FLUX_K16, FLUX_K8, FLUX_T = 0, 1, 2      # k modes of the flux kernels (flux_kernels.hpp: FluxMode)


def flux_plan_host(n_species, n_reactions, B, n_cu, temperature_form=False, segmented=False, k_stride=None, u_bits=0, k_bits=0,
                   rates_bits=None):
    """kin_flux_plan_host (no device, no handle): a dict of the FLUX_PLAN_INFO values - the instantiation and grid a call of the
    per-state flux pass (segmented: of the segmented pass, B = S L) takes on a device of n_cu compute units. k_stride: doubles
    between k rows (None: n_reactions, 0: one shared row); u_bits / k_bits / rates_bits: the low four address bits of the
    buffers (rates_bits None: no per-state rates). Reads KIN_FLUX_LDS / KIN_FLUX_ROWS as a real call does."""
    info = np.zeros(len(FLUX_PLAN_INFO), np.int64)
    st = lib().kin_flux_plan_host(int(n_species), int(n_reactions), int(B), int(n_cu), int(bool(temperature_form)), int(bool(segmented)),
                                  int(n_reactions if k_stride is None else k_stride), int(u_bits), int(k_bits),
                                  -1 if rates_bits is None else int(rates_bits), _p64(info))
    if st != KIN_OK:
        raise KineticaHipError(st, "flux plan query: argument out of range")
    return {k: int(v) for k, v in zip(FLUX_PLAN_INFO, info)}


SWEEP_PLAN_INFO = ("kernel", "BS", "TR", "ILP", "BLK", "ADJ", "U_IN_LDS", "n_a", "n_b", "grid", "per_cu", "n_copy", "n_expl",
                   "tail_tiles", "tail_by_species", "lds_bytes", "n_tiles", "hubs", "records")
SWEEP_KERNELS = ("reg", "gen", "lds", "big", "per_state")      # sweep_plan.hpp: SweepKernel
TILED_PLAN_INFO = ("BS", "TMODE", "UN", "SINGLES", "NB", "grid", "per_cu", "lds_bytes", "identity", "windows", "n_copy",
                   "has_singles")


def _plan_dict(names, info):
    d = {k: int(v) for k, v in zip(names, info)}
    if "kernel" in d:
        d["kernel"] = SWEEP_KERNELS[d["kernel"]]
    return d


def sweep_plan_host(net, n_cu, B, u_bits=0, k_bits=0, du_bits=0):
    """kin_sweep_plan_host (no device, no handle): a dict of the SWEEP_PLAN_INFO values - the kernel instantiation and launch
    configuration kin_rhs_batched_dev takes for a FlatNetwork on a device of n_cu compute units; u_bits / k_bits / du_bits are
    the low four address bits of the buffers."""
    info = np.zeros(len(SWEEP_PLAN_INFO), np.int64)
    st = lib().kin_sweep_plan_host(*_net_head(net), int(n_cu), int(B), int(u_bits), int(k_bits), int(du_bits), _p64(info))
    if st != KIN_OK:
        raise KineticaHipError(st, "sweep plan query: " + lib().kin_last_error(None).decode())
    return _plan_dict(SWEEP_PLAN_INFO, info)


def tiled_sweep_plan_host(net, n_cu, B, temperature_form=False):
    """kin_tiled_sweep_plan_host (no device, no handle): a dict of the TILED_PLAN_INFO values for a FlatNetwork (under the
    caller's KIN_TILED_ENTRIES / KIN_TILED_SINGLES, as a handle would build the layout)."""
    info = np.zeros(len(TILED_PLAN_INFO), np.int64)
    st = lib().kin_tiled_sweep_plan_host(*_net_head(net), int(n_cu), int(B), int(bool(temperature_form)), _p64(info))
    if st != KIN_OK:
        raise KineticaHipError(st, "network has no tiled layout")
    return _plan_dict(TILED_PLAN_INFO, info)


def arrhenius_eval(Ea, A, T, k_max=None, t_mult=1.0):
    """calculator(; T) on the device without a network handle."""
    Ea, A = _f64(Ea), _f64(A)
    out = np.empty(len(Ea))
    st = lib().kin_arrhenius_eval(_pd(Ea), _pd(A), len(Ea), float("nan") if k_max is None else k_max, t_mult, T, _pd(out))
    if st != KIN_OK:
        raise KineticaHipError(st, lib().kin_last_error(None).decode())
    return out


class HipNetwork:
    """Owning wrapper of a kin_network handle."""

    def __init__(self, n_species, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base=0):
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto)]
        self._h = c_void_p()
        st = lib().kin_network_create(int(n_species), len(arrs[0]) - 1, *[_p64(a) for a in arrs], index_base,
                                      ctypes.byref(self._h))
        if st != KIN_OK:
            raise KineticaHipError(st, lib().kin_last_error(None).decode())
        self.n = int(n_species)
        self.nr = len(arrs[0]) - 1
        self.index_base = int(index_base)

    @classmethod
    def from_flat(cls, net):
        return cls(net.n_species, net.reac_ptr, net.reac_idx, net.reac_sto, net.prod_ptr, net.prod_idx, net.prod_sto)

    def close(self):
        if getattr(self, "_h", None):
            lib().kin_network_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: module globals may already be gone
            pass

    def _chk(self, st):
        if st != KIN_OK:
            raise KineticaHipError(st, lib().kin_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def compute_units(self):
        """kin_network_compute_units: compute units of the handle's device (the n_cu of flux_plan_host)."""
        n = c_int(0)
        self._chk(lib().kin_network_compute_units(self._h, ctypes.byref(n)))
        return n.value

    # --- rates -------------------------------------------------------------------------
    def set_rates(self, k):
        k = _f64(k)
        assert len(k) == self.nr
        self._chk(lib().kin_set_rates(self._h, _pd(k)))

    def get_rates(self):
        out = np.empty(self.nr)
        self._chk(lib().kin_get_rates(self._h, _pd(out)))
        return out

    def set_arrhenius(self, Ea, A, k_max=None, t_mult=1.0):
        Ea, A = _f64(Ea), _f64(A)
        assert len(Ea) == self.nr and len(A) == self.nr
        self._chk(lib().kin_set_arrhenius(self._h, _pd(Ea), _pd(A), float("nan") if k_max is None else k_max, t_mult))

    def rates_at(self, T):
        out = np.empty(self.nr)
        self._chk(lib().kin_rates_at(self._h, float(T), _pd(out)))
        return out

    def rate_table(self, T_stops, fetch=True):
        T_stops = _f64(T_stops)
        out = np.empty((len(T_stops), self.nr)) if fetch else None
        self._chk(lib().kin_rate_table(self._h, _pd(T_stops), len(T_stops), _pd(out)))
        return out

    # --- RHS / Jacobian ------------------------------------------------------------------
    def rhs(self, u):
        u = _f64(u)
        assert len(u) == self.n
        du = np.empty(self.n)
        self._chk(lib().kin_rhs(self._h, _pd(u), _pd(du)))
        return du

    def rhs_batched(self, u, k=None):
        u = _f64(u)
        B = u.shape[0]
        assert u.shape == (B, self.n)
        if k is not None:
            k = _f64(k)
            assert k.shape == (B, self.nr)
        du = np.empty((B, self.n))
        self._chk(lib().kin_rhs_batched(self._h, B, _pd(u), _pd(k), _pd(du)))
        return du

    def rhs_batched_dev(self, B, d_u, d_k, d_du, stream=0):
        """Device pointers (ints), state-major u[b][N], k[b][R] or 0, du[b][N]; only enqueues."""
        self._chk(lib().kin_rhs_batched_dev(self._h, int(B), c_void_p(d_u), _dp(d_k),
                                            c_void_p(d_du), _dp(stream)))

    def sweep_plan(self, B, d_u, d_k, d_du):
        """kin_sweep_plan: what rhs_batched_dev launches for these device pointers (ints; d_k 0: the handle's rates)."""
        info = np.zeros(len(SWEEP_PLAN_INFO), np.int64)
        self._chk(lib().kin_sweep_plan(self._h, int(B), c_void_p(d_u), _dp(d_k), c_void_p(d_du), _p64(info)))
        return _plan_dict(SWEEP_PLAN_INFO, info)

    def tiled_sweep_plan(self, B, temperature_form=False):
        """kin_tiled_sweep_plan: the tiled sweep's instantiation and grid for B states on this handle's device."""
        info = np.zeros(len(TILED_PLAN_INFO), np.int64)
        self._chk(lib().kin_tiled_sweep_plan(self._h, int(B), int(bool(temperature_form)), _p64(info)))
        return _plan_dict(TILED_PLAN_INFO, info)

    # --- where the states of an analysis pass come from: (B, the C arguments that hand them over) ----------------------------
    def _batched(self, u):
        """Host states u[B][N]: the entry takes B, u."""
        u = np.ascontiguousarray(np.atleast_2d(_f64(u)))
        B = u.shape[0]
        assert u.shape == (B, self.n)
        return B, (B, _pd(u))

    def _solution(self):
        """The saved states of the last solve, read where they live: B = n_saved, nothing to hand over."""
        n_saved = c_int64(0)
        self._chk(lib().kin_solution_size(self._h, ctypes.byref(n_saved), None))
        return n_saved.value, ()

    def _stored_ensemble(self):
        """Every row of every member of the stored ensemble: B = K n_rows, nothing to hand over."""
        K, rows = self.ensemble_size()[:2]
        return K * rows, ()

    def _k_args(self, B, k, k_row, T):
        """The C arguments (k, n_k_rows, k_row, T) of a pass over B states: contiguous float64 / int64, shapes checked against B."""
        n_rows = 0
        if k is not None:
            k = np.ascontiguousarray(np.atleast_2d(_f64(k)))
            assert k.ndim == 2 and k.shape[1] == self.nr
            n_rows = k.shape[0]
        if k_row is not None:
            k_row = np.ascontiguousarray(k_row, dtype=np.int64).ravel()
            assert len(k_row) == B
        if T is not None:
            T = np.ascontiguousarray(_f64(T).ravel())
            assert len(T) == B
        return _pd(k), n_rows, _p64(k_row), _pd(T)

    def _pattern_nnz(self, entry, pairing):
        """Entries of the handle's kin_drg_pattern / kin_pfa_pattern (no device call)."""
        nnz = c_int64(0)
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), 0, ctypes.byref(nnz), None, None))
        return nnz.value

    def _pattern(self, entry, pairing):
        nnz = self._pattern_nnz(entry, pairing)
        rowptr, colidx = np.empty(self.n + 1, np.int64), np.empty(max(nnz, 1), np.int64)
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), 0, None, _p64(rowptr), _p64(colidx)))
        return rowptr, colidx[:nnz]

    # --- reaction fluxes ---------------------------------------------------------------------
    @staticmethod
    def _weights(B, w):
        if w is not None:
            w = np.ascontiguousarray(_f64(w).ravel())
            assert len(w) == B
        return _pd(w)

    def _flux(self, entry, states, k, k_row, T, w, want_rates, want_flux):
        B, given = states
        ks = self._k_args(B, k, k_row, T)
        w = self._weights(B, w)
        flux = np.empty(self.nr) if want_flux else None
        rates = np.empty((B, self.nr)) if want_rates else None
        args = given + ks + (w,) if given else (w,) + ks      # (kin_solution_flux takes w before the rate constants)
        self._chk(getattr(lib(), entry)(self._h, *args, _pd(flux), _pd(rates)))
        return (flux, rates) if want_rates else flux

    def flux_batched(self, u, k=None, k_row=None, T=None, w=None, want_rates=False, want_flux=True):
        """kin_flux_batched on host arrays: per-reaction rates of the states u[B][N], rate_r = k_r u[x0_r] u[x1_r], and their
        weighted sum flux[R] = sum_b w[b] rate_r(u_b) (w=None: weights 1). Rate constants of state b: row k_row[b] of k
        (k_row=None: row b), or the Arrhenius law at T[b], or the handle's current rates. Returns flux[R], or
        (flux, rates[B][R]) with want_rates (flux is None with want_flux=False)."""
        return self._flux("kin_flux_batched", self._batched(u), k, k_row, T, w, want_rates, want_flux)

    def flux_batched_dev(self, B, d_u, d_k=0, d_k_row=0, d_T=0, d_w=0, d_flux=0, d_rates=0, stream=0):
        """kin_flux_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B], w[B],
        flux[R] and / or rates[B][R]. One stream per handle at a time; allocates only when the workspace has to grow."""
        self._chk(lib().kin_flux_batched_dev(self._h, int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T), _dp(d_w), _dp(d_flux),
                                             _dp(d_rates), _dp(stream)))

    def solution_flux(self, w=None, k=None, k_row=None, T_rows=None, want_rates=False, want_flux=True):
        """kin_solution_flux: flux_batched over the saved states of the last solve, read where they live on the device.
        k=None with k_row reads rows of the device-resident rate table (solve(k_table=...) / rate_table leave it there)."""
        return self._flux("kin_solution_flux", self._solution(), k, k_row, T_rows, w, want_rates, want_flux)

    def flux_segmented(self, u, seg_n=None, k=None, k_row=None, T=None, w=None):
        """kin_flux_segmented on host arrays: u[S][L][N] (S segments of up to L states), flux[S][R] with
        flux[s] = sum over j < seg_n[s] of w[s][j] rate(u[s][j]) - one launch, every segment summed in row order by a workgroup
        of its own (bit-identical whatever else the call holds). seg_n[S] (None: L rows each); rate constants of a state as in
        flux_batched with k_row / T / w of shape [S][L] (entries of rows j >= seg_n[s] are ignored)."""
        u = np.ascontiguousarray(_f64(u))
        assert u.ndim == 3 and u.shape[2] == self.n
        S, Lr = u.shape[0], u.shape[1]
        if seg_n is not None:
            seg_n = np.ascontiguousarray(seg_n, dtype=np.int64).ravel()
            assert len(seg_n) == S
        ks = self._k_args(S * Lr, k, k_row, T)
        flux = np.empty((S, self.nr))
        self._chk(lib().kin_flux_segmented(self._h, S, Lr, _p64(seg_n), _pd(u), *ks, self._weights(S * Lr, w), _pd(flux)))
        return flux

    def flux_segmented_dev(self, S, L, d_u, d_flux, d_seg_n=0, d_k=0, d_k_row=0, d_T=0, d_w=0, stream=0):
        """kin_flux_segmented_dev: device pointers (ints; 0 = not given), u[S L][N], seg_n[S] (int64), k rows / k_row[S L] (int64)
        / T[S L], w[S L], flux[S][R]. Only enqueues; one stream per handle at a time."""
        self._chk(lib().kin_flux_segmented_dev(self._h, int(S), int(L), _dp(d_seg_n), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T), _dp(d_w),
                                               _dp(d_flux), _dp(stream)))

    # --- the last ensemble call's saved states, analysed where they live ------------------------
    def ensemble_size(self):
        """kin_ensemble_size: (K, n_rows, n_species, n_saved[K]) of the stored ensemble (KIN_ERR_STATE without one)."""
        K, rows, n = c_int64(0), c_int64(0), c_int64(0)
        self._chk(lib().kin_ensemble_size(self._h, ctypes.byref(K), ctypes.byref(rows), ctypes.byref(n), None))
        ns = np.zeros(K.value, np.int64)
        self._chk(lib().kin_ensemble_size(self._h, None, None, None, _p64(ns)))
        return K.value, rows.value, n.value, ns

    def ensemble_max(self):
        """kin_ensemble_max: umax[K][N], every member's maximum over its own saved rows."""
        K = self.ensemble_size()[0]
        out = np.empty((K, self.n))
        self._chk(lib().kin_ensemble_max(self._h, _pd(out)))
        return out

    def ensemble_dot(self, w):
        """kin_ensemble_dot: out[K][n_rows] = sum_i w[i] u_m(t_j)[i], zeros past a member's saved rows."""
        w = _f64(w)
        assert len(w) == self.n
        K, rows = self.ensemble_size()[:2]
        out = np.empty((K, rows))
        self._chk(lib().kin_ensemble_dot(self._h, _pd(w), _pd(out)))
        return out

    def ensemble_flux(self, w=None, k=None, k_row=None, T_rows=None):
        """kin_ensemble_flux: flux[K][R] of every member of the stored ensemble, the segmented pass over the saved states where
        they live. w / k_row / T_rows: [K][n_rows] (entries past a member's saved rows are ignored); k: rows for k_row to
        index, or one row per (member, row); none of k / T_rows: the handle's current rates."""
        K, rows = self.ensemble_size()[:2]
        ks = self._k_args(K * rows, k, k_row, T_rows)
        flux = np.empty((K, self.nr))
        self._chk(lib().kin_ensemble_flux(self._h, self._weights(K * rows, w), *ks, _pd(flux)))
        return flux

    # --- directed relation graph ---------------------------------------------------------------
    def drg_pattern(self, pairing=True):
        """kin_drg_pattern: (rowptr[N + 1], colidx[edges]) of the handle's directed relation graph, 0-based (no device call)."""
        return self._pattern("kin_drg_pattern", pairing)

    def _drg(self, entry, states, k, k_row, T, pairing, coef):
        B, given = states
        ks = self._k_args(B, k, k_row, T)
        nnz = self._pattern_nnz("kin_drg_pattern", pairing)
        out, acc = _acc_buffer(nnz, coef, "coef")
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), *given, *ks, acc, _pd(out)))
        return out[:nnz]

    def drg_batched(self, u, k=None, k_row=None, T=None, pairing=True, coef=None):
        """kin_drg_batched on host arrays: coef[edges] (CSR order of drg_pattern) = max over the states u[B][N] of
        num_AB / den_A, the directed-relation-graph coefficients of the network's records (pairing: a reaction with its exact
        reverse; else every reaction alone). Rate constants of state b as in flux_batched. coef given: its values take part
        in the maximum (the result is returned, the argument is left alone)."""
        return self._drg("kin_drg_batched", self._batched(u), k, k_row, T, pairing, coef)

    def drg_batched_dev(self, B, d_u, d_coef, d_k=0, d_k_row=0, d_T=0, pairing=True, accumulate=False, stream=0):
        """kin_drg_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B], coef[edges].
        One stream per handle at a time; allocates only when the workspace has to grow."""
        self._chk(lib().kin_drg_batched_dev(self._h, int(bool(pairing)), int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T),
                                            1 if accumulate else 0, _dp(d_coef), _dp(stream)))

    def solution_drg(self, k=None, k_row=None, T_rows=None, pairing=True, coef=None):
        """kin_solution_drg: drg_batched over the saved states of the last solve, read where they live on the device
        (rate-constant sources as solution_flux)."""
        return self._drg("kin_solution_drg", self._solution(), k, k_row, T_rows, pairing, coef)

    def ensemble_drg(self, k=None, k_row=None, T_rows=None, pairing=True, coef=None):
        """kin_ensemble_drg: one graph over every saved row of every member of the stored ensemble (k_row / T_rows: [K][n_rows],
        entries past a member's saved rows are ignored)."""
        return self._drg("kin_ensemble_drg", self._stored_ensemble(), k, k_row, T_rows, pairing, coef)

    # --- DRG with error propagation -----------------------------------------------------------
    def _drgep(self, entry, states, targets, k, k_row, T, pairing, importance, stages=None):
        """stages: None for an entry without the stage outputs (the stored forms)."""
        B, given = states
        ks = self._k_args(B, k, k_row, T)
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).ravel())
        out, acc = _acc_buffer(self.n, importance, "importance")
        shown = () if stages is None else (None, None, None)
        if stages:
            shown = (np.zeros((B, self._pattern_nnz("kin_drg_pattern", pairing))), np.zeros((B, self.n)), np.zeros(B, np.int32))
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), *given, *ks, _p64(tg), len(tg), 0, acc, _pd(out),
                                        *[(_p32 if i == 2 else _pd)(_nonempty(a)) for i, a in enumerate(shown)]))
        return (out[:self.n], *shown) if stages else out[:self.n]

    def drgep_batched(self, u, targets, k=None, k_row=None, T=None, pairing=True, importance=None, stages=False):
        """kin_drgep_batched on host arrays: importance[N] = max over the states u[B][N] of R_B, the largest product of the
        direct-interaction coefficients r_AB along any path from a target (0-based ids) to B (include/kinetica_hip.h has the
        definition). Rate constants of state b as in flux_batched. importance given: its values take part in the maximum (the
        result is returned, the argument is left alone). stages=True: (importance, r[B][edges], R[B][N], rounds[B])."""
        return self._drgep("kin_drgep_batched", self._batched(u), targets, k, k_row, T, pairing, importance, bool(stages))

    def drgep_batched_dev(self, B, d_u, d_targets, n_targets, d_importance, d_k=0, d_k_row=0, d_T=0, pairing=True, accumulate=False,
                          stream=0):
        """kin_drgep_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B],
        targets[n_targets] (int64, 0-based), importance[N]. One stream per handle at a time."""
        self._chk(lib().kin_drgep_batched_dev(self._h, int(bool(pairing)), int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T),
                                              _dp(d_targets), int(n_targets), 1 if accumulate else 0, _dp(d_importance), _dp(stream)))

    def drgep_paths(self, r, targets, pairing=True, importance=None, stages=False):
        """kin_drgep_paths: the path search alone on the caller's coefficients r[B][edges] in [0, 1] (CSR order of drg_pattern).
        stages=True: (importance, R[B][N], rounds[B])."""
        E = self._pattern_nnz("kin_drg_pattern", pairing)
        r = np.ascontiguousarray(_f64(r)).reshape(-1, E) if E else np.zeros((len(r), 0))
        B = r.shape[0]
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.int64).ravel())
        out, acc = _acc_buffer(self.n, importance, "importance")
        R, rounds = np.zeros((B, self.n)), np.zeros(B, np.int32)
        self._chk(lib().kin_drgep_paths(self._h, int(bool(pairing)), B, _pd(_nonempty(r)), _p64(tg), len(tg), 0, acc, _pd(out),
                                        _pd(_nonempty(R)) if stages else None, _p32(_nonempty(rounds)) if stages else None))
        return (out[:self.n], R, rounds) if stages else out[:self.n]

    def solution_drgep(self, targets, k=None, k_row=None, T_rows=None, pairing=True, importance=None):
        """kin_solution_drgep: drgep_batched over the saved states of the last solve, read where they live on the device
        (rate-constant sources as solution_flux)."""
        return self._drgep("kin_solution_drgep", self._solution(), targets, k, k_row, T_rows, pairing, importance)

    def ensemble_drgep(self, targets, k=None, k_row=None, T_rows=None, pairing=True, importance=None):
        """kin_ensemble_drgep: one importance vector over every saved row of every member of the stored ensemble (k_row / T_rows:
        [K][n_rows], entries past a member's saved rows are ignored)."""
        return self._drgep("kin_ensemble_drgep", self._stored_ensemble(), targets, k, k_row, T_rows, pairing, importance)

    # --- reaction elimination -------------------------------------------------------------------------
    def _reaction_importance(self, entry, states, species, k, k_row, T, pairing, importance, per_state=None):
        """per_state: None for an entry without the per-state output (the stored forms)."""
        B, given = states
        ks = self._k_args(B, k, k_row, T)
        sp, ns, _ = self._ms_species(species)
        out, acc = _acc_buffer(self.nr, importance, "importance")
        shown = () if per_state is None else (np.zeros((B, self.nr)) if per_state else None,)
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), *given, *ks, _p64(sp), ns, 0, acc, _pd(out),
                                        *[_pd(_nonempty(a)) for a in shown]))
        return (out[:self.nr], *shown) if per_state else out[:self.nr]

    def reaction_importance_batched(self, u, species=None, pairing=True, importance=None, per_state=False, k=None, k_row=None, T=None):
        """kin_reaction_importance_batched on host arrays: importance[R] = max over the states u[B][N] of the largest share
        |nu_A| |w| / den_A a reaction's record holds of the turnover of any species A it changes (include/kinetica_hip.h has
        the definition) - A among `species` (0-based ids; None: every species), den_A always over the whole network. Rate
        constants of state b as in flux_batched. importance given: its values take part in the maximum (the result is
        returned, the argument is left alone). per_state=True: (importance, I[B][R])."""
        return self._reaction_importance("kin_reaction_importance_batched", self._batched(u), species, k, k_row, T, pairing, importance,
                                         bool(per_state))

    def reaction_importance_batched_dev(self, B, d_u, d_importance, d_species=0, n_sel=0, d_k=0, d_k_row=0, d_T=0, pairing=True,
                                        accumulate=False, stream=0):
        """kin_reaction_importance_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B],
        species[n_sel] (int64, 0-based; 0: every species), importance[R]. One stream per handle at a time."""
        self._chk(lib().kin_reaction_importance_batched_dev(self._h, int(bool(pairing)), int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T),
                                                            _dp(d_species), int(n_sel), 1 if accumulate else 0, _dp(d_importance),
                                                            _dp(stream)))

    def solution_reaction_importance(self, species=None, k=None, k_row=None, T_rows=None, pairing=True, importance=None):
        """kin_solution_reaction_importance: reaction_importance_batched over the saved states of the last solve, read where
        they live on the device (rate-constant sources as solution_flux)."""
        return self._reaction_importance("kin_solution_reaction_importance", self._solution(), species, k, k_row, T_rows, pairing,
                                         importance)

    def ensemble_reaction_importance(self, species=None, k=None, k_row=None, T_rows=None, pairing=True, importance=None):
        """kin_ensemble_reaction_importance: one importance vector over every saved row of every member of the stored ensemble
        (k_row / T_rows: [K][n_rows], entries past a member's saved rows are ignored)."""
        return self._reaction_importance("kin_ensemble_reaction_importance", self._stored_ensemble(), species, k, k_row, T_rows, pairing,
                                         importance)

    # --- path flux analysis ------------------------------------------------------------------------
    def pfa_pattern(self, pairing=True):
        """kin_pfa_pattern: (rowptr[N + 1], colidx[pairs]) of the handle's path-flux-analysis pattern E2, 0-based (no device call)."""
        return self._pattern("kin_pfa_pattern", pairing)

    def _pfa_buffer(self, pairing, coef):
        """(pairs, buffer, accumulate) of a PFA entry; a coef of another length is this pass's KIN_ERR_INVALID_ARG."""
        nnz = self._pattern_nnz("kin_pfa_pattern", pairing)
        if coef is not None and np.size(coef) != nnz:
            raise KineticaHipError(KIN_ERR_INVALID_ARG, f"coef has {np.size(coef)} entries, the PFA pattern {nnz} pairs")
        return (nnz,) + _acc_buffer(nnz, coef, "coef")

    def _pfa(self, entry, states, k, k_row, T, pairing, coef, stages=None):
        """stages: None for an entry without the stage outputs (the stored forms)."""
        B, given = states
        ks = self._k_args(B, k, k_row, T)
        nnz, out, acc = self._pfa_buffer(pairing, coef)
        shown = () if stages is None else (None, None, None)
        if stages:
            E = self._pattern_nnz("kin_drg_pattern", pairing)
            shown = (np.zeros((B, E)), np.zeros((B, E)), np.zeros((B, nnz)))
        self._chk(getattr(lib(), entry)(self._h, int(bool(pairing)), *given, *ks, acc, _pd(out), *[_pd(_nonempty(a)) for a in shown]))
        return (out[:nnz], *shown) if stages else out[:nnz]

    def pfa_batched(self, u, k=None, k_row=None, T=None, pairing=True, coef=None, stages=False):
        """kin_pfa_batched on host arrays: coef[pairs] (CSR order of pfa_pattern) = max over the states u[B][N] of
        r_AB = rp_AB + rc_AB + sum_M (rp_AM rp_MB + rc_AM rc_MB), the path-flux-analysis coefficients (include/kinetica_hip.h has
        the definition). Rate constants of state b as in flux_batched. coef given: its values take part in the maximum (the
        result is returned, the argument is left alone). stages=True: (coef, rp[B][edges], rc[B][edges], r[B][pairs])."""
        return self._pfa("kin_pfa_batched", self._batched(u), k, k_row, T, pairing, coef, bool(stages))

    def pfa_batched_dev(self, B, d_u, d_coef, d_k=0, d_k_row=0, d_T=0, pairing=True, accumulate=False, stream=0):
        """kin_pfa_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B], coef[pairs].
        One stream per handle at a time; allocates only when the workspace has to grow."""
        self._chk(lib().kin_pfa_batched_dev(self._h, int(bool(pairing)), int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T),
                                            1 if accumulate else 0, _dp(d_coef), _dp(stream)))

    def pfa_paths(self, rp, rc, pairing=True, coef=None, stages=False):
        """kin_pfa_paths: the second-generation stage alone on the caller's coefficients rp[B][edges], rc[B][edges] >= 0 (CSR
        order of drg_pattern). stages=True: (coef, r[B][pairs])."""
        E = self._pattern_nnz("kin_drg_pattern", pairing)
        rp, rc = (np.ascontiguousarray(_f64(x)).reshape(-1, E) if E else np.zeros((len(x), 0)) for x in (rp, rc))
        B = rp.shape[0]
        assert rc.shape == rp.shape
        nnz, out, acc = self._pfa_buffer(pairing, coef)
        r = np.zeros((B, nnz))
        self._chk(lib().kin_pfa_paths(self._h, int(bool(pairing)), B, _pd(_nonempty(rp)), _pd(_nonempty(rc)), acc, _pd(out),
                                      _pd(_nonempty(r)) if stages else None))
        return (out[:nnz], r) if stages else out[:nnz]

    def solution_pfa(self, k=None, k_row=None, T_rows=None, pairing=True, coef=None):
        """kin_solution_pfa: pfa_batched over the saved states of the last solve, read where they live on the device
        (rate-constant sources as solution_flux)."""
        return self._pfa("kin_solution_pfa", self._solution(), k, k_row, T_rows, pairing, coef)

    def ensemble_pfa(self, k=None, k_row=None, T_rows=None, pairing=True, coef=None):
        """kin_ensemble_pfa: one set of coefficients over every saved row of every member of the stored ensemble (k_row / T_rows:
        [K][n_rows], entries past a member's saved rows are ignored)."""
        return self._pfa("kin_ensemble_pfa", self._stored_ensemble(), k, k_row, T_rows, pairing, coef)

    # --- timescale analysis ---------------------------------------------------------------------
    def _jac_nnz(self):
        nnz = c_int64(0)
        self._chk(lib().kin_jac_nnz(self._h, ctypes.byref(nnz)))
        return nnz.value

    def _summary(self, summary):
        """(summary[3][N], accumulate) of a timescale entry: a fresh buffer, or a copy of `summary` that takes part."""
        assert summary is None or _f64(summary).shape == (3, self.n)
        out, acc = _acc_buffer(3 * self.n, summary, "summary")
        return out[:3 * self.n].reshape(3, self.n), acc

    def jac_batched(self, u, k=None, k_row=None, T=None):
        """kin_jac_batched on host arrays: vals[B][nnz], the Jacobian values of the states u[B][N] in the CSR order of
        jac_pattern. Rate constants of state b as in flux_batched."""
        B, given = self._batched(u)
        ks = self._k_args(B, k, k_row, T)
        vals = np.empty((B, self._jac_nnz()))
        self._chk(lib().kin_jac_batched(self._h, *given, *ks, _pd(vals)))
        return vals

    def jac_batched_dev(self, B, d_u, d_vals, d_k=0, d_k_row=0, d_T=0, stream=0):
        """kin_jac_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B], vals[B][nnz].
        One stream per handle at a time; allocates only when the workspace has to grow."""
        self._chk(lib().kin_jac_batched_dev(self._h, int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T), _dp(d_vals), _dp(stream)))

    def timescale_batched(self, u, k=None, k_row=None, T=None, summary=None, want_summary=True, want_diag=False, want_err=False,
                          want_norm=True):
        """kin_timescale_batched on host arrays, over the states u[B][N]: a dict of the outputs asked for - summary[3][N] (rows
        decay_max = max_b -J_ii, decay_min = min_b -J_ii, qss_err = max_b |f_i| / |J_ii|), diag[B][N] = J_ii, err[B][N] =
        |f_i| / |J_ii|, norm[B] = the infinity norm of J(u_b). Rate constants of state b as in flux_batched. summary given: its
        values take part in the extrema (the result is returned, the argument is left alone)."""
        B, given = self._batched(u)
        ks = self._k_args(B, k, k_row, T)
        out, acc = self._summary(summary) if want_summary else (None, 0)
        diag = np.empty((B, self.n)) if want_diag else None
        err = np.empty((B, self.n)) if want_err else None
        norm = np.empty(B) if want_norm else None
        self._chk(lib().kin_timescale_batched(self._h, *given, *ks, acc, _pd(out), _pd(diag), _pd(err), _pd(norm)))
        return {q: v for q, v in (("summary", out), ("diag", diag), ("err", err), ("norm", norm)) if v is not None}

    def timescale_batched_dev(self, B, d_u, d_summary=0, d_diag=0, d_err=0, d_norm=0, d_k=0, d_k_row=0, d_T=0, accumulate=False, stream=0):
        """kin_timescale_batched_dev: device pointers (ints; 0 = not given), u[B][N], k rows / k_row[B] (int64) / T[B],
        summary[3][N], diag[B][N], err[B][N], norm[B]. One stream per handle at a time."""
        self._chk(lib().kin_timescale_batched_dev(self._h, int(B), _dp(d_u), _dp(d_k), _dp(d_k_row), _dp(d_T), 1 if accumulate else 0,
                                                  _dp(d_summary), _dp(d_diag), _dp(d_err), _dp(d_norm), _dp(stream)))

    def _timescale(self, entry, shape, k, k_row, T, row_begin, summary, want_norm):
        """A stored form of the pass; `shape`: of its states, and of their norms."""
        ks = self._k_args(int(np.prod(shape)), k, k_row, T)
        out, acc = self._summary(summary)
        norm = np.empty(shape) if want_norm else None
        self._chk(getattr(lib(), entry)(self._h, *ks, int(row_begin), acc, _pd(out), _pd(norm)))
        return out, norm

    def solution_timescale(self, k=None, k_row=None, T_rows=None, row_begin=0, summary=None, want_norm=True):
        """kin_solution_timescale: timescale_batched over the saved states of the last solve from row_begin on, read where they
        live on the device (rate-constant sources as solution_flux). Returns (summary[3][N], norm[n_saved] or None); the norm
        of a row below row_begin is 0.0."""
        return self._timescale("kin_solution_timescale", self._solution()[:1], k, k_row, T_rows, row_begin, summary, want_norm)

    def ensemble_timescale(self, k=None, k_row=None, T_rows=None, row_begin=0, summary=None, want_norm=True):
        """kin_ensemble_timescale: one summary over the saved rows row_begin .. n_saved[m] - 1 of every member of the stored
        ensemble (k_row / T_rows: [K][n_rows], entries of rows that take no part are ignored). Returns (summary[3][N],
        norm[K][n_rows] or None); the norm of a row that takes no part is 0.0."""
        return self._timescale("kin_ensemble_timescale", self.ensemble_size()[:2], k, k_row, T_rows, row_begin, summary, want_norm)

    # --- cross-member statistics ------------------------------------------------------------------
    def _ms_species(self, species):
        """(species int64 or None, n_sel as the C entries take it, number of selected species)."""
        if species is None:
            return None, 0, self.n
        sp = np.ascontiguousarray(np.asarray(species, dtype=np.int64).ravel())
        ns = len(sp)
        return (sp if ns else np.zeros(1, np.int64)), ns, ns      # (an empty list stays a list - and an error - not "all species")

    @staticmethod
    def _ms_block(u, n_species):
        u = np.ascontiguousarray(_f64(u))
        if u.ndim != 3 or u.shape[2] != n_species:
            raise ValueError(f"u must be [K][L][{n_species}] (member, row, species); got {u.shape}")
        return u, u.shape[0], u.shape[1]

    def _members(self, u):
        """(K, L, the C arguments that hand the block over): K, L, u of host states u[K][L][N]; nothing of the stored ensemble
        (u None), read where it lives. (The public methods pass _f64(u): a caller's None is a wrong block, as it always was.)"""
        if u is None:
            K, L = self.ensemble_size()[:2]
            return K, L, ()
        u, K, L = self._ms_block(u, self.n)
        return K, L, (K, L, _pd(u))

    def _moments(self, entry, u, use, want):
        K, L, given = self._members(u)
        use = _use32(use, K)
        names = ("mean", "var", "min", "max")
        bad = [w for w in want if w not in names + ("count",)]
        if bad:
            raise ValueError(f"unknown moments {bad}; choose among {names + ('count',)}")
        out = {w: np.empty((L, self.n)) for w in names if w in want}
        cnt = c_int64(0)
        self._chk(getattr(lib(), entry)(self._h, *given, _p32(use), ctypes.byref(cnt), *[_pd(out.get(w)) for w in names]))
        if "count" in want:
            out["count"] = cnt.value
        return out

    def members_moments(self, u, use=None, want=("count", "mean", "var", "min", "max")):
        """kin_members_moments over a block u[K][L][N] on the host: dict of count (int) and mean / var / min / max [L][N] over the
        members use[m] != 0 (None: all), those `want` names (include/kinetica_hip.h has the definitions)."""
        return self._moments("kin_members_moments", _f64(u), use, want)

    def members_moments_dev(self, K, L, d_u, use=None, d_mean=0, d_var=0, d_min=0, d_max=0, stream=0):
        """kin_members_moments_dev: device pointers (ints; 0 = not wanted) u[K][L][N] and mean / var / min / max [L][N]; `use` is a
        host mask. Only enqueues; returns the number of participants."""
        use = _use32(use, K)
        cnt = c_int64(0)
        self._chk(lib().kin_members_moments_dev(self._h, int(K), int(L), _dp(d_u), _p32(use), ctypes.byref(cnt), _dp(d_mean), _dp(d_var),
                                                _dp(d_min), _dp(d_max), _dp(stream)))
        return cnt.value

    def ensemble_moments(self, use=None, want=("count", "mean", "var", "min", "max")):
        """kin_ensemble_moments: members_moments over the stored ensemble, read where it lives (use None: the members that
        completed the save grid)."""
        return self._moments("kin_ensemble_moments", None, use, want)

    def _quantiles(self, entry, u, p, species, use):
        K, L, given = self._members(u)
        use = _use32(use, K)
        p = np.ascontiguousarray(np.atleast_1d(_f64(p)))
        sp, ns, nsel = self._ms_species(species)
        out = np.empty((len(p), L, nsel))
        self._chk(getattr(lib(), entry)(self._h, *given, _p32(use), _p64(sp), ns, _pd(p), len(p), _pd(out)))
        return out

    def members_quantiles(self, u, p, species=None, use=None):
        """kin_members_quantiles: out[Q][L][n_sel], the quantiles p[Q] (in [0, 1]) over the participants of the selected species
        (ids in the handle's index base; None: all N) at every row."""
        return self._quantiles("kin_members_quantiles", _f64(u), p, species, use)

    def members_quantiles_dev(self, K, L, d_u, p, d_out, species=None, use=None, stream=0):
        """kin_members_quantiles_dev: device pointers u[K][L][N] and out[Q][L][n_sel]; p, species and use are host arrays."""
        use = _use32(use, K)
        p = np.ascontiguousarray(np.atleast_1d(_f64(p)))
        sp, ns, _ = self._ms_species(species)
        self._chk(lib().kin_members_quantiles_dev(self._h, int(K), int(L), _dp(d_u), _p32(use), _p64(sp), ns, _pd(p), len(p), _dp(d_out),
                                                  _dp(stream)))

    def ensemble_quantiles(self, p, species=None, use=None):
        """kin_ensemble_quantiles: members_quantiles over the stored ensemble, out[Q][n_rows][n_sel]."""
        return self._quantiles("kin_ensemble_quantiles", None, p, species, use)

    @staticmethod
    def _ms_inputs(X, K):
        X = np.ascontiguousarray(_f64(X))
        if X.ndim != 2 or X.shape[0] != K:
            raise ValueError(f"inputs must be [K = {K}][P] (one row per member); got {X.shape}")
        return X, X.shape[1]

    def _correlate(self, entry, u, X, species, rank, use):
        K, L, given = self._members(u)
        use = _use32(use, K)
        X, P = self._ms_inputs(X, K)
        sp, ns, nsel = self._ms_species(species)
        out = np.empty((L, nsel, P))
        self._chk(getattr(lib(), entry)(self._h, *given, _p32(use), _p64(sp), ns, _pd(X), P, int(bool(rank)), _pd(out)))
        return out

    def members_correlate(self, u, X, species=None, rank=True, use=None):
        """kin_members_correlate: out[L][n_sel][P], the correlation of input X[:, p] (X[K][P], one row per member) with the selected
        species at every row over the participants: Spearman's coefficient (rank=True) or Pearson's."""
        return self._correlate("kin_members_correlate", _f64(u), X, species, rank, use)

    def members_correlate_dev(self, K, L, d_u, X, d_out, species=None, rank=True, use=None, stream=0):
        """kin_members_correlate_dev: device pointers u[K][L][N] and out[L][n_sel][P]; X, species and use are host arrays."""
        use = _use32(use, K)
        X, P = self._ms_inputs(X, K)
        sp, ns, _ = self._ms_species(species)
        self._chk(lib().kin_members_correlate_dev(self._h, int(K), int(L), _dp(d_u), _p32(use), _p64(sp), ns, _pd(X), P, int(bool(rank)),
                                                  _dp(d_out), _dp(stream)))

    def ensemble_correlate(self, X, species=None, rank=True, use=None):
        """kin_ensemble_correlate: members_correlate over the stored ensemble, out[n_rows][n_sel][P]."""
        return self._correlate("kin_ensemble_correlate", None, X, species, rank, use)

    # --- Sobol indices of a Saltelli design ---------------------------------------------------------
    @staticmethod
    def _sobol_weights(w, M):
        """Sample weights as the kin_*_sobol entries take them: int32[M] multiplicities or None (negative ones are the entry's
        KIN_ERR_INVALID_ARG)."""
        if w is None:
            return None
        w = np.asarray(w)
        if w.shape != (M,) or w.dtype.kind not in "iub":
            raise ValueError(f"w must be {M} integer multiplicities, one per base sample; got {w.dtype} {w.shape}")
        return np.ascontiguousarray(w, dtype=np.int32)

    def ensemble_sobol_weights(self, M, P):
        """The default weights of ensemble_sobol: int32[M], 1 where all P + 2 members of sample m completed the save grid."""
        K, L, _, ns = self.ensemble_size()
        if M < 1 or P < 1 or K != M * (P + 2):
            raise KineticaHipError(KIN_ERR_INVALID_ARG, f"the stored ensemble has {K} members, not M (P + 2) = {M * (P + 2)}")
        return np.all(ns.reshape(P + 2, M) == L, axis=0).astype(np.int32)

    def _sobol(self, entry, u, M, P, species, w):
        M, P = int(M), int(P)
        K, L, given = self._members(u)
        if u is not None and M >= 1 and P >= 1 and K != M * (P + 2):
            raise ValueError(f"u must hold M (P + 2) = {M * (P + 2)} members; got {K}")
        w = self._sobol_weights(w, M)
        sp, ns, nsel = self._ms_species(species)
        shape = (L, nsel, max(P, 0))
        out = dict(first=np.empty(shape), total=np.empty(shape), mean=np.empty((L, nsel)), var=np.empty((L, nsel)))
        # (given[1:]: M and P stand for K = M (P + 2), so kin_members_sobol takes L, u after them)
        self._chk(getattr(lib(), entry)(self._h, M, P, *given[1:], _p32(w), _p64(sp), ns,
                                        *[_pd(out[q]) for q in ("first", "total", "mean", "var")]))
        if u is not None:       # count = sum w; of the stored ensemble without w, of the samples whose members all completed the grid
            out["count"] = M if w is None else int(np.maximum(w, 0).sum())
        else:
            out["count"] = int((self.ensemble_sobol_weights(M, P) if w is None else w).sum())
        return out

    def members_sobol(self, u, M, P, species=None, w=None):
        """kin_members_sobol over the Saltelli design u[M (P + 2)][L][N] (member b M + m: sample m of block A, B, AB_0 ..): dict of
        first, total [L][n_sel][P] (S1, ST), mean, var [L][n_sel] (over A and B) and count = sum w. w: int multiplicities per base
        sample (None: all ones); species: ids in the handle's index base (None: all)."""
        return self._sobol("kin_members_sobol", _f64(u), M, P, species, w)

    def members_sobol_dev(self, M, P, L, d_u, d_first=0, d_total=0, d_mean=0, d_var=0, species=None, w=None, stream=0):
        """kin_members_sobol_dev: device pointers (ints; 0 = not wanted) u[M (P + 2)][L][N], first / total [L][n_sel][P] and
        mean / var [L][n_sel]; w and species are host arrays. Only enqueues."""
        w = self._sobol_weights(w, int(M))
        sp, ns, _ = self._ms_species(species)
        self._chk(lib().kin_members_sobol_dev(self._h, int(M), int(P), int(L), _dp(d_u), _p32(w), _p64(sp), ns, _dp(d_first), _dp(d_total),
                                              _dp(d_mean), _dp(d_var), _dp(stream)))

    def ensemble_sobol(self, M, P, species=None, w=None):
        """kin_ensemble_sobol: members_sobol over the stored ensemble, read where it lives (w None: the samples all of whose
        members completed the save grid)."""
        return self._sobol("kin_ensemble_sobol", None, M, P, species, w)

    # --- event times: per-species peak and level-crossing times ----------------------------------------------
    @staticmethod
    def _event_code(value, names, what):
        """A level kind, direction or start by name (ValueError for an unknown one) or as the integer the library takes."""
        if isinstance(value, str):
            if value not in names:
                raise ValueError(f"{what} must be one of {tuple(names)}; got {value!r}")
            return names[value]
        return int(value)

    def _event_opts(self, level, kind, direction, start, row_begin, never, want):
        """(level[N] or None, the C arguments level_kind .. never, the wanted outputs): a scalar level broadcasts to [N]; without
        a level t_cross is not wanted."""
        want = tuple(want)
        bad = [w for w in want if w not in EVENT_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want must name some of {EVENT_OUTPUTS}; got {want}")
        if level is None:
            if "t_cross" in want and want != EVENT_OUTPUTS:
                raise ValueError("t_cross needs a level")
            want = tuple(w for w in want if w != "t_cross")
        else:
            level = np.asarray(level, dtype=np.float64)      # (ascontiguousarray would make a number an array of one)
            if level.ndim == 0:
                level = np.full(self.n, float(level))
            level = np.ascontiguousarray(level.ravel())
            if len(level) != self.n:
                raise ValueError(f"level must be a number or one per species ({self.n}); got {len(level)}")
        codes = (self._event_code(kind, EVENT_KINDS, "kind"), self._event_code(direction, EVENT_DIRECTIONS, "direction"),
                 self._event_code(start, EVENT_STARTS, "start"), int(row_begin), float(never))
        return level, codes, want

    def _event_times(self, t, S, L):
        """(t as float64, the t_per_segment flag): t[L] shared by the S segments, or t[S][L]."""
        t = np.ascontiguousarray(_f64(t))
        if t.shape == (L,):
            return t, 0
        if t.shape == (S, L):
            return t, 1
        raise ValueError(f"t must be [{L}] (one save grid) or [{S}][{L}] (one per segment); got {t.shape}")

    def _events(self, entry, shape, head, level, codes, want):
        out = {w: np.empty(shape) for w in want}
        self._chk(getattr(lib(), entry)(self._h, *head, _pd(level), *codes, *[_pd(out.get(w)) for w in EVENT_OUTPUTS]))
        return out

    def events_segmented(self, u, t, level=None, kind="abs", direction="rise", start="begin", row_begin=0, never=float("nan"),
                         seg_n=None, want=EVENT_OUTPUTS):
        """kin_events_segmented on host arrays: u[S][L][N] (S segments of up to L rows, seg_n[S] of them real; None: L each), times
        t[L] or t[S][L]. Returns a dict of u_peak, t_peak, t_cross [S][N] (those `want` names; without a level no t_cross): the
        maximum over a segment's rows from row_begin on, the time of the first row that holds it, and the time at which the
        species first reaches the level - `level` a number or [N]; kind "abs": the level itself, "of_peak": level x the peak,
        "of_start": level x the value at row_begin; direction "rise" (u >= l) or "fall" (u <= l); start "begin" (search from
        row_begin) or "peak" (from the peak's row) - by the chord between the two rows around the crossing; `never` where no row
        meets the level or the segment is empty (include/kinetica_hip.h has the definitions)."""
        u, S, L = self._ms_block(u, self.n)
        if seg_n is not None:
            seg_n = np.ascontiguousarray(seg_n, dtype=np.int64).ravel()
            if len(seg_n) != S:
                raise ValueError(f"seg_n must have one entry per segment ({S}); got {len(seg_n)}")
        t, flag = self._event_times(t, S, L)
        level, codes, want = self._event_opts(level, kind, direction, start, row_begin, never, want)
        return self._events("kin_events_segmented", (S, self.n), (S, L, _p64(seg_n), _pd(u), _pd(t), flag), level, codes, want)

    def events_segmented_dev(self, S, L, d_u, d_t, d_level=0, kind="abs", direction="rise", start="begin", row_begin=0,
                             never=float("nan"), d_seg_n=0, t_per_segment=False, d_u_peak=0, d_t_peak=0, d_t_cross=0, stream=0):
        """kin_events_segmented_dev: device pointers (ints; 0 = not given / not wanted) u[S][L][N], t[L] (t[S][L] with
        t_per_segment), level[N], seg_n[S] (int64) and u_peak / t_peak / t_cross [S][N]. Only enqueues; one stream per handle
        at a time."""
        codes = (self._event_code(kind, EVENT_KINDS, "kind"), self._event_code(direction, EVENT_DIRECTIONS, "direction"),
                 self._event_code(start, EVENT_STARTS, "start"), int(row_begin), float(never))
        self._chk(lib().kin_events_segmented_dev(self._h, int(S), int(L), _dp(d_seg_n), _dp(d_u), _dp(d_t), int(bool(t_per_segment)),
                                                 _dp(d_level), *codes, _dp(d_u_peak), _dp(d_t_peak), _dp(d_t_cross), _dp(stream)))

    def ensemble_events(self, t, level=None, kind="abs", direction="rise", start="begin", row_begin=0, never=float("nan"),
                        want=EVENT_OUTPUTS):
        """kin_ensemble_events: events_segmented over the stored ensemble, every member's own saved rows read where they live;
        t: the save grid [n_rows] or one per member [K][n_rows]. Returns the dict of [K][N] arrays."""
        K, L = self.ensemble_size()[:2]
        t, flag = self._event_times(t, K, L)
        level, codes, want = self._event_opts(level, kind, direction, start, row_begin, never, want)
        return self._events("kin_ensemble_events", (K, self.n), (_pd(t), flag), level, codes, want)

    def solution_events(self, level=None, kind="abs", direction="rise", start="begin", row_begin=0, never=float("nan"),
                        want=EVENT_OUTPUTS):
        """kin_solution_events: the same over the saved states and times of the last solve, read where they live. Returns the
        dict of [N] arrays."""
        level, codes, want = self._event_opts(level, kind, direction, start, row_begin, never, want)
        return self._events("kin_solution_events", (self.n,), (), level, codes, want)

    # --- resampling: stored trajectories on a common axis ------------------------------------------------------
    @staticmethod
    def _resample_opts(mode, fill, row_begin):
        """The C arguments mode, fill, row_begin; the mode by name (ValueError for an unknown one) or as the library's integer."""
        if isinstance(mode, str):
            if mode not in RESAMPLE_MODES:
                raise ValueError(f"mode must be one of {tuple(RESAMPLE_MODES)}; got {mode!r}")
            mode = RESAMPLE_MODES[mode]
        return int(mode), float(fill), int(row_begin)

    def resample_segmented(self, u, x, xq, seg_n=None, mode="fill", fill=float("nan"), row_begin=0, want_brackets=False):
        """kin_resample_segmented on host arrays: u[S][L][N] (S segments of up to L rows, seg_n[S] of them real; None: L each)
        evaluated at the queries xq[Q] or xq[S][Q] of the axis x[L] or x[S][L] (non-decreasing over the rows read). Returns
        u_q[S][Q][N]: a row copied bit for bit where the axis holds the query, else the chord between the two rows around it;
        a query outside the segment's range gets `fill` (mode "fill") or the segment's first / last row (mode "hold").
        want_brackets: (u_q, jc[S][Q], w[S][Q]) - resample_brackets' pair as the device formed it."""
        u, S, L = self._ms_block(u, self.n)
        seg_n = _seg_n(seg_n, S)
        x, x_per = _axis(x, S, L, "x")
        xq, Q, q_per = _queries(xq, S)
        out = np.empty((S, Q, self.n))
        jc, w = (np.zeros((S, Q), np.int32), np.zeros((S, Q))) if want_brackets else (None, None)
        self._chk(lib().kin_resample_segmented(self._h, S, L, _p64(seg_n), _pd(u), _pd(x), x_per, Q, _pd(xq), q_per,
                                               *self._resample_opts(mode, fill, row_begin), _pd(out), _p32(jc), _pd(w)))
        return (out, jc, w) if want_brackets else out

    def resample_segmented_dev(self, S, L, d_u, d_x, Q, d_xq, d_out, mode="fill", fill=float("nan"), row_begin=0, d_seg_n=0,
                               x_per_segment=False, xq_per_segment=False, d_jc=0, d_w=0, stream=0):
        """kin_resample_segmented_dev: device pointers (ints; 0 = not given / not wanted) u[S][L][N], x[L] (x[S][L] with
        x_per_segment), xq[Q] (xq[S][Q] with xq_per_segment), seg_n[S] (int64), out[S][Q][N], jc[S][Q] (int32), w[S][Q]. Only
        enqueues; one stream per handle at a time."""
        self._chk(lib().kin_resample_segmented_dev(self._h, int(S), int(L), _dp(d_seg_n), _dp(d_u), _dp(d_x), int(bool(x_per_segment)),
                                                   int(Q), _dp(d_xq), int(bool(xq_per_segment)), *self._resample_opts(mode, fill, row_begin),
                                                   _dp(d_out), _dp(d_jc), _dp(d_w), _dp(stream)))

    def solution_resample(self, xq, x=None, mode="fill", fill=float("nan"), row_begin=0):
        """kin_solution_resample: the saved states of the last solve, read where they live, at the queries xq[Q] of the axis
        x[n_saved] (None: the saved times). Returns u_q[Q][N]."""
        xq = np.ascontiguousarray(_f64(xq)).ravel()
        if x is not None:
            x = np.ascontiguousarray(_f64(x)).ravel()
            n = self._solution()[0]
            if len(x) != n:
                raise ValueError(f"x must have one entry per saved row ({n}); got {len(x)}")
        out = np.empty((len(xq), self.n))
        self._chk(lib().kin_solution_resample(self._h, _pd(x), len(xq), _pd(xq), *self._resample_opts(mode, fill, row_begin), _pd(out)))
        return out

    def ensemble_resample(self, x, xq, mode="fill", fill=float("nan"), row_begin=0, store=False, download=True):
        """kin_ensemble_resample: the stored ensemble, every member's own saved rows read where they live, at the queries xq[Q]
        or xq[K][Q] of the axis x[n_rows] or x[K][n_rows]. Returns u_q[K][Q][N], or None with download=False (which needs
        store). store: the result becomes the stored ensemble - Q rows, a member's n_saved the length of its leading run of
        covered queries, zeros from its first uncovered query on - and every ensemble_* method reads it from then on."""
        if not download and not store:
            raise ValueError("download=False needs store=True: the result would go nowhere")
        K, L = self.ensemble_size()[:2]
        x, x_per = _axis(x, K, L, "x")
        xq, Q, q_per = _queries(xq, K)
        out = np.empty((K, Q, self.n)) if download else None
        self._chk(lib().kin_ensemble_resample(self._h, _pd(x), x_per, Q, _pd(xq), q_per, *self._resample_opts(mode, fill, row_begin),
                                              int(bool(store)), _pd(out)))
        return out

    # --- observables: weighted species sums and ratios of stored states ---------------------------------------
    def observables_segmented(self, u, form_ptr, form_idx, form_w, num, den, pitch=None, seg_n=None):
        """kin_observables_segmented on host arrays: u[S][L][N] (seg_n[S] rows of each segment real; None: L each), the forms in
        CSR over the species (form_idx in the handle's index base), observable g form num[g] divided by form den[g] unless that
        is -1. Returns out[S][L][pitch] (pitch None: G), bit for bit what observables_host gives."""
        u, S, L = self._ms_block(u, self.n)
        seg_n = _seg_n(seg_n, S)
        args, G, pitch = _observable_args(form_ptr, form_idx, form_w, num, den, pitch)
        out = np.empty((S, L, max(pitch, 0)))
        self._chk(lib().kin_observables_segmented(self._h, S, L, _p64(seg_n), _pd(u), *args, _pd(out) if out.size else None))
        return out

    def observables_segmented_dev(self, S, L, d_u, form_ptr, form_idx, form_w, num, den, pitch, d_out, d_seg_n=0, stream=0):
        """kin_observables_segmented_dev: device pointers (ints; 0 = not given) u[S][L][N], seg_n[S] (int64), out[S][L][pitch];
        the forms and observables are host arrays, read before the call returns. Only enqueues; one stream per handle at a time."""
        args, _, _ = _observable_args(form_ptr, form_idx, form_w, num, den, pitch)
        self._chk(lib().kin_observables_segmented_dev(self._h, int(S), int(L), _dp(d_seg_n), _dp(d_u), *args, _dp(d_out), _dp(stream)))

    def solution_observables(self, form_ptr, form_idx, form_w, num, den, pitch=None):
        """kin_solution_observables: the saved states of the last solve, read where they live. Returns out[n_saved][pitch]."""
        args, G, pitch = _observable_args(form_ptr, form_idx, form_w, num, den, pitch)
        out = np.empty((self._solution()[0], max(pitch, 0)))
        self._chk(lib().kin_solution_observables(self._h, *args, _pd(out) if out.size else None))
        return out

    def ensemble_observables(self, form_ptr, form_idx, form_w, num, den, pitch=None, store=False, download=True):
        """kin_ensemble_observables: the stored ensemble, every member's own saved rows read where they live. Returns
        out[K][n_rows][pitch], or None with download=False (which needs store). store (pitch None: N; it must be N, and
        1 <= G <= N): the result becomes the stored ensemble - the observables in the columns below G, zeros in the others - and
        every ensemble_* method that treats columns as columns reads it from then on; ensemble_observable_count gives G."""
        if not download and not store:
            raise ValueError("download=False needs store=True: the result would go nowhere")
        K, L = self.ensemble_size()[:2]
        args, G, pitch = _observable_args(form_ptr, form_idx, form_w, num, den, self.n if store and pitch is None else pitch)
        out = np.empty((K, L, max(pitch, 0))) if download else None
        self._chk(lib().kin_ensemble_observables(self._h, *args, int(bool(store)), _pd(out) if download and out.size else None))
        return out

    def ensemble_observable_count(self):
        """kin_ensemble_observable_count: G of a stored record of observables, 0 for a record of states."""
        G = c_int64(0)
        self._chk(lib().kin_ensemble_observable_count(self._h, ctypes.byref(G)))
        return G.value

    # --- library order (tiled sweep) --------------------------------------------------------
    def lib_layout(self):
        """dict(k_len, species_of_lib[N], slot_of_reaction[R], identity, hubs, windows, records, entries, copies, block)."""
        k_len, ident = c_int64(0), c_int32(0)
        sp = np.empty(self.n, np.int64)
        slot = np.empty(self.nr, np.int64)
        info = np.zeros(6, np.int64)
        self._chk(lib().kin_lib_layout(self._h, 0, ctypes.byref(k_len), _p64(sp), _p64(slot), ctypes.byref(ident), _p64(info)))
        return dict(k_len=k_len.value, species_of_lib=sp, slot_of_reaction=slot, identity=bool(ident.value), hubs=int(info[0]),
                    windows=int(info[1]), records=int(info[2]), entries=int(info[3]), copies=int(info[4]), block=int(info[5]))

    def states_to_lib_dev(self, B, d_in, d_out, stream=0):
        self._chk(lib().kin_states_to_lib_dev(self._h, int(B), c_void_p(d_in), c_void_p(d_out), _dp(stream)))

    def states_from_lib_dev(self, B, d_in, d_out, stream=0):
        self._chk(lib().kin_states_from_lib_dev(self._h, int(B), c_void_p(d_in), c_void_p(d_out), _dp(stream)))

    def rates_to_lib_dev(self, B, d_k, d_k_lib, stream=0):
        self._chk(lib().kin_rates_to_lib_dev(self._h, int(B), c_void_p(d_k), c_void_p(d_k_lib), _dp(stream)))

    def rate_table_lib_dev(self, T_stops, d_out):
        """Rate table for T_stops in library order straight into a device buffer [len(T_stops)][k_len]."""
        T_stops = _f64(T_stops)
        self._chk(lib().kin_rate_table_lib_dev(self._h, _pd(T_stops), len(T_stops), c_void_p(d_out)))

    def rhs_tiled_dev(self, B, d_u_lib, d_du_lib, d_k_lib=0, d_T=0, stream=0):
        """Batched RHS in library order; exactly one of d_k_lib / d_T (device pointers as ints); only enqueues."""
        self._chk(lib().kin_rhs_tiled_dev(self._h, int(B), c_void_p(d_u_lib), _dp(d_k_lib),
                                          _dp(d_T), c_void_p(d_du_lib), _dp(stream)))

    def rhs_batched_T_dev(self, B, d_u, d_T, d_du, stream=0):
        """Batched RHS on caller-order states with rate constants formed in the sweep from T[b]; only enqueues."""
        self._chk(lib().kin_rhs_batched_T_dev(self._h, int(B), c_void_p(d_u), c_void_p(d_T), c_void_p(d_du),
                                              _dp(stream)))

    def rhs_batched_klib_dev(self, B, d_u, d_k_lib, d_du, stream=0):
        """Batched RHS on caller-order states u[b][N] -> du[b][N] with rate constants in the library's slot order k_lib[b][k_len]
        (from rate_table_lib_dev / rates_to_lib_dev); device pointers as ints; only enqueues."""
        self._chk(lib().kin_rhs_batched_klib_dev(self._h, int(B), c_void_p(d_u), c_void_p(d_k_lib), c_void_p(d_du),
                                                 _dp(stream)))

    def jac_pattern(self, index_base=0):
        rowptr = np.empty(self.n + 1, np.int64)
        col = np.empty(self._jac_nnz(), np.int64)
        self._chk(lib().kin_jac_pattern(self._h, _p64(rowptr), _p64(col), index_base))
        return rowptr, col

    def jac_values(self, u):
        u = _f64(u)
        vals = np.empty(self._jac_nnz())
        self._chk(lib().kin_jac_values(self._h, _pd(u), _pd(vals)))
        return vals

    # --- solve -----------------------------------------------------------------------------
    def solve(self, params: KinParams, u0, tstops=None, T_stops=None, k_table=None, explicit=False):
        """kin_solve (explicit=True: kin_solve_explicit, Dormand-Prince 5(4)) + kin_solution_copy.
        Returns (t[M], u[M][N], retcode, stats dict, status)."""
        u0 = _f64(u0)
        assert len(u0) == self.n
        n_stops = 0
        if tstops is not None:
            tstops = _f64(tstops)
            n_stops = len(tstops)
            if T_stops is not None:
                T_stops = _f64(T_stops)
                assert len(T_stops) == n_stops
            if k_table is not None:
                k_table = _f64(k_table)
                assert k_table.shape == (n_stops, self.nr)
        fn = lib().kin_solve_explicit if explicit else lib().kin_solve
        return self._solved(fn, params, _pd(u0), _pd(tstops), _pd(T_stops), _pd(k_table), n_stops)

    def _solved(self, fn, params, *inputs):
        """A solve entry `fn` (`inputs`: its arguments between params and n_saved), then kin_solution_copy: (t[M], u[M][N],
        retcode, stats dict, status) - also of a solve that failed (KIN_ERR_SOLVE_FAILED), with what it saved."""
        n_saved, rc, stats = c_int64(0), c_int32(0), KinStats()
        st = fn(self._h, ctypes.byref(params), *inputs, ctypes.byref(n_saved), ctypes.byref(rc), ctypes.byref(stats))
        if st not in (KIN_OK, KIN_ERR_SOLVE_FAILED):
            self._chk(st)
        t = np.empty(n_saved.value)
        u = np.empty((n_saved.value, self.n))
        if n_saved.value:
            self._chk(lib().kin_solution_copy(self._h, _pd(t), _pd(u)))
        return t, u, rc.value, stats.as_dict(), st

    def solve_ensemble(self, params: KinParams, u0, k=None, T=None, tstops=None, T_stops=None, k_table=None, trajectories=True):
        """kin_solve_ensemble: K trajectories of this network in ONE launch (one workgroup per trajectory, resident on the GPU).
        u0[K][N]; k[K][R] or T[K] (or neither: the handle's current rates); tstops / T_stops / k_table are shared by the members.
        Returns (t[M], u[K][M][N], n_saved[K], retcodes[K], [stats dict] * K). trajectories=False: no state is downloaded
        (out_u = NULL) and u is None - the members' states stay on the device for ensemble_max / _dot / _flux."""
        u0 = np.ascontiguousarray(np.atleast_2d(_f64(u0)))
        K = u0.shape[0]
        assert u0.shape == (K, self.n)
        k = None if k is None else np.ascontiguousarray(_f64(k).reshape(K, self.nr))
        T = None if T is None else np.ascontiguousarray(_f64(T).reshape(K))
        n_stops = 0
        if tstops is not None:
            tstops = _f64(tstops); n_stops = len(tstops)
            T_stops = None if T_stops is None else _f64(T_stops)
            k_table = None if k_table is None else np.ascontiguousarray(_f64(k_table).reshape(n_stops, self.nr))
        return self._ensemble(lib().kin_solve_ensemble, params, K, _pd(u0), _pd(k), _pd(T), _pd(tstops), _pd(T_stops), _pd(k_table),
                              n_stops, trajectories=trajectories)

    def _member_arrhenius(self, K, Ea, A):
        """Per-member Arrhenius parameters of an ensemble call as contiguous float64 [K][R] arrays, or (None, None); ValueError
        for one without the other, a wrong shape or a dtype that is not real numbers - before the library is called."""
        if Ea is None and A is None:
            return None, None
        if Ea is None or A is None:
            raise ValueError("per-member Arrhenius parameters: give both Ea and A, or neither")
        out = []
        for name, x in (("Ea", Ea), ("A", A)):
            x = np.asarray(x)
            if x.dtype.kind not in "fiu":
                raise ValueError(f"per-member {name} must be real numbers, got dtype {x.dtype}")
            if x.shape != (K, self.nr):
                raise ValueError(f"per-member {name} must be [K][R] = {(K, self.nr)}, got {x.shape}")
            out.append(np.ascontiguousarray(x, dtype=np.float64))
        return out[0], out[1]

    def solve_ensemble_continuous(self, params: KinParams, u0, nodes, trajectories=True, Ea=None, A=None):
        """kin_solve_ensemble_continuous: K trajectories under continuous rate updates, member m's rates at T(t) of its own
        profile. u0[K][N]; nodes: K pairs (t_nodes, T_nodes) in global time (node counts may differ). Ea[K][R], A[K][R] (both or
        neither; ValueError for a wrong shape or dtype): Arrhenius parameters of each member's own
        (kin_solve_ensemble_continuous_params; k_max and t_mult are the handle's); without them the call is the one it always was.
        Returns what solve_ensemble returns: (t[M], u[K][M][N], n_saved[K], retcodes[K], [stats dict] * K); trajectories as there."""
        return self._member_ensemble("kin_solve_ensemble_continuous", params, u0, nodes, trajectories, Ea, A)

    def solve_ensemble_discrete(self, params: KinParams, u0, stops, trajectories=True, Ea=None, A=None):
        """kin_solve_ensemble_discrete: K trajectories under discrete rate updates, member m's rates the Arrhenius rates at
        T_stops held from tstops on (kin_solve's zero-order hold) of its own schedule. u0[K][N]; stops: K pairs
        (tstops, T_stops) in global time (stop counts may differ). Ea[K][R], A[K][R]: as in solve_ensemble_continuous
        (kin_solve_ensemble_discrete_params).
        Returns what solve_ensemble returns: (t[M], u[K][M][N], n_saved[K], retcodes[K], [stats dict] * K); trajectories as there."""
        return self._member_ensemble("kin_solve_ensemble_discrete", params, u0, stops, trajectories, Ea, A)

    def _member_ensemble(self, entry, params, u0, pairs, trajectories, Ea, A):
        """An ensemble whose member m has a time series (times, temperatures) = pairs[m] of its own: the pairs flattened to
        ptr[K + 1], t, T for `entry`, or with Ea, A for its _params form."""
        u0 = np.ascontiguousarray(np.atleast_2d(_f64(u0)))
        K = u0.shape[0]
        assert u0.shape == (K, self.n) and len(pairs) == K
        Ea, A = self._member_arrhenius(K, Ea, A)
        ts = [_f64(a).ravel() for a, _ in pairs]
        Ts = [_f64(b).ravel() for _, b in pairs]
        assert all(len(a) == len(b) for a, b in zip(ts, Ts))
        ptr = np.zeros(K + 1, np.int64)
        ptr[1:] = np.cumsum([len(a) for a in ts])
        t_all = np.ascontiguousarray(np.concatenate(ts))
        T_all = np.ascontiguousarray(np.concatenate(Ts))
        own = () if Ea is None else (_pd(Ea), _pd(A))
        return self._ensemble(getattr(lib(), entry + "_params" if own else entry), params, K, _pd(u0), *own, _p64(ptr), _pd(t_all),
                              _pd(T_all), trajectories=trajectories)

    def _ensemble(self, fn, params, K, *inputs, trajectories=True):
        """The two calls of an ensemble entry point `fn`: the size query, then the solve into fresh outputs. `inputs`: its
        arguments between K and n_rows. Returns (t[M], u[K][M][N], n_saved[K], retcodes[K], [stats dict] * K); u is None with
        trajectories=False (out_u = NULL: nothing but the times and the members' counters crosses the bus)."""
        rows = c_int64(0)
        self._chk(fn(self._h, ctypes.byref(params), K, *inputs, ctypes.byref(rows), None, None, None, None, None))
        M = rows.value
        t = np.empty(M); u = np.empty((K, M, self.n)) if trajectories else None; ns = np.zeros(K, np.int64); rcs = np.zeros(K, np.int32)
        stats = (KinStats * K)()
        self._chk(fn(self._h, ctypes.byref(params), K, *inputs, ctypes.byref(rows), _pd(t), _pd(u), _p64(ns), _p32(rcs), stats))
        return t, u, ns, rcs, [s_.as_dict() for s_ in stats]

    def solve_continuous(self, params: KinParams, u0, t_nodes, T_nodes):
        """kin_solve_continuous + kin_solution_copy: k(t) = Arrhenius(T(t)), T piecewise linear."""
        u0, t_nodes, T_nodes = _f64(u0), _f64(t_nodes), _f64(T_nodes)
        assert len(u0) == self.n and len(t_nodes) == len(T_nodes)
        return self._solved(lib().kin_solve_continuous, params, _pd(u0), _pd(t_nodes), _pd(T_nodes), len(t_nodes))

    def integrator_init(self, params: KinParams, u0, tstops=None, T_stops=None, k_table=None):
        """kin_integrator_init: init(oprob, solver; kwargs...) without solve! (return_integrator=true)."""
        u0 = _f64(u0)
        assert len(u0) == self.n
        n_stops = 0
        if tstops is not None:
            tstops = _f64(tstops)
            n_stops = len(tstops)
            T_stops = _f64(T_stops) if T_stops is not None else None
            k_table = _f64(k_table) if k_table is not None else None
        self._chk(lib().kin_integrator_init(self._h, ctypes.byref(params), _pd(u0), _pd(tstops), _pd(T_stops),
                                            _pd(k_table), n_stops))

    def integrator_init_continuous(self, params: KinParams, u0, t_nodes, T_nodes):
        """kin_integrator_init_continuous: the integrator of a continuous-rate solve (k(t) = Arrhenius(T(t)))."""
        u0, t_nodes, T_nodes = _f64(u0), _f64(t_nodes), _f64(T_nodes)
        assert len(u0) == self.n and len(t_nodes) == len(T_nodes)
        self._chk(lib().kin_integrator_init_continuous(self._h, ctypes.byref(params), _pd(u0), _pd(t_nodes), _pd(T_nodes),
                                                       len(t_nodes)))

    def integrator_step(self, max_steps=1):
        """step!(integ) x max_steps (<= 0: solve!(integ)); returns the number of accepted steps taken."""
        n = c_int64(0)
        self._chk(lib().kin_integrator_step(self._h, int(max_steps), ctypes.byref(n)))
        return n.value

    def integrator_state(self, with_u=True):
        """(integ.t, integ.u or None, retcode, stats dict)."""
        t, rc, stats = c_double(0.0), c_int32(0), KinStats()
        u = np.empty(self.n) if with_u else None
        self._chk(lib().kin_integrator_state(self._h, ctypes.byref(t), _pd(u), ctypes.byref(rc), ctypes.byref(stats)))
        return t.value, u, rc.value, stats.as_dict()

    def newton_solve(self, c, u, b):
        """(I - c J(u)) x = b through the solver's on-device LU (diagnostic)."""
        u, b = _f64(u), _f64(b)
        x = np.empty(self.n)
        self._chk(lib().kin_newton_solve(self._h, float(c), _pd(u), _pd(b), _pd(x)))
        return x

    def resident_probe(self, u, c, b):
        """The resident kernel's phases once per member (diagnostic, kin_resident_probe). u, b: (K, N) or (N,); c: (K,) or scalar.
        Returns dict(du, jac, x: (K, ...) arrays; bad: (K,) int; info: dict of m, ns, rounds, solve_form, desc_in_lds, dyn_lds,
        mpad, dense_species)."""
        u = np.atleast_2d(_f64(u)); b = np.atleast_2d(_f64(b))
        K = u.shape[0]
        c = _f64(np.broadcast_to(np.asarray(c, dtype=np.float64), (K,)))
        assert u.shape == (K, self.n) and b.shape == (K, self.n)
        nnz = c_int64(0)
        self._chk(lib().kin_jac_nnz(self._h, ctypes.byref(nnz)))
        du, x = np.empty((K, self.n)), np.empty((K, self.n))
        jac = np.empty((K, max(nnz.value, 1)))
        bad = np.zeros(K, np.int32)
        info = np.zeros(8 + self.n, np.int64)
        self._chk(lib().kin_resident_probe(self._h, K, _pd(u), _pd(c), _pd(b), _pd(du), _pd(jac), _pd(x),
                                           bad.ctypes.data_as(POINTER(c_int32)), _p64(info)))
        m = int(info[0])
        keys = ("m", "ns", "rounds", "solve_form", "desc_in_lds", "dyn_lds", "mpad")
        inf = {k: int(v) for k, v in zip(keys, info[:7])}
        inf["dense_species"] = info[8:8 + m].copy()
        return dict(du=du, jac=jac[:, :nnz.value], x=x, bad=bad, info=inf)

    def cache_probe(self, path, jv_slots=None, c_fact=None, valid=None, jv_now=None, max_drift=1.0, table=None, queries=None):
        """The LU cache's drift guard or slot rules once through the integrators' own code (diagnostic, kin_cache_probe;
        include/kinetica_hip.h). Drift: jv_slots (ns, nnz), c_fact (ns,), valid (ns,), jv_now (nnz,) ->
        dict(jd (ns, N), drift (ns,) [path 0: also drift_offset, the ensemble's form], valid_after (ns,), dropped (ns,) bool,
        n_dropped, n_tested, n_dropped_offset, clean, info). Slot rules (path 1): table = dict of valid, c_fact, jac_stamp, step_stamp,
        last_use; queries = list of dicts c, band, n_restarts, max_age, n_steps, step_age, n_slots -> (Q, 2) array of nearest, victim."""
        P32 = POINTER(c_int32)
        info = np.zeros(8, np.int64)
        if table is not None:
            v = np.ascontiguousarray(table["valid"], np.int32); cf = _f64(table["c_fact"])
            st = np.ascontiguousarray(np.stack([np.asarray(table[k], np.int64) for k in ("jac_stamp", "step_stamp", "last_use")]))
            qd = _f64(np.array([[q["c"], q["band"]] for q in queries]))
            qi = np.ascontiguousarray(np.array([[q["n_restarts"], q["max_age"], q["n_steps"], q["step_age"], q["n_slots"]] for q in queries], np.int64))
            out = np.full((len(queries), 2), -2, np.int32)
            self._chk(lib().kin_cache_probe(self._h, int(path), 1, len(v), None, _pd(cf), v.ctypes.data_as(P32), None, 0.0, _p64(st), len(queries),
                                            _pd(qd), _p64(qi), None, None, out.ctypes.data_as(P32), _p64(info)))
            return out
        jv_slots = np.atleast_2d(_f64(jv_slots)); jv_now = _f64(jv_now)
        ns = jv_slots.shape[0]
        c_fact = _f64(np.broadcast_to(np.asarray(c_fact, np.float64), (ns,)))
        valid = np.ascontiguousarray(np.broadcast_to(np.asarray(valid, np.int32), (ns,)))
        nnz = c_int64(0)
        self._chk(lib().kin_jac_nnz(self._h, ctypes.byref(nnz)))
        assert jv_slots.shape == (ns, nnz.value) and jv_now.shape == (nnz.value,)
        jd = np.full((ns, self.n), np.nan); drift = np.full((2, ns), np.nan); after = np.full(ns, -2, np.int32)
        self._chk(lib().kin_cache_probe(self._h, int(path), 0, ns, _pd(jv_slots), _pd(c_fact), valid.ctypes.data_as(P32), _pd(jv_now),
                                        float(max_drift), None, 0, None, None, _pd(jd), _pd(drift), after.ctypes.data_as(P32), _p64(info)))
        out = dict(jd=jd, drift=drift[0], valid_after=after, dropped=(valid != 0) & (after == 0), n_dropped=int(info[0]), n_tested=int(info[1]),
                   n_dropped_offset=int(info[2]), info=info)
        if int(path) == 0:
            out.update(drift_offset=drift[1], clean=bool(info[6]))
        return out

    def newton_probe(self, u, c, b, batched=False):
        """K Newton-matrix solves through the host-driven factorisation and solve kernels (diagnostic, kin_newton_probe). u, b:
        (K, N) or (N,); c: (K,) or scalar; batched: the dense inverses of up to 16 members as one batched Gauss-Jordan chain.
        Returns dict(x: (K, N); bad: (K,) int; info: dict of ns, m, mpad, rounds, solve_form, gj_steps, long_rows, max_row,
        dense_species)."""
        u = np.atleast_2d(_f64(u)); b = np.atleast_2d(_f64(b))
        K = u.shape[0]
        c = _f64(np.broadcast_to(np.asarray(c, dtype=np.float64), (K,)))
        assert u.shape == (K, self.n) and b.shape == (K, self.n)
        x = np.empty((K, self.n))
        bad = np.zeros(K, np.int32)
        info = np.zeros(8 + self.n, np.int64)
        self._chk(lib().kin_newton_probe(self._h, K, 1 if batched else 0, _pd(u), _pd(c), _pd(b), _pd(x),
                                         bad.ctypes.data_as(POINTER(c_int32)), _p64(info)))
        keys = ("ns", "m", "mpad", "rounds", "solve_form", "gj_steps", "long_rows", "max_row")
        inf = {k: int(v) for k, v in zip(keys, info[:8])}
        inf["dense_species"] = info[8:8 + inf["m"]].copy()
        return dict(x=x, bad=bad, info=inf)

    def step_probe(self, path, op, state, ctrl, entries, xloc=None):
        """One operation of the step, once, on the caller's state (diagnostic, kin_step_probe; layouts: include/kinetica_hip.h).
        path: 0 host-driven kernels, 1 the update fused into the solve, 2 the lockstep ensemble's kernels, 3 / 4 the resident kernel's
        dispatch in its default / shared-CU build (one entry per member, n = the handle's species count); op: a key of STEP_OPS;
        state: (K, STEP_ROWS, n) or (STEP_ROWS, n); ctrl: (K, STEP_CTRL) or (STEP_CTRL,), in the order of STEP_CTRL_FIELDS;
        entries: a list of dicts (one dict: a list of one) with the integer keys of STEP_IARGS and the scalar keys of STEP_DARGS
        ("w": up to 7 stage weights), everything left out 0 except order = 1 and maxit = 4; xloc: permutation of 0 .. n-1.
        Returns dict(state, ctrl: copies after the operation, shaped as given; pub: the published block, STEP_CTRL values; seq: the
        published sequence word; info: dict of the stage-C plan's groups, wave_rows, wave_rows_long, block_rows, max_row, m, grid, wg; on
        paths 3 and 4 of N, trips, waves_owning, m, solve_form, desc_in_lds, dyn_lds, waves_per_eu)."""
        st = np.array(state, dtype=np.float64, order="C")
        ct = np.array(ctrl, dtype=np.float64, order="C")
        single = st.ndim == 2
        st3 = st.reshape((1,) + st.shape) if single else st
        ct2 = ct.reshape(1, -1) if ct.ndim == 1 else ct
        K, rows, n = st3.shape
        assert rows == STEP_ROWS and ct2.shape == (K, STEP_CTRL)
        entries = [entries] if isinstance(entries, dict) else list(entries)
        ia = np.zeros((len(entries), STEP_IARGS), np.int32)
        da = np.zeros((len(entries), STEP_DARGS))
        for e, ent in enumerate(entries):
            ia[e, STEP_IARG_NAMES.index("order")] = 1
            ia[e, STEP_IARG_NAMES.index("maxit")] = 4
            for q, v in ent.items():
                if q in STEP_IARG_NAMES:
                    ia[e, STEP_IARG_NAMES.index(q)] = int(v)
                elif q == "w":
                    da[e, STEP_DARG_W:STEP_DARG_W + len(v)] = v
                elif q in STEP_DARG_TAIL:
                    da[e, STEP_DARG_TAIL[q]] = float(v)
                else:
                    da[e, STEP_DARG_NAMES.index(q)] = float(v)
        P32 = POINTER(c_int32)
        xl = None if xloc is None else np.ascontiguousarray(xloc, dtype=np.int32)
        assert xl is None or xl.shape == (n,)
        pub = np.zeros(STEP_CTRL + 1)
        info = np.zeros(8, np.int64)
        self._chk(lib().kin_step_probe(self._h, int(path), STEP_OPS[op], n, K, len(entries), ia.ctypes.data_as(P32), _pd(da),
                                       None if xl is None else xl.ctypes.data_as(P32), _pd(st3), _pd(ct2), _pd(pub), _p64(info)))
        keys = (("groups", "wave_rows", "wave_rows_long", "block_rows", "max_row", "m", "grid", "wg") if path < 3 else
                ("N", "trips", "waves_owning", "m", "solve_form", "desc_in_lds", "dyn_lds", "waves_per_eu"))
        return dict(state=st3[0] if single else st3, ctrl=ct2[0] if ct.ndim == 1 else ct2, pub=pub[:STEP_CTRL], seq=int(pub[STEP_CTRL]),
                    info={k: int(v) for k, v in zip(keys, info)})

    def eval_probe(self, path, op, u, k=None, T=0.0, c=None, psi=None, d=None, done=None, members=None, mode=0, sentinel=-3.5e200):
        """The right-hand side, the Jacobian values or the Newton residual once through the integrators' launchers (diagnostic,
        kin_eval_probe; include/kinetica_hip.h). path 0: the single-state kernels with the handle's rates (T > 0: formed from that
        pending temperature on the spot); path 2: the lockstep ensemble's kernels, k: (K, R) per member, members: the entries of
        the launch (default: all), mode: ens_rhs's source mode. op: 'rhs' | 'jac' | 'resid' | 'sizes'; u: (K, N) or (N,); resid: c (K,)
        or scalar, psi, d shaped as u, done (K,) or scalar = the value of newton_done.
        Returns dict(out: (K, ...) - rhs: N values (path 2: f0, f1 of N each), jac: nnz, resid: the solve-vector window; rate: (K, R)
        the rate buffers (rhs on path 2, resid), on path 2 jac (K, 2 R) the operand-derivative buffers; yloc: (N,) positions of the residual inside the window; info: dict of the plan's
        G, S, B, max_row, short, wg, and vec_len, nnz)."""
        ops = dict(rhs=0, jac=1, resid=2, sizes=3)
        keys = ("G", "S", "B", "max_row", "short", "wg", "vec_len", "nnz")
        info = np.zeros(8, np.int64)
        P32 = POINTER(c_int32)
        if op == "sizes":
            self._chk(lib().kin_eval_probe(self._h, int(path), 3, 0, 0, 0, None, None, None, 0.0, None, None, None, None, 0.0, None, 0,
                                           None, None, _p64(info)))
            return dict(info={q: int(v) for q, v in zip(keys, info)})
        u = np.atleast_2d(_f64(u))
        K = u.shape[0]
        assert u.shape == (K, self.n)
        mem = np.arange(K, dtype=np.int32) if members is None else np.ascontiguousarray(members, dtype=np.int32)
        kk = None if k is None else np.atleast_2d(_f64(k))
        assert kk is None or kk.shape == (K, self.nr)
        cc = pp = dd = dn = None
        rate = yloc = None
        if op == "resid":
            sz = self.eval_probe(path, "sizes", None)["info"]
            out_len = sz["vec_len"]
            cc = _f64(np.broadcast_to(np.asarray(c, dtype=np.float64), (K,)))
            pp, dd = np.atleast_2d(_f64(psi)), np.atleast_2d(_f64(d))
            assert pp.shape == u.shape and dd.shape == u.shape
            dn = np.ascontiguousarray(np.broadcast_to(np.asarray(done, dtype=np.int32), (K,)))
            yloc = np.zeros(self.n, np.int32)
        elif op == "jac":
            nnz = c_int64(0)
            self._chk(lib().kin_jac_nnz(self._h, ctypes.byref(nnz)))
            out_len = nnz.value
        else:
            out_len = self.n * (2 if path == 2 else 1)
        if op == "resid" or (op == "rhs" and path == 2):
            rate = np.full((K, self.nr), np.nan)
        elif op == "jac" and path == 2:
            rate = np.full((K, 2 * self.nr), np.nan)      # the members' operand-derivative buffers
        out = np.full((K, max(out_len, 1)), np.nan)
        self._chk(lib().kin_eval_probe(self._h, int(path), ops[op], int(mode), K, len(mem), mem.ctypes.data_as(P32), _pd(u), _pd(kk),
                                       float(T), _pd(cc), _pd(pp), _pd(dd), None if dn is None else dn.ctypes.data_as(P32),
                                       float(sentinel), _pd(out), out.shape[1], _pd(rate),
                                       None if yloc is None else yloc.ctypes.data_as(P32), _p64(info)))
        return dict(out=out[:, :out_len], rate=rate, yloc=yloc, info={q: int(v) for q, v in zip(keys, info)})

    def solution_max_dev(self, d_out):
        """kin_solution_max into a device buffer (pointer as int) of N doubles."""
        self._chk(lib().kin_solution_max_dev(self._h, c_void_p(d_out)))

    def rate_table_dev(self, T_stops, d_out):
        """Rows of the rate table for T_stops straight into a device buffer [len(T_stops)][R]."""
        T_stops = _f64(T_stops)
        self._chk(lib().kin_rate_table_dev(self._h, _pd(T_stops), len(T_stops), c_void_p(d_out)))

    def rhs_block_dev(self, r_lo, r_hi, d_u, d_du, stream=0):
        """Partial RHS of reactions [r_lo, r_hi) on device buffers; only enqueues."""
        self._chk(lib().kin_rhs_block_dev(self._h, int(r_lo), int(r_hi), c_void_p(d_u), c_void_p(d_du),
                                          _dp(stream)))

    def solution_dot(self, w):
        """sum_i w[i] u_i(t) at every saved time, reduced on the device (conserved quantities)."""
        w = _f64(w)
        assert len(w) == self.n
        out = np.empty(self._solution()[0])
        self._chk(lib().kin_solution_dot(self._h, _pd(w), _pd(out)))
        return out

    def rate_table_rows(self, rows):
        """Selected rows of the device-resident rate table."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((len(rows), self.nr))
        self._chk(lib().kin_rate_table_rows(self._h, _p64(rows), len(rows), _pd(out)))
        return out

    def solution_max(self):
        out = np.empty(self.n)
        self._chk(lib().kin_solution_max(self._h, _pd(out)))
        return out
