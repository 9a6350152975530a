// BDF integrator + chunk/tstop driver behind kin_solve (solver.cpp, lu.cpp, solver_kernels.hip).
#pragma once
#include <string>
#include "../../include/kinetica_hip.h"
#include "handle.hpp"

namespace kin {

// One ensemble call (kin_solve_ensemble / _continuous / _discrete), validated, as every route takes it (resident.cpp,
// ensemble.cpp, capi.cpp: replica_ensemble): K members of the handle's network from u0[K][N]; per-member rate constants k[K][R],
// or temperatures T[K] (Arrhenius), or else the handle's current rates for all; optional discrete rate updates shared by the
// members (tstops + T_stops or k_table, n_stops of them); with stop_ptr, discrete rate updates of each member's own: member m
// holds the Arrhenius rates at T_stops[j] from tstops[j] on, j in [stop_ptr[m], stop_ptr[m + 1]) of the concatenated arrays; or,
// with node_ptr, continuous rate updates: member m's rates at T(t) of its own profile (t_nodes, T_nodes)[node_ptr[m] .. node_ptr[m + 1]).
// The last two forms may carry Arrhenius parameters of each member's own, Ea[K][R] / A[K][R] (kin_solve_ensemble_*_params): every
// route reads a member's parameters through member_arrhenius only, as it reads its stops through member_stops.
// Outputs (each may be null): n_rows = cap (rows of the save grid), out_t[cap], out_u[K][cap][N], n_saved[K], retcodes[K], stats[K].
struct EnsembleCall {
  kin_params p;
  int64_t K;
  const double *u0, *k, *T;
  const double *tstops, *T_stops, *k_table;
  int64_t n_stops;
  const int64_t* stop_ptr;
  const int64_t* node_ptr;
  const double *t_nodes, *T_nodes;
  int64_t* n_rows;
  double *out_t, *out_u;
  int64_t* n_saved;
  int32_t* retcodes;
  kin_stats* stats;
  // per-member Arrhenius parameters of a continuous / per-member-stops call (kin_solve_ensemble_*_params): the caller's
  // Ea[K][R], A[K][R] (both or neither), and their device copies, which run_ensemble uploads before a route sees the call
  const double *Ea = nullptr, *A = nullptr;
  const double *d_Ea = nullptr, *d_A = nullptr;
  bool member_params() const { return Ea != nullptr; }
  // member m's Arrhenius parameters on the device: its rows of the per-member blocks, else the handle's own arrays
  struct Arrhenius { const double *Ea, *A; };
  Arrhenius member_arrhenius(const kin_network* h, int64_t m) const {
    if (!d_Ea) return {h->Ea.p, h->A.p};
    return {d_Ea + m * h->host.R, d_A + m * h->host.R};
  }
  bool continuous() const { return node_ptr != nullptr; }
  bool static_rates() const { return n_stops == 0 && !stop_ptr && !node_ptr; }   // the members' own k / T / the handle's k for the whole span
  // member m's discrete rate updates: its slice of the concatenated stops, else the shared ones (n = 0: none)
  struct Stops { const double *tstops, *T_stops; int64_t n; };
  Stops member_stops(int64_t m) const {
    if (!stop_ptr) return {tstops, T_stops, n_stops};
    return {tstops + stop_ptr[m], T_stops + stop_ptr[m], stop_ptr[m + 1] - stop_ptr[m]};
  }
};

// Runs the whole solve (chunk loop, discrete rate updates, retry loop); stores the solution in
// the handle; returns the final KIN_RETCODE_*.
int solve_entry(kin_network* h, const kin_params& p, const double* u0, const double* tstops,
                const double* T_stops, const double* k_table, int64_t n_stops, kin_stats* stats,
                const double* t_nodes = nullptr, const double* T_nodes = nullptr, int64_t n_nodes = 0,
                bool explicit_solver = false);   // explicit: Dormand-Prince 5(4) instead of the BDF (kin_solve_explicit)
// return_integrator=true: initialise / advance / inspect the integrator without solving (solver.cpp)
void integrator_init(kin_network* h, const kin_params& p, const double* u0, const double* tstops, const double* T_stops,
                     const double* k_table, int64_t n_stops, const double* t_nodes = nullptr, const double* T_nodes = nullptr,
                     int64_t n_nodes = 0);   // n_nodes > 0: continuous rate updates (kin_integrator_init_continuous)
int64_t integrator_step(kin_network* h, int64_t max_steps);
void integrator_state(kin_network* h, double* t, double* u, int32_t* retcode, kin_stats* stats);
// Resident integrator (resident.cpp): the whole solve in one launch, one workgroup per trajectory. `resident_eligible`:
// the network is small enough (KIN_RESIDENT_MAX_N, default 400 species: measured crossover against the host-driven path), the call has a save grid and uses none of the
// features that stay on the host-driven path (continuous rates, explicit solver, manual stepping, traces, fault injection);
// KIN_RESIDENT=0 switches the path off.
bool resident_eligible(kin_network* h, const kin_params& p, bool continuous, bool explicit_solver);
int resident_solve(kin_network* h, const kin_params& p, const double* u0, const double* tstops, const double* T_stops,
                   const double* k_table, int64_t n_stops, kin_stats* stats);
// K members of one network in ONE launch (one workgroup each)
void resident_ensemble(kin_network* h, const EnsembleCall& c);
// does the network fit the resident kernel (its state, rates and solve vectors in one compute unit's LDS)?
bool resident_fits(kin_network* h);
// ... and does an ensemble of K members take the one-launch form (resident.cpp: not few members of a network at the kernel's upper end)?
bool resident_ensemble_route(kin_network* h, int64_t K);
// diagnostic: the resident kernel's RHS, Jacobian, factorisation and solve once per member (kin_resident_probe)
void resident_probe(kin_network* h, int64_t K, const double* u, const double* c, const double* b, double* du, double* jac, double* x,
                    int32_t* bad, int64_t* info);
// diagnostic: the LU cache's drift guard (mode 1) or slot rules (mode 2) through the resident kernel (kin_cache_probe, path 1;
// resident.hpp: ResProbeIO has the argument layout)
void resident_cache_probe(kin_network* h, int mode, int64_t n_slots, const double* jv_slots, const double* c_fact, const int32_t* valid,
                          const double* jv_now, double max_drift, const int64_t* stamps, int64_t n_queries, const double* qd, const int64_t* qi,
                          double* jd, double* drift, int32_t* out_i, int64_t* info);
// diagnostic (kin_step_probe, paths 3 and 4): one operation of the step (resident.hpp: RES_STEP_*) for K members through the resident
// kernel's own dispatch, default build (waves_per_eu 2) or shared-CU build (4). args[K], state[K][RES_STEP_ROWS][N] and
// ctrl[K][RES_STEP_CTRL] are indexed by member; state and ctrl are uploaded, operated on and downloaded whole. info[8]: the header
struct ResStepArg;
void resident_step_probe(kin_network* h, int waves_per_eu, int op, int64_t K, const ResStepArg* args, double* state, double* ctrl,
                         int64_t* info);
// can the lockstep form (ensemble.cpp) take this network's factorisation? (fused solve with a dense Schur block)
bool ensemble_batched_supported(kin_network* h, std::string* why);
// K members of a network beyond that, advanced in lockstep rounds of batched launches (ensemble.cpp)
void batched_ensemble(kin_network* h, const EnsembleCall& c);
// member m's rate constants into d_k (R doubles) on stream s: its row of c.k, Arrhenius at c.T[m] from (Ea, A) - the caller's
// copy of the handle's parameters -, else the handle's current k (resident.cpp)
void stage_member_rates(kin_network* h, const EnsembleCall& c, int64_t m, const double* Ea, const double* A, double* d_k, hipStream_t s);
// validation of a solve's arguments (ODESimulationParams constructor, params.jl:77-104, and the rate inputs); throws.
// with_save_grid false: save_interval is not looked at (kin_integrator_init saves nothing on a grid)
void validate_solve(kin_network* h, const kin_params& p, const double* tstops, const double* T_stops, const double* k_table,
                    int64_t n_stops, const double* t_nodes, const double* T_nodes, int64_t n_nodes, bool need_handle_rates,
                    bool with_save_grid = true);
// max over saved times per species, reduced on the device
void solution_max(kin_network* h, double* out_umax);
// diagnostic: (I - c J(u)) x = b through the solver's LU
void newton_solve(kin_network* h, double c, const double* u, const double* b, double* x);
// diagnostic: K such solves through the product kernels, each member with a slot and a pivot flag of its own; batched: the dense
// inverses of up to GJ_BMAX members as one launch_gauss_jordan_batched chain (kin_newton_probe)
void newton_probe(kin_network* h, int64_t K, int32_t batched, const double* u, const double* c, const double* b, double* x,
                  int32_t* bad, int64_t* info);
// diagnostic (kin_step_probe, path 1): I - c J(u) factorised into slot 0, b placed, then SparseLU::solve_newton with `f` - the
// caller fills the device pointers of the step state, the control block, the publication targets and the scalars; N, the skip
// flag and the partial-sum buffer (the host backend's own) are set here. x: the solution that launch left in W; info[8]: see the header
struct NewtonFuse;
void step_probe_fused(kin_network* h, double c, const double* u, const double* b, NewtonFuse& f, double* x, int64_t* info);
// diagnostic (kin_eval_probe): the residual plan of the host-driven solver (path 0: solver.cpp) and of the lockstep ensemble
// (path 2: ensemble.cpp; built from the analysis whether or not the network takes the batched form), the device copy of yloc, and
// the window [off_y, off_y + vec_len) of W that holds the solve vectors. The first call on a handle runs the analysis.
struct EvalResidPlan { const SegPlanDev* plan; const int32_t* yloc; int64_t off_y, vec_len; };
EvalResidPlan eval_probe_solver_plan(kin_network* h);
EvalResidPlan eval_probe_ensemble_plan(kin_network* h);
// ... path 0's residual pair through HostBackend::launch_residual (what newton_iteration calls) on y = u, psi, d, c and the flag value
// `done`: slot 0's solve vectors and the handle's rate buffer are filled with `sentinel` first and come back in vec[vec_len] and
// rate[R]; the slot's vectors and the control block are restored afterwards
void eval_probe_solver_resid(kin_network* h, const double* u, double c, const double* psi, const double* d, int done, double sentinel,
                             double* vec, double* rate);

}  // namespace kin
