// BDF integrator + chunk/tstop driver behind kin_solve (solver.cpp, lu.cpp, solver_kernels.hip).
#pragma once
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "../../include/kinetica_hip.h"
#include "handle.hpp"
#include "resident_setup.hpp"

namespace kin {

// One ensemble call (kin_solve_ensemble / _continuous / _discrete), validated, as every route takes it (resident.cpp,
// ensemble.cpp, ensemble_routes.cpp: replica_ensemble): K members of the handle's network from u0[K][N]; per-member rate constants k[K][R],
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
  // The call restricted to members [m0, m0 + n) of a network of N species and R reactions: every per-member input and output is
  // advanced to member m0, the shared inputs (p, the shared stops, k_table) and the call-wide outputs (n_rows, out_t) are left
  // alone. The offsets in stop_ptr / node_ptr stay ABSOLUTE - member_stops and the continuous routes add them to tstops /
  // T_stops / t_nodes / T_nodes - so those four do not move.
  EnsembleCall block(int64_t N, int64_t R, int64_t m0, int64_t n) const {
    EnsembleCall b = *this;
    b.K = n;
    const auto adv = [m0](auto*& q, int64_t stride) { if (q) q += m0 * stride; };
    adv(b.u0, N); adv(b.k, R); adv(b.T, 1); adv(b.stop_ptr, 1); adv(b.node_ptr, 1);
    adv(b.Ea, R); adv(b.A, R); adv(b.d_Ea, R); adv(b.d_A, R);
    if (out_u) b.out_u += m0 * make_res_grid(p).cap * N;
    adv(b.n_saved, 1); adv(b.retcodes, 1); adv(b.stats, 1);
    return b;
  }
};

// The finishing layer of every route, host part: the members' results into the call's per-member outputs (each may be null) -
// n_saved clamped to the save grid's `cap` rows, retcodes, stats - and the call's out_t[cap]: the save times of res_furthest of
// the members, zeros from its n_saved on. `times`: every member's save times on the host, or null when the furthest member's are
// elsewhere (finish_ensemble then fetches them; the zeros are written here either way). Returns the clamped rows and that member.
struct EnsembleRows { std::vector<int64_t> n_saved; int64_t best; };
inline EnsembleRows finish_members(const EnsembleCall& c, int64_t cap, const MemberResult* res, const std::vector<double>* times) {
  EnsembleRows f{std::vector<int64_t>((size_t)c.K), 0};
  for (int64_t m = 0; m < c.K; m++) {
    f.n_saved[(size_t)m] = std::min(res[m].n_saved, cap);
    if (c.n_saved) c.n_saved[m] = f.n_saved[(size_t)m];
    if (c.retcodes) c.retcodes[m] = res[m].retcode;
    if (c.stats) c.stats[m] = res[m].stats;
  }
  f.best = res_furthest(f.n_saved);
  if (c.out_t) {
    int64_t n = f.n_saved[(size_t)f.best];
    if (times) { n = std::min<int64_t>(n, (int64_t)times[f.best].size()); std::copy_n(times[f.best].begin(), n, c.out_t); }
    std::fill(c.out_t + n, c.out_t + cap, 0.0);
  }
  return f;
}
// ... and the whole of it (ensemble_routes.cpp): finish_members, the furthest member's times from row `best` of dev_times[K][cap]
// on the device where host_times is null, and the handle's ensemble record over sol[K][cap][N]. Drains the handle's stream.
void finish_ensemble(kin_network* h, const EnsembleCall& c, int64_t cap, const std::vector<MemberResult>& res, const double* sol,
                     const std::vector<double>* host_times, const double* dev_times = nullptr);

// Member threads: body(i) for i in [0, n) on a host thread each. Every thread that started is joined before anything is thrown (a
// joinable std::thread that goes out of scope terminates the process); when the host refuses a thread, never_started(q) is
// called for that index and every later one - on the calling thread, while the started ones run - and no further thread is
// tried. Then the spawn failure, else the first body's exception, is rethrown as a KinError.
template <class Body, class NeverStarted>
void run_member_threads(int64_t n, Body body, NeverStarted never_started) {
  std::vector<std::string> errs((size_t)n);
  std::vector<std::thread> th;
  th.reserve((size_t)n);
  std::string spawn_err;
  for (int64_t i = 0; i < n && spawn_err.empty(); i++) {
    try {
      th.emplace_back([&, i] { try { body(i); } catch (const std::exception& e) { errs[(size_t)i] = e.what(); } });
    } catch (const std::exception& e) {
      spawn_err = e.what();
      for (int64_t q = i; q < n; q++) never_started(q);
    }
  }
  for (auto& x : th) x.join();
  if (!spawn_err.empty()) throw KinError(ERR_DEVICE, "ensemble: could not start a member thread: " + spawn_err);
  for (auto& e : errs) if (!e.empty()) throw KinError(ERR_DEVICE, "ensemble member failed: " + e);
}

// The thread route's assignment: K members over at most `limit` threads - `per` = ceil(K / limit) members a thread at the most,
// `threads` = ceil(K / per) threads, member m on thread m mod threads (K <= limit: a thread per member; else the loads differ by
// at most one)
struct ThreadShare {
  int64_t per, threads;
  int64_t thread_of(int64_t m) const { return m % threads; }
};
inline ThreadShare replica_thread_share(int64_t K, int64_t limit) {
  const int64_t per = ceil_div(K, limit);
  return {per, ceil_div(K, per)};
}

// The ensemble entry points behind the extern "C" wrappers (ensemble_routes.cpp). ensemble_entry: the checks every form shares
// - handle, params / u0 / K, the form's own `checks`, the save grid, then `validate` -, the size query (n_rows alone), or the call
// with p filled in through run_ensemble: per-member parameters uploaded, route chosen (KIN_ENSEMBLE_ROUTE, KIN_ENSEMBLE_BATCHED)
int ensemble_entry(kin_network* h, const kin_params* params, EnsembleCall c, const std::function<void()>& checks,
                   const std::function<void()>& validate);
// ... and the per-member forms through it: kin_solve_ensemble_continuous / _discrete and their _params forms (Ea == A == null:
// the shared call, bit for bit). `nodes`: ptr / t / T are node_ptr / t_nodes / T_nodes, else stop_ptr / tstops / T_stops
int ensemble_member_entry(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* Ea, const double* A,
                          bool nodes, const int64_t* ptr, const double* t, const double* T, int64_t* n_rows, double* out_t,
                          double* out_u, int64_t* n_saved, int32_t* retcodes, kin_stats* stats);
// the compiled tables a solve reads on the device, and its work vectors, on the handle's stream (kin_network_create, which adds
// the sweep tables; a replica of the thread route)
void upload_solve_tables(kin_network* h);

// what kin_solve / _explicit / _continuous hand back from solve_entry's retcode
inline void finish_solve(const kin_network* h, int rc, int64_t* n_saved, int32_t* retcode) {
  if (n_saved) *n_saved = h->n_saved;
  if (retcode) *retcode = rc;
  if (rc != KIN_RETCODE_SUCCESS) throw KinError(ERR_SOLVE_FAILED, "ODE solution failed.");
}

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
