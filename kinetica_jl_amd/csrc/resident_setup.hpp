// Host-side preparation of a solve, shared by every owner of an integrator (solver.cpp, resident.cpp, ensemble.cpp) and the CPU
// replays (tests/native/): the save grid, chunk count and dtmin (reference src/solving/methods.jl:756-758, 829-846, 164, 232,
// 694, 770) and the ResParams the solve driver reads (resident_core.hpp: res_drive), and the integrator settings with their
// environment switches.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/kinetica_hip.h"
#include "resident_core.hpp"

namespace kin {

struct ResGrid {
  std::vector<double> save_local;
  int64_t n_chunks = 1, cap = 0;
  bool save_hits_end = false;
  double dtmin = 0.0;
};

// dtmin handed to the integrator: the caller's value, else what the reference passes - eps(solve_chunkstep) for chunkwise
// solves (methods.jl:232, 770), eps(tspan[end]) for complete-timespan ones (methods.jl:164, 694); Julia's eps(x) is the
// spacing of the doubles at x
inline double res_dtmin(const kin_params& p) {
  if (p.dtmin > 0.0) return p.dtmin;
  const double x = std::fabs(p.solve_chunks != 0 ? p.solve_chunkstep : p.tspan1);
  return std::nextafter(x, std::numeric_limits<double>::infinity()) - x;
}

// requires a save grid (chunkwise, or a save_interval): the resident path writes into a solution buffer of known size
inline bool res_has_grid(const kin_params& p) { return p.solve_chunks != 0 || p.save_interval >= 0; }

// per-chunk local save grid: 0:save_interval:chunkstep (methods.jl:756-758); element i is the correctly rounded i*save_interval as
// produced by Julia's float ranges. Chunkwise, saveat_local = collect(0:save_interval:chunkstep) is a VECTOR, so the chunk end is
// saved only when it is a grid point (save_hits_end; methods.jl:756-758, 829-846). Needs res_has_grid(p): without a grid and
// without chunks, solve_chunkstep may be 0.
inline ResGrid make_res_grid(const kin_params& p) {
  ResGrid g;
  const bool chunks = p.solve_chunks != 0, has_save = p.save_interval >= 0;
  if (chunks) g.n_chunks = (int64_t)(p.tspan1 / p.solve_chunkstep);
  const double span_len = chunks ? p.solve_chunkstep : (p.tspan1 - p.tspan0);
  const double si = has_save ? p.save_interval : p.solve_chunkstep;
  const double base = chunks ? 0.0 : p.tspan0;
  const double last = chunks ? p.solve_chunkstep : p.tspan1;
  const int64_t cnt = (int64_t)std::floor(span_len / si + 1e-9) + 1;
  for (int64_t i = 0; i < cnt; i++) g.save_local.push_back(std::min(base + (double)i * si, last));
  if (!chunks && g.save_local.back() < last) g.save_local.push_back(last);
  if (chunks && std::fabs(g.save_local.back() - last) <= 1e-9 * last) g.save_local.back() = last;
  const int64_t L = (int64_t)g.save_local.size();
  g.save_hits_end = chunks && L > 0 && g.save_local.back() == p.solve_chunkstep;
  g.cap = chunks ? (L - 1) * g.n_chunks + 1 : L;
  g.dtmin = res_dtmin(p);
  return g;
}

// The integrator settings of the LU cache and the carried convergence rate, one definition each; res_default_settings puts
// them into the ResParams of every controller.
// LU_REUSE_RATE_MAX 0.15: the slowest contraction accepted from a reused factorisation (0.1: C3 11 % slower, in refreshes that
// were not needed; 0.2: not robust; 0.5: 17 % slower on the C4 ramp).
// LU_CRATE_MAX_AGE: the remembered rate is trusted for that many accepted steps after it was last measured and never across a
// restart (new rates, new Jacobian): CVODE resets crate at every linear-solver setup, i.e. at least every 20 steps, with a
// Jacobian at most 50 steps old. Without a bound a slot whose contraction has degraded is never found out - one-iteration steps
// measure nothing - and the unconverged iterates pile up in the difference history until the error test collapses the step
// size (seen on the first segment of the C4 ramp).
// LU_CRATE_DY_MAX: a first correction larger than this (in error-weight units) always gets a second iteration. If the true
// contraction is worse than the remembered one - up to the 0.2 that a measurement would still accept - the error left behind is
// 0.25 dy: 0.2 keeps that at the corrector tolerance. (With 1.0 a static 1 400 K solve of a 1k-species network accepted first
// corrections of 0.66 units on a stale rate, poisoned its difference history and ended in DtLessThanMin at every tolerance.)
// LU_MAX_AGE: a slot is offered for that many restarts after its Jacobian was evaluated. Unlimited reuse is UNSAFE: a direction
// that was stiff when the slot was made (c J ~ 1e6) and is not any more (its species consumed) is damped to nothing by the old
// matrix - the corrections vanish, the corrector "converges" at once, and both the convergence test and the error test (which
// only see the corrections) are blind to the component being left at its predictor; the full C4 ramp then ran into
// DtLessThanMin a few hundred restarts later. CVODE bounds the same staleness by re-evaluating J at least every 50 steps.
// LU_DRIFT_MAX: at every restart the Jacobian is fresh; one test compares, for every slot, diag(I - c_s J) as it was when the slot
// was made with what today's Jacobian gives at the same c_s, and slots whose diagonal moved by more than a factor of
// 1 + LU_DRIFT_MAX (either way) are dropped. For mass-action kinetics a column's off-diagonal entries are bounded by its diagonal
// (a reactant's loss terms), so the diagonal is a sound proxy for the unsafe case above, which is a change by ORDERS of
// magnitude. 25 % until round 4; profiles/r05_lu_drift_ab.txt has what that cost (157 of the 307 factorisations of the
// 100-chunk C3 solve re-made matrices the guard had dropped although the corrector converged with them).
constexpr double LU_REUSE_RATE_MAX = 0.15, LU_CRATE_DY_MAX = 0.2, LU_DRIFT_MAX = 1.0, LU_BAND = 0.35;
constexpr int64_t LU_CRATE_MAX_AGE = 10, LU_MAX_AGE = 50;
constexpr size_t LU_CACHE_MB = 32768;

// ... and the cache's environment switches, each read in one place. KIN_LU_CACHE_SLOTS: slots wanted (`dflt` without it; the
// caller applies its own cap), KIN_LU_CACHE_MB: device memory the slots may take, KIN_LU_BAND: the reuse band
inline int lu_env_slots(int dflt) { const char* e = getenv("KIN_LU_CACHE_SLOTS"); return e ? std::max(1, atoi(e)) : dflt; }
inline size_t lu_env_budget_mb() { const char* e = getenv("KIN_LU_CACHE_MB"); return e ? (size_t)std::max(1, atoi(e)) : LU_CACHE_MB; }
// the reuse band of a cache of n_slots: a single slot keeps a band only if KIN_LU_BAND is set (CVODE's own scheme)
inline double lu_env_band(int n_slots) {
  const char* e = getenv("KIN_LU_BAND");
  return e ? atof(e) : (n_slots > 1 ? LU_BAND : 0.0);
}

inline void res_default_settings(ResParams& P, int n_slots_max) {
  P.n_slots = std::max(1, std::min(lu_env_slots(RES_MAX_SLOTS), std::min(n_slots_max, RES_MAX_SLOTS)));
  P.lu_band = lu_env_band(P.n_slots);
  P.upd_in_band = 0;   // (1: the host-driven path, solver.cpp)
  P.reuse_rate_max = LU_REUSE_RATE_MAX;
  P.crate_dy_max = LU_CRATE_DY_MAX;
  P.lu_drift_max = LU_DRIFT_MAX;
  P.newton_frac = -1.0;   // < 0: bdf_newton_frac(rtol), the rule of bdf_rules.hpp (a test may pin a value here)
  P.crate_max_age = LU_CRATE_MAX_AGE;
  P.lu_max_age = LU_MAX_AGE;
  P.carry_rate = 1;
}

inline void res_fill_params(ResParams& P, const kin_params& p, const ResGrid& g) {
  P.tspan0 = p.tspan0; P.tspan1 = p.tspan1; P.abstol = p.abstol; P.reltol = p.reltol; P.chunkstep = p.solve_chunkstep;
  P.dtmin = g.dtmin;
  P.solve_chunks = p.solve_chunks == 2 ? 2 : (p.solve_chunks != 0 ? 1 : 0); P.adaptive_tols = p.adaptive_tols != 0; P.ban_negatives = p.ban_negatives != 0;
  P.save_hits_end = g.save_hits_end ? 1 : 0;
  P.maxiters = p.maxiters; P.n_chunks = g.n_chunks;
  P.L = (int32_t)g.save_local.size();
  P.sol_cap = g.cap;
}

// LU-cache slots per member of K: up to RES_MAX_SLOTS (KIN_LU_CACHE_SLOTS), bounded by KIN_LU_CACHE_MB over
// all members; slot_bytes = one slot's factorisation values and diag(J) copy
inline int res_lu_slots(size_t slot_bytes, int64_t K) {
  const size_t fit = std::max<size_t>(1, lu_env_budget_mb() * 1024 * 1024 / std::max<size_t>(1, slot_bytes * (size_t)K));
  return (int)std::min<size_t>((size_t)std::min(lu_env_slots(RES_MAX_SLOTS), RES_MAX_SLOTS), fit);
}

// the kin_stats of a controller's result; `lu`: the SparseLU it factorised with (lu.hpp), `slots` its LU-cache slots
template <class LU>
kin_stats res_stats(const ResResult& r, const LU& lu, int slots, double wall) {
  kin_stats st{};
  st.n_steps = r.st.n_steps; st.n_rejected = r.st.n_rejected; st.n_rhs = r.st.n_rhs; st.n_jac = r.st.n_jac;
  st.n_factor = r.st.n_factor; st.n_linsolve = r.st.n_linsolve; st.n_newton_fail = r.st.n_newton_fail;
  st.n_chunks = r.st.n_chunks; st.n_restarts = r.st.n_restarts; st.n_retries = r.st.n_retries;
  st.final_abstol = r.final_abstol; st.final_reltol = r.final_reltol; st.wall_seconds = wall;
  st.lu_dense_dim = lu.m; st.lu_sparse_rows = lu.ns; st.lu_rounds = lu.nrounds;
  st.lu_nnz = 2 * lu.nnzU + lu.ns + (int64_t)lu.m * lu.m;
  st.n_lu_reused = r.st.n_lu_reused; st.lu_slots = slots; st.n_bad_pivot = r.st.n_bad_pivot; st.n_lu_dropped = r.st.n_lu_dropped;
  return st;
}

// the member whose save times are an ensemble's common grid: the one with the most saved rows (the first of them)
inline int64_t res_furthest(const std::vector<int64_t>& n_saved) {
  return std::max_element(n_saved.begin(), n_saved.end()) - n_saved.begin();
}

// One member's result as every ensemble route hands it to the finishing layer (solver.hpp: finish_members): its saved rows as the
// integrator counted them, its retcode and its statistics
struct MemberResult {
  int64_t n_saved = 0;
  int32_t retcode = 0;
  kin_stats stats{};
};
template <class LU>
MemberResult res_member_result(const ResResult& r, const LU& lu, int slots, double wall) {
  return MemberResult{r.n_saved, r.retcode, res_stats(r, lu, slots, wall)};
}

}  // namespace kin
