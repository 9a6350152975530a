// Two things, each written once. (1) The solve driver res_drive<D>: the whole of kin_solve's orchestration (chunk loop, discrete
// rate updates, save grid, adaptive_solve! retries - reference src/solving/methods.jl:185-303, 717-865; solve_utils.jl:376-424,
// 435-509) around an integrator D - the controller below, or solver.cpp's HostDriven adapter around it and the explicit mode.
// (2) The controller ResidentBdf<B>: the BDF integrator that stands in for the reference's CVODE_BDF - restart, warm continuation,
// step, order selection, dense output, the LU cache's slot policy and its guards (the settings: resident_setup.hpp) -
// the ONE copy of the step algorithm in the library (oracle/ restates it as its independent check). It runs against a backend
// `B` that supplies the vector operations, the Jacobian, the factorisation and the corrector iteration. There are four:
//   * resident.hip (DevBackend) compiles it for the device: ONE 512-thread workgroup owns one trajectory for the whole solve -
//     every thread runs this controller redundantly on identical scalars (reduction results are broadcast), the backend's
//     operations are workgroup-wide phases separated by barriers; no host round trip, no kernel boundary per step;
//   * solver.cpp (HostBackend): the host-driven integrator, the path for large networks - every operation is a launch on the
//     handle's stream, the corrector a blind batch of launches with one hand-over, the next step enqueued speculatively;
//   * ensemble.cpp (MemberBackend): one controller per member on a host thread, its operations batched into lockstep rounds;
//   * tests/native/resident_host.cpp compiles it for the CPU with a sequential backend over the same tables: the
//     controller's logic is checked without a GPU (test infrastructure, not a product path).
// Where the backends need different things of the controller, the difference is written down once: ResParams::upd_in_band (when
// the Newton update is scaled), ResAttempt::bad_pivot (a vanished pivot reported with the corrector's result instead of by
// factor()), and the operations of a backend whose work is in flight while the controller goes on (ResIsAsync, below):
// drift_launch / drift_collect in place of drift_check, and attempt_begin at every step attempt.
// The paths share the algorithm and its constants, not their linear algebra: at the default tolerances (1e-10 / 1e-8) resident and
// host-driven trajectories agree within the step-sequence
// tolerance (<= 201 units over the 312 solves of profiles/r05_robustness_resident.jsonl), not bit for bit. At rtol = 1e-10 every
// implementation runs on the rounding floor of the right-hand side and they differ by the accuracy of their LINEAR ALGEBRA: against
// a Radau truth (tests/golden/truth_tight_200.npz) the CPU port's pivoted LU lands at rms 61 / max 378 tight units in 4 073
// steps, this controller over the in-workgroup factorisation at 55 / 757 in 5 656, the host-driven path's explicit inverses at
// 394 / 5 572 in 9 785 with 6 172 corrector failures (profiles/r05_tight_tol_truth.jsonl; tests/test_gpu_resident.py bounds both).
#pragma once
#include <cmath>
#include <cstdint>

#include "bdf_rules.hpp"

namespace kin {

// (the scalar rules and their constants: bdf_rules.hpp)
constexpr int RES_MAX_ORDER = BDF_MAX_ORDER;
constexpr int RES_NEWTON_MAXITER = BDF_NEWTON_MAXITER;
constexpr int RES_D_ROWS = BDF_D_ROWS;
constexpr int RES_MAX_SLOTS = 64;   // one LU-cache slot per lane of a wavefront (resident.hip keeps the slot table in registers)

enum : int { RES_RET_SUCCESS = 0, RES_RET_MAXITERS = 1, RES_RET_DTLESSTHANMIN = 2, RES_RET_UNSTABLE = 3 };   // = KIN_RETCODE_*
enum StepStatus { STEP_OK = 0, STEP_DT_MIN = 1, STEP_UNSTABLE = 2 };   // how an integrator's step() ended (res_step_retcode)

// what a solve needs besides the network (plain data; pointers are device pointers in the product, host pointers in the test)
struct ResParams {
  double tspan0, tspan1, abstol, reltol, chunkstep, dtmin;
  int32_t solve_chunks, adaptive_tols, ban_negatives, save_hits_end;
  int64_t maxiters, n_chunks;
  int32_t L;                       // points of the per-chunk (or whole-span) save grid
  const double* save_local;        // L local save times (resident_setup.hpp: make_res_grid)
  int32_t n_stops, rate_mode;      // rate_mode 0: static k; 1: k_table[n_stops][R]; 2: Arrhenius at T_stops[n_stops];
                                   // 3: Arrhenius at T(t) of every step attempt (continuous, nodes below)
  const double* tstops;
  // integrator settings of the controller, the same fields for every backend (resident_setup.hpp: res_default_settings)
  double lu_band, reuse_rate_max, crate_dy_max, lu_drift_max, newton_frac;
  int64_t crate_max_age, lu_max_age;
  int32_t n_slots, carry_rate;
  int64_t sol_cap;                 // rows of the solution buffer
  int32_t profile;                 // device: fill ResResult::prof (KIN_RESIDENT_PROFILE)
  int32_t upd_in_band;             // the Newton update is scaled for a factorisation made at another c (res_update_scale) only
                                   // when c lies within lu_band of it (the host-driven backend); 0: whenever c differs
  // rate_mode 3: T(t) = linear interpolation of (t_nodes, T_nodes)[n_nodes] in global time (the device kernel's prologue sets
  // them per member from ResTrajDev)
  const double *t_nodes, *T_nodes;
  int64_t n_nodes;
};

// Continuous rate updates: the temperature at global time tg of the profile (tn, Tn)[n] (n >= 2) - the linear interpolation of
// the DiffEqArray functor of src/utils.jl:135-139, clamped to the first / last node, else inside [tn[i-1], tn[i]) with
// i = upper_bound(tn, tg). The one copy every integrator calls (this controller on the device and in its CPU replay, solver.cpp's
// kin_solve and manual integrator), so that all of them form their rates at the same temperatures; no contraction into FMAs.
KIN_HD inline double res_T_of(const double* tn, const double* Tn, int64_t n, double tg) {
#pragma clang fp contract(off)
  if (tg <= tn[0]) return Tn[0];
  if (tg >= tn[n - 1]) return Tn[n - 1];
  int64_t lo = 0, hi = n;   // first node with t > tg (std::upper_bound)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (tg < tn[mid]) hi = mid; else lo = mid + 1;
  }
  const int64_t i = lo;
  const double dt = tn[i] - tn[i - 1];
  const double th = dt > 0 ? (tg - tn[i - 1]) / dt : 1.0;
  return (1.0 - th) * Tn[i - 1] + th * Tn[i];
}

// The continuous rate mode needs a backend operation the other modes do not: apply_T(T), the rate constants at one
// temperature. Backends without it (the CPU replay of tests/native/resident_host.cpp) compile as before and never run mode 3.
template <class B, class = void> struct ResHasApplyT { static constexpr bool value = false; };
template <class B> struct ResHasApplyT<B, decltype((void)static_cast<B*>(nullptr)->apply_T(0.0))> { static constexpr bool value = true; };
// A backend that enqueues its work and reads results later (solver.cpp's HostBackend) has three operations the synchronous ones
// do not: attempt_begin(t_new, t_bound) at every step attempt, and the drift guard as drift_launch(max_drift) behind the restart's
// Jacobian + drift_collect(max_drift) after the next wait, in place of drift_check(max_drift). Detected - as a set: a backend is
// asynchronous when it has ALL THREE, one of them alone changes nothing - because the CPU replay cannot compile otherwise: the
// replay sources (tests/native*) are held fixed across a change of this file, so that its tests check the controller and not
// an edit of their own backend; they know drift_check only.
template <class B, class = void> struct ResIsAsync { static constexpr bool value = false; };
template <class B>
struct ResIsAsync<B, decltype((void)static_cast<B*>(nullptr)->attempt_begin(0.0, 0.0), (void)static_cast<B*>(nullptr)->drift_launch(0.0),
                              (void)static_cast<B*>(nullptr)->drift_collect(0.0))> { static constexpr bool value = true; };

struct ResStats {
  int64_t n_steps, n_rejected, n_rhs, n_jac, n_factor, n_linsolve, n_newton_fail, n_chunks, n_restarts, n_retries,
      n_lu_reused, n_bad_pivot, n_lu_dropped;
};

struct ResResult {
  int32_t retcode, pad;
  int64_t n_saved;
  double final_abstol, final_reltol;
  ResStats st;
  int64_t prof[20];   // device only: 10 ns ticks per phase kind (resident.hip: ProfId), 0 in the CPU replay
};

// rms(y / w), rms(f0 / w), rms((f1 - f0) / w), max |f0| / (0.1 |y| + w) over the species, w = atol + rtol |y|
struct ResNorms { double d0, d1, d2, dmax; int nonfinite; };
struct ResSums { double s, se, sm, sp, neg; };   // update, error test of order / order - 1 / order + 1, negative entries

// one corrector attempt: what the controller hands to the backend, and what it gets back
struct ResCorrIn {
  int32_t slot, order;
  double c, upd, rate_max, crate0, tol_first, newton_tol, dy_first_max, ec, ec_m, ec_p, atol, rtol, alpha_o;
};
// (bad_pivot: a pivot of the factorisation in hand vanished - for a backend whose factor() cannot say so yet, because the
// flag comes back with the corrector's result)
struct ResAttempt { bool done, converged, nonfinite, any_negative, deep_negative, bad_pivot; int n_iter; double err, err_m, err_p, crate; };
constexpr double RES_NEG_DEEP = BDF_NEG_DEEP, RES_NEG_MARK = BDF_NEG_MARK;

// A factorisation made for c_fact used at c: the Newton update is scaled by 2 / (1 + c / c_fact) (CVODE's gamrat correction),
// if c lies within `band` of c_fact (ResParams::upd_in_band)
KIN_HD inline double res_update_scale(double c_fact, double c, double band) {
  return (c_fact != c && fabs(c / c_fact - 1.0) <= band) ? 2.0 / (1.0 + c / c_fact) : 1.0;
}

// Predictor + corrector iterations until decided: the decisions of newton_decide (step_dev.hpp), taken in sequence.
// `I` supplies predict_inner / newton_iter_inner (the CPU replay: the backend itself; the device: the phase's own inlined
// operations, run by all wavefronts).
template <class I>
KIN_HD ResAttempt res_corrector_loop(I& b, const ResCorrIn& in, const double* gamma, int n_species) {
  ResAttempt a{false, false, false, false, false, false, 0, 0.0, 0.0, 0.0, 1.0};
  b.predict_inner(in.order, gamma, in.alpha_o, in.atol, in.rtol);
  const double N = (double)n_species;
  double crate = in.crate0, dy_old = 0.0;
  for (int it = 0; it < RES_NEWTON_MAXITER && !a.done; it++) {
    const ResSums q = b.newton_iter_inner(in.slot, in.c, in.upd, in.order, in.ec, in.ec_m, in.ec_p, in.atol, in.rtol);
    const double dy_norm = sqrt(q.s / N);
    const bool nonfinite = !(fabs(q.s) <= 1.79769313486231570815e308);   // !isfinite
    const bool have_rate = it > 0;
    const double rate = have_rate ? dy_norm / dy_old : 0.0;
    if (have_rate && !nonfinite) crate = (0.3 * crate > rate) ? 0.3 * crate : rate;
    bool diverged = nonfinite;
    if (!diverged && have_rate) {
      double rp = rate;
      for (int e = 1; e < RES_NEWTON_MAXITER - it; e++) rp *= rate;
      if (rate >= in.rate_max || rp / (1.0 - rate) * dy_norm > in.newton_tol) diverged = true;
    }
    a.n_iter = it + 1;
    a.done = true;
    if (diverged) { a.nonfinite = nonfinite; }
    else if (dy_norm == 0.0 || (have_rate && rate / (1.0 - rate) * dy_norm < in.newton_tol) ||
             (!have_rate && (dy_norm < in.newton_tol || (in.crate0 < 1.0 && dy_norm <= in.dy_first_max &&
                                                         in.crate0 / (1.0 - in.crate0) * dy_norm < in.tol_first)))) {
      a.converged = true;
    } else {
      dy_old = dy_norm;
      a.done = it == RES_NEWTON_MAXITER - 1;
    }
    if (a.converged) {
      a.err = sqrt(q.se / N); a.err_m = sqrt(q.sm / N); a.err_p = sqrt(q.sp / N);
      a.any_negative = q.neg > 0.0;
      a.deep_negative = q.neg >= RES_NEG_MARK;
      if (!(fabs(q.se) <= 1.79769313486231570815e308)) a.nonfinite = true;
    }
  }
  a.crate = crate;
  return a;
}

template <class B>
struct ResidentBdf {
  B& b;
  const ResParams& P;
  double gamma[RES_MAX_ORDER + 1], alpha[RES_MAX_ORDER + 1], errc[RES_MAX_ORDER + 2];
  // integrator state
  double t = 0, h_abs = 0, atol = 0, rtol = 0, newton_tol = 0, dtmin = 0, fail_score = 0;
  int order = 1, n_equal = 0, cur_slot = 0;
  bool lu_valid = false, jac_current = false, force_jac_refresh = false, force_fresh_lu = false, cache_suspended = false,
       slot_is_fresh = false, pending_order_change = false,
       first_selection = false;   // the next step-size selection is the first since a (re)initialisation: growth cap 1e4 (CVODE's ETAMX1), 10 afterwards
  int64_t steps_since_jac = 0, jac_stamp_now = 0, use_clock = 0, iters_left = 0;
  double err_m = 0, err_p = 0, err_o = 0, safety_o = 0.9;
  double seg_origin = 0;   // global time of the current segment's local time 0 (rate_mode 3)
  ResStats st;

  KIN_HD ResidentBdf(B& bb, const ResParams& pp) : b(bb), P(pp) {
    bdf_fill_coef(gamma, alpha, errc);
    st = ResStats{};
  }

  KIN_HD void set_tols(double a, double r) {
    atol = a; rtol = r;
    newton_tol = bdf_newton_tol(r, P.newton_frac);
  }

  // work matrices of change_D: MEMBERS, not locals - on the device the controller object lives in LDS, dynamically indexed
  // local arrays would live in scratch (= global memory: a dependent store / load pair there costs microseconds)
  double wM[6][6], wR[6][6], wU[6][6], wRU[6][6], wp[RES_MAX_ORDER + 1];
  KIN_HD void change_D(int ord, double factor) {
    bdf_change_D_matrix(ord, factor, wM, wR, wU, wRU);
    b.change_D(ord, wRU);
  }

  KIN_HD bool continuous() const { return ResHasApplyT<B>::value && P.rate_mode == 3; }

  // rate_mode 3: the rate constants at the conditions of segment-local time tau (bdf.py's hook)
  KIN_HD void rates_at(double tau) {
    if constexpr (ResHasApplyT<B>::value) b.apply_T(res_T_of(P.t_nodes, P.T_nodes, P.n_nodes, seg_origin + tau));
  }
  // LU-cache lookup; under continuous rate updates only slots whose Jacobian is at most BDF_CONT_JAC_AGE accepted steps old
  // (a backend without apply_T never runs that mode and offers the lookup without the step-age arguments)
  KIN_HD int nearest_slot(double c, double band) {
    if constexpr (ResHasApplyT<B>::value) {
      const bool cont = continuous();
      return b.nearest_slot(c, band, st.n_restarts, P.lu_max_age, cont ? st.n_steps : 0, cont ? BDF_CONT_JAC_AGE : -1);
    } else {
      return b.nearest_slot(c, band, st.n_restarts, P.lu_max_age);
    }
  }

  KIN_HD void eval_jac() { b.eval_jac_y(); st.n_jac++; lu_valid = false; steps_since_jac = 0; jac_stamp_now = st.n_restarts; }
  KIN_HD void predict() { b.predict(order, gamma, alpha[order], atol, rtol); }

  // Warm continuation at a chunk start whose rates did not change (kin_params.solve_chunks == 2): the system
  // is autonomous and chunks run in local time, so difference history, order and step size stay valid. The Jacobian is
  // evaluated at the chunk's first state and the LU cache's drift guard runs, as at a re-initialisation.
  KIN_HD void resume() {
    t = 0.0;
    st.n_restarts++;
    eval_jac();
    jac_current = true;
    drift_launch(); drift_collect();
  }
  // The LU cache's drift guard, after every fresh Jacobian of a (re)start: the slots are tested against that Jacobian and the
  // drifted ones dropped. An asynchronous backend launches the test right behind the Jacobian and reads it after the next
  // wait it has anyway; the others do the whole test when it is collected (where it runs changes no value)
  KIN_HD bool drift_guard() const { return P.lu_band > 0.0 && P.lu_drift_max > 0.0; }
  KIN_HD void drift_launch() {
    if constexpr (ResIsAsync<B>::value) { if (drift_guard()) b.drift_launch(P.lu_drift_max); }
  }
  KIN_HD void drift_collect() {
    if (!drift_guard()) return;
    if constexpr (ResIsAsync<B>::value) st.n_lu_dropped += b.drift_collect(P.lu_drift_max);
    else st.n_lu_dropped += b.drift_check(P.lu_drift_max);
  }

  // (re)start at segment-local time 0 from the state in y: order 1, fresh Jacobian, CVODE's initial step on the decade grid
  // (bdf_rules.hpp: bdf_h0_begin / _update / _finish)
  KIN_HD bool restart(double t_bound) {
    t = 0.0;
    st.n_restarts++;
    eval_jac();
    jac_current = true;
    drift_launch();
    b.rhs_y_to_f0(); st.n_rhs++;
    ResNorms n0 = b.norms(false, atol, rtol);
    drift_collect();
    if (n0.nonfinite) return false;
    const double tdist = fabs(t_bound);
    BdfFirstStep fs = bdf_h0_begin(tdist, tdist, n0.dmax);
    if (fs.iterate()) {
      for (int count = 1; count <= BDF_H0_EVALS; count++) {
        b.ytmp_axpy(fs.hg);
        b.rhs_ytmp_to_f1(); st.n_rhs++;
        ResNorms n1 = b.norms(true, atol, rtol);
        if (n1.nonfinite) return false;
        if (bdf_h0_update(fs, count, n1.d2)) break;
      }
    }
    h_abs = bdf_h0_finish(fs, tdist);
    b.init_D(false, h_abs);
    order = 1; n_equal = 0; fail_score = 0.0;
    first_selection = true;
    return true;
  }

  KIN_HD void reset_history() {
    b.ytmp_from_D0();
    b.rhs_ytmp_to_f0(); st.n_rhs++;
    b.init_D(true, h_abs);
    order = 1; n_equal = 0; lu_valid = false; fail_score = 0.0;
    b.slots_invalidate(false);
    force_jac_refresh = true;
  }

  KIN_HD void invalidate_lu_keep_counters() { b.slots_invalidate(false); lu_valid = false; cur_slot = 0; force_fresh_lu = false; }
  KIN_HD void invalidate_lu() {
    b.slots_invalidate(true);
    lu_valid = false; cur_slot = 0; use_clock = 0; force_fresh_lu = false; steps_since_jac = 0; cache_suspended = false;
  }

  KIN_HD bool crate_fresh(int slot) const {
    return P.carry_rate && b.slot_crate(slot) < 1.0 && b.slot_crate_restart(slot) == st.n_restarts &&
           st.n_steps - b.slot_crate_step(slot) <= P.crate_max_age;
  }

  // returns true when a pivot vanished
  KIN_HD bool factor_into(int slot, double c) {
    const bool bad = b.factor(slot, c, P.lu_band > 0.0);
    b.slot_made(slot, c, ++use_clock, jac_stamp_now, st.n_steps - steps_since_jac);
    cur_slot = slot;
    st.n_factor++;
    return bad;
  }

  // predictor + corrector iterations until decided (one backend operation: on the device one phase, no round trip through
  // the controller between the iterations)
  KIN_HD ResAttempt corrector(double c) {
    ResCorrIn in;
    const double cf = b.slot_c_fact(cur_slot);
    in.slot = cur_slot; in.order = order; in.c = c;
    in.upd = res_update_scale(cf, c, P.upd_in_band ? P.lu_band : bdf_inf());
    in.rate_max = (P.lu_band > 0.0 && !cache_suspended && !slot_is_fresh) ? P.reuse_rate_max : 1.0;
    in.crate0 = P.carry_rate ? b.slot_crate(cur_slot) : 1.0;
    in.tol_first = crate_fresh(cur_slot) ? newton_tol : -1.0;
    in.newton_tol = newton_tol; in.dy_first_max = P.crate_dy_max;
    in.ec = errc[order]; in.ec_m = order > 1 ? errc[order - 1] : 0.0; in.ec_p = errc[order + 1];
    in.atol = atol; in.rtol = rtol; in.alpha_o = alpha[order];
    return b.corrector(in, gamma);
  }

  // one accepted step towards t_bound (what is asynchronous on the host-driven path is inside its backend's operations)
  KIN_HD StepStatus step(double t_bound) {
    bool accepted = false, first_attempt = true;
    double safety = 0.9, err_norm = 0.0, t_new = t;
    ResAttempt a{};
    while (!accepted) {
      if (iters_left-- <= 0) return STEP_OK;   // caller checks iters_left < 0 -> MaxIters
      const double min_step = bdf_min_step(dtmin, t);
      if (h_abs < min_step) {
        if (!first_attempt) return STEP_DT_MIN;
        change_D(order, min_step / h_abs);
        h_abs = min_step; n_equal = 0; lu_valid = false;
      }
      first_attempt = false;
      t_new = t + h_abs;
      if (t_new - t_bound > 0.0) {
        t_new = t_bound;
        change_D(order, fabs(t_new - t) / h_abs);
        n_equal = 0; lu_valid = false;
      }
      const double hh = t_new - t;
      h_abs = fabs(hh);
      const double c = hh / alpha[order];
      if (continuous()) rates_at(t_new);
      if constexpr (ResIsAsync<B>::value) b.attempt_begin(t_new, t_bound);
      bool converged = false;
      if (force_jac_refresh) { predict(); eval_jac(); jac_current = true; force_jac_refresh = false; }
      bool fresh = false, bad = false;
      const double band = cache_suspended ? 0.0 : P.lu_band;
      if (band > 0.0) {
        const int hit = nearest_slot(c, band);
        if (hit >= 0 && !force_fresh_lu) { cur_slot = hit; b.slot_touch(hit, ++use_clock); st.n_lu_reused++; }
        else {
          if (force_fresh_lu && !jac_current && steps_since_jac > 20) { predict(); eval_jac(); jac_current = true; }
          bad = factor_into(hit >= 0 ? hit : b.victim_slot(st.n_restarts, P.lu_max_age, P.n_slots), c);
          fresh = jac_current;
        }
        force_fresh_lu = false;
      } else if (!lu_valid) {
        bad = factor_into(0, c);
        lu_valid = true;
        fresh = jac_current;
      }
      for (;;) {
        slot_is_fresh = fresh || b.slot_c_fact(cur_slot) == c;
        a = corrector(c);
        st.n_rhs += a.n_iter; st.n_linsolve += a.n_iter;
        if (a.n_iter > 1) b.slot_rate(cur_slot, a.crate, st.n_steps, st.n_restarts);
        converged = a.done && a.converged && !a.nonfinite;
        if (bad || a.bad_pivot) {
          // a pivot of the factorisation in hand vanished (static pivoting): the slot is dropped, the step is retried at
          // half the size from a Jacobian at its own predictor
          b.slot_drop(cur_slot);
          lu_valid = false; force_jac_refresh = true; st.n_bad_pivot++;
          converged = false;
          break;
        }
        if (converged) break;
        st.n_newton_fail++;
        if (band > 0.0) {
          if (fresh) break;
          if (!jac_current) { predict(); eval_jac(); jac_current = true; }
          bad = factor_into(cur_slot, c);
          fresh = true;
          continue;
        }
        if (jac_current) break;
        predict(); eval_jac(); jac_current = true;
        bad = factor_into(0, c);
        lu_valid = true;
      }
      if (!converged || (P.ban_negatives && a.any_negative)) {
        // a failed corrector cuts the step to a quarter and does not count towards the history reset (CVODE: ETACF = 0.25,
        // history rebuilt only after repeated error-test failures: after a reset the order-1 predictor is explicit Euler, far
        // outside the corrector's convergence region at the step sizes of a late, slowly varying solution -
        // docs/DESIGN_HISTORY.md R4 has the A/B); a banned negative state
        // (isoutofdomain, methods.jl:169-171) halves it and counts
        const double eta = !converged ? 0.25 : 0.5;
        h_abs *= eta;
        change_D(order, eta);
        n_equal = 0; lu_valid = false;
        st.n_rejected++;
        first_selection = false;   // (CVODE: any failed attempt sets etamax = 1, the first step's 1e4 is gone)
        if (converged) fail_score += 1.0;
        if (fail_score >= 3.0 && order > 1) reset_history();
        continue;
      }
      if (band > 0.0 && !fresh && a.n_iter >= RES_NEWTON_MAXITER) b.slot_drop(cur_slot);
      safety = bdf_safety(a.n_iter);
      err_norm = a.err;
      if (err_norm > 1.0) {
        const double factor = bdf_reject_factor(safety, err_norm, order);
        h_abs *= factor;
        change_D(order, factor);
        n_equal = 0;
        force_fresh_lu = band > 0.0;
        st.n_rejected++;
        first_selection = false;
        fail_score += 1.0;
        if (fail_score >= 3.0 && order > 1) reset_history();
      } else {
        if (a.deep_negative) return STEP_UNSTABLE;   // BDF_NEG_DEEP: the negative excursion, given up early
        accepted = true;
      }
    }
    st.n_steps++;
    steps_since_jac++;
    fail_score = fail_score - 0.2 > 0.0 ? fail_score - 0.2 : 0.0;
    n_equal++;
    t = t_new;
    b.accept(order);
    jac_current = false;
    pending_order_change = (n_equal >= order + 1);
    if (pending_order_change) {
      err_m = order > 1 ? a.err_m : bdf_inf();
      err_p = order < RES_MAX_ORDER ? a.err_p : bdf_inf();
      err_o = err_norm;
      safety_o = safety;
    }
    return STEP_OK;
  }

  KIN_HD void select_order() {
    if (!pending_order_change) return;
    pending_order_change = false;
    const BdfOrderChoice ch = bdf_select_order(order, err_m, err_o, err_p, safety_o, first_selection);
    order += ch.d_order;
    first_selection = false;
    h_abs *= ch.factor;
    change_D(order, ch.factor);
    n_equal = 0;
    lu_valid = false;
  }

  // dense output of the step that ended at t into solution row `row`
  KIN_HD void interpolate(double ts, int64_t row) {
    bdf_interp_weights(order, ts, t, h_abs, wp);
    b.interp(order, wp, row);
  }

  // ---- what res_drive (below) asks of an integrator; solver.cpp's HostDriven (this controller or the explicit mode, rows into a
  // buffer that grows) is the other one
  static constexpr bool saves_every_step = false;   // there is always a save grid (resident_setup.hpp: res_has_grid)
  KIN_HD void begin() { set_tols(P.abstol, P.reltol); dtmin = P.dtmin; invalidate_lu(); b.load_u0(); }   // the call's reset, state <- u0
  KIN_HD double time() const { return t; }
  KIN_HD int64_t iters() const { return iters_left; }
  KIN_HD void chunk_begin(int64_t) { st.n_chunks++; cache_suspended = false; b.chunk_start_from_y(); }
  KIN_HD void attempt_begin(int64_t maxiters) { iters_left = maxiters; }
  KIN_HD void apply_rates(int64_t stop) { b.apply_rates(stop); }
  // rows past the solution buffer are counted, not written
  KIN_HD void save_y(int64_t row, double tg) { if (row < P.sol_cap) b.save_y(row, tg); }
  KIN_HD void save_interp(int64_t row, double tl, double tg) { if (row < P.sol_cap) { interpolate(tl, row); b.set_time(row, tg); } }
  KIN_HD bool segment_start(double origin, double seg_len, bool warm) {
    seg_origin = origin;
    if (continuous()) rates_at(0.0);   // rates at the segment start for f0 / J of the restart
    // (continuous rates: every chunk start re-initialises, solve_chunks == 2 is 1)
    if (warm && !continuous()) { resume(); return true; }
    return restart(seg_len);
  }
  KIN_HD void segment_end(bool failed) { if (!failed) b.y_from_D0(); }
  KIN_HD void attempt_failed(int64_t, int, int, double, double, double) {}
  KIN_HD void retry(double a, double r, int64_t) {
    set_tols(a, r);
    st.n_retries++;
    invalidate_lu_keep_counters();
    cache_suspended = true;
    b.y_from_chunk_start_clipped();
  }

  // the whole solve; returns the result block
  KIN_HD ResResult run();
};

// ---- The solve driver: kin_solve's orchestration around an integrator `d`, written once. Chunk loop in local time, discrete rate
// updates at tstops with zero-order hold, segments, the per-chunk save grid with its dropped last point, warm chunk starts
// (solve_chunks == 2) and the adaptive_solve! tolerance retries. `D` integrates and stores: ResidentBdf<B> above (device kernel,
// CPU replays, lockstep ensemble members) and solver.cpp's HostDriven. What differs between them is an operation
// of D: where rows go (save_y / save_interp / retry's rewind), how a segment starts and ends, the host's diagnostics
// (chunk_begin, attempt_failed). D::saves_every_step: without a save grid (P.L == 0) every accepted step is a row (save_step).
// The solve's parameters are D's member P, read as d.P at every use: the device kernel's controller lives in LDS, and a copy
// of the reference held across the loop costs it registers (scratch grew by 32 bytes per lane with one).

// stops [from, result) lie at or before global time tg: the first stop not yet applied at tg
KIN_HD inline int64_t res_stops_passed(const double* tstops, int64_t n_stops, int64_t from, double tg) {
  while (from < n_stops && tstops[from] <= tg) from++;
  return from;
}
// index of the rates in force when `stop_i` is the first stop not yet applied: the last stop passed (zero-order hold); before
// the first stop: the initial conditions, stop 0
KIN_HD inline int64_t res_rates_at_stop(int64_t stop_i) { return stop_i > 0 ? stop_i - 1 : 0; }

// end, in chunk-local time (= global - shift), of the segment whose next stop is stop_i: that stop if it lies before the chunk's
// end (t_end_global, locally t_loc1), else the chunk's end
struct ResSegEnd { double end; bool at_stop; };
KIN_HD inline ResSegEnd res_segment_end(const double* tstops, int64_t n_stops, int64_t stop_i, double t_end_global, double shift,
                                        double t_loc1) {
  if (stop_i < n_stops && tstops[stop_i] < t_end_global) {
    const double loc = tstops[stop_i] - shift;
    if (loc < t_loc1) return ResSegEnd{loc, true};
  }
  return ResSegEnd{t_loc1, false};
}

// a step's outcome as a return code: D::step's status, D::iters() afterwards
KIN_HD inline int res_step_retcode(StepStatus ss, int64_t iters_left) {
  if (iters_left < 0) return RES_RET_MAXITERS;
  if (ss == STEP_DT_MIN) return RES_RET_DTLESSTHANMIN;
  if (ss == STEP_UNSTABLE) return RES_RET_UNSTABLE;
  return RES_RET_SUCCESS;
}

struct ResDriven { int retcode; int64_t n_saved; double abstol, reltol; };   // (the tolerances: as tightened by the retries)

template <class D>
KIN_HD ResDriven res_drive(D& d) {
  const bool chunks = d.P.solve_chunks != 0;
  const int L = d.P.L;
  bool every_step = false;
  if constexpr (D::saves_every_step) every_step = L == 0;
  d.begin();
  double abstol = d.P.abstol, reltol = d.P.reltol;
  int64_t next_stop = 0, n_saved = 0, rates_in_force = -1;
  bool have_history = false, rates_changed = false;   // warm continuation across chunk starts (solve_chunks == 2)
  int retcode = RES_RET_SUCCESS;
  for (int64_t nc = 0; nc < d.P.n_chunks && retcode == RES_RET_SUCCESS; nc++) {
    const double t_start_global = chunks ? d.P.chunkstep * (double)nc : d.P.tspan0;
    const double t_end_global = chunks ? t_start_global + d.P.chunkstep : d.P.tspan1;
    const double shift = chunks ? (double)nc * d.P.chunkstep : 0.0;   // global = local + shift
    const double t_loc0 = chunks ? 0.0 : d.P.tspan0;
    const double t_loc1 = chunks ? d.P.chunkstep : d.P.tspan1;
    // local stops of this chunk: tg - nc*chunkstep for tstops in [t_start, t_end) (methods.jl:798-800); the complete-timespan
    // variant takes all of them (methods.jl:697)
    const int64_t stop_first = next_stop;
    d.chunk_begin(nc);
    const int64_t saved_at_chunk_start = n_saved;
    int attempts = 0;
    for (;;) {   // adaptive_solve! (solve_utils.jl:376-424)
      attempts++;
      if (attempts > 1) have_history = false;   // a retry starts cold from the chunk's first state
      retcode = RES_RET_SUCCESS;
      d.attempt_begin(d.P.maxiters);
      int64_t stop_i = res_stops_passed(d.P.tstops, d.P.n_stops, stop_first, t_start_global);
      if (d.P.n_stops > 0) {
        const int64_t want = res_rates_at_stop(stop_i);
        if (want != rates_in_force) { d.apply_rates(want); rates_in_force = want; rates_changed = true; }
      }
      double t_seg = t_loc0;
      bool failed = false;
      // the chunk's first point (saveat = []: every step, starting with the initial state)
      d.save_y(n_saved, (every_step ? t_loc0 : d.P.save_local[0]) + shift);
      n_saved++;
      int save_i = 1;
      while (t_seg < t_loc1 && !failed) {
        const ResSegEnd seg = res_segment_end(d.P.tstops, d.P.n_stops, stop_i, t_end_global, shift, t_loc1);
        if (seg.end > t_seg) {
          // Every segment is integrated in segment-local time tau in [0, seg_len]: the rates are constant inside a segment
          // (autonomous system), and restarting at tau = 0 keeps the tiny first steps of a restart (1e-20 s is common) above the
          // floating-point resolution of the time variable - the underflow the reference's chunking exists to avoid
          // (docs/src/development/implementation-details.md:5-28) but re-creates at tstops > 0.
          const double seg_len = seg.end - t_seg;
          // every segment start re-initialises like the reference (reinit!, methods.jl:260, 819), except a chunk start of
          // solve_chunks == 2 whose rates did not change (a StaticODESolve's chunk boundaries)
          const bool warm = d.P.solve_chunks == 2 && have_history && !rates_changed;
          if (!d.segment_start(t_seg + shift, seg_len, warm)) { retcode = RES_RET_UNSTABLE; failed = true; break; }
          have_history = true;
          rates_changed = false;
          while (d.time() < seg_len) {
            retcode = res_step_retcode(d.step(seg_len), d.iters());
            if (retcode != RES_RET_SUCCESS) { failed = true; break; }
            const double t_abs = d.time() >= seg_len ? seg.end : t_seg + d.time();   // chunk-local time reached
            // saves covered by this step. The chunk's last local point: dropped except on the final chunk (methods.jl:829-846),
            // where it is the chunk's end state (saved below) or, off the grid, a dense-output value
            const int last = (chunks && !(nc == d.P.n_chunks - 1 && !d.P.save_hits_end)) ? L - 1 : L;
            while (save_i < last && d.P.save_local[save_i] <= t_abs) {
              const double tl = d.P.save_local[save_i] - t_seg;
              d.save_interp(n_saved, tl < d.time() ? tl : d.time(), d.P.save_local[save_i] + shift);
              n_saved++;
              save_i++;
            }
            if constexpr (D::saves_every_step) {
              if (every_step) { d.save_step(n_saved, t_abs + shift); n_saved++; }
            }
            d.select_order();
          }
          d.segment_end(failed);   // state at the segment end = D[0]
          if (failed) break;
        }
        t_seg = seg.end;
        if (seg.at_stop) { d.apply_rates(stop_i); rates_in_force = stop_i; stop_i++; rates_changed = true; }
      }
      if (!failed) {
        // the chunk's last save point goes to the output only on the final chunk; its value is the state at the chunk end
        if (chunks && nc == d.P.n_chunks - 1 && L > 1 && d.P.save_hits_end) {
          d.save_y(n_saved, d.P.save_local[L - 1] + shift);
          n_saved++;
        }
        next_stop = stop_i;
        break;
      }
      // failure: tighten the tolerances and redo this chunk from its (clipped) start state
      d.attempt_failed(nc, attempts, retcode, t_seg, abstol, reltol);
      rates_in_force = -1;
      const double mintol = 2.220446049250313e-16;
      if (!d.P.adaptive_tols || attempts >= 5 || abstol / 10 <= mintol || reltol / 10 <= mintol) break;
      abstol /= 10; reltol /= 10;
      n_saved = saved_at_chunk_start;
      d.retry(abstol, reltol, n_saved);
    }
  }
  return ResDriven{retcode, n_saved, abstol, reltol};
}

template <class B>
KIN_HD ResResult ResidentBdf<B>::run() {
  const ResDriven o = res_drive(*this);
  ResResult r;
  r.retcode = o.retcode; r.pad = 0; r.n_saved = o.n_saved; r.final_abstol = o.abstol; r.final_reltol = o.reltol; r.st = st;
  for (int i = 0; i < 20; i++) r.prof[i] = 0;
  b.profile_out(r.prof);
  return r;
}

}  // namespace kin
