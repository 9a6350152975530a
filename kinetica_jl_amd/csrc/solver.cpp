// kin_solve: the MI355X replacement for init / solve! / reinit! of the reference's stiff
// integrator together with the orchestration around it:
//   * chunkwise local-time solving + output stitching  (reference src/solving/methods.jl:185-303, 717-865)
//   * complete-timespan solving                        (methods.jl:132-183, 655-714)
//   * discrete rate-constant updates at tstops         (src/solving/solve_utils.jl:435-509)
//   * adaptive_solve! tolerance-tightening retries     (solve_utils.jl:376-424)
//
// Integrator. The reference delegates to a user-supplied SciML algorithm (documented choice:
// Sundials CVODE_BDF + KLU, docs/src/getting-started.md:69) that is not vendored, so the
// algorithm restated here is the published quasi-constant-step variable-order BDF/NDF of
// Shampine & Reichelt ("The MATLAB ODE Suite", SIAM J. Sci. Comput. 18, 1997; orders 1-5,
// backward-difference form, modified Newton with an iteration-count dependent safety factor,
// order selection from the error estimates one order down/up). oracle/bdf.py restates the
// same algorithm on the CPU; both are checked against closed-form and high-accuracy truths.
//
// Neither the orchestration nor the step algorithm is written here: the solve driver (resident_core.hpp: res_drive) and the
// BDF controller (ResidentBdf<B>) are shared with the resident integrator and the lockstep ensemble. This file holds the
// controller's host-driven backend (HostBackend: what an operation of the controller launches, and how its result comes
// back), the explicit Dormand-Prince mode, the adapter between driver and integrator (HostDriven) and what surrounds the loop.
//
// Control flow lives on the host; every vector operation, the RHS, the Jacobian, the LU and
// the triangular solves are device kernels on one stream. A step attempt enqueues predictor +
// two Newton iterations + error estimate blind (kernels turn into no-ops once the device-side
// convergence flag is set) and synchronises ONCE to read a 96-byte control block.
#include "solver.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <thread>

#include "lu.hpp"
#include "resident_setup.hpp"
#include "solver_kernels.hpp"

namespace kin {

namespace {
constexpr double MIN_FACTOR = 0.2, MAX_FACTOR = 10.0;   // the explicit pair's step-size factors (the BDF's rules: bdf_rules.hpp)
}  // namespace

struct HostBackend;
using HostBdf = ResidentBdf<HostBackend>;

// The backend of the host-driven integrator's controller (resident_core.hpp: ResidentBdf<HostBackend>): every operation is a
// launch (or a few) on the handle's stream; results come back through a pinned control block. What is asynchronous - the
// deferred accept, the blind corrector batches, the speculatively enqueued next step - lives here and nowhere else.
struct HostBackend {
  kin_network* h;
  const ResParams& P;
  const HostBdf* ctl = nullptr;           // the controller that drives this backend, to read (Solver's constructor sets it)
  int N;
  hipStream_t s;
  SparseLU lu;
  SegPlanDev resid_plan;                  // Newton residual written straight into the permuted solve vector
  DevBuf<double> D, y, psi, d, scale, f0, f1, ytmp, jv, red;
  DevBuf<double> chunk_start;             // the chunk's first state, for its retries
  DevBuf<BdfCtrl> ctrl;
  BdfCtrl* hc = nullptr;                  // pinned host mirror: the block of the hand-over last waited for (hc_buf[seq & 1])
  BdfCtrl* hc_buf = nullptr;
  BdfCoef cf;

  HostBackend(kin_network* hh, const ResParams& pp) : h(hh), P(pp), N((int)hh->host.N), s(hh->stream) {
    const NetworkHost& H = h->host;
    lu.analyze(N, H.j_ptr, H.j_col, lu_options_for(N), s);
    if (const char* e = getenv("KIN_INJECT_BAD_PIVOT")) inject_bad_pivot_at = atoll(e);
    if (const char* e = getenv("KIN_SPECULATE")) speculate = atoi(e) != 0;
    fuse_newton = lu.fused_tri && lu.m > 0 && lu.newton_grid() <= 10;
    if (const char* e = getenv("KIN_FUSE_NEWTON")) fuse_newton = atoi(e) != 0 && lu.fused_tri && lu.m > 0;
    d_jdiag.upload(H.j_diag, s);
    d_drift.alloc(LU_MAX_SLOTS + 1);
    KIN_HIP(hipHostMalloc((void**)&h_drift, (LU_MAX_SLOTS + 1) * sizeof(double), hipHostMallocDefault));
    h_drift[LU_MAX_SLOTS] = 0.0;
    std::vector<int32_t> yl(N), ident(N);
    lu.yloc.download(yl.data(), N, s);
    KIN_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < N; i++) ident[i] = i;
    resid_plan.upload(build_seg_plan(N, H.sp_ptr.data(), yl.data(), H.sp_rxn.data(), nullptr, H.sp_coef.data(), false, ident.data()), s);
    D.alloc((size_t)BDF_D_ROWS * N);
    y.alloc(N); psi.alloc(N); d.alloc(N); scale.alloc(N); f0.alloc(N); f1.alloc(N); ytmp.alloc(N); chunk_start.alloc(N);
    jv.alloc(H.nnz());
    ctrl.alloc(1);
    red.alloc((size_t)bdf_reduce_slot() * std::max(bdf_reduce_blocks(N), (lu.fused_tri && lu.m > 0) ? lu.newton_grid() : 0));
    KIN_HIP(hipMemsetAsync(ctrl.p, 0, sizeof(BdfCtrl), s));
    // the step-end hand-over needs device writes to become visible to the spinning host thread while the stream
    // keeps running: fine-grained (coherent), device-mapped pinned memory
    // (two blocks, used alternately by consecutive hand-overs: with a speculatively enqueued step behind the one the host
    // is reading, the next publication must not land in the block being read)
    KIN_HIP(hipHostMalloc((void**)&hc_buf, 2 * sizeof(BdfCtrl), hipHostMallocCoherent | hipHostMallocMapped));
    hc = hc_buf;
    KIN_HIP(hipHostMalloc((void**)&hseq, sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped));
    *hseq = 0;
    if (hipHostGetDevicePointer((void**)&hc_dev, hc_buf, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&hseq_dev, hseq, 0) != hipSuccess || getenv("KIN_NO_FAST_SYNC")) {
      (void)hipGetLastError();
      fast_sync = false; fast_sync_allowed = false; hc_dev = nullptr; hseq_dev = nullptr;
    }
    bdf_fill_coef(cf.gamma, cf.alpha, cf.error_const);
  }
  ~HostBackend() { if (hc_buf) (void)hipHostFree(hc_buf); if (hseq) (void)hipHostFree(hseq); if (h_drift) (void)hipHostFree(h_drift); }
  HostBackend(const HostBackend&) = delete;

  // LU cache (CVODE keeps ONE factorisation while gamma drifts < 30 %; with 288 GB of HBM this solver keeps MANY):
  // factorisations stay resident in slots and are reused - across step-size changes AND across restarts (every chunk
  // start and rate update replays the same ramp of step sizes) - whenever a slot's c_fact is within the band of the
  // current c = h / alpha_k (the rules: the controller; the settings and their reasons: resident_setup.hpp).
  // Cache size: KIN_LU_CACHE_SLOTS (default 128), bounded by KIN_LU_CACHE_MB of device memory. A restart replays a ramp of
  // step sizes over up to ~12 decades of c; slots sit >= 35 % apart, i.e. ~8 per decade: the cache must hold the whole ramp
  // (~90 slots), or the cyclic sweep evicts every slot just before its next use (32 slots: the full C4 run made 405 k
  // factorisations; its first second, a narrower ramp, only 446)
  int cache_slots() const {
    size_t budget_mb = lu_env_budget_mb();
    if (h->lu_budget_mb > 0) budget_mb = std::min(budget_mb, h->lu_budget_mb);   // a replica's share (ensemble_routes.cpp: replica_ensemble)
    const size_t fit = std::max<size_t>(1, budget_mb * 1024 * 1024 / std::max<size_t>(1, lu.slot_bytes()));
    return (int)std::min<size_t>(std::min<size_t>((size_t)lu_env_slots(128), fit), (size_t)LU_MAX_SLOTS);
  }

  // what every call on the handle starts with: nothing pending of an earlier call survives (its solution buffer may be gone)
  void begin_call() {
    accept_pending = false; accept_copy = nullptr;
    spec = Spec{};
    sync_wait_s = 0.0;
    std::fill(iter_hist, iter_hist + 8, 0);
  }
  // ... and every segment: no speculative batch, no deferred accept
  void begin_segment() { spec = Spec{}; flush_accept(); }

  // step-end hand-over without a stream synchronisation: the corrector launch that decides the attempt publishes the
  // control block into pinned host memory and bumps `*hseq`; the host spins on it (bounded), else falls back to sync_ctrl()
  unsigned long long* hseq = nullptr;
  BdfCtrl* hc_dev = nullptr;                // device-side address of hc
  unsigned long long* hseq_dev = nullptr;
  unsigned long long seq_no = 0;
  bool fast_sync = true, fast_sync_allowed = true;
  int64_t n_sync_fallbacks = 0;   // step-end hand-overs that timed out and went through copy + stream sync (KIN_TIMING=1)
  int sync_ok_streak = 0;
  double sync_wait_s = 0.0;   // host time spent blocked in sync_ctrl (diagnostic, KIN_TIMING=1)
  BdfCtrl* hc_dev_at(unsigned long long seq) const { return hc_dev ? hc_dev + (seq & 1) : nullptr; }
  void wait_ctrl(unsigned long long want) {
    auto t0 = std::chrono::steady_clock::now();
    hc = hc_buf + (want & 1);
    if (fast_sync) {
      for (unsigned spins = 0;; spins++) {
        // (>=: a speculative batch behind the awaited one may have published its own number by the time the host looks)
        if (*(volatile unsigned long long*)hseq >= want) {
          std::atomic_thread_fence(std::memory_order_acquire);
          sync_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          return;
        }
        // not seen within 50 ms (an attempt incl. a large factorisation takes a few ms at most): the platform does not
        // make device writes to pinned host memory visible while the kernel runs - use the synchronising path from now on
        if ((spins & 1023) == 1023 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 50e-3) {
          fast_sync = false; n_sync_fallbacks++; sync_ok_streak = 0; break;
        }
        // a hand-over takes 10-100 us: spin politely (the sibling hardware thread keeps its issue slots), and once the wait
        // is longer than a plain attempt - a factorisation is in the batch, or K handles share fewer cores - give the core away
        __builtin_ia32_pause();
        if (spins > 20000 && (spins & 63) == 63) std::this_thread::yield();
      }
    }
    sync_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    sync_ctrl();
    // a slow wait may have been a one-off (first-launch code loading, a profiler, a preempted GPU): after 64
    // synchronising hand-overs in a row whose sequence number DID arrive the fast path is tried again
    if (fast_sync_allowed && !fast_sync && *(volatile unsigned long long*)hseq >= want && ++sync_ok_streak >= 64) {
      fast_sync = true; sync_ok_streak = 0;
    }
  }
  int64_t iter_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // corrector iterations executed per converged attempt (diagnostic)
  void sync_ctrl() {
    // (with a speculative step enqueued behind the awaited batch the device block has moved on by the time the stream
    // is idle; the awaited batch's last launch has published its block to hc all the same)
    if (!spec.enq) KIN_HIP(hipMemcpyAsync(hc, ctrl.p, sizeof(BdfCtrl), hipMemcpyDeviceToHost, s));
    auto t0 = std::chrono::steady_clock::now();
    KIN_HIP(hipStreamSynchronize(s));
    sync_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    drift_landed = true;
  }

  // ---- slot table of the LU cache: SparseLU's slots, allocated on demand up to P.n_slots
  double slot_c_fact(int i) const { return lu.slots[i].c_fact; }
  double slot_crate(int i) const { return lu.slots[i].crate; }
  long long slot_crate_step(int i) const { return lu.slots[i].crate_step; }
  long long slot_crate_restart(int i) const { return lu.slots[i].crate_restart; }
  void slot_touch(int i, long long clock) { lu.slots[i].last_use = clock; }
  void slot_rate(int i, double cr, long long st, long long rs) { SparseLU::Slot& q = lu.slots[i]; q.crate = cr; q.crate_step = st; q.crate_restart = rs; }
  void slot_drop(int i) { lu.slots[i].valid = false; }
  void slot_made(int i, double c, long long clock, long long js, long long ss) {
    SparseLU::Slot& q = lu.slots[i];
    q.c_fact = c; q.crate = 1.0; q.valid = true; q.last_use = clock; q.jac_stamp = js; q.step_stamp = ss;
  }
  void slots_invalidate(bool reset) { for (auto& q : lu.slots) { q.valid = false; if (reset) { q.c_fact = 0.0; q.last_use = 0; } } }
  int nearest_slot(double c, double band, long long n_restarts, long long max_age, long long n_steps = 0, long long step_age = -1) const {
    return slot_nearest(lu.slots.data(), (int)lu.slots.size(), c, band, n_restarts, max_age, n_steps, step_age);
  }
  // a slot for a new factorisation: an unused or expired one, else a new one (allocated on demand), else the least recently used
  int victim_slot(long long n_restarts, long long max_age, int n_slots) {
    const int n = (int)lu.slots.size();
    const int free_ = slot_first_free(lu.slots.data(), n, n_restarts, max_age);
    if (free_ >= 0) return free_;
    if (n < n_slots) { lu.ensure_slots(n + 1, s); return n; }
    return slot_lru(lu.slots.data(), n);
  }

  // ---- vectors, right-hand sides, Jacobian
  // The accept of a step (D <- D + d, new difference rows) is deferred and rides in the next step's predictor launch
  // (bdf_accept_predict_kernel: both are one pass over the same columns of D); so does the copy of the new state into
  // the solution buffer when every step is saved. Everything else that reads D calls flush_accept() first.
  bool accept_pending = false;
  int accept_order = 0;
  double* accept_copy = nullptr;
  void flush_accept() {
    if (!accept_pending) return;
    launch_bdf_accept(N, accept_order, D.p, d.p, accept_copy, s);
    accept_pending = false; accept_copy = nullptr;
  }
  void accept(int order) {
    if (spec.enq) {   // the device has accepted this step and is computing the next one: nothing is pending
      spec.alive = true; spec.enq = false;
      accept_pending = false; accept_copy = nullptr;
    } else {
      accept_pending = true; accept_order = order; accept_copy = nullptr;   // rides in the next predictor launch
    }
  }
  void predict(int order, const double*, double, double atol, double rtol) {
    drop_take_up();
    launch_predict(order, atol, rtol);
  }
  void launch_predict(int order, double atol, double rtol) {
    if (accept_pending) {
      launch_bdf_accept_predict(N, accept_order, order, D.p, cf, atol, rtol, y.p, psi.p, d.p, scale.p, ctrl.p, accept_copy, s);
      accept_pending = false; accept_copy = nullptr;
    } else
      launch_bdf_predict(N, order, D.p, cf, atol, rtol, y.p, psi.p, d.p, scale.p, ctrl.p, s);
  }
  // the state after the last accepted step (D[0]), for readers outside the integrator
  double* state_ptr() { flush_accept(); return D.p; }
  // copy of that state into `dst` (a row of the solution buffer): rides with the pending accept when there is one
  void save_state(double* dst) {
    if (accept_pending && !accept_copy) accept_copy = dst;
    else copy(dst, state_ptr());
  }
  void copy(double* dst, const double* src) { KIN_HIP(hipMemcpyAsync(dst, src, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s)); }
  double* row(long long r) { return h->d_sol_u.p + (size_t)r * N; }   // of the handle's solution buffer (HostDriven reserves it)

  void chunk_start_from_y() { copy(chunk_start.p, y.p); }
  // The retried chunk starts from its start state with NEGATIVE entries set to zero. A chunk can inherit concentrations
  // of -1e-9 (tolerance-sized, 10 x abstol is common) from its predecessor, and mass-action kinetics is unstable under
  // them - a bimolecular term flips its sign - up to a finite-time blow-up of the exact solution from that state: every
  // retry then dies at the same local time whatever its tolerances (3k species, 1 500 K: five attempts, all at
  // t = 7.0e-4). The first attempt of a chunk is untouched (reference semantics); only the rescue path clips.
  void y_from_chunk_start_clipped() { launch_clip_negative(N, chunk_start.p, y.p, s); }
  void y_from_D0() { copy(y.p, state_ptr()); }
  void ytmp_from_D0() { copy(ytmp.p, state_ptr()); }
  void ytmp_axpy(double h0) { launch_axpy_out(N, y.p, h0, f0.p, ytmp.p, s); }
  void rhs_y_to_f0() { h->rhs_dev(y.p, f0.p); }
  void rhs_ytmp_to_f1() { h->rhs_dev(ytmp.p, f1.p); }
  void rhs_ytmp_to_f0() { h->rhs_dev(ytmp.p, f0.p); }
  void eval_jac_y() { drop_take_up(); h->jac_dev(y.p, jv.p); }
  // continuous rates: no launch - the first kernel of the attempt that reads k forms it from this temperature (handle.hpp)
  void apply_T(double T) { h->set_pending_T(T); }
  ResNorms norms(bool with_f1, double atol, double rtol) {
    launch_bdf_norms(N, y.p, f0.p, with_f1 ? f1.p : nullptr, atol, rtol, ctrl.p, s);
    sync_ctrl();
    return ResNorms{hc->scratch[0], hc->scratch[1], hc->scratch[2], hc->scratch[3], hc->nonfinite};
  }
  void init_D(bool from_ytmp, double hh) {
    drop_take_up();
    launch_bdf_init_D(N, BDF_D_ROWS, from_ytmp ? ytmp.p : y.p, f0.p, hh, D.p, s);
  }
  void change_D(int ord, const double (*RU)[6]) {
    drop_take_up();
    flush_accept();
    BdfMat ru;
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) ru.v[i][j] = RU[i][j];
    launch_bdf_change_D(N, ord, ru, D.p, s);
  }
  void interp(int order, const double* p, long long r) {
    flush_accept();
    BdfVec pv;
    for (int j = 0; j <= BDF_MAX_ORDER; j++) pv.v[j] = p[j];
    launch_bdf_interp(N, order, D.p, pv, row(r), s);
  }

  // ---- drift guard of the LU cache (its reasons: resident_setup.hpp). The test is launched behind the Jacobian of a
  // restart and read after the synchronisation the restart's norms need anyway; a warm chunk start has none and waits here
  DevBuf<int32_t> d_jdiag;
  DevBuf<double> d_drift;
  double* h_drift = nullptr;     // pinned
  int n_drift_checked = 0;
  bool drift_landed = true;      // the stream has been waited for since the last drift test was launched
  void drift_launch(double) {
    n_drift_checked = launch_drift_test(N, lu.slots, jv.p, d_jdiag.p, d_drift.p, h_drift, s);
    drift_landed = false;
  }
  int drift_collect(double max_drift) {
    if (!drift_landed) { KIN_HIP(hipStreamSynchronize(s)); drift_landed = true; }
    return drop_drifted(lu.slots, n_drift_checked, h_drift, max_drift);
  }

  // the flag of a vanished pivot arrives with the corrector's control block (ResAttempt::bad_pivot), not here
  bool factor(int slot, double c, bool keep_diag) {
    drop_take_up();
    lu.factor(c, jv.p, slot, &ctrl.p->lu_bad, s);
    if (keep_diag) {
      lu.slots[slot].jd.alloc(N);
      launch_jac_diag(N, jv.p, d_jdiag.p, lu.slots[slot].jd.p, s);
    }
    return false;
  }

  // ---- the corrector
  // The corrector update folded into the solve's last gather launch (stagec_newton_kernel). One launch less per iteration,
  // but every workgroup of the gather then takes part in the reduction hand-over (partial sums + arrival ticket), and that
  // costs ~0.3 us per workgroup: measured per 20-chunk solve, fused against separate: 300 species 0.101 / 0.110 s, 1 000
  // 0.107-0.110 / 0.116, 2 000 0.139 / 0.138, 5 000 0.204 / 0.174, 10 000 (65 workgroups) 0.572 / 0.449 s per 100 chunks.
  // Default: fused when the fused launch has at most 10 workgroups; KIN_FUSE_NEWTON=1 / 0 forces it on / off.
  bool fuse_newton = false;
  int last_iters = 0, last_iter_slot = -1;
  // the residual pair of a corrector iteration: the rates of y and c f(y) - psi - d into the permuted solve vector inside W;
  // both no-ops once *skip is set (a pending temperature's rate constants are stored all the same)
  void launch_residual(double c, const int* skip, double* W) {
    SegExtra ex;
    ex.psi = psi.p; ex.d = d.p; ex.cscal = c; ex.skip = skip;
    // (forming the rates inside the residual gather - three gathers per entry instead of one, no rate launch - was
    // measured slower: 0.565 against 0.553 s on the C3 solve)
    if (h->k_pending) { launch_rates_skip_T(h->host.R, h->pending_at(), h->k.p, y.p, h->x0.p, h->x1.p, h->rate.p, skip, s); h->k_pending = false; }
    else launch_rates_skip(h->host.R, h->k.p, y.p, h->x0.p, h->x1.p, h->rate.p, skip, s);
    launch_segsum(resid_plan.view(), SEG_COEF_BDF, h->rate.p, W, ex, s);
  }
  // `last`: the batch's last launch publishes the control block even when nothing is decided yet (seq = the number the
  // host waits for; the launch that decides publishes it itself - there is no separate error-estimate launch)
  // `spec_it`: an iteration of a speculatively enqueued step - the carried rate comes from the device's control block (the
  // host does not know yet what the step before leaves there)
  void newton_iteration(int it, const ResCorrIn& in, unsigned long long seq, bool last, bool spec_it = false) {
    const int* skip = &ctrl.p->newton_done;
    SparseLU::Slot& q = lu.slots[in.slot];
    launch_residual(in.c, skip, q.W.p);
    if (fuse_newton) {
      // the solve's last gather stage and the corrector update in one launch
      NewtonFuse f;
      f.skip = skip; f.N = N; f.m = 0; f.off_x = 0; f.x2_species = nullptr;
      f.scale = scale.p; f.y = y.p; f.d = d.p; f.D = D.p; f.order = in.order;
      f.upd = in.upd; f.atol = in.atol; f.rtol = in.rtol;
      f.ec = in.ec; f.ec_m = in.ec_m; f.ec_p = in.ec_p;
      f.iter = it; f.maxit = BDF_NEWTON_MAXITER; f.tol = in.newton_tol; f.rate_max = in.rate_max; f.crate0 = in.crate0;
      f.tol_first = in.tol_first; f.dy_first_max = in.dy_first_max; f.crate_from_ctrl = spec_it ? 1 : 0; f.ban_negatives = P.ban_negatives ? 1 : 0;
      f.ctrl = ctrl.p; f.part = red.p; f.host_ctrl = hc_dev_at(seq); f.host_seq = hseq_dev; f.seq = seq; f.publish_always = last ? 1 : 0;
      lu.solve_newton(in.slot, f, s);
    } else {
      lu.solve(skip, in.slot, s);
      launch_bdf_newton(N, it, BDF_NEWTON_MAXITER, in.newton_tol, lu.xloc.p, q.W.p, scale.p, y.p, d.p, in.upd, in.rate_max, in.crate0,
                        in.tol_first, in.dy_first_max, in.order, D.p, in.atol, in.rtol, cf, ctrl.p, red.p, hc_dev_at(seq), hseq_dev, seq, last, s,
                        spec_it, P.ban_negatives != 0);
    }
  }

  // ---- Speculative enqueue of the next step (KIN_SPECULATE=0 switches it off). The quasi-constant-step BDF keeps step size
  // and order for order + 1 steps, so after most steps the next one is fully known in advance IF this one is accepted: its
  // accept + predictor launch and its first corrector batch are enqueued right behind this step's batch, before the host has
  // seen this step's result. The deciding corrector launch writes `spec_go` (1 = accepted, by the host's own rule); the
  // speculative predictor does nothing unless it reads 1, and then the iterations behind it stay no-ops as well. The host
  // takes the batch up when the controller asks for the next step's corrector (same arithmetic, bit-identical results) - the
  // device no longer idles for the hand-over, the host's decision and the launch latency of the next predictor (~8-10 us of
  // ~100 per step).
  bool speculate = true;
  bool hold_speculation = false;   // set by integrator_step for the LAST step of a call: nothing half-run may outlive the call
  struct Spec {
    bool enq = false;      // a speculative batch sits behind the batch being waited for
    bool alive = false;    // ... and the device ran it: the next corrector takes it up instead of enqueueing
    unsigned long long seq = 0;
    double t_new = 0.0, hh = 0.0, c = 0.0;
    int slot = -1, blind = 0, order = 0;
  } spec;
  int64_t n_spec = 0, n_spec_dead = 0;   // speculative batches taken up / enqueued for nothing (KIN_TIMING=1)
  double att_t_new = 0.0, att_t_bound = 0.0;   // the attempt under way ends at att_t_new, its segment at att_t_bound
  // fault injection for the tests (KIN_INJECT_BAD_PIVOT=n): the n-th step attempt of a call finds the flag raised, as
  // if its factorisation had met a vanishing pivot (in accuracy-controlled integration of mass-action kinetics that
  // needs c J_ii ~ 1 on an autocatalytic species and practically never happens by itself)
  int64_t inject_bad_pivot_at = -1, attempt_no = 0;
  bool trace = false;   // KIN_TRACE_CHUNK=n: one line per corrector attempt of chunk n (diagnostic)
  // the controller's hook: a step attempt begins
  void attempt_begin(double t_new, double t_bound) {
    att_t_new = t_new; att_t_bound = t_bound;
    if (attempt_no++ == inject_bad_pivot_at) KIN_HIP(hipMemsetAsync(&ctrl.p->lu_bad, 1, sizeof(int), s));
  }
  // called right after the blind batch of the attempt `in` is enqueued
  void enqueue_speculative(const ResCorrIn& in, int blind) {
    if (!speculate || hold_speculation || !fast_sync || ctl->continuous() || trace || inject_bad_pivot_at >= 0 || P.lu_band <= 0.0 ||
        ctl->cache_suspended) return;
    if (ctl->n_equal >= in.order) return;              // the step after this one may change order / step size
    if (ctl->iters_left < 1) return;
    const double h_abs = ctl->h_abs, t2 = att_t_new + h_abs;
    if (t2 - att_t_bound > 0.0) return;                // would be cut at the segment end
    if (h_abs < bdf_min_step(ctl->dtmin, att_t_new)) return;
    const double hh2 = t2 - att_t_new, c2 = hh2 / cf.alpha[in.order];
    // (the slot can only drop out by the rule that also clears spec_go)
    if (nearest_slot(c2, P.lu_band, ctl->st.n_restarts, P.lu_max_age) != in.slot) return;
    const SparseLU::Slot& q = lu.slots[in.slot];
    // the carried rate must count as fresh in the next step whether or not this one measures it anew
    if (!(q.crate < 1.0 && q.crate_restart == ctl->st.n_restarts && (ctl->st.n_steps + 1) - q.crate_step <= P.crate_max_age)) return;
    spec.enq = true; spec.alive = false;
    spec.t_new = t2; spec.hh = hh2; spec.c = c2; spec.slot = in.slot; spec.blind = blind; spec.order = in.order;
    spec.seq = ++seq_no;
    launch_bdf_accept_predict(N, in.order, in.order, D.p, cf, in.atol, in.rtol, y.p, psi.p, d.p, scale.p, ctrl.p, nullptr, s, &ctrl.p->spec_go);
    // the next step's attempt as the controller will hand it in, except that its carried rate counts as fresh whatever this
    // step does (checked above)
    ResCorrIn in2 = in;
    in2.c = c2;
    in2.upd = res_update_scale(q.c_fact, c2, P.lu_band);
    in2.rate_max = q.c_fact == c2 ? 1.0 : P.reuse_rate_max;
    in2.tol_first = in.newton_tol;
    for (int b = 0; b < blind; b++) newton_iteration(b, in2, spec.seq, b == blind - 1, true);
  }
  void drop_speculation() { if (spec.enq || spec.alive) n_spec_dead++; spec.enq = false; spec.alive = false; }
  // an operation between two steps that the speculative batch did not foresee (cannot happen by the rules of
  // enqueue_speculative; kept as a recovery, not a throw): the device HAS accepted the previous step, so D is current and
  // nothing is pending - the next corrector re-runs the predictor (which clears the control block) and enqueues a batch of
  // its own; what the speculative iterations left in y / d is rebuilt by that predictor
  void drop_take_up() { if (spec.alive) drop_speculation(); }

  // One corrector attempt: predictor + iterations until the device has decided, the next step's batch behind them.
  ResAttempt corrector(const ResCorrIn& in, const double*) {
    // Blind depth: two iterations are enqueued ahead of the decision, one when this factorisation converged the previous
    // step in its first iteration (the carried rate makes that the common case; the second launch chain would be
    // six no-ops). Whatever is not decided when the host looks gets up to two more iterations per hand-over.
    int it = 0;
    int blind = (last_iters == 1 && last_iter_slot == in.slot && ctl->crate_fresh(in.slot)) ? 1 : 2;
    unsigned long long batch_seq;
    // this attempt's first batch is on the device already (enqueued speculatively behind the previous step's), if the
    // controller arrived at the step it was enqueued for
    if (spec.alive && !(att_t_new == spec.t_new && ctl->h_abs == spec.hh && in.c == spec.c && in.order == spec.order && in.slot == spec.slot))
      drop_take_up();
    if (spec.alive) {       // predictor and `blind` iterations of this attempt are running already
      spec.alive = false;
      blind = spec.blind; it = blind; batch_seq = spec.seq;
      n_spec++;
    } else {
      launch_predict(in.order, in.atol, in.rtol);
      batch_seq = ++seq_no;
      for (int b = 0; b < blind; b++, it++) newton_iteration(it, in, batch_seq, b == blind - 1);
    }
    enqueue_speculative(in, blind);
    wait_ctrl(batch_seq);
    while (!hc->newton_done && it < BDF_NEWTON_MAXITER) {
      if (spec.enq) {       // undecided: the speculative batch behind has ended itself and left newton_done raised
        KIN_HIP(hipMemsetAsync(&ctrl.p->newton_done, 0, sizeof(int), s));
        drop_speculation();
      }
      const int more = std::min(2, BDF_NEWTON_MAXITER - it);
      ++seq_no;
      for (int b = 0; b < more; b++, it++) newton_iteration(it, in, seq_no, b == more - 1);
      wait_ctrl(seq_no);
    }
    if (spec.enq && !(hc->newton_done && hc->spec_go)) drop_speculation();   // the device did not run it either
    ResAttempt a{};
    a.done = hc->newton_done != 0; a.converged = hc->converged != 0; a.nonfinite = hc->nonfinite != 0;
    a.any_negative = hc->any_negative != 0; a.deep_negative = (hc->any_negative & 2) != 0; a.bad_pivot = hc->lu_bad != 0;
    a.n_iter = hc->n_iter;   // iterations the device executed (blind launches behind the decision are no-ops)
    a.err = hc->err_norm; a.err_m = hc->err_m_norm; a.err_p = hc->err_p_norm; a.crate = hc->crate;
    last_iters = (a.done && a.converged) ? a.n_iter : 0;
    last_iter_slot = in.slot;
    if (trace)
      fprintf(stderr, "[trace] t=%.6e h=%.3e order=%d c=%.3e slot=%d c_fact=%.3e slot_fresh=%d jac_cur=%d -> done=%d conv=%d iters=%d dy=%.3e err=%.3e nonfinite=%d lu_bad=%d\n",
              ctl->t, ctl->h_abs, in.order, in.c, in.slot, lu.slots[in.slot].c_fact, (int)ctl->slot_is_fresh, (int)ctl->jac_current,
              hc->newton_done, hc->converged, hc->n_iter, hc->dy_norm, hc->err_norm, hc->nonfinite, hc->lu_bad);
    if (a.bad_pivot) KIN_HIP(hipMemsetAsync(&ctrl.p->lu_bad, 0, sizeof(int), s));   // (cleared by the host, not by the predictor)
    else if (a.done && a.converged && !a.nonfinite && !(P.ban_negatives && a.any_negative)) iter_hist[std::min(a.n_iter, 7)]++;
    return a;
  }
};

static_assert(ResIsAsync<HostBackend>::value && ResHasApplyT<HostBackend>::value, "the controller must find this backend's own operations");

// What a handle owns for its host-driven solves: the backend, the controller on it (its settings and the call's parameters in
// P), and the explicit Dormand-Prince 5(4) mode (kin_solve_explicit; SciPy's RK45 is the oracle), which shares the backend's
// vectors and control block and the controller's scalars (t, h_abs, tolerances, iters_left, the counters).
struct Solver {
  ResParams P{};
  HostBackend b;
  HostBdf ctl;
  // explicit mode: stage array K[7][N], state before the last step (dense output), FSAL derivative in K[0]
  bool explicit_mode = false;
  DevBuf<double> rk_K, rk_yold, rk_ynew;
  double rk_h_last = 0.0;

  explicit Solver(kin_network* h) : b(h, P), ctl(b, P) {
    b.ctl = &ctl;
    // the controller's settings (resident_setup.hpp), with this path's cache size; the Newton update is scaled for a
    // factorisation made at another c only inside the reuse band (a matrix kept across an error-test rejection with the cache
    // off or suspended is used unscaled)
    res_default_settings(P, LU_MAX_SLOTS);
    P.n_slots = b.cache_slots();
    P.lu_band = lu_env_band(P.n_slots);
    P.upd_in_band = 1;
  }

  // the reset every call on the handle starts with (solve_entry, integrator_init). The LU cache lives within one call:
  // identical calls give identical results. `g`: the call's save grid (none: ResGrid{})
  void begin_call(const kin_params& p, const ResGrid& g, bool explicit_solver) {
    forget_call();
    res_fill_params(P, p, g);
    P.dtmin = res_dtmin(p);
    P.save_local = g.save_local.empty() ? nullptr : g.save_local.data();
    explicit_mode = explicit_solver;
    b.begin_call();
    ctl.st = ResStats{};
    reset_cache();
    ctl.force_jac_refresh = false;
    ctl.dtmin = P.dtmin;
    ctl.set_tols(p.abstol, p.reltol);
  }
  // continuous rate updates: T(t) = linear interpolation of the nodes in global time (resident_core.hpp: res_T_of), the rate
  // constants re-evaluated on the device at every step attempt
  void set_profile(const double* t_nodes, const double* T_nodes, int64_t n_nodes) {
    P.rate_mode = 3; P.t_nodes = t_nodes; P.T_nodes = T_nodes; P.n_nodes = n_nodes;
    b.h->has_rates = true;
  }

  // P points into the call that filled it (its save grid, the caller's stops and profile nodes): nothing of a finished
  // kin_solve stays behind (CallGuard). An integrator session's pointers are into its own IntegratorState and stay
  void forget_call() {
    P.save_local = nullptr; P.L = 0;
    P.tstops = nullptr; P.n_stops = 0;
    P.t_nodes = P.T_nodes = nullptr; P.n_nodes = 0;
    P.rate_mode = 0;
  }
  // an empty LU cache; KIN_INJECT_BAD_PIVOT counts its attempts from here (every call, and the probes, which borrow slot 0)
  void reset_cache() { ctl.invalidate_lu(); b.attempt_no = 0; }

  // the controller's counters and the tolerances a call ended with, for res_stats (resident_setup.hpp)
  ResResult result(int retcode, double abstol, double reltol) const {
    ResResult r{};
    r.retcode = retcode; r.final_abstol = abstol; r.final_reltol = reltol; r.st = ctl.st;
    return r;
  }

  // (re)start at segment-local time 0 from the state in y, over a segment whose origin is global time `origin`; `warm`: the
  // controller's warm continuation, if the mode allows. Returns false when f(y0) is not finite.
  bool segment_start(double origin, double seg_len, bool warm) {
    b.begin_segment();
    if (!explicit_mode) return ctl.segment_start(origin, seg_len, warm);   // (y = D[0] since the segment before ended)
    ctl.seg_origin = origin;
    if (ctl.continuous()) ctl.rates_at(0.0);   // rates at the segment start for f0 of the restart
    return rk_restart(seg_len);
  }
  StepStatus step(double t_bound) { return explicit_mode ? rk_step_fsal(t_bound) : ctl.step(t_bound); }
  void select_order() { if (!explicit_mode) ctl.select_order(); }
  // dense output of the step that ended at ctl.t into row `row` of the solution buffer
  void interpolate(double ts, int64_t row) {
    if (explicit_mode) rk_interpolate(ts, b.row(row));
    else ctl.interpolate(ts, row);
  }

  void rhs(const double* u, double* out) { b.h->rhs_dev(u, out); ctl.st.n_rhs++; }

  bool rk_restart(double t_bound) {
    const int N = b.N;
    ctl.t = 0.0;
    ctl.st.n_restarts++;
    rhs(b.y.p, b.f0.p);
    const ResNorms n0 = b.norms(false, ctl.atol, ctl.rtol);
    if (n0.nonfinite) return false;
    const double interval = std::fabs(t_bound);
    // the explicit pair keeps SciPy's select_initial_step (its oracle is SciPy's own RK45): exponent 1 / (error order + 1)
    double h0 = (n0.d0 < 1e-5 || n0.d1 < 1e-5) ? 1e-6 : 0.01 * n0.d0 / n0.d1;
    h0 = std::min(h0, interval);
    b.ytmp_axpy(h0);
    rhs(b.ytmp.p, b.f1.p);
    const ResNorms n1 = b.norms(true, ctl.atol, ctl.rtol);
    if (n1.nonfinite) return false;
    const double d1 = n0.d1, d2 = n1.d2 / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 0.2);
    ctl.h_abs = std::min({100.0 * h0, h1, interval});
    rk_K.alloc((size_t)7 * N); rk_yold.alloc(N); rk_ynew.alloc(N);
    b.copy(b.D.p, b.y.p);          // D[0] = current state
    b.copy(rk_K.p, b.f0.p);        // FSAL: K[0] = f(y0)
    b.copy(rk_yold.p, b.y.p);
    rk_h_last = 0.0;
    rk_fsal_pending = false;
    return true;
  }

  // One accepted explicit step (Dormand & Prince 1980, the RK5(4)7M pair; step-size control as in SciPy's
  // RK45: SAFETY 0.9, factors in [0.2, 10], no growth right after a rejection, FSAL). The state lives in D[0].
  StepStatus rk_step(double t_bound) {
    static const double A[6][5] = {{0, 0, 0, 0, 0},
                                   {1.0 / 5, 0, 0, 0, 0},
                                   {3.0 / 40, 9.0 / 40, 0, 0, 0},
                                   {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
                                   {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
                                   {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
    static const double Bw[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    static const double E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
    const int N = b.N;
    hipStream_t s = b.s;
    double& t = ctl.t;
    double& h_abs = ctl.h_abs;
    const bool ban_negatives = P.ban_negatives != 0;
    bool rejected = false;
    for (;;) {
      if (ctl.iters_left-- <= 0) return STEP_OK;   // caller checks iters_left < 0 -> MaxIters
      const double min_step = bdf_min_step(ctl.dtmin, t);
      if (h_abs < min_step) {
        if (rejected) return STEP_DT_MIN;
        h_abs = min_step;                       // SciPy clips the proposed step to [min_step, max_step] once per step
      }
      double t_new = t + h_abs;
      if (t_new - t_bound > 0.0) t_new = t_bound;
      const double hh = t_new - t;
      h_abs = std::fabs(hh);
      if (ctl.continuous()) ctl.rates_at(t_new);
      RkVec w;
      for (int st_i = 1; st_i < 6; st_i++) {
        for (int j = 0; j < 7; j++) w.v[j] = j < st_i ? hh * A[st_i][j] : 0.0;
        launch_rk_combine(N, st_i, w, b.D.p, rk_K.p, b.ytmp.p, s);
        rhs(b.ytmp.p, rk_K.p + (size_t)st_i * N);
      }
      for (int j = 0; j < 7; j++) w.v[j] = j < 6 ? hh * Bw[j] : 0.0;
      launch_rk_combine(N, 6, w, b.D.p, rk_K.p, rk_ynew.p, s);
      rhs(rk_ynew.p, rk_K.p + (size_t)6 * N);
      RkVec e;
      for (int j = 0; j < 7; j++) e.v[j] = hh * E[j];
      const unsigned long long seq = ++b.seq_no;
      launch_rk_error(N, e, b.D.p, rk_ynew.p, rk_K.p, ctl.atol, ctl.rtol, b.ctrl.p, b.red.p, b.hc_dev_at(seq), b.hseq_dev, seq, s);
      b.wait_ctrl(seq);
      const BdfCtrl* hc = b.hc;
      if (hc->nonfinite) {
        // SciPy would propagate the NaN; here a non-finite stage is treated like a failed step (halve)
        h_abs *= 0.5; rejected = true; ctl.st.n_rejected++;
        continue;
      }
      const double err = hc->err_norm;
      if (err < 1.0 && !(ban_negatives && hc->any_negative)) {
        double factor = err == 0.0 ? MAX_FACTOR : std::min(MAX_FACTOR, 0.9 * std::pow(err, -0.2));
        if (rejected) factor = std::min(1.0, factor);
        // accept: y_old <- D[0], D[0] <- y_new, K[0] <- K[6] (FSAL)
        b.copy(rk_yold.p, b.D.p);
        b.copy(b.D.p, rk_ynew.p);
        rk_h_last = hh;
        h_abs *= factor;
        t = t_new;
        ctl.st.n_steps++;
        return STEP_OK;
      }
      h_abs *= (ban_negatives && hc->any_negative && err < 1.0) ? 0.5 : std::max(MIN_FACTOR, 0.9 * std::pow(err, -0.2));
      rejected = true;
      ctl.st.n_rejected++;
    }
  }
  // the stage derivatives of the accepted step are needed for dense output until the next step starts:
  // the FSAL copy K[0] <- K[6] is therefore done lazily, at the start of the next step
  bool rk_fsal_pending = false;
  StepStatus rk_step_fsal(double t_bound) {
    if (rk_fsal_pending) {
      b.copy(rk_K.p, rk_K.p + (size_t)6 * b.N);
      rk_fsal_pending = false;
    }
    const StepStatus r = rk_step(t_bound);
    rk_fsal_pending = true;
    return r;
  }
  // SciPy's RkDenseOutput for RK45: y(t) = y_old + h x sum_j K_j (sum_p P[j][p] x^p), x = (t - t_old) / h
  void rk_interpolate(double ts, double* out) {
    static const double Pd[7][4] = {
        {1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
        {0, 0, 0, 0},
        {0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
        {0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
        {0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
        {0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
        {0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};
    const double x = (ts - (ctl.t - rk_h_last)) / rk_h_last;
    RkVec w;
    for (int j = 0; j < 7; j++) {
      double acc = 0.0, xp = x;
      for (int q = 0; q < 4; q++) { acc += Pd[j][q] * xp; xp *= x; }
      w.v[j] = rk_h_last * acc;
    }
    launch_rk_combine(b.N, 7, w, rk_yold.p, rk_K.p, out, b.s);
  }
};

// ------------------------------------------------------------------------------------------
// orchestration
// ------------------------------------------------------------------------------------------
namespace {

// Whatever way a call that drives the integrator ends (a throw included): no temperature stays pending on the handle (kin_rhs /
// kin_jac and the batched sweeps would otherwise see rate constants of different temperatures), and no speculative batch is
// left half-taken-up or held back; a kin_solve (`solve`) also takes its pointers out of the controller's parameters
struct CallGuard {
  kin_network* h; Solver& S; bool solve;
  ~CallGuard() {
    if (solve) S.forget_call();
    S.b.spec = HostBackend::Spec{};
    S.b.hold_speculation = false;
    if (h->k_pending) { try { h->flush_pending_T(h->stream); } catch (...) { h->k_pending = false; } }
  }
};

struct SaveBuf {
  kin_network* h;
  int N;
  int64_t cap = 0;
  void reserve(int64_t rows) {
    if (rows <= cap) return;
    int64_t ncap = std::max<int64_t>(rows, cap * 2);
    DevBuf<double> nb;
    nb.alloc((size_t)ncap * N);
    if (h->n_saved > 0)
      KIN_HIP(hipMemcpyAsync(nb.p, h->d_sol_u.p, (size_t)h->n_saved * N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    KIN_HIP(hipStreamSynchronize(h->stream));
    std::swap(h->d_sol_u.p, nb.p);
    std::swap(h->d_sol_u.n, nb.n);
    cap = ncap;
  }
  double* row(int64_t i) { return h->d_sol_u.p + (size_t)i * N; }
  void push_time(double t) { h->sol_t.push_back(t); h->n_saved++; }
};

// sets the handle's current rates for time-stop index si
void apply_rates(kin_network* h, const double* T_stops, bool have_table, int64_t si) {
  const int64_t R = h->host.R;
  if (have_table) {
    KIN_HIP(hipMemcpyAsync(h->k.p, h->table.p + (size_t)si * R, R * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  } else {
    launch_arrhenius(R, h->Ea.p, h->A.p, h->has_kmax, h->k_max, h->t_mult, T_stops[si], h->k.p, h->stream);
  }
  h->has_rates = true;
  h->k_pending = false;
}

// The host-driven integrator as the solve driver sees it (resident_core.hpp: res_drive): Solver integrates - the controller, or
// the explicit mode - and rows go to the handle's solution buffer, which grows, and their times to h->sol_t
struct HostDriven {
  static constexpr bool saves_every_step = true;   // no save grid (saveat = []): every accepted step is a row
  kin_network* h;
  Solver& S;
  const ResParams& P;
  const double* T_stops;
  bool have_table;
  std::chrono::steady_clock::time_point wall0;
  SaveBuf sb{h, (int)h->host.N};
  // KIN_PROGRESS=<seconds>: a status line on stderr at most that often (the reference's `progress` option drives a progress
  // bar from the same place, methods.jl:822-827); KIN_TRACE_CHUNK=n: HostBackend::trace during chunk n
  const double progress_every = getenv("KIN_PROGRESS") ? std::max(1.0, atof(getenv("KIN_PROGRESS"))) : 0.0;
  std::chrono::steady_clock::time_point progress_last = wall0;
  const long long trace_chunk = getenv("KIN_TRACE_CHUNK") ? atoll(getenv("KIN_TRACE_CHUNK")) : -1;

  void begin() {}   // (Solver::begin_call and the upload of u0: solve_entry, before the driver)
  double time() const { return S.ctl.t; }
  int64_t iters() const { return S.ctl.iters_left; }
  StepStatus step(double t_bound) { return S.step(t_bound); }
  void select_order() { S.select_order(); }
  void chunk_begin(int64_t nc) {
    S.b.trace = (nc == trace_chunk);
    if (progress_every > 0.0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - progress_last).count() >= progress_every) {
      progress_last = std::chrono::steady_clock::now();
      fprintf(stderr, "[kin_solve] chunk %lld / %lld, %.1f s, %lld steps, %lld factorisations, %lld restarts\n", (long long)nc,
              (long long)P.n_chunks, std::chrono::duration<double>(progress_last - wall0).count(), (long long)S.ctl.st.n_steps,
              (long long)S.ctl.st.n_factor, (long long)S.ctl.st.n_restarts);
      fflush(stderr);
    }
    S.ctl.chunk_begin(nc);
  }
  void attempt_begin(int64_t maxiters) { S.ctl.attempt_begin(maxiters); }
  void apply_rates(int64_t si) { kin::apply_rates(h, T_stops, have_table, si); }
  // row `row` (= h->n_saved) at global time tg joins the solution
  void new_row(int64_t row, double tg) { sb.reserve(row + 1); sb.push_time(tg); }
  void save_y(int64_t row, double tg) { new_row(row, tg); S.b.copy(S.b.row(row), S.b.y.p); }
  void save_interp(int64_t row, double tl, double tg) { new_row(row, tg); S.interpolate(tl, row); }
  void save_step(int64_t row, double tg) { new_row(row, tg); S.b.save_state(S.b.row(row)); }   // (rides in the pending accept)
  // (carrying the history across RATE UPDATES was built and measured in round 4 - 3 180 rejected steps and 4x the time on the
  // C4 prefix - and is gone, docs/DESIGN_HISTORY.md R4)
  bool segment_start(double origin, double seg_len, bool warm) { return S.segment_start(origin, seg_len, warm); }
  void segment_end(bool failed) {
    // a failed attempt leaves the accept of its last good step (and the copy of that state into the solution buffer, whose
    // time is already recorded) pending: it must not outlive the buffers it points into
    if (failed) S.b.flush_accept();
    else S.b.y_from_D0();
  }
  void attempt_failed(int64_t nc, int attempts, int retcode, double t_seg, double abstol, double reltol) {
    if (progress_every > 0.0 || getenv("KIN_TIMING"))
      fprintf(stderr, "[kin_solve] chunk %lld attempt %d failed with retcode %d at local t = %.6e (h = %.3e, order %d); tolerances %.1e / %.1e\n",
              (long long)nc, attempts, retcode, t_seg + S.ctl.t, S.ctl.h_abs, S.ctl.order, abstol, reltol);
  }
  void retry(double abstol, double reltol, int64_t rows) {
    S.ctl.retry(abstol, reltol, rows);   // (the chunk's start state, clipped: HostBackend::y_from_chunk_start_clipped)
    h->n_saved = rows;
    h->sol_t.resize((size_t)rows);
  }
};

}  // namespace

// the save grid of a chunkwise solve (params.jl:89-99); a call that saves nothing on a grid (kin_integrator_init) skips it
static void validate_save_grid(const kin_params& p) {
  const bool has_save = p.save_interval >= 0;
  if (has_save && p.save_interval > p.solve_chunkstep) throw KinError(ERR_INVALID_ARG, "Solution save interval must be less than chunkwise simulation step size");
  if (has_save && !(p.save_interval > 0)) throw KinError(ERR_INVALID_ARG, "save_interval must be positive");
}

void validate_solve(kin_network* h, const kin_params& p, const double* tstops, const double* T_stops, const double* k_table,
                    int64_t n_stops, const double* t_nodes, const double* T_nodes, int64_t n_nodes, bool need_handle_rates,
                    bool with_save_grid) {
  // ---- validation (ODESimulationParams constructor, params.jl:77-104)
  if (!(p.tspan0 < p.tspan1)) throw KinError(ERR_INVALID_ARG, "Invalid time span");
  if (!(p.abstol > 0) || !(p.reltol > 0)) throw KinError(ERR_INVALID_ARG, "tolerances must be positive");
  const bool chunks = p.solve_chunks != 0;
  if (chunks) {
    if (!(p.solve_chunkstep > 0)) throw KinError(ERR_INVALID_ARG, "solve_chunkstep must be positive");
    const double q = p.tspan1 / p.solve_chunkstep;   // Int(tspan[2] / solve_chunkstep) must be exact (params.jl:89-99)
    if (q != std::floor(q) || q < 1) throw KinError(ERR_INVALID_ARG, "Simulation timespan is not divisible by requested chunkwise simulation step size");
    if (with_save_grid) validate_save_grid(p);
  }
  const bool continuous = n_nodes > 0;
  if (continuous) {
    if (n_stops > 0) throw KinError(ERR_INVALID_ARG, "continuous and discrete rate updates are mutually exclusive");
    if (!t_nodes || !T_nodes || n_nodes < 2) throw KinError(ERR_INVALID_ARG, "need >= 2 (t, T) nodes");
    if (!h->has_arrhenius) throw KinError(ERR_STATE, "continuous rates need the Arrhenius parameters");
    for (int64_t i = 1; i < n_nodes; i++)
      if (!(t_nodes[i] >= t_nodes[i - 1])) throw KinError(ERR_INVALID_ARG, "t_nodes must be non-decreasing");
  }
  const bool variable = n_stops > 0;
  if (variable) {
    if (!tstops) throw KinError(ERR_INVALID_ARG, "tstops is null");
    if (!k_table && !T_stops) throw KinError(ERR_INVALID_ARG, "need k_table or T_stops with tstops");
    if (!k_table && !h->has_arrhenius) throw KinError(ERR_STATE, "T_stops given but Arrhenius parameters were never set");
    for (int64_t i = 1; i < n_stops; i++)
      if (!(tstops[i] > tstops[i - 1])) throw KinError(ERR_INVALID_ARG, "tstops must be strictly increasing");
  } else if (!continuous && need_handle_rates && !h->has_rates) {
    throw KinError(ERR_STATE, "rates were never set");
  }
}

int solve_entry(kin_network* h, const kin_params& p, const double* u0, const double* tstops, const double* T_stops,
                const double* k_table, int64_t n_stops, kin_stats* stats, const double* t_nodes, const double* T_nodes,
                int64_t n_nodes, bool explicit_solver) {
  auto wall0 = std::chrono::steady_clock::now();
  const int64_t N = h->host.N, R = h->host.R;
  validate_solve(h, p, tstops, T_stops, k_table, n_stops, t_nodes, T_nodes, n_nodes, true);
  const bool continuous = n_nodes > 0;
  const bool variable = n_stops > 0;
  // small networks: the whole solve in one launch, one workgroup owns the trajectory (resident.cpp)
  if (resident_eligible(h, p, continuous, explicit_solver)) {
    if (h->k_pending) h->flush_pending_T(h->stream);
    return resident_solve(h, p, u0, tstops, T_stops, k_table, n_stops, stats);
  }
  if (!h->solver) h->solver.reset(new Solver(h));
  Solver& S = *h->solver;
  hipStream_t s = h->stream;
  CallGuard exit_guard{h, S, true};
  // the save grid (resident_setup.hpp; none: every step is saved). save_hits_end true: the chunk end is the last local save point
  // (the usual case). false (save_interval does not divide the chunk): the final chunk's last output is the dense-output value at
  // its last local save point. (The reference then also restarts every chunk from integ.sol.u[end] = the state at that last
  // SAVED point while labelling it as the chunk end - a defect that is not copied: chunks always continue from the state at the
  // chunk end.)
  const bool has_grid = res_has_grid(p);
  const ResGrid grid = has_grid ? make_res_grid(p) : ResGrid{};
  S.begin_call(p, grid, explicit_solver);
  S.P.n_stops = (int32_t)n_stops;
  S.P.tstops = tstops;
  if (continuous) S.set_profile(t_nodes, T_nodes, n_nodes);
  const bool have_table = variable && k_table != nullptr;
  if (have_table) {
    h->table.upload(k_table, (size_t)n_stops * R, s);
    h->table_rows = n_stops;
  }

  // ---- output storage
  h->sol_t.clear();
  h->n_saved = 0;
  HostDriven drv{h, S, S.P, T_stops, have_table, wall0};
  drv.sb.reserve(has_grid ? grid.cap : 1024);

  // initial state
  S.b.y.upload(u0, N, s);
  const ResDriven out = res_drive(drv);
  S.b.flush_accept();
  h->flush_pending_T(s);     // a temperature no kernel has consumed yet: k is what the caller may read next
  KIN_HIP(hipStreamSynchronize(s));
  const kin_stats st = res_stats(S.result(out.retcode, out.abstol, out.reltol), S.b.lu, S.P.n_slots,
                                 std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count());
  if (getenv("KIN_TIMING")) {
    fprintf(stderr, "[kin_solve] wall %.4f s, of which blocked in step syncs %.4f s (the rest is host-side enqueue); "
            "step-end hand-overs that fell back to copy + sync: %lld (fast path %s)\n",
            st.wall_seconds, S.b.sync_wait_s, (long long)S.b.n_sync_fallbacks, S.b.fast_sync ? "on" : "off");
    fprintf(stderr, "[kin_solve] corrector iterations per converged attempt: 1:%lld 2:%lld 3:%lld 4:%lld\n", (long long)S.b.iter_hist[1],
            (long long)S.b.iter_hist[2], (long long)S.b.iter_hist[3], (long long)S.b.iter_hist[4]);
    fprintf(stderr, "[kin_solve] speculatively enqueued steps taken up: %lld of %lld steps, enqueued for nothing: %lld\n",
            (long long)S.b.n_spec, (long long)st.n_steps, (long long)S.b.n_spec_dead);
  }
  if (stats) *stats = st;
  return out.retcode;
}

// ------------------------------------------------------------------------------------------
// return_integrator=true (methods.jl:175-178, 242-246, 706-709): the initialised integrator is
// handed back instead of being solved; the caller advances it with step!(integ) / solve!(integ)
// and reads integ.t / integ.u. It spans what the reference's integrator spans: the whole tspan for
// solve_chunks=false, the first chunk [0, solve_chunkstep] otherwise; discrete rate updates
// (tstops inside that span) fire when the time reaches them, as the PresetTimeCallback /
// DiscreteCallback of solve_utils.jl:435-509 do.
// ------------------------------------------------------------------------------------------
struct IntegratorState {
  bool active = false, in_segment = false, have_table = false;
  double t_loc0 = 0, t_loc1 = 0, t_seg = 0;
  ResSegEnd seg{0.0, false};   // the current segment's end
  std::vector<double> tstops, T_stops;
  std::vector<double> t_nodes, T_nodes;   // continuous rate updates: T(t) = linear interpolation of these (global time)
  int64_t stop_i = 0;
  int retcode = KIN_RETCODE_SUCCESS;
};

void integrator_init(kin_network* h, const kin_params& p, const double* u0, const double* tstops, const double* T_stops,
                     const double* k_table, int64_t n_stops, const double* t_nodes, const double* T_nodes, int64_t n_nodes) {
  const int64_t N = h->host.N, R = h->host.R;
  validate_solve(h, p, tstops, T_stops, k_table, n_stops, t_nodes, T_nodes, n_nodes, true, false);
  const bool continuous = n_nodes > 0, chunks = p.solve_chunks != 0, variable = n_stops > 0;
  if (!h->solver) h->solver.reset(new Solver(h));
  if (!h->integ) h->integ.reset(new IntegratorState());
  Solver& S = *h->solver;
  IntegratorState& I = *h->integ;
  hipStream_t s = h->stream;
  S.begin_call(p, ResGrid{}, false);
  S.ctl.attempt_begin(p.maxiters);
  I = IntegratorState{};
  I.have_table = variable && k_table != nullptr;
  if (I.have_table) { h->table.upload(k_table, (size_t)n_stops * R, s); h->table_rows = n_stops; }
  if (variable) {
    I.tstops.assign(tstops, tstops + n_stops);
    if (T_stops) I.T_stops.assign(T_stops, T_stops + n_stops);
  }
  if (continuous) {
    I.t_nodes.assign(t_nodes, t_nodes + n_nodes);
    I.T_nodes.assign(T_nodes, T_nodes + n_nodes);
    S.set_profile(I.t_nodes.data(), I.T_nodes.data(), n_nodes);   // (the integrator's span starts at global time t_loc0)
  }
  I.t_loc0 = chunks ? 0.0 : p.tspan0;
  I.t_loc1 = chunks ? p.solve_chunkstep : p.tspan1;
  I.t_seg = I.t_loc0;
  S.b.y.upload(u0, N, s);
  // rates in force at the start (the driver's rules, resident_core.hpp)
  I.stop_i = res_stops_passed(I.tstops.data(), n_stops, 0, chunks ? 0.0 : p.tspan0);
  if (variable) apply_rates(h, I.T_stops.data(), I.have_table, res_rates_at_stop(I.stop_i));
  I.active = true;
  S.ctl.t = 0.0;
  KIN_HIP(hipStreamSynchronize(s));
}

// up to max_steps accepted steps (max_steps <= 0: to the end of the span); returns the number taken
int64_t integrator_step(kin_network* h, int64_t max_steps) {
  if (!h->integ || !h->integ->active) throw KinError(ERR_STATE, "no integrator: call kin_integrator_init first");
  Solver& S = *h->solver;
  IntegratorState& I = *h->integ;
  hipStream_t s = h->stream;
  int64_t taken = 0;
  CallGuard exit_guard{h, S, false};
  while (I.retcode == KIN_RETCODE_SUCCESS && I.t_seg < I.t_loc1 && (max_steps <= 0 || taken < max_steps)) {
    if (!I.in_segment) {
      I.seg = res_segment_end(I.tstops.data(), (int64_t)I.tstops.size(), I.stop_i, I.t_loc1, 0.0, I.t_loc1);   // (local = global time)
      if (!S.segment_start(I.t_seg, I.seg.end - I.t_seg, false)) { I.retcode = KIN_RETCODE_UNSTABLE; break; }
      I.in_segment = true;
    }
    const double seg_len = I.seg.end - I.t_seg;
    // the last step of this call gets no speculative batch behind it: other entry points on the handle (kin_set_rates,
    // kin_rates_at, kin_newton_solve) may run before the next call and must not find a half-run step
    S.b.hold_speculation = max_steps > 0 && taken + 1 >= max_steps;
    const StepStatus ss = S.step(seg_len);
    I.retcode = res_step_retcode(ss, S.ctl.iters_left);
    if (I.retcode != KIN_RETCODE_SUCCESS) { S.b.flush_accept(); break; }
    S.select_order();
    taken++;
    if (S.ctl.t >= seg_len) {   // segment finished: state = D[0]; switch the rates at a tstop
      S.b.y_from_D0();
      I.t_seg = I.seg.end;
      I.in_segment = false;
      S.ctl.t = 0.0;
      if (I.seg.at_stop) { apply_rates(h, I.T_stops.data(), I.have_table, I.stop_i); I.stop_i++; }
    }
  }
  h->flush_pending_T(s);
  KIN_HIP(hipStreamSynchronize(s));
  return taken;
}

void integrator_state(kin_network* h, double* t, double* u, int32_t* retcode, kin_stats* stats) {
  if (!h->integ || !h->integ->active) throw KinError(ERR_STATE, "no integrator: call kin_integrator_init first");
  Solver& S = *h->solver;
  IntegratorState& I = *h->integ;
  if (t) *t = I.in_segment ? I.t_seg + S.ctl.t : I.t_seg;
  if (u) {
    if (I.in_segment) S.b.flush_accept();
    (I.in_segment ? S.b.D : S.b.y).download(u, h->host.N, h->stream);   // D[0] = state after the last accepted step
    KIN_HIP(hipStreamSynchronize(h->stream));
  }
  if (retcode) *retcode = I.retcode;
  // the counters and the tolerances in force; the analysis' sizes, the cache size and the wall time are kin_solve's to report
  struct { int m = 0, ns = 0, nrounds = 0; int64_t nnzU = 0; } no_analysis;
  if (stats) *stats = res_stats(S.result(I.retcode, S.ctl.atol, S.ctl.rtol), no_analysis, 0, 0.0);
}

void solution_max(kin_network* h, double* out_umax) {
  if (h->n_saved <= 0) throw KinError(ERR_STATE, "no solution stored");
  // (the stored solution may come from the resident integrator: no Solver object then; the scratch vector is the handle's)
  h->du.alloc(h->host.N);
  launch_colmax((int)h->host.N, h->n_saved, h->d_sol_u.p, h->du.p, h->stream);
  h->du.download(out_umax, h->host.N, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
}

// scatter b into the permuted solve vector / gather x back (diagnostic path only)
void newton_solve(kin_network* h, double c, const double* u, const double* b, double* x) {
  if (!h->solver) h->solver.reset(new Solver(h));
  Solver& S = *h->solver;
  hipStream_t s = h->stream;
  const int N = S.b.N;
  S.b.begin_segment();
  S.b.y.upload(u, N, s);
  S.ctl.eval_jac();
  S.b.lu.factor(c, S.b.jv.p, 0, &S.b.ctrl.p->lu_bad, s);
  S.ctl.cur_slot = 0;
  std::vector<int32_t> yl(N), xl(N);
  S.b.lu.yloc.download(yl.data(), N, s);
  S.b.lu.xloc.download(xl.data(), N, s);
  std::vector<double> W(S.b.lu.w_size);
  KIN_HIP(hipStreamSynchronize(s));
  std::vector<double> stage(N);
  // the solve vectors live at the tail of W: write b there element by element
  std::vector<double> tail((size_t)(S.b.lu.off_x + S.b.lu.mpad + 8 - S.b.lu.off_y), 0.0);   // the solve vectors only
  for (int i = 0; i < N; i++) tail[yl[i] - S.b.lu.off_y] = b[i];
  KIN_HIP(hipMemcpyAsync(S.b.lu.slots[0].W.p + S.b.lu.off_y, tail.data(), tail.size() * sizeof(double), hipMemcpyHostToDevice, s));
  S.b.lu.solve(nullptr, 0, s);
  KIN_HIP(hipMemcpyAsync(tail.data(), S.b.lu.slots[0].W.p + S.b.lu.off_y, tail.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  int bad = 0;
  KIN_HIP(hipMemcpyAsync(&bad, &S.b.ctrl.p->lu_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  KIN_HIP(hipStreamSynchronize(s));
  S.reset_cache();
  if (bad) {
    KIN_HIP(hipMemsetAsync(&S.b.ctrl.p->lu_bad, 0, sizeof(int), s));
    KIN_HIP(hipStreamSynchronize(s));
    throw KinError(ERR_SOLVE_FAILED, "vanishing pivot in the factorisation of I - c J (static diagonal pivoting)");
  }
  for (int i = 0; i < N; i++) x[i] = tail[xl[i] - S.b.lu.off_y];
}

// Diagnostic counterpart of resident_probe for the host-driven path: K Newton-matrix solves through the solver's own analysis
// and the product kernels, each member factorised into a slot of its own with a flag word of its own. batched == 0: every member
// through factor_into (launch_gauss_jordan), as kin_solve does; batched == 1: the sparse part per member, then ONE
// launch_gauss_jordan_batched chain over the dense blocks of up to GJ_BMAX members, as the lockstep ensemble's server does.
void newton_probe(kin_network* h, int64_t K, int32_t batched, const double* u, const double* c, const double* b, double* x,
                  int32_t* bad, int64_t* info) {
  if (!h->solver) h->solver.reset(new Solver(h));
  Solver& S = *h->solver;
  SparseLU& lu = S.b.lu;
  hipStream_t s = h->stream;
  const int N = S.b.N;
  S.b.begin_segment();
  const int G = (int)std::min<int64_t>(K, GJ_BMAX);
  lu.ensure_slots(G, s);
  DevBuf<int> d_bad;                        // one flag word per member
  d_bad.alloc((size_t)K);
  d_bad.zero(s);
  DevBuf<double> gpinv;                     // pivot scratch of a batched chain (2 x 32 x 32 doubles per matrix)
  if (batched) gpinv.alloc((size_t)GJ_BMAX * 2 * 32 * 32);
  std::vector<int32_t> yl(N), xl(N);
  lu.yloc.download(yl.data(), N, s);
  lu.xloc.download(xl.data(), N, s);
  KIN_HIP(hipStreamSynchronize(s));
  const size_t tail_n = (size_t)(lu.off_x + lu.mpad + 8 - lu.off_y);   // the solve vectors only
  std::vector<double> tails((size_t)G * tail_n);
  for (int64_t g0 = 0; g0 < K; g0 += G) {
    const int n = (int)std::min<int64_t>(G, K - g0);
    double* Sp[GJ_BMAX]; double* S2p[GJ_BMAX]; int* badp[GJ_BMAX];
    for (int i = 0; i < n; i++) {
      const int64_t t = g0 + i;
      SparseLU::Slot& q = lu.slots[i];
      S.b.y.upload(u + t * N, N, s);
      S.ctl.eval_jac();
      if (batched) lu.factor_sparse_into(c[t], S.b.jv.p, q, d_bad.p + t, s);
      else lu.factor_into(c[t], S.b.jv.p, q, lu.pinv.p, d_bad.p + t, s);
      Sp[i] = q.W.p + lu.off_S; S2p[i] = q.S2.p; badp[i] = d_bad.p + t;
    }
    if (batched && lu.m > 0) {
      const int where = launch_gauss_jordan_batched(n, Sp, S2p, lu.mpad, gpinv.p, badp, s);
      for (int i = 0; i < n; i++) lu.slots[i].sinv = where ? S2p[i] : Sp[i];
    }
    std::fill(tails.begin(), tails.end(), 0.0);
    for (int i = 0; i < n; i++) {
      double* tail = tails.data() + (size_t)i * tail_n;
      for (int v = 0; v < N; v++) tail[yl[v] - lu.off_y] = b[(g0 + i) * N + v];
      KIN_HIP(hipMemcpyAsync(lu.slots[i].W.p + lu.off_y, tail, tail_n * sizeof(double), hipMemcpyHostToDevice, s));
      lu.solve(nullptr, i, s);
      KIN_HIP(hipMemcpyAsync(tail, lu.slots[i].W.p + lu.off_y, tail_n * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    KIN_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++)
      for (int v = 0; v < N; v++) x[(g0 + i) * N + v] = tails[(size_t)i * tail_n + (xl[v] - lu.off_y)];
  }
  std::vector<int> hb((size_t)K);
  d_bad.download(hb.data(), (size_t)K, s);
  d_bad.zero(s);
  KIN_HIP(hipStreamSynchronize(s));
  for (int64_t t = 0; t < K; t++) bad[t] = hb[t] ? 1 : 0;
  S.ctl.cur_slot = 0;
  S.reset_cache();
  info[0] = lu.ns; info[1] = lu.m; info[2] = lu.mpad; info[3] = lu.nrounds;
  info[4] = lu.fused_tri ? 0 : lu.explicit_tri ? 1 : 2;
  // whole-workgroup rows and the longest row over every gather plan of the analysis, read back from the plans on the device
  int64_t long_rows = 0, max_row = 0;
  auto scan = [&](const SegPlanDev& p) {
    std::vector<int32_t> off((size_t)p.G + 1), sb((size_t)p.S), se((size_t)p.S), bb((size_t)p.B), be((size_t)p.B);
    if (p.G > 0) p.grp_off.download(off.data(), off.size(), s);
    p.seg_beg.download(sb.data(), sb.size(), s); p.seg_end.download(se.data(), se.size(), s);
    p.blk_beg.download(bb.data(), bb.size(), s); p.blk_end.download(be.data(), be.size(), s);
    KIN_HIP(hipStreamSynchronize(s));
    for (int g = 0; g < p.G; g++) max_row = std::max<int64_t>(max_row, off[g + 1] - off[g]);
    for (int q = 0; q < p.S; q++) max_row = std::max<int64_t>(max_row, se[q] - sb[q]);
    for (int q = 0; q < p.B; q++) max_row = std::max<int64_t>(max_row, be[q] - bb[q]);
    long_rows += p.B;
  };
  for (const auto* v : {&lu.schur, &lu.fwd, &lu.bwd}) for (const SegPlanDev& p : *v) scan(p);
  for (const SegPlanDev* p : {&lu.fwd_dense, &lu.fwdZ, &lu.bwdT, &lu.bwdV, &lu.lz_build, &lu.nvu_build, &lu.stageA, &lu.stageC}) scan(*p);
  info[5] = lu.mpad / 32; info[6] = long_rows; info[7] = max_row;
  for (int32_t j = 0; j < lu.m; j++) info[8 + j] = lu.perm[lu.ns + j];
}

// Path 1 of kin_step_probe: the corrector update inside the solve's last gather launch, on the caller's step state
void step_probe_fused(kin_network* h, double c, const double* u, const double* b, NewtonFuse& f, double* x, int64_t* info) {
  if (!h->solver) h->solver.reset(new Solver(h));
  Solver& S = *h->solver;
  SparseLU& lu = S.b.lu;
  if (!(lu.fused_tri && lu.m > 0)) throw KinError(ERR_UNSUPPORTED, "the analysis of this network has no fused solve with a dense block");
  hipStream_t s = h->stream;
  const int N = S.b.N;
  S.b.begin_segment();
  lu.ensure_slots(1, s);
  S.b.y.upload(u, N, s);
  S.ctl.eval_jac();
  lu.factor(c, S.b.jv.p, 0, &f.ctrl->lu_bad, s);   // (the flag of a vanished pivot goes where the integrator puts it)
  std::vector<int32_t> yl(N), xl(N);
  lu.yloc.download(yl.data(), N, s);
  lu.xloc.download(xl.data(), N, s);
  KIN_HIP(hipStreamSynchronize(s));
  std::vector<double> tail((size_t)(lu.off_x + lu.mpad + 8 - lu.off_y), 0.0);   // the solve vectors only
  for (int i = 0; i < N; i++) tail[yl[i] - lu.off_y] = b[i];
  KIN_HIP(hipMemcpyAsync(lu.slots[0].W.p + lu.off_y, tail.data(), tail.size() * sizeof(double), hipMemcpyHostToDevice, s));
  f.N = N; f.skip = &f.ctrl->newton_done; f.part = S.b.red.p;
  lu.solve_newton(0, f, s);
  KIN_HIP(hipMemcpyAsync(tail.data(), lu.slots[0].W.p + lu.off_y, tail.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  const SegPlanDev& p = lu.stageC;
  std::vector<int32_t> off((size_t)p.G + 1), sb((size_t)p.S), se((size_t)p.S), bb((size_t)p.B), be((size_t)p.B);
  if (p.G > 0) p.grp_off.download(off.data(), off.size(), s);
  p.seg_beg.download(sb.data(), sb.size(), s); p.seg_end.download(se.data(), se.size(), s);
  p.blk_beg.download(bb.data(), bb.size(), s); p.blk_end.download(be.data(), be.size(), s);
  KIN_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < N; i++) x[i] = tail[xl[i] - lu.off_y];
  int64_t max_row = 0, s_long = 0;
  for (int g = 0; g < p.G; g++) max_row = std::max<int64_t>(max_row, off[g + 1] - off[g]);
  for (int q = 0; q < p.S; q++) { max_row = std::max<int64_t>(max_row, se[q] - sb[q]); if (se[q] - sb[q] > 256) s_long++; }
  for (int q = 0; q < p.B; q++) max_row = std::max<int64_t>(max_row, be[q] - bb[q]);
  info[0] = p.G; info[1] = p.S; info[2] = s_long; info[3] = p.B; info[4] = max_row; info[5] = lu.m;
  info[6] = lu.newton_grid(); info[7] = stagec_newton_wg(p.view());
  S.ctl.cur_slot = 0;
  S.reset_cache();
}

// kin_eval_probe, path 0: the residual pair as newton_iteration launches it, on the caller's y, psi, d and flag value
EvalResidPlan eval_probe_solver_plan(kin_network* h) {
  if (!h->solver) h->solver.reset(new Solver(h));
  Solver& S = *h->solver;
  return EvalResidPlan{&S.b.resid_plan, S.b.lu.yloc.p, S.b.lu.off_y, S.b.lu.off_vec_end - S.b.lu.off_y};
}
void eval_probe_solver_resid(kin_network* h, const double* u, double c, const double* psi, const double* d, int done, double sentinel,
                             double* vec, double* rate) {
  const EvalResidPlan pl = eval_probe_solver_plan(h);
  Solver& S = *h->solver;
  SparseLU& lu = S.b.lu;
  hipStream_t s = h->stream;
  const int N = S.b.N;
  const int64_t R = h->host.R;
  S.b.begin_segment();
  lu.ensure_slots(1, s);
  double* W = lu.slots[0].W.p;
  // what the probe overwrites and a solve expects as it left it: the solve vectors of slot 0 and the control block
  std::vector<double> keep((size_t)pl.vec_len), fill((size_t)std::max<int64_t>(pl.vec_len, R), sentinel);
  BdfCtrl keep_ctrl, c_in{};
  KIN_HIP(hipMemcpyAsync(keep.data(), W + pl.off_y, keep.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  KIN_HIP(hipMemcpyAsync(&keep_ctrl, S.b.ctrl.p, sizeof(BdfCtrl), hipMemcpyDeviceToHost, s));
  KIN_HIP(hipStreamSynchronize(s));
  c_in.newton_done = done;
  KIN_HIP(hipMemcpyAsync(S.b.ctrl.p, &c_in, sizeof(BdfCtrl), hipMemcpyHostToDevice, s));
  KIN_HIP(hipMemcpyAsync(W + pl.off_y, fill.data(), (size_t)pl.vec_len * sizeof(double), hipMemcpyHostToDevice, s));
  if (R > 0) KIN_HIP(hipMemcpyAsync(h->rate.p, fill.data(), (size_t)R * sizeof(double), hipMemcpyHostToDevice, s));
  S.b.y.upload(u, N, s); S.b.psi.upload(psi, N, s); S.b.d.upload(d, N, s);
  S.b.launch_residual(c, &S.b.ctrl.p->newton_done, W);
  KIN_HIP(hipGetLastError());
  KIN_HIP(hipMemcpyAsync(vec, W + pl.off_y, (size_t)pl.vec_len * sizeof(double), hipMemcpyDeviceToHost, s));
  if (R > 0) h->rate.download(rate, (size_t)R, s);
  KIN_HIP(hipMemcpyAsync(W + pl.off_y, keep.data(), keep.size() * sizeof(double), hipMemcpyHostToDevice, s));
  KIN_HIP(hipMemcpyAsync(S.b.ctrl.p, &keep_ctrl, sizeof(BdfCtrl), hipMemcpyHostToDevice, s));
  KIN_HIP(hipStreamSynchronize(s));
  S.ctl.cur_slot = 0;
  S.reset_cache();
}

}  // namespace kin

kin_network::kin_network() {}
kin_network::~kin_network() {
  for (kin_network* r : replicas) delete r;
  replicas.clear();
  integ.reset();
  solver.reset();
  if (stream) (void)hipStreamDestroy(stream);
}
