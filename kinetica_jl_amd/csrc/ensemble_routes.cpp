// The ensemble call layer under kin_solve_ensemble*: the validated entries, the per-member parameter upload, the routing between
// the resident launch (resident.cpp), the lockstep rounds (ensemble.cpp) and kin_solve calls on host threads (replica_ensemble,
// here), and the finishing layer every route hands its results to.
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "handle.hpp"
#include "solver.hpp"

namespace kin {

void upload_solve_tables(kin_network* h) {
  const NetworkHost& N = h->host;
  hipStream_t s = h->stream;
  h->x0.upload(N.x0, s); h->x1.upload(N.x1, s);
  h->sp_ptr.upload(N.sp_ptr, s); h->sp_rxn.upload(N.sp_rxn, s); h->sp_coef.upload(N.sp_coef, s);
  h->rhs_plan.upload(build_seg_plan(N.N, N.sp_ptr.data(), nullptr, N.sp_rxn.data(), nullptr, N.sp_coef.data(), false), s);
  h->jac_plan.upload(build_seg_plan(N.nnz(), N.jc_ptr.data(), nullptr, N.jc_src.data(), nullptr, N.jc_coef.data(), false), s);
  h->k.alloc(N.R); h->rate.alloc(N.R); h->dr.alloc(2 * N.R + 2);
  h->u.alloc(N.N); h->du.alloc(N.N); h->jvals.alloc(N.nnz());
}

void finish_ensemble(kin_network* h, const EnsembleCall& c, int64_t cap, const std::vector<MemberResult>& res, const double* sol,
                     const std::vector<double>* host_times, const double* dev_times) {
  EnsembleRows f = finish_members(c, cap, res.data(), host_times);
  const int64_t n = f.n_saved[(size_t)f.best];
  if (c.out_t && !host_times && n > 0)
    KIN_HIP(hipMemcpyAsync(c.out_t, dev_times + (size_t)f.best * (size_t)cap, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KIN_HIP(hipStreamSynchronize(h->stream));   // (the route's own downloads on this stream as well)
  h->set_ensemble_record(sol, c.K, cap, std::move(f.n_saved));
}

namespace {

// A solve-only copy of a handle: the solve tables again on the device, own stream and work vectors; Solver, symbolic LU and LU
// cache are built by its first solve and stay with it
kin_network* clone_for_solves(kin_network* h) {
  std::unique_ptr<kin_network> c(new kin_network());
  c->host = h->host;
  c->device = h->device; c->n_cu = h->n_cu;
  KIN_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  upload_solve_tables(c.get());
  KIN_HIP(hipStreamSynchronize(c->stream));
  return c.release();
}

int replica_threads_max() {
  const char* e = getenv("KIN_ENSEMBLE_THREADS");   // (read per call: tests change it)
  return std::max(1, e ? atoi(e) : 12);
}

// A SMALL ensemble of a LARGE network: K independent kin_solve calls on K host threads, one solve-only copy of the handle each.
// Every member is, bit for bit, what kin_solve gives for its inputs. A chain of ~14 small dependent launches per step keeps one
// trajectory at 6.7 solves/s (first 2 chunks of the 10k-species network) and K of them at 11 / 17 / 17 / 16 for K = 2 / 4 / 8 / 12 - the
// dispatch rate of the chip's queues; the lockstep rounds of ensemble.cpp only overtake that from K = 16 on.
// A continuous call's member m is the kin_solve_continuous of its own profile, a per-member-stops call's the kin_solve of its
// own (tstops, T_stops).
void replica_ensemble(kin_network* h, const EnsembleCall& c) {
  const int64_t N = h->host.N, R = h->host.R, K = c.K;
  const int64_t cap = make_res_grid(c.p).cap;
  if (c.n_rows) *c.n_rows = cap;
  // EMPIRICAL (ROCm 7.2, MI355X; tools/replica_sequence.py): members whose streams are among the first ~4 streams of the
  // process slow each other down when they run together - K = 4: 11.4 solves/s, with three or more streams created BEFORE theirs
  // (and kept alive; destroyed ones do not count) 17.0; K = 8: 13.3 -> 16.7; K = 12: 13.9 -> 16.3. Which thread creates a
  // stream makes no difference. bench.py's concurrent_replicas never saw it: torch's own streams play that role there. Four
  // idle placeholder streams are therefore created once per process in front of the first replica's.
  {
    static std::once_flag once;
    std::call_once(once, [] {
      const int n = getenv("KIN_REPLICA_PLACEHOLDER_STREAMS") ? atoi(getenv("KIN_REPLICA_PLACEHOLDER_STREAMS")) : 4;
      for (int i = 0; i < n; i++) { hipStream_t d = nullptr; if (hipStreamCreateWithFlags(&d, hipStreamNonBlocking) != hipSuccess) (void)hipGetLastError(); }
    });
  }
  // a thread solves its members one after the other on its own replica
  const ThreadShare share = replica_thread_share(K, replica_threads_max());
  while ((int64_t)h->replicas.size() < share.threads) {
    // LU-cache budget of a replica: its share of 70 % of what the device has FREE now, as if every thread of the limit were to get
    // a replica (a later call with more members then finds the same share left for the replicas it adds; the budget is fixed when a
    // replica's Solver is built, at its first solve)
    size_t free_b = 0, total_b = 0;
    KIN_HIP(hipMemGetInfo(&free_b, &total_b));
    h->replicas.push_back(clone_for_solves(h));
    h->replicas.back()->lu_budget_mb = std::max<size_t>(64, (size_t)((double)free_b * 0.7 / (1024.0 * 1024.0)) / (size_t)replica_threads_max());
  }
  // kin_ensemble_*: every member's saved rows are copied device-to-device into the handle's own [K][cap][N], zeros past n_saved
  h->ens_sol.alloc((size_t)K * (size_t)cap * (size_t)N);
  KIN_HIP(hipStreamSynchronize(h->stream));
  std::vector<MemberResult> res((size_t)K);
  std::vector<std::vector<double>> times((size_t)K);    // every member's save times (out_t: those of the furthest)
  run_member_threads(share.threads, [&](int64_t t) {
    kin_network* rep = h->replicas[(size_t)t];
    KIN_HIP(hipSetDevice(rep->device));
    hipStream_t s = rep->stream;
    if (h->has_arrhenius) {
      rep->Ea.alloc(R); rep->A.alloc(R);
      KIN_HIP(hipMemcpyAsync(rep->Ea.p, h->Ea.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
      KIN_HIP(hipMemcpyAsync(rep->A.p, h->A.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
      rep->has_arrhenius = true; rep->has_kmax = h->has_kmax; rep->k_max = h->k_max; rep->t_mult = h->t_mult;
    }
    for (int64_t m = t; m < K; m += share.threads) {
      if (c.member_params()) {
        // the member's own (Ea, A) into the replica's arrays, which the next call's copy of the handle's overwrites again;
        // the handle's own are never written
        const EnsembleCall::Arrhenius pm = c.member_arrhenius(h, m);
        KIN_HIP(hipMemcpyAsync(rep->Ea.p, pm.Ea, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
        KIN_HIP(hipMemcpyAsync(rep->A.p, pm.A, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
      }
      if (c.static_rates()) {
        stage_member_rates(h, c, m, rep->Ea.p, rep->A.p, rep->k.p, s);
        rep->has_rates = true; rep->k_pending = false;
      }
      KIN_HIP(hipStreamSynchronize(s));
      MemberResult& r = res[(size_t)m];
      const int64_t* ptr = c.node_ptr;
      const EnsembleCall::Stops ms = c.member_stops(m);
      r.retcode = ptr ? solve_entry(rep, c.p, c.u0 + m * N, nullptr, nullptr, nullptr, 0, &r.stats, c.t_nodes + ptr[m], c.T_nodes + ptr[m],
                                    ptr[m + 1] - ptr[m])
                      : solve_entry(rep, c.p, c.u0 + m * N, ms.tstops, ms.T_stops, c.k_table, ms.n, &r.stats);
      r.n_saved = rep->n_saved;
      const int64_t ns = std::min<int64_t>(rep->n_saved, cap);
      if (c.out_u && ns > 0) rep->d_sol_u.download(c.out_u + (size_t)m * cap * N, (size_t)ns * N, s);
      if (c.out_u && ns < cap) std::memset(c.out_u + ((size_t)m * cap + (size_t)ns) * N, 0, (size_t)(cap - ns) * N * sizeof(double));   // rows a failed member never wrote
      // (on the replica's stream, before its next member overwrites d_sol_u; drained by the synchronisation below)
      double* keep = h->ens_sol.p + (size_t)m * (size_t)cap * (size_t)N;
      if (ns > 0) KIN_HIP(hipMemcpyAsync(keep, rep->d_sol_u.p, (size_t)ns * N * sizeof(double), hipMemcpyDeviceToDevice, s));
      if (ns < cap) KIN_HIP(hipMemsetAsync(keep + (size_t)ns * N, 0, (size_t)(cap - ns) * N * sizeof(double), s));
      KIN_HIP(hipStreamSynchronize(s));
      if (c.out_t) times[(size_t)m] = rep->sol_t;
    }
  }, [](int64_t) {});   // (a thread that never started leaves nothing behind: the call fails as a whole)
  finish_ensemble(h, c, cap, res, h->ens_sol.p, times.data());
}

// Which form an ensemble call takes. Networks whose trajectory fits one compute unit: one workgroup per member, one launch
// (resident.cpp); larger ones: kin_solve calls on host threads (replica_ensemble) or lockstep rounds of batched launches
// (ensemble.cpp). KIN_ENSEMBLE_ROUTE = threads | lockstep forces a form (A/B runs: tools/ensemble_route_crossover.py);
// KIN_ENSEMBLE_BATCHED=1 forces the lockstep form of a static call. The lockstep form has no continuous rate updates.
void route_ensemble(kin_network* h, const EnsembleCall& c) {
  const char* e = getenv("KIN_ENSEMBLE_ROUTE");
  const std::string route = e ? e : "";
  const bool force_batched = getenv("KIN_ENSEMBLE_BATCHED") && atoi(getenv("KIN_ENSEMBLE_BATCHED")) != 0;
  if (route == "threads") return replica_ensemble(h, c);
  if (c.continuous()) {
    require(route != "lockstep", ERR_UNSUPPORTED, "the lockstep ensemble has no continuous rate updates");
    return resident_ensemble_route(h, c.K) ? resident_ensemble(h, c) : replica_ensemble(h, c);
  }
  if (route == "lockstep" || force_batched) return batched_ensemble(h, c);
  if (resident_ensemble_route(h, c.K)) return resident_ensemble(h, c);
  // few members of a network too large for a compute unit: kin_solve calls on host threads, one member per thread up to the
  // thread limit (beyond it the lockstep rounds are ahead at 3 000 and 10 000 species: profiles/r04_ensemble_route_crossover.jsonl)
  // ... and ANY number of members when the lockstep form does not take the network's factorisation (it needs the fused solve
  // with a dense Schur block; KIN_LU_FUSED=0 or a network without hubs has none): the threads then take several members each
  if (c.K <= replica_threads_max() || !ensemble_batched_supported(h, nullptr)) return replica_ensemble(h, c);
  batched_ensemble(h, c);
}

// A call with per-member Arrhenius parameters has its Ea[K][R], A[K][R] uploaded once, here, into the buffers that stay with the
// ensemble record (16 K R bytes; reused by later calls); every route reads them through EnsembleCall::member_arrhenius, and
// kin_ensemble_flux reads them from the record. A shared call takes the route as it is and leaves a shared record.
void run_ensemble(kin_network* h, const EnsembleCall& c) {
  h->ens.clear();   // (whatever route: its buffers are about to be reallocated or overwritten; set again by a call that succeeds)
  if (!c.member_params()) return route_ensemble(h, c);
  const size_t n = (size_t)c.K * (size_t)h->host.R;
  try {
    h->ens_Ea.alloc(n); h->ens_A.alloc(n);
  } catch (const std::exception& e) {
    (void)hipGetLastError();
    throw KinError(ERR_DEVICE, "ensemble: no device memory for the per-member Arrhenius parameters (" + std::to_string(2 * n * sizeof(double)) +
                                   " bytes): " + e.what());
  }
  KIN_HIP(hipMemcpyAsync(h->ens_Ea.p, c.Ea, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KIN_HIP(hipMemcpyAsync(h->ens_A.p, c.A, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KIN_HIP(hipStreamSynchronize(h->stream));   // (the thread route's replicas read the blocks on streams of their own)
  EnsembleCall m = c;
  m.d_Ea = h->ens_Ea.p; m.d_A = h->ens_A.p;
  route_ensemble(h, m);
  if (h->ens.valid()) { h->ens.Ea = h->ens_Ea.p; h->ens.A = h->ens_A.p; }
}

}  // namespace

int ensemble_entry(kin_network* h, const kin_params* params, EnsembleCall c, const std::function<void()>& checks,
                   const std::function<void()>& validate) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && c.u0 && c.K >= 1, ERR_INVALID_ARG, "params / u0 is null, or K < 1");
  checks();
  require(res_has_grid(*params), ERR_INVALID_ARG, "an ensemble solve needs a save grid (solve_chunks or save_interval)");
  validate();
  if (c.n_rows && !c.out_u && !c.n_saved) { *c.n_rows = make_res_grid(*params).cap; }   // size query
  else {
    // (kin_solve_ensemble's members may start from the handle's own k: a temperature still pending is formed first)
    if (!c.stop_ptr && !c.node_ptr && h->k_pending) h->flush_pending_T(h->stream);
    c.p = *params;
    run_ensemble(h, c);
  }
  KIN_CATCH(h)
}

int ensemble_member_entry(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* Ea, const double* A,
                          bool nodes, const int64_t* ptr, const double* t, const double* T, int64_t* n_rows, double* out_t,
                          double* out_u, int64_t* n_saved, int32_t* retcodes, kin_stats* stats) {
  EnsembleCall c{kin_params{}, K, u0, nullptr, nullptr, nodes ? nullptr : t, nodes ? nullptr : T, nullptr, 0, nodes ? nullptr : ptr,
                 nodes ? ptr : nullptr, nodes ? t : nullptr, nodes ? T : nullptr, n_rows, out_t, out_u, n_saved, retcodes, stats};
  c.Ea = Ea; c.A = A;
  return ensemble_entry(h, params, c, [&] {
    require(ptr && t && T, ERR_INVALID_ARG, nodes ? "node_ptr / t_nodes / T_nodes is null" : "stop_ptr / tstops / T_stops is null");
    require((Ea == nullptr) == (A == nullptr), ERR_INVALID_ARG, "give both per-member Ea and A, or neither");
  }, [&] {
    for (int64_t m = 0; m < K; m++) {
      // every member needs a profile / a stop of its own: an empty profile would leave the controller's T(t) nothing to read, and
      // the rates in force before the first stop are those of stop 0
      const int64_t n = ptr[m + 1] - ptr[m];
      require(ptr[m] >= 0 && n >= (nodes ? 2 : 1), ERR_INVALID_ARG, nodes ? "need >= 2 (t, T) nodes per member" : "need >= 1 stop per member");
      if (nodes) validate_solve(h, *params, nullptr, nullptr, nullptr, 0, t + ptr[m], T + ptr[m], n, false);
      else validate_solve(h, *params, t + ptr[m], T + ptr[m], nullptr, n, nullptr, nullptr, 0, false);
    }
  });
}

}  // namespace kin
