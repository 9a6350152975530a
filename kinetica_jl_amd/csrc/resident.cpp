// Host-side owner of the resident integrator (resident.hip / resident_core.hpp): symbolic analysis, table upload,
// per-trajectory workspaces, ONE launch per solve (or per ensemble of solves) and the read-back of its result block.
// Takes the networks whose trajectory fits one workgroup (up to a few thousand species): at those sizes the host-driven
// integrator of solver.cpp spends its time in launch calls and dependency gaps (~75 us per step whatever N is), which is
// the regime of the reference's documented CRNs (docs/src/getting-started.md:43-70) and of BASELINE configs[0..1].
#include "resident.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>

#include "handle.hpp"
#include "lu.hpp"
#include "resident_setup.hpp"
#include "solver.hpp"

namespace kin {

struct ResidentSolver {
  kin_network* h;
  SparseLU lu;
  SegPlanDev resid_plan;
  DevBuf<int32_t> d_jdiag, d_round_dummy;
  ResNetDev hn{};
  DevBuf<ResNetDev> d_net;
  bool ok = false;
  std::string why;
  size_t dyn_lds = 0;
  // workspaces (grown on demand)
  int K_cap = 0, n_slots = 0;
  size_t per_traj = 0;
  DevBuf<double> work, Wbuf, jdbuf, gjbuf, d_u0, d_sol, d_solt, d_save, d_tstops, d_Tstops, d_tnodes, d_Tnodes;
  DevBuf<ResTrajDev> d_traj;
  DevBuf<ResResult> d_res;
  DevBuf<ResParams> d_par;
  std::vector<ResTrajDev> h_traj;

  explicit ResidentSolver(kin_network* hh) : h(hh) {
    const NetworkHost& H = h->host;
    hipStream_t s = h->stream;
    LUOptions opt;
    opt.min_round = 2;   // a round costs two barriers here, not two dependent launches
    opt.max_rounds = std::min(opt.max_rounds, RES_MAX_ROUNDS);
    lu.analyze((int32_t)H.N, H.j_ptr, H.j_col, opt, s);
    if (lu.m > RES_MAX_DENSE) { why = "dense Schur block beyond the resident integrator's limit"; return; }
    if (lu.nrounds > RES_MAX_ROUNDS) { why = "too many elimination rounds"; return; }
    dyn_lds = resident_dyn_lds((int)H.N, (int)H.R, lu.m, lu.off_vec_end - lu.off_y);
    if (dyn_lds > RES_LDS_BUDGET) { why = "state, rates and solve vectors do not fit one compute unit's LDS"; return; }
    std::vector<int32_t> yl(H.N), ident(H.N);
    lu.yloc.download(yl.data(), H.N, s);
    KIN_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < H.N; i++) ident[i] = (int32_t)i;
    resid_plan.upload(build_seg_plan(H.N, H.sp_ptr.data(), yl.data(), H.sp_rxn.data(), nullptr, H.sp_coef.data(), false, ident.data()), s);
    d_jdiag.upload(H.j_diag, s);
    hn.N = (int32_t)H.N; hn.R = (int32_t)H.R; hn.nnzJ = (int32_t)H.nnz();
    hn.ns = lu.ns; hn.m = lu.m; hn.mpad = lu.mpad; hn.nrounds = lu.nrounds; hn.n_mono_ent = lu.n_mono_ent;
    hn.solve_mode = lu.fused_tri ? RES_SOLVE_FUSED : (lu.explicit_tri ? RES_SOLVE_EXPLICIT : RES_SOLVE_PLAIN);
    hn.off_diag = lu.off_diag; hn.off_U = lu.off_U; hn.off_L = lu.off_L; hn.off_S = lu.off_S; hn.off_y = lu.off_y; hn.off_x = lu.off_x;
    hn.off_dinv = lu.off_dinv; hn.off_vec_end = lu.off_vec_end; hn.w_size = lu.w_size;
    hn.x0 = h->x0.p; hn.x1 = h->x1.p; hn.jmap = lu.jmap.p; hn.ent_pivot = lu.ent_pivot.p; hn.yloc = lu.yloc.p; hn.xloc = lu.xloc.p;
    hn.j_diag = d_jdiag.p;
    hn.mono_ent_ptr = lu.mono_ent_ptr.p; hn.mono_ptr = lu.mono_ptr.p; hn.mono_fac = lu.mono_fac.p; hn.mono_dst = lu.mono_dst.p;
    hn.mono_sign = lu.mono_sign.p;
    for (int r = 0; r <= lu.nrounds; r++) hn.round_e0[r] = lu.ent_ptr[lu.round_ptr[r]];
    hn.rhs_plan = h->rhs_plan.view(); hn.jac_plan = h->jac_plan.view(); hn.resid_plan = resid_plan.view();
    hn.lz_build = lu.lz_build.view(); hn.nvu_build = lu.nvu_build.view(); hn.stageA = lu.stageA.view(); hn.stageC = lu.stageC.view();
    // LDS for the task descriptors of the corrector's three gather plans, where it is to be had: not beyond the kernel's budget,
    // and not at the price of the second workgroup per compute unit an ensemble would get without them
    {
      const size_t desc = resident_desc_bytes(hn.resid_plan, hn.stageA, hn.stageC);
      const size_t static_lds = resident_static_lds();
      const bool two_before = 2 * (dyn_lds + static_lds) <= (size_t)160 * 1024, two_after = 2 * (dyn_lds + desc + static_lds) <= (size_t)160 * 1024;
      hn.desc_in_lds = (lu.fused_tri && dyn_lds + desc <= RES_LDS_BUDGET && (two_after || !two_before)) ? 1 : 0;
      if (hn.desc_in_lds) dyn_lds += desc;
    }
    hn.fwdZ = lu.fwdZ.view(); hn.fwd_dense = lu.fwd_dense.view(); hn.bwdT = lu.bwdT.view(); hn.bwdV = lu.bwdV.view();
    for (int r = 0; r < lu.nrounds; r++) { hn.schur[r] = lu.schur[r].view(); hn.fwd[r] = lu.fwd[r].view(); hn.bwd[r] = lu.bwd[r].view(); }
    // the multi-workgroup factorisation's slot (SparseLU::analyze allocates one) is not used by this path
    lu.slots.clear();
    ok = true;
  }

  size_t slot_bytes() const { return ((size_t)lu.w_size + (size_t)h->host.N) * sizeof(double); }

  // (re)allocates the workspaces of K trajectories with `slots` LU-cache slots each
  void ensure(int K, int slots, int64_t sol_rows, bool own_sol) {
    const NetworkHost& H = h->host;
    hipStream_t s = h->stream;
    auto al = [](size_t x) { return (x + 7) / 8 * 8; };
    const size_t N = (size_t)H.N, R = (size_t)H.R;
    per_traj = al(R) + al((size_t)RES_D_ROWS * N) + 8 * al(N) + al((size_t)H.nnz()) + al(R) + al(2 * R + 2);
    if (K > K_cap || slots != n_slots) {
      work.alloc((size_t)K * per_traj);
      Wbuf.alloc((size_t)K * slots * (size_t)lu.w_size);
      jdbuf.alloc((size_t)K * slots * N);
      gjbuf.alloc((size_t)K * std::max<size_t>(1, (size_t)lu.mpad * lu.mpad));
      KIN_HIP(hipMemsetAsync(gjbuf.p, 0, (size_t)K * std::max<size_t>(1, (size_t)lu.mpad * lu.mpad) * sizeof(double), s));
      // padding entries of the value-ordered stages and the `zero` operand are never written by a factorisation
      KIN_HIP(hipMemsetAsync(Wbuf.p, 0, (size_t)K * slots * (size_t)lu.w_size * sizeof(double), s));
      d_traj.alloc(K); d_res.alloc(K); d_u0.alloc((size_t)K * N);
      K_cap = K; n_slots = slots;
    }
    d_solt.alloc((size_t)K * (size_t)sol_rows);
    if (own_sol) {
      d_sol.alloc((size_t)K * (size_t)sol_rows * N);
      // rows beyond a member's n_saved (a member that failed early) read as zeros in out_u
      KIN_HIP(hipMemsetAsync(d_sol.p, 0, (size_t)K * (size_t)sol_rows * N * sizeof(double), s));
    }
    h_traj.assign(K, ResTrajDev{});
    for (int t = 0; t < K; t++) {
      ResTrajDev& q = h_traj[t];
      double* w = work.p + (size_t)t * per_traj;
      q.u0 = d_u0.p + (size_t)t * N;
      q.k = w; w += al(R);
      q.D = w; w += al((size_t)RES_D_ROWS * N);
      q.y = w; w += al(N); q.psi = w; w += al(N); q.d = w; w += al(N); q.scale = w; w += al(N);
      q.f0 = w; w += al(N); q.f1 = w; w += al(N); q.ytmp = w; w += al(N); q.chunk_start = w; w += al(N);
      q.jv = w; w += al((size_t)H.nnz());
      q.rate = w; w += al(R);
      q.dr = w;
      q.gj_scratch = gjbuf.p + (size_t)t * (size_t)lu.mpad * lu.mpad;
      q.W = Wbuf.p + (size_t)t * slots * (size_t)lu.w_size;
      q.jd = jdbuf.p + (size_t)t * slots * N;
      q.sol = own_sol ? d_sol.p + (size_t)t * (size_t)sol_rows * N : nullptr;
      q.sol_t = d_solt.p + (size_t)t * (size_t)sol_rows;
      q.result = d_res.p + t;
      q.Ea = h->Ea.p; q.A = h->A.p;   // (run_resident points a per-member call's members at their own rows)
    }
  }
};

void ResidentDeleter::operator()(ResidentSolver* p) const { delete p; }

namespace {

int resident_max_n() {
  static const int v = getenv("KIN_RESIDENT_MAX_N") ? atoi(getenv("KIN_RESIDENT_MAX_N")) : 400;   // (plus RES_MAX_DENSE on the Schur block)
  return v;
}

// ... and on the dense Schur block of the Newton matrix: the in-workgroup dense inverse and GEMV grow with m^3 / m^2 while the
// host-driven path's costs are flat; at the crossover network size of the synthetic CRNs (400 species) m is 130
int resident_max_dense_single() {
  static const int v = getenv("KIN_RESIDENT_MAX_DENSE") ? atoi(getenv("KIN_RESIDENT_MAX_DENSE")) : 160;
  return v;
}

ResidentSolver* get_resident(kin_network* h) {
  if (!h->resident) h->resident.reset(new ResidentSolver(h));
  return h->resident.get();
}

// common part: parameters, the members' stops, tables of the variable conditions, launch, results. `c`: the call whose
// member_stops every member reads (resident_solve: a call of its one member); a continuous call (rate_mode 3) has every member's
// profile in its ResTrajDev already
void run_resident(kin_network* h, ResidentSolver& RS, const EnsembleCall& c, const ResGrid& g, int K, int slots, std::vector<ResResult>& res) {
  hipStream_t s = h->stream;
  const int64_t R = h->host.R;
  ResParams P{};
  res_fill_params(P, c.p, g);
  res_default_settings(P, slots);
  P.profile = getenv("KIN_RESIDENT_PROFILE") ? 1 : 0;
  RS.d_save.upload(g.save_local, s);
  P.save_local = RS.d_save.p;
  const bool stops = !c.static_rates() && !c.continuous();
  P.rate_mode = c.continuous() ? 3 : (stops ? (c.k_table ? 1 : 2) : 0);
  if (stops) {
    // one upload of every member's stops - the concatenated arrays of a per-member call, the shared ones else - and each member
    // pointed at its own (the kernel's prologue copies them into its ResParams: P.tstops / P.n_stops stay unset here)
    const EnsembleCall::Stops s0 = c.member_stops(0);
    const size_t n_all = c.stop_ptr ? (size_t)(c.stop_ptr[K] - c.stop_ptr[0]) : (size_t)c.n_stops;
    RS.d_tstops.upload(s0.tstops, n_all, s);
    if (c.k_table) { h->table.upload(c.k_table, (size_t)c.n_stops * R, s); h->table_rows = c.n_stops; RS.hn.k_table = h->table.p; }
    else RS.d_Tstops.upload(s0.T_stops, n_all, s);
    for (int t = 0; t < K; t++) {
      const EnsembleCall::Stops ms = c.member_stops(t);
      RS.h_traj[t].tstops = RS.d_tstops.p + (ms.tstops - s0.tstops);
      RS.h_traj[t].T_stops = c.k_table ? nullptr : RS.d_Tstops.p + (ms.T_stops - s0.T_stops);
      RS.h_traj[t].n_stops = ms.n;
    }
  }
  // each member's Arrhenius parameters: its rows of a per-member call's blocks, the handle's arrays for a shared call
  for (int t = 0; t < K; t++) {
    const EnsembleCall::Arrhenius pm = c.member_arrhenius(h, t);
    RS.h_traj[t].Ea = pm.Ea; RS.h_traj[t].A = pm.A;
  }
  RS.hn.Ea = h->Ea.p; RS.hn.A = h->A.p; RS.hn.has_kmax = h->has_kmax ? 1 : 0; RS.hn.k_max = h->k_max; RS.hn.t_mult = h->t_mult;
  RS.d_net.upload(&RS.hn, 1, s);
  RS.d_par.upload(&P, 1, s);
  RS.d_traj.upload(RS.h_traj.data(), (size_t)K, s);
  // more members than compute units, and two workgroups fit one compute unit's LDS: the build with half the registers per lane
  // (two co-resident workgroups hide each other's latencies: +20-40 % solves/s at 300 species; a member alone is 10-15 % slower)
  static const size_t static_lds = resident_static_lds();
  bool shared_cu = K > h->n_cu && 2 * (RS.dyn_lds + static_lds) <= (size_t)160 * 1024;
  if (const char* e = getenv("KIN_RESIDENT_SHARED_CU")) shared_cu = atoi(e) != 0 && 2 * (RS.dyn_lds + static_lds) <= (size_t)160 * 1024;
  if (shared_cu) launch_resident_shared_cu(K, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, s);
  else launch_resident(K, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, s);
  res.resize(K);
  RS.d_res.download(res.data(), (size_t)K, s);
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

bool resident_eligible(kin_network* h, const kin_params& p, bool continuous, bool explicit_solver) {
  if (const char* e = getenv("KIN_RESIDENT")) { if (atoi(e) == 0) return false; }
  if (continuous || explicit_solver) return false;
  if (h->host.N > resident_max_n()) return false;
  if (!res_has_grid(p)) return false;
  if (getenv("KIN_TRACE_CHUNK") || getenv("KIN_INJECT_BAD_PIVOT")) return false;
  ResidentSolver* RS = get_resident(h);
  return RS->ok && RS->lu.m <= resident_max_dense_single();
}

// the dynamic LDS is at least 8 (4 N + R) bytes whatever the factorisation looks like (resident_dyn_lds): a network beyond that
// never fits, and is told so WITHOUT the symbolic analysis a ResidentSolver starts with (0.2-1.4 s and a second set of LU plans
// on a 10k-50k species handle)
static bool resident_can_fit(const kin_network* h) {
  return (size_t)(4 * h->host.N + h->host.R) * sizeof(double) <= RES_LDS_BUDGET;
}

bool resident_fits(kin_network* h) { return resident_can_fit(h) && get_resident(h)->ok; }

// Does an ensemble of K members take the one-launch form? Not beyond the kernel's limits, and not FEW members of a network at the
// upper end of what the kernel takes: one workgroup per member lasts as long as its slowest member's resident solve, which from
// ~700 species on is slower than the member's own kin_solve on the host-driven path (table DESIGN 0 "resident vs host-driven"),
// so up to 32 members of such a network are faster as kin_solve calls on host threads / lockstep rounds
// (profiles/r04_ensemble_route_crossover.jsonl: 1 000 species, 16 members 0.5 s against 0.34-1.1 s; from 64 members on the launch
// is 3-4x ahead, at <= 700 species at every K).
bool resident_ensemble_route(kin_network* h, int64_t K) {
  if (!resident_can_fit(h)) return false;
  if (h->host.N > 700 && K < 32) return false;
  return get_resident(h)->ok;
}

int resident_solve(kin_network* h, const kin_params& p, const double* u0, const double* tstops, const double* T_stops,
                   const double* k_table, int64_t n_stops, kin_stats* stats) {
  auto wall0 = std::chrono::steady_clock::now();
  ResidentSolver& RS = *get_resident(h);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, R = h->host.R;
  const ResGrid g = make_res_grid(p);
  const int slots = res_lu_slots(RS.slot_bytes(), 1);
  // the solution goes straight into the handle's buffer (kin_solution_copy / _max / _dot read it there)
  h->d_sol_u.alloc((size_t)g.cap * N);
  RS.ensure(1, slots, g.cap, false);
  RS.h_traj[0].sol = h->d_sol_u.p;
  RS.d_u0.upload(u0, (size_t)N, s);
  if (n_stops == 0) KIN_HIP(hipMemcpyAsync(RS.h_traj[0].k, h->k.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
  EnsembleCall c{};
  c.p = p; c.K = 1; c.u0 = u0; c.tstops = tstops; c.T_stops = T_stops; c.k_table = k_table; c.n_stops = n_stops;
  std::vector<ResResult> res;
  run_resident(h, RS, c, g, 1, slots, res);
  const ResResult& r = res[0];
  h->n_saved = std::min<int64_t>(r.n_saved, g.cap);
  h->sol_t.resize((size_t)h->n_saved);
  if (h->n_saved > 0) RS.d_solt.download(h->sol_t.data(), (size_t)h->n_saved, s);
  // the rates in force at the end of the solve are what the handle holds afterwards, as on the host-driven path
  if (n_stops > 0) { KIN_HIP(hipMemcpyAsync(h->k.p, RS.h_traj[0].k, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s)); h->has_rates = true; h->k_pending = false; }
  KIN_HIP(hipStreamSynchronize(s));
  if (stats) *stats = res_stats(r, RS.lu, slots, std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count());
  if (getenv("KIN_RESIDENT_PROFILE")) {
    static const char* names[20] = {"kernel", "factor", "(of which dense inverse)", "corrector attempts", "(solve)", "predict", "change_D",
                                    "accept", "jacobian", "rhs", "(rates + residual)", "(update + sums)", "((rates))", "((stage A))", "((gemv))",
                                    "((stage C))", "((reduce))", "(((reduce: lane sums)))", "(((reduce: first barrier)))", "controller between phases (a worker wavefront waiting for its next command)"};
    fprintf(stderr, "[resident] N=%lld m=%d slots=%d steps=%lld factor=%lld linsolve=%lld wall %.4f s\n", (long long)N, RS.lu.m, slots,
            (long long)r.st.n_steps, (long long)r.st.n_factor, (long long)r.st.n_linsolve,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count());
    for (int i = 0; i < 20; i++) fprintf(stderr, "[resident]   %-26s %9.3f ms\n", names[i], (double)r.prof[i] * 1e-5);
  }
  return r.retcode;
}

void stage_member_rates(kin_network* h, const EnsembleCall& c, int64_t m, const double* Ea, const double* A, double* d_k, hipStream_t s) {
  const int64_t R = h->host.R;
  if (c.k) KIN_HIP(hipMemcpyAsync(d_k, c.k + m * R, (size_t)R * sizeof(double), hipMemcpyHostToDevice, s));
  else if (c.T) launch_arrhenius(R, Ea, A, h->has_kmax, h->k_max, h->t_mult, c.T[m], d_k, s);
  else KIN_HIP(hipMemcpyAsync(d_k, h->k.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
}

// K independent trajectories of one network in ONE launch (one workgroup each); a continuous call's member profiles and a
// per-member-stops call's schedules are uploaded once
void resident_ensemble(kin_network* h, const EnsembleCall& c) {
  auto wall0 = std::chrono::steady_clock::now();
  ResidentSolver& RS = *get_resident(h);
  if (!RS.ok) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: " + RS.why);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, K = c.K;
  const ResGrid g = make_res_grid(c.p);
  if (c.n_rows) *c.n_rows = g.cap;
  const int slots = res_lu_slots(RS.slot_bytes(), K);
  RS.ensure((int)K, slots, g.cap, true);
  RS.d_u0.upload(c.u0, (size_t)K * N, s);
  if (c.continuous()) {
    const int64_t* ptr = c.node_ptr;
    const size_t n_all = (size_t)(ptr[K] - ptr[0]);
    RS.d_tnodes.upload(c.t_nodes + ptr[0], n_all, s);
    RS.d_Tnodes.upload(c.T_nodes + ptr[0], n_all, s);
    for (int64_t t = 0; t < K; t++) {
      RS.h_traj[t].t_nodes = RS.d_tnodes.p + (ptr[t] - ptr[0]);
      RS.h_traj[t].T_nodes = RS.d_Tnodes.p + (ptr[t] - ptr[0]);
      RS.h_traj[t].n_nodes = ptr[t + 1] - ptr[t];
    }
  } else if (c.static_rates()) {
    for (int64_t t = 0; t < K; t++) stage_member_rates(h, c, t, h->Ea.p, h->A.p, RS.h_traj[t].k, s);
  }
  std::vector<ResResult> res;
  run_resident(h, RS, c, g, (int)K, slots, res);
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
  if (c.out_u) RS.d_sol.download(c.out_u, (size_t)K * (size_t)g.cap * N, s);
  std::vector<MemberResult> out((size_t)K);
  for (int64_t t = 0; t < K; t++) out[(size_t)t] = res_member_result(res[(size_t)t], RS.lu, slots, wall);
  finish_ensemble(h, c, g.cap, out, RS.d_sol.p, nullptr, RS.d_solt.p);   // (kin_ensemble_*: the members' states stay where they are)
}

// Diagnostic: the kernel's own phases once per member on given inputs (resident_probe.hip), with the handle's current rates and
// the ResidentSolver every resident solve of this handle uses (analysis, plans, descriptors-in-LDS decision, LDS size)
void resident_probe(kin_network* h, int64_t K, const double* u, const double* c, const double* b, double* du, double* jac, double* x,
                    int32_t* bad, int64_t* info) {
  if (!resident_can_fit(h)) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: its state and rates exceed the LDS");
  ResidentSolver& RS = *get_resident(h);
  if (!RS.ok) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: " + RS.why);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, R = h->host.R, nnz = h->host.nnz();
  RS.ensure((int)K, 1, 1, false);
  RS.d_u0.upload(u, (size_t)K * N, s);
  DevBuf<double> d_c, d_b, d_x, d_du, d_jac;
  DevBuf<int32_t> d_bad;
  d_c.upload(c, (size_t)K, s);
  d_b.upload(b, (size_t)K * N, s);
  d_x.alloc((size_t)K * N); d_du.alloc((size_t)K * N); d_jac.alloc((size_t)K * std::max<int64_t>(nnz, 1)); d_bad.alloc((size_t)K);
  for (int64_t t = 0; t < K; t++) {
    ResTrajDev& q = RS.h_traj[t];
    KIN_HIP(hipMemcpyAsync(q.k, h->k.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
    q.f0 = d_du.p + t * N;
    q.jv = d_jac.p + t * nnz;
  }
  ResParams P{};
  P.n_slots = 1;
  RS.hn.Ea = h->Ea.p; RS.hn.A = h->A.p; RS.hn.has_kmax = h->has_kmax ? 1 : 0; RS.hn.k_max = h->k_max; RS.hn.t_mult = h->t_mult;
  RS.d_net.upload(&RS.hn, 1, s);
  RS.d_par.upload(&P, 1, s);
  RS.d_traj.upload(RS.h_traj.data(), (size_t)K, s);
  launch_resident_probe((int)K, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, ResProbeIO{d_c.p, d_b.p, d_x.p, d_bad.p}, s);
  d_du.download(du, (size_t)K * N, s);
  d_jac.download(jac, (size_t)K * nnz, s);
  d_x.download(x, (size_t)K * N, s);
  d_bad.download(bad, (size_t)K, s);
  KIN_HIP(hipStreamSynchronize(s));
  info[0] = RS.lu.m; info[1] = RS.lu.ns; info[2] = RS.lu.nrounds; info[3] = RS.hn.solve_mode; info[4] = RS.hn.desc_in_lds;
  info[5] = (int64_t)RS.dyn_lds; info[6] = RS.lu.mpad; info[7] = 0;
  for (int32_t j = 0; j < RS.lu.m; j++) info[8 + j] = RS.lu.perm[RS.lu.ns + j];
}

// Diagnostic (kin_cache_probe, path 1): the LU cache's drift guard or its slot rules through the kernel's own phases and backend
// (resident_probe.hip, modes RES_PROBE_DRIFT / RES_PROBE_RULES), in the workspaces of the ResidentSolver every resident solve of
// this handle uses, sized for n_slots slots. Sizes were checked by the caller; the kernel indexes with the handle's tables only.
void resident_cache_probe(kin_network* h, int mode, int64_t n_slots, const double* jv_slots, const double* c_fact, const int32_t* valid,
                          const double* jv_now, double max_drift, const int64_t* stamps, int64_t n_queries, const double* qd, const int64_t* qi,
                          double* jd, double* drift, int32_t* out_i, int64_t* info) {
  if (!resident_can_fit(h)) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: its state and rates exceed the LDS");
  ResidentSolver& RS = *get_resident(h);
  if (!RS.ok) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: " + RS.why);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, nnz = h->host.nnz();
  const bool drift_mode = mode == RES_PROBE_DRIFT;
  const int slots = drift_mode ? (int)n_slots : 1;
  RS.ensure(1, slots, 1, false);
  DevBuf<double> d_jvs, d_now, d_c, d_qd, d_drift;
  DevBuf<int32_t> d_valid, d_out;
  DevBuf<long long> d_stamps, d_qi;
  ResProbeIO io{};
  io.mode = mode; io.n_slots = (int32_t)n_slots; io.n_queries = (int32_t)n_queries; io.max_drift = max_drift;
  const size_t n_out = drift_mode ? (size_t)RES_MAX_SLOTS + 1 : (size_t)2 * n_queries;
  std::vector<int32_t> h_out(n_out, -2);
  d_out.upload(h_out, s);
  d_c.upload(c_fact, (size_t)n_slots, s); d_valid.upload(valid, (size_t)n_slots, s);
  io.c_fact = d_c.p; io.valid = d_valid.p; io.out_i = d_out.p;
  if (drift_mode) {
    d_jvs.upload(jv_slots, (size_t)(n_slots * nnz), s); d_now.upload(jv_now, (size_t)nnz, s);
    d_drift.alloc((size_t)RES_MAX_SLOTS);
    io.jv_slots = d_jvs.p; io.jv_now = d_now.p; io.drift = d_drift.p;
  } else {
    static_assert(sizeof(long long) == sizeof(int64_t), "stamps travel as they are");
    d_stamps.upload(reinterpret_cast<const long long*>(stamps), (size_t)(3 * n_slots), s);
    d_qd.upload(qd, (size_t)(2 * n_queries), s); d_qi.upload(reinterpret_cast<const long long*>(qi), (size_t)(5 * n_queries), s);
    io.stamps = d_stamps.p; io.qd = d_qd.p; io.qi = d_qi.p;
  }
  ResParams P{};
  P.n_slots = slots;
  RS.hn.Ea = h->Ea.p; RS.hn.A = h->A.p; RS.hn.has_kmax = h->has_kmax ? 1 : 0; RS.hn.k_max = h->k_max; RS.hn.t_mult = h->t_mult;
  RS.d_net.upload(&RS.hn, 1, s);
  RS.d_par.upload(&P, 1, s);
  RS.d_traj.upload(RS.h_traj.data(), 1, s);
  launch_resident_probe(1, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, io, s);
  d_out.download(h_out.data(), n_out, s);
  if (drift_mode) {
    RS.jdbuf.download(jd, (size_t)(n_slots * N), s);
    d_drift.download(drift, (size_t)n_slots, s);
  }
  KIN_HIP(hipStreamSynchronize(s));
  std::fill(info, info + 8, (int64_t)0);
  if (drift_mode) {
    std::copy(h_out.begin(), h_out.begin() + n_slots, out_i);
    info[0] = h_out[RES_MAX_SLOTS]; info[1] = n_slots; info[2] = info[0];
  } else {
    std::copy(h_out.begin(), h_out.end(), out_i);
  }
  info[3] = RS.lu.m; info[4] = RS.lu.ns; info[5] = (int64_t)RS.dyn_lds;
}

// Diagnostic (kin_step_probe, paths 3 and 4): one operation of the step per member through the kernel's own dispatch
// (resident_probe.hip / resident_probe_w4.hip, mode RES_PROBE_STEP), in the workspaces of the ResidentSolver every resident solve
// of this handle uses. Each member's ResTrajDev points into its block of the caller's state: D at rows 0-7, f0 / f1 / ytmp /
// chunk_start at rows 12-15, the two solution rows at 24-25, u0 at row 26; the times of the two solution rows travel in ctrl's
// scratch0 / scratch1 for the operations that write them (VEC's save_y and set_time, INTERP). Arguments were checked by the caller.
void resident_step_probe(kin_network* h, int waves_per_eu, int op, int64_t K, const ResStepArg* args, double* state, double* ctrl,
                         int64_t* info) {
  if (!resident_can_fit(h)) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: its state and rates exceed the LDS");
  ResidentSolver& RS = *get_resident(h);
  if (!RS.ok) throw KinError(ERR_UNSUPPORTED, "network does not fit the resident integrator: " + RS.why);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, R = h->host.R;
  const size_t per = (size_t)RES_STEP_ROWS * N;
  const bool times = op == RES_STEP_SAVE_Y || op == RES_STEP_SET_TIME || op == RES_STEP_INTERP;
  RS.ensure((int)K, 1, 2, false);
  DevBuf<double> d_state, d_ctrl;
  DevBuf<ResStepArg> d_args;
  DevBuf<int32_t> d_shape;
  std::vector<int32_t> h_shape((size_t)3 * K, 0);
  d_shape.upload(h_shape, s);
  d_state.upload(state, (size_t)K * per, s);
  d_ctrl.upload(ctrl, (size_t)K * RES_STEP_CTRL, s);
  d_args.upload(args, (size_t)K, s);
  std::vector<double> solt((size_t)2 * K);
  for (int64_t t = 0; t < K; t++) { solt[2 * t] = ctrl[t * RES_STEP_CTRL + 6]; solt[2 * t + 1] = ctrl[t * RES_STEP_CTRL + 7]; }
  RS.d_solt.upload(solt.data(), solt.size(), s);
  for (int64_t t = 0; t < K; t++) {
    ResTrajDev& q = RS.h_traj[t];
    double* blk = d_state.p + (size_t)t * per;
    if (h->has_rates) KIN_HIP(hipMemcpyAsync(q.k, h->k.p, (size_t)R * sizeof(double), hipMemcpyDeviceToDevice, s));
    q.D = blk;
    q.f0 = blk + 12 * N; q.f1 = blk + 13 * N; q.ytmp = blk + 14 * N; q.chunk_start = blk + 15 * N;
    q.sol = blk + 24 * N;
    q.u0 = blk + 26 * N;
  }
  ResParams P{};
  P.n_slots = 1;
  RS.hn.Ea = h->Ea.p; RS.hn.A = h->A.p; RS.hn.has_kmax = h->has_kmax ? 1 : 0; RS.hn.k_max = h->k_max; RS.hn.t_mult = h->t_mult;
  RS.d_net.upload(&RS.hn, 1, s);
  RS.d_par.upload(&P, 1, s);
  RS.d_traj.upload(RS.h_traj.data(), (size_t)K, s);
  ResProbeIO io{};
  io.mode = RES_PROBE_STEP; io.step_op = op; io.step_arg = d_args.p; io.state = d_state.p; io.ctrl = d_ctrl.p; io.out_i = d_shape.p;
  if (waves_per_eu == 4) launch_resident_probe_shared_cu((int)K, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, io, s);
  else launch_resident_probe((int)K, RS.dyn_lds, RS.d_net.p, RS.d_traj.p, RS.d_par.p, io, s);
  d_state.download(state, (size_t)K * per, s);
  d_ctrl.download(ctrl, (size_t)K * RES_STEP_CTRL, s);
  RS.d_solt.download(solt.data(), solt.size(), s);
  d_shape.download(h_shape.data(), h_shape.size(), s);
  KIN_HIP(hipStreamSynchronize(s));
  if (times)
    for (int64_t t = 0; t < K; t++) { ctrl[t * RES_STEP_CTRL + 6] = solt[2 * t]; ctrl[t * RES_STEP_CTRL + 7] = solt[2 * t + 1]; }
  // N, trips and owning wavefronts as the kernel counted them (every member must report the same: -1 otherwise)
  for (int q = 0; q < 3; q++) {
    info[q] = h_shape[q];
    for (int64_t t = 1; t < K; t++) if (h_shape[3 * t + q] != h_shape[q]) info[q] = -1;
  }
  info[3] = RS.lu.m; info[4] = RS.hn.solve_mode;
  info[5] = RS.hn.desc_in_lds; info[6] = (int64_t)RS.dyn_lds; info[7] = waves_per_eu;
}

}  // namespace kin
