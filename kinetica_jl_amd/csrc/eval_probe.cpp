// kin_eval_probe (declaration and argument layout: include/kinetica_hip.h): the right-hand side, the Jacobian values or the
// Newton residual once, on the caller's states, through the launchers the integrators use - kin_network::rhs_dev / jac_dev and
// HostBackend::launch_residual (path 0), ens_rhs / ens_jac / ens_resid of the lockstep ensemble (path 2). Nothing here computes: the
// probe uploads, fills the launchers' arguments the way HostBackend / EnsembleSolver fill them, launches, downloads.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "ensemble.hpp"
#include "handle.hpp"
#include "solver.hpp"

using namespace kin;

namespace {

// G, S, B, the longest row and the rows of the ELL groups, read back from the plan on the device; the workgroup size the
// launchers take for it (segsum_wg: what launch_segsum / launch_e_segsum branch on)
void plan_info(const SegPlanDev& p, hipStream_t s, int64_t* info) {
  std::vector<int32_t> off((size_t)p.G + 1), dst((size_t)p.G * 64), sb((size_t)p.S), se((size_t)p.S), bb((size_t)p.B), be((size_t)p.B);
  if (p.G > 0) { p.grp_off.download(off.data(), off.size(), s); p.grp_dst.download(dst.data(), dst.size(), s); }
  p.seg_beg.download(sb.data(), sb.size(), s); p.seg_end.download(se.data(), se.size(), s);
  p.blk_beg.download(bb.data(), bb.size(), s); p.blk_end.download(be.data(), be.size(), s);
  KIN_HIP(hipStreamSynchronize(s));
  int64_t max_row = 0, n_short = 0;
  for (int g = 0; g < p.G; g++) max_row = std::max<int64_t>(max_row, off[g + 1] - off[g]);
  for (int q = 0; q < p.S; q++) max_row = std::max<int64_t>(max_row, se[q] - sb[q]);
  for (int q = 0; q < p.B; q++) max_row = std::max<int64_t>(max_row, be[q] - bb[q]);
  for (int32_t v : dst) n_short += v >= 0;
  info[0] = p.G; info[1] = p.S; info[2] = p.B; info[3] = max_row; info[4] = n_short; info[5] = segsum_wg(p.view());
}

struct Args {
  int path, op, mode;
  int64_t K, ne;
  const int32_t* members;
  const double *u, *k;
  double T;
  const double *c, *psi, *d;
  const int32_t* done;
  double sentinel;
  double* out; int64_t out_len;
  double* rate; int32_t* yloc; int64_t* info;
};

void eval_probe(kin_network* h, const Args& a) {
  const int64_t N = h->host.N, R = h->host.R, nnz = h->host.nnz();
  hipStream_t s = h->stream;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::fill(a.info, a.info + 8, (int64_t)0);
  a.info[7] = nnz;
  const bool resid = a.op == KIN_EVAL_RESID || a.op == KIN_EVAL_SIZES;
  EvalResidPlan pl{nullptr, nullptr, 0, 0};
  if (resid) {
    pl = a.path == 0 ? eval_probe_solver_plan(h) : eval_probe_ensemble_plan(h);
    a.info[6] = pl.vec_len;
  }
  const SegPlanDev& plan = resid ? *pl.plan : a.op == KIN_EVAL_JAC ? h->jac_plan : h->rhs_plan;
  plan_info(plan, s, a.info);
  if (a.op == KIN_EVAL_SIZES) return;

  // ---- what the kernels index with is checked here: they trust their launchers
  const int64_t need = a.op == KIN_EVAL_JAC ? nnz : a.op == KIN_EVAL_RESID ? pl.vec_len : (a.path == 2 ? 2 * N : N);
  require(a.out_len >= need, ERR_CAPACITY, "out_len is smaller than the operation's output (info[6], info[7]: kin_eval_probe with KIN_EVAL_SIZES)");
  std::vector<char> seen((size_t)a.K, 0);
  for (int64_t e = 0; e < a.ne; e++) {
    require(a.members[e] >= 0 && a.members[e] < a.K && !seen[a.members[e]], ERR_INVALID_ARG, "entry names no member, or one member twice");
    seen[a.members[e]] = 1;
  }
  std::vector<int32_t> yl;
  if (a.op == KIN_EVAL_RESID) {
    require(a.c && a.psi && a.d && a.done && a.rate && a.yloc, ERR_INVALID_ARG, "the residual takes c, psi, d, done and returns rate and yloc");
    yl.resize((size_t)N);
    KIN_HIP(hipMemcpyAsync(yl.data(), pl.yloc, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    KIN_HIP(hipStreamSynchronize(s));
    std::vector<char> hit((size_t)pl.vec_len, 0);
    for (int64_t i = 0; i < N; i++) {
      const int64_t q = (int64_t)yl[i] - pl.off_y;
      require(q >= 0 && q < pl.vec_len && !hit[q], ERR_DEVICE, "yloc leaves the solve vectors or names a position twice");
      hit[q] = 1;
    }
    for (int64_t i = 0; i < N; i++) a.yloc[i] = (int32_t)(yl[i] - pl.off_y);   // positions inside the returned window
  }

  if (a.path == 0) {
    require(!a.k, ERR_INVALID_ARG, "path 0 evaluates with the handle's rate constants: k must be null");
    // (every refusal comes before the temperature is made pending: a refused call leaves the handle as it was)
    if (a.T > 0.0) require(h->has_arrhenius, ERR_STATE, "a temperature needs Arrhenius parameters (kin_set_arrhenius)");
    else require(h->has_rates, ERR_STATE, "rates were never set");
    if (a.T > 0.0) h->set_pending_T(a.T);
    if (a.op == KIN_EVAL_RESID) {
      eval_probe_solver_resid(h, a.u, a.c[0], a.psi, a.d, a.done[0], a.sentinel, a.out, a.rate);
      return;
    }
    DevBuf<double> d_u, d_out;
    d_u.upload(a.u, (size_t)N, s);
    std::vector<double> fill((size_t)std::max<int64_t>(need, 1), nan);
    d_out.upload(fill.data(), (size_t)need, s);
    if (a.op == KIN_EVAL_RHS) h->rhs_dev(d_u.p, d_out.p);
    else h->jac_dev(d_u.p, d_out.p);
    KIN_HIP(hipGetLastError());
    d_out.download(a.out, (size_t)need, s);
    KIN_HIP(hipStreamSynchronize(s));
    return;
  }

  // ---- path 2: K members with buffers of the probe's own, n_entries of them in one launch
  require(a.k != nullptr, ERR_INVALID_ARG, "path 2 takes rate constants per member: k is null");
  const int64_t K = a.K;
  auto al = [](int64_t x) { return (x + 7) / 8 * 8; };
  const int64_t nN = al(N), nR = al(R), nDR = al(2 * R + 2), nJ = al(nnz), nV = al(std::max<int64_t>(pl.vec_len, 1));
  DevBuf<double> d_y, d_ytmp, d_f0, d_f1, d_psi, d_d, d_k, d_rate, d_dr, d_jv, d_vec;
  DevBuf<BdfCtrl> d_ctrl;
  auto filled = [&](DevBuf<double>& b, int64_t per, double v) {
    std::vector<double> f((size_t)(K * per), v);
    b.upload(f.data(), f.size(), s);
    KIN_HIP(hipStreamSynchronize(s));
  };
  auto rows = [&](DevBuf<double>& b, int64_t per, const double* src, int64_t len, double pad) {
    std::vector<double> f((size_t)(K * per), pad);
    for (int64_t m = 0; m < K; m++) std::copy(src + m * len, src + (m + 1) * len, f.begin() + m * per);
    b.upload(f.data(), f.size(), s);
    KIN_HIP(hipStreamSynchronize(s));
  };
  // the state goes where the operation reads it; the other source holds the sentinel
  const bool from_ytmp = a.op == KIN_EVAL_RHS && a.mode != 0;
  if (from_ytmp) { rows(d_ytmp, nN, a.u, N, 0.0); filled(d_y, nN, a.sentinel); }
  else { rows(d_y, nN, a.u, N, 0.0); filled(d_ytmp, nN, a.sentinel); }
  rows(d_k, nR, a.k, R, 0.0);
  filled(d_f0, nN, nan); filled(d_f1, nN, nan); filled(d_jv, nJ, nan);
  filled(d_rate, nR, a.sentinel); filled(d_dr, nDR, a.sentinel);
  std::vector<BdfCtrl> hc((size_t)K, BdfCtrl{});
  if (a.op == KIN_EVAL_RESID) {
    rows(d_psi, nN, a.psi, N, 0.0); rows(d_d, nN, a.d, N, 0.0);
    filled(d_vec, nV, a.sentinel);
    for (int64_t m = 0; m < K; m++) hc[m].newton_done = a.done[m];
  }
  d_ctrl.upload(hc.data(), hc.size(), s);
  std::vector<EnsRep> reps((size_t)K);
  for (int64_t m = 0; m < K; m++) {
    EnsRep& r = reps[m];
    r = EnsRep{};
    r.y = d_y.p + m * nN; r.ytmp = d_ytmp.p + m * nN; r.f0 = d_f0.p + m * nN; r.f1 = d_f1.p + m * nN;
    r.psi = d_psi.p ? d_psi.p + m * nN : nullptr; r.d = d_d.p ? d_d.p + m * nN : nullptr;
    r.k = d_k.p + m * nR; r.rate = d_rate.p + m * nR; r.dr = d_dr.p + m * nDR; r.jv = d_jv.p + m * nJ;
    r.ctrl = d_ctrl.p + m;
  }
  std::vector<EnsOp> ops((size_t)a.ne);
  for (int64_t e = 0; e < a.ne; e++) {
    EnsOp& o = ops[e];
    o = EnsOp{};
    o.rep = a.members[e];
    o.i0 = a.op == KIN_EVAL_RHS ? a.mode : 0;
    if (a.op == KIN_EVAL_RESID) {
      o.in.c = a.c[o.rep];
      // W such that W[yloc[i]] is the member's own window: yloc was checked to stay inside [off_y, off_y + vec_len)
      o.W = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(d_vec.p + (int64_t)o.rep * nV) - (uintptr_t)pl.off_y * sizeof(double));
    }
  }
  DevBuf<EnsRep> d_reps;
  DevBuf<EnsOp> d_ops;
  d_reps.upload(reps.data(), reps.size(), s);
  d_ops.upload(ops.data(), ops.size(), s);
  const int cnt = (int)a.ne;
  if (a.op == KIN_EVAL_RHS) ens_rhs((int)N, (int)R, h->x0.p, h->x1.p, h->rhs_plan.view(), d_reps.p, d_ops.p, cnt, s);
  else if (a.op == KIN_EVAL_JAC) ens_jac((int)R, h->x0.p, h->x1.p, h->jac_plan.view(), d_reps.p, d_ops.p, cnt, s);
  else ens_resid((int)R, h->x0.p, h->x1.p, pl.plan->view(), d_reps.p, d_ops.p, cnt, s);
  KIN_HIP(hipGetLastError());
  KIN_HIP(hipStreamSynchronize(s));   // (the tables above live until the launch has run)
  for (int64_t m = 0; m < K; m++) {
    double* o = a.out + m * a.out_len;
    if (a.op == KIN_EVAL_RHS) { KIN_HIP(hipMemcpyAsync(o, d_f0.p + m * nN, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
                                KIN_HIP(hipMemcpyAsync(o + N, d_f1.p + m * nN, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s)); }
    else if (a.op == KIN_EVAL_JAC) { if (nnz > 0) KIN_HIP(hipMemcpyAsync(o, d_jv.p + m * nJ, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, s)); }
    else KIN_HIP(hipMemcpyAsync(o, d_vec.p + m * nV, (size_t)pl.vec_len * sizeof(double), hipMemcpyDeviceToHost, s));
    if (a.rate && R > 0 && a.op != KIN_EVAL_JAC)
      KIN_HIP(hipMemcpyAsync(a.rate + m * R, d_rate.p + m * nR, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, s));
    if (a.rate && R > 0 && a.op == KIN_EVAL_JAC)   // the operand derivatives, 2 R per member
      KIN_HIP(hipMemcpyAsync(a.rate + m * 2 * R, d_dr.p + m * nDR, (size_t)(2 * R) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" int kin_eval_probe(kin_network* h, int32_t path, int32_t op, int32_t mode, int64_t K, int64_t n_entries, const int32_t* members,
                              const double* u, const double* k, double T, const double* c, const double* psi, const double* d,
                              const int32_t* done, double sentinel, double* out, int64_t out_len, double* rate, int32_t* yloc,
                              int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  try {
    KIN_HIP(hipSetDevice(h->device));
    require((path == 0 || path == 2) && op >= KIN_EVAL_RHS && op <= KIN_EVAL_SIZES, ERR_INVALID_ARG, "unknown path or operation");
    require(info != nullptr, ERR_INVALID_ARG, "info is null");
    if (op != KIN_EVAL_SIZES) {
      require(K >= 1 && K <= 64 && n_entries >= 1 && n_entries <= K, ERR_INVALID_ARG, "K or n_entries out of range");
      require(path == 2 || (K == 1 && n_entries == 1), ERR_INVALID_ARG, "path 0 takes one member");
      require(u && out && (path == 0 || members), ERR_INVALID_ARG, "null buffer");
      require(mode >= 0 && mode <= 2 && (mode == 0 || (path == 2 && op == KIN_EVAL_RHS)), ERR_INVALID_ARG, "the source mode belongs to ens_rhs: 0, 1 or 2");
      require(!(T > 0.0) || path == 0, ERR_INVALID_ARG, "a pending temperature belongs to path 0");
      require(T >= 0.0 && std::isfinite(T), ERR_INVALID_ARG, "T must be 0 (none) or a finite temperature");
    }
    static const int32_t member0 = 0;
    eval_probe(h, Args{path, op, mode, K, n_entries, path == 0 ? &member0 : members, u, k, T, c, psi, d, done, sentinel, out, out_len, rate,
                       yloc, info});
  } catch (const KinError& e) {
    h->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}
