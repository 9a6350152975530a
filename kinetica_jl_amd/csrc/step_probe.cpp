// kin_step_probe (declaration and argument layout: include/kinetica_hip.h): one operation of the step, once, on the caller's
// state, through the launchers the integrators use - launch_bdf_* / launch_rk_* (path 0), SparseLU::solve_newton (path 1,
// solver.cpp: step_probe_fused), the ens_* launchers of the lockstep ensemble (path 2), the resident kernel's own dispatch in its
// default and its shared-CU build (paths 3 and 4, resident.cpp: resident_step_probe - the kernel's leader wavefront calls the
// controller's or the backend's method, the other seven decode the command in worker_loop). Nothing here computes: the probe
// uploads, fills the launchers' arguments the way HostBackend / MemberBackend / ResidentBdf fill them, launches, downloads.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "ensemble.hpp"
#include "handle.hpp"
#include "resident.hpp"
#include "solver.hpp"
#include "solver_kernels.hpp"

using namespace kin;

namespace {

enum Row : int { ROW_D = 0, ROW_Y = 8, ROW_PSI, ROW_DD, ROW_SCALE, ROW_F0, ROW_F1, ROW_YTMP, ROW_CS, ROW_K = 16, ROW_X = 23, ROW_OUT, ROW_YNEW,
                 ROW_U, ROW_B };
static_assert(ROW_B + 1 == KIN_STEP_ROWS && BDF_D_ROWS == 8, "row layout of kin_step_probe");
// argument slots (kinetica_hip.h)
enum : int { IA_REP = 0, IA_ORDER, IA_AUX, IA_COPY_OUT, IA_GO, IA_ITER, IA_MAXIT, IA_PUBLISH, IA_CRATE_CTRL, IA_BAN_NEG, IA_SEQ, IA_ROW };
enum : int { DA_ATOL = 0, DA_RTOL, DA_H, DA_UPD, DA_TOL, DA_RATE_MAX, DA_CRATE0, DA_TOL_FIRST, DA_DY_FIRST_MAX, DA_C, DA_TS, DA_T, DA_HABS, DA_W,
             DA_C_FACT = 20, DA_EC, DA_EC_M, DA_EC_P };
static_assert(RES_STEP_ROWS == KIN_STEP_ROWS && RES_STEP_CTRL == KIN_STEP_CTRL && DA_EC_P + 1 == KIN_STEP_DARGS && IA_ROW + 1 == KIN_STEP_IARGS,
              "layouts of the resident kernel's step mode");
constexpr int VEC_SAVE_Y = 6, VEC_SET_TIME = 8;   // (EnsVecOp's EV_SAVE_Y; set_time exists on paths 3 and 4 only)

void ctrl_from(const double* v, BdfCtrl& c) {
  c.dy_norm_old = v[0]; c.dy_norm = v[1]; c.err_norm = v[2]; c.err_m_norm = v[3]; c.err_p_norm = v[4]; c.crate = v[5];
  for (int i = 0; i < 4; i++) c.scratch[i] = v[6 + i];
  c.newton_done = (int)v[10]; c.converged = (int)v[11]; c.n_iter = (int)v[12]; c.nonfinite = (int)v[13]; c.any_negative = (int)v[14];
  c.ticket = (int)v[15]; c.lu_bad = (int)v[16]; c.spec_go = (int)v[17];
}
void ctrl_to(const BdfCtrl& c, double* v) {
  v[0] = c.dy_norm_old; v[1] = c.dy_norm; v[2] = c.err_norm; v[3] = c.err_m_norm; v[4] = c.err_p_norm; v[5] = c.crate;
  for (int i = 0; i < 4; i++) v[6 + i] = c.scratch[i];
  v[10] = c.newton_done; v[11] = c.converged; v[12] = c.n_iter; v[13] = c.nonfinite; v[14] = c.any_negative;
  v[15] = c.ticket; v[16] = c.lu_bad; v[17] = c.spec_go;
}

// publication targets of the probe's own, allocated as HostBackend allocates its pair; all bits set until a launch publishes
struct Pinned {
  BdfCtrl* hc = nullptr; unsigned long long* hseq = nullptr;
  BdfCtrl* hc_dev = nullptr; unsigned long long* hseq_dev = nullptr;
  Pinned() {
    KIN_HIP(hipHostMalloc((void**)&hc, sizeof(BdfCtrl), hipHostMallocCoherent | hipHostMallocMapped));
    KIN_HIP(hipHostMalloc((void**)&hseq, sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped));
    memset(hc, 0xff, sizeof(BdfCtrl));
    *hseq = 0;
    KIN_HIP(hipHostGetDevicePointer((void**)&hc_dev, hc, 0));
    KIN_HIP(hipHostGetDevicePointer((void**)&hseq_dev, hseq, 0));
  }
  ~Pinned() { if (hc) (void)hipHostFree(hc); if (hseq) (void)hipHostFree(hseq); }
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
};

void step_probe(kin_network* h, int path, int op, int64_t n64, int64_t K, int64_t ne, const int32_t* iarg, const double* darg,
                const int32_t* xloc, double* state, double* ctrl, double* pub, int64_t* info) {
  const int n = (int)n64;
  hipStream_t s = h->stream;
  BdfCoef cf;
  bdf_fill_coef(cf.gamma, cf.alpha, cf.error_const);
  // ---- what the kernels index with is checked here: they trust their launchers
  std::vector<char> seen((size_t)K, 0);
  for (int64_t e = 0; e < ne; e++) {
    const int32_t* ia = iarg + e * KIN_STEP_IARGS;
    require(ia[IA_REP] >= 0 && ia[IA_REP] < K && !seen[ia[IA_REP]], ERR_INVALID_ARG, "entry names no member, or one member twice");
    seen[ia[IA_REP]] = 1;
    require(ia[IA_ORDER] >= 1 && ia[IA_ORDER] <= BDF_MAX_ORDER, ERR_INVALID_ARG, "order outside 1 .. 5");
    if (op == KIN_STEP_ACCEPT_PREDICT)
      require(ia[IA_AUX] >= 1 && ia[IA_AUX] <= BDF_MAX_ORDER && ia[IA_ORDER] <= ia[IA_AUX] + 1, ERR_INVALID_ARG, "accepted order outside 1 .. 5, or order > it + 1");
    if (op == KIN_STEP_RK_COMBINE) require(ia[IA_AUX] >= 0 && ia[IA_AUX] <= 7, ERR_INVALID_ARG, "stages outside 0 .. 7");
    if (op == KIN_STEP_VEC) require(ia[IA_AUX] >= EV_LOAD_U0 && ia[IA_AUX] <= EV_INTERP, ERR_INVALID_ARG, "unknown vector operation");
    if (op == KIN_STEP_NEWTON)
      require(ia[IA_ITER] >= 0 && ia[IA_MAXIT] >= 1 && ia[IA_MAXIT] <= 16 && ia[IA_ITER] < ia[IA_MAXIT] && ia[IA_SEQ] >= 0, ERR_INVALID_ARG,
              "iter / maxit / seq out of range");
  }
  const bool scatter = op == KIN_STEP_NEWTON && path != 1;
  if (scatter) {
    require(xloc != nullptr, ERR_INVALID_ARG, "xloc is null");
    std::vector<char> hit((size_t)n, 0);
    for (int i = 0; i < n; i++) {
      require(xloc[i] >= 0 && xloc[i] < n && !hit[xloc[i]], ERR_INVALID_ARG, "xloc is no permutation of 0 .. n-1");
      hit[xloc[i]] = 1;
    }
  }

  const size_t per = (size_t)KIN_STEP_ROWS * n;
  DevBuf<double> d_state, d_W, d_part;
  DevBuf<BdfCtrl> d_ctrl;
  DevBuf<int32_t> d_xloc;
  d_state.upload(state, (size_t)K * per, s);
  std::vector<BdfCtrl> hctrl((size_t)K);
  for (int64_t k = 0; k < K; k++) ctrl_from(ctrl + k * KIN_STEP_CTRL, hctrl[k]);
  d_ctrl.upload(hctrl.data(), (size_t)K, s);
  auto row = [&](int64_t k, int r) { return d_state.p + (size_t)k * per + (size_t)r * n; };
  const size_t part_n = (size_t)bdf_reduce_slot() * bdf_reduce_blocks(n);   // as HostBackend sizes `red` (ens_reduce_doubles: the same)
  d_part.alloc((size_t)K * part_n);
  d_part.zero(s);
  std::vector<double> hW;
  if (scatter) {
    hW.assign((size_t)K * n, 0.0);
    for (int64_t k = 0; k < K; k++)
      for (int i = 0; i < n; i++) hW[(size_t)k * n + xloc[i]] = state[(size_t)k * per + (size_t)ROW_X * n + i];
    d_W.upload(hW.data(), hW.size(), s);
    d_xloc.upload(xloc, (size_t)n, s);
  }
  Pinned pin;
  std::fill(info, info + 8, (int64_t)0);
  std::vector<double> x_fused;

  auto interp_weights = [&](const int32_t* ia, const double* da, double (&p)[BDF_MAX_ORDER + 1]) {
    for (double& v : p) v = 0.0;
    bdf_interp_weights(ia[IA_ORDER], da[DA_TS], da[DA_T], da[DA_HABS], p);
  };

  if (path == 0) {
    const int32_t* ia = iarg; const double* da = darg;
    const int order = ia[IA_ORDER];
    double* D = row(0, ROW_D);
    BdfCtrl* c = d_ctrl.p;
    const unsigned long long seq = (unsigned long long)ia[IA_SEQ];
    switch (op) {
      case KIN_STEP_INIT_D:
        launch_bdf_init_D(n, BDF_D_ROWS, row(0, ia[IA_AUX] ? ROW_YTMP : ROW_Y), row(0, ROW_F0), da[DA_H], D, s); break;
      case KIN_STEP_PREDICT:
        launch_bdf_predict(n, order, D, cf, da[DA_ATOL], da[DA_RTOL], row(0, ROW_Y), row(0, ROW_PSI), row(0, ROW_DD), row(0, ROW_SCALE), c, s); break;
      case KIN_STEP_ACCEPT:
        launch_bdf_accept(n, order, D, row(0, ROW_DD), ia[IA_COPY_OUT] ? row(0, ROW_OUT) : nullptr, s); break;
      case KIN_STEP_ACCEPT_PREDICT:
        launch_bdf_accept_predict(n, ia[IA_AUX], order, D, cf, da[DA_ATOL], da[DA_RTOL], row(0, ROW_Y), row(0, ROW_PSI), row(0, ROW_DD),
                                  row(0, ROW_SCALE), c, ia[IA_COPY_OUT] ? row(0, ROW_OUT) : nullptr, s, ia[IA_GO] ? &c->spec_go : nullptr);
        break;
      case KIN_STEP_CHANGE_D: {
        double M[6][6], R[6][6], U[6][6];
        BdfMat ru{};
        bdf_change_D_matrix(order, da[DA_H], M, R, U, ru.v);
        launch_bdf_change_D(n, order, ru, D, s);
      } break;
      case KIN_STEP_INTERP: {
        BdfVec p;
        interp_weights(ia, da, p.v);
        launch_bdf_interp(n, order, D, p, row(0, ROW_OUT), s);
      } break;
      case KIN_STEP_NORMS:
        launch_bdf_norms(n, row(0, ROW_Y), row(0, ROW_F0), ia[IA_AUX] ? row(0, ROW_F1) : nullptr, da[DA_ATOL], da[DA_RTOL], c, s); break;
      case KIN_STEP_NEWTON:
        launch_bdf_newton(n, ia[IA_ITER], ia[IA_MAXIT], da[DA_TOL], d_xloc.p, d_W.p, row(0, ROW_SCALE), row(0, ROW_Y), row(0, ROW_DD), da[DA_UPD],
                          da[DA_RATE_MAX], da[DA_CRATE0], da[DA_TOL_FIRST], da[DA_DY_FIRST_MAX], order, D, da[DA_ATOL], da[DA_RTOL], cf, c,
                          d_part.p, pin.hc_dev, pin.hseq_dev, seq, ia[IA_PUBLISH] != 0, s, ia[IA_CRATE_CTRL] != 0, ia[IA_BAN_NEG] != 0);
        break;
      case KIN_STEP_RK_COMBINE: {
        RkVec w;
        for (int j = 0; j < 7; j++) w.v[j] = da[DA_W + j];
        launch_rk_combine(n, ia[IA_AUX], w, row(0, ROW_Y), row(0, ROW_K), row(0, ROW_OUT), s);
      } break;
      case KIN_STEP_RK_ERROR: {
        RkVec w;
        for (int j = 0; j < 7; j++) w.v[j] = da[DA_W + j];
        launch_rk_error(n, w, row(0, ROW_Y), row(0, ROW_YNEW), row(0, ROW_K), da[DA_ATOL], da[DA_RTOL], c, d_part.p, pin.hc_dev, pin.hseq_dev,
                        seq, s);
      } break;
      default: throw KinError(ERR_UNSUPPORTED, "the host-driven path has no such operation");
    }
  } else if (path == 1) {
    require(op == KIN_STEP_NEWTON, ERR_UNSUPPORTED, "the fused path has the corrector update only");
    const int32_t* ia = iarg; const double* da = darg;
    const int order = ia[IA_ORDER];
    NewtonFuse f;   // as HostBackend::newton_iteration fills it
    f.skip = nullptr; f.N = n; f.m = 0; f.off_x = 0; f.x2_species = nullptr;
    f.scale = row(0, ROW_SCALE); f.y = row(0, ROW_Y); f.d = row(0, ROW_DD); f.D = row(0, ROW_D); f.order = order;
    f.upd = da[DA_UPD]; f.atol = da[DA_ATOL]; f.rtol = da[DA_RTOL];
    f.ec = cf.error_const[order]; f.ec_m = order > 1 ? cf.error_const[order - 1] : 0.0; f.ec_p = cf.error_const[order + 1];
    f.iter = ia[IA_ITER]; f.maxit = ia[IA_MAXIT]; f.tol = da[DA_TOL]; f.rate_max = da[DA_RATE_MAX]; f.crate0 = da[DA_CRATE0];
    f.tol_first = da[DA_TOL_FIRST]; f.dy_first_max = da[DA_DY_FIRST_MAX]; f.crate_from_ctrl = ia[IA_CRATE_CTRL] ? 1 : 0;
    f.ban_negatives = ia[IA_BAN_NEG] ? 1 : 0;
    f.ctrl = d_ctrl.p; f.part = nullptr; f.host_ctrl = pin.hc_dev; f.host_seq = pin.hseq_dev; f.seq = (unsigned long long)ia[IA_SEQ];
    f.publish_always = ia[IA_PUBLISH] ? 1 : 0;
    x_fused.resize((size_t)n);
    step_probe_fused(h, da[DA_C], state + (size_t)ROW_U * n, state + (size_t)ROW_B * n, f, x_fused.data(), info);
  } else {
    std::vector<EnsRep> reps((size_t)K);
    for (int64_t k = 0; k < K; k++) {
      EnsRep& r = reps[k];
      r = EnsRep{};
      r.D = row(k, ROW_D); r.y = row(k, ROW_Y); r.psi = row(k, ROW_PSI); r.d = row(k, ROW_DD); r.scale = row(k, ROW_SCALE);
      r.f0 = row(k, ROW_F0); r.f1 = row(k, ROW_F1); r.ytmp = row(k, ROW_YTMP); r.cs = row(k, ROW_CS);
      r.part = d_part.p + (size_t)k * part_n; r.ctrl = d_ctrl.p + k;
    }
    std::vector<EnsOp> ops((size_t)ne);
    for (int64_t e = 0; e < ne; e++) {
      const int32_t* ia = iarg + e * KIN_STEP_IARGS; const double* da = darg + e * KIN_STEP_DARGS;
      const int order = ia[IA_ORDER];
      EnsOp& o = ops[e];
      o = EnsOp{};
      o.rep = ia[IA_REP];
      o.out = row(o.rep, ROW_OUT);
      switch (op) {
        case KIN_STEP_INIT_D: o.i0 = ia[IA_AUX] ? 1 : 0; o.d0 = da[DA_H]; break;
        case KIN_STEP_ACCEPT: o.i0 = order; break;
        case KIN_STEP_NORMS: o.i0 = ia[IA_AUX] ? 1 : 0; o.d0 = da[DA_ATOL]; o.d1 = da[DA_RTOL]; break;
        case KIN_STEP_CHANGE_D: {   // (MemberBackend::change_D: the identity outside the orders involved)
          double M[6][6], R[6][6], U[6][6], RU[6][6];
          bdf_change_D_matrix(order, da[DA_H], M, R, U, RU);
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) o.ru[i * 6 + j] = (i <= order && j <= order) ? RU[i][j] : (i == j ? 1.0 : 0.0);
        } break;
        case KIN_STEP_INTERP:
        case KIN_STEP_VEC: {
          o.i0 = op == KIN_STEP_INTERP ? (int)EV_INTERP : ia[IA_AUX];
          o.i1 = order; o.d0 = da[DA_H];
          if (o.i0 == EV_INTERP) {
            double p[BDF_MAX_ORDER + 1];
            interp_weights(ia, da, p);
            for (int j = 0; j <= BDF_MAX_ORDER; j++) o.p[j] = p[j];
          }
        } break;
        case KIN_STEP_PREDICT:
        case KIN_STEP_NEWTON: {   // (ResidentBdf::corrector)
          ResCorrIn& in = o.in;
          in.slot = 0; in.order = order; in.c = da[DA_C]; in.upd = da[DA_UPD]; in.rate_max = da[DA_RATE_MAX]; in.crate0 = da[DA_CRATE0];
          in.tol_first = da[DA_TOL_FIRST]; in.newton_tol = da[DA_TOL]; in.dy_first_max = da[DA_DY_FIRST_MAX];
          in.ec = cf.error_const[order]; in.ec_m = order > 1 ? cf.error_const[order - 1] : 0.0; in.ec_p = cf.error_const[order + 1];
          in.atol = da[DA_ATOL]; in.rtol = da[DA_RTOL]; in.alpha_o = cf.alpha[order];
          o.i0 = op == KIN_STEP_PREDICT ? (ia[IA_AUX] ? 1 : 0) : 0;
          o.W = scatter ? d_W.p + (size_t)o.rep * n : nullptr;
        } break;
        default: throw KinError(ERR_UNSUPPORTED, "the lockstep ensemble has no such operation");
      }
    }
    DevBuf<EnsRep> d_reps;
    DevBuf<EnsOp> d_ops;
    d_reps.upload(reps.data(), reps.size(), s);
    d_ops.upload(ops.data(), ops.size(), s);
    const int cnt = (int)ne;
    switch (op) {
      case KIN_STEP_INIT_D: ens_init_D(n, d_reps.p, d_ops.p, cnt, s); break;
      case KIN_STEP_ACCEPT: ens_accept(n, d_reps.p, d_ops.p, cnt, s); break;
      case KIN_STEP_NORMS: ens_norms(n, d_reps.p, d_ops.p, cnt, s); break;
      case KIN_STEP_CHANGE_D: ens_change_D(n, d_reps.p, d_ops.p, cnt, s); break;
      case KIN_STEP_INTERP:
      case KIN_STEP_VEC: ens_vec(n, d_reps.p, d_ops.p, cnt, s); break;
      case KIN_STEP_PREDICT: {
        EnsSolveTables T{};
        T.N = n; T.cf = cf;
        ens_predict(T, d_reps.p, d_ops.p, cnt, s);
      } break;
      default: ens_newton(n, iarg[IA_ITER], d_xloc.p, cf, d_reps.p, d_ops.p, cnt, s); break;
    }
    KIN_HIP(hipGetLastError());
    KIN_HIP(hipStreamSynchronize(s));   // (the tables above live until the launch has run)
  }
  KIN_HIP(hipGetLastError());
  d_state.download(state, (size_t)K * per, s);
  d_ctrl.download(hctrl.data(), (size_t)K, s);
  KIN_HIP(hipStreamSynchronize(s));
  for (int64_t k = 0; k < K; k++) ctrl_to(hctrl[k], ctrl + k * KIN_STEP_CTRL);
  if (path == 1) std::copy(x_fused.begin(), x_fused.end(), state + (size_t)ROW_X * n);
  ctrl_to(*pin.hc, pub);
  pub[KIN_STEP_CTRL] = (double)*pin.hseq;
}

// paths 3 and 4: the resident kernel's own dispatch (resident.cpp: resident_step_probe). Everything the kernel indexes with - orders,
// solution rows, members, the operation - is checked here, before any launch; the entries are reordered by member.
void step_probe_resident(kin_network* h, int path, int op, int64_t n, int64_t K, int64_t ne, const int32_t* iarg, const double* darg,
                         double* state, double* ctrl, double* pub, int64_t* info) {
  require(n == h->host.N, ERR_INVALID_ARG, "the resident paths run on the handle's network: n must be its species count");
  require(ne == K, ERR_INVALID_ARG, "the resident paths take one entry per member");
  std::vector<ResStepArg> args((size_t)K);
  std::vector<char> seen((size_t)K, 0);
  BdfCoef cf;
  bdf_fill_coef(cf.gamma, cf.alpha, cf.error_const);
  int rop = -1;
  for (int64_t e = 0; e < ne; e++) {
    const int32_t* ia = iarg + e * KIN_STEP_IARGS; const double* da = darg + e * KIN_STEP_DARGS;
    require(ia[IA_REP] >= 0 && ia[IA_REP] < K && !seen[ia[IA_REP]], ERR_INVALID_ARG, "entry names no member, or one member twice");
    seen[ia[IA_REP]] = 1;
    require(ia[IA_ORDER] >= 1 && ia[IA_ORDER] <= BDF_MAX_ORDER, ERR_INVALID_ARG, "order outside 1 .. 5");
    require(ia[IA_ROW] == 0 || ia[IA_ROW] == 1, ERR_INVALID_ARG, "solution row outside {0, 1}");
    int aux = ia[IA_AUX], r = -1;
    switch (op) {
      case KIN_STEP_VEC:
        require((aux >= 0 && aux <= VEC_SAVE_Y) || aux == VEC_SET_TIME, ERR_INVALID_ARG, "unknown vector operation");
        r = aux == VEC_SAVE_Y ? RES_STEP_SAVE_Y : (aux == VEC_SET_TIME ? RES_STEP_SET_TIME : RES_STEP_VEC);
        if (r != RES_STEP_VEC) aux = 0;
        break;
      case KIN_STEP_NORMS: r = RES_STEP_NORMS; aux = aux ? 1 : 0; break;
      case KIN_STEP_INIT_D: r = RES_STEP_INIT_D; aux = aux ? 1 : 0; break;
      case KIN_STEP_PREDICT: r = RES_STEP_PREDICT; aux = 0; break;
      case KIN_STEP_ACCEPT: r = RES_STEP_ACCEPT; aux = 0; break;
      case KIN_STEP_CHANGE_D: r = RES_STEP_CHANGE_D; aux = 0; break;
      case KIN_STEP_INTERP: r = RES_STEP_INTERP; aux = 0; break;
      case KIN_STEP_NEWTON: r = RES_STEP_NEWTON; aux = 0; break;
      case KIN_STEP_CORRECTOR: r = RES_STEP_CORRECTOR; aux = 0; break;
      default: throw KinError(ERR_UNSUPPORTED, "the resident kernel has no such operation");
    }
    require(rop < 0 || rop == r, ERR_INVALID_ARG, "the entries of one launch name different operations");
    rop = r;
    ResStepArg& a = args[ia[IA_REP]];
    a = ResStepArg{};
    a.order = ia[IA_ORDER]; a.aux = aux; a.row = ia[IA_ROW];
    a.atol = da[DA_ATOL]; a.rtol = da[DA_RTOL]; a.h = da[DA_H]; a.t = da[DA_T]; a.h_abs = da[DA_HABS]; a.ts = da[DA_TS]; a.c_fact = da[DA_C_FACT];
    ResCorrIn& in = a.in;   // (ResidentBdf::corrector)
    in.slot = 0; in.order = a.order; in.c = da[DA_C]; in.upd = da[DA_UPD]; in.rate_max = da[DA_RATE_MAX]; in.crate0 = da[DA_CRATE0];
    in.tol_first = da[DA_TOL_FIRST]; in.newton_tol = da[DA_TOL]; in.dy_first_max = da[DA_DY_FIRST_MAX];
    in.ec = da[DA_EC]; in.ec_m = da[DA_EC_M]; in.ec_p = da[DA_EC_P];
    in.atol = da[DA_ATOL]; in.rtol = da[DA_RTOL]; in.alpha_o = cf.alpha[a.order];
  }
  if (rop == RES_STEP_NEWTON || rop == RES_STEP_CORRECTOR) require(h->has_rates, ERR_STATE, "rates were never set");
  resident_step_probe(h, path == 4 ? 4 : 2, rop, K, args.data(), state, ctrl, info);
  for (int i = 0; i < KIN_STEP_CTRL; i++) pub[i] = i < 10 ? NAN : -1.0;   // (nothing is published on these paths)
  pub[KIN_STEP_CTRL] = 0.0;
}

}  // namespace

extern "C" int kin_step_probe(kin_network* h, int32_t path, int32_t op, int64_t n, int64_t K, int64_t n_entries, const int32_t* iarg,
                              const double* darg, const int32_t* xloc, double* state, double* ctrl, double* pub, int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  try {
    KIN_HIP(hipSetDevice(h->device));
    require(path >= 0 && path <= 4 && op >= KIN_STEP_INIT_D && op <= KIN_STEP_CORRECTOR, ERR_INVALID_ARG, "unknown path or operation");
    require(n >= 1 && n <= (1 << 24) && K >= 1 && K <= 64 && n_entries >= 1 && n_entries <= K, ERR_INVALID_ARG, "n, K or n_entries out of range");
    require(path >= 2 || (K == 1 && n_entries == 1), ERR_INVALID_ARG, "paths 0 and 1 take one member");
    require(iarg && darg && state && ctrl && pub && info, ERR_INVALID_ARG, "null buffer");
    if (path >= 3) {
      step_probe_resident(h, path, op, n, K, n_entries, iarg, darg, state, ctrl, pub, info);
      return KIN_OK;
    }
    require(op != KIN_STEP_CORRECTOR, ERR_UNSUPPORTED, "a whole corrector attempt is an operation of the resident kernel (paths 3 and 4)");
    if (path == 1) {
      require(n == h->host.N, ERR_INVALID_ARG, "the fused path runs on the handle's network: n must be its species count");
      require(h->has_rates, ERR_STATE, "rates were never set");
    }
    step_probe(h, path, op, n, K, n_entries, iarg, darg, xloc, state, ctrl, pub, info);
  } catch (const KinError& e) {
    h->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}
