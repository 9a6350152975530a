// extern "C" entry points of DRG with error propagation (declarations: include/kinetica_hip.h; tables: drg.cpp; stage 2:
// drg_kernels.hip, SIGNED; path stage: drgep_kernels.hip). Stage 1, the checks and the rate-constant sources are the
// directed-relation-graph pass's (drg_api.hpp).
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "drg_api.hpp"

using namespace kin;

namespace {

void require(bool c, int code, const char* msg) {
  if (!c) throw KinError(code, msg);
}

// States per block: none of rates[nb][R], r[nb][E] and work[nb][2][N] above 256 MB; KIN_DRG_BLOCK_STATES as in the DRG pass.
int64_t drgep_block(const kin_network* h, int64_t E, int64_t B) {
  const size_t row = (size_t)std::max<int64_t>(std::max<int64_t>(h->host.R, E), std::max<int64_t>(2 * h->host.N, 1)) * sizeof(double);
  int64_t nb_max = std::max<int64_t>(1, (int64_t)(DRG_RATES_BYTES / row));
  if (const char* e = getenv("KIN_DRG_BLOCK_STATES")) {   // (read per call: tests change it)
    const int64_t v = atoll(e);
    if (v >= 1) nb_max = std::min(nb_max, v);
  }
  return std::min(nb_max, B);
}

bool drgep_in_lds(int64_t N) {
  int64_t lim = DRGEP_LDS_SPECIES;
  if (const char* e = getenv("KIN_DRGEP_LDS_SPECIES")) {  // (read per call: tests force the global form with it)
    const int64_t v = atoll(e);
    if (v >= 0) lim = std::min(lim, v);
  }
  return N <= lim;
}

struct DrgepOut { double* r; double* R; int32_t* rounds; };   // optional host outputs of the host entries, per state

// The path stage of one block whose coefficients are in h->drgep_r, folded into d_imp; the optional outputs are downloaded.
void drgep_paths_block(kin_network* h, kin_network::DrgMode& m, int64_t b0, int64_t nb, const int64_t* d_seg_n, int64_t L,
                       const int64_t* d_targets, int64_t n_targets, int use_prev, double* d_imp, const DrgepOut& out, hipStream_t s) {
  const DrgTables& t = *m.host;
  const int64_t N = t.N, E = t.E;
  DrgepPathArgs p{};
  p.N = (int)N; p.E = (int)E; p.nb = (int)nb; p.n_targets = (int)n_targets;
  p.in_ptr = m.in_ptr.p; p.in_src = m.in_src.p; p.in_edge = m.in_edge.p; p.in_order = m.in_order.p;
  p.n_short = (int)t.in_cls[0]; p.n_wave = (int)t.in_cls[1]; p.n_long = (int)t.in_cls[2];
  p.targets = d_targets; p.r = h->drgep_r.p;
  p.b0 = b0; p.seg_n = d_seg_n; p.L = L;
  p.R = h->drgep_R.p; p.work = h->drgep_work.p; p.rounds = h->drgep_rounds.p;
  launch_drgep_paths(p, drgep_in_lds(N), s);
  launch_drgep_max(N, nb, h->drgep_R.p, d_imp, use_prev, s);
  if (out.r && E > 0) h->drgep_r.download(out.r + (size_t)b0 * E, (size_t)nb * E, s);
  if (out.R) h->drgep_R.download(out.R + (size_t)b0 * N, (size_t)nb * N, s);
  if (out.rounds) h->drgep_rounds.download(out.rounds + b0, (size_t)nb, s);
}

void drgep_alloc(kin_network* h, int64_t nb_max, int64_t E) {
  const int64_t N = h->host.N;
  h->drgep_r.alloc((size_t)nb_max * E);
  h->drgep_R.alloc((size_t)nb_max * N);
  if (!drgep_in_lds(N)) h->drgep_work.alloc((size_t)nb_max * 2 * N);
  h->drgep_rounds.alloc((size_t)nb_max);
}

// The pass on device buffers, block by block: stage 1 (the flux sweep) writes the block's rates, the signed stage 2 its
// denominators and r[nb][E], the path stage R[nb][N], folded into d_imp. seg_n / L: see DrgArgs.
void drgep_run(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
               const int64_t* d_targets, int64_t n_targets, int accumulate, double* d_imp, const DrgepOut& out, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  auto& m = drgep_dev(h, pairing, s);
  const int64_t E = m.host->E;
  if (N == 0) return;
  if (B == 0) {
    if (!accumulate) KIN_HIP(hipMemsetAsync(d_imp, 0, (size_t)N * sizeof(double), s));
    return;
  }
  int upto = 3;      // KIN_DRGEP_STAGES=1 / 2 ends every block after stage 1 / 2 and leaves d_imp alone: for timing the stages only
  if (const char* e = getenv("KIN_DRGEP_STAGES")) upto = atoi(e) >= 1 ? atoi(e) : 3;
  const int64_t nb_max = drgep_block(h, E, B);
  if (E > 0) { h->drg_rates.alloc((size_t)nb_max * R); h->drg_den.alloc((size_t)nb_max * N); }
  drgep_alloc(h, nb_max, E);
  const SegPlanView dv = m.den_plan.view(), ev = m.edge_plan.view();
  for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
    const int64_t nb = std::min(nb_max, B - b0);
    if (E > 0) {
      FluxSource bs = src;
      if (bs.k && !bs.k_row) bs.k += (size_t)b0 * (size_t)bs.k_stride;
      if (bs.k_row) bs.k_row += b0;
      if (bs.T) bs.T += b0;
      flux_run(h, nb, d_u + (size_t)b0 * N, bs, nullptr, nullptr, h->drg_rates.p, s);
      if (upto < 2) continue;
      DrgArgs a{};
      a.N = (int)N; a.R = (int)R; a.E = (int)E; a.nb = (int)nb;
      a.rates = h->drg_rates.p; a.b0 = b0; a.seg_n = d_seg_n; a.L = L;
      a.den = h->drg_den.p; a.r = h->drgep_r.p;
      a.p = dv; a.ell_c = m.den_ell_s.p; a.long_c = m.den_long_s.p;
      launch_drgep_den(a, slices_cap(drg_slices(dv, nb, h->n_cu)), s);
      a.p = ev; a.ell_c = m.edge_ell_s.p; a.long_c = m.edge_long_s.p;
      launch_drgep_edges(a, slices_cap(drg_slices(ev, nb, h->n_cu)), s);
    }
    if (upto < 3) continue;
    drgep_paths_block(h, m, b0, nb, d_seg_n, L, d_targets, n_targets, (accumulate || b0 > 0) ? 1 : 0, d_imp, out, s);
  }
}

// targets of a host entry: checked, made 0-based and uploaded
const int64_t* drgep_targets(kin_network* h, const int64_t* targets, int64_t n_targets, int index_base, hipStream_t s) {
  require(targets != nullptr && n_targets >= 1, ERR_INVALID_ARG, "DRGEP needs at least one target species");
  std::vector<int64_t> t(targets, targets + n_targets);
  for (int64_t& x : t) {
    x -= index_base;
    require(x >= 0 && x < h->host.N, ERR_INVALID_ARG, "target species out of range");
  }
  h->drgep_targets.upload(t, s);
  KIN_HIP(hipStreamSynchronize(s));      // (t leaves scope)
  return h->drgep_targets.p;
}

// host entries: importance staged through the handle's buffer (uploaded first when it takes part in the maximum)
template <class F>
void drgep_host_call(kin_network* h, int accumulate, double* importance, hipStream_t s, F run) {
  const int64_t N = h->host.N;
  h->drgep_imp.alloc((size_t)N);
  if (accumulate && N > 0) h->drgep_imp.upload(importance, (size_t)N, s);
  run(h->drgep_imp.p);
  if (N > 0) h->drgep_imp.download(importance, (size_t)N, s);
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

namespace kin {

kin_network::DrgMode& drgep_dev(kin_network* h, int pairing, hipStream_t s) {
  auto& m = drg_dev(h, pairing, s);
  if (!m.ep_ready) {
    const DrgTables& t = *m.host;
    m.den_ell_s.upload(t.den_ell_s, s); m.den_long_s.upload(t.den_long_s, s);
    m.edge_ell_s.upload(t.edge_ell_s, s); m.edge_long_s.upload(t.edge_long_s, s);
    m.in_ptr.upload(t.in_ptr, s); m.in_src.upload(t.in_src, s); m.in_edge.upload(t.in_edge, s); m.in_order.upload(t.in_order, s);
    KIN_HIP(hipStreamSynchronize(s));
    m.ep_ready = true;
  }
  return m;
}

}  // namespace kin

#define KIN_TRY(h) try { KIN_HIP(hipSetDevice((h)->device));
#define KIN_CATCH(h)                                                        \
  }                                                                         \
  catch (const KinError& e) { (h)->err = e.what(); return e.code; }         \
  catch (const std::exception& e) { (h)->err = e.what(); return KIN_ERR_DEVICE; } \
  return KIN_OK;

extern "C" {

int kin_drgep_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                          const double* d_T, const int64_t* d_targets, int64_t n_targets, int accumulate, double* d_importance,
                          void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_importance != nullptr);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  require(d_targets != nullptr && n_targets >= 1 && n_targets < ((int64_t)1 << 31), ERR_INVALID_ARG, "DRGEP needs at least one target species");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  drgep_run(h, pairing, B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0, d_targets, n_targets, accumulate, d_importance,
            DrgepOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_drgep_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T, const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance,
                      double* r_out, double* R_out, int32_t* rounds_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, importance != nullptr);
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); flux_check_rows(k_row, B, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == B)");
  const int64_t N = h->host.N, R = h->host.R;
  hipStream_t s = h->stream;
  const int64_t* d_t = drgep_targets(h, targets, n_targets, index_base, s);
  if (B > 0) h->f_u.upload(u, (size_t)B * N, s);
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row && B > 0) h->f_krow.upload(k_row, (size_t)B, s);
  if (T && B > 0) h->f_T.upload(T, (size_t)B, s);
  const FluxSource src{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T ? h->f_T.p : nullptr};
  drgep_host_call(h, accumulate, importance, s, [&](double* d_imp) {
    drgep_run(h, pairing, B, h->f_u.p, src, nullptr, 0, d_t, n_targets, accumulate, d_imp, DrgepOut{r_out, R_out, rounds_out}, s);
  });
  KIN_CATCH(h)
}

int kin_drgep_paths(kin_network* h, int pairing, int64_t B, const double* r, const int64_t* targets, int64_t n_targets, int index_base,
                    int accumulate, double* importance, double* R_out, int32_t* rounds_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B >= 0 && B < ((int64_t)1 << 31), ERR_INVALID_ARG, "B out of range");
  require(importance != nullptr, ERR_INVALID_ARG, "null output buffer");
  require(h->host.N < ((int64_t)1 << 31) / 2, ERR_UNSUPPORTED, "DRG pass: N beyond 32-bit offsets");
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, E = drg_host(h, pairing).E;
  require(r != nullptr || B == 0 || E == 0, ERR_INVALID_ARG, "null coefficient buffer");
  for (size_t i = 0, n = (size_t)B * (size_t)E; i < n; i++)
    require(std::isfinite(r[i]) && r[i] >= 0.0 && r[i] <= 1.0, ERR_INVALID_ARG, "r: coefficients must be finite and in [0, 1]");
  const int64_t* d_t = drgep_targets(h, targets, n_targets, index_base, s);
  drgep_host_call(h, accumulate, importance, s, [&](double* d_imp) {
    auto& m = drgep_dev(h, pairing, s);
    if (N == 0) return;
    if (B == 0) {
      if (!accumulate) KIN_HIP(hipMemsetAsync(d_imp, 0, (size_t)N * sizeof(double), s));
      return;
    }
    const int64_t nb_max = drgep_block(h, E, B);
    drgep_alloc(h, nb_max, E);
    for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
      const int64_t nb = std::min(nb_max, B - b0);
      if (E > 0) h->drgep_r.upload(r + (size_t)b0 * E, (size_t)nb * E, s);
      drgep_paths_block(h, m, b0, nb, nullptr, 0, d_t, n_targets, (accumulate || b0 > 0) ? 1 : 0, d_imp, DrgepOut{nullptr, R_out, rounds_out}, s);
    }
  });
  KIN_CATCH(h)
}

int kin_solution_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                       const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_solution_source(h, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  const int64_t* d_t = drgep_targets(h, targets, n_targets, index_base, s);
  drgep_host_call(h, accumulate, importance, s, [&](double* d_imp) {
    drgep_run(h, pairing, h->n_saved, h->d_sol_u.p, src, nullptr, 0, d_t, n_targets, accumulate, d_imp, DrgepOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

int kin_ensemble_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                       const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_ensemble_source(h, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  const int64_t* d_t = drgep_targets(h, targets, n_targets, index_base, s);
  drgep_host_call(h, accumulate, importance, s, [&](double* d_imp) {
    drgep_run(h, pairing, h->ens.K * h->ens.cap, h->ens.sol, src, h->ens_segn.p, h->ens.cap, d_t, n_targets, accumulate, d_imp,
              DrgepOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

}  // extern "C"
