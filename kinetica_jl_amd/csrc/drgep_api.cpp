// extern "C" entry points of DRG with error propagation (declarations: include/kinetica_hip.h; tables: drg.cpp; stage 2:
// drg_kernels.hip, SIGNED; path stage: drgep_kernels.hip). Batches, blocks and staging: flux_api.hpp; stage 1 with the
// denominators and the tables of a pairing mode: drg_api.hpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>

#include "drg_api.hpp"

using namespace kin;

namespace {

// States per block: none of rates[nb][R], r[nb][E] and work[nb][2][N] above the bound
int64_t drgep_block(const kin_network* h, int64_t E, int64_t B) {
  return block_states((size_t)std::max<int64_t>(std::max<int64_t>(h->host.R, E), std::max<int64_t>(2 * h->host.N, 1)), B, DRG_BLOCK_ENV);
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

// The pass on the device, block by block: stage 1 (the flux sweep) writes the block's rates, the signed stage 2 its
// denominators and r[nb][E], the path stage R[nb][N], folded into d_imp. Without an edge only the path stage runs.
void drgep_run(kin_network* h, int pairing, const StateBatch& b, const int64_t* d_targets, int64_t n_targets, int accumulate,
               double* d_imp, const DrgepOut& out, hipStream_t s) {
  const int64_t N = h->host.N;
  auto& m = drgep_dev(h, pairing, s);
  const int64_t E = m.host->E;
  if (N == 0 || empty_batch(b.B, d_imp, N, accumulate, s)) return;
  int upto = 3;      // KIN_DRGEP_STAGES=1 / 2 ends every block after stage 1 / 2 and leaves d_imp alone: for timing the stages only
  if (const char* e = getenv("KIN_DRGEP_STAGES")) upto = atoi(e) >= 1 ? atoi(e) : 3;
  const int64_t nb_max = drgep_block(h, E, b.B);
  if (E > 0) drg_stage_alloc(h, nb_max);
  drgep_alloc(h, nb_max, E);
  const DrgPlan den = signed_den_plan(m), edge = signed_edge_plan(m);
  for_blocks(b.B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
    if (E > 0) {
      DrgArgs a{};
      a.E = (int)E; a.r = h->drgep_r.p;
      drg_rates_den(h, b, b0, nb, den, true, upto, a, s);
      if (upto < 2) return;
      edge.into(a);
      launch_drgep_edges(a, slices_cap(drg_slices(edge.p, nb, h->n_cu)), s);
    }
    if (upto < 3) return;
    drgep_paths_block(h, m, b0, nb, b.seg_n, b.L, d_targets, n_targets, use_prev, d_imp, out, s);
  });
}

// host entries: the targets behind the batch (checked, made 0-based and uploaded), importance staged through the handle
template <class F>
void drgep_host_call(kin_network* h, const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance,
                     hipStream_t s, F run) {
  const int64_t* d_t =
      species_list(h, targets, n_targets, index_base, "DRGEP needs at least one target species", "target species out of range", s);
  staged_result(h, h->host.N, importance, accumulate, s, [&](double* d_imp) { run(d_t, d_imp); });
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
  drgep_run(h, pairing, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, d_targets, n_targets, accumulate,
            d_importance, DrgepOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_drgep_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T, const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance,
                      double* r_out, double* R_out, int32_t* rounds_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, importance != nullptr);
  hipStream_t s = h->stream;
  const StateBatch b = host_batch(h, B, u, k, n_k_rows, k_row, T, s);
  drgep_host_call(h, targets, n_targets, index_base, accumulate, importance, s, [&](const int64_t* d_t, double* d_imp) {
    drgep_run(h, pairing, b, d_t, n_targets, accumulate, d_imp, DrgepOut{r_out, R_out, rounds_out}, s);
  });
  KIN_CATCH(h)
}

int kin_drgep_paths(kin_network* h, int pairing, int64_t B, const double* r, const int64_t* targets, int64_t n_targets, int index_base,
                    int accumulate, double* importance, double* R_out, int32_t* rounds_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B >= 0 && B < ((int64_t)1 << 31), ERR_INVALID_ARG, "B out of range");
  require(importance != nullptr, ERR_INVALID_ARG, "null output buffer");
  drg_limit(h);
  hipStream_t s = h->stream;
  const int64_t N = h->host.N, E = drg_host(h, pairing).E;
  require(r != nullptr || B == 0 || E == 0, ERR_INVALID_ARG, "null coefficient buffer");
  for (size_t i = 0, n = (size_t)B * (size_t)E; i < n; i++)
    require(std::isfinite(r[i]) && r[i] >= 0.0 && r[i] <= 1.0, ERR_INVALID_ARG, "r: coefficients must be finite and in [0, 1]");
  drgep_host_call(h, targets, n_targets, index_base, accumulate, importance, s, [&](const int64_t* d_t, double* d_imp) {
    auto& m = drgep_dev(h, pairing, s);
    if (N == 0 || empty_batch(B, d_imp, N, accumulate, s)) return;
    const int64_t nb_max = drgep_block(h, E, B);
    drgep_alloc(h, nb_max, E);
    for_blocks(B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
      if (E > 0) h->drgep_r.upload(r + (size_t)b0 * E, (size_t)nb * E, s);
      drgep_paths_block(h, m, b0, nb, nullptr, 0, d_t, n_targets, use_prev, d_imp, DrgepOut{nullptr, R_out, rounds_out}, s);
    });
  });
  KIN_CATCH(h)
}

int kin_solution_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                       const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const StateBatch b = solution_batch(h, drg_check, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  drgep_host_call(h, targets, n_targets, index_base, accumulate, importance, s, [&](const int64_t* d_t, double* d_imp) {
    drgep_run(h, pairing, b, d_t, n_targets, accumulate, d_imp, DrgepOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

int kin_ensemble_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                       const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const StateBatch b = ensemble_batch(h, drg_check, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  drgep_host_call(h, targets, n_targets, index_base, accumulate, importance, s, [&](const int64_t* d_t, double* d_imp) {
    drgep_run(h, pairing, b, d_t, n_targets, accumulate, d_imp, DrgepOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

}  // extern "C"
