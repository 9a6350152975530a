// extern "C" entry points of the directed-relation-graph pass (declarations: include/kinetica_hip.h; tables: drg.cpp;
// kernels: drg_kernels.hip) and of the reaction-importance pass, which runs that pass's first two stages (kernel:
// reaction_importance_kernels.hip). Batches, blocks and staging: flux_api.hpp; the family's own: drg_api.hpp, defined here.
// kin_drg_pattern_host and kin_reaction_importance_plan_host, which need no handle, sit with the other host-only entries in
// capi.cpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>

#include "drg_api.hpp"

using namespace kin;

namespace kin {

DrgTables& drg_host(kin_network* h, int pairing) {
  auto& m = h->drg[pairing ? 1 : 0];
  if (!m.host) m.host = std::make_unique<DrgTables>(build_drg_tables(h->host, pairing, true));
  return *m.host;
}

kin_network::DrgMode& drg_dev(kin_network* h, int pairing, hipStream_t s) {
  auto& m = h->drg[pairing ? 1 : 0];
  const DrgTables& t = drg_host(h, pairing);
  if (!m.dev_ready) {
    m.den_plan.upload(t.den_plan, s); m.edge_plan.upload(t.edge_plan, s);
    m.den_ell_c.upload(t.den_ell_c, s); m.den_long_c.upload(t.den_long_c, s);
    m.edge_ell_c.upload(t.edge_ell_c, s); m.edge_long_c.upload(t.edge_long_c, s);
    KIN_HIP(hipStreamSynchronize(s));
    m.dev_ready = true;
  }
  return m;
}

void drg_stage_alloc(kin_network* h, int64_t nb_max) {
  h->drg_rates.alloc((size_t)nb_max * h->host.R);
  h->drg_den.alloc((size_t)nb_max * h->host.N);
}

void drg_rates_den(kin_network* h, const StateBatch& b, int64_t b0, int64_t nb, const DrgPlan& den, bool signed_den, int stages,
                   DrgArgs& a, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  flux_run(h, nb, b.u + (size_t)b0 * N, b.src.at(b0), nullptr, nullptr, h->drg_rates.p, s);
  if (stages < 2) return;
  a.N = (int)N; a.R = (int)R; a.nb = (int)nb;
  a.rates = h->drg_rates.p; a.b0 = b0; a.seg_n = b.seg_n; a.L = b.L;
  a.den = h->drg_den.p;
  den.into(a);
  const int Y = slices_cap(drg_slices(den.p, nb, h->n_cu));
  if (signed_den) launch_drgep_den(a, Y, s);
  else launch_drg_den(a, Y, s);
}

}  // namespace kin

namespace {

// The pass on the device. The batch's states are taken block by block: stage 1 (the flux sweep) writes the block's rates,
// stage 2 its denominators and the maxima of the ratios, folded into d_coef.
void drg_run(kin_network* h, int pairing, const StateBatch& b, int accumulate, double* d_coef, hipStream_t s) {
  auto& m = drg_dev(h, pairing, s);
  const int64_t E = m.host->E;
  if (E == 0 || empty_batch(b.B, d_coef, E, accumulate, s)) return;
  const int64_t nb_max = block_states((size_t)h->host.R, b.B, DRG_BLOCK_ENV);
  drg_stage_alloc(h, nb_max);
  const DrgPlan den{m.den_plan.view(), m.den_ell_c.p, m.den_long_c.p}, edge{m.edge_plan.view(), m.edge_ell_c.p, m.edge_long_c.p};
  h->drg_part.alloc((size_t)slices_cap(drg_slices(edge.p, nb_max, h->n_cu)) * E);
  for_blocks(b.B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
    DrgArgs a{};
    a.E = (int)E; a.part = h->drg_part.p;
    drg_rates_den(h, b, b0, nb, den, false, 2, a, s);
    edge.into(a);
    const int Ye = slices_cap(drg_slices(edge.p, nb, h->n_cu));
    launch_drg_edges(a, Ye, s);
    launch_drg_max(E, Ye, h->drg_part.p, d_coef, use_prev, s);
  });
}

// host entries: coef staged through the handle
void drg_host_call(kin_network* h, int pairing, const StateBatch& b, int accumulate, double* coef, hipStream_t s) {
  staged_result(h, drg_host(h, pairing).E, coef, accumulate, s, [&](double* d_coef) { drg_run(h, pairing, b, accumulate, d_coef, s); });
}

// ---- reaction importance ------------------------------------------------------------------------------------------------
RiTables& ri_host(kin_network* h, int pairing) {
  auto& m = h->ri[pairing ? 1 : 0];
  if (!m.host) m.host = std::make_unique<RiTables>(build_ri_tables(h->host, pairing));
  return *m.host;
}

// the denominator plan of a pairing mode on the device: the DRG pass's when that has been uploaded, else one built without edges
DrgPlan ri_dev(kin_network* h, int pairing, hipStream_t s) {
  auto& m = h->ri[pairing ? 1 : 0];
  auto& g = h->drg[pairing ? 1 : 0];
  if (!m.dev_ready) {
    m.tab.upload(ri_host(h, pairing).dev(), s);
    if (!g.dev_ready) {
      m.den_host = std::make_unique<DrgTables>(build_drg_tables(h->host, pairing, true, false));
      m.den_plan.upload(m.den_host->den_plan, s);
      m.den_ell_c.upload(m.den_host->den_ell_c, s); m.den_long_c.upload(m.den_host->den_long_c, s);
    }
    KIN_HIP(hipStreamSynchronize(s));
    m.dev_ready = true;
  }
  if (m.den_host) return DrgPlan{m.den_plan.view(), m.den_ell_c.p, m.den_long_c.p};
  return DrgPlan{g.den_plan.view(), g.den_ell_c.p, g.den_long_c.p};
}

// The pass on the device, block by block: stage 1 (the flux sweep) writes the block's rates, the denominator launch
// den[nb][N], the importance launch the maxima per slice, folded into d_imp. d_sel: the selected species on the device (null:
// all). per_state: host rows [B][R] to download every block's values into, or null.
void ri_run(kin_network* h, int pairing, const StateBatch& b, const int64_t* d_sel, int64_t n_sel, int accumulate, double* d_imp,
            double* per_state, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  const DrgPlan den = ri_dev(h, pairing, s);
  if (R == 0 || empty_batch(b.B, d_imp, R, accumulate, s)) return;
  const int64_t nb_max = block_states((size_t)R, b.B, DRG_BLOCK_ENV);
  drg_stage_alloc(h, nb_max);
  h->ri_part.alloc((size_t)slices_cap(ri_slices(R, nb_max, h->n_cu)) * R);
  if (per_state) h->ri_state.alloc((size_t)nb_max * R);
  if (d_sel) { h->ri_mask.alloc((size_t)std::max<int64_t>(N, 1)); launch_ri_mask(n_sel, d_sel, N, h->ri_mask.p, s); }
  for_blocks(b.B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
    DrgArgs a{};
    drg_rates_den(h, b, b0, nb, den, false, 2, a, s);
    RiArgs ra{};
    ra.N = (int)N; ra.R = (int)R; ra.nb = (int)nb;
    ra.tab = h->ri[pairing ? 1 : 0].tab.p; ra.mask = d_sel ? h->ri_mask.p : nullptr;
    ra.rates = h->drg_rates.p; ra.den = h->drg_den.p;
    ra.b0 = b0; ra.seg_n = b.seg_n; ra.L = b.L;
    ra.part = h->ri_part.p; ra.per_state = per_state ? h->ri_state.p : nullptr;
    const int Y = slices_cap(ri_slices(R, nb, h->n_cu));
    launch_ri(ra, Y, s);
    launch_drg_max(R, Y, h->ri_part.p, d_imp, use_prev, s);
    if (per_state) h->ri_state.download(per_state + (size_t)b0 * R, (size_t)nb * R, s);
  });
}

// host entries: the species list (null: all species) behind the batch, importance staged through the handle
void ri_host_call(kin_network* h, int pairing, const StateBatch& b, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                  double* importance, double* per_state, hipStream_t s) {
  const int64_t* d_sel =
      species ? species_list(h, species, n_sel, index_base, "a species list needs at least one entry", "species out of range", s) : nullptr;
  staged_result(h, h->host.R, importance, accumulate, s,
                [&](double* d_imp) { ri_run(h, pairing, b, d_sel, n_sel, accumulate, d_imp, per_state, s); });
}

}  // namespace

extern "C" {

int kin_drg_pattern(kin_network* h, int pairing, int index_base, int64_t* nnz, int64_t* rowptr, int64_t* colidx) {
  if (!h) return KIN_ERR_INVALID_ARG;
  try {     // (host tables only: no device call)
    const DrgTables& t = drg_host(h, pairing);
    if (nnz) *nnz = t.E;
    if (rowptr) for (int64_t i = 0; i <= t.N; i++) rowptr[i] = t.rowptr[i] + index_base;
    if (colidx) for (int64_t e = 0; e < t.E; e++) colidx[e] = t.colidx[e] + index_base;
  } catch (const KinError& e) { h->err = e.what(); return e.code; }
  catch (const std::exception& e) { h->err = e.what(); return KIN_ERR_INVALID_ARG; }
  return KIN_OK;
}

int kin_drg_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                        const double* d_T, int accumulate, double* d_coef, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_coef != nullptr);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  drg_run(h, pairing, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, accumulate, d_coef, s);
  KIN_CATCH(h)
}

int kin_drg_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, coef != nullptr);
  hipStream_t s = h->stream;
  drg_host_call(h, pairing, host_batch(h, B, u, k, n_k_rows, k_row, T, s), accumulate, coef, s);
  KIN_CATCH(h)
}

int kin_solution_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  drg_host_call(h, pairing, solution_batch(h, drg_check, k, n_k_rows, k_row, T_rows, coef != nullptr, s), accumulate, coef, s);
  KIN_CATCH(h)
}

int kin_ensemble_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  drg_host_call(h, pairing, ensemble_batch(h, drg_check, k, n_k_rows, k_row, T_rows, coef != nullptr, s), accumulate, coef, s);
  KIN_CATCH(h)
}

int kin_reaction_importance_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                                        const double* d_T, const int64_t* d_species, int64_t n_sel, int accumulate, double* d_importance,
                                        void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_importance != nullptr);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  require(d_species == nullptr || (n_sel >= 1 && n_sel < ((int64_t)1 << 31)), ERR_INVALID_ARG, "a species list needs at least one entry");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  ri_run(h, pairing, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, d_species, n_sel, accumulate, d_importance,
         nullptr, s);
  KIN_CATCH(h)
}

int kin_reaction_importance_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows,
                                    const int64_t* k_row, const double* T, const int64_t* species, int64_t n_sel, int index_base,
                                    int accumulate, double* importance, double* per_state) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, importance != nullptr);
  hipStream_t s = h->stream;
  ri_host_call(h, pairing, host_batch(h, B, u, k, n_k_rows, k_row, T, s), species, n_sel, index_base, accumulate, importance, per_state, s);
  KIN_CATCH(h)
}

int kin_solution_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row,
                                     const double* T_rows, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                                     double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  ri_host_call(h, pairing, solution_batch(h, drg_check, k, n_k_rows, k_row, T_rows, importance != nullptr, s), species, n_sel, index_base,
               accumulate, importance, nullptr, s);
  KIN_CATCH(h)
}

int kin_ensemble_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row,
                                     const double* T_rows, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                                     double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  ri_host_call(h, pairing, ensemble_batch(h, drg_check, k, n_k_rows, k_row, T_rows, importance != nullptr, s), species, n_sel, index_base,
               accumulate, importance, nullptr, s);
  KIN_CATCH(h)
}

}  // extern "C"
