// extern "C" entry points of the directed-relation-graph pass (declarations: include/kinetica_hip.h; tables: drg.cpp;
// kernels: drg_kernels.hip) and of the reaction-importance pass, which runs that pass's first two stages (kernel:
// reaction_importance_kernels.hip). kin_drg_pattern_host and kin_reaction_importance_plan_host, which need no handle, sit with the
// other host-only entries in capi.cpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cstdlib>

#include "drg_api.hpp"
#include "handle.hpp"

using namespace kin;

namespace {

void require(bool c, int code, const char* msg) {
  if (!c) throw KinError(code, msg);
}

}  // namespace

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

}  // namespace kin

namespace {

// The pass on device buffers. States b0, b0 + nb, ... are taken block by block: stage 1 (the flux sweep) writes the block's
// rates, stage 2 its denominators and the maxima of the ratios, folded into d_coef. seg_n / L: see DrgArgs.
void drg_run(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
             int accumulate, double* d_coef, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  auto& m = drg_dev(h, pairing, s);
  const int64_t E = m.host->E;
  if (E == 0) return;
  if (B == 0) {
    if (!accumulate) KIN_HIP(hipMemsetAsync(d_coef, 0, (size_t)E * sizeof(double), s));
    return;
  }
  int64_t nb_max = std::max<int64_t>(1, (int64_t)(DRG_RATES_BYTES / ((size_t)R * sizeof(double))));
  if (const char* e = getenv("KIN_DRG_BLOCK_STATES")) {   // (read per call: tests change it)
    const int64_t v = atoll(e);
    if (v >= 1) nb_max = std::min(nb_max, v);
  }
  nb_max = std::min(nb_max, B);
  h->drg_rates.alloc((size_t)nb_max * R);
  h->drg_den.alloc((size_t)nb_max * N);
  const SegPlanView dv = m.den_plan.view(), ev = m.edge_plan.view();
  const int Ye_max = slices_cap(drg_slices(ev, nb_max, h->n_cu));
  h->drg_part.alloc((size_t)Ye_max * E);
  for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
    const int64_t nb = std::min(nb_max, B - b0);
    FluxSource bs = src;
    if (bs.k && !bs.k_row) bs.k += (size_t)b0 * (size_t)bs.k_stride;
    if (bs.k_row) bs.k_row += b0;
    if (bs.T) bs.T += b0;
    flux_run(h, nb, d_u + (size_t)b0 * N, bs, nullptr, nullptr, h->drg_rates.p, s);
    DrgArgs a{};
    a.N = (int)N; a.R = (int)R; a.E = (int)E; a.nb = (int)nb;
    a.rates = h->drg_rates.p; a.b0 = b0; a.seg_n = d_seg_n; a.L = L;
    a.den = h->drg_den.p; a.part = h->drg_part.p;
    a.p = dv; a.ell_c = m.den_ell_c.p; a.long_c = m.den_long_c.p;
    launch_drg_den(a, slices_cap(drg_slices(dv, nb, h->n_cu)), s);
    a.p = ev; a.ell_c = m.edge_ell_c.p; a.long_c = m.edge_long_c.p;
    const int Ye = slices_cap(drg_slices(ev, nb, h->n_cu));
    launch_drg_edges(a, Ye, s);
    launch_drg_max(E, Ye, h->drg_part.p, d_coef, (accumulate || b0 > 0) ? 1 : 0, s);
  }
}

// ---- reaction importance ------------------------------------------------------------------------------------------------
RiTables& ri_host(kin_network* h, int pairing) {
  auto& m = h->ri[pairing ? 1 : 0];
  if (!m.host) m.host = std::make_unique<RiTables>(build_ri_tables(h->host, pairing));
  return *m.host;
}

// the denominator plan of a pairing mode on the device: the DRG pass's when that has been uploaded, else one built without edges
struct RiDen { SegPlanView p; const float* ell_c; const float* long_c; };
RiDen ri_dev(kin_network* h, int pairing, hipStream_t s) {
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
  if (m.den_host) return RiDen{m.den_plan.view(), m.den_ell_c.p, m.den_long_c.p};
  return RiDen{g.den_plan.view(), g.den_ell_c.p, g.den_long_c.p};
}

// The pass on device buffers, block by block: stage 1 (the flux sweep) writes the block's rates, the denominator launch
// den[nb][N], the importance launch the maxima per slice, folded into d_imp. d_sel: the selected species on the device (null:
// all). per_state: host rows [B][R] to download every block's values into, or null. seg_n / L: see DrgArgs.
void ri_run(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
            const int64_t* d_sel, int64_t n_sel, int accumulate, double* d_imp, double* per_state, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  const RiDen dn = ri_dev(h, pairing, s);
  if (R == 0) return;
  if (B == 0) {
    if (!accumulate) KIN_HIP(hipMemsetAsync(d_imp, 0, (size_t)R * sizeof(double), s));
    return;
  }
  int64_t nb_max = std::max<int64_t>(1, (int64_t)(DRG_RATES_BYTES / ((size_t)R * sizeof(double))));
  if (const char* e = getenv("KIN_DRG_BLOCK_STATES")) {   // (read per call: tests change it)
    const int64_t v = atoll(e);
    if (v >= 1) nb_max = std::min(nb_max, v);
  }
  nb_max = std::min(nb_max, B);
  h->drg_rates.alloc((size_t)nb_max * R);
  h->drg_den.alloc((size_t)nb_max * N);
  h->ri_part.alloc((size_t)slices_cap(ri_slices(R, nb_max, h->n_cu)) * R);
  if (per_state) h->ri_state.alloc((size_t)nb_max * R);
  if (d_sel) { h->ri_mask.alloc((size_t)std::max<int64_t>(N, 1)); launch_ri_mask(n_sel, d_sel, N, h->ri_mask.p, s); }
  for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
    const int64_t nb = std::min(nb_max, B - b0);
    FluxSource bs = src;
    if (bs.k && !bs.k_row) bs.k += (size_t)b0 * (size_t)bs.k_stride;
    if (bs.k_row) bs.k_row += b0;
    if (bs.T) bs.T += b0;
    flux_run(h, nb, d_u + (size_t)b0 * N, bs, nullptr, nullptr, h->drg_rates.p, s);
    DrgArgs a{};
    a.N = (int)N; a.R = (int)R; a.E = 0; a.nb = (int)nb;
    a.rates = h->drg_rates.p; a.b0 = b0; a.seg_n = d_seg_n; a.L = L;
    a.den = h->drg_den.p;
    a.p = dn.p; a.ell_c = dn.ell_c; a.long_c = dn.long_c;
    launch_drg_den(a, slices_cap(drg_slices(dn.p, nb, h->n_cu)), s);
    RiArgs ra{};
    ra.N = (int)N; ra.R = (int)R; ra.nb = (int)nb;
    ra.tab = h->ri[pairing ? 1 : 0].tab.p; ra.mask = d_sel ? h->ri_mask.p : nullptr;
    ra.rates = h->drg_rates.p; ra.den = h->drg_den.p;
    ra.b0 = b0; ra.seg_n = d_seg_n; ra.L = L;
    ra.part = h->ri_part.p; ra.per_state = per_state ? h->ri_state.p : nullptr;
    const int Y = slices_cap(ri_slices(R, nb, h->n_cu));
    launch_ri(ra, Y, s);
    launch_drg_max(R, Y, h->ri_part.p, d_imp, (accumulate || b0 > 0) ? 1 : 0, s);
    if (per_state) h->ri_state.download(per_state + (size_t)b0 * R, (size_t)nb * R, s);
  }
}

// the species list of a host entry: null = all species; else checked, made 0-based and uploaded
const int64_t* ri_species(kin_network* h, const int64_t* species, int64_t n_sel, int index_base, hipStream_t s) {
  if (!species) return nullptr;
  require(n_sel >= 1 && n_sel < ((int64_t)1 << 31), ERR_INVALID_ARG, "a species list needs at least one entry");
  std::vector<int64_t> t(species, species + n_sel);
  for (int64_t& x : t) {
    x -= index_base;
    require(x >= 0 && x < h->host.N, ERR_INVALID_ARG, "species out of range");
  }
  h->ri_sel.upload(t, s);
  KIN_HIP(hipStreamSynchronize(s));      // (t leaves scope)
  return h->ri_sel.p;
}

// host entries: importance staged through the handle's buffer (uploaded first when it takes part in the maximum)
void ri_host_call(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
                  const int64_t* d_sel, int64_t n_sel, int accumulate, double* importance, double* per_state, hipStream_t s) {
  const int64_t R = h->host.R;
  h->ri_imp.alloc((size_t)R);
  if (accumulate && R > 0) h->ri_imp.upload(importance, (size_t)R, s);
  ri_run(h, pairing, B, d_u, src, d_seg_n, L, d_sel, n_sel, accumulate, h->ri_imp.p, per_state, s);
  if (R > 0) h->ri_imp.download(importance, (size_t)R, s);
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

namespace kin {

void drg_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out) {
  flux_check(h, B, have_k, have_row, have_T, true);
  require(have_out, ERR_INVALID_ARG, "null output buffer");
  require(h->host.N < ((int64_t)1 << 31) / 2, ERR_UNSUPPORTED, "DRG pass: N beyond 32-bit offsets");
}

FluxSource drg_solution_source(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                               bool have_out, hipStream_t s) {
  const int64_t B = h->n_saved, R = h->host.R;
  const bool table = !k && k_row;    // rows of the device-resident rate table
  drg_check(h, B, k != nullptr || table, k_row != nullptr, T_rows != nullptr, have_out);
  require(B > 0, ERR_STATE, "no solution stored");
  require(!table || h->table_rows > 0, ERR_STATE, "no rate table resident (kin_rate_table / kin_solve with a table first)");
  if (k_row) flux_check_rows(k_row, B, table ? h->table_rows : n_k_rows);
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per saved state (n_k_rows == n_saved)");
  if (k) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row) h->f_krow.upload(k_row, (size_t)B, s);
  if (T_rows) h->f_T.upload(T_rows, (size_t)B, s);
  const double* ksrc = k ? h->f_k.p : (table ? h->table.p : nullptr);
  return FluxSource{ksrc, R, k_row ? h->f_krow.p : nullptr, T_rows ? h->f_T.p : nullptr};
}

FluxSource drg_ensemble_source(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                               bool have_out, hipStream_t s) {
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  const int64_t K = h->ens.K, cap = h->ens.cap, B = K * cap, R = h->host.R;
  require(cap < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && B < ((int64_t)1 << 31), ERR_UNSUPPORTED,
          "ensemble DRG pass: K n_rows beyond 32-bit offsets");
  drg_check(h, B, k != nullptr, k_row != nullptr, T_rows != nullptr, have_out);
  // stage 1 forms the rate constants of all K n_rows states in one unsegmented pass from the handle's one (Ea, A)
  require(!(T_rows && h->ens.member_params()), ERR_UNSUPPORTED,
          "the stored ensemble was solved with per-member Arrhenius parameters: T_rows would use the handle's; give the rate "
          "constants explicitly (k with k_row, one kin_arrhenius_eval row per member and temperature)");
  if (k && k_row) require(n_k_rows >= 1, ERR_INVALID_ARG, "k has no rows");
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per saved row (n_k_rows == K n_rows)");
  // Stage 1 runs over every row of the record; the keys of the rows past a member's saved ones are ignored by contract, so
  // they are replaced by harmless ones here (row 0, 1000 K) and stage 2 leaves those states out.
  std::vector<int64_t> rows;
  std::vector<double> Ts;
  if (k_row) rows.assign(k_row, k_row + B);
  if (T_rows) Ts.assign(T_rows, T_rows + B);
  for (int64_t m = 0; m < K; m++) {
    const int64_t n = h->ens.n_saved[m];
    for (int64_t j = 0; j < cap; j++) {
      const int64_t b = m * cap + j;
      if (j < n) { if (k_row) require(rows[b] >= 0 && rows[b] < n_k_rows, ERR_INVALID_ARG, "k_row: row index out of range"); }
      else { if (k_row) rows[b] = 0; if (T_rows) Ts[b] = 1000.0; }
    }
  }
  h->ens_segn.upload(h->ens.n_saved, s);
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row) h->f_krow.upload(rows, s);
  if (T_rows) h->f_T.upload(Ts, s);
  KIN_HIP(hipStreamSynchronize(s));      // (rows and Ts leave scope)
  return FluxSource{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T_rows ? h->f_T.p : nullptr};
}

}  // namespace kin

namespace {

// host entries: coef staged through the handle's buffer (uploaded first when it takes part in the maximum)
void drg_host_call(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
                   int accumulate, double* coef, hipStream_t s) {
  const int64_t E = drg_host(h, pairing).E;
  h->drg_coef.alloc((size_t)E);
  if (accumulate && E > 0) h->drg_coef.upload(coef, (size_t)E, s);
  drg_run(h, pairing, B, d_u, src, d_seg_n, L, accumulate, h->drg_coef.p, s);
  if (E > 0) h->drg_coef.download(coef, (size_t)E, s);
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

#define KIN_TRY(h) try { KIN_HIP(hipSetDevice((h)->device));
#define KIN_CATCH(h)                                                        \
  }                                                                         \
  catch (const KinError& e) { (h)->err = e.what(); return e.code; }         \
  catch (const std::exception& e) { (h)->err = e.what(); return KIN_ERR_DEVICE; } \
  return KIN_OK;

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
  drg_run(h, pairing, B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0, accumulate, d_coef, s);
  KIN_CATCH(h)
}

int kin_drg_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, coef != nullptr);
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); flux_check_rows(k_row, B, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == B)");
  const int64_t N = h->host.N, R = h->host.R;
  hipStream_t s = h->stream;
  if (B > 0) h->f_u.upload(u, (size_t)B * N, s);
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row && B > 0) h->f_krow.upload(k_row, (size_t)B, s);
  if (T && B > 0) h->f_T.upload(T, (size_t)B, s);
  drg_host_call(h, pairing, B, h->f_u.p, FluxSource{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T ? h->f_T.p : nullptr},
                nullptr, 0, accumulate, coef, s);
  KIN_CATCH(h)
}

int kin_solution_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_solution_source(h, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  drg_host_call(h, pairing, h->n_saved, h->d_sol_u.p, src, nullptr, 0, accumulate, coef, s);
  KIN_CATCH(h)
}

int kin_ensemble_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_ensemble_source(h, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  drg_host_call(h, pairing, h->ens.K * h->ens.cap, h->ens.sol, src, h->ens_segn.p, h->ens.cap, accumulate, coef, s);
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
  ri_run(h, pairing, B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0, d_species, n_sel, accumulate, d_importance, nullptr, s);
  KIN_CATCH(h)
}

int kin_reaction_importance_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows,
                                    const int64_t* k_row, const double* T, const int64_t* species, int64_t n_sel, int index_base,
                                    int accumulate, double* importance, double* per_state) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, importance != nullptr);
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); flux_check_rows(k_row, B, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == B)");
  const int64_t N = h->host.N, R = h->host.R;
  hipStream_t s = h->stream;
  const int64_t* d_sel = ri_species(h, species, n_sel, index_base, s);
  if (B > 0) h->f_u.upload(u, (size_t)B * N, s);
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row && B > 0) h->f_krow.upload(k_row, (size_t)B, s);
  if (T && B > 0) h->f_T.upload(T, (size_t)B, s);
  ri_host_call(h, pairing, B, h->f_u.p, FluxSource{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T ? h->f_T.p : nullptr},
               nullptr, 0, d_sel, n_sel, accumulate, importance, per_state, s);
  KIN_CATCH(h)
}

int kin_solution_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row,
                                     const double* T_rows, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                                     double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_solution_source(h, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  const int64_t* d_sel = ri_species(h, species, n_sel, index_base, s);
  ri_host_call(h, pairing, h->n_saved, h->d_sol_u.p, src, nullptr, 0, d_sel, n_sel, accumulate, importance, nullptr, s);
  KIN_CATCH(h)
}

int kin_ensemble_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row,
                                     const double* T_rows, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                                     double* importance) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_ensemble_source(h, k, n_k_rows, k_row, T_rows, importance != nullptr, s);
  const int64_t* d_sel = ri_species(h, species, n_sel, index_base, s);
  ri_host_call(h, pairing, h->ens.K * h->ens.cap, h->ens.sol, src, h->ens_segn.p, h->ens.cap, d_sel, n_sel, accumulate, importance,
               nullptr, s);
  KIN_CATCH(h)
}

}  // extern "C"
