// extern "C" entry points of the reaction-flux pass (declarations: include/kinetica_hip.h; kernels: flux_kernels.hip), and
// the batch-of-states layer every analysis pass's host side is written with (flux_api.hpp).
#include "../../include/kinetica_hip.h"

#include <algorithm>

#include "flux_api.hpp"
#include "flux_kernels.hpp"

using namespace kin;

namespace kin {

// checks shared by the three entry points (have_k: a rate-constant array or, for kin_solution_flux, the resident table)
void flux_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out) {
  require(B >= 0, ERR_INVALID_ARG, "B < 0");
  require(have_out, ERR_INVALID_ARG, "neither flux nor rates requested");
  require(!(have_k && have_T), ERR_INVALID_ARG, "give rate constants or temperatures, not both");
  require(!have_row || have_k, ERR_INVALID_ARG, "k_row given without rate constants to index");
  require(!have_T || h->has_arrhenius, ERR_STATE, "temperatures given but Arrhenius parameters were never set");
  require(have_k || have_T || h->has_rates, ERR_STATE, "rates were never set and neither k nor T given");
  require(h->host.R < ((int64_t)1 << 28) && B < ((int64_t)1 << 31), ERR_UNSUPPORTED, "flux pass: B or R beyond 32-bit offsets");
}

// the index tables of both passes: uploaded at the first call that needs them
static void ensure_flux_tables(kin_network* h, hipStream_t s) {
  if (h->flux_ready) return;
  const FluxTables t = build_flux_tables(h->host);
  if (!t.idx16.empty()) h->flux_idx16.upload(t.idx16, s);
  h->flux_idx32.upload(t.idx32, s);
  KIN_HIP(hipStreamSynchronize(s));   // the host vectors die here
  h->flux_ready = true;
}

// The pass itself on device buffers: grows the handle's workspace (may allocate when B or the plan grows), then enqueues.
void flux_run(kin_network* h, int64_t B, const double* d_u, const FluxSource& src, const double* d_w, double* d_flux,
              double* d_rates, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  if (B == 0 || R == 0) {
    if (d_flux && R > 0) KIN_HIP(hipMemsetAsync(d_flux, 0, (size_t)R * sizeof(double), s));
    return;
  }
  ensure_flux_tables(h, s);
  if (!src.k && !src.T) h->flush_pending_T(s);   // the handle's own k is about to be read
  const FluxPlan plan = flux_plan(B, R, N, h->n_cu, src.T != nullptr, (reinterpret_cast<uintptr_t>(d_u) & 15) == 0);
  if (d_flux) h->flux_part.alloc((size_t)plan.G * (size_t)R);
  FluxArgs a{};
  a.N = (int)N; a.R = (int)R; a.P = (int)((R + 1) / 2); a.B = (int)B;
  a.idx16 = reinterpret_cast<const uint2*>(h->flux_idx16.p);
  a.idx32 = reinterpret_cast<const int4*>(h->flux_idx32.p);
  a.u = d_u;
  if (src.T) a.T = src.T;
  else if (src.k) { a.k = src.k; a.k_stride = src.k_stride; a.k_row = src.k_row; }
  else { a.k = h->k.p; a.k_stride = 0; a.k_row = nullptr; }
  a.Ea = h->Ea.p; a.A = h->A.p; a.has_kmax = h->has_kmax ? 1 : 0; a.k_max = h->k_max; a.t_mult = h->t_mult;
  a.w = d_w;
  a.part = d_flux ? h->flux_part.p : nullptr;
  a.rates = d_rates;
  launch_flux_sweep(plan, a, s);
  if (d_flux) launch_flux_reduce(R, plan.G, h->flux_part.p, d_flux, s);
}

void flux_check_rows(const int64_t* k_row, int64_t B, int64_t n_rows) {
  for (int64_t b = 0; b < B; b++) require(k_row[b] >= 0 && k_row[b] < n_rows, ERR_INVALID_ARG, "k_row: row index out of range");
}

void drg_limit(const kin_network* h) {
  require(h->host.N < ((int64_t)1 << 31) / 2, ERR_UNSUPPORTED, "DRG pass: N beyond 32-bit offsets");
}

void drg_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out) {
  flux_check(h, B, have_k, have_row, have_T, true);
  require(have_out, ERR_INVALID_ARG, "null output buffer");
  drg_limit(h);
}

FluxSource stage_source(kin_network* h, int64_t B, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T, hipStream_t s) {
  const int64_t R = h->host.R;
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row && B > 0) h->f_krow.upload(k_row, (size_t)B, s);
  if (T && B > 0) h->f_T.upload(T, (size_t)B, s);
  return FluxSource{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T ? h->f_T.p : nullptr};
}

StateBatch host_batch(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T, hipStream_t s) {
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); flux_check_rows(k_row, B, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == B)");
  if (B > 0) h->f_u.upload(u, (size_t)B * h->host.N, s);
  return StateBatch{B, h->f_u.p, stage_source(h, B, k, n_k_rows, k_row, T, s), nullptr, 0};
}

StateBatch solution_batch(kin_network* h, PassCheck check, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T_rows, bool have_out, hipStream_t s) {
  const int64_t B = h->n_saved;
  const bool table = !k && k_row;    // rows of the device-resident rate table
  check(h, B, k != nullptr || table, k_row != nullptr, T_rows != nullptr, have_out);
  require(B > 0, ERR_STATE, "no solution stored");
  require(!table || h->table_rows > 0, ERR_STATE, "no rate table resident (kin_rate_table / kin_solve with a table first)");
  if (k_row) flux_check_rows(k_row, B, table ? h->table_rows : n_k_rows);
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per saved state (n_k_rows == n_saved)");
  FluxSource src = stage_source(h, B, k, n_k_rows, k_row, T_rows, s);
  if (table) src.k = h->table.p;
  return StateBatch{B, h->d_sol_u.p, src, nullptr, 0};
}

StateBatch ensemble_batch(kin_network* h, PassCheck check, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T_rows, bool have_out, hipStream_t s) {
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  require(h->ens.observables == 0, ERR_STATE, OBSERVABLES_RECORD_MSG);
  const int64_t K = h->ens.K, cap = h->ens.cap, B = K * cap;
  require(cap < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && B < ((int64_t)1 << 31), ERR_UNSUPPORTED,
          "ensemble DRG pass: K n_rows beyond 32-bit offsets");
  check(h, B, k != nullptr, k_row != nullptr, T_rows != nullptr, have_out);
  // stage 1 forms the rate constants of all K n_rows states in one unsegmented pass from the handle's one (Ea, A)
  require(!(T_rows && h->ens.member_params()), ERR_UNSUPPORTED,
          "the stored ensemble was solved with per-member Arrhenius parameters: T_rows would use the handle's; give the rate "
          "constants explicitly (k with k_row, one kin_arrhenius_eval row per member and temperature)");
  if (k && k_row) require(n_k_rows >= 1, ERR_INVALID_ARG, "k has no rows");
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per saved row (n_k_rows == K n_rows)");
  // Stage 1 runs over every row of the record; the keys of the rows past a member's saved ones are ignored by contract, so
  // they are replaced by harmless ones here (row 0, 1000 K) and the later stages leave those states out.
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
  const FluxSource src = stage_source(h, B, k, n_k_rows, k_row ? rows.data() : nullptr, T_rows ? Ts.data() : nullptr, s);
  KIN_HIP(hipStreamSynchronize(s));      // (rows and Ts leave scope)
  return StateBatch{B, h->ens.sol, src, h->ens_segn.p, cap};
}

const int64_t* species_list(kin_network* h, const int64_t* list, int64_t n, int index_base, const char* none_msg, const char* range_msg,
                            hipStream_t s) {
  require(list != nullptr && n >= 1 && n < ((int64_t)1 << 31), ERR_INVALID_ARG, none_msg);
  std::vector<int64_t> t(list, list + n);
  for (int64_t& x : t) {
    x -= index_base;
    require(x >= 0 && x < h->host.N, ERR_INVALID_ARG, range_msg);
  }
  h->f_sel.upload(t, s);
  KIN_HIP(hipStreamSynchronize(s));      // (t leaves scope)
  return h->f_sel.p;
}

}  // namespace kin

namespace {

// The segmented pass on device buffers (kin_flux_segmented*, kin_ensemble_flux): ONE launch that writes d_flux[S][R] itself.
// member_Ea / member_A: per-segment Arrhenius parameters [S][R] for the temperature form (a per-member ensemble record); null:
// the handle's own
void flux_seg_run(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const FluxSource& src,
                  const double* d_w, double* d_flux, hipStream_t s, const double* member_Ea = nullptr, const double* member_A = nullptr) {
  const int64_t N = h->host.N, R = h->host.R;
  if (S * L == 0 || R == 0) {
    if (S * R > 0) KIN_HIP(hipMemsetAsync(d_flux, 0, (size_t)S * (size_t)R * sizeof(double), s));
    return;
  }
  ensure_flux_tables(h, s);
  if (!src.k && !src.T) h->flush_pending_T(s);   // the handle's own k is about to be read
  // (every row of a segment must be aligned for path 0: the base and, N being even there, every row behind it)
  const FluxPlan plan = flux_plan(S * L, R, N, h->n_cu, src.T != nullptr, (reinterpret_cast<uintptr_t>(d_u) & 15) == 0, FLUX_SEG_MAX_ROWS);
  FluxSegArgs a{};
  a.N = (int)N; a.R = (int)R; a.P = (int)((R + 1) / 2); a.S = S; a.L = L;
  a.seg_n = d_seg_n;
  a.idx16 = reinterpret_cast<const uint2*>(h->flux_idx16.p);
  a.idx32 = reinterpret_cast<const int4*>(h->flux_idx32.p);
  a.u = d_u;
  if (src.T) a.T = src.T;
  else if (src.k) { a.k = src.k; a.k_stride = src.k_stride; a.k_row = src.k_row; }
  else { a.k = h->k.p; a.k_stride = 0; a.k_row = nullptr; }
  a.Ea = h->Ea.p; a.A = h->A.p; a.has_kmax = h->has_kmax ? 1 : 0; a.k_max = h->k_max; a.t_mult = h->t_mult;
  if (member_Ea) { a.Ea = member_Ea; a.A = member_A; a.par_stride = R; }
  a.w = d_w;
  a.flux = d_flux;
  launch_flux_seg(plan, a, s);
}

void flux_seg_check(kin_network* h, int64_t S, int64_t L, bool have_k, bool have_row, bool have_T, bool have_out) {
  require(S >= 0 && L >= 0, ERR_INVALID_ARG, "S or L < 0");
  require(have_out, ERR_INVALID_ARG, "null output buffer");
  require(L < ((int64_t)1 << 31) && S < ((int64_t)1 << 31) && S * L < ((int64_t)1 << 31), ERR_UNSUPPORTED,
          "segmented flux pass: S L beyond 32-bit offsets");
  flux_check(h, S * L, have_k, have_row, have_T, true);
}

// host-side checks of per-state keys: only the rows a segment really has are looked at
void check_seg_rows(const int64_t* k_row, int64_t S, int64_t L, const int64_t* seg_n, int64_t n_rows) {
  for (int64_t s = 0; s < S; s++) {
    const int64_t n = seg_n ? seg_n[s] : L;
    for (int64_t j = 0; j < n; j++)
      require(k_row[s * L + j] >= 0 && k_row[s * L + j] < n_rows, ERR_INVALID_ARG, "k_row: row index out of range");
  }
}

// the unsegmented host entries: weights up, flux[R] and / or rates[B][R] staged through the handle's buffers
void flux_host_call(kin_network* h, const StateBatch& b, const double* w, double* flux, double* rates, hipStream_t s) {
  const size_t R = (size_t)h->host.R;
  if (w && b.B > 0) h->f_w.upload(w, (size_t)b.B, s);
  if (flux) h->f_flux.alloc(R);
  if (rates) h->f_rates.alloc((size_t)b.B * R);
  flux_run(h, b.B, b.u, b.src, w ? h->f_w.p : nullptr, flux ? h->f_flux.p : nullptr, rates ? h->f_rates.p : nullptr, s);
  if (flux) h->f_flux.download(flux, R, s);
  if (rates) h->f_rates.download(rates, (size_t)b.B * R, s);
  KIN_HIP(hipStreamSynchronize(s));
}

void require_ensemble(const kin_network* h) {
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
}

}  // namespace

extern "C" {

int kin_flux_plan_host(int64_t n_species, int64_t n_reactions, int64_t B, int n_cu, int temperature_form, int segmented,
                       int64_t k_stride, int u_bits, int k_bits, int rates_bits, int64_t* info) {
  if (!info || n_species < 1 || n_reactions < 1 || B < 1 || n_cu < 1 || u_bits < 0 || u_bits > 15 || k_bits < 0 || k_bits > 15 ||
      rates_bits > 15 || (segmented && rates_bits >= 0))
    return KIN_ERR_INVALID_ARG;
  // exactly what flux_run / flux_seg_run ask for
  const FluxPlan p = flux_plan(B, n_reactions, n_species, n_cu, temperature_form != 0, u_bits == 0, segmented ? FLUX_SEG_MAX_ROWS : 8);
  const FluxModes m = flux_modes(n_reactions, temperature_form != 0, k_stride, (unsigned)k_bits, rates_bits >= 0,
                                 rates_bits >= 0 ? (unsigned)rates_bits : 0u);
  info[0] = p.path; info[1] = p.rows; info[2] = p.parts; info[3] = p.G; info[4] = m.k_mode; info[5] = m.rates_mode;
  return KIN_OK;
}

int kin_flux_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                         const double* d_w, double* d_flux, double* d_rates, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  flux_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_flux || d_rates);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  flux_run(h, B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, d_w, d_flux, d_rates, s);
  KIN_CATCH(h)
}

int kin_flux_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                     const double* T, const double* w, double* flux, double* rates) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  flux_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, flux || rates);
  hipStream_t s = h->stream;
  flux_host_call(h, host_batch(h, B, u, k, n_k_rows, k_row, T, s), w, flux, rates, s);
  KIN_CATCH(h)
}

int kin_solution_flux(kin_network* h, const double* w, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T_rows, double* flux, double* rates) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  flux_host_call(h, solution_batch(h, flux_check, k, n_k_rows, k_row, T_rows, flux || rates, s), w, flux, rates, s);
  KIN_CATCH(h)
}

int kin_flux_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const double* d_k,
                           const int64_t* d_k_row, const double* d_T, const double* d_w, double* d_flux, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  flux_seg_check(h, S, L, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_flux != nullptr);
  require(d_u != nullptr || S * L == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  flux_seg_run(h, S, L, d_seg_n, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, d_w, d_flux, s);
  KIN_CATCH(h)
}

int kin_flux_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* k, int64_t n_k_rows,
                       const int64_t* k_row, const double* T, const double* w, double* flux) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  flux_seg_check(h, S, L, k != nullptr, k_row != nullptr, T != nullptr, flux != nullptr);
  const int64_t B = S * L, N = h->host.N, R = h->host.R;
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (seg_n) for (int64_t i = 0; i < S; i++) require(seg_n[i] >= 0 && seg_n[i] <= L, ERR_INVALID_ARG, "seg_n outside [0, L]");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); check_seg_rows(k_row, S, L, seg_n, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == S L)");
  hipStream_t s = h->stream;
  if (B > 0) h->f_u.upload(u, (size_t)B * N, s);
  if (seg_n && S > 0) h->f_segn.upload(seg_n, (size_t)S, s);
  const FluxSource src = stage_source(h, B, k, n_k_rows, k_row, T, s);
  if (w && B > 0) h->f_w.upload(w, (size_t)B, s);
  h->f_flux.alloc((size_t)S * R);
  flux_seg_run(h, S, L, seg_n ? h->f_segn.p : nullptr, h->f_u.p, src, w ? h->f_w.p : nullptr, h->f_flux.p, s);
  h->f_flux.download(flux, (size_t)S * R, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_ensemble_size(const kin_network* h, int64_t* K, int64_t* n_rows, int64_t* n_species, int64_t* n_saved) {
  if (!h) return KIN_ERR_INVALID_ARG;
  if (!h->ens.valid()) {
    const_cast<kin_network*>(h)->err = "no ensemble stored (kin_solve_ensemble* first)";
    return KIN_ERR_STATE;
  }
  if (K) *K = h->ens.K;
  if (n_rows) *n_rows = h->ens.cap;
  if (n_species) *n_species = h->host.N;
  if (n_saved) std::copy(h->ens.n_saved.begin(), h->ens.n_saved.end(), n_saved);
  return KIN_OK;
}

int kin_ensemble_max(kin_network* h, double* out_umax) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out_umax != nullptr, ERR_INVALID_ARG, "null output buffer");
  require_ensemble(h);
  const int64_t K = h->ens.K, N = h->host.N;
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  h->ens_out.alloc((size_t)K * N);
  launch_seg_max((int)N, K, h->ens.cap, h->ens_segn.p, h->ens.sol, h->ens_out.p, s);
  h->ens_out.download(out_umax, (size_t)K * N, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_ensemble_dot(kin_network* h, const double* w, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(w && out, ERR_INVALID_ARG, "null buffer");
  require_ensemble(h);
  const int64_t K = h->ens.K, N = h->host.N, cap = h->ens.cap;
  require(K * cap < ((int64_t)1 << 31), ERR_UNSUPPORTED, "ensemble dot: K n_rows beyond 32-bit offsets");
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  h->ens_w.upload(w, (size_t)N, s);
  h->ens_out.alloc((size_t)K * cap);
  launch_seg_dot((int)N, K, cap, h->ens_segn.p, h->ens.sol, h->ens_w.p, h->ens_out.p, s);
  h->ens_out.download(out, (size_t)K * cap, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_ensemble_flux(kin_network* h, const double* w, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                      double* flux) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(flux != nullptr, ERR_INVALID_ARG, "null output buffer");
  require_ensemble(h);
  require(h->ens.observables == 0, ERR_STATE, OBSERVABLES_RECORD_MSG);
  const int64_t K = h->ens.K, cap = h->ens.cap, B = K * cap, R = h->host.R;
  flux_seg_check(h, K, cap, k != nullptr, k_row != nullptr, T_rows != nullptr, true);
  if (k && k_row) { require(n_k_rows >= 1, ERR_INVALID_ARG, "k has no rows"); check_seg_rows(k_row, K, cap, h->ens.n_saved.data(), n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per saved row (n_k_rows == K n_rows)");
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  const FluxSource src = stage_source(h, B, k, n_k_rows, k_row, T_rows, s);
  if (w) h->f_w.upload(w, (size_t)B, s);
  h->f_flux.alloc((size_t)K * R);
  // (T_rows is not refused on a per-member record as ensemble_batch refuses it: this pass takes each member's own Ea / A)
  flux_seg_run(h, K, cap, h->ens_segn.p, h->ens.sol, src, w ? h->f_w.p : nullptr, h->f_flux.p, s, h->ens.Ea, h->ens.A);
  h->f_flux.download(flux, (size_t)K * R, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

}  // extern "C"
