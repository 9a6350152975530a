// extern "C" entry points of the timescale analysis (declarations: include/kinetica_hip.h; kernels: timescale_kernels.hip).
// Batches, blocks and staging: flux_api.hpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>

#include "flux_api.hpp"
#include "timescale.hpp"

using namespace kin;

namespace {

// which outputs a call wants (device pointers; null: not wanted)
struct TsOut { double* vals; double* summary; double* diag; double* err; double* norm; };

void ensure_ts_tables(kin_network* h, hipStream_t s) {
  if (h->ts_ready) return;
  const TsTables t = build_ts_tables(h->host);
  h->ts_rows.upload(t.rows, s);
  KIN_HIP(hipStreamSynchronize(s));   // t dies here
  h->ts_G = t.G; h->ts_S = t.S; h->ts_Bl = t.Bl;
  h->ts_ready = true;
}

// The pass on the device, block of states by block: stage 1 (rates and operand derivatives), the entry gather into the
// caller's vals or the handle's jv, and - when any of summary / diag / err / norm is wanted - the row pass with its closing
// launches. Of the batch's states those from row_begin on in their segment count (TsCount; its b0 is set per block here).
void ts_run(kin_network* h, const StateBatch& b, int64_t row_begin, int accumulate, const TsOut& o, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R, nnz = h->host.nnz(), B = b.B;
  const FluxSource& src = b.src;
  // (the passes hold the number of rows below 2^31)
  TsCount cnt{0, b.seg_n, (int32_t)b.L, (int32_t)std::min<int64_t>(row_begin, INT32_MAX)};
  if (B == 0) {
    if (o.summary && !accumulate) launch_ts_identity(N, o.summary, s);
    return;
  }
  const bool rows = o.summary || o.diag || o.err || o.norm;
  // the per-state workspace of a block: dr, rates, jv, g
  const size_t per_state = (size_t)2 * R + (rows ? (size_t)R : 0) + (o.vals ? 0 : (size_t)nnz) + (o.norm ? (size_t)N : 0);
  const int64_t nb_max = block_states(per_state, B, "KIN_TS_BLOCK_STATES");
  int stages = 3;      // KIN_TS_STAGES=1|2 ends every block after stage 1 / the entry gather: a knob for timing, never for results
  if (const char* e = getenv("KIN_TS_STAGES")) { const int v = atoi(e); if (v == 1 || v == 2) stages = v; }
  h->ts_dr.alloc((size_t)nb_max * 2 * R);
  if (rows) h->ts_rates.alloc((size_t)nb_max * R);
  if (!o.vals) h->ts_jv.alloc((size_t)nb_max * nnz);
  if (o.norm) h->ts_g.alloc((size_t)nb_max * N);
  if (rows) ensure_ts_tables(h, s);
  if (!src.k && !src.T) h->flush_pending_T(s);   // the handle's own k is about to be read
  const SegPlanView jp = h->jac_plan.view();
  TsRowArgs ra{};
  ra.N = (int)N; ra.R = (int)R; ra.nnz = (int)nnz; ra.G = h->ts_G; ra.S = h->ts_S; ra.Bl = h->ts_Bl;
  ra.rows = reinterpret_cast<const int4*>(h->ts_rows.p); ra.sp_rxn = h->sp_rxn.p; ra.sp_coef = h->sp_coef.p;
  if (o.summary) {
    ra.nb = (int)nb_max;
    h->ts_part.alloc((size_t)slices_cap(ts_row_slices(ra, h->n_cu)) * 3 * N);
  }
  for_blocks(B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
    cnt.b0 = (int32_t)b0;
    TsRateArgs q{};
    q.N = (int)N; q.R = (int)R; q.nb = (int)nb; q.x0 = h->x0.p; q.x1 = h->x1.p; q.u = b.u + (size_t)b0 * N;
    const FluxSource bs = src.at(b0);
    if (bs.T) q.T = bs.T;
    else if (bs.k) { q.k = bs.k; q.k_stride = bs.k_stride; q.k_row = bs.k_row; }
    else { q.k = h->k.p; q.k_stride = 0; q.k_row = nullptr; }
    q.Ea = h->Ea.p; q.A = h->A.p; q.has_kmax = h->has_kmax ? 1 : 0; q.k_max = h->k_max; q.t_mult = h->t_mult;
    q.rates = rows ? h->ts_rates.p : nullptr; q.dr = h->ts_dr.p;
    launch_ts_rates(q, s);
    if (stages == 1) return;
    TsEntryArgs ea{};
    ea.p = jp; ea.R = (int)R; ea.nb = (int)nb; ea.nnz = nnz; ea.dr = h->ts_dr.p;
    ea.jv = o.vals ? o.vals + (size_t)b0 * nnz : h->ts_jv.p; ea.cnt = cnt;
    launch_ts_entries(ea, slices_cap(ts_entry_slices(jp, nb, h->n_cu)), s);
    if (!rows || stages == 2) return;
    ra.nb = (int)nb; ra.jv = ea.jv; ra.rates = h->ts_rates.p; ra.cnt = cnt;
    ra.part = o.summary ? h->ts_part.p : nullptr; ra.g = o.norm ? h->ts_g.p : nullptr;
    ra.diag = o.diag ? o.diag + (size_t)b0 * N : nullptr; ra.err = o.err ? o.err + (size_t)b0 * N : nullptr;
    const int Y = slices_cap(ts_row_slices(ra, h->n_cu));
    launch_ts_rows(ra, Y, s);
    if (o.summary) launch_ts_fold(N, Y, h->ts_part.p, o.summary, use_prev, s);
    if (o.norm) launch_ts_norm(N, nb, h->ts_g.p, cnt, o.norm + b0, s);
  });
}

void ts_limits(kin_network* h) {
  require(h->host.nnz() < ((int64_t)1 << 31), ERR_UNSUPPORTED, "timescale pass: nnz beyond 32-bit offsets");
}

void ts_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out) {
  flux_check(h, B, have_k, have_row, have_T, true);
  require(have_out, ERR_INVALID_ARG, "no output requested");
  ts_limits(h);
}

// host entries of the timescale form: summary (optional, accumulating) staged through the handle as every pass's result, the
// per-state outputs through the pass's own buffers
void ts_host_call(kin_network* h, const StateBatch& b, int64_t row_begin, int accumulate, double* summary, double* diag, double* err,
                  double* norm, hipStream_t s) {
  const size_t N = (size_t)h->host.N, B = (size_t)b.B;
  staged_result(h, 3 * (int64_t)N, summary, accumulate, s, [&](double* d_summary) {
    TsOut o{};
    o.summary = d_summary;
    if (diag) { h->ts_o_diag.alloc(B * N); o.diag = h->ts_o_diag.p; }
    if (err) { h->ts_o_err.alloc(B * N); o.err = h->ts_o_err.p; }
    if (norm) { h->ts_o_norm.alloc(B); o.norm = h->ts_o_norm.p; }
    ts_run(h, b, row_begin, accumulate, o, s);
    if (diag) h->ts_o_diag.download(diag, B * N, s);
    if (err) h->ts_o_err.download(err, B * N, s);
    if (norm) h->ts_o_norm.download(norm, B, s);
  });
}

}  // namespace

namespace kin {

TsTables build_ts_tables(const NetworkHost& h) {
  TsTables t;
  t.N = h.N; t.nnz = h.nnz();
  std::vector<int32_t> shorts, medium, longs;
  for (int64_t i = 0; i < h.N; i++) {
    const int32_t len = h.j_ptr[i + 1] - h.j_ptr[i];
    if (len <= TsTables::TS_SHORT_MAX) { shorts.push_back((int32_t)i); t.cls[0]++; }
    else if (len <= TsTables::TS_WAVE_MAX) { medium.push_back((int32_t)i); t.cls[1]++; }
    else { longs.push_back((int32_t)i); t.cls[2]++; }
  }
  t.G = (int32_t)ceil_div((int64_t)shorts.size(), 64);
  shorts.resize((size_t)t.G * 64, -1);
  t.S = (int32_t)medium.size(); t.Bl = (int32_t)longs.size();
  for (const auto* list : {&shorts, &medium, &longs})
    for (int32_t i : *list) {
      if (i < 0) { t.rows.insert(t.rows.end(), {-1, 0, 0, 0, 0, 0, 0, 0}); continue; }
      t.rows.insert(t.rows.end(), {i, h.j_ptr[i], h.j_ptr[i + 1], h.j_diag[i], h.sp_ptr[i], h.sp_ptr[i + 1], 0, 0});
    }
  return t;
}

}  // namespace kin

extern "C" {

int kin_timescale_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                            const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                            int index_base, int64_t* info) {
  if (!info) return KIN_ERR_INVALID_ARG;
  try {     // (host tables only: no device call)
    const NetworkHost H = compile_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base);
    const TsTables t = build_ts_tables(H);
    info[0] = t.nnz;
    for (int c = 0; c < 3; c++) info[1 + c] = t.cls[c];
  } catch (const KinError& e) { return e.code; }
  catch (const std::exception&) { return KIN_ERR_INVALID_ARG; }
  return KIN_OK;
}

int kin_jac_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                        double* d_vals, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  ts_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_vals != nullptr);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  ts_run(h, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, 0, 0, TsOut{d_vals, nullptr, nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_jac_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T,
                    double* vals) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  ts_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, vals != nullptr);
  hipStream_t s = h->stream;
  const StateBatch b = host_batch(h, B, u, k, n_k_rows, k_row, T, s);
  const size_t n = (size_t)B * (size_t)h->host.nnz();
  h->ts_o_vals.alloc(n);
  ts_run(h, b, 0, 0, TsOut{h->ts_o_vals.p, nullptr, nullptr, nullptr, nullptr}, s);
  h->ts_o_vals.download(vals, n, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_timescale_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                              int accumulate, double* d_summary, double* d_diag, double* d_err, double* d_norm, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  ts_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_summary || d_diag || d_err || d_norm);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  ts_run(h, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, 0, accumulate,
         TsOut{nullptr, d_summary, d_diag, d_err, d_norm}, s);
  KIN_CATCH(h)
}

int kin_timescale_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T, int accumulate, double* summary, double* diag, double* err, double* norm) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  ts_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, summary || diag || err || norm);
  hipStream_t s = h->stream;
  ts_host_call(h, host_batch(h, B, u, k, n_k_rows, k_row, T, s), 0, accumulate, summary, diag, err, norm, s);
  KIN_CATCH(h)
}

int kin_solution_timescale(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                           int64_t row_begin, int accumulate, double* summary, double* norm) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(row_begin >= 0, ERR_INVALID_ARG, "row_begin < 0");
  hipStream_t s = h->stream;
  const StateBatch b = solution_batch(h, drg_check, k, n_k_rows, k_row, T_rows, summary || norm, s);
  ts_limits(h);
  ts_host_call(h, b, row_begin, accumulate, summary, nullptr, nullptr, norm, s);
  KIN_CATCH(h)
}

int kin_ensemble_timescale(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                           int64_t row_begin, int accumulate, double* summary, double* norm) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(row_begin >= 0, ERR_INVALID_ARG, "row_begin < 0");
  hipStream_t s = h->stream;
  const StateBatch b = ensemble_batch(h, drg_check, k, n_k_rows, k_row, T_rows, summary || norm, s);
  ts_limits(h);
  ts_host_call(h, b, row_begin, accumulate, summary, nullptr, nullptr, norm, s);
  KIN_CATCH(h)
}

}  // extern "C"
