// extern "C" entry points of path flux analysis (declarations: include/kinetica_hip.h; tables: pfa.cpp; split stage:
// drg_kernels.hip, SPLIT; second-generation stage: pfa_kernels.hip). Batches, blocks and staging: flux_api.hpp; stage 1 with
// the denominators, the tables of a pairing mode and the fold over slices are the DRG family's (drg_api.hpp).
// kin_pfa_pattern_host, which needs no handle, sits with the other host-only entries in capi.cpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "drg_api.hpp"
#include "pfa.hpp"

using namespace kin;

namespace {

void pfa_check_size(const kin_network* h) {
  if (h->host.N > PFA_LDS_SPECIES)
    throw KinError(ERR_UNSUPPORTED, "PFA: at most " + std::to_string(PFA_LDS_SPECIES) +
                                        " species (a row buffer of 8 n_species bytes has to fit the 160 KB of LDS of a compute unit)");
}

PfaTables& pfa_host(kin_network* h, int pairing) {
  auto& m = h->pfa[pairing ? 1 : 0];
  if (!m.host) {
    const DrgTables& g = drg_host(h, pairing);
    m.host = std::make_unique<PfaTables>(build_pfa_tables(g.N, g.rowptr, g.colidx));
  }
  return *m.host;
}

kin_network::PfaMode& pfa_dev(kin_network* h, int pairing, hipStream_t s) {
  auto& m = h->pfa[pairing ? 1 : 0];
  const PfaTables& t = pfa_host(h, pairing);
  if (!m.dev_ready) {
    const DrgTables& g = drg_host(h, pairing);
    m.rowptr.upload(g.rowptr, s); m.colidx.upload(g.colidx, s);
    m.rowptr2.upload(t.rowptr2, s); m.colidx2.upload(t.colidx2, s); m.order.upload(t.order, s);
    KIN_HIP(hipStreamSynchronize(s));
    m.dev_ready = true;
  }
  return m;
}

// States per block: none of rates[nb][R], rp[nb][E] + rc[nb][E] and (when asked for) r[nb][E2] above the bound
int64_t pfa_block(const kin_network* h, const PfaTables& t, int64_t B, bool want_r) {
  return block_states((size_t)std::max<int64_t>(std::max<int64_t>(h->host.R, 2 * t.E), std::max<int64_t>(want_r ? t.E2 : 0, 1)), B,
                      DRG_BLOCK_ENV);
}

int64_t pfa_wg_cost(int64_t N) {
  if (const char* e = getenv("KIN_PFA_WG_COST")) {        // (read per call: tests and the benchmark move rows between the classes)
    const int64_t v = atoll(e);
    if (v >= 0) return v;
  }
  return N > PFA_WAVE_SPECIES ? 0 : PFA_WG_COST;
}

struct PfaOut { double* rp; double* rc; double* r; };       // optional host outputs of the host entries, per state

void pfa_alloc(kin_network* h, const PfaTables& t, int64_t nb_max, bool want_r) {
  h->pfa_rp.alloc((size_t)nb_max * t.E);
  h->pfa_rc.alloc((size_t)nb_max * t.E);
  if (want_r) h->pfa_r.alloc((size_t)nb_max * t.E2);
  h->pfa_part.alloc((size_t)slices_cap(pfa_slices(t, nb_max, h->n_cu)) * t.E2);
}

// The second-generation stage of one block whose coefficients are in h->pfa_rp / pfa_rc, folded into d_coef.
void pfa_second_block(kin_network* h, kin_network::PfaMode& m, int64_t b0, int64_t nb, const int64_t* d_seg_n, int64_t L, int use_prev,
                      double* d_coef, const PfaOut& out, hipStream_t s) {
  const PfaTables& t = *m.host;
  PfaArgs a{};
  a.N = (int)t.N; a.nb = (int)nb; a.E = t.E; a.E2 = t.E2;
  a.rowptr = m.rowptr.p; a.colidx = m.colidx.p; a.rowptr2 = m.rowptr2.p; a.colidx2 = m.colidx2.p; a.order = m.order.p;
  a.rp = h->pfa_rp.p; a.rc = h->pfa_rc.p;
  a.b0 = b0; a.seg_n = d_seg_n; a.L = L;
  a.part = h->pfa_part.p; a.r = out.r ? h->pfa_r.p : nullptr;
  const int Y = slices_cap(pfa_slices(t, nb, h->n_cu));
  launch_pfa_second(t, a, pfa_wg_cost(t.N), Y, s);
  launch_drg_max(t.E2, Y, h->pfa_part.p, d_coef, use_prev, s);
  if (out.rp) h->pfa_rp.download(out.rp + (size_t)b0 * t.E, (size_t)nb * t.E, s);
  if (out.rc) h->pfa_rc.download(out.rc + (size_t)b0 * t.E, (size_t)nb * t.E, s);
  if (out.r) h->pfa_r.download(out.r + (size_t)b0 * t.E2, (size_t)nb * t.E2, s);
}

// The pass on device buffers, block by block: stage 1 (the flux sweep) writes the block's rates, the signed denominator
// launch den = max(P, C), the split stage rp and rc, the second-generation stage the maxima of r, folded into d_coef.
void pfa_run(kin_network* h, int pairing, const StateBatch& b, int accumulate, double* d_coef, const PfaOut& out, hipStream_t s) {
  auto& g = drgep_dev(h, pairing, s);
  auto& m = pfa_dev(h, pairing, s);
  const PfaTables& t = *m.host;
  if (t.E2 == 0 || empty_batch(b.B, d_coef, t.E2, accumulate, s)) return;
  int upto = 3;      // KIN_PFA_STAGES=1 / 2 ends every block after stage 1 / the split stage and leaves d_coef alone: for timing the stages only
  if (const char* e = getenv("KIN_PFA_STAGES")) upto = atoi(e) >= 1 ? atoi(e) : 3;
  const int64_t nb_max = pfa_block(h, t, b.B, out.r != nullptr);
  drg_stage_alloc(h, nb_max);
  pfa_alloc(h, t, nb_max, out.r != nullptr);
  const DrgPlan den = signed_den_plan(g), edge = signed_edge_plan(g);
  for_blocks(b.B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
    DrgArgs a{};
    a.E = (int)t.E; a.r = h->pfa_rp.p; a.rc = h->pfa_rc.p;
    drg_rates_den(h, b, b0, nb, den, true, upto, a, s);
    if (upto < 2) return;
    edge.into(a);
    launch_pfa_split(a, slices_cap(drg_slices(edge.p, nb, h->n_cu)), s);
    if (upto < 3) return;
    pfa_second_block(h, m, b0, nb, b.seg_n, b.L, use_prev, d_coef, out, s);
  });
}

// host entries of a batch: coef staged through the handle
void pfa_host_call(kin_network* h, int pairing, const StateBatch& b, int accumulate, double* coef, const PfaOut& out, hipStream_t s) {
  staged_result(h, pfa_host(h, pairing).E2, coef, accumulate, s,
                [&](double* d_coef) { pfa_run(h, pairing, b, accumulate, d_coef, out, s); });
}

}  // namespace

extern "C" {

int kin_pfa_pattern(kin_network* h, int pairing, int index_base, int64_t* nnz, int64_t* rowptr, int64_t* colidx) {
  if (!h) return KIN_ERR_INVALID_ARG;
  try {     // (host tables only: no device call)
    const PfaTables& t = pfa_host(h, pairing);
    if (nnz) *nnz = t.E2;
    if (rowptr) for (int64_t i = 0; i <= t.N; i++) rowptr[i] = t.rowptr2[i] + index_base;
    if (colidx) for (int64_t e = 0; e < t.E2; e++) colidx[e] = t.colidx2[e] + index_base;
  } catch (const KinError& e) { h->err = e.what(); return e.code; }
  catch (const std::exception& e) { h->err = e.what(); return KIN_ERR_INVALID_ARG; }
  return KIN_OK;
}

int kin_pfa_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                        const double* d_T, int accumulate, double* d_coef, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, d_k != nullptr, d_k_row != nullptr, d_T != nullptr, d_coef != nullptr);
  pfa_check_size(h);
  require(d_u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  pfa_run(h, pairing, StateBatch{B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0}, accumulate, d_coef,
          PfaOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_pfa_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef, double* rp_out, double* rc_out, double* r_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, coef != nullptr);
  pfa_check_size(h);
  hipStream_t s = h->stream;
  pfa_host_call(h, pairing, host_batch(h, B, u, k, n_k_rows, k_row, T, s), accumulate, coef, PfaOut{rp_out, rc_out, r_out}, s);
  KIN_CATCH(h)
}

int kin_pfa_paths(kin_network* h, int pairing, int64_t B, const double* rp, const double* rc, int accumulate, double* coef, double* r_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B >= 0 && B < ((int64_t)1 << 31), ERR_INVALID_ARG, "B out of range");
  require(coef != nullptr, ERR_INVALID_ARG, "null output buffer");
  drg_limit(h);
  pfa_check_size(h);
  hipStream_t s = h->stream;
  const PfaTables& t = pfa_host(h, pairing);
  require((rp != nullptr && rc != nullptr) || B == 0 || t.E == 0, ERR_INVALID_ARG, "null coefficient buffer");
  for (size_t i = 0, n = (size_t)B * (size_t)t.E; i < n; i++)
    require(std::isfinite(rp[i]) && rp[i] >= 0.0 && std::isfinite(rc[i]) && rc[i] >= 0.0, ERR_INVALID_ARG,
            "rp, rc: coefficients must be finite and not negative");
  staged_result(h, t.E2, coef, accumulate, s, [&](double* d_coef) {
    auto& m = pfa_dev(h, pairing, s);
    if (t.E2 == 0 || empty_batch(B, d_coef, t.E2, accumulate, s)) return;
    const int64_t nb_max = pfa_block(h, t, B, r_out != nullptr);
    pfa_alloc(h, t, nb_max, r_out != nullptr);
    for_blocks(B, nb_max, accumulate, [&](int64_t b0, int64_t nb, int use_prev) {
      h->pfa_rp.upload(rp + (size_t)b0 * t.E, (size_t)nb * t.E, s);
      h->pfa_rc.upload(rc + (size_t)b0 * t.E, (size_t)nb * t.E, s);
      pfa_second_block(h, m, b0, nb, nullptr, 0, use_prev, d_coef, PfaOut{nullptr, nullptr, r_out}, s);
    });
  });
  KIN_CATCH(h)
}

int kin_solution_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const StateBatch b = solution_batch(h, drg_check, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  pfa_check_size(h);
  pfa_host_call(h, pairing, b, accumulate, coef, PfaOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_ensemble_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const StateBatch b = ensemble_batch(h, drg_check, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  pfa_check_size(h);
  pfa_host_call(h, pairing, b, accumulate, coef, PfaOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

}  // extern "C"
