// extern "C" entry points of path flux analysis (declarations: include/kinetica_hip.h; tables: pfa.cpp; split stage:
// drg_kernels.hip, SPLIT; second-generation stage: pfa_kernels.hip). Stage 1, the checks, the rate-constant sources and the
// fold over slices, blocks and the caller's coefficients are the directed-relation-graph pass's (drg_api.hpp).
// kin_pfa_pattern_host, which needs no handle, sits with the other host-only entries in capi.cpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "drg_api.hpp"
#include "pfa.hpp"

using namespace kin;

namespace {

void require(bool c, int code, const char* msg) {
  if (!c) throw KinError(code, msg);
}

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

// States per block: none of rates[nb][R], rp[nb][E] + rc[nb][E] and (when asked for) r[nb][E2] above 256 MB;
// KIN_DRG_BLOCK_STATES as in the DRG pass.
int64_t pfa_block(const kin_network* h, const PfaTables& t, int64_t B, bool want_r) {
  const size_t row = (size_t)std::max<int64_t>(std::max<int64_t>(h->host.R, 2 * t.E), std::max<int64_t>(want_r ? t.E2 : 0, 1)) * sizeof(double);
  int64_t nb_max = std::max<int64_t>(1, (int64_t)(DRG_RATES_BYTES / row));
  if (const char* e = getenv("KIN_DRG_BLOCK_STATES")) {   // (read per call: tests change it)
    const int64_t v = atoll(e);
    if (v >= 1) nb_max = std::min(nb_max, v);
  }
  return std::min(nb_max, B);
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
void pfa_run(kin_network* h, int pairing, int64_t B, const double* d_u, const FluxSource& src, const int64_t* d_seg_n, int64_t L,
             int accumulate, double* d_coef, const PfaOut& out, hipStream_t s) {
  const int64_t N = h->host.N, R = h->host.R;
  auto& g = drgep_dev(h, pairing, s);
  auto& m = pfa_dev(h, pairing, s);
  const PfaTables& t = *m.host;
  if (t.E2 == 0) return;
  if (B == 0) {
    if (!accumulate) KIN_HIP(hipMemsetAsync(d_coef, 0, (size_t)t.E2 * sizeof(double), s));
    return;
  }
  int upto = 3;      // KIN_PFA_STAGES=1 / 2 ends every block after stage 1 / the split stage and leaves d_coef alone: for timing the stages only
  if (const char* e = getenv("KIN_PFA_STAGES")) upto = atoi(e) >= 1 ? atoi(e) : 3;
  const int64_t nb_max = pfa_block(h, t, B, out.r != nullptr);
  h->drg_rates.alloc((size_t)nb_max * R);
  h->drg_den.alloc((size_t)nb_max * N);
  pfa_alloc(h, t, nb_max, out.r != nullptr);
  const SegPlanView dv = g.den_plan.view(), ev = g.edge_plan.view();
  for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
    const int64_t nb = std::min(nb_max, B - b0);
    FluxSource bs = src;
    if (bs.k && !bs.k_row) bs.k += (size_t)b0 * (size_t)bs.k_stride;
    if (bs.k_row) bs.k_row += b0;
    if (bs.T) bs.T += b0;
    flux_run(h, nb, d_u + (size_t)b0 * N, bs, nullptr, nullptr, h->drg_rates.p, s);
    if (upto < 2) continue;
    DrgArgs a{};
    a.N = (int)N; a.R = (int)R; a.E = (int)t.E; a.nb = (int)nb;
    a.rates = h->drg_rates.p; a.b0 = b0; a.seg_n = d_seg_n; a.L = L;
    a.den = h->drg_den.p; a.r = h->pfa_rp.p; a.rc = h->pfa_rc.p;
    a.p = dv; a.ell_c = g.den_ell_s.p; a.long_c = g.den_long_s.p;
    launch_drgep_den(a, slices_cap(drg_slices(dv, nb, h->n_cu)), s);
    a.p = ev; a.ell_c = g.edge_ell_s.p; a.long_c = g.edge_long_s.p;
    launch_pfa_split(a, slices_cap(drg_slices(ev, nb, h->n_cu)), s);
    if (upto < 3) continue;
    pfa_second_block(h, m, b0, nb, d_seg_n, L, (accumulate || b0 > 0) ? 1 : 0, d_coef, out, s);
  }
}

// host entries: coef staged through the handle's buffer (uploaded first when it takes part in the maximum)
template <class F>
void pfa_host_call(kin_network* h, int pairing, int accumulate, double* coef, hipStream_t s, F run) {
  const int64_t E2 = pfa_host(h, pairing).E2;
  h->pfa_coef.alloc((size_t)E2);
  if (accumulate && E2 > 0) h->pfa_coef.upload(coef, (size_t)E2, s);
  run(h->pfa_coef.p);
  if (E2 > 0) h->pfa_coef.download(coef, (size_t)E2, s);
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
  pfa_run(h, pairing, B, d_u, FluxSource{d_k, h->host.R, d_k_row, d_T}, nullptr, 0, accumulate, d_coef, PfaOut{nullptr, nullptr, nullptr}, s);
  KIN_CATCH(h)
}

int kin_pfa_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef, double* rp_out, double* rc_out, double* r_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  drg_check(h, B, k != nullptr, k_row != nullptr, T != nullptr, coef != nullptr);
  pfa_check_size(h);
  require(u != nullptr || B == 0, ERR_INVALID_ARG, "null state buffer");
  if (k && k_row) { require(n_k_rows >= 1 || B == 0, ERR_INVALID_ARG, "k has no rows"); flux_check_rows(k_row, B, n_k_rows); }
  else if (k) require(n_k_rows == B, ERR_INVALID_ARG, "k without k_row needs one row per state (n_k_rows == B)");
  const int64_t N = h->host.N, R = h->host.R;
  hipStream_t s = h->stream;
  if (B > 0) h->f_u.upload(u, (size_t)B * N, s);
  if (k && n_k_rows > 0) h->f_k.upload(k, (size_t)n_k_rows * R, s);
  if (k_row && B > 0) h->f_krow.upload(k_row, (size_t)B, s);
  if (T && B > 0) h->f_T.upload(T, (size_t)B, s);
  const FluxSource src{k ? h->f_k.p : nullptr, R, k_row ? h->f_krow.p : nullptr, T ? h->f_T.p : nullptr};
  pfa_host_call(h, pairing, accumulate, coef, s, [&](double* d_coef) {
    pfa_run(h, pairing, B, h->f_u.p, src, nullptr, 0, accumulate, d_coef, PfaOut{rp_out, rc_out, r_out}, s);
  });
  KIN_CATCH(h)
}

int kin_pfa_paths(kin_network* h, int pairing, int64_t B, const double* rp, const double* rc, int accumulate, double* coef, double* r_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B >= 0 && B < ((int64_t)1 << 31), ERR_INVALID_ARG, "B out of range");
  require(coef != nullptr, ERR_INVALID_ARG, "null output buffer");
  require(h->host.N < ((int64_t)1 << 31) / 2, ERR_UNSUPPORTED, "DRG pass: N beyond 32-bit offsets");
  pfa_check_size(h);
  hipStream_t s = h->stream;
  const PfaTables& t = pfa_host(h, pairing);
  require((rp != nullptr && rc != nullptr) || B == 0 || t.E == 0, ERR_INVALID_ARG, "null coefficient buffer");
  for (size_t i = 0, n = (size_t)B * (size_t)t.E; i < n; i++)
    require(std::isfinite(rp[i]) && rp[i] >= 0.0 && std::isfinite(rc[i]) && rc[i] >= 0.0, ERR_INVALID_ARG,
            "rp, rc: coefficients must be finite and not negative");
  pfa_host_call(h, pairing, accumulate, coef, s, [&](double* d_coef) {
    auto& m = pfa_dev(h, pairing, s);
    if (t.E2 == 0) return;
    if (B == 0) {
      if (!accumulate) KIN_HIP(hipMemsetAsync(d_coef, 0, (size_t)t.E2 * sizeof(double), s));
      return;
    }
    const int64_t nb_max = pfa_block(h, t, B, r_out != nullptr);
    pfa_alloc(h, t, nb_max, r_out != nullptr);
    for (int64_t b0 = 0; b0 < B; b0 += nb_max) {
      const int64_t nb = std::min(nb_max, B - b0);
      h->pfa_rp.upload(rp + (size_t)b0 * t.E, (size_t)nb * t.E, s);
      h->pfa_rc.upload(rc + (size_t)b0 * t.E, (size_t)nb * t.E, s);
      pfa_second_block(h, m, b0, nb, nullptr, 0, (accumulate || b0 > 0) ? 1 : 0, d_coef, PfaOut{nullptr, nullptr, r_out}, s);
    }
  });
  KIN_CATCH(h)
}

int kin_solution_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_solution_source(h, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  pfa_check_size(h);
  pfa_host_call(h, pairing, accumulate, coef, s, [&](double* d_coef) {
    pfa_run(h, pairing, h->n_saved, h->d_sol_u.p, src, nullptr, 0, accumulate, d_coef, PfaOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

int kin_ensemble_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  hipStream_t s = h->stream;
  const FluxSource src = drg_ensemble_source(h, k, n_k_rows, k_row, T_rows, coef != nullptr, s);
  pfa_check_size(h);
  pfa_host_call(h, pairing, accumulate, coef, s, [&](double* d_coef) {
    pfa_run(h, pairing, h->ens.K * h->ens.cap, h->ens.sol, src, h->ens_segn.p, h->ens.cap, accumulate, d_coef,
            PfaOut{nullptr, nullptr, nullptr}, s);
  });
  KIN_CATCH(h)
}

}  // extern "C"
