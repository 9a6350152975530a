// extern "C" boundary of libkinetica_hip.so (declarations + reference citations:
// include/kinetica_hip.h). Every entry point converts exceptions into status codes.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "handle.hpp"
#include "lu.hpp"
#include "solver.hpp"
#include "solver_kernels.hpp"

using namespace kin;

static thread_local std::string g_create_err;

// handle.hpp's guard, but for entries that may run without a handle (kin_network_create): the message then goes to g_create_err
#undef KIN_TRY
#undef KIN_CATCH
#define KIN_TRY(h) try { if (h) KIN_HIP(hipSetDevice((h)->device));
#define KIN_CATCH(h)                                                        \
  }                                                                         \
  catch (const KinError& e) {                                               \
    if (h) (h)->err = e.what(); else g_create_err = e.what();               \
    return e.code;                                                          \
  }                                                                         \
  catch (const std::exception& e) {                                         \
    if (h) (h)->err = e.what(); else g_create_err = e.what();               \
    return KIN_ERR_DEVICE;                                                  \
  }                                                                         \
  return KIN_OK;

extern "C" {

const char* kin_version(void) { return "kinetica-hip 0.5 (gfx950)"; }

int kin_abi_version(void) { return KIN_ABI_VERSION; }

int64_t kin_struct_size(int which) {
  return which == 0 ? (int64_t)sizeof(kin_params) : which == 1 ? (int64_t)sizeof(kin_stats) : -1;
}

int kin_device_count(int* n) {
  if (!n) return KIN_ERR_INVALID_ARG;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) { *n = 0; return KIN_ERR_DEVICE; }
  *n = c;
  return KIN_OK;
}

int kin_set_device(int device) { return hipSetDevice(device) == hipSuccess ? KIN_OK : KIN_ERR_DEVICE; }

const char* kin_last_error(const kin_network* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int kin_network_create(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                       const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx,
                       const int64_t* prod_sto, int index_base, kin_network** out) {
  kin_network* h = nullptr;
  if (!out) { g_create_err = "out is null"; return KIN_ERR_INVALID_ARG; }
  *out = nullptr;
  try {
    NetworkHost H = compile_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx,
                                    prod_sto, index_base);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
      throw KinError(ERR_DEVICE, "no HIP device available (libkinetica_hip has no CPU fallback)");
    h = new kin_network();
    h->host = std::move(H);
    h->index_base = index_base;
    KIN_HIP(hipGetDevice(&h->device));
    KIN_HIP(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    KIN_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const NetworkHost& N = h->host;
    hipStream_t s = h->stream;
    upload_solve_tables(h);
    if (N.N < 65535) { h->sweep_rec.upload(N.pair_rec, s); h->sweep_k.upload(N.pair_k, s); }
    if (!N.gen_rec8.empty()) { h->gen_rec8.upload(N.gen_rec8, s); h->gen_k.upload(N.gen_k, s); h->gen_expl.upload(N.gen_expl, s); }
    if (!N.pair_rec64.empty()) { h->sweep_rec64.upload(N.pair_rec64, s); h->sweep_copy.upload(N.sweep_copy_species, s); }
    if (N.big_H > 0) {
      h->big_rec.upload(N.big_rec, s); h->big_rec8.upload(N.big_rec8, s); h->big_expl.upload(N.big_expl, s);
      h->big_spec.upload(N.big_spec_of_label, s);
      h->big_tptr.upload(N.big_tail_ptr, s); h->big_tent.upload(N.big_tail_ent, s);
    }
    KIN_HIP(hipStreamSynchronize(s));
    *out = h;
  } catch (const KinError& e) {
    g_create_err = e.what();
    delete h;
    return e.code;
  } catch (const std::exception& e) {
    g_create_err = e.what();
    delete h;
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}

// Symbolic analysis of the Newton-matrix factorisation without a device (sizes only): info[0..11] = ns, m, rounds, nnzU, nnzZ,
// nnzV, nnzLZ, nnzNVU, w_size, fused products, gather-plan entries, gather-plan wavefront tasks
int kin_lu_analyze_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                        const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                        int index_base, int hub_degree, int max_rounds, int max_tail_degree, int max_degree, int min_round,
                        int64_t* info) {
  return with_compiled_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base, g_create_err,
                               [&](const NetworkHost& H) {
    SparseLU lu;
    lu.host_only = true;
    LUOptions opt;
    if (hub_degree > 0) opt.hub_degree = hub_degree;
    if (max_rounds > 0) opt.max_rounds = max_rounds;
    if (max_tail_degree > 0) opt.max_tail_degree = max_tail_degree;
    if (max_degree > 0) opt.max_degree = max_degree;
    if (min_round > 0) opt.min_round = min_round;
    lu.analyze((int32_t)H.N, H.j_ptr, H.j_col, opt, nullptr);
    if (info) {
      info[0] = lu.ns; info[1] = lu.m; info[2] = lu.nrounds; info[3] = lu.nnzU; info[4] = lu.nnzZ; info[5] = lu.nnzV;
      info[6] = lu.nnzLZ; info[7] = lu.nnzNVU; info[8] = lu.w_size; info[9] = lu.n_fused_products; info[10] = lu.plan_entries;
      info[11] = lu.plan_tasks;
    }
  });
}

int kin_network_destroy(kin_network* h) {
  delete h;
  return KIN_OK;
}

int kin_network_sizes(const kin_network* h, int64_t* n_species, int64_t* n_reactions) {
  if (!h) return KIN_ERR_INVALID_ARG;
  if (n_species) *n_species = h->host.N;
  if (n_reactions) *n_reactions = h->host.R;
  return KIN_OK;
}

int kin_network_compute_units(const kin_network* h, int* n_cu) {
  if (!h || !n_cu) return KIN_ERR_INVALID_ARG;
  *n_cu = h->n_cu;
  return KIN_OK;
}

int kin_set_rates(kin_network* h, const double* k) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(k != nullptr, ERR_INVALID_ARG, "k is null");
  h->k.upload(k, h->host.R, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  h->has_rates = true;
  h->k_pending = false;
  KIN_CATCH(h)
}

int kin_get_rates(kin_network* h, double* k_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(k_out != nullptr, ERR_INVALID_ARG, "k_out is null");
  require(h->has_rates, ERR_STATE, "rates were never set");
  h->flush_pending_T(h->stream);
  h->k.download(k_out, h->host.R, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_set_arrhenius(kin_network* h, const double* Ea, const double* A, double k_max, double t_mult) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(Ea && A, ERR_INVALID_ARG, "Ea / A is null");
  h->Ea.upload(Ea, h->host.R, h->stream);
  h->A.upload(A, h->host.R, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  // a cap at +inf is no cap (1 / (0 + 1/k_r) = k_r): the capped fast form would take the reciprocal of x = 0 where k_r overflows
  h->has_kmax = !std::isnan(k_max) && !std::isinf(k_max);
  h->k_max = h->has_kmax ? k_max : 1.0;
  h->t_mult = t_mult;
  h->has_arrhenius = true;
  h->t_par_valid = false;
  KIN_CATCH(h)
}

int kin_rates_at(kin_network* h, double T, double* k_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->has_arrhenius, ERR_STATE, "Arrhenius parameters were never set");
  launch_arrhenius(h->host.R, h->Ea.p, h->A.p, h->has_kmax, h->k_max, h->t_mult, T, h->k.p, h->stream);
  h->k_pending = false;
  if (k_out) h->k.download(k_out, h->host.R, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  h->has_rates = true;
  KIN_CATCH(h)
}

int kin_arrhenius_eval(const double* Ea, const double* A, int64_t n, double k_max, double t_mult, double T,
                       double* k_out) {
  kin_network* h = nullptr;
  KIN_TRY(h)
  require(Ea && A && k_out && n >= 0, ERR_INVALID_ARG, "bad arguments");
  DevBuf<double> dEa, dA, dk;
  dEa.upload(Ea, n); dA.upload(A, n); dk.alloc(n);
  const bool has = !std::isnan(k_max) && !std::isinf(k_max);   // (as kin_set_arrhenius)
  launch_arrhenius(n, dEa.p, dA.p, has, has ? k_max : 1.0, t_mult, T, dk.p, nullptr);
  dk.download(k_out, n);
  KIN_HIP(hipStreamSynchronize(nullptr));
  KIN_CATCH(h)
}

int kin_rate_table(kin_network* h, const double* T, int64_t n_stops, double* out_table) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->has_arrhenius, ERR_STATE, "Arrhenius parameters were never set");
  require(T != nullptr && n_stops >= 0, ERR_INVALID_ARG, "bad arguments");
  h->T_stops.upload(T, n_stops, h->stream);
  h->table.alloc((size_t)n_stops * h->host.R);
  launch_rate_table(h->host.R, n_stops, h->Ea.p, h->A.p, h->has_kmax, h->k_max, h->t_mult, h->T_stops.p, h->table.p, h->stream);
  h->table_rows = n_stops;
  if (out_table) h->table.download(out_table, (size_t)n_stops * h->host.R, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_rhs(kin_network* h, const double* u, double* du) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(u && du, ERR_INVALID_ARG, "u / du is null");
  require(h->has_rates, ERR_STATE, "rates were never set");
  h->u.upload(u, h->host.N, h->stream);
  h->rhs_dev(h->u.p, h->du.p);
  h->du.download(du, h->host.N, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_rhs_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, double* d_du, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B > 0, ERR_INVALID_ARG, "B must be positive");
  require(d_u && d_du, ERR_INVALID_ARG, "null device buffer");
  require(d_k || h->has_rates, ERR_STATE, "rates were never set and no per-state k given");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  h->sweep_dev(B, d_u, d_k, d_du, s);
  KIN_CATCH(h)
}

static void sweep_plan_info(const SweepPlan& p, int64_t* info) {
  const int64_t v[KIN_SWEEP_PLAN_INFO] = {p.kernel, p.bs, p.tr, p.ilp, p.blk, p.adj, p.u_in_lds, p.n_a, p.n_b, p.grid, p.per_cu,
                                          p.n_copy, p.n_expl, p.tail_tiles, p.tail_by_species, (int64_t)p.smem, p.n_tiles, p.H, p.P};
  std::copy(v, v + KIN_SWEEP_PLAN_INFO, info);
}

int kin_sweep_plan(kin_network* h, int64_t B, const double* d_u, const double* d_k, const double* d_du, int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B > 0 && info, ERR_INVALID_ARG, "bad arguments");
  sweep_plan_info(h->sweep_plan_dev(B, d_u, d_k, d_du), info);   // exactly what kin_rhs_batched_dev asks for
  KIN_CATCH(h)
}

int kin_sweep_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                        const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                        int index_base, int n_cu, int64_t B, int u_bits, int k_bits, int du_bits, int64_t* info) {
  if (!info || n_cu < 1 || B < 1 || u_bits < 0 || u_bits > 15 || k_bits < 0 || k_bits > 15 || du_bits < 0 || du_bits > 15)
    return KIN_ERR_INVALID_ARG;
  return with_compiled_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base, g_create_err,
                               [&](const NetworkHost& H) {
    sweep_plan_info(sweep_plan(sweep_net_info(H), n_cu, B, SweepAlign{(unsigned)u_bits, (unsigned)k_bits, (unsigned)du_bits}), info);
  });
}

int kin_rhs_batched(kin_network* h, int64_t B, const double* u, const double* k, double* du) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(B > 0 && u && du, ERR_INVALID_ARG, "bad arguments");
  require(k || h->has_rates, ERR_STATE, "rates were never set and no per-state k given");
  const int64_t N = h->host.N, R = h->host.R;
  hipStream_t s = h->stream;
  h->b_u.upload(u, (size_t)B * N, s);
  h->b_du.alloc((size_t)B * N);
  if (k) h->b_k.upload(k, (size_t)B * R, s);
  h->sweep_dev(B, h->b_u.p, k ? h->b_k.p : nullptr, h->b_du.p, s);
  h->b_du.download(du, (size_t)B * N, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_jac_nnz(kin_network* h, int64_t* nnz) {
  if (!h || !nnz) return KIN_ERR_INVALID_ARG;
  *nnz = h->host.nnz();
  return KIN_OK;
}

int kin_drg_pattern_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                         const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                         int index_base, int pairing, int64_t* info, int64_t* rowptr, int64_t* colidx) {
  return with_compiled_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base, g_create_err,
                               [&](const NetworkHost& H) {
    const DrgTables t = build_drg_tables(H, pairing, false);
    if (info) {
      info[0] = t.E; info[1] = t.n_den; info[2] = t.n_num;
      for (int c = 0; c < 3; c++) { info[3 + c] = t.den_cls[c]; info[6 + c] = t.edge_cls[c]; }
    }
    if (rowptr) for (int64_t i = 0; i <= t.N; i++) rowptr[i] = t.rowptr[i] + index_base;
    if (colidx) for (int64_t e = 0; e < t.E; e++) colidx[e] = t.colidx[e] + index_base;
  });
}

int kin_reaction_importance_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                                      const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                                      int index_base, int pairing, int64_t* info, int64_t* partner, int64_t* species, int64_t* nu) {
  return with_compiled_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base, g_create_err,
                               [&](const NetworkHost& H) {
    const RiTables t = build_ri_tables(H, pairing);
    if (info) { info[0] = t.n_records; info[1] = t.n_paired; info[2] = t.n_empty; }
    if (partner) for (int64_t r = 0; r < t.R; r++) partner[r] = t.partner[r];
    if (species) for (int64_t i = 0; i < 4 * t.R; i++) species[i] = t.species[i];
    if (nu) for (int64_t i = 0; i < 4 * t.R; i++) nu[i] = t.nu[i];
  });
}

int kin_pfa_pattern_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                         const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                         int index_base, int pairing, int64_t* info, int64_t* rowptr, int64_t* colidx) {
  return with_compiled_network(n_species, n_reactions, reac_ptr, reac_idx, reac_sto, prod_ptr, prod_idx, prod_sto, index_base, g_create_err,
                               [&](const NetworkHost& H) {
    const DrgTables g = build_drg_tables(H, pairing, false);
    const PfaTables t = build_pfa_tables(g.N, g.rowptr, g.colidx);
    if (info) { info[0] = t.E; info[1] = t.E2; info[2] = t.products; info[3] = t.max_row; }
    if (rowptr) for (int64_t i = 0; i <= t.N; i++) rowptr[i] = t.rowptr2[i] + index_base;
    if (colidx) for (int64_t e = 0; e < t.E2; e++) colidx[e] = t.colidx2[e] + index_base;
  });
}

int kin_jac_pattern(kin_network* h, int64_t* rowptr, int64_t* colidx, int index_base) {
  if (!h || !rowptr || !colidx) return KIN_ERR_INVALID_ARG;
  const NetworkHost& N = h->host;
  for (int64_t i = 0; i <= N.N; i++) rowptr[i] = N.j_ptr[i] + index_base;
  for (int64_t e = 0; e < N.nnz(); e++) colidx[e] = N.j_col[e] + index_base;
  return KIN_OK;
}

int kin_jac_values(kin_network* h, const double* u, double* vals) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(u && vals, ERR_INVALID_ARG, "u / vals is null");
  require(h->has_rates, ERR_STATE, "rates were never set");
  h->u.upload(u, h->host.N, h->stream);
  h->jac_dev(h->u.p, h->jvals.p);
  h->jvals.download(vals, h->host.nnz(), h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_solve(kin_network* h, const kin_params* params, const double* u0, const double* tstops,
              const double* T_stops, const double* k_table, int64_t n_stops, int64_t* n_saved, int32_t* retcode,
              kin_stats* stats) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && u0, ERR_INVALID_ARG, "params / u0 is null");
  finish_solve(h, solve_entry(h, *params, u0, tstops, T_stops, k_table, n_stops, stats), n_saved, retcode);
  KIN_CATCH(h)
}

int kin_solve_ensemble(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* k, const double* T,
                       const double* tstops, const double* T_stops, const double* k_table, int64_t n_stops, int64_t* n_rows,
                       double* out_t, double* out_u, int64_t* n_saved, int32_t* retcodes, kin_stats* stats) {
  const EnsembleCall c{kin_params{}, K, u0, k, T, tstops, T_stops, k_table, n_stops, nullptr, nullptr, nullptr, nullptr, n_rows, out_t, out_u, n_saved,
                       retcodes, stats};
  return ensemble_entry(h, params, c, [&] {
    require(!(k && T), ERR_INVALID_ARG, "give per-member rate constants or per-member temperatures, not both");
    require(!(n_stops > 0 && (k || T)), ERR_INVALID_ARG, "discrete rate updates are shared by the ensemble: no per-member k / T with tstops");
    require(!T || h->has_arrhenius, ERR_STATE, "temperatures given but Arrhenius parameters were never set");
  }, [&] { validate_solve(h, *params, tstops, T_stops, k_table, n_stops, nullptr, nullptr, 0, !(k || T)); });
}

int kin_solve_ensemble_continuous(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                  const int64_t* node_ptr, const double* t_nodes, const double* T_nodes,
                                  int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved,
                                  int32_t* retcodes, kin_stats* stats) {
  return ensemble_member_entry(h, params, K, u0, nullptr, nullptr, true, node_ptr, t_nodes, T_nodes, n_rows, out_t, out_u, n_saved, retcodes, stats);
}

int kin_solve_ensemble_continuous_params(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* Ea,
                                         const double* A, const int64_t* node_ptr, const double* t_nodes, const double* T_nodes,
                                         int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved, int32_t* retcodes,
                                         kin_stats* stats) {
  return ensemble_member_entry(h, params, K, u0, Ea, A, true, node_ptr, t_nodes, T_nodes, n_rows, out_t, out_u, n_saved, retcodes, stats);
}

int kin_solve_ensemble_discrete(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                const int64_t* stop_ptr, const double* tstops, const double* T_stops,
                                int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved,
                                int32_t* retcodes, kin_stats* stats) {
  return ensemble_member_entry(h, params, K, u0, nullptr, nullptr, false, stop_ptr, tstops, T_stops, n_rows, out_t, out_u, n_saved, retcodes, stats);
}

int kin_solve_ensemble_discrete_params(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* Ea,
                                       const double* A, const int64_t* stop_ptr, const double* tstops, const double* T_stops,
                                       int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved, int32_t* retcodes,
                                       kin_stats* stats) {
  return ensemble_member_entry(h, params, K, u0, Ea, A, false, stop_ptr, tstops, T_stops, n_rows, out_t, out_u, n_saved, retcodes, stats);
}

int kin_newton_solve(kin_network* h, double c, const double* u, const double* b, double* x) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(u && b && x, ERR_INVALID_ARG, "null buffer");
  require(h->has_rates, ERR_STATE, "rates were never set");
  newton_solve(h, c, u, b, x);
  KIN_CATCH(h)
}

int kin_newton_probe(kin_network* h, int64_t K, int32_t batched, const double* u, const double* c, const double* b,
                     double* x, int32_t* bad, int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(K >= 1 && K <= (1 << 20), ERR_INVALID_ARG, "K outside 1 .. 2^20");
  require(u && c && b && x && bad && info, ERR_INVALID_ARG, "null buffer");
  require(h->has_rates, ERR_STATE, "rates were never set");
  newton_probe(h, K, batched, u, c, b, x, bad, info);
  KIN_CATCH(h)
}

int kin_resident_probe(kin_network* h, int64_t K, const double* u, const double* c, const double* b, double* du, double* jac,
                       double* x, int32_t* bad, int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(K >= 1 && K <= (1 << 20), ERR_INVALID_ARG, "K outside 1 .. 2^20");
  require(u && c && b && du && jac && x && bad && info, ERR_INVALID_ARG, "null buffer");
  require(h->has_rates, ERR_STATE, "rates were never set");
  resident_probe(h, K, u, c, b, du, jac, x, bad, info);
  KIN_CATCH(h)
}

int kin_solve_explicit(kin_network* h, const kin_params* params, const double* u0, const double* tstops, const double* T_stops,
                       const double* k_table, int64_t n_stops, int64_t* n_saved, int32_t* retcode, kin_stats* stats) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && u0, ERR_INVALID_ARG, "params / u0 is null");
  require(n_stops >= 0, ERR_INVALID_ARG, "n_stops < 0");
  finish_solve(h, solve_entry(h, *params, u0, tstops, T_stops, k_table, n_stops, stats, nullptr, nullptr, 0, true), n_saved, retcode);
  KIN_CATCH(h)
}

int kin_solve_continuous(kin_network* h, const kin_params* params, const double* u0, const double* t_nodes,
                         const double* T_nodes, int64_t n_nodes, int64_t* n_saved, int32_t* retcode, kin_stats* stats) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && u0, ERR_INVALID_ARG, "params / u0 is null");
  finish_solve(h, solve_entry(h, *params, u0, nullptr, nullptr, nullptr, 0, stats, t_nodes, T_nodes, n_nodes), n_saved, retcode);
  KIN_CATCH(h)
}

int kin_integrator_init(kin_network* h, const kin_params* params, const double* u0, const double* tstops,
                        const double* T_stops, const double* k_table, int64_t n_stops) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && u0, ERR_INVALID_ARG, "params / u0 is null");
  require(n_stops >= 0, ERR_INVALID_ARG, "n_stops < 0");
  integrator_init(h, *params, u0, tstops, T_stops, k_table, n_stops);
  KIN_CATCH(h)
}

int kin_integrator_init_continuous(kin_network* h, const kin_params* params, const double* u0, const double* t_nodes,
                                   const double* T_nodes, int64_t n_nodes) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(params && u0, ERR_INVALID_ARG, "params / u0 is null");
  require(n_nodes >= 2, ERR_INVALID_ARG, "need >= 2 (t, T) nodes");
  integrator_init(h, *params, u0, nullptr, nullptr, nullptr, 0, t_nodes, T_nodes, n_nodes);
  KIN_CATCH(h)
}

int kin_integrator_step(kin_network* h, int64_t max_steps, int64_t* steps_taken) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const int64_t n = integrator_step(h, max_steps);
  if (steps_taken) *steps_taken = n;
  KIN_CATCH(h)
}

int kin_integrator_state(kin_network* h, double* t, double* u, int32_t* retcode, kin_stats* stats) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  integrator_state(h, t, u, retcode, stats);
  KIN_CATCH(h)
}

int kin_solution_size(const kin_network* h, int64_t* n_saved, int64_t* n_species) {
  if (!h) return KIN_ERR_INVALID_ARG;
  if (n_saved) *n_saved = h->n_saved;
  if (n_species) *n_species = h->host.N;
  return KIN_OK;
}

int kin_solution_copy(const kin_network* hc, double* out_t, double* out_u) {
  kin_network* h = const_cast<kin_network*>(hc);
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out_t && out_u, ERR_INVALID_ARG, "null output buffer");
  std::copy(h->sol_t.begin(), h->sol_t.begin() + h->n_saved, out_t);
  h->d_sol_u.download(out_u, (size_t)h->n_saved * h->host.N, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_solution_max(const kin_network* hc, double* out_umax) {
  kin_network* h = const_cast<kin_network*>(hc);
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out_umax != nullptr, ERR_INVALID_ARG, "null output buffer");
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  solution_max(h, out_umax);
  KIN_CATCH(h)
}

int kin_solution_max_dev(const kin_network* hc, double* d_out) {
  kin_network* h = const_cast<kin_network*>(hc);
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(d_out != nullptr, ERR_INVALID_ARG, "null device buffer");
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  launch_colmax((int)h->host.N, h->n_saved, h->d_sol_u.p, d_out, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_rate_table_dev(kin_network* h, const double* T, int64_t n_stops, double* d_out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->has_arrhenius, ERR_STATE, "Arrhenius parameters were never set");
  require(T != nullptr && d_out != nullptr && n_stops >= 0, ERR_INVALID_ARG, "bad arguments");
  h->T_stops.upload(T, n_stops, h->stream);
  launch_rate_table(h->host.R, n_stops, h->Ea.p, h->A.p, h->has_kmax, h->k_max, h->t_mult, h->T_stops.p, d_out, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_rhs_block_dev(kin_network* h, int64_t r_lo, int64_t r_hi, const double* d_u, double* d_du, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(d_u && d_du, ERR_INVALID_ARG, "null device buffer");
  require(h->has_rates, ERR_STATE, "rates were never set");
  require(0 <= r_lo && r_lo <= r_hi && r_hi <= h->host.R, ERR_INVALID_ARG, "reaction block out of range");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  h->flush_pending_T(s);
  // rates of the block, zeros elsewhere; the species-major gather then sums exactly this block's contributions
  KIN_HIP(hipMemsetAsync(h->rate.p, 0, (size_t)h->host.R * sizeof(double), s));
  launch_rates(r_hi - r_lo, h->k.p + r_lo, d_u, h->x0.p + r_lo, h->x1.p + r_lo, h->rate.p + r_lo, s);
  launch_segsum(h->rhs_plan.view(), SEG_COEF_SET, h->rate.p, d_du, SegExtra{}, s);
  KIN_CATCH(h)
}

int kin_solution_dot(const kin_network* hc, const double* w, double* out) {
  kin_network* h = const_cast<kin_network*>(hc);
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(w && out, ERR_INVALID_ARG, "null buffer");
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  DevBuf<double> dw, dout;
  dw.upload(w, h->host.N, h->stream);
  dout.alloc(h->n_saved);
  launch_rowdot((int)h->host.N, h->n_saved, h->d_sol_u.p, dw.p, dout.p, h->stream);
  dout.download(out, h->n_saved, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_rate_table_rows(kin_network* h, const int64_t* rows, int64_t n_rows, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(rows && out && n_rows >= 0, ERR_INVALID_ARG, "bad arguments");
  require(h->table_rows > 0, ERR_STATE, "no rate table resident (kin_rate_table / kin_solve with a table first)");
  const int64_t R = h->host.R;
  for (int64_t i = 0; i < n_rows; i++) {
    require(rows[i] >= 0 && rows[i] < h->table_rows, ERR_INVALID_ARG, "row index out of range");
    KIN_HIP(hipMemcpyAsync(out + (size_t)i * R, h->table.p + (size_t)rows[i] * R, R * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

}  // extern "C"
