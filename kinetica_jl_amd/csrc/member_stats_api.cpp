// extern "C" entry points of the cross-member statistics (declarations: include/kinetica_hip.h; kernels:
// member_stats_kernels.hip; sum orders: member_stats.hpp).
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "handle.hpp"
#include "member_stats.hpp"

using namespace kin;

static_assert(MS_MAX_SORTED == KIN_MEMBERS_MAX_SORTED, "the header states the limit of the sorted passes");

namespace {

// the members a mask names, ascending (null: all K)
std::vector<int32_t> participants(int64_t K, const int32_t* use) {
  std::vector<int32_t> idx;
  idx.reserve((size_t)K);
  for (int64_t m = 0; m < K; m++)
    if (!use || use[m] != 0) idx.push_back((int32_t)m);
  return idx;
}

// Xhat[q][p] of kin_members_inputs_host. Sums in long double: two passes for the mean (the second gives the mean of the
// residuals, kept as a separate term), deviations and their squares formed in long double and rounded once at the end.
void normalised_inputs(int64_t P, const double* X, const std::vector<int32_t>& idx, bool rank, double* xhat) {
  const size_t n = idx.size();
  std::vector<double> v(n);
  std::vector<size_t> order(n);
  for (int64_t p = 0; p < P; p++) {
    bool nan = false;
    for (size_t q = 0; q < n; q++) { v[q] = X[(size_t)idx[q] * (size_t)P + (size_t)p]; nan |= v[q] != v[q]; }
    if (nan) { for (size_t q = 0; q < n; q++) xhat[q * (size_t)P + (size_t)p] = std::nan(""); continue; }
    if (rank) {
      std::iota(order.begin(), order.end(), (size_t)0);
      std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
      std::vector<double> r(n);
      for (size_t i = 0; i < n;) {
        size_t e = i + 1;
        while (e < n && v[order[e]] == v[order[i]]) e++;      // (-0.0 == +0.0: they tie)
        const double avg = 0.5 * (double)(i + 1 + e);           // positions i + 1 .. e, 1-based
        for (size_t k = i; k < e; k++) r[order[k]] = avg;
        i = e;
      }
      v.swap(r);
    }
    long double m = 0.0L;
    for (size_t q = 0; q < n; q++) m += v[q];
    if (n) m /= (long double)n;
    long double c = 0.0L;
    for (size_t q = 0; q < n; q++) c += (long double)v[q] - m;
    if (n) c /= (long double)n;      // the mean is m + c: kept apart, a mean far above the spread would round the sum
    long double S = 0.0L;
    for (size_t q = 0; q < n; q++) { const long double d = ((long double)v[q] - m) - c; S += d * d; }
    if (n && *std::min_element(v.begin(), v.end()) == *std::max_element(v.begin(), v.end())) S = 0.0L;   // constant: no spread
    const long double root = sqrtl(S);
    for (size_t q = 0; q < n; q++) {
      const long double d = ((long double)v[q] - m) - c;
      xhat[q * (size_t)P + (size_t)p] = (n >= 2 && S > 0.0L && std::isfinite((double)S)) ? (double)(d / root) : (S == S ? 0.0 : std::nan(""));
    }
  }
}

// what a call works on: the block of states on the device and its participants
struct MsBlock {
  int64_t K, L;
  const double* d_u;
  int32_t n;
};

void check_shape(kin_network* h, int64_t K, int64_t L) {
  require(K >= 0 && L >= 0, ERR_INVALID_ARG, "K or L < 0");
  require(K < ((int64_t)1 << 31), ERR_UNSUPPORTED, "member statistics: K beyond 32-bit member indices");
  require(L * h->host.N < ((int64_t)1 << 36), ERR_UNSUPPORTED, "member statistics: L N beyond the grid of the moments launch");
}

// the participants on the device (the host copy lives in the handle: the asynchronous upload reads it)
int32_t upload_participants(kin_network* h, std::vector<int32_t> idx, hipStream_t s) {
  h->ms_h_idx = std::move(idx);
  h->ms_idx.upload(h->ms_h_idx, s);
  return (int32_t)h->ms_h_idx.size();
}

// the stored ensemble's participants: the members that completed the save grid, or the caller's mask checked against them
std::vector<int32_t> ensemble_participants(kin_network* h, const int32_t* use) {
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  std::vector<int32_t> idx;
  for (int64_t m = 0; m < h->ens.K; m++) {
    const bool complete = h->ens.n_saved[(size_t)m] == h->ens.cap;
    if (use) require(use[m] == 0 || complete, ERR_INVALID_ARG, "use names a member that did not complete the save grid (n_saved < n_rows)");
    if (use ? use[m] != 0 : complete) idx.push_back((int32_t)m);
  }
  return idx;
}

// the selected species, 0-based on the device; returns n_sel (N for a null list, which selects nothing on the device)
int64_t upload_species(kin_network* h, const int64_t* species, int64_t n_sel, const int32_t** d_sel, hipStream_t s) {
  const int64_t N = h->host.N;
  *d_sel = nullptr;
  if (!species) return N;
  require(n_sel >= 0, ERR_INVALID_ARG, "n_sel < 0");
  h->ms_h_sel.resize((size_t)n_sel);
  for (int64_t i = 0; i < n_sel; i++) {
    const int64_t x = species[i] - h->index_base;
    require(x >= 0 && x < N, ERR_INVALID_ARG, "species index outside the network");
    h->ms_h_sel[(size_t)i] = (int32_t)x;
  }
  h->ms_sel.upload(h->ms_h_sel, s);
  *d_sel = h->ms_sel.p;
  return n_sel;
}

void moments_run(kin_network* h, const MsBlock& b, double* d_mean, double* d_var, double* d_mn, double* d_mx, hipStream_t s) {
  const int64_t C = b.L * h->host.N;
  if (C == 0) return;
  if (b.n == 0) {
    for (double* o : {d_mean, d_var, d_mn, d_mx})
      if (o) KIN_HIP(hipMemsetAsync(o, 0, (size_t)C * sizeof(double), s));
    return;
  }
  launch_ms_moments(MsMomArgs{b.d_u, h->ms_idx.p, b.n, C, C, d_mean, d_var, d_mn, d_mx}, s);
}

// The column passes, block of columns by block: quantiles (Q > 0) and / or correlations with d_xhat[n][P] (P > 0).
void columns_run(kin_network* h, const MsBlock& b, const int32_t* d_sel, int64_t n_sel, int64_t Q, const double* d_p, double* d_quant,
                 int64_t P, bool rank, const double* d_xhat, double* d_corr, hipStream_t s) {
  const int64_t total = b.L * n_sel;
  if (total == 0) return;
  if (b.n == 0) {
    if (Q > 0) KIN_HIP(hipMemsetAsync(d_quant, 0, (size_t)(Q * total) * sizeof(double), s));
    if (P > 0) KIN_HIP(hipMemsetAsync(d_corr, 0, (size_t)(total * P) * sizeof(double), s));
    return;
  }
  const bool sorted = Q > 0 || (P > 0 && rank);
  if (sorted && b.n > MS_MAX_SORTED) {
    char msg[200];
    snprintf(msg, sizeof msg, "member statistics: %d participants; quantiles and rank correlations take at most %d (KIN_MEMBERS_MAX_SORTED)",
             (int)b.n, MS_MAX_SORTED);
    throw KinError(ERR_UNSUPPORTED, msg);
  }
  int64_t nb_max = P > 0 ? std::max<int64_t>(1, (int64_t)(MS_WORK_BYTES / ((size_t)b.n * sizeof(double)))) : total;
  if (const char* e = getenv("KIN_MEMBERS_BLOCK_COLUMNS")) {   // (read per call: tests change it)
    const int64_t v = atoll(e);
    if (v >= 1) nb_max = std::min(nb_max, v);
  }
  nb_max = std::min(nb_max, total);
  if (P > 0) h->ms_yhat.alloc((size_t)nb_max * (size_t)b.n);
  MsColArgs a{};
  a.u = b.d_u; a.idx = h->ms_idx.p; a.sel = d_sel; a.n = b.n; a.N = (int32_t)h->host.N; a.n_sel = (int32_t)n_sel;
  a.stride = b.L * h->host.N; a.c_total = total;
  a.P2 = 2;
  while (a.P2 < b.n) a.P2 <<= 1;
  a.T = sorted ? ms_sorted_tile(a.P2) : 0;
  a.Q = (int32_t)Q; a.p = d_p; a.q_out = Q > 0 ? d_quant : nullptr;
  a.yhat = P > 0 ? h->ms_yhat.p : nullptr;
  for (int64_t c0 = 0; c0 < total; c0 += nb_max) {
    a.c0 = c0; a.nc = std::min(nb_max, total - c0);
    if (sorted) {
      MsColArgs q = a;
      if (!rank) q.yhat = nullptr;
      launch_ms_sorted(q, s);
    }
    if (P > 0 && !rank) launch_ms_values(a, s);
    if (P > 0) launch_ms_corr(a.nc, b.n, (int32_t)P, d_xhat, h->ms_yhat.p, d_corr + (size_t)c0 * (size_t)P, s);
  }
}

void check_probabilities(const double* p, int64_t Q) {
  require(Q >= 0, ERR_INVALID_ARG, "Q < 0");
  require(p != nullptr || Q == 0, ERR_INVALID_ARG, "null probabilities");
  for (int64_t i = 0; i < Q; i++) require(p[i] >= 0.0 && p[i] <= 1.0, ERR_INVALID_ARG, "a probability outside [0, 1]");
}

// quantiles of a block on the device into d_out [Q][L][n_sel]
void quantiles_call(kin_network* h, const MsBlock& b, const int64_t* species, int64_t n_sel, const double* p, int64_t Q, double* d_out,
                    hipStream_t s) {
  const int32_t* d_sel;
  n_sel = upload_species(h, species, n_sel, &d_sel, s);
  require(n_sel < ((int64_t)1 << 31) && b.L * n_sel < ((int64_t)1 << 40), ERR_UNSUPPORTED, "member statistics: too many selected columns");
  h->ms_h_p.assign(p, p + Q);
  h->ms_p.upload(h->ms_h_p, s);
  columns_run(h, b, d_sel, n_sel, Q, h->ms_p.p, d_out, 0, false, nullptr, nullptr, s);
}

// correlations of a block on the device with the host inputs X[K][P] into d_out [L][n_sel][P]
void correlate_call(kin_network* h, const MsBlock& b, const int64_t* species, int64_t n_sel, const double* X, int64_t P, int rank,
                    double* d_out, hipStream_t s) {
  require(P >= 0 && P < ((int64_t)1 << 31), ERR_INVALID_ARG, "P < 0");
  require(X != nullptr || P == 0 || b.K == 0, ERR_INVALID_ARG, "null inputs");
  const int32_t* d_sel;
  n_sel = upload_species(h, species, n_sel, &d_sel, s);
  require(n_sel < ((int64_t)1 << 31) && b.L * n_sel < ((int64_t)1 << 40), ERR_UNSUPPORTED, "member statistics: too many selected columns");
  if (P == 0) return;
  h->ms_h_xhat.resize((size_t)b.n * (size_t)P);
  normalised_inputs(P, X, h->ms_h_idx, rank != 0, h->ms_h_xhat.data());
  h->ms_xhat.upload(h->ms_h_xhat, s);
  columns_run(h, b, d_sel, n_sel, 0, nullptr, nullptr, P, rank != 0, h->ms_xhat.p, d_out, s);
}

// the host entries' block: the states uploaded, the participants on the device
MsBlock host_block(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, hipStream_t s) {
  check_shape(h, K, L);
  const size_t len = (size_t)K * (size_t)L * (size_t)h->host.N;
  require(u != nullptr || len == 0, ERR_INVALID_ARG, "null state buffer");
  h->ms_u.upload(u, len, s);
  return MsBlock{K, L, h->ms_u.p, upload_participants(h, participants(K, use), s)};
}

MsBlock dev_block(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, hipStream_t s) {
  check_shape(h, K, L);
  require(d_u != nullptr || K * L * h->host.N == 0, ERR_INVALID_ARG, "null state buffer");
  return MsBlock{K, L, d_u, upload_participants(h, participants(K, use), s)};
}

MsBlock ensemble_block(kin_network* h, const int32_t* use, hipStream_t s) {
  std::vector<int32_t> idx = ensemble_participants(h, use);
  check_shape(h, h->ens.K, h->ens.cap);
  return MsBlock{h->ens.K, h->ens.cap, h->ens.sol, upload_participants(h, std::move(idx), s)};
}

// moments into host buffers through the handle's staging buffers
void moments_to_host(kin_network* h, const MsBlock& b, int64_t* count, double* mean, double* var, double* mn, double* mx, hipStream_t s) {
  const size_t C = (size_t)(b.L * h->host.N);
  double* host[4] = {mean, var, mn, mx};
  double* dev[4] = {};
  for (int i = 0; i < 4; i++)
    if (host[i]) { h->ms_o[i].alloc(C); dev[i] = h->ms_o[i].p; }
  moments_run(h, b, dev[0], dev[1], dev[2], dev[3], s);
  for (int i = 0; i < 4; i++)
    if (host[i]) h->ms_o[i].download(host[i], C, s);
  KIN_HIP(hipStreamSynchronize(s));
  if (count) *count = b.n;
}

void quantiles_to_host(kin_network* h, const MsBlock& b, const int64_t* species, int64_t n_sel, const double* p, int64_t Q, double* out,
                       hipStream_t s) {
  const int64_t ns = species ? n_sel : h->host.N;
  const size_t len = (size_t)std::max<int64_t>(Q * b.L * ns, 0);
  h->ms_o[0].alloc(len);
  quantiles_call(h, b, species, n_sel, p, Q, h->ms_o[0].p, s);
  h->ms_o[0].download(out, len, s);
  KIN_HIP(hipStreamSynchronize(s));
}

void correlate_to_host(kin_network* h, const MsBlock& b, const int64_t* species, int64_t n_sel, const double* X, int64_t P, int rank,
                       double* out, hipStream_t s) {
  const int64_t ns = species ? n_sel : h->host.N;
  const size_t len = (size_t)std::max<int64_t>(b.L * ns * P, 0);
  h->ms_o[0].alloc(len);
  correlate_call(h, b, species, n_sel, X, P, rank, h->ms_o[0].p, s);
  h->ms_o[0].download(out, len, s);
  KIN_HIP(hipStreamSynchronize(s));
}

// ---- Sobol indices of a Saltelli design -------------------------------------------------------------------------------------
// K = M (P + 2) of a design, checked
int64_t design_members(int64_t M, int64_t P) {
  require(M >= 1 && P >= 1, ERR_INVALID_ARG, "sobol: M or P < 1");
  require(M < ((int64_t)1 << 31) && P < (int64_t)SB_CHUNK * 65535, ERR_UNSUPPORTED, "sobol: M or P beyond the launch's grid");
  return M * (P + 2);
}

// The participating samples and their weights on the device; returns n = sum w. complete: null (every sample may take part) or
// [M], the samples all of whose members completed the save grid - the default weights, and the only ones a caller may name.
int64_t upload_weights(kin_network* h, int64_t M, const int32_t* w, const std::vector<char>* complete, hipStream_t s) {
  std::vector<int32_t> idx, wt;
  int64_t n = 0;
  for (int64_t m = 0; m < M; m++) {
    const bool ok = !complete || (*complete)[(size_t)m];
    if (w) {
      require(w[m] >= 0, ERR_INVALID_ARG, "sobol: a negative weight");
      require(w[m] == 0 || ok, ERR_INVALID_ARG, "sobol: w names a sample with a member that did not complete the save grid (n_saved < n_rows)");
    }
    const int32_t v = w ? w[m] : (ok ? 1 : 0);
    if (v > 0) { idx.push_back((int32_t)m); wt.push_back(v); n += v; }
  }
  h->ms_h_wt = std::move(wt);
  h->ms_wt.upload(h->ms_h_wt, s);
  upload_participants(h, std::move(idx), s);
  return n;
}

// the pass over a block on the device into device outputs (any null)
void sobol_run(kin_network* h, const double* d_u, int64_t M, int64_t P, int64_t L, int64_t n, const int64_t* species, int64_t n_sel,
               double* d_S1, double* d_ST, double* d_mean, double* d_var, hipStream_t s) {
  const int32_t* d_sel;
  n_sel = upload_species(h, species, n_sel, &d_sel, s);
  require(n_sel < ((int64_t)1 << 31) && L * n_sel < ((int64_t)1 << 36), ERR_UNSUPPORTED, "sobol: too many selected columns");
  const int64_t total = L * n_sel;
  if (total == 0) return;
  if (n == 0) {
    for (double* o : {d_S1, d_ST})
      if (o) KIN_HIP(hipMemsetAsync(o, 0, (size_t)(total * P) * sizeof(double), s));
    for (double* o : {d_mean, d_var})
      if (o) KIN_HIP(hipMemsetAsync(o, 0, (size_t)total * sizeof(double), s));
    return;
  }
  SobolArgs a{};
  a.u = d_u; a.idx = h->ms_idx.p; a.wt = h->ms_wt.p; a.sel = d_sel;
  a.np = (int32_t)h->ms_h_idx.size(); a.M = (int32_t)M; a.P = (int32_t)P; a.N = (int32_t)h->host.N; a.n_sel = (int32_t)n_sel;
  a.n = n; a.stride = L * h->host.N; a.c_total = total;
  a.S1 = d_S1; a.ST = d_ST; a.mean = d_mean; a.var = d_var;
  launch_sobol(a, s);
}

void sobol_to_host(kin_network* h, const double* d_u, int64_t M, int64_t P, int64_t L, int64_t n, const int64_t* species, int64_t n_sel,
                   double* S1, double* ST, double* mean, double* var, hipStream_t s) {
  const size_t C = (size_t)std::max<int64_t>(L * (species ? n_sel : h->host.N), 0);
  double* host[4] = {S1, ST, mean, var};
  const size_t len[4] = {C * (size_t)P, C * (size_t)P, C, C};
  double* dev[4] = {};
  for (int i = 0; i < 4; i++)
    if (host[i]) { h->ms_o[i].alloc(len[i]); dev[i] = h->ms_o[i].p; }
  sobol_run(h, d_u, M, P, L, n, species, n_sel, dev[0], dev[1], dev[2], dev[3], s);
  for (int i = 0; i < 4; i++)
    if (host[i]) h->ms_o[i].download(host[i], len[i], s);
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int kin_members_inputs_host(int64_t K, int64_t P, const double* X, const int32_t* use, int rank, int64_t* n, double* Xhat) {
  if (K < 0 || P < 0 || K >= ((int64_t)1 << 31) || (!X && K * P > 0 && Xhat) || (!n && !Xhat)) return KIN_ERR_INVALID_ARG;
  try {     // (host work only: no device call)
    const std::vector<int32_t> idx = participants(K, use);
    if (n) *n = (int64_t)idx.size();
    if (Xhat && P > 0) normalised_inputs(P, X, idx, rank != 0, Xhat);
  } catch (const std::exception&) { return KIN_ERR_INVALID_ARG; }
  return KIN_OK;
}

int kin_members_moments_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, int64_t* count, double* d_mean,
                            double* d_var, double* d_min, double* d_max, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(count || d_mean || d_var || d_min || d_max, ERR_INVALID_ARG, "no output requested");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const MsBlock b = dev_block(h, K, L, d_u, use, s);
  moments_run(h, b, d_mean, d_var, d_min, d_max, s);
  if (count) *count = b.n;
  KIN_CATCH(h)
}

int kin_members_moments(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, int64_t* count, double* mean,
                        double* var, double* min, double* max) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(count || mean || var || min || max, ERR_INVALID_ARG, "no output requested");
  hipStream_t s = h->stream;
  moments_to_host(h, host_block(h, K, L, u, use, s), count, mean, var, min, max, s);
  KIN_CATCH(h)
}

int kin_ensemble_moments(kin_network* h, const int32_t* use, int64_t* count, double* mean, double* var, double* min, double* max) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(count || mean || var || min || max, ERR_INVALID_ARG, "no output requested");
  hipStream_t s = h->stream;
  moments_to_host(h, ensemble_block(h, use, s), count, mean, var, min, max, s);
  KIN_CATCH(h)
}

int kin_members_quantiles_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, const int64_t* species,
                              int64_t n_sel, const double* p, int64_t Q, double* d_out, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(d_out != nullptr, ERR_INVALID_ARG, "null output buffer");
  check_probabilities(p, Q);
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  quantiles_call(h, dev_block(h, K, L, d_u, use, s), species, n_sel, p, Q, d_out, s);
  KIN_CATCH(h)
}

int kin_members_quantiles(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, const int64_t* species,
                          int64_t n_sel, const double* p, int64_t Q, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out != nullptr, ERR_INVALID_ARG, "null output buffer");
  require(!species || n_sel >= 0, ERR_INVALID_ARG, "n_sel < 0");
  check_probabilities(p, Q);
  hipStream_t s = h->stream;
  quantiles_to_host(h, host_block(h, K, L, u, use, s), species, n_sel, p, Q, out, s);
  KIN_CATCH(h)
}

int kin_ensemble_quantiles(kin_network* h, const int32_t* use, const int64_t* species, int64_t n_sel, const double* p, int64_t Q,
                           double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out != nullptr, ERR_INVALID_ARG, "null output buffer");
  require(!species || n_sel >= 0, ERR_INVALID_ARG, "n_sel < 0");
  check_probabilities(p, Q);
  hipStream_t s = h->stream;
  quantiles_to_host(h, ensemble_block(h, use, s), species, n_sel, p, Q, out, s);
  KIN_CATCH(h)
}

int kin_members_correlate_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, const int64_t* species,
                              int64_t n_sel, const double* X, int64_t P, int rank, double* d_out, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(d_out != nullptr, ERR_INVALID_ARG, "null output buffer");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  correlate_call(h, dev_block(h, K, L, d_u, use, s), species, n_sel, X, P, rank, d_out, s);
  KIN_CATCH(h)
}

int kin_members_correlate(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, const int64_t* species,
                          int64_t n_sel, const double* X, int64_t P, int rank, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out != nullptr, ERR_INVALID_ARG, "null output buffer");
  require((!species || n_sel >= 0) && P >= 0, ERR_INVALID_ARG, "n_sel or P < 0");
  hipStream_t s = h->stream;
  correlate_to_host(h, host_block(h, K, L, u, use, s), species, n_sel, X, P, rank, out, s);
  KIN_CATCH(h)
}

int kin_ensemble_correlate(kin_network* h, const int32_t* use, const int64_t* species, int64_t n_sel, const double* X, int64_t P, int rank,
                           double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(out != nullptr, ERR_INVALID_ARG, "null output buffer");
  require((!species || n_sel >= 0) && P >= 0, ERR_INVALID_ARG, "n_sel or P < 0");
  hipStream_t s = h->stream;
  correlate_to_host(h, ensemble_block(h, use, s), species, n_sel, X, P, rank, out, s);
  KIN_CATCH(h)
}

int kin_members_sobol_dev(kin_network* h, int64_t M, int64_t P, int64_t L, const double* d_u, const int32_t* w, const int64_t* species,
                          int64_t n_sel, double* d_S1, double* d_ST, double* d_mean, double* d_var, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(d_S1 || d_ST || d_mean || d_var, ERR_INVALID_ARG, "no output requested");
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  const int64_t K = design_members(M, P);
  check_shape(h, K, L);
  require(d_u != nullptr || L * h->host.N == 0, ERR_INVALID_ARG, "null state buffer");
  const int64_t n = upload_weights(h, M, w, nullptr, s);
  sobol_run(h, d_u, M, P, L, n, species, n_sel, d_S1, d_ST, d_mean, d_var, s);
  KIN_CATCH(h)
}

int kin_members_sobol(kin_network* h, int64_t M, int64_t P, int64_t L, const double* u, const int32_t* w, const int64_t* species,
                      int64_t n_sel, double* S1, double* ST, double* mean, double* var) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(S1 || ST || mean || var, ERR_INVALID_ARG, "no output requested");
  require(!species || n_sel >= 0, ERR_INVALID_ARG, "n_sel < 0");
  hipStream_t s = h->stream;
  const int64_t K = design_members(M, P);
  check_shape(h, K, L);
  const size_t len = (size_t)K * (size_t)L * (size_t)h->host.N;
  require(u != nullptr || len == 0, ERR_INVALID_ARG, "null state buffer");
  const int64_t n = upload_weights(h, M, w, nullptr, s);
  h->ms_u.upload(u, len, s);
  sobol_to_host(h, h->ms_u.p, M, P, L, n, species, n_sel, S1, ST, mean, var, s);
  KIN_CATCH(h)
}

int kin_ensemble_sobol(kin_network* h, int64_t M, int64_t P, const int32_t* w, const int64_t* species, int64_t n_sel, double* S1, double* ST,
                       double* mean, double* var) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(S1 || ST || mean || var, ERR_INVALID_ARG, "no output requested");
  require(!species || n_sel >= 0, ERR_INVALID_ARG, "n_sel < 0");
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  hipStream_t s = h->stream;
  require(design_members(M, P) == h->ens.K, ERR_INVALID_ARG, "sobol: the stored ensemble does not have M (P + 2) members");
  check_shape(h, h->ens.K, h->ens.cap);
  std::vector<char> complete((size_t)M, 1);
  for (int64_t k = 0; k < h->ens.K; k++)
    if (h->ens.n_saved[(size_t)k] != h->ens.cap) complete[(size_t)(k % M)] = 0;
  const int64_t n = upload_weights(h, M, w, &complete, s);
  sobol_to_host(h, h->ens.sol, M, P, h->ens.cap, n, species, n_sel, S1, ST, mean, var, s);
  KIN_CATCH(h)
}

}  // extern "C"
