// extern "C" entry points of the observables pass (declarations and definitions: include/kinetica_hip.h; kernel:
// observable_kernels.hip). Staging of the host entries and the stored records: flux_api.hpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <cstring>

#include "flux_api.hpp"
#include "observable_kernels.hpp"

#pragma clang fp contract(off)

using namespace kin;

namespace {

// a call's forms (CSR over the species, in the caller's index base) and observables, on the host
struct ObsSpec { int64_t H; const int64_t* ptr; const int64_t* idx; const double* w; int64_t G; const int64_t* num; const int64_t* den; };

constexpr int64_t OBS_LIMIT = (int64_t)1 << 30;

// The checks every entry shares; nothing here touches the device or a handle. Returns the number of form entries.
int64_t obs_check(int64_t N, int index_base, int64_t S, int64_t L, bool have_u, const ObsSpec& f, int64_t pitch, bool have_out) {
  require(N >= 0 && S >= 0 && L >= 0 && f.H >= 0 && f.G >= 0 && pitch >= 0, ERR_INVALID_ARG, "N, S, L, H, G or pitch < 0");
  require(f.ptr != nullptr || f.H == 0, ERR_INVALID_ARG, "null form_ptr");
  const int64_t nnz = f.H > 0 ? f.ptr[f.H] : 0;
  if (f.H > 0) {
    require(f.ptr[0] == 0, ERR_INVALID_ARG, "form_ptr does not start at 0");
    for (int64_t i = 0; i < f.H; i++) require(f.ptr[i] <= f.ptr[i + 1], ERR_INVALID_ARG, "form_ptr decreases");
  }
  require((f.idx != nullptr && f.w != nullptr) || nnz == 0, ERR_INVALID_ARG, "null form_idx or form_w");
  for (int64_t e = 0; e < nnz; e++)
    require(f.idx[e] - index_base >= 0 && f.idx[e] - index_base < N, ERR_INVALID_ARG, "form_idx: species index outside the network");
  require((f.num != nullptr && f.den != nullptr) || f.G == 0, ERR_INVALID_ARG, "null num or den");
  for (int64_t g = 0; g < f.G; g++) {
    require(f.num[g] >= 0 && f.num[g] < f.H, ERR_INVALID_ARG, "num outside [0, H)");
    require(f.den[g] >= -1 && f.den[g] < f.H, ERR_INVALID_ARG, "den outside [-1, H)");
  }
  require(pitch >= f.G, ERR_INVALID_ARG, "pitch < G");
  // (factor by factor: the products of unchecked sizes could overflow)
  require(have_u || S == 0 || L == 0 || N == 0, ERR_INVALID_ARG, "null state buffer");
  require(have_out || S == 0 || L == 0 || pitch == 0, ERR_INVALID_ARG, "null output buffer");
  return nnz;
}

// what the kernel's 32-bit indexing takes
void obs_limits(int64_t N, int64_t S, int64_t L, const ObsSpec& f, int64_t nnz, int64_t pitch) {
  require(S < ((int64_t)1 << 31) && L < ((int64_t)1 << 31) && S * L < ((int64_t)1 << 31), ERR_UNSUPPORTED,
          "observables: S L beyond 32-bit offsets (2^31 rows)");
  require(N < OBS_LIMIT && pitch < OBS_LIMIT && f.H < OBS_LIMIT && f.G < OBS_LIMIT && nnz < OBS_LIMIT, ERR_UNSUPPORTED,
          "observables: N, pitch, H, G or the form entries beyond 2^30");
}

void check_seg_n(const int64_t* seg_n, int64_t S, int64_t L) {
  if (seg_n) for (int64_t s = 0; s < S; s++) require(seg_n[s] >= 0 && seg_n[s] <= L, ERR_INVALID_ARG, "seg_n outside [0, L]");
}

// the value of the form with the entries e0 .. e1 - 1 at the state u: the definition, in plain loops
double form_value(const ObsSpec& f, int index_base, int64_t e0, int64_t e1, const double* u) {
  const int64_t n = e1 - e0;
  if (n == 0) return 0.0;
  auto chain = [&](int64_t first, int64_t step) {      // the short rule over the entries first, first + step, ...
    double acc = f.w[first] * u[f.idx[first] - index_base];
    for (int64_t e = first + step; e < e1; e += step) {
      const double t = f.w[e] * u[f.idx[e] - index_base];
      acc = acc + t;
    }
    return acc;
  };
  if (n <= OBS_SHORT_MAX) return chain(e0, 1);
  double v[64];
  for (int l = 0; l < 64; l++) v[l] = chain(e0 + l, 64);
  for (int off = 32; off >= 1; off /= 2)
    for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
  return v[0];
}

// The plan of the call's forms and observables on the device: the handle's, when the call brings what the last one brought.
void obs_upload_plan(kin_network* h, const ObsSpec& f, int64_t nnz, hipStream_t s) {
  auto same = [](const std::vector<int64_t>& v, const int64_t* p, int64_t n) { return (int64_t)v.size() == n && std::equal(v.begin(), v.end(), p); };
  if (h->ob_ready && same(h->ob_h_ptr, f.ptr, f.H > 0 ? f.H + 1 : 0) && same(h->ob_h_idx, f.idx, nnz) && same(h->ob_h_num, f.num, f.G) &&
      same(h->ob_h_den, f.den, f.G) && (int64_t)h->ob_h_w.size() == nnz &&
      (nnz == 0 || memcmp(h->ob_h_w.data(), f.w, (size_t)nnz * sizeof(double)) == 0))      // (the weights' bits: -0.0 is not 0.0)
    return;
  h->ob_ready = false;
  h->ob_h_ptr.assign(f.ptr, f.ptr + (f.H > 0 ? f.H + 1 : 0));
  h->ob_h_idx.assign(f.idx, f.idx + nnz);
  h->ob_h_w.assign(f.w, f.w + nnz);
  h->ob_h_num.assign(f.num, f.num + f.G);
  h->ob_h_den.assign(f.den, f.den + f.G);
  std::vector<int32_t> idx0((size_t)nnz);
  for (int64_t e = 0; e < nnz; e++) idx0[(size_t)e] = (int32_t)(f.idx[e] - h->index_base);
  h->ob_plan = observable_plan(f.ptr, idx0, f.w, f.G, f.num, f.den);
  h->ob_idx.upload(h->ob_plan.idx, s);
  h->ob_w.upload(h->ob_plan.w, s);
  h->ob_tasks.upload(h->ob_plan.tasks, s);
  h->ob_phases.upload(h->ob_plan.phases, s);
  h->ob_ready = true;
}

// the pass on device buffers: one launch that writes every out[s][j][:] itself
void obs_run(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const ObsSpec& f, int64_t nnz, int64_t pitch,
             double* d_out, hipStream_t s) {
  if (S * L == 0 || pitch == 0) return;
  obs_upload_plan(h, f, nnz, s);
  ObsArgs a{};
  a.N = (int)h->host.N; a.L = (int)L; a.G = (int)f.G; a.pitch = (int)pitch; a.rows_total = S * L;
  a.n_phases = (int)h->ob_plan.phases.size();
  a.seg_n = d_seg_n; a.u = d_u; a.idx = h->ob_idx.p; a.w = h->ob_w.p; a.tasks = h->ob_tasks.p; a.phases = h->ob_phases.p; a.out = d_out;
  launch_observables(observable_launch_plan(h->host.N), a, s);
}

// a host entry's tail: the run into d_out (null: f_result) and the result down; the caller waits for the stream
void obs_host_call(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const ObsSpec& f, int64_t nnz,
                   int64_t pitch, double* d_out, double* out, hipStream_t s) {
  const size_t n = (size_t)(S * L) * (size_t)pitch;
  if (!d_out) { h->f_result.alloc(n); d_out = h->f_result.p; }
  obs_run(h, S, L, d_seg_n, d_u, f, nnz, pitch, d_out, s);
  if (out && n > 0) KIN_HIP(hipMemcpyAsync(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, s));
}

}  // namespace

extern "C" {

int kin_observables_host(int64_t N, int index_base, int64_t S, int64_t L, const int64_t* seg_n, const double* u, int64_t H,
                         const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                         const int64_t* den, int64_t pitch, double* out) {
  try {
    const ObsSpec f{H, form_ptr, form_idx, form_w, G, num, den};
    obs_check(N, index_base, S, L, u != nullptr, f, pitch, out != nullptr);
    check_seg_n(seg_n, S, L);
    // (per observable, as the kernel does: a form nobody names is never evaluated, a form named twice gives the same bits twice)
    auto F = [&](int64_t i, const double* uj) { return form_value(f, index_base, form_ptr[i], form_ptr[i + 1], uj); };
    for (int64_t s = 0; s < S; s++) {
      const int64_t n = seg_n ? seg_n[s] : L;
      for (int64_t j = 0; j < L; j++) {
        double* o = out + (size_t)(s * L + j) * (size_t)pitch;
        for (int64_t c = 0; c < pitch; c++) o[c] = 0.0;
        if (j >= n) continue;
        const double* uj = u + (size_t)(s * L + j) * (size_t)N;
        for (int64_t g = 0; g < G; g++) o[g] = den[g] < 0 ? F(num[g], uj) : F(num[g], uj) / F(den[g], uj);
      }
    }
  } catch (const KinError& e) {
    return e.code;
  } catch (const std::exception&) {
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}

int kin_observables_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, int64_t H,
                                  const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                                  const int64_t* den, int64_t pitch, double* d_out, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const ObsSpec f{H, form_ptr, form_idx, form_w, G, num, den};
  const int64_t nnz = obs_check(h->host.N, h->index_base, S, L, d_u != nullptr, f, pitch, d_out != nullptr);
  obs_limits(h->host.N, S, L, f, nnz, pitch);
  obs_run(h, S, L, d_seg_n, d_u, f, nnz, pitch, d_out, stream ? (hipStream_t)stream : h->stream);
  KIN_CATCH(h)
}

int kin_observables_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, int64_t H,
                              const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                              const int64_t* den, int64_t pitch, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const ObsSpec f{H, form_ptr, form_idx, form_w, G, num, den};
  const int64_t nnz = obs_check(h->host.N, h->index_base, S, L, u != nullptr, f, pitch, out != nullptr);
  obs_limits(h->host.N, S, L, f, nnz, pitch);
  check_seg_n(seg_n, S, L);
  hipStream_t s = h->stream;
  if (S * L > 0) h->f_u.upload(u, (size_t)(S * L) * (size_t)h->host.N, s);
  if (seg_n && S > 0) h->f_segn.upload(seg_n, (size_t)S, s);
  obs_host_call(h, S, L, seg_n ? h->f_segn.p : nullptr, h->f_u.p, f, nnz, pitch, nullptr, out, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_solution_observables(kin_network* h, int64_t H, const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G,
                             const int64_t* num, const int64_t* den, int64_t pitch, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  const ObsSpec f{H, form_ptr, form_idx, form_w, G, num, den};
  const int64_t nnz = obs_check(h->host.N, h->index_base, 1, h->n_saved, true, f, pitch, out != nullptr);
  obs_limits(h->host.N, 1, h->n_saved, f, nnz, pitch);
  obs_host_call(h, 1, h->n_saved, nullptr, h->d_sol_u.p, f, nnz, pitch, nullptr, out, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_ensemble_observables(kin_network* h, int64_t H, const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G,
                             const int64_t* num, const int64_t* den, int64_t pitch, int store, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  const int64_t K = h->ens.K, cap = h->ens.cap, N = h->host.N;
  const ObsSpec f{H, form_ptr, form_idx, form_w, G, num, den};
  const int64_t nnz = obs_check(N, h->index_base, K, cap, true, f, pitch, out != nullptr || store != 0);
  obs_limits(N, K, cap, f, nnz, pitch);
  require(store == 0 || (pitch == N && G >= 1), ERR_INVALID_ARG,
          "a stored record of observables needs pitch == N and 1 <= G <= N (store != 0)");
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  if (!store) {
    obs_host_call(h, K, cap, h->ens_segn.p, h->ens.sol, f, nnz, pitch, nullptr, out, s);
    KIN_HIP(hipStreamSynchronize(s));
    return OK;
  }
  // the result becomes the record: it goes to the one of the two handle buffers the record does not live in; K, n_rows and
  // n_saved stay, and the rows past a member's saved ones are zeros as the pass writes them, the record's invariant
  DevBuf<double>& dst = h->ens_rs[h->ens.sol == h->ens_rs[0].p ? 1 : 0];
  dst.alloc((size_t)(K * cap) * (size_t)N);
  obs_host_call(h, K, cap, h->ens_segn.p, h->ens.sol, f, nnz, pitch, dst.p, out, s);
  KIN_HIP(hipStreamSynchronize(s));
  h->ens.sol = dst.p; h->ens.observables = G;
  KIN_CATCH(h)
}

int kin_ensemble_observable_count(const kin_network* h, int64_t* G) {
  if (!h || !G) return KIN_ERR_INVALID_ARG;
  if (!h->ens.valid()) {
    const_cast<kin_network*>(h)->err = "no ensemble stored (kin_solve_ensemble* first)";
    return KIN_ERR_STATE;
  }
  *G = h->ens.observables;
  return KIN_OK;
}

}  // extern "C"
