// extern "C" entry points of the resampling pass (declarations and definitions: include/kinetica_hip.h; kernel:
// resample_kernels.hip). Staging of the host entries and the stored records: flux_api.hpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>

#include "flux_api.hpp"
#include "resample_kernels.hpp"

using namespace kin;

namespace {

// a call's axis x[L] / x[S][L] and queries xq[Q] / xq[S][Q], on the host or on the device
struct ResampleAxes { const double* x; bool x_per; int64_t Q; const double* xq; bool xq_per; };

// what a call asks for besides its states and axes: what an outside query gets and the first row that takes part
struct ResampleOpts { int mode; double fill; int64_t row_begin; };

// the results on the device or, in a host entry, where the caller wants them (jc, w null: not wanted)
struct ResampleOut { double* u; int32_t* jc; double* w; };

// the checks every entry shares; nothing here touches the device or a handle
void resample_check(int64_t S, int64_t L, bool have_u, const ResampleAxes& ax, int64_t row_begin) {
  require(S >= 0 && L >= 0 && ax.Q >= 0, ERR_INVALID_ARG, "S, L or Q < 0");
  require(row_begin >= 0, ERR_INVALID_ARG, "row_begin < 0");
  require(S < ((int64_t)1 << 31) && L < ((int64_t)1 << 31) && ax.Q < ((int64_t)1 << 31), ERR_UNSUPPORTED,
          "resampling: S, L or Q beyond 32-bit offsets");
  require((have_u && ax.x != nullptr) || S * L == 0, ERR_INVALID_ARG, "null state or axis buffer");
  require(ax.xq != nullptr || S * ax.Q == 0, ERR_INVALID_ARG, "null query buffer");
}

// the rest of what an entry with states checks
void resample_check_states(const kin_network* h, int64_t S, const ResampleAxes& ax, const ResampleOpts& o, bool have_out) {
  require(have_out, ERR_INVALID_ARG, "null output buffer");
  require(o.mode == KIN_RESAMPLE_FILL || o.mode == KIN_RESAMPLE_HOLD, ERR_INVALID_ARG, "unknown mode");
  require(h->host.N <= (int64_t)RESAMPLE_LANES * 65535, ERR_UNSUPPORTED, "resampling: N beyond 64 x 65535 species");
  require(S * ceil_div(ax.Q, 4) < ((int64_t)1 << 31), ERR_UNSUPPORTED, "resampling: S Q / 4 beyond the grid's 2^31 workgroups");
}

void check_seg_n(const int64_t* seg_n, int64_t S, int64_t L) {
  if (seg_n) for (int64_t s = 0; s < S; s++) require(seg_n[s] >= 0 && seg_n[s] <= L, ERR_INVALID_ARG, "seg_n outside [0, L]");
}

// x non-decreasing and without a NaN over the rows row_begin .. n - 1 that are read
void check_axis_rows(const double* x, int64_t row_begin, int64_t n) {
  if (row_begin < n) require(x[row_begin] == x[row_begin], ERR_INVALID_ARG, "the axis holds a NaN among the rows read");
  for (int64_t j = row_begin + 1; j < n; j++) require(x[j - 1] <= x[j], ERR_INVALID_ARG, "the axis decreases or holds a NaN among the rows read");
}

void check_axis(const double* x, bool per_segment, int64_t S, int64_t L, const int64_t* seg_n, int64_t row_begin) {
  int64_t longest = 0;
  for (int64_t s = 0; s < S; s++) {
    const int64_t n = seg_n ? seg_n[s] : L;
    if (per_segment) check_axis_rows(x + s * L, row_begin, n);
    longest = std::max(longest, n);
  }
  if (!per_segment) check_axis_rows(x, row_begin, longest);
}

// the bracket of every (segment, query) on host arrays: the rule of resample_kernels.hpp, segment by segment
void bracket_host(int64_t S, int64_t L, const int64_t* seg_n, const ResampleAxes& ax, int64_t row_begin, int32_t* jc, double* w) {
  const int jb = (int)std::min(row_begin, L);
  for (int64_t s = 0; s < S; s++) {
    const int n = (int)(seg_n ? seg_n[s] : L);
    const double* xs = ax.x_per ? ax.x + s * L : ax.x;
    const double* qs = ax.xq_per ? ax.xq + s * ax.Q : ax.xq;
    for (int64_t q = 0; q < ax.Q; q++) {
      double wq;
      const int j = resample_bracket(xs, jb, n, qs[q], &wq);
      if (jc) jc[s * ax.Q + q] = j;
      if (w) w[s * ax.Q + q] = wq;
    }
  }
}

// the pass on device buffers: one launch that writes every out[s][q][:] itself
void resample_run(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const ResampleAxes& dax,
                  const ResampleOpts& o, const ResampleOut& out, hipStream_t s) {
  const int64_t N = h->host.N;
  if (S * dax.Q == 0 || N == 0) return;
  ResampleArgs a{};
  a.N = (int)N; a.L = (int)L; a.Q = (int)dax.Q; a.seg_n = d_seg_n; a.u = d_u;
  a.x = dax.x; a.x_stride = dax.x_per ? L : 0; a.xq = dax.xq; a.xq_stride = dax.xq_per ? dax.Q : 0;
  a.mode = o.mode; a.fill = o.fill;
  a.row_begin = (int)std::min<int64_t>(o.row_begin, L);      // (at or past every n_s: the same empty segments)
  a.out = out.u; a.jc = out.jc; a.w = out.w;
  launch_resample(S, resample_plan(S, dax.Q, N, h->n_cu), a, s);
}

// a host entry's tail: the axes up through f_T and f_w, the run into d_out (null: f_result), the results down; the caller waits
// for the stream
void resample_host_call(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const ResampleAxes& ax,
                        const ResampleOpts& o, double* d_out, const ResampleOut& out, hipStream_t s) {
  const size_t nx = (size_t)(ax.x_per ? S * L : L), nq = (size_t)(ax.xq_per ? S * ax.Q : ax.Q), sq = (size_t)(S * ax.Q);
  const size_t n = sq * (size_t)h->host.N;
  if (S * L > 0) h->f_T.upload(ax.x, nx, s);
  if (sq > 0) h->f_w.upload(ax.xq, nq, s);
  if (!d_out) { h->f_result.alloc(n); d_out = h->f_result.p; }
  if (out.jc) h->rs_jc.alloc(sq);
  if (out.w) h->rs_w.alloc(sq);
  const ResampleAxes dax{h->f_T.p, ax.x_per, ax.Q, h->f_w.p, ax.xq_per};
  resample_run(h, S, L, d_seg_n, d_u, dax, o, ResampleOut{d_out, out.jc ? h->rs_jc.p : nullptr, out.w ? h->rs_w.p : nullptr}, s);
  if (h->host.N > 0) {
    if (out.u && n > 0) KIN_HIP(hipMemcpyAsync(out.u, d_out, n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out.jc) h->rs_jc.download(out.jc, sq, s);
    if (out.w) h->rs_w.download(out.w, sq, s);
  }
}

// the length of the leading run of covered queries of every segment: inside, or under KIN_RESAMPLE_HOLD any query but a NaN
// one of a non-empty segment
std::vector<int64_t> covered_runs(int64_t S, int64_t L, const int64_t* seg_n, const ResampleAxes& ax, const ResampleOpts& o) {
  std::vector<int64_t> run((size_t)S, 0);
  const int64_t jb = std::min(o.row_begin, L);
  for (int64_t s = 0; s < S; s++) {
    const int64_t n = seg_n ? seg_n[s] : L;
    if (n <= jb) continue;
    const double* xs = ax.x_per ? ax.x + s * L : ax.x;
    const double* qs = ax.xq_per ? ax.xq + s * ax.Q : ax.xq;
    int64_t q = 0;
    for (; q < ax.Q; q++) {
      const double v = qs[q];
      if (!(o.mode == KIN_RESAMPLE_HOLD ? v == v : (xs[jb] <= v && v <= xs[n - 1]))) break;
    }
    run[(size_t)s] = q;
  }
  return run;
}

}  // namespace

extern "C" {

int kin_resample_bracket_host(int64_t S, int64_t L, const int64_t* seg_n, const double* x, int x_per_segment, int64_t Q, const double* xq,
                              int xq_per_segment, int64_t row_begin, int32_t* jc, double* w) {
  try {
    const ResampleAxes ax{x, x_per_segment != 0, Q, xq, xq_per_segment != 0};
    resample_check(S, L, true, ax, row_begin);
    require(jc != nullptr || w != nullptr, ERR_INVALID_ARG, "null output buffer");
    check_seg_n(seg_n, S, L);
    if (S * L > 0) check_axis(x, ax.x_per, S, L, seg_n, row_begin);
    bracket_host(S, L, seg_n, ax, row_begin, jc, w);
  } catch (const KinError& e) {
    return e.code;
  } catch (const std::exception&) {
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}

int kin_resample_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const double* d_x,
                               int x_per_segment, int64_t Q, const double* d_xq, int xq_per_segment, int mode, double fill,
                               int64_t row_begin, double* d_out, int32_t* d_jc, double* d_w, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const ResampleAxes dax{d_x, x_per_segment != 0, Q, d_xq, xq_per_segment != 0};
  const ResampleOpts o{mode, fill, row_begin};
  resample_check(S, L, d_u != nullptr, dax, row_begin);
  resample_check_states(h, S, dax, o, d_out != nullptr);
  resample_run(h, S, L, d_seg_n, d_u, dax, o, ResampleOut{d_out, d_jc, d_w}, stream ? (hipStream_t)stream : h->stream);
  KIN_CATCH(h)
}

int kin_resample_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* x, int x_per_segment,
                           int64_t Q, const double* xq, int xq_per_segment, int mode, double fill, int64_t row_begin, double* out,
                           int32_t* jc, double* w) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const ResampleAxes ax{x, x_per_segment != 0, Q, xq, xq_per_segment != 0};
  const ResampleOpts o{mode, fill, row_begin};
  resample_check(S, L, u != nullptr, ax, row_begin);
  resample_check_states(h, S, ax, o, out != nullptr);
  check_seg_n(seg_n, S, L);
  if (S * L > 0) check_axis(x, ax.x_per, S, L, seg_n, row_begin);
  hipStream_t s = h->stream;
  if (S * L > 0) h->f_u.upload(u, (size_t)S * (size_t)L * (size_t)h->host.N, s);
  if (seg_n && S > 0) h->f_segn.upload(seg_n, (size_t)S, s);
  resample_host_call(h, S, L, seg_n ? h->f_segn.p : nullptr, h->f_u.p, ax, o, nullptr, ResampleOut{out, jc, w}, s);
  KIN_HIP(hipStreamSynchronize(s));
  KIN_CATCH(h)
}

int kin_solution_resample(kin_network* h, const double* x, int64_t Q, const double* xq, int mode, double fill, int64_t row_begin, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  const ResampleAxes ax{x ? x : h->sol_t.data(), false, Q, xq, false};
  const ResampleOpts o{mode, fill, row_begin};
  resample_check(1, h->n_saved, true, ax, row_begin);
  resample_check_states(h, 1, ax, o, out != nullptr);
  check_axis_rows(ax.x, row_begin, h->n_saved);
  resample_host_call(h, 1, h->n_saved, nullptr, h->d_sol_u.p, ax, o, nullptr, ResampleOut{out, nullptr, nullptr}, h->stream);
  KIN_HIP(hipStreamSynchronize(h->stream));
  KIN_CATCH(h)
}

int kin_ensemble_resample(kin_network* h, const double* x, int x_per_member, int64_t Q, const double* xq, int xq_per_member, int mode,
                          double fill, int64_t row_begin, int store, double* out) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  const int64_t K = h->ens.K, cap = h->ens.cap, N = h->host.N;
  const ResampleAxes ax{x, x_per_member != 0, Q, xq, xq_per_member != 0};
  const ResampleOpts o{mode, fill, row_begin};
  resample_check(K, cap, true, ax, row_begin);
  resample_check_states(h, K, ax, o, out != nullptr || store != 0);
  require(store == 0 || Q >= 1, ERR_INVALID_ARG, "a stored record needs at least one query (Q >= 1 with store != 0)");
  if (K * cap > 0) check_axis(x, ax.x_per, K, cap, h->ens.n_saved.data(), row_begin);
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  if (!store) {
    resample_host_call(h, K, cap, h->ens_segn.p, h->ens.sol, ax, o, nullptr, ResampleOut{out, nullptr, nullptr}, s);
    KIN_HIP(hipStreamSynchronize(s));
    return OK;
  }
  // the result becomes the record: it goes to the one of the two handle buffers the record does not live in, a member keeps
  // its leading run of covered queries and the rows from its first uncovered query on are zeros, the record's invariant
  std::vector<int64_t> run = covered_runs(K, cap, h->ens.n_saved.data(), ax, o);
  DevBuf<double>& dst = h->ens_rs[h->ens.sol == h->ens_rs[0].p ? 1 : 0];
  dst.alloc((size_t)K * (size_t)Q * (size_t)N);
  resample_host_call(h, K, cap, h->ens_segn.p, h->ens.sol, ax, o, dst.p, ResampleOut{out, nullptr, nullptr}, s);
  if (std::any_of(run.begin(), run.end(), [Q](int64_t r) { return r < Q; })) {      // (after the download of `out` on the stream)
    h->ens_segn.upload(run, s);
    launch_resample_zero_tail(K, Q, N, h->ens_segn.p, dst.p, s);
  }
  KIN_HIP(hipStreamSynchronize(s));      // (run goes into the record below; later passes upload n_saved again)
  h->ens.sol = dst.p; h->ens.cap = Q; h->ens.n_saved = std::move(run);
  KIN_CATCH(h)
}

}  // extern "C"
