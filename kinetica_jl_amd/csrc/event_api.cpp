// extern "C" entry points of the event-time pass (declarations and definitions: include/kinetica_hip.h; kernel:
// event_kernels.hip). Staging of the host entries and the stored records: flux_api.hpp.
#include "../../include/kinetica_hip.h"

#include <algorithm>

#include "event_kernels.hpp"
#include "flux_api.hpp"

using namespace kin;

namespace {

// what a call asks for besides its states: the level's kind, the crossing's direction, where the search starts, the first row
// that takes part and the value of a time that does not exist
struct EventOpts { int kind, direction, start; int64_t row_begin; double never; };

// the three results [S][N] on the device or, in a host entry, where the caller wants them (null: not wanted)
struct EventOut { double *u_peak, *t_peak, *t_cross; };

// the checks every entry shares; nothing here touches the device or the handle
void event_check(const kin_network* h, int64_t S, int64_t L, bool have_t, bool have_level, const EventOpts& o, const EventOut& out) {
  require(S >= 0 && L >= 0, ERR_INVALID_ARG, "S or L < 0");
  require(L < ((int64_t)1 << 31) && S < ((int64_t)1 << 31), ERR_UNSUPPORTED, "event pass: S or L beyond 32-bit offsets");
  require(out.u_peak || out.t_peak || out.t_cross, ERR_INVALID_ARG, "none of u_peak, t_peak, t_cross requested");
  require(o.direction != 0, ERR_INVALID_ARG, "direction == 0 (positive: rising, negative: falling)");
  require(o.kind == KIN_LEVEL_ABS || o.kind == KIN_LEVEL_OF_PEAK || o.kind == KIN_LEVEL_OF_START, ERR_INVALID_ARG, "unknown level_kind");
  require(o.start == KIN_FROM_BEGIN || o.start == KIN_FROM_PEAK, ERR_INVALID_ARG, "unknown start");
  require(o.row_begin >= 0, ERR_INVALID_ARG, "row_begin < 0");
  require(have_level || !out.t_cross || h->host.N == 0, ERR_INVALID_ARG, "t_cross requested without a level");
  require(have_t || S * L == 0, ERR_INVALID_ARG, "null time buffer");
  require(h->host.N <= (int64_t)EVENT_LANES * 65535, ERR_UNSUPPORTED, "event pass: N beyond the grid's 65535 slices of 64 species");
}

// t strictly increasing over the rows row_begin .. n - 1 that are read (a NaN is refused with them)
void check_times(const double* t, int64_t row_begin, int64_t n) {
  for (int64_t j = row_begin + 1; j < n; j++) require(t[j - 1] < t[j], ERR_INVALID_ARG, "t is not strictly increasing over the rows read");
}

void check_seg_times(const double* t, bool per_segment, int64_t S, int64_t L, const int64_t* seg_n, int64_t row_begin) {
  int64_t longest = 0;
  for (int64_t s = 0; s < S; s++) {
    const int64_t n = seg_n ? seg_n[s] : L;
    if (per_segment) check_times(t + s * L, row_begin, n);
    longest = std::max(longest, n);
  }
  if (!per_segment) check_times(t, row_begin, longest);
}

// the pass on device buffers: one launch that writes every requested [S][N] itself, empty segments included
void event_run(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const double* d_t, bool per_segment,
               const double* d_level, const EventOpts& o, const EventOut& out, hipStream_t s) {
  const int64_t N = h->host.N;
  if (S == 0 || N == 0) return;
  EventArgs a{};
  a.N = (int)N; a.L = (int)L; a.seg_n = d_seg_n; a.u = d_u; a.t = d_t; a.t_stride = per_segment ? L : 0;
  a.level = d_level; a.kind = o.kind; a.direction = o.direction > 0 ? 1 : -1; a.start = o.start;
  a.row_begin = (int)std::min<int64_t>(o.row_begin, L);      // (at or past every n_s: the same empty segments)
  a.never = o.never; a.u_peak = out.u_peak; a.t_peak = out.t_peak; a.t_cross = out.t_cross;
  launch_events(S, event_plan(S, L, N, h->n_cu), a, s);
}

// a host entry's tail: level and times up (d_t null: t goes through f_T), the results staged through f_result
void event_host_call(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const double* t, bool per_segment,
                     const double* level, const EventOpts& o, const EventOut& out, hipStream_t s) {
  const size_t n = (size_t)S * (size_t)h->host.N, nt = (size_t)(per_segment ? S * L : L);
  if (nt > 0) h->f_T.upload(t, nt, s);
  if (level && h->host.N > 0) h->f_w.upload(level, (size_t)h->host.N, s);
  h->f_result.alloc(3 * n);
  double* const d = h->f_result.p;
  const EventOut dev{out.u_peak ? d : nullptr, out.t_peak ? d + n : nullptr, out.t_cross ? d + 2 * n : nullptr};
  event_run(h, S, L, d_seg_n, d_u, h->f_T.p, per_segment, level ? h->f_w.p : nullptr, o, dev, s);
  if (out.u_peak) h->f_result.download(out.u_peak, n, s);
  if (out.t_peak) KIN_HIP(hipMemcpyAsync(out.t_peak, d + n, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (out.t_cross) KIN_HIP(hipMemcpyAsync(out.t_cross, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, s));
  KIN_HIP(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int kin_events_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u, const double* d_t,
                             int t_per_segment, const double* d_level, int level_kind, int direction, int start, int64_t row_begin,
                             double never, double* d_u_peak, double* d_t_peak, double* d_t_cross, void* stream) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const EventOpts o{level_kind, direction, start, row_begin, never};
  const EventOut out{d_u_peak, d_t_peak, d_t_cross};
  event_check(h, S, L, d_t != nullptr, d_level != nullptr, o, out);
  require(d_u != nullptr || S * L == 0, ERR_INVALID_ARG, "null state buffer");
  event_run(h, S, L, d_seg_n, d_u, d_t, t_per_segment != 0, d_level, o, out, stream ? (hipStream_t)stream : h->stream);
  KIN_CATCH(h)
}

int kin_events_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* t, int t_per_segment,
                         const double* level, int level_kind, int direction, int start, int64_t row_begin, double never,
                         double* u_peak, double* t_peak, double* t_cross) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  const EventOpts o{level_kind, direction, start, row_begin, never};
  const EventOut out{u_peak, t_peak, t_cross};
  event_check(h, S, L, t != nullptr, level != nullptr, o, out);
  require(u != nullptr || S * L == 0, ERR_INVALID_ARG, "null state buffer");
  if (seg_n) for (int64_t i = 0; i < S; i++) require(seg_n[i] >= 0 && seg_n[i] <= L, ERR_INVALID_ARG, "seg_n outside [0, L]");
  if (S * L > 0) check_seg_times(t, t_per_segment != 0, S, L, seg_n, row_begin);
  hipStream_t s = h->stream;
  if (S * L > 0) h->f_u.upload(u, (size_t)S * (size_t)L * (size_t)h->host.N, s);
  if (seg_n && S > 0) h->f_segn.upload(seg_n, (size_t)S, s);
  event_host_call(h, S, L, seg_n ? h->f_segn.p : nullptr, h->f_u.p, t, t_per_segment != 0, level, o, out, s);
  KIN_CATCH(h)
}

int kin_ensemble_events(kin_network* h, const double* t, int t_per_member, const double* level, int level_kind, int direction, int start,
                        int64_t row_begin, double never, double* u_peak, double* t_peak, double* t_cross) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->ens.valid(), ERR_STATE, "no ensemble stored (kin_solve_ensemble* first)");
  const int64_t K = h->ens.K, cap = h->ens.cap;
  const EventOpts o{level_kind, direction, start, row_begin, never};
  const EventOut out{u_peak, t_peak, t_cross};
  event_check(h, K, cap, t != nullptr, level != nullptr, o, out);
  if (K * cap > 0) check_seg_times(t, t_per_member != 0, K, cap, h->ens.n_saved.data(), row_begin);
  hipStream_t s = h->stream;
  h->ens_segn.upload(h->ens.n_saved, s);
  event_host_call(h, K, cap, h->ens_segn.p, h->ens.sol, t, t_per_member != 0, level, o, out, s);
  KIN_CATCH(h)
}

int kin_solution_events(kin_network* h, const double* level, int level_kind, int direction, int start, int64_t row_begin, double never,
                        double* u_peak, double* t_peak, double* t_cross) {
  if (!h) return KIN_ERR_INVALID_ARG;
  KIN_TRY(h)
  require(h->n_saved > 0, ERR_STATE, "no solution stored");
  const EventOpts o{level_kind, direction, start, row_begin, never};
  const EventOut out{u_peak, t_peak, t_cross};
  event_check(h, 1, h->n_saved, true, level != nullptr, o, out);
  check_times(h->sol_t.data(), row_begin, h->n_saved);
  event_host_call(h, 1, h->n_saved, nullptr, h->d_sol_u.p, h->sol_t.data(), false, level, o, out, h->stream);
  KIN_CATCH(h)
}

}  // extern "C"
