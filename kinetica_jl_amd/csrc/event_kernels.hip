// Event times over stored trajectories: for every segment s (an ensemble member, the one trajectory of a solve) and species i
// the peak over the segment's rows, the time of the first row that holds it and the time at which the species first crosses a
// level, by the chord between the two saved rows around the crossing (definitions: include/kinetica_hip.h).
//
// One launch. A workgroup owns (segment, 64 species): the lanes run along the species, so a wavefront's load of a row is 512
// contiguous bytes, and the workgroup's wavefronts (4, 8 or 16, all on the same 64 species) split the segment's rows: the rows
// from row_begin on are cut into parts of part_rows rows and part p goes to wavefront p % waves, which walks its parts in
// order, EVENT_ROWS_IN_FLIGHT loads issued ahead of their use. Every output is an extremum or a first index, so the wavefronts'
// results combine exactly: "larger value, then smaller row" for the peak, "smaller row" for the crossing, through LDS, no
// atomics; the result does not depend on waves or part_rows. A level and a search start known in advance (KIN_LEVEL_ABS,
// KIN_LEVEL_OF_START with KIN_FROM_BEGIN) are searched in the pass that finds the peak: one read of the states. A level or a
// start that depends on the peak is searched in a second walk by the same workgroup, parts that end before the earliest
// peak row of the wavefront's 64 species skipped: the (segment, 64 species) slab it has just read - rows x 512 bytes, a few
// hundred KB at ensemble sizes - comes from L2. The chord needs the row before the crossing, which may belong to another
// wavefront's part: the crossing row is found first and wavefront 0 reads the two rows around it at the end.
//
// The chord is evaluated in the documented order, every operation rounded on its own: the file is compiled with floating-point
// contraction off (the pragma below), so neither level * peak - a nor t + f * dt becomes a fused multiply-add; the division is
// hipcc's IEEE double division.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "../../include/kinetica_hip.h"
#include "event_kernels.hpp"

#pragma clang fp contract(off)

namespace kin {

namespace {

__device__ __forceinline__ bool event_met(double x, double l, bool rising) { return rising ? x >= l : x <= l; }

// the first row of this wavefront's parts (lane: its species) with j >= j0 that meets the level; INT_MAX: none. PEAK: the peak
// value and its first row are found in the same walk (j0 and l then hold for the walk only when SEARCH)
template <bool PEAK, bool SEARCH>
__device__ __forceinline__ void event_walk(const EventArgs& a, const double* __restrict__ us, bool live, int jb, int n, int w, int W,
                                           int skip_below, double l, int j0, bool rising, double& pv, int& pr, int& cr) {
  const int C = a.part_rows;
  const int nparts = (int)(((long long)(n - jb) + C - 1) / C);
  for (int p = w; p < nparts; p += W) {
    const long long q0 = (long long)jb + (long long)p * C;
    const int p0 = (int)q0, p1 = (int)(q0 + C < n ? q0 + C : n);
    if (!PEAK && p1 <= skip_below) continue;      // (the same in every lane)
    for (int j = p0; j < p1; j += EVENT_ROWS_IN_FLIGHT) {
      double x[EVENT_ROWS_IN_FLIGHT];
#pragma unroll
      for (int q = 0; q < EVENT_ROWS_IN_FLIGHT; q++) x[q] = (live && j + q < p1) ? us[(size_t)(j + q) * a.N] : 0.0;
#pragma unroll
      for (int q = 0; q < EVENT_ROWS_IN_FLIGHT; q++) {
        if (j + q >= p1) break;
        if (PEAK) {
          if (pr == INT_MAX || x[q] > pv) pr = j + q;
          pv = fmax(pv, x[q]);      // (from NaN, "no row yet": the first row's value, then seg_max_kernel's chain)
        }
        if (SEARCH && cr == INT_MAX && j + q >= j0 && event_met(x[q], l, rising)) cr = j + q;
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(EVENT_WAVES_MAX * 64) void event_kernel(EventArgs a) {
  __shared__ double sh_v[EVENT_WAVES_MAX][EVENT_LANES];
  __shared__ int sh_r[EVENT_WAVES_MAX][EVENT_LANES];
  __shared__ int sh_c[EVENT_WAVES_MAX][EVENT_LANES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
  const int i = blockIdx.y * EVENT_LANES + lane;
  const bool live = i < a.N;
  const size_t seg = blockIdx.x;
  long long nn = a.seg_n ? a.seg_n[seg] : a.L;
  const int n = (int)(nn < 0 ? 0 : (nn > a.L ? a.L : nn));
  const int jb = a.row_begin;
  const size_t o = seg * (size_t)a.N + (size_t)i;
  if (n <= jb) {      // an empty segment (the same in every lane): nothing is read
    if (live && w == 0) {
      if (a.u_peak) a.u_peak[o] = 0.0;
      if (a.t_peak) a.t_peak[o] = a.never;
      if (a.t_cross) a.t_cross[o] = a.never;
    }
    return;
  }
  const double* us = a.u + seg * (size_t)a.L * (size_t)a.N + (size_t)i;      // (dereferenced by live lanes only)
  const double* ts = a.t + seg * (size_t)a.t_stride;
  const bool rising = a.direction > 0, want_cross = a.t_cross != nullptr;
  const bool second_walk = want_cross && (a.kind == KIN_LEVEL_OF_PEAK || a.start == KIN_FROM_PEAK);
  double l = 0.0;
  if (want_cross && live) {
    l = a.level[i];
    if (a.kind == KIN_LEVEL_OF_START) l = l * us[(size_t)jb * a.N];
  }

  // the peak and, where level and start are known, the crossing row: one walk
  double pv = __builtin_nan("");
  int pr = INT_MAX, cr = INT_MAX;
  if (want_cross && !second_walk) event_walk<true, true>(a, us, live, jb, n, w, W, 0, l, jb, rising, pv, pr, cr);
  else event_walk<true, false>(a, us, live, jb, n, w, W, 0, l, jb, rising, pv, pr, cr);
  sh_v[w][lane] = pv; sh_r[w][lane] = pr;
  if (!second_walk) sh_c[w][lane] = cr;
  __syncthreads();
  double bv = 0.0;
  int br = INT_MAX;
  for (int ww = 0; ww < W; ww++) {      // larger value, then smaller row (every wavefront forms the same)
    const int r = sh_r[ww][lane];
    if (r == INT_MAX) continue;         // a wavefront without a part
    const double v = sh_v[ww][lane];
    const bool first = br == INT_MAX;
    if (first || v > bv || (v == bv && r < br)) br = r;
    bv = first ? v : fmax(bv, v);
  }

  if (second_walk) {
    if (a.kind == KIN_LEVEL_OF_PEAK && live) l = a.level[i] * bv;
    const int j0 = a.start == KIN_FROM_PEAK ? br : jb;
    int lo = live ? j0 : INT_MAX;       // the earliest search start of the wavefront's species: parts that end before it hold nothing
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lo = min(lo, __shfl_xor(lo, off, 64));
    cr = INT_MAX;
    event_walk<false, true>(a, us, live, jb, n, w, W, lo, l, j0, rising, pv, pr, cr);
    sh_c[w][lane] = cr;
    __syncthreads();
  }
  if (w != 0 || !live) return;

  if (a.u_peak) a.u_peak[o] = bv;
  if (a.t_peak) a.t_peak[o] = ts[br];
  if (!want_cross) return;
  int jc = INT_MAX;
  for (int ww = 0; ww < W; ww++) jc = min(jc, sh_c[ww][lane]);
  const int j0 = a.start == KIN_FROM_PEAK ? br : jb;
  double tc = a.never;
  if (jc == j0) tc = ts[j0];
  else if (jc != INT_MAX) {
    const double ua = us[(size_t)(jc - 1) * a.N], ub = us[(size_t)jc * a.N], ta = ts[jc - 1], tb = ts[jc];
    const double num = l - ua, den = ub - ua, dt = tb - ta;
    const double f = num / den;
    const double step = f * dt;
    tc = ta + step;
  }
  a.t_cross[o] = tc;
}

EventPlan event_plan(int64_t S, int64_t L, int64_t N, int n_cu) {
  // enough wavefronts to keep every compute unit's loads in flight: four per workgroup when the segments alone give them,
  // up to sixteen for a few long segments (one trajectory of many species)
  const int64_t groups = S * ceil_div(N, EVENT_LANES), want = (int64_t)8 * std::max(n_cu, 1);
  int waves = groups * 4 >= want ? 4 : (groups * 8 >= want ? 8 : EVENT_WAVES_MAX);
  if (const char* e = getenv("KIN_EVENT_WAVES")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= EVENT_WAVES_MAX) waves = (int)v;
  }
  int64_t rows = std::max<int64_t>(EVENT_ROWS_IN_FLIGHT, ceil_div(ceil_div(std::max<int64_t>(L, 1), waves), EVENT_ROWS_IN_FLIGHT) * EVENT_ROWS_IN_FLIGHT);
  if (const char* e = getenv("KIN_EVENT_PART_ROWS")) {
    const long long v = atoll(e);
    if (v >= 1) rows = std::min<int64_t>(rows, v);
  }
  return EventPlan{waves, (int)std::min<int64_t>(rows, INT_MAX)};
}

void launch_events(int64_t S, const EventPlan& plan, const EventArgs& a, hipStream_t s) {
  if (S == 0 || a.N == 0) return;
  EventArgs b = a;
  b.part_rows = plan.part_rows;
  hipLaunchKernelGGL(event_kernel, dim3((unsigned)S, (unsigned)ceil_div(a.N, EVENT_LANES)), dim3((unsigned)plan.waves * 64), 0, s, b);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
