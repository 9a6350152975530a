// Resampling of stored trajectories: for every segment s (an ensemble member, the one trajectory of a solve) and query q the
// state at the query point xq of the segment's axis x - a saved row copied bit for bit where the axis holds the query, else the
// chord between the two saved rows around it (definitions: include/kinetica_hip.h).
//
// One launch, no atomics. A workgroup owns (segment, a tile of queries, a slice of 1024 species). First its threads search one
// query each - a bisection over the segment's axis, lane-parallel, about log2 L dependent loads per thread and not per species -
// and leave (jc, w) in LDS. After one barrier the wavefronts deal the tile's queries out among themselves: a wavefront reads the
// one or two rows of its query with the lanes along the species, 512 contiguous bytes per wave instruction, four of them issued
// before the first is used, and writes the query's row the same way. Neighbouring queries of a tile read the same or neighbouring
// rows: a row is fetched from memory once and comes from L2 afterwards. A network of more than 1024 species has several slices,
// each of which repeats the tile's searches (amortised over 1024 species); slice 0 writes jc and w.
//
// The chord is evaluated in the documented order, every operation rounded on its own: the file is compiled with floating-point
// contraction off (the pragma below), so a + w * (b - a) does not become a fused multiply-add; the division is hipcc's IEEE
// double division. A copied row goes through a double register untouched: its bits, -0.0 and NaN payloads included.
#include <algorithm>
#include <cstdlib>

#include "../../include/kinetica_hip.h"
#include "resample_kernels.hpp"

#pragma clang fp contract(off)

namespace kin {

namespace {

constexpr int RESAMPLE_IN_FLIGHT = 4;      // species chunks of 64 whose loads are issued before the first is used

// what a query's row is made of: `fill`, a copy of row `row`, or the chord between rows row - 1 and row
enum : int { RS_FILL = 0, RS_COPY = 1, RS_CHORD = 2 };

}  // namespace

__global__ __launch_bounds__(RESAMPLE_WAVES_MAX * 64) void resample_kernel(ResampleArgs a) {
  __shared__ int sh_row[RESAMPLE_TILE_MAX];
  __shared__ int sh_kind[RESAMPLE_TILE_MAX];
  __shared__ double sh_w[RESAMPLE_TILE_MAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = blockDim.x >> 6;
  const size_t seg = blockIdx.x / (unsigned)a.tiles;
  const int q0 = (int)(blockIdx.x % (unsigned)a.tiles) * a.tile;
  const int nq = min(a.tile, a.Q - q0);
  long long nn = a.seg_n ? a.seg_n[seg] : a.L;
  const int n = (int)(nn < 0 ? 0 : (nn > a.L ? a.L : nn));
  const int jb = a.row_begin;
  const double* xs = a.x + seg * (size_t)a.x_stride;        // (rows jb .. n - 1 are dereferenced, nothing else)
  const double* xqs = a.xq + seg * (size_t)a.xq_stride;

  // the brackets of the tile's queries, one per thread
  for (int t = threadIdx.x; t < nq; t += blockDim.x) {
    double w;
    const double v = xqs[q0 + t];
    const int jc = resample_bracket(xs, jb, n, v, &w);
    int kind = RS_FILL, row = 0;
    if (jc >= 0) { kind = xs[jc] == v ? RS_COPY : RS_CHORD; row = jc; }
    else if (a.mode == KIN_RESAMPLE_HOLD && jc != RESAMPLE_NONE) { kind = RS_COPY; row = jc == RESAMPLE_BELOW ? jb : n - 1; }
    sh_row[t] = row; sh_kind[t] = kind; sh_w[t] = w;
    if (blockIdx.y == 0) {
      const size_t o = seg * (size_t)a.Q + (size_t)(q0 + t);
      if (a.jc) a.jc[o] = jc;
      if (a.w) a.w[o] = w;
    }
  }
  __syncthreads();

  const int i0 = blockIdx.y * RESAMPLE_SLICE, i1 = min(a.N, i0 + RESAMPLE_SLICE);
  const double* us = a.u + seg * (size_t)a.L * (size_t)a.N;
  double* outs = a.out + (seg * (size_t)a.Q + (size_t)q0) * (size_t)a.N;
  for (int t = wv; t < nq; t += W) {      // (t, and with it kind, row and w, is the same in every lane)
    const int kind = sh_kind[t], row = sh_row[t];
    const double w = sh_w[t];
    double* o = outs + (size_t)t * a.N;
    if (kind == RS_FILL) {
      for (int i = i0 + lane; i < i1; i += RESAMPLE_LANES) o[i] = a.fill;
      continue;
    }
    const double* rb = us + (size_t)row * a.N;
    const double* ra = kind == RS_CHORD ? rb - a.N : rb;      // (a copy reads its one row twice: the second load hits)
    for (int i = i0 + lane; i < i1; i += RESAMPLE_LANES * RESAMPLE_IN_FLIGHT) {
      double va[RESAMPLE_IN_FLIGHT], vb[RESAMPLE_IN_FLIGHT];
#pragma unroll
      for (int c = 0; c < RESAMPLE_IN_FLIGHT; c++) {
        const int ii = i + c * RESAMPLE_LANES;
        const bool live = ii < i1;
        vb[c] = live ? rb[ii] : 0.0;
        va[c] = live && kind == RS_CHORD ? ra[ii] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < RESAMPLE_IN_FLIGHT; c++) {
        const int ii = i + c * RESAMPLE_LANES;
        if (ii >= i1) break;
        double r = vb[c];
        if (kind == RS_CHORD) {
          const double d = vb[c] - va[c];
          const double p = w * d;
          r = va[c] + p;
        }
        o[ii] = r;
      }
    }
  }
}

__global__ __launch_bounds__(256) void resample_zero_tail_kernel(int Q, int N, const int64_t* __restrict__ keep_n, double* __restrict__ out) {
  const size_t seg = blockIdx.x;
  long long k = keep_n[seg];
  k = k < 0 ? 0 : (k > Q ? Q : k);
  const size_t len = (size_t)(Q - k) * (size_t)N;
  double* o = out + (seg * (size_t)Q + (size_t)k) * (size_t)N;
  for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.y * blockDim.x) o[i] = 0.0;
}

ResamplePlan resample_plan(int64_t S, int64_t Q, int64_t N, int n_cu) {
  // tiles of 32 queries on 4 wavefronts; smaller tiles while the grid would leave compute units without a workgroup
  const int64_t slices = ceil_div(std::max<int64_t>(N, 1), RESAMPLE_SLICE), want = (int64_t)2 * std::max(n_cu, 1);
  int tile = 32;
  while (tile > 4 && S * ceil_div(std::max<int64_t>(Q, 1), tile) * slices < want) tile /= 2;
  int waves = 4;
  if (const char* e = getenv("KIN_RESAMPLE_TILE_QUERIES")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= RESAMPLE_TILE_MAX) tile = (int)v;
  }
  if (const char* e = getenv("KIN_RESAMPLE_WAVES")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= RESAMPLE_WAVES_MAX) waves = (int)v;
  }
  return ResamplePlan{tile, waves};
}

void launch_resample(int64_t S, const ResamplePlan& plan, const ResampleArgs& a, hipStream_t s) {
  if (S == 0 || a.Q == 0 || a.N == 0) return;
  ResampleArgs b = a;
  b.tile = plan.tile;
  b.tiles = (int)ceil_div(a.Q, plan.tile);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(S * b.tiles), (unsigned)ceil_div(a.N, RESAMPLE_SLICE)), dim3((unsigned)plan.waves * 64), 0, s, b);
  KIN_HIP(hipGetLastError());
}

void launch_resample_zero_tail(int64_t S, int64_t Q, int64_t N, const int64_t* d_keep_n, double* d_out, hipStream_t s) {
  if (S == 0 || Q == 0 || N == 0) return;
  const unsigned Y = (unsigned)std::min<int64_t>(64, ceil_div(Q * N, 256 * 8));
  hipLaunchKernelGGL(resample_zero_tail_kernel, dim3((unsigned)S, Y), dim3(256), 0, s, (int)Q, (int)N, d_keep_n, d_out);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
