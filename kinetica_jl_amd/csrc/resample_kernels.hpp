// Resampling of stored trajectories onto query points of a per-segment axis (resample_kernels.hip; entry points:
// resample_api.cpp; definitions: include/kinetica_hip.h): per segment and query the bracket (jc, w) and the state at the query,
// a row copied bit for bit or the chord between two saved rows.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace kin {

constexpr int RESAMPLE_LANES = 64;          // species per wave instruction: a row's 512 contiguous bytes per load
constexpr int RESAMPLE_SLICE = 1024;        // species of a workgroup's slice (64 x 16): one slice up to 1024 species
constexpr int RESAMPLE_WAVES_MAX = 16;      // wavefronts of a workgroup, the tile's queries dealt out among them
constexpr int RESAMPLE_TILE_MAX = 256;      // queries of a workgroup's tile (their brackets sit in LDS)
constexpr int RESAMPLE_BELOW = -1, RESAMPLE_ABOVE = -2, RESAMPLE_NONE = -3;   // jc of a query that is not inside

// The bracket of one query v on the axis rows x[jb .. n - 1] (non-decreasing, no NaN): jc, the first row with x[j] >= v, found
// by bisection, or the code of a query that is not inside; *w the chord's weight, 0.0 where the value is a copy or the query is
// outside. The one statement of the rule for kin_resample_bracket_host and the kernel.
__host__ __device__ inline int resample_bracket(const double* x, int jb, int n, double v, double* w) {
#pragma clang fp contract(off)
  *w = 0.0;
  if (n <= jb || v != v) return RESAMPLE_NONE;
  if (v < x[jb]) return RESAMPLE_BELOW;
  if (v > x[n - 1]) return RESAMPLE_ABOVE;
  int lo = jb, hi = n - 1;      // x[hi] >= v holds; the first such row is wanted
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (x[mid] < v) lo = mid + 1; else hi = mid;
  }
  const double xb = x[lo];
  if (xb == v) return lo;
  const double xa = x[lo - 1];
  const double num = v - xa, den = xb - xa;
  *w = num / den;
  return lo;
}

struct ResampleArgs {
  int N, L, Q;                    // species; rows of a segment's block; queries
  const int64_t* seg_n;           // rows a segment really has (null: L)
  const double* u;                // [S][L][N]
  const double* x;                // [L], or [S][L] with x_stride == L
  int64_t x_stride;
  const double* xq;               // [Q], or [S][Q] with xq_stride == Q
  int64_t xq_stride;
  int mode;                       // KIN_RESAMPLE_*
  int row_begin;
  int tile, tiles;                // queries of a tile; tiles of a segment (blockIdx.x = segment * tiles + tile)
  double fill;
  double* out;                    // [S][Q][N]
  int32_t* jc;                    // [S][Q] or null
  double* w;                      // [S][Q] or null
};

// How the launcher cuts the work: `tile` queries per workgroup, dealt out to `waves` wavefronts. Results do not depend on
// either; KIN_RESAMPLE_TILE_QUERIES and KIN_RESAMPLE_WAVES (read per call: tests change them) force them.
struct ResamplePlan { int tile, waves; };
ResamplePlan resample_plan(int64_t S, int64_t Q, int64_t N, int n_cu);

// one launch over S segments: grid (S tiles, ceil(N / 1024)); S, Q, N >= 1, S ceil(Q / tile) < 2^31, N <= 64 * 65535
void launch_resample(int64_t S, const ResamplePlan& plan, const ResampleArgs& a, hipStream_t s);

// out[s][q][:] = 0 for q >= keep_n[s]: the rows past a member's leading run of covered queries in a stored record
void launch_resample_zero_tail(int64_t S, int64_t Q, int64_t N, const int64_t* d_keep_n, double* d_out, hipStream_t s);

}  // namespace kin
