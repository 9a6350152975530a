// Event times over stored trajectories (event_kernels.hip; entry points: event_api.cpp; definitions: include/kinetica_hip.h):
// per segment and species the peak, the time of its first row and the time of the first crossing of a level.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace kin {

constexpr int EVENT_LANES = 64;        // species per workgroup: one wavefront's width, a row's 512 contiguous bytes per load
constexpr int EVENT_WAVES_MAX = 16;    // wavefronts of a workgroup, all on the same 64 species, the rows split among them
constexpr int EVENT_ROWS_IN_FLIGHT = 4;

struct EventArgs {
  int N, L;                       // species; rows of a segment's block
  const int64_t* seg_n;           // rows a segment really has (null: L)
  const double* u;                // [S][L][N]
  const double* t;                // [L], or [S][L] with t_stride == L
  int64_t t_stride;
  const double* level;            // [N] (null when t_cross is)
  int kind, direction, start;     // KIN_LEVEL_*, the sign of the direction, KIN_FROM_*
  int row_begin;
  int part_rows;                  // rows of a part; part p of a segment goes to wavefront p % waves
  double never;
  double *u_peak, *t_peak, *t_cross;   // [S][N], any may be null
};

// How the launcher cuts the work: `waves` wavefronts per workgroup and `part_rows` rows per part. Results do not depend on
// either; KIN_EVENT_WAVES and KIN_EVENT_PART_ROWS (read per call: tests change them) force the first and cap the second.
struct EventPlan { int waves, part_rows; };
EventPlan event_plan(int64_t S, int64_t L, int64_t N, int n_cu);

// one launch over S segments: grid (S, ceil(N / 64)); S, N >= 1, N <= 64 * 65535, L < 2^31
void launch_events(int64_t S, const EventPlan& plan, const EventArgs& a, hipStream_t s);

}  // namespace kin
