// Reaction-flux pass over batched states (kin_flux_batched*, kin_solution_flux): per-reaction rates of B states, their
// weighted sum over the states, launch plan and launchers (flux_kernels.hip).
#pragma once
#include "common.hpp"
#include "network.hpp"

namespace kin {

// Index tables of the flux pass, one entry per PAIR of adjacent reactions (2j, 2j + 1); R odd: the last pair's second
// reaction does not exist and reads dummies only.
//   idx16: (x0 | x1 << 16) per reaction, LDS labels; label N is the dummy entry holding 1.0 (x1 < 0, or no reaction).
//          Only built when N + 1 fits 16 bits.
//   idx32: (x0, x1) per reaction as they are (x1 = -1: no second operand; no reaction: (0, -1)) - the gather path.
struct FluxTables {
  std::vector<uint32_t> idx16;   // 2 words per pair
  std::vector<int32_t> idx32;    // 4 words per pair
};
FluxTables build_flux_tables(const NetworkHost& h);

// How a call is cut (depends on B, R, N, the compute units, the rate-constant source and the KIN_FLUX_* switches only):
//   rows   double2 rows a thread owns per part (compile-time instantiations: 1, 2, 4, 8)
//   parts  reaction parts (blockIdx.y), each re-staging u
//   G      state slices (blockIdx.x); slice g takes states g, g + G, ...: partial sums part[G][R]
//   path   0: u in LDS, staged as double2 (N even, N <= 10 240, aligned rows); 1: u in LDS, any N that fits and any alignment, staged without prefetch;
//          2: u gathered from global memory (8 (N + 1) bytes do not fit LDS, or KIN_FLUX_LDS=0)
struct FluxPlan { int rows, parts, G, path; };
enum FluxMode : int { FLUX_K16 = 0, FLUX_K8 = 1, FLUX_T = 2 };   // k rows as double2 / as doubles / Arrhenius law at T[b]
FluxPlan flux_plan(int64_t B, int64_t R, int64_t N, int n_cu, bool temperature_form, bool u_aligned, int max_rows = 8);

// The rest of an instantiation, chosen from R and the alignment of the caller's pointers (their low four address bits):
//   k_mode      FLUX_T with temperatures; else FLUX_K16 when every k row is 16-byte aligned and holds whole pairs (R even,
//               k_stride even, aligned base), else FLUX_K8. The segmented pass takes the same rule.
//   rates_mode  the kernel's RATES: 0 no per-state rates, 1 written as double2 (R even, aligned base), 2 as doubles
struct FluxModes { int k_mode, rates_mode; };
FluxModes flux_modes(int64_t R, bool temperature_form, int64_t k_stride, unsigned k_bits, bool want_rates, unsigned rates_bits);

struct FluxArgs {
  int N, R, P, B;                  // P = ceil(R / 2) pairs
  const uint2* idx16; const int4* idx32;
  const double* u;                 // u[B][N]
  const double* k;                 // MODE K16 / K8: state b reads row (k_row ? k_row[b] : b) of k, rows k_stride doubles apart (0: one shared row)
  int64_t k_stride;
  const int64_t* k_row;
  const double* T;                 // MODE T: T[B]
  const double* Ea; const double* A; int has_kmax; double k_max, t_mult;
  const double* w;                 // w[B] or null (weights 1)
  double* part;                    // part[G][R] or null (no flux wanted)
  double* rates;                   // rates[B][R] or null
};

// Enqueues the sweep (a.part filled for plan.G slices) - and nothing else; flux = launch_flux_reduce(part).
void launch_flux_sweep(const FluxPlan& plan, const FluxArgs& a, hipStream_t s);
// flux[r] = part[0][r] + part[1][r] + ... + part[G - 1][r], in that order
void launch_flux_reduce(int64_t R, int G, const double* part, double* flux, hipStream_t s);

// Segmented flux pass (kin_flux_segmented*, kin_ensemble_flux): S segments of up to L states each, state b = s L + j at
// u[b][N]; flux[s][r] = sum over j < seg_n[s] of w[b] rate_r(u_b; k of state b), summed in row order by the ONE workgroup
// that owns (segment, part of the reactions) - no partial sums, no reduce launch; a segment's result depends on its own
// rows only. rows / parts / path are flux_plan's with max_rows = FLUX_SEG_MAX_ROWS - eight rows AND their rate constants held
// across states do not fit 128 registers - and its G is not used: the grid is (S, parts).
constexpr int FLUX_SEG_MAX_ROWS = 4;
struct FluxSegArgs {
  int N, R, P;                     // P = ceil(R / 2) pairs
  int64_t S, L;
  const int64_t* seg_n;            // seg_n[S] (clamped to [0, L]) or null: every segment has L rows
  const uint2* idx16; const int4* idx32;
  const double* u;                 // u[S L][N]
  const double* k; int64_t k_stride; const int64_t* k_row;   // as FluxArgs
  const double* T;                 // T[S L]
  const double* Ea; const double* A; int has_kmax; double k_max, t_mult;
  const double* w;                 // w[S L] or null (weights 1)
  double* flux;                    // flux[S][R]
  int64_t par_stride;              // MODE T: segment s reads Ea / A from s par_stride doubles behind the base (0: one shared pair of rows)
};
void launch_flux_seg(const FluxPlan& plan, const FluxSegArgs& a, hipStream_t s);
// umax[s][i] = max over j < seg_n[s] of u[s L + j][i]; zeros for an empty segment
void launch_seg_max(int N, int64_t S, int64_t L, const int64_t* seg_n, const double* u, double* umax, hipStream_t s);
// dot[s][j] = sum_i w[i] u[s L + j][i] for j < seg_n[s] (rowdot_kernel's summation order), zeros beyond
void launch_seg_dot(int N, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* w, double* dot, hipStream_t s);

}  // namespace kin
