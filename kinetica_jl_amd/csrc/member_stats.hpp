// Cross-member statistics of a block of states u[K][L][N] (member, row of the save grid, species): moments, quantiles and
// correlations over the PARTICIPANTS, the members a call's `use` mask names, in member order (include/kinetica_hip.h has the
// definitions; kernels: member_stats_kernels.hip; entries: member_stats_api.cpp).
//
// A COLUMN is one (row j, species i): the n participants' values u[idx[q]][j][i], q = 0..n-1. Every statistic is a function of
// its own column alone and every sum below has one fixed order, so results repeat bit for bit and do not depend on how a call
// cuts its columns into blocks or tiles.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace kin {

// the sorted passes (quantiles, rank correlation) hold a column's padded power of two in LDS: the largest n they take
// (include/kinetica_hip.h: KIN_MEMBERS_MAX_SORTED)
constexpr int MS_MAX_SORTED = 4096;
constexpr size_t MS_WORK_BYTES = (size_t)256 << 20;   // bound of the workspace Yhat[columns][n] of a block of columns

// Moments of all C = L N columns: lanes along the columns (the contiguous axis), the participants split over the MS_MOM_WAVES
// wavefronts of a workgroup. Wave w adds the participants q = w, w + W, w + 2W, ... in that order into one accumulator; the W
// partial sums are added in the order w = 0..W-1; mean = sum / n. The second pass forms d = x - mean and S = sum fma(d, d, S)
// in the same order; var = S / (n - 1) (n == 1: S, which is 0.0 for a finite value). min / max are exact; a NaN among the
// column's values makes all four NaN. n == 0 is the caller's case (zeros), never launched.
constexpr int MS_MOM_WAVES = 8;
struct MsMomArgs {
  const double* u;
  const int32_t* idx;    // [n] members taking part, ascending
  int32_t n;
  int64_t C, stride;     // columns; doubles between two members (L N)
  double *mean, *var, *mn, *mx;   // [C] each, any null
};
void launch_ms_moments(const MsMomArgs& a, hipStream_t s);

// The selected columns of a call, c = j n_sel + s in [0, L n_sel): row j, species sel[s] (sel null: s itself). A launch takes
// the columns [c0, c0 + nc).
struct MsColArgs {
  const double* u;
  const int32_t* idx;
  const int32_t* sel;    // [n_sel] 0-based species or null
  int32_t n, N, n_sel;
  int64_t stride, c0, nc, c_total;
  // sorted pass only: T columns per workgroup (a power of two <= 8), P2 the padded power of two >= max(n, 2)
  int32_t T, P2;
  int32_t Q;
  const double* p;       // [Q] probabilities
  double* q_out;         // [Q][c_total] or null
  double* yhat;          // [nc][n] of this launch's columns, or null: the normalised ranks (sorted pass) / values (value pass)
};
// Gathers a tile of columns into LDS (consecutive species share sectors: the tile's columns are the fast index of the gather),
// sorts each by a bitonic network over P2 (+Inf padding), writes the quantiles by the header's rule (separately rounded
// multiply and add) and, with yhat, the normalised ranks: a value's run [lo, hi) comes from two binary searches in the sorted
// column, rank = (lo + hi + 1) / 2, d = rank - (n + 1) / 2, S = sum d^2 - every term a multiple of 1/4 below 2^53 / 4, so the
// sum is exact in any order - yhat = d / sqrt(S), zeros where S == 0. A column holding a NaN gives NaN everywhere.
void launch_ms_sorted(const MsColArgs& a, hipStream_t s);
int ms_sorted_tile(int32_t P2);   // columns per workgroup of the sorted pass for this padded size
// yhat = (y - mean) / sqrt(S) of the values themselves, any n: a workgroup takes 8 columns x 32 participant lanes; lane l adds
// q = l, l + 32, ... in order, the 32 partials are added in the order l = 0..31; mean = sum / n, d = y - mean, S = sum fma(d, d, S)
// in the same order; zeros where S == 0, NaN where S is NaN.
void launch_ms_values(const MsColArgs& a, hipStream_t s);
// out[c][p] = sum over q = 0..n-1, in that order, of fma(xhat[q][p], yhat[c][q], acc): LDS tiles of 16 columns x 16 inputs x 64
// participants, plain FMA loops
void launch_ms_corr(int64_t nc, int32_t n, int32_t P, const double* xhat, const double* yhat, double* out, hipStream_t s);

// Sobol indices of a Saltelli design (include/kinetica_hip.h: the definition; kernel: sobol_kernels.hip). The block holds
// K = M (P + 2) members, member b M + m = sample m of block b (0: A, 1: B, 2 + p: AB_p). The PARTICIPANTS are the samples with
// a weight > 0, ascending: idx[q] is the q-th one's m, wt[q] its weight, np of them, n = sum wt. For one column (the selected
// columns c = j n_sel + s of MsColArgs) and participant q write a, b, c_p for the values of sample idx[q] in A, B, AB_p and
// wq = (double)wt[q]. Every product with wq is rounded on its own (exact for wq == 1); every fma below is one rounding.
//
// Lanes along the columns; the participants split over the SB_WAVES wavefronts of a workgroup: wave w takes q = w, w + W, ...
// in that order, every accumulator starts at 0.0, and the W partials of a quantity are added in the order w = 0..W-1,
// starting from wave 0's.
//   pass 1   TA = sum (TA + wq a), TB = sum (TB + wq b);  mu = (TA + TB) / (2 n).  Beside it the exact minimum and maximum of
//            the participants' a and b: the column is FLAT when max - min == 0 and mu is not NaN.
//   pass 2   da = a - mu, db = b - mu;  SA = fma(wq da, da, SA), SB = fma(wq db, db, SB);
//            per input p:  C1_p = fma(wq db, c_p - a, C1_p);  e = a - c_p, C2_p = fma(wq e, e, C2_p).
//   result   V = (SA + SB) / (2 n), exactly 0.0 for a flat column (the sum of n equal values need not be n times the value:
//            without the rule a constant column would get a V of rounding noise);
//            S1_p = (C1_p / n) / V,  ST_p = (C2_p / (2 n)) / V;  both exactly 0.0 when n < 2 or V == 0.
// A launch takes SB_CHUNK inputs per workgroup (the accumulators 2 + 2 SB_CHUNK live in registers; the chunks of a larger P
// are further workgroups, grid.y, each repeating pass 1 and SA, SB in the same order: nothing depends on the chunking).
// n == 0 is the caller's case (zeros), never launched.
constexpr int SB_WAVES = 8;
constexpr int SB_CHUNK = 8;
struct SobolArgs {
  const double* u;
  const int32_t* idx;    // [np] participating samples m, ascending
  const int32_t* wt;     // [np] their weights (> 0)
  const int32_t* sel;    // [n_sel] 0-based species or null
  int32_t np, M, P, N, n_sel;
  int64_t n;             // sum wt
  int64_t stride, c_total;   // doubles between two members (L N); selected columns L n_sel
  double *S1, *ST;       // [c_total][P] or null
  double *mean, *var;    // [c_total] or null
};
void launch_sobol(const SobolArgs& a, hipStream_t s);

}  // namespace kin
