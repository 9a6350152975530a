// Timescale analysis of a network over batched states (kin_jac_batched*, kin_timescale_*; definitions: include/kinetica_hip.h):
// the host table of the row pass (timescale_api.cpp), the kernels' arguments and their launchers (timescale_kernels.hip).
//
// Stage 1 forms rates[nb][R] and the operand derivatives dr[nb][2R] of a block of states (mass_action_rate / _drates with the
// state's own rate constants). Stage 2 is two many-states gathers: the ENTRY gather jv[bl][e] = sum c dr[bl][src] over the
// handle's Jacobian plan (the plan jac_dev walks for one state), and the ROW pass, which reads the stored entries of a
// species row, forms d_i = J_ii, g_i = sum |J_ij| and f_i = sum nu q along sp_ptr, and keeps the three running extrema of its
// slice of the states. Two small launches close a block: the fold of the slices into summary[3][N] and the maximum of g.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "network.hpp"

namespace kin {

// The rows of J by their number of stored entries: <= TS_SHORT_MAX 64 to a wavefront (a lane each), <= TS_WAVE_MAX a
// wavefront each, longer ones a workgroup each. rows: one slot of eight words per row - the species i, its stored entries
// [e0, e1) with the diagonal at dp, its reactions [s0, s1) in sp_rxn / sp_coef, two words unused - the short rows first, padded
// with i = -1 to whole groups of 64, then the medium ones, then the long ones.
struct TsTables {
  static constexpr int TS_SHORT_MAX = 8, TS_WAVE_MAX = 256;
  int64_t N = 0, nnz = 0;
  int64_t cls[3] = {0, 0, 0};
  int32_t G = 0, S = 0, Bl = 0;
  std::vector<int32_t> rows;      // 8 (64 G + S + Bl)
};
TsTables build_ts_tables(const NetworkHost& h);

// which states of a block count: global index gb = b0 + bl; with seg_n (the stored ensemble) row j = gb % L of member gb / L
// counts when row_begin <= j < seg_n[gb / L], without (L == 0) when gb >= row_begin (32-bit: the passes hold B below 2^31)
struct TsCount { int32_t b0; const int64_t* seg_n; int32_t L; int32_t row_begin; };

struct TsRateArgs {
  int N, R, nb;
  const int32_t* x0; const int32_t* x1;
  const double* u;                 // u[nb][N]
  const double* k; int64_t k_stride; const int64_t* k_row;   // row k_row[bl] (null: row bl) of k, k_stride doubles apart (0: one row)
  const double* T; const double* Ea; const double* A; int has_kmax; double k_max, t_mult;   // T != null: the Arrhenius law at T[bl]
  double* rates;                   // rates[nb][R] or null
  double* dr;                      // dr[nb][2R]
};
void launch_ts_rates(const TsRateArgs& a, hipStream_t s);

struct TsEntryArgs {
  SegPlanView p;                   // the Jacobian's contribution lists (rows = stored entries)
  int R, nb;
  int64_t nnz;
  const double* dr;                // dr[nb][2R]
  double* jv;                      // jv[nb][nnz]
  TsCount cnt;
};
// entries one thread takes per pass of a long contribution list (a pass: TS_WG * TS_LONG_NX entries)
constexpr int TS_WG = 256, TS_WAVES = TS_WG / 64, TS_LONG_NX = 4;
int ts_entry_slices(const SegPlanView& p, int64_t nb, int n_cu);
void launch_ts_entries(const TsEntryArgs& a, int Y, hipStream_t s);

struct TsRowArgs {
  int N, R, nb;
  int nnz;
  int G, S, Bl;
  const int4* rows;                // TsTables::rows, two int4 per slot
  const int32_t* sp_rxn; const float* sp_coef;
  const double* jv;                // jv[nb][nnz]
  const double* rates;             // rates[nb][R]
  TsCount cnt;
  double* part;                    // part[Y][3][N] or null
  double* g;                       // g[nb][N] or null
  double* diag; double* err;       // [nb][N] each, or null
};
int ts_row_slices(const TsRowArgs& a, int n_cu);
// two launches: the long rows (when there are any), then the short groups and the medium rows
void launch_ts_rows(const TsRowArgs& a, int Y, hipStream_t s);
// summary[q][i] = the slices' extremum (q = 0, 2: maximum, q = 1: minimum), with the current contents when use_prev
void launch_ts_fold(int64_t N, int Y, const double* part, double* summary, int use_prev, hipStream_t s);
// summary rows = -Inf, +Inf, 0.0
void launch_ts_identity(int64_t N, double* summary, hipStream_t s);
// norm[bl] = max_i g[bl][i], 0.0 for a state that does not count
void launch_ts_norm(int64_t N, int64_t nb, const double* g, const TsCount& cnt, double* norm, hipStream_t s);

}  // namespace kin
