// Directed relation graph (Lu & Law) of a network over batched states (kin_drg_*): host tables (drg.cpp), the gather
// kernels and their launchers (drg_kernels.hip).
//
// Records group the reactions: with pairing a record is a reaction kf and its exact reverse kr as compile_network pairs
// them (NetworkHost::pair_k; kr = -1: no partner) and progresses at w = q_kf - q_kr; without pairing every reaction is a
// record (kr = -1, w = q_r). Per record nu_A is the forward reaction's net coefficient of species A (slot_sp / slot_co)
// and S its species on either side (operands and slots: a collider with zero net coefficient belongs to S). For a state
//   den_A  = sum over records with nu_A != 0                     of |nu_A| |w|
//   num_AB = sum over records with nu_A != 0, B in S, B != A     of |nu_A| |w|
//   r_AB   = num_AB / den_A  (0 where den_A == 0),   coef_AB = max over the states of r_AB.
// An edge (A, B) exists when some record contributes to num_AB: a CSR over A, columns sorted, no diagonal.
//
// DRG with error propagation (kin_drgep_*; definition: include/kinetica_hip.h) walks the same plans with the SIGNED
// coefficients nu_A (stage 2: r[nb][E], no maximum over the states) and then searches, per state, the largest product of
// r along any path from a target (drgep_kernels.hip) over the transpose of the pattern.
//
// Path flux analysis (kin_pfa_*; pfa.hpp) walks the edge plan with the signed coefficients a third way (SPLIT: the positive and
// the negative part of every edge's sum apart, each over den_A) and multiplies the two sparse matrices per state.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "network.hpp"

namespace kin {

// Both sums are gather plans of build_seg_plan with payload (a, b) = (kf, kr) - laid out as a product plan, but b < 0
// is a record without a reverse here, not padding - and the coefficients |nu| in arrays of their own, addressed by the
// plan's payload slot (0.0f: padding). The edge plan's aux is the edge's row A, where its divisor den_A lives.
struct DrgTables {
  int64_t N = 0, E = 0, n_den = 0, n_num = 0;
  std::vector<int32_t> rowptr, colidx;          // N + 1, E
  int64_t den_cls[3] = {0, 0, 0};               // rows of the denominator plan with <= SHORT_MAX, <= SEG_LEN, more contributions
  int64_t edge_cls[3] = {0, 0, 0};              // edges of the edge plan likewise
  bool have_plans = false;
  SegPlanHost den_plan, edge_plan;
  std::vector<float> den_ell_c, den_long_c, edge_ell_c, edge_long_c;
  // DRGEP: nu_A with its sign in the same payload slots, and the incoming edges of every species (the transpose of the
  // pattern: in_src[j] -> B over edge in_edge[j] for j in [in_ptr[B], in_ptr[B + 1]), sources ascending). in_order lists the
  // species by in-degree class - <= IN_SHORT_MAX (a lane each), <= IN_WAVE_MAX (a wavefront), more (the workgroup) - in_cls
  // counts them. (The gather plans' SHORT_MAX = 8 was measured against 32 for the lanes: profiles/drgep_ab.txt.)
  static constexpr int IN_SHORT_MAX = 32, IN_WAVE_MAX = SegPlanHost::SEG_LEN;
  std::vector<float> den_ell_s, den_long_s, edge_ell_s, edge_long_s;
  std::vector<int32_t> in_ptr, in_src, in_edge, in_order;
  int64_t in_cls[3] = {0, 0, 0};
};
// pairing != 0 needs the pair records (compile_network builds them for N < 65535): KinError(ERR_UNSUPPORTED) without.
// with_edges = false (reaction importance): the denominator side alone - no edge pattern, edge plan or transpose (E = 0).
DrgTables build_drg_tables(const NetworkHost& h, int pairing, bool with_plans, bool with_edges = true);

struct DrgArgs {
  SegPlanView p;
  const float* ell_c; const float* long_c;
  int N, R, E, nb;                 // nb: states of this block, rates[nb][R]
  const double* rates;
  int64_t b0;                      // global index of the block's first state (for seg_n)
  const int64_t* seg_n; int64_t L; // state b counts only when b % L < seg_n[b / L] (seg_n null: every state counts)
  double* den;                     // den[nb][N]: written by the denominator launch, read by the edge launch
  double* part;                    // part[Y][E]: the edge launch's maxima per slice of the states
  double* r;                       // r[nb][E]: the signed edge launch's per-state coefficients (rows of states that do not count: untouched)
  double* rc;                      // rc[nb][E]: the split edge launch's consumption part (its production part goes to r)
};
// slices of the states a launch is cut into so that the device is filled (depends on the plan, nb and n_cu only)
int drg_slices(const SegPlanView& p, int64_t nb, int n_cu);
void launch_drg_den(const DrgArgs& a, int Y, hipStream_t s);
void launch_drg_edges(const DrgArgs& a, int Y, hipStream_t s);
// coef[e] = max(use_prev ? coef[e] : 0, part[0][e], ..., part[Y - 1][e])
void launch_drg_max(int64_t E, int Y, const double* part, double* coef, int use_prev, hipStream_t s);
// DRGEP stage 2 (ell_c / long_c: the SIGNED coefficients): den[bl][A] = max(P_A, C_A); r[bl][e] = min(1, |s_AB| / den_A)
void launch_drgep_den(const DrgArgs& a, int Y, hipStream_t s);
void launch_drgep_edges(const DrgArgs& a, int Y, hipStream_t s);
// PFA split stage (pfa.hpp) on the signed plans, after launch_drgep_den: r[bl][e] = P_AB / den_A, rc[bl][e] = C_AB / den_A
void launch_pfa_split(const DrgArgs& a, int Y, hipStream_t s);

// Reaction importance (kin_reaction_importance_*; definition: include/kinetica_hip.h; reaction_importance_kernels.hip): after
// stage 1 and the denominator launch, one thread per REACTION forms max over its record's selected species of |nu_A| |w| / den_A.
// The table it reads has one row per reaction: the other reaction of its pair (-1: none; always -1 without pairing) and the
// record's up to four (species, nu) slots - the forward reaction's, the sign flipped for the reverse member.
struct RiTables {
  int64_t R = 0, n_records = 0, n_paired = 0, n_empty = 0;   // n_paired: reactions with a partner; n_empty: without a slot
  std::vector<int32_t> partner;          // R
  std::vector<int32_t> species, nu;      // 4 R each: 0-based species or -1, signed net coefficient (0 beside -1)
  std::vector<int32_t> dev() const;      // the device form [6][R]: partner, the four species, |nu| in four packed bytes
};
RiTables build_ri_tables(const NetworkHost& h, int pairing);   // pairing without pair records: KinError(ERR_UNSUPPORTED)

struct RiArgs {
  int N, R, nb;
  const int32_t* tab;              // RiTables::dev()
  const uint8_t* mask;             // mask[N]: 1 for a selected species; null: all of them
  const double* rates;             // rates[nb][R]
  const double* den;               // den[nb][N] of launch_drg_den
  int64_t b0; const int64_t* seg_n; int64_t L;     // as DrgArgs
  double* part;                    // part[Y][R]: the maxima per slice of the states
  double* per_state;               // per_state[nb][R] or null (a state that does not count: 0.0)
};
int ri_slices(int64_t R, int64_t nb, int n_cu);
// mask[N] from n_sel species ids on the device (0-based; ids outside [0, N) are passed over)
void launch_ri_mask(int64_t n_sel, const int64_t* sel, int64_t N, uint8_t* mask, hipStream_t s);
void launch_ri(const RiArgs& a, int Y, hipStream_t s);

// DRGEP path stage (drgep_kernels.hip): one workgroup per state relaxes R_B = max(R_B, R_A r_AB) over the incoming edges
// until nothing changes (at most N rounds). R is double-buffered in LDS (in_lds: N <= DRGEP_LDS_SPECIES), else in work.
struct DrgepPathArgs {
  int N, E, nb, n_targets;
  const int32_t *in_ptr, *in_src, *in_edge, *in_order;
  int n_short, n_wave, n_long;     // in_order: the short species first, then the wavefront ones, then the long ones
  const int64_t* targets;         // 0-based; one outside [0, N) is passed over
  const double* r;                 // r[nb][E]
  int64_t b0; const int64_t* seg_n; int64_t L;     // as DrgArgs: a state that does not count gets R = 0 and 0 rounds
  double* R;                       // R[nb][N]
  double* work;                    // work[nb][2][N] (global form only)
  int32_t* rounds;                 // rounds[nb]
};
// 64 KB of LDS per workgroup, less the kernel's own few words: two buffers of N doubles fit up to this N
constexpr int64_t DRGEP_LDS_SPECIES = ((64 << 10) - 256) / 16;
void launch_drgep_paths(const DrgepPathArgs& a, bool in_lds, hipStream_t s);
// imp[i] = max(use_prev ? imp[i] : 0, R[0][i], ..., R[nb - 1][i])
void launch_drgep_max(int64_t N, int64_t nb, const double* R, double* imp, int use_prev, hipStream_t s);

}  // namespace kin
