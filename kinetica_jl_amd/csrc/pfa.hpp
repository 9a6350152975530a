// Path flux analysis (Sun, Chen, Gou & Ju 2010) of a network over batched states (kin_pfa_*; definition:
// include/kinetica_hip.h): host tables (pfa.cpp), the second-generation kernel and its launcher (pfa_kernels.hip).
//
// Stage 1 is the flux sweep, the split stage the DRG pass's signed gathers on the DRG plans (drg_kernels.hip, SPLIT):
//   rp[bl][e] = P_AB / den_A,  rc[bl][e] = C_AB / den_A    over the edges E of kin_drg_pattern.
// The second-generation stage is, per state, a product of two sparse matrices on a fixed pattern:
//   r_AB = rp_AB + rc_AB + sum over M in out(A) of (rp_AM rp_MB + rc_AM rc_MB),   B != A
// on the pattern E2 = E plus every two-hop pair, folded into the exact maximum over the states.
#pragma once
#include "drg.hpp"

namespace kin {

// One row buffer of N doubles (and a spare slot) in LDS beside the staged out-edges of the row (PFA_CHUNK of them at a time,
// 24 bytes each): what fits the 160 KB of a CDNA4 compute unit. Networks above it: KinError(ERR_UNSUPPORTED).
constexpr int PFA_CHUNK = 64;
constexpr int64_t PFA_LDS_SPECIES = (160 * 1024 - PFA_CHUNK * 24) / 8 - 2;      // 20286
// A row whose cost sum over M in out(A) of deg(M) is above this is taken by a workgroup of 256, else by one wavefront. The two
// classes are two launches, and with enough slices of the states a wavefront per row was as fast or faster up to 1 000 species
// (profiles/pfa_ab.txt): the workgroup is for the rows next to a hub of a large network, whose single state is 10^5 products.
constexpr int64_t PFA_WG_COST = 65536;
// ... and above this many species fewer than eight row buffers fit a compute unit, so that single wavefronts would leave it
// nearly empty: every row goes to a workgroup (at 10 000 species one buffer fits; measured 105 ms against 112 ms)
constexpr int64_t PFA_WAVE_SPECIES = (160 * 1024 / 8 - PFA_CHUNK * 24) / 8 - 2;      // 2366

struct PfaTables {
  int64_t N = 0, E = 0, E2 = 0;
  int64_t products = 0;             // sum over the edges (A, M) of deg(M): multiply-adds of the two products per state
  int64_t max_row = 0;              // largest out-degree in E
  std::vector<int32_t> rowptr2, colidx2;      // N + 1, E2: CSR, sorted columns, no diagonal
  // the rows with at least one out-edge by falling cost sum over M in out(A) of deg(M) (the heaviest start first; ties by
  // row), and that cost in the same order
  std::vector<int32_t> order;
  std::vector<int64_t> order_cost;
};
// rowptr / colidx: the DRG pattern. Throws KinError(ERR_UNSUPPORTED) when E2 leaves 32-bit offsets.
PfaTables build_pfa_tables(int64_t N, const std::vector<int32_t>& rowptr, const std::vector<int32_t>& colidx);

struct PfaArgs {
  int N, nb;
  int64_t E, E2;
  const int32_t *rowptr, *colidx;   // E
  const int32_t *rowptr2, *colidx2; // E2
  const int32_t* order;             // the rows of this launch
  int n_rows, Y;                    // blocks: n_rows x Y, the slices of a row next to each other
  const double *rp, *rc;            // [nb][E]
  int64_t b0; const int64_t* seg_n; int64_t L;     // as DrgArgs: a state that does not count takes no part
  double* part;                     // part[Y][E2]: the maxima per slice of the states (every entry of a launched row is written)
  double* r;                        // r[nb][E2] or null: the per-state coefficients (rows of states that do not count: untouched)
};
// slices of the states so that the device is filled (depends on the tables, nb and n_cu only)
int pfa_slices(const PfaTables& t, int64_t nb, int n_cu);
// both classes: the rows costing more than wg_cost by a workgroup each, the others by a wavefront each. a.order: the device
// copy of PfaTables::order (a.n_rows is set here)
void launch_pfa_second(const PfaTables& t, PfaArgs a, int64_t wg_cost, int Y, hipStream_t s);

}  // namespace kin
