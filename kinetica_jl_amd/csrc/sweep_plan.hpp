// Launch plans of the two batched RHS sweeps, host code only (no HIP types): which kernel instantiation a call takes and
// with which launch configuration. kin_network::sweep_dev / launch_sweep / launch_sweep_big (kernels.hip) and
// launch_tiled_sweep (tiled_kernels.hip) execute exactly what these functions return - the rules live here and nowhere
// else - and kin_sweep_plan / kin_sweep_plan_host / kin_tiled_sweep_plan / kin_tiled_sweep_plan_host report them
// (include/kinetica_hip.h), as kin_flux_plan_host does for the flux passes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace kin {

constexpr int SWEEP_DUMMY = 64;   // dummy entries behind u_s / du_s of the LDS sweeps, one per lane
// rows per batch of sweep_reg_kernel (ILP); a build-time knob for the depth comparison in docs/DESIGN_HISTORY.md
#ifndef KIN_SWEEP_ILP
#define KIN_SWEEP_ILP 4
#endif
constexpr size_t SWEEP_LDS_MAX = 160 * 1024;

// Batch plan of the streamed rows of sweep_reg_kernel: `rows` record rows of BS records, the first TR of them register-
// resident; the S = rows - TR streamed ones run as n_a batches of ILP and n_b batches of ILP + 1, in the fewest
// rounds ceil(S / (ILP + 1)) - a remainder row rides in a wider batch instead of costing a load round of its own
// (C3, BS = 1024: 17 streamed rows = 4 + 4 + 4 + 5, not 4 x 4 + a fifth batch of one real row and three padding rows).
// Rows past `rows` that the last ILP-batch covers (S < ILP * rounds) are padding records.
struct SweepStreamPlan { int n_a, n_b; };
inline SweepStreamPlan sweep_stream_plan(int64_t P, int bs, int tr, int ilp) {
  const int64_t rows = (P + bs - 1) / bs, S = std::max<int64_t>(0, rows - tr);
  const int64_t rounds = (S + ilp) / (ilp + 1);
  const int64_t n_b = std::max<int64_t>(0, S - ilp * rounds);
  return {(int)(rounds - n_b), (int)n_b};
}

enum SweepKernel : int { SWEEP_REG = 0, SWEEP_GEN = 1, SWEEP_LDS = 2, SWEEP_BIG = 3, SWEEP_PER_STATE = 4 };

// what the caller-layout sweep needs to know of a compiled network (NetworkHost) and of a call's buffers
struct SweepNetInfo {
  int64_t N, R, P;                 // species, reactions, records (n_pairs)
  bool adjacent, block;            // pairs_adjacent, pairs_block
  bool has_rec64, has_gen;         // pair_rec64 / gen_rec8 were built
  int n_copy, n_gen_expl;          // split-accumulator entries; explicit-operand records of the general sweep
  int32_t big_H, big_tail_tiles, big_n_expl;
  bool big_tail_by_species;
};
// the low four address bits of u, du and of the rate constants in effect (k_b, or the handle's own row)
struct SweepAlign { unsigned u, k, du; };

struct SweepPlan {
  int kernel = SWEEP_LDS;                    // SweepKernel
  int bs = 1024, tr = 0, ilp = 0;            // workgroup size; register-resident rows and rows per batch (sweep_reg_kernel)
  bool blk = false, adj = false, u_in_lds = false;
  int n_a = 0, n_b = 0;                      // sweep_stream_plan
  int grid = 0, per_cu = 1;
  int n_copy = 0, n_expl = 0, tail_tiles = 0;
  bool tail_by_species = false;
  int tile = 0, n_tiles = 1;                 // LDS entries per array; species tiles (sweep_lds_kernel<false, *>)
  size_t smem = 0;                           // dynamic LDS bytes
  int H = 0;
  int64_t P = 0;                             // records the kernel walks
};

inline SweepPlan sweep_plan(const SweepNetInfo& n, int n_cu, int64_t B, SweepAlign al) {
  SweepPlan p;
  const int64_t N = n.N, P = n.P;
  p.P = P;
  if (N >= 65535) {
    // the packed sweep records hold species ids in 16 bits; wider networks take the single-state kernels
    // (32-bit ids) state after state on the same stream - correct at any size, one state per launch pair
    p.kernel = SWEEP_PER_STATE; p.bs = 256; p.grid = 0; p.per_cu = 0;
    return p;
  }
  // the double2 fast path also needs 16-byte aligned rows of k: R even (checked by the host) and an aligned base
  p.adj = n.adjacent && (al.k & 15) == 0;
  p.grid = (int)std::min<int64_t>(B, n_cu);
  if (n.big_H > 0) {
    p.kernel = SWEEP_BIG; p.H = n.big_H; p.tail_tiles = n.big_tail_tiles; p.n_expl = n.big_n_expl;
    p.tail_by_species = n.big_tail_by_species; p.u_in_lds = false;
    p.tile = n.big_H + SWEEP_DUMMY;
    p.smem = (size_t)2 * (n.big_H + SWEEP_DUMMY) * 8;
    return p;
  }
  if ((size_t)(2 * N) * 8 <= SWEEP_LDS_MAX) {
    p.u_in_lds = true;
    if ((p.adj || n.block) && n.has_rec64 && n.R < ((int64_t)1 << 29) && ((al.u | al.du) & 15) == 0 && N % 2 == 0 &&
        (size_t)(2 * (N + SWEEP_DUMMY + n.n_copy)) * 8 <= SWEEP_LDS_MAX && n.n_copy <= 1024) {
      p.kernel = SWEEP_REG; p.n_copy = n.n_copy; p.blk = !p.adj;
      p.tile = (int)N + SWEEP_DUMMY + n.n_copy + (n.n_copy & 1);   // even: keeps u_s 16-byte aligned
      p.smem = (size_t)2 * p.tile * 8;
      // smaller states run in smaller workgroups, several per CU (LDS permitting): more states in flight per CU and
      // enough records per thread to keep them register-resident (C2, N = 1000: 0.073 -> 0.050 ms)
      p.bs = (N <= 2560 && n.n_copy <= 256) ? 256 : ((N <= 5120 && n.n_copy <= 512) ? 512 : 1024);
      p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / p.bs, SWEEP_LDS_MAX / p.smem));
      p.grid = (int)std::min<int64_t>(B, (int64_t)n_cu * p.per_cu);
      // two register-resident batches where the network has the rows for them, else one, else none
      const int64_t Tr = P / p.bs;   // full record rows available for residency
      p.ilp = KIN_SWEEP_ILP;
      p.tr = Tr >= 2 * p.ilp ? 2 * p.ilp : (Tr >= p.ilp ? p.ilp : 0);
      const SweepStreamPlan sp = sweep_stream_plan(P, p.bs, p.tr, p.ilp);
      p.n_a = sp.n_a; p.n_b = sp.n_b;
      return p;
    }
    if (n.has_gen && (size_t)(2 * (N + SWEEP_DUMMY)) * 8 <= SWEEP_LDS_MAX) {
      p.kernel = SWEEP_GEN; p.adj = false; p.ilp = 4; p.n_expl = n.n_gen_expl;
      p.tile = (int)N + SWEEP_DUMMY;
      p.smem = (size_t)2 * p.tile * 8;
      p.bs = N <= 2560 ? 256 : (N <= 5120 ? 512 : 1024);     // smaller states: smaller workgroups, several per CU
      p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / p.bs, SWEEP_LDS_MAX / p.smem));
      p.grid = (int)std::min<int64_t>(B, (int64_t)n_cu * p.per_cu);
      return p;
    }
    p.kernel = SWEEP_LDS; p.ilp = 8;
    p.tile = (int)((N + 1) / 2 * 2);
    p.smem = (size_t)(p.tile + N) * 8;
    return p;
  }
  p.kernel = SWEEP_LDS; p.ilp = 8; p.u_in_lds = false;
  p.tile = 16 * 1024;   // 128 kB of accumulators per pass
  p.n_tiles = (int)((N + p.tile - 1) / p.tile);
  p.smem = (size_t)p.tile * 8;
  return p;
}

// ---- tiled sweep (library order) ----
struct TiledSweepPlan {
  int bs = 1024, un = 5, nb = 4;       // workgroup size, staged doubles per thread, record rows per batch
  bool tmode = false, singles = false;
  int grid = 0, per_cu = 1;
  size_t smem = 0;
};
// E: LDS entries per array; h: hubs; win_cnt_max: the largest window; exp_tab: entries of the temperature form's exp table
inline TiledSweepPlan tiled_sweep_plan(int bs, int E, int h, int win_cnt_max, bool has_singles, int exp_tab, int n_cu, int64_t B,
                                       bool tmode) {
  TiledSweepPlan p;
  p.bs = bs; p.tmode = tmode;
  p.smem = ((size_t)2 * E + (tmode ? exp_tab : 0)) * 8;
  p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(2048 / bs, SWEEP_LDS_MAX / p.smem));
  p.grid = (int)std::min<int64_t>(B, (int64_t)n_cu * p.per_cu);
  p.un = std::max(h, win_cnt_max) <= 5 * bs ? 5 : 10;
  p.singles = !tmode && has_singles;   // (the temperature form reads no rate constants: one instantiation)
  p.nb = (tmode || p.un > 5) ? 2 : 4;  // tiled_sweep_kernel: NB
  return p;
}

}  // namespace kin
