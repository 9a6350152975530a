// Path flux analysis, second-generation stage (gfx950, wave64): from the per-state first-generation coefficients rp[nb][E]
// and rc[nb][E] of a block of states (the split stage: drg_kernels.hip, SPLIT) to the per-row maxima over the states of
//   r_AB = rp_AB + rc_AB + sum over M in out(A) of (rp_AM rp_MB + rc_AM rc_MB)
// on the pattern E2 - per state a product of two sparse matrices whose pattern is fixed.
// A task owns one row A for a slice of the states. It keeps a row buffer acc[N] in LDS and takes the out-edges M of A ONE
// AFTER THE OTHER in pattern order: the first-generation term of (A, M) goes to acc[M] when M is staged, then the task's
// threads add the row M of (rp, rc), scaled by (rp_AM, rc_AM), into acc - within one M every target B is distinct, so every
// value has one writer and the order of every sum is fixed: no atomics, no dependence on the width of the task. The global
// loads of PFA_AHEAD rows M are issued before the first of them is added, since only the additions have an order to keep.
// The row is then read out through E2's columns (which zeroes the buffer again), written to r[bl] if asked for, and folded
// into the task's maxima: registers for the first PFA_KEEP columns of every thread, beyond them part[y][row of E2] in global
// memory, every entry read and written by the same thread each time. drg_max_kernel folds the slices, the blocks and the
// caller's coefficients.
// Rows cost sum over M in out(A) of deg(M), from 10^2 to 10^6 within one network. The host orders them by falling cost and
// the states are cut into many more slices than the device has room for, so that the heavy tasks start first and the light
// ones fill in behind them; the rows above a cost threshold are taken by a workgroup of 256 (a barrier after every M), the
// others by a single wavefront each (LDS operations of one wavefront complete in order: no barrier at all).
#include "pfa.hpp"

#include <algorithm>

namespace kin {

// WG == 64: the task is one wavefront, whose LDS operations are issued and completed in program order - only the compiler
// has to be kept from moving them across the point.
template <int WG>
__device__ __forceinline__ void pfa_sync() {
  if (WG == 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// acc has a spare slot behind the species, acc[N]: lanes without a target add 0.0 to it instead of being masked off
__host__ __device__ inline int pfa_row_len(int N) { return (N + 2) & ~1; }
__host__ __device__ inline size_t pfa_lds_bytes(int N) { return (size_t)pfa_row_len(N) * 8 + (size_t)PFA_CHUNK * 24; }

constexpr int PFA_OVERSUBSCRIBE = 4;      // tasks per wavefront the device holds
constexpr int PFA_AHEAD = 4;      // rows M whose loads are in flight together
constexpr int PFA_KEEP = 6;       // columns of the E2 row per thread whose maximum lives in registers

// KEEP = PFA_KEEP, or 0 when the per-state r is asked for (a.r is looked at in that form only: every column goes through part)
template <int WG, int KEEP>
__global__ __launch_bounds__(WG) void pfa_second_kernel(PfaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char pfa_lds[];
  double* acc = (double*)pfa_lds;                              // [N] and the spare slot, zero between two rows
  double* st_p = acc + pfa_row_len(a.N);                       // the staged out-edges of A: rp_AM, rc_AM, the row of M
  double* st_c = st_p + PFA_CHUNK;
  int32_t* st_beg = (int32_t*)(st_c + PFA_CHUNK);
  int32_t* st_end = st_beg + PFA_CHUNK;
  const int tid = threadIdx.x, Y = a.Y, y = (int)(blockIdx.x % (unsigned)Y);
  const int32_t A = a.order[blockIdx.x / (unsigned)Y];
  const int32_t a0 = a.rowptr[A], a1 = a.rowptr[A + 1], z0 = a.rowptr2[A], z1 = a.rowptr2[A + 1];
  const int32_t* __restrict__ col = a.colidx;
  const bool one_chunk = a1 - a0 <= PFA_CHUNK;                 // the rows of the M are staged once for all the states
  double* part = a.part + (size_t)y * (size_t)a.E2;
  for (int i = tid; i <= a.N; i += WG) acc[i] = 0.0;
  int32_t Bk[KEEP ? KEEP : 1]; double mk[KEEP ? KEEP : 1];
#pragma unroll
  for (int k = 0; k < KEEP; k++) {
    const int32_t z = z0 + tid + k * WG;
    Bk[k] = z < z1 ? a.colidx2[z] : a.N;
    mk[k] = 0.0;
  }
  for (int32_t z = z0 + tid + KEEP * WG; z < z1; z += WG) part[z] = 0.0;
  const int nk = min(KEEP, (z1 - z0 + WG - 1) / WG);           // register columns in use
  bool staged = false;
  pfa_sync<WG>();
  for (int bl = y; bl < a.nb; bl += Y) {
    if (a.seg_n) {                    // (the same in every thread of the grid)
      const int64_t gb = a.b0 + bl;
      if (gb % a.L >= a.seg_n[gb / a.L]) continue;
    }
    const double* __restrict__ rp = a.rp + (size_t)bl * (size_t)a.E;
    const double* __restrict__ rc = a.rc + (size_t)bl * (size_t)a.E;
    for (int32_t c0 = a0; c0 < a1; c0 += PFA_CHUNK) {
      const int n = min(PFA_CHUNK, a1 - c0);
      if (tid < n) {
        const int32_t e = c0 + tid, M = col[e];
        const double p = rp[e], c = rc[e];
        st_p[tid] = p; st_c[tid] = c;
        if (!staged) { st_beg[tid] = a.rowptr[M]; st_end[tid] = a.rowptr[M + 1]; }
        acc[M] += p + c;              // the first generation (before any M of this chunk is added: M is no target of itself)
      }
      staged = one_chunk;
      pfa_sync<WG>();
      for (int j0 = 0; j0 < n; j0 += PFA_AHEAD) {
        int32_t Bq[PFA_AHEAD]; double vq[PFA_AHEAD];
#pragma unroll
        for (int x = 0; x < PFA_AHEAD; x++) {      // the first WG targets of each M: all loads, then the additions in order
          const int j = min(j0 + x, n - 1);
          const int32_t f = st_beg[j] + tid;
          const bool on = j0 + x < n && f < st_end[j];
          Bq[x] = on ? col[f] : a.N;
          vq[x] = on ? st_p[j] * rp[f] + st_c[j] * rc[f] : 0.0;
        }
#pragma unroll
        for (int x = 0; x < PFA_AHEAD; x++) {
          if (j0 + x >= n) break;
          const int j = j0 + x;
          acc[Bq[x]] += vq[x];
          const int32_t f1 = st_end[j];
          if (f1 - st_beg[j] > WG) {               // (uniform) a long M: its further targets
            const double p = st_p[j], c = st_c[j];
            for (int32_t f = st_beg[j] + tid + WG; f < f1; f += WG) acc[col[f]] += p * rp[f] + c * rc[f];
          }
          pfa_sync<WG>();             // the next M may hit the same B (and, after the last one, the stage is free again)
        }
      }
    }
    if (tid == 0) acc[A] = 0.0;       // A -> M -> A is no pair of E2 (nothing below reads acc[A])
#pragma unroll
    for (int k = 0; k < KEEP; k++) {
      if (k >= nk) break;             // (uniform)
      const double v = acc[Bk[k]];
      acc[Bk[k]] = 0.0;
      mk[k] = fmax(mk[k], v);
    }
    double* r = (KEEP == 0 && a.r) ? a.r + (size_t)bl * (size_t)a.E2 : nullptr;
    for (int32_t z = z0 + tid + KEEP * WG; z < z1; z += WG) {
      const int32_t B = a.colidx2[z];
      const double v = acc[B];
      acc[B] = 0.0;
      if (r) r[z] = v;
      part[z] = fmax(part[z], v);
    }
    pfa_sync<WG>();
  }
#pragma unroll
  for (int k = 0; k < KEEP; k++)
    if (z0 + tid + k * WG < z1) part[z0 + tid + k * WG] = mk[k];
}

int pfa_slices(const PfaTables& t, int64_t nb, int n_cu) {
  // many more tasks than the device holds at a time (about 32 wavefronts per compute unit), so that the rows' uneven costs
  // even out, and part[Y][E2] within the workspace bound
  const int64_t want = ceil_div((int64_t)std::max(n_cu, 1) * 32 * PFA_OVERSUBSCRIBE, std::max<int64_t>((int64_t)t.order.size(), 1));
  const int64_t fit = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / ((size_t)std::max<int64_t>(t.E2, 1) * sizeof(double))));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(std::min(want, fit), nb), 65535));
}

template <int WG, int KEEP>
static void pfa_launch(const PfaArgs& a, int Y, hipStream_t s) {
  if (a.n_rows == 0) return;
  KIN_HIP(hipFuncSetAttribute((const void*)pfa_second_kernel<WG, KEEP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL((pfa_second_kernel<WG, KEEP>), dim3((unsigned)((int64_t)a.n_rows * Y)), dim3(WG), pfa_lds_bytes(a.N), s, a);
  KIN_HIP(hipGetLastError());
}

void launch_pfa_second(const PfaTables& t, PfaArgs a, int64_t wg_cost, int Y, hipStream_t s) {
  if (t.order.empty() || a.nb == 0) return;
  if ((int64_t)a.N > PFA_LDS_SPECIES) throw KinError(ERR_UNSUPPORTED, "PFA: the row buffer does not fit LDS");
  // order_cost falls: the rows above wg_cost come first
  const int64_t n_wg = std::partition_point(t.order_cost.begin(), t.order_cost.end(), [&](int64_t c) { return c > wg_cost; }) -
                       t.order_cost.begin();
  const int32_t* order = a.order;
  a.Y = Y;
  a.n_rows = (int)n_wg;
  if (a.r) pfa_launch<256, 0>(a, Y, s); else pfa_launch<256, PFA_KEEP>(a, Y, s);
  a.order = order + n_wg; a.n_rows = (int)((int64_t)t.order.size() - n_wg);
  if (a.r) pfa_launch<64, 0>(a, Y, s); else pfa_launch<64, PFA_KEEP>(a, Y, s);
}

}  // namespace kin
