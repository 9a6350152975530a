// DRGEP path stage (gfx950, wave64): from the per-state direct-interaction coefficients r[nb][E] of a block of states
// (stage 2: drg_kernels.hip, SIGNED) to R[nb][N], the largest product of r along any path from a target, and to the
// exact maximum of R over the states.
//
// One workgroup per state. A round is a Jacobi relaxation in pull form: every species B takes
//   new_B = max(cur_B, max over the incoming edges (A, B) of cur_A * r_AB)
// from the round's input buffer into the other one - one writer per value, no atomics, nothing read that the round
// writes. Species are taken by in-degree class (DrgTables::in_order): a lane per short species, a wavefront per medium
// one (a shuffle tree of maxima), the workgroup per long one (a collider has two incoming edges per reaction it is in).
// The two buffers are LDS when 2 N doubles fit (LDS = true: the gathers cur_A are LDS reads at random addresses; with 64
// banks of 4 bytes a wavefront's doubles are served in two halves and collide only by chance), else rows of a global
// workspace that stays in L2. Rounds repeat until one changes nothing, and never more than N times: a product of factors
// in [0, 1] is largest on a simple path, which has at most N - 1 edges, and round j has seen every path of j edges.
// Multiplication by a factor in [0, 1] is monotone in floating point as well, so the fixed point is the maximum over the
// paths of the left-to-right product and does not depend on the order of relaxation: bit-identical to any other search.
#include "drg.hpp"

namespace kin {

constexpr int DRGEP_WG = 256, DRGEP_WAVES = DRGEP_WG / 64;

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

template <bool LDS>
__global__ __launch_bounds__(DRGEP_WG) void drgep_path_kernel(DrgepPathArgs a) {
  extern __shared__ double lds_R[];        // [2][N] (LDS form)
  __shared__ double sh[DRGEP_WAVES];
  __shared__ int changed[3];               // of rounds j % 3: set in round j, read after its barrier, cleared in round j + 2
  const int bl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N;
  double* Rout = a.R + (size_t)bl * N;
  if (a.seg_n) {                           // (uniform over the workgroup)
    const int64_t gb = a.b0 + bl;
    if (!(gb % a.L < a.seg_n[gb / a.L])) {
      for (int i = tid; i < N; i += DRGEP_WG) Rout[i] = 0.0;
      if (tid == 0) a.rounds[bl] = 0;
      return;
    }
  }
  double* g = LDS ? nullptr : a.work + (size_t)bl * 2 * N;
  auto ld = [&](int i) -> double { return LDS ? lds_R[i] : g[i]; };
  auto st = [&](int i, double v) { if (LDS) lds_R[i] = v; else g[i] = v; };
  for (int i = tid; i < N; i += DRGEP_WG) st(i, 0.0);
  if (tid < 3) changed[tid] = 0;
  __syncthreads();
  for (int i = tid; i < a.n_targets; i += DRGEP_WG) {       // (a target named twice: the same store)
    const int64_t t = a.targets[i];
    if (t >= 0 && t < N) st((int)t, 1.0);
  }
  __syncthreads();
  const double* __restrict__ rs = a.r + (size_t)bl * a.E;
  const int32_t* __restrict__ in_ptr = a.in_ptr;
  const int32_t* __restrict__ in_src = a.in_src;
  const int32_t* __restrict__ in_edge = a.in_edge;
  int cur = 0, rounds = 0;
  while (rounds < N) {                     // the hard cap: see the head of the file
    const int nxt = N - cur;
    bool ch = false;
    if (tid == 0) changed[(rounds + 1) % 3] = 0;
    for (int i = tid; i < a.n_short; i += DRGEP_WG) {
      const int32_t B = a.in_order[i];
      const double old = ld(cur + B);
      double m = old;
      for (int32_t j = in_ptr[B], j1 = in_ptr[B + 1]; j < j1; j++) m = fmax(m, ld(cur + in_src[j]) * rs[in_edge[j]]);
      st(nxt + B, m);
      ch |= m != old;
    }
    for (int i = wave; i < a.n_wave; i += DRGEP_WAVES) {
      const int32_t B = a.in_order[a.n_short + i];
      double m = 0.0;
      for (int32_t j = in_ptr[B] + lane, j1 = in_ptr[B + 1]; j < j1; j += 64) m = fmax(m, ld(cur + in_src[j]) * rs[in_edge[j]]);
      m = wave_max(m);
      if (lane == 0) {
        const double old = ld(cur + B);
        m = fmax(m, old);
        st(nxt + B, m);
        ch |= m != old;
      }
    }
    for (int i = 0; i < a.n_long; i++) {   // (uniform trip count: barriers inside)
      const int32_t B = a.in_order[a.n_short + a.n_wave + i];
      double m = 0.0;
      for (int32_t j = in_ptr[B] + tid, j1 = in_ptr[B + 1]; j < j1; j += DRGEP_WG) m = fmax(m, ld(cur + in_src[j]) * rs[in_edge[j]]);
      m = wave_max(m);
      if (lane == 0) sh[wave] = m;
      __syncthreads();
      if (tid == 0) {
        const double old = ld(cur + B);
        m = old;
#pragma unroll
        for (int w = 0; w < DRGEP_WAVES; w++) m = fmax(m, sh[w]);
        st(nxt + B, m);
        ch |= m != old;
      }
      __syncthreads();                     // sh is written again for the next species
    }
    if (ch) changed[rounds % 3] = 1;
    __syncthreads();                       // the round's values and its flag are visible to the workgroup
    const int any = changed[rounds % 3];
    rounds++;
    cur = nxt;
    if (!any) break;
  }
  for (int i = tid; i < N; i += DRGEP_WG) Rout[i] = ld(cur + i);
  if (tid == 0) a.rounds[bl] = rounds;
}

__global__ __launch_bounds__(256) void drgep_max_kernel(long long N, long long nb, const double* __restrict__ R, double* __restrict__ imp,
                                                         int use_prev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double m = use_prev ? fmax(imp[i], 0.0) : 0.0;
  for (long long b = 0; b < nb; b++) m = fmax(m, R[(size_t)b * N + i]);
  imp[i] = m;
}

void launch_drgep_paths(const DrgepPathArgs& a, bool in_lds, hipStream_t s) {
  if (a.nb == 0 || a.N == 0) return;
  if (in_lds)
    hipLaunchKernelGGL((drgep_path_kernel<true>), dim3((unsigned)a.nb), dim3(DRGEP_WG), (size_t)2 * a.N * sizeof(double), s, a);
  else
    hipLaunchKernelGGL((drgep_path_kernel<false>), dim3((unsigned)a.nb), dim3(DRGEP_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_drgep_max(int64_t N, int64_t nb, const double* R, double* imp, int use_prev, hipStream_t s) {
  if (N == 0) return;
  hipLaunchKernelGGL(drgep_max_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, (long long)N, (long long)nb, R, imp, use_prev);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
