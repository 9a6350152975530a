// Sobol first-order and total-effect indices over the members of a Saltelli design (gfx950, wave64). member_stats.hpp states
// the layout and the order of every sum; include/kinetica_hip.h the definition. One bandwidth-bound pass: no atomics, the
// cross-wave reduction goes through LDS in the fixed order.
//
// Layout facts the kernel rests on: a member's states are L N doubles apart, the species axis is contiguous. The lanes of a
// wavefront lie along 64 consecutive selected columns (512 B per wave-instruction when the species are consecutive), the
// participants are split over the workgroup's wavefronts. Per participant a wave issues the loads of a, b and of its chunk's
// c_p together - SB_CHUNK + 2 independent rows in flight per wave - before the first of them is used. The 2 + 2 SB_CHUNK
// accumulators stay in registers; a larger P is cut into chunks over grid.y, each workgroup reading a and b again.
#include "member_stats.hpp"

#include <algorithm>
#include <limits>

// No contraction: the products with the weight and the differences are rounded on their own; every fused multiply-add of the
// order is written as __fma_rn (member_stats_kernels.hip has the reason in full).
#pragma clang fp contract(off)

namespace kin {

namespace {

constexpr int W = SB_WAVES, PC = SB_CHUNK;

// the W partials of one quantity, added in the order of the waves
__device__ inline double sb_ordered(const double (*p)[64], int lane) {
  double t = p[0][lane];
#pragma unroll
  for (int k = 1; k < W; k++) t += p[k][lane];
  return t;
}

}  // namespace

__global__ __launch_bounds__(SB_WAVES * 64) void sobol_kernel(SobolArgs a) {
  __shared__ double part[PC + 1][W][64];
  __shared__ double tot[2 * PC + 2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool on = c < a.c_total;
  const int p0 = (int)blockIdx.y * PC, npc = std::min(PC, a.P - p0);
  size_t off = 0;
  if (on) {
    const int64_t j = c / a.n_sel, s = c % a.n_sel;
    off = (size_t)(j * a.N + (a.sel ? a.sel[s] : (int32_t)s));
  }
  const size_t stride = (size_t)a.stride, blk = (size_t)a.M * stride;
  const double* colA = a.u + off;
  const double* colB = colA + blk;
  const double* colC = colA + (size_t)(2 + p0) * blk;
  const int np = a.np;
  const double inf = std::numeric_limits<double>::infinity();

  // pass 1: the weighted sums of A and of B, the extremes of both
  double ta = 0.0, tb = 0.0, mn = inf, mx = -inf;
  if (on) {
#pragma unroll 4
    for (int q = w; q < np; q += W) {
      const size_t m = (size_t)a.idx[q] * stride;
      const double wq = (double)a.wt[q];
      const double x = colA[m], y = colB[m];
      ta = ta + wq * x;
      tb = tb + wq * y;
      mn = fmin(mn, fmin(x, y));
      mx = fmax(mx, fmax(x, y));
    }
  }
  part[0][w][lane] = ta; part[1][w][lane] = tb; part[2][w][lane] = mn; part[3][w][lane] = mx;
  __syncthreads();
  if (w < 2) tot[w][lane] = sb_ordered(part[w], lane);
  else if (w == 2) { double t = part[2][0][lane]; for (int k = 1; k < W; k++) t = fmin(t, part[2][k][lane]); tot[2][lane] = t; }
  else if (w == 3) { double t = part[3][0][lane]; for (int k = 1; k < W; k++) t = fmax(t, part[3][k][lane]); tot[3][lane] = t; }
  __syncthreads();
  const double dn = (double)a.n, dn2 = 2.0 * dn;
  const double mu = (tot[0][lane] + tot[1][lane]) / dn2;
  const bool flat = (tot[3][lane] - tot[2][lane] == 0.0) && mu == mu;

  // pass 2: the centred sums of A and B and this chunk's two sums per input
  double SA = 0.0, SB = 0.0, C1[PC], C2[PC];
#pragma unroll
  for (int k = 0; k < PC; k++) C1[k] = C2[k] = 0.0;
  if (on) {
#pragma unroll 2
    for (int q = w; q < np; q += W) {
      const int32_t mi = a.idx[q];
      const size_t m = (size_t)mi * stride;
      const double wq = (double)a.wt[q];
      const double x = colA[m], y = colB[m];
      double cv[PC];
#pragma unroll
      for (int k = 0; k < PC; k++)
        if (k < npc) cv[k] = colC[(size_t)k * blk + m];
      const double da = x - mu, db = y - mu;
      const double wda = wq * da, wdb = wq * db;
      SA = __fma_rn(wda, da, SA);
      SB = __fma_rn(wdb, db, SB);
#pragma unroll
      for (int k = 0; k < PC; k++)
        if (k < npc) {
          C1[k] = __fma_rn(wdb, cv[k] - x, C1[k]);
          const double e = x - cv[k];
          C2[k] = __fma_rn(wq * e, e, C2[k]);
        }
    }
  }
  // two rounds through the same LDS image: SA and the C1, then SB and the C2; quantity k is added up by wave k mod W
  part[0][w][lane] = SA;      // (part was last read before the barrier above)
#pragma unroll
  for (int k = 0; k < PC; k++) part[1 + k][w][lane] = C1[k];
  __syncthreads();
  for (int k = w; k < PC + 1; k += W) tot[k][lane] = sb_ordered(part[k], lane);
  __syncthreads();
  part[0][w][lane] = SB;
#pragma unroll
  for (int k = 0; k < PC; k++) part[1 + k][w][lane] = C2[k];
  __syncthreads();
  for (int k = w; k < PC + 1; k += W) tot[PC + 1 + k][lane] = sb_ordered(part[k], lane);
  __syncthreads();
  if (!on) return;
  const double V = flat ? 0.0 : (tot[0][lane] + tot[PC + 1][lane]) / dn2;
  if (blockIdx.y == 0 && w == 0) {
    if (a.mean) a.mean[c] = mu;
    if (a.var) a.var[c] = V;
  }
  const bool zero = a.n < 2 || V == 0.0;
  for (int k = w; k < npc; k += W) {
    const size_t o = (size_t)c * (size_t)a.P + (size_t)(p0 + k);
    if (a.S1) a.S1[o] = zero ? 0.0 : (tot[1 + k][lane] / dn) / V;
    if (a.ST) a.ST[o] = zero ? 0.0 : (tot[PC + 2 + k][lane] / dn2) / V;
  }
}

void launch_sobol(const SobolArgs& a, hipStream_t s) {
  if (a.c_total == 0 || a.np == 0 || a.P == 0) return;
  hipLaunchKernelGGL(sobol_kernel, dim3((unsigned)ceil_div(a.c_total, 64), (unsigned)ceil_div(a.P, SB_CHUNK)), dim3(SB_WAVES * 64), 0, s, a);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
