// Cross-member statistics (gfx950, wave64): the moments, the sorted column pass (quantiles, normalised ranks), the value
// column pass (normalised values) and the correlation product. member_stats.hpp states every sum order; nothing here uses a
// global atomic, and the one LDS atomic (the sum of squared rank deviations) adds exactly representable terms to an exactly
// representable sum, so no result depends on the order threads arrive in.
//
// Layout facts the kernels rest on: a member's states are L N doubles apart, the species axis is contiguous. The moments put
// the lanes of a wavefront along the columns c = j N + i (512 B per wave-instruction) and split the participants over the
// waves; the column passes read a tile of up to 8 consecutive selected columns per participant (one 64-byte sector when the
// species are consecutive) with the tile's column as the fastest thread index. LDS images of the sorted pass are padded by two
// doubles per column: the tile's columns then start 4 banks apart and a 16-lane store group (8 columns x 2 participants) hits
// 16 different bank pairs.
#include "member_stats.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

// No contraction anywhere in this file: the compiler's default would fuse the quantile rule's product and sum, and it does so
// through __dmul_rn / __dadd_rn as well (inline functions of a header compiled under that default: their operations carry the
// permission to fuse along when inlined). Plain operators under this pragma do not; every fused multiply-add the sum orders
// name is written as __fma_rn.
#pragma clang fp contract(off)

namespace kin {

namespace {

constexpr int MS_WG = 256;
constexpr int MS_TILE = 8;               // columns per workgroup of the column passes, at most
constexpr int MS_PAD = 2;                // doubles between the LDS images of two columns
constexpr size_t MS_LDS_BUDGET = (size_t)132 << 10;   // dynamic LDS of the sorted pass (of 160 KiB per compute unit)

__device__ inline int64_t ms_col_offset(const MsColArgs& a, int64_t c) {
  const int64_t j = c / a.n_sel, s = c % a.n_sel;
  return j * a.N + (a.sel ? a.sel[s] : (int32_t)s);
}

}  // namespace

__global__ __launch_bounds__(MS_MOM_WAVES * 64) void ms_moments_kernel(MsMomArgs a) {
  constexpr int W = MS_MOM_WAVES;
  __shared__ double part[3][W][64];
  __shared__ int bad[W][64];
  __shared__ double mean_s[64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool on = c < a.C;
  const double* col = a.u + (on ? c : 0);
  const int n = a.n;
  const double inf = std::numeric_limits<double>::infinity();
  double s = 0.0, mn = inf, mx = -inf;
  int nan = 0;
  if (on) {
    // four loads in flight, added in the order of q
    int q = w;
    for (; q + 3 * W < n; q += 4 * W) {
      double x[4];
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] = col[(size_t)a.idx[q + k * W] * (size_t)a.stride];
#pragma unroll
      for (int k = 0; k < 4; k++) { s += x[k]; mn = fmin(mn, x[k]); mx = fmax(mx, x[k]); nan |= x[k] != x[k]; }
    }
    for (; q < n; q += W) {
      const double x = col[(size_t)a.idx[q] * (size_t)a.stride];
      s += x; mn = fmin(mn, x); mx = fmax(mx, x); nan |= x != x;
    }
  }
  part[0][w][lane] = s; part[1][w][lane] = mn; part[2][w][lane] = mx; bad[w][lane] = nan;
  __syncthreads();
  if (w == 0) {
    double t = part[0][0][lane];
    mn = part[1][0][lane]; mx = part[2][0][lane]; nan = bad[0][lane];
#pragma unroll
    for (int k = 1; k < W; k++) { t += part[0][k][lane]; mn = fmin(mn, part[1][k][lane]); mx = fmax(mx, part[2][k][lane]); nan |= bad[k][lane]; }
    const double m = t / (double)n;
    mean_s[lane] = m;
    if (on) {
      const double qn = std::numeric_limits<double>::quiet_NaN();
      if (a.mean) a.mean[c] = m;
      if (a.mn) a.mn[c] = nan ? qn : mn;
      if (a.mx) a.mx[c] = nan ? qn : mx;
    }
  }
  if (!a.var) return;      // (uniform over the workgroup)
  __syncthreads();
  const double m = mean_s[lane];
  double S = 0.0;
  if (on) {
    int q = w;
    for (; q + 3 * W < n; q += 4 * W) {
      double x[4];
#pragma unroll
      for (int k = 0; k < 4; k++) x[k] = col[(size_t)a.idx[q + k * W] * (size_t)a.stride];
#pragma unroll
      for (int k = 0; k < 4; k++) { const double d = x[k] - m; S = __fma_rn(d, d, S); }
    }
    for (; q < n; q += W) {
      const double d = col[(size_t)a.idx[q] * (size_t)a.stride] - m;
      S = __fma_rn(d, d, S);
    }
  }
  __syncthreads();      // part[0] was read by wave 0 before the barrier above
  part[0][w][lane] = S;
  __syncthreads();
  if (w == 0 && on) {
    double t = part[0][0][lane];
#pragma unroll
    for (int k = 1; k < W; k++) t += part[0][k][lane];
    a.var[c] = n > 1 ? t / (double)(n - 1) : t;
  }
}

__global__ __launch_bounds__(MS_WG) void ms_sorted_kernel(MsColArgs a) {
  extern __shared__ double sh[];
  __shared__ int64_t off[MS_TILE];
  __shared__ int bad[MS_TILE];
  __shared__ double S[MS_TILE];
  const int tid = threadIdx.x, T = a.T, P2 = a.P2, n = a.n, PS = P2 + MS_PAD;
  const int64_t cl = (int64_t)blockIdx.x * T;          // the tile's first column within the launch
  const int nt = (int)std::min<int64_t>(T, a.nc - cl);
  if (tid < MS_TILE) {
    bad[tid] = 0; S[tid] = 0.0;
    off[tid] = tid < nt ? ms_col_offset(a, a.c0 + cl + tid) : 0;
  }
  __syncthreads();
  const double inf = std::numeric_limits<double>::infinity();
  for (int e = tid; e < P2 * T; e += MS_WG) {
    const int t = e & (T - 1), q = e / T;
    double v = inf;
    if (q < n && t < nt) {
      v = a.u[(size_t)a.idx[q] * (size_t)a.stride + (size_t)off[t]];
      if (v != v) bad[t] = 1;      // (every writer stores the same value)
    }
    sh[t * PS + q] = v;
  }
  __syncthreads();
  const int half = P2 >> 1;
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int pi = tid; pi < T * half; pi += MS_WG) {
        const int t = pi / half, r = pi & (half - 1);
        const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1)), l = i | j;
        double* col = sh + t * PS;
        const double x = col[i], y = col[l];
        if ((i & k) == 0 ? x > y : x < y) { col[i] = y; col[l] = x; }
      }
      __syncthreads();
    }
  const double qn = std::numeric_limits<double>::quiet_NaN();
  if (a.q_out) {
    for (int e = tid; e < nt * a.Q; e += MS_WG) {
      const int t = e / a.Q, qi = e % a.Q;
      const double* col = sh + t * PS;
      const double h = (double)(n - 1) * a.p[qi];
      const double fl = floor(h), g = h - fl;
      const int lo = std::min((int)fl, n - 1);
      double v = col[lo];
      if (g != 0.0 && lo + 1 < n) {
        const double prod = (col[lo + 1] - v) * g;      // rounded here, then added: plain operators under this file's pragma
        v = v + prod;
      }
      a.q_out[(size_t)qi * (size_t)a.c_total + (size_t)(a.c0 + cl + t)] = bad[t] ? qn : v;
    }
  }
  if (!a.yhat) return;
  // average-tie ranks from the run of equal values around each participant's own value; the deviations go to yhat first
  const double mid = 0.5 * (double)(n + 1);
  for (int e = tid; e < n * T; e += MS_WG) {
    const int t = e & (T - 1), q = e / T;
    if (t >= nt) continue;
    const double* col = sh + t * PS;
    const double y = a.u[(size_t)a.idx[q] * (size_t)a.stride + (size_t)off[t]];
    int lo = 0, hi = n;                       // first index with col >= y
    while (lo < hi) { const int m = (lo + hi) >> 1; if (col[m] < y) lo = m + 1; else hi = m; }
    int lo2 = lo, hi2 = n;                    // first index with col > y
    while (lo2 < hi2) { const int m = (lo2 + hi2) >> 1; if (col[m] <= y) lo2 = m + 1; else hi2 = m; }
    const double d = 0.5 * (double)(lo + lo2 + 1) - mid;
    atomicAdd(&S[t], d * d);                  // exact: see member_stats.hpp
    a.yhat[(size_t)(cl + t) * (size_t)n + q] = d;
  }
  __syncthreads();
  for (int e = tid; e < n * T; e += MS_WG) {   // (every thread reads back what it wrote itself)
    const int t = e & (T - 1), q = e / T;
    if (t >= nt) continue;
    double* y = a.yhat + (size_t)(cl + t) * (size_t)n + q;
    const double Sx = S[t];
    *y = bad[t] ? qn : (Sx > 0.0 ? *y / sqrt(Sx) : 0.0);
  }
}

__global__ __launch_bounds__(MS_WG) void ms_values_kernel(MsColArgs a) {
  constexpr int LN = MS_WG / MS_TILE;      // participant lanes
  __shared__ double part[LN][MS_TILE], lo_s[LN][MS_TILE], hi_s[LN][MS_TILE];
  __shared__ double tot[MS_TILE];
  __shared__ int flat[MS_TILE];
  const int tid = threadIdx.x, t = tid & (MS_TILE - 1), ql = tid / MS_TILE, n = a.n;
  const int64_t cl = (int64_t)blockIdx.x * MS_TILE;
  const bool on = cl + t < a.nc;
  const double* col = a.u + (on ? (size_t)ms_col_offset(a, a.c0 + cl + t) : 0);
  const double inf = std::numeric_limits<double>::infinity();
  double s = 0.0, mn = inf, mx = -inf;
  if (on) for (int q = ql; q < n; q += LN) { const double x = col[(size_t)a.idx[q] * (size_t)a.stride]; s += x; mn = fmin(mn, x); mx = fmax(mx, x); }
  part[ql][t] = s; lo_s[ql][t] = mn; hi_s[ql][t] = mx;
  __syncthreads();
  if (tid < MS_TILE) {
    double x = part[0][tid];
    mn = lo_s[0][tid]; mx = hi_s[0][tid];
    for (int l = 1; l < LN; l++) { x += part[l][tid]; mn = fmin(mn, lo_s[l][tid]); mx = fmax(mx, hi_s[l][tid]); }
    tot[tid] = x / (double)n;
    flat[tid] = mn == mx;      // a constant column has no spread, whatever its mean rounds to (a NaN still shows in S)
  }
  __syncthreads();
  const double m = tot[t];
  double S = 0.0;
  if (on) for (int q = ql; q < n; q += LN) { const double d = col[(size_t)a.idx[q] * (size_t)a.stride] - m; S = __fma_rn(d, d, S); }
  __syncthreads();      // tot is read above, written below
  part[ql][t] = S;
  __syncthreads();
  if (tid < MS_TILE) {
    double x = part[0][tid];
    for (int l = 1; l < LN; l++) x += part[l][tid];
    tot[tid] = x;
  }
  __syncthreads();
  if (!on) return;
  const double Sx = (flat[t] && tot[t] == tot[t]) ? 0.0 : tot[t], root = sqrt(Sx);
  const double qn = std::numeric_limits<double>::quiet_NaN();
  double* y = a.yhat + (size_t)(cl + t) * (size_t)n;
  for (int q = ql; q < n; q += LN) {
    const double d = col[(size_t)a.idx[q] * (size_t)a.stride] - m;
    y[q] = Sx > 0.0 ? d / root : (Sx == 0.0 ? 0.0 : qn);
  }
}

constexpr int MS_CC = 16, MS_CP = 16, MS_CQ = 64;

__global__ __launch_bounds__(MS_CC * MS_CP) void ms_corr_kernel(long long nc, int n, int P, const double* __restrict__ xhat,
                                                               const double* __restrict__ yhat, double* __restrict__ out) {
  __shared__ double Ys[MS_CC][MS_CQ + 1];
  __shared__ double Xs[MS_CQ][MS_CP];
  const int tid = threadIdx.x, c = tid / MS_CP, p = tid % MS_CP;
  const long long cb = (long long)blockIdx.x * MS_CC;
  const int pb = (int)blockIdx.y * MS_CP;
  double acc = 0.0;
  for (int q0 = 0; q0 < n; q0 += MS_CQ) {
    for (int e = tid; e < MS_CC * MS_CQ; e += MS_CC * MS_CP) {
      const int cc = e / MS_CQ, qq = e % MS_CQ;
      Ys[cc][qq] = (cb + cc < nc && q0 + qq < n) ? yhat[(size_t)(cb + cc) * (size_t)n + q0 + qq] : 0.0;
    }
    for (int e = tid; e < MS_CQ * MS_CP; e += MS_CC * MS_CP) {
      const int qq = e / MS_CP, pp = e % MS_CP;
      Xs[qq][pp] = (q0 + qq < n && pb + pp < P) ? xhat[(size_t)(q0 + qq) * (size_t)P + pb + pp] : 0.0;
    }
    __syncthreads();
    const int qe = std::min(MS_CQ, n - q0);
    for (int qq = 0; qq < qe; qq++) acc = __fma_rn(Xs[qq][p], Ys[c][qq], acc);
    __syncthreads();
  }
  if (cb + c < nc && pb + p < P) out[(size_t)(cb + c) * (size_t)P + pb + p] = acc;
}

void launch_ms_moments(const MsMomArgs& a, hipStream_t s) {
  if (a.C == 0 || a.n == 0) return;
  hipLaunchKernelGGL(ms_moments_kernel, dim3((unsigned)ceil_div(a.C, 64)), dim3(MS_MOM_WAVES * 64), 0, s, a);
  KIN_HIP(hipGetLastError());
}

int ms_sorted_tile(int32_t P2) {
  int T = MS_TILE;
  while (T > 1 && (size_t)T * (size_t)(P2 + MS_PAD) * sizeof(double) > MS_LDS_BUDGET) T >>= 1;
  return T;
}

void launch_ms_sorted(const MsColArgs& a, hipStream_t s) {
  if (a.nc == 0 || a.n == 0) return;
  const size_t lds = (size_t)a.T * (size_t)(a.P2 + MS_PAD) * sizeof(double);
  if (lds > MS_LDS_BUDGET) throw KinError(ERR_UNSUPPORTED, "member statistics: a sorted column does not fit the LDS budget");
  // (per launch: the attribute is kept per device, and handles of one process may live on several)
  if (lds > ((size_t)64 << 10))
    KIN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ms_sorted_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MS_LDS_BUDGET));
  hipLaunchKernelGGL(ms_sorted_kernel, dim3((unsigned)ceil_div(a.nc, a.T)), dim3(MS_WG), lds, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_ms_values(const MsColArgs& a, hipStream_t s) {
  if (a.nc == 0 || a.n == 0) return;
  hipLaunchKernelGGL(ms_values_kernel, dim3((unsigned)ceil_div(a.nc, MS_TILE)), dim3(MS_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_ms_corr(int64_t nc, int32_t n, int32_t P, const double* xhat, const double* yhat, double* out, hipStream_t s) {
  if (nc == 0 || P == 0) return;
  hipLaunchKernelGGL(ms_corr_kernel, dim3((unsigned)ceil_div(nc, MS_CC), (unsigned)ceil_div(P, MS_CP)), dim3(MS_CC * MS_CP), 0, s,
                     (long long)nc, (int)n, (int)P, xhat, yhat, out);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
