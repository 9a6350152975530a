// Timescale analysis (gfx950, wave64): the batched Jacobian values of a block of states and, from them, per species the
// diagonal d_i = J_ii, the absolute row sum g_i, the right-hand side f_i and the quasi-steady-state error |f_i| / |d_i|, with
// their extrema over the states (timescale.hpp; definitions: include/kinetica_hip.h).
// Stage 1 is one sweep over the reactions: a thread keeps the operands of its reaction (and its Arrhenius parameters) in
// registers and goes state after state, writing rates[bl][r] and dr[bl][2r .. 2r + 1] coalesced.
// Stage 2 walks plans the way drg_gather_kernel does - a workgroup per long row, a wavefront per medium row, a wavefront per
// group of 64 short rows - for MANY states: the entry gather reads the index payload of its rows once into registers (short
// and medium rows) and gathers c dr[src] state after state; the row pass reads the contiguous stored entries of its species
// row per state and keeps the running extrema of its slice of the states in registers. Every sum is formed in a fixed order
// (slot order per lane, a shuffle tree per wavefront, the four wavefronts in order), the extrema across slices go through
// part[Y][3][N] and ts_fold_kernel: no atomics, nothing depends on how the states are cut into blocks or slices.
#include "timescale.hpp"

#include "exp_tab.hpp"
#include "segsum_dev.hpp"
#include "step_dev.hpp"

#include <algorithm>

namespace kin {

__device__ __forceinline__ bool ts_counts(const TsCount& c, int bl) {     // (the same in every lane of the grid)
  const int32_t gb = c.b0 + bl;
  if (!c.seg_n) return gb >= c.row_begin;
  const int32_t j = gb % c.L;
  return j >= c.row_begin && j < c.seg_n[gb / c.L];
}

// ------------------------------------------------------------------------------------------
// stage 1: rates and operand derivatives of every reaction, state after state
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_rates_kernel(TsRateArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const int32_t xa = a.x0[r], xb = a.x1[r];
  double ea = 0.0, aa = 0.0;
  if (a.T) { ea = a.Ea[r]; aa = a.A[r]; }
  for (int bl = blockIdx.y; bl < a.nb; bl += gridDim.y) {
    const double* u = a.u + (size_t)bl * a.N;
    double k;
    if (a.T) k = arrhenius_one(ea, aa, 8.314462618 * a.T[bl], a.has_kmax, a.k_max, a.t_mult);
    else {
      const int64_t row = a.k_row ? a.k_row[bl] : bl;
      k = a.k[(size_t)row * (size_t)a.k_stride + r];
    }
    if (a.rates) a.rates[(size_t)bl * a.R + r] = mass_action_rate(k, u, xa, xb);
    reinterpret_cast<double2*>(a.dr + (size_t)bl * 2 * a.R)[r] = mass_action_drates(k, u, xa, xb);
  }
}

void launch_ts_rates(const TsRateArgs& a, hipStream_t s) {
  if (a.R == 0 || a.nb == 0) return;
  hipLaunchKernelGGL(ts_rates_kernel, dim3((unsigned)ceil_div(a.R, 256), (unsigned)std::min(a.nb, 65535)), dim3(256), 0, s, a);
  KIN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------
// stage 2, entry gather: jv[bl][e] = sum c dr[bl][src] along the Jacobian's contribution lists
// ------------------------------------------------------------------------------------------
// NX entries of one lane: all gathers first, then the sum in slot order. c == 0 marks padding (nothing is read for it).
template <int NX>
__device__ __forceinline__ double ts_terms(const double* __restrict__ db, const int32_t (&ia)[NX], const float (&c)[NX]) {
  double v[NX];
#pragma unroll
  for (int x = 0; x < NX; x++) v[x] = c[x] != 0.0f ? db[ia[x]] : 0.0;
  double acc = 0.0;
#pragma unroll
  for (int x = 0; x < NX; x++) acc += (double)c[x] * v[x];
  return acc;
}

__global__ __launch_bounds__(TS_WG) void ts_entry_kernel(TsEntryArgs a) {
  const SegPlanView& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, Y = gridDim.y, y = blockIdx.y;
  const int nb = a.nb;
  const size_t R2 = (size_t)2 * a.R;
  if ((int)blockIdx.x < p.B) {        // a long list: the whole workgroup, its payload read again for every state
    __shared__ double sh[TS_WAVES];
    const int r = blockIdx.x;
    const int32_t e0 = p.blk_beg[r], e1 = p.blk_end[r], dst = p.blk_dst[r];
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      const double* db = a.dr + (size_t)bl * R2;
      double acc = 0.0;
      for (int32_t base = e0; base < e1; base += TS_WG * TS_LONG_NX) {
        int32_t ia[TS_LONG_NX]; float c[TS_LONG_NX];
#pragma unroll
        for (int x = 0; x < TS_LONG_NX; x++) {
          const int32_t e = base + tid + TS_WG * x;
          const bool ok = e < e1;
          ia[x] = ok ? p.long_a[e] : 0; c[x] = ok ? p.long_c[e] : 0.0f;
        }
        acc += ts_terms<TS_LONG_NX>(db, ia, c);
      }
      acc = wave_sum(acc);
      if (lane == 0) sh[tid >> 6] = acc;
      __syncthreads();
      if (tid == 0) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < TS_WAVES; w++) tot += sh[w];
        a.jv[(size_t)bl * a.nnz + dst] = tot;
      }
      __syncthreads();     // sh is written again for the next state
    }
    return;
  }
  const int task = ((int)blockIdx.x - p.B) * TS_WAVES + (tid >> 6);
  if (task < p.G) {                   // 64 short lists, one per lane
    const int32_t dst = p.grp_dst[task * 64 + lane];
    const int32_t c0 = p.grp_off[task], c1 = p.grp_off[task + 1];
    static_assert(SegPlanHost::SHORT_MAX == 8, "an ELL group is eight columns at most");
    int32_t ia[8]; float c[8];
#pragma unroll
    for (int x = 0; x < 8; x++) {
      const bool ok = c0 + x < c1;
      const int32_t e = (c0 + x) * 64 + lane;
      ia[x] = ok ? p.ell_a[e] : 0; c[x] = ok ? p.ell_c[e] : 0.0f;
    }
    if (dst < 0) return;
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      a.jv[(size_t)bl * a.nnz + dst] = ts_terms<8>(a.dr + (size_t)bl * R2, ia, c);
    }
  } else if (task < p.G + p.S) {      // a medium list: four entries per lane
    const int sidx = task - p.G;
    const int32_t e0 = p.seg_beg[sidx], e1 = p.seg_end[sidx], dst = p.seg_dst[sidx];
    static_assert(SegPlanHost::SEG_LEN <= 256, "a medium row is four entries per lane");
    int32_t ia[4]; float c[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const int32_t e = e0 + lane + 64 * x;
      const bool ok = e < e1;
      ia[x] = ok ? p.long_a[e] : 0; c[x] = ok ? p.long_c[e] : 0.0f;
    }
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      const double acc = wave_sum(ts_terms<4>(a.dr + (size_t)bl * R2, ia, c));
      if (lane == 0) a.jv[(size_t)bl * a.nnz + dst] = acc;
    }
  }
}

// Slices of a block's states. A task walks its slice state after state, every state a chain of dependent loads, so the launch
// lasts as long as its slowest task's chain: the states are cut until the grid holds the wavefronts a compute unit can keep
// resident (32: these kernels run at 8 per SIMD) and - a long row or list takes several passes and a barrier pair per state,
// ~20 us at 10k / 50k, and there are only a few dozen of them - until the long tasks alone are four workgroups per compute unit.
static int ts_slices(int64_t waves, int64_t n_long, int64_t nb, int n_cu) {
  const int64_t cu = std::max(n_cu, 1);
  int64_t want = ceil_div(cu * 32, std::max<int64_t>(waves, 1));
  if (n_long > 0) want = std::max(want, ceil_div(cu * 4, n_long));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, nb), 65535));
}

int ts_entry_slices(const SegPlanView& p, int64_t nb, int n_cu) {
  return ts_slices((int64_t)p.B * TS_WAVES + p.G + p.S, p.B, nb, n_cu);
}

void launch_ts_entries(const TsEntryArgs& a, int Y, hipStream_t s) {
  const unsigned blocks = (unsigned)(a.p.B + ceil_div(a.p.G + a.p.S, TS_WAVES));
  if (blocks == 0 || a.nb == 0) return;
  hipLaunchKernelGGL(ts_entry_kernel, dim3(blocks, (unsigned)Y), dim3(TS_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------
// stage 2, row pass: d_i, g_i, f_i, e_i per species and state; the extrema over the slice's states
// ------------------------------------------------------------------------------------------
// the running extrema of one species over a slice's states, and what a (species, state) pair adds and stores
struct TsExt { double dmax, dmin, emax; };
__device__ __forceinline__ void ts_take(const TsRowArgs& a, int bl, int32_t i, double d, double g, double f, TsExt& m) {
  const double e = f == 0.0 ? 0.0 : (d == 0.0 ? INFINITY : fabs(f) / fabs(d));
  m.dmax = fmax(m.dmax, -d); m.dmin = fmin(m.dmin, -d); m.emax = fmax(m.emax, e);
  const size_t o = (size_t)bl * a.N + i;
  if (a.diag) a.diag[o] = d;
  if (a.err) a.err[o] = e;
  if (a.g) a.g[o] = g;
}
__device__ __forceinline__ void ts_put(const TsRowArgs& a, int y, int32_t i, const TsExt& m) {
  if (!a.part) return;
  double* q = a.part + (size_t)y * 3 * a.N + i;
  q[0] = m.dmax; q[(size_t)a.N] = m.dmin; q[(size_t)2 * a.N] = m.emax;
}

// slot q of the row table (TsTables::rows): two 16-byte loads
struct TsRow { int32_t i, e0, e1, dp, s0, s1; };
__device__ __forceinline__ TsRow ts_row(const TsRowArgs& a, int q) {
  const int4 lo = a.rows[2 * q], hi = a.rows[2 * q + 1];
  return TsRow{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y};
}

// LONG: a workgroup per long row (a grid of Bl), else four wavefront tasks per workgroup over the short groups and the medium
// rows - two launches, so that neither holds the other's scalars (together they spilled SGPRs)
template <bool LONG>
__global__ __launch_bounds__(TS_WG) void ts_row_kernel(TsRowArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, Y = gridDim.y, y = blockIdx.y;
  const int nb = a.nb;
  TsExt m{-INFINITY, INFINITY, 0.0};
  if (LONG) {                         // a long row: the whole workgroup, TS_WG * TS_LONG_NX stored entries per pass
    __shared__ double shg[TS_WAVES], shf[TS_WAVES];
    const TsRow rw = ts_row(a, 64 * a.G + a.S + (int)blockIdx.x);
    const int32_t i = rw.i, e0 = rw.e0, e1 = rw.e1, dp = rw.dp, s0 = rw.s0, s1 = rw.s1;
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      const double* jb = a.jv + (size_t)bl * a.nnz;
      const double* rb = a.rates + (size_t)bl * a.R;
      double g = 0.0, f = 0.0;
      for (int32_t base = e0; base < e1; base += TS_WG * TS_LONG_NX) {
        double v[TS_LONG_NX];
#pragma unroll
        for (int x = 0; x < TS_LONG_NX; x++) {
          const int32_t e = base + tid + TS_WG * x;
          v[x] = e < e1 ? jb[e] : 0.0;
        }
#pragma unroll
        for (int x = 0; x < TS_LONG_NX; x++) g += fabs(v[x]);
      }
      for (int32_t base = s0; base < s1; base += TS_WG * TS_LONG_NX) {     // the terms of f_i in passes of the same shape
        int32_t fr[TS_LONG_NX]; float fc[TS_LONG_NX];
#pragma unroll
        for (int x = 0; x < TS_LONG_NX; x++) {
          const int32_t q = base + tid + TS_WG * x;
          const bool ok = q < s1;
          fr[x] = ok ? a.sp_rxn[q] : 0; fc[x] = ok ? a.sp_coef[q] : 0.0f;
        }
        f += ts_terms<TS_LONG_NX>(rb, fr, fc);
      }
      g = wave_sum(g); f = wave_sum(f);
      if (lane == 0) { shg[tid >> 6] = g; shf[tid >> 6] = f; }
      __syncthreads();
      if (tid == 0) {
        double tg = 0.0, tf = 0.0;
#pragma unroll
        for (int w = 0; w < TS_WAVES; w++) { tg += shg[w]; tf += shf[w]; }
        ts_take(a, bl, i, jb[dp], tg, tf, m);
      }
      __syncthreads();     // the sums are written again for the next state
    }
    if (tid == 0) ts_put(a, y, i, m);
    return;
  }
  const int task = (int)blockIdx.x * TS_WAVES + (tid >> 6);
  if (task < a.G) {                   // 64 short rows, one per lane
    const TsRow rw = ts_row(a, task * 64 + lane);
    const int32_t i = rw.i;
    if (i < 0) return;
    static_assert(TsTables::TS_SHORT_MAX == 8, "a short row is eight stored entries at most");
    const int32_t e0 = rw.e0, n = rw.e1 - e0, dp = rw.dp - e0, s0 = rw.s0, s1 = rw.s1;
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      const double* jb = a.jv + (size_t)bl * a.nnz + e0;
      const double* rb = a.rates + (size_t)bl * a.R;
      double v[8];
#pragma unroll
      for (int x = 0; x < 8; x++) v[x] = x < n ? jb[x] : 0.0;
      double g = 0.0, d = 0.0, f = 0.0;
#pragma unroll
      for (int x = 0; x < 8; x++) { g += fabs(v[x]); d = x == dp ? v[x] : d; }
      for (int32_t q = s0; q < s1; q += 8) {     // eight terms per trip, their loads in flight together; the sum in list order
        int32_t fr[8]; float fc[8];
#pragma unroll
        for (int x = 0; x < 8; x++) {
          const bool ok = q + x < s1;
          fr[x] = ok ? a.sp_rxn[q + x] : 0; fc[x] = ok ? a.sp_coef[q + x] : 0.0f;
        }
        f += ts_terms<8>(rb, fr, fc);
      }
      ts_take(a, bl, i, d, g, f, m);
    }
    ts_put(a, y, i, m);
  } else if (task < a.G + a.S) {      // a medium row: four stored entries per lane
    const TsRow rw = ts_row(a, 64 * a.G + (task - a.G));
    static_assert(TsTables::TS_WAVE_MAX <= 256, "a medium row is four entries per lane");
    const int32_t i = rw.i, e0 = rw.e0, e1 = rw.e1, dp = rw.dp, s0 = rw.s0, s1 = rw.s1;
    for (int bl = y; bl < nb; bl += Y) {
      if (!ts_counts(a.cnt, bl)) continue;
      const double* jb = a.jv + (size_t)bl * a.nnz;
      const double* rb = a.rates + (size_t)bl * a.R;
      double v[4];
#pragma unroll
      for (int x = 0; x < 4; x++) {
        const int32_t e = e0 + lane + 64 * x;
        v[x] = e < e1 ? jb[e] : 0.0;
      }
      double g = 0.0, f = 0.0;
#pragma unroll
      for (int x = 0; x < 4; x++) g += fabs(v[x]);
      for (int32_t q = s0 + lane; q < s1; q += 64) f += (double)a.sp_coef[q] * rb[a.sp_rxn[q]];
      g = wave_sum(g); f = wave_sum(f);
      if (lane == 0) ts_take(a, bl, i, jb[dp], g, f, m);
    }
    if (lane == 0) ts_put(a, y, i, m);
  }
}

int ts_row_slices(const TsRowArgs& a, int n_cu) {
  return ts_slices((int64_t)a.Bl * TS_WAVES + a.G + a.S, a.Bl, a.nb, n_cu);
}

void launch_ts_rows(const TsRowArgs& a, int Y, hipStream_t s) {
  if (a.nb == 0) return;
  if (a.Bl > 0) hipLaunchKernelGGL(ts_row_kernel<true>, dim3((unsigned)a.Bl, (unsigned)Y), dim3(TS_WG), 0, s, a);
  const unsigned blocks = (unsigned)ceil_div(a.G + a.S, TS_WAVES);
  if (blocks > 0) hipLaunchKernelGGL(ts_row_kernel<false>, dim3(blocks, (unsigned)Y), dim3(TS_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------
// closing launches
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_fold_kernel(long long N, int Y, const double* __restrict__ part, double* __restrict__ summary,
                                                       int use_prev) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double dmax = use_prev ? summary[i] : -INFINITY, dmin = use_prev ? summary[N + i] : INFINITY, emax = use_prev ? summary[2 * N + i] : 0.0;
  for (int y = 0; y < Y; y++) {
    const double* q = part + (size_t)y * 3 * N + i;
    dmax = fmax(dmax, q[0]); dmin = fmin(dmin, q[N]); emax = fmax(emax, q[2 * N]);
  }
  summary[i] = dmax; summary[N + i] = dmin; summary[2 * N + i] = emax;
}

void launch_ts_fold(int64_t N, int Y, const double* part, double* summary, int use_prev, hipStream_t s) {
  if (N == 0) return;
  hipLaunchKernelGGL(ts_fold_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, s, (long long)N, Y, part, summary, use_prev);
  KIN_HIP(hipGetLastError());
}

void launch_ts_identity(int64_t N, double* summary, hipStream_t s) {
  launch_ts_fold(N, 0, nullptr, summary, 0, s);
}

// one workgroup per state: the maximum is exact, so its order does not matter
__global__ __launch_bounds__(256) void ts_norm_kernel(long long N, const double* __restrict__ g, TsCount cnt, double* __restrict__ norm) {
  __shared__ double sh[4];
  const int bl = blockIdx.x;
  if (!ts_counts(cnt, bl)) {
    if (threadIdx.x == 0) norm[bl] = 0.0;
    return;
  }
  const double* gb = g + (size_t)bl * N;
  double v = 0.0;
  for (long long i = threadIdx.x; i < N; i += 256) v = fmax(v, gb[i]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) norm[bl] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

void launch_ts_norm(int64_t N, int64_t nb, const double* g, const TsCount& cnt, double* norm, hipStream_t s) {
  if (nb == 0) return;
  hipLaunchKernelGGL(ts_norm_kernel, dim3((unsigned)nb), dim3(256), 0, s, (long long)N, g, cnt, norm);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
