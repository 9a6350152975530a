// Directed-relation-graph pass, stage 2 (gfx950, wave64): from the per-state reaction rates rates[nb][R] of a block of
// states (stage 1 is the flux sweep, flux_kernels.hip) to den[nb][N] and to the per-edge maxima of num / den.
// Both launches walk a gather plan (drg.hpp) the way seg_traverse does - a workgroup per long row, a wavefront per medium
// row, a wavefront per ELL group of 64 short rows - but for MANY states: a task reads the index payload of its rows once
// into registers (short and medium rows) and then gathers c |rates[a] - rates[b]| state after state; a record without a
// reverse (b < 0) contributes c |rates[a]| and reads nothing else. Every sum is formed in a fixed order (slot order per
// lane, a shuffle tree per wavefront, the four wavefronts in order), the maximum over the states is kept in a register
// by the task that owns the edge and across slices of the states through part[Y][E] and drg_max_kernel: no atomics, the
// result does not depend on how the states are cut into blocks or slices.
// SIGNED = true is DRGEP's stage 2 on the same plans and in the same order of summation, with c = nu_A carrying its sign:
// the denominator launch forms P = sum max(c w, 0) and C = sum max(-c w, 0) and writes den = max(P, C), the edge launch
// forms s = sum c w and writes r[bl][e] = min(1, |s| / den) for every state that counts - no maximum over the states.
// SPLIT (with EDGE and SIGNED) is the first-generation stage of path flux analysis (pfa.hpp): the edge launch forms the two
// parts P and C the way the denominator launch does and writes r[bl][e] = P / den and rc[bl][e] = C / den, not clipped.
#include "drg.hpp"

#include "segsum_dev.hpp"

#include <algorithm>

namespace kin {

constexpr int DRG_WG = 256, DRG_WAVES = DRG_WG / 64;
constexpr int DRG_LONG_NX = 4;      // entries per thread and pass of a long row

// NX entries of one lane: all gathers first, then the sum in slot order. c == 0 marks padding (nothing is read for it).
template <int NX>
__device__ __forceinline__ double drg_terms(const double* __restrict__ rb, const int32_t (&ia)[NX], const int32_t (&ib)[NX],
                                            const float (&c)[NX]) {
  double qa[NX], qb[NX];
#pragma unroll
  for (int x = 0; x < NX; x++) {
    const bool on = c[x] != 0.0f;
    qa[x] = on ? rb[ia[x]] : 0.0;
    qb[x] = (on && ib[x] >= 0) ? rb[ib[x]] : 0.0;
  }
  double acc = 0.0;
#pragma unroll
  for (int x = 0; x < NX; x++) acc += (double)c[x] * fabs(qa[x] - qb[x]);
  return acc;
}

// The signed sums of one lane: EDGE the plain sum s of c (qa - qb) in p, else its positive and negative parts in p and n.
struct DrgSigned { double p, n; };
template <int NX, bool EDGE>
__device__ __forceinline__ DrgSigned drg_terms_signed(const double* __restrict__ rb, const int32_t (&ia)[NX], const int32_t (&ib)[NX],
                                                      const float (&c)[NX]) {
  double qa[NX], qb[NX];
#pragma unroll
  for (int x = 0; x < NX; x++) {
    const bool on = c[x] != 0.0f;
    qa[x] = on ? rb[ia[x]] : 0.0;
    qb[x] = (on && ib[x] >= 0) ? rb[ib[x]] : 0.0;
  }
  DrgSigned acc{0.0, 0.0};
#pragma unroll
  for (int x = 0; x < NX; x++) {
    const double t = (double)c[x] * (qa[x] - qb[x]);
    if (EDGE) acc.p += t;
    else { acc.p += fmax(t, 0.0); acc.n += fmax(-t, 0.0); }
  }
  return acc;
}
template <bool EDGE>
__device__ __forceinline__ DrgSigned wave_sum(DrgSigned v) {
  v.p = wave_sum(v.p);
  if (!EDGE) v.n = wave_sum(v.n);
  return v;
}
// what a signed row stores for state bl: den = max(P, C), or r = min(1, |s| / den) (exactly 0.0 where den == 0)
template <bool EDGE, bool SPLIT>
__device__ __forceinline__ void drg_store_signed(const DrgArgs& a, int bl, int32_t dst, int32_t aux, const DrgSigned& v) {
  if (SPLIT) {
    const double d = a.den[(size_t)bl * a.N + aux];
    a.r[(size_t)bl * a.E + dst] = d > 0.0 ? v.p / d : 0.0;
    a.rc[(size_t)bl * a.E + dst] = d > 0.0 ? v.n / d : 0.0;
  } else if (EDGE) {
    const double d = a.den[(size_t)bl * a.N + aux];
    a.r[(size_t)bl * a.E + dst] = d > 0.0 ? fmin(1.0, fabs(v.p) / d) : 0.0;
  } else {
    a.den[(size_t)bl * a.N + dst] = fmax(v.p, v.n);
  }
}

// EDGE = false: den[bl][dst] = row sum. EDGE = true: m = max over the slice's states of (row sum / den[bl][aux]), part[y][dst] = m.
// SIGNED: see the head of the file (part and the maximum take no part).
template <bool EDGE, bool SIGNED = false, bool SPLIT = false>
__global__ __launch_bounds__(DRG_WG) void drg_gather_kernel(DrgArgs a) {
  static_assert(!SPLIT || (EDGE && SIGNED), "the split stage is a signed edge launch");
  constexpr bool PLAIN = EDGE && !SPLIT;      // the signed sum is the plain one s, not the two parts
  const SegPlanView& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, Y = gridDim.y, y = blockIdx.y;
  const int nb = a.nb, N = a.N, R = a.R;
  auto counts = [&](int bl) -> bool {     // (the same in every lane of the grid)
    if (!a.seg_n) return true;
    const int64_t gb = a.b0 + bl;
    return gb % a.L < a.seg_n[gb / a.L];
  };
  auto ratio = [&](int bl, int32_t aux, double num) -> double {
    const double d = a.den[(size_t)bl * N + aux];
    return d > 0.0 ? num / d : 0.0;
  };
  if ((int)blockIdx.x < p.B) {        // a long row: the whole workgroup, its payload read again for every state
    __shared__ double sh[DRG_WAVES];
    __shared__ double shn[SIGNED ? DRG_WAVES : 1];
    const int r = blockIdx.x;
    const int32_t e0 = p.blk_beg[r], e1 = p.blk_end[r], dst = p.blk_dst[r], aux = p.blk_aux[r];
    double m = 0.0;
    for (int bl = y; bl < nb; bl += Y) {
      if (!counts(bl)) continue;
      const double* rb = a.rates + (size_t)bl * R;
      double acc = 0.0;
      DrgSigned sg{0.0, 0.0};
      for (int32_t base = e0; base < e1; base += DRG_WG * DRG_LONG_NX) {
        int32_t ia[DRG_LONG_NX], ib[DRG_LONG_NX]; float c[DRG_LONG_NX];
#pragma unroll
        for (int x = 0; x < DRG_LONG_NX; x++) {
          const int32_t e = base + tid + DRG_WG * x;
          const bool ok = e < e1;
          ia[x] = ok ? p.long_a[e] : 0; ib[x] = ok ? p.long_b[e] : -1; c[x] = ok ? a.long_c[e] : 0.0f;
        }
        if (SIGNED) {
          const DrgSigned t = drg_terms_signed<DRG_LONG_NX, PLAIN>(rb, ia, ib, c);
          sg.p += t.p; sg.n += t.n;
        } else {
          acc += drg_terms<DRG_LONG_NX>(rb, ia, ib, c);
        }
      }
      if (SIGNED) {
        sg = wave_sum<PLAIN>(sg);
        if (lane == 0) { sh[tid >> 6] = sg.p; shn[tid >> 6] = sg.n; }
        __syncthreads();
        if (tid == 0) {
          DrgSigned tot{0.0, 0.0};
#pragma unroll
          for (int w = 0; w < DRG_WAVES; w++) { tot.p += sh[w]; tot.n += shn[w]; }
          drg_store_signed<EDGE, SPLIT>(a, bl, dst, aux, tot);
        }
        __syncthreads();
        continue;
      }
      acc = wave_sum(acc);
      if (lane == 0) sh[tid >> 6] = acc;
      __syncthreads();
      if (tid == 0) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < DRG_WAVES; w++) tot += sh[w];
        if (EDGE) m = fmax(m, ratio(bl, aux, tot)); else a.den[(size_t)bl * N + dst] = tot;
      }
      __syncthreads();     // sh is written again for the next state
    }
    if (EDGE && !SIGNED && tid == 0) a.part[(size_t)y * a.E + dst] = m;
    return;
  }
  const int task = ((int)blockIdx.x - p.B) * DRG_WAVES + (tid >> 6);
  if (task < p.G) {                   // 64 short rows, one per lane
    const int32_t dst = p.grp_dst[task * 64 + lane], aux = p.grp_aux[task * 64 + lane];
    const int32_t c0 = p.grp_off[task], c1 = p.grp_off[task + 1];
    static_assert(SegPlanHost::SHORT_MAX == 8, "an ELL group is eight columns at most");
    int32_t ia[8], ib[8]; float c[8];
#pragma unroll
    for (int x = 0; x < 8; x++) {
      const bool ok = c0 + x < c1;
      const int32_t e = (c0 + x) * 64 + lane;
      ia[x] = ok ? p.ell_a[e] : 0; ib[x] = ok ? p.ell_b[e] : -1; c[x] = ok ? a.ell_c[e] : 0.0f;
    }
    double m = 0.0;
    for (int bl = y; bl < nb; bl += Y) {
      if (!counts(bl)) continue;
      if (SIGNED) {
        const DrgSigned sg = drg_terms_signed<8, PLAIN>(a.rates + (size_t)bl * R, ia, ib, c);
        if (dst >= 0) drg_store_signed<EDGE, SPLIT>(a, bl, dst, aux, sg);
        continue;
      }
      const double acc = drg_terms<8>(a.rates + (size_t)bl * R, ia, ib, c);
      if (dst >= 0) {
        if (EDGE) m = fmax(m, ratio(bl, aux, acc)); else a.den[(size_t)bl * N + dst] = acc;
      }
    }
    if (EDGE && !SIGNED && dst >= 0) a.part[(size_t)y * a.E + dst] = m;
  } else if (task < p.G + p.S) {      // a medium row: four entries per lane
    const int sidx = task - p.G;
    const int32_t e0 = p.seg_beg[sidx], e1 = p.seg_end[sidx], dst = p.seg_dst[sidx], aux = p.seg_aux[sidx];
    static_assert(SegPlanHost::SEG_LEN <= 256, "a medium row is four entries per lane");
    int32_t ia[4], ib[4]; float c[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
      const int32_t e = e0 + lane + 64 * x;
      const bool ok = e < e1;
      ia[x] = ok ? p.long_a[e] : 0; ib[x] = ok ? p.long_b[e] : -1; c[x] = ok ? a.long_c[e] : 0.0f;
    }
    double m = 0.0;
    for (int bl = y; bl < nb; bl += Y) {
      if (!counts(bl)) continue;
      if (SIGNED) {
        const DrgSigned sg = wave_sum<PLAIN>(drg_terms_signed<4, PLAIN>(a.rates + (size_t)bl * R, ia, ib, c));
        if (lane == 0) drg_store_signed<EDGE, SPLIT>(a, bl, dst, aux, sg);
        continue;
      }
      const double acc = wave_sum(drg_terms<4>(a.rates + (size_t)bl * R, ia, ib, c));
      if (lane == 0) {
        if (EDGE) m = fmax(m, ratio(bl, aux, acc)); else a.den[(size_t)bl * N + dst] = acc;
      }
    }
    if (EDGE && !SIGNED && lane == 0) a.part[(size_t)y * a.E + dst] = m;
  }
}

__global__ __launch_bounds__(256) void drg_max_kernel(long long E, int Y, const double* __restrict__ part, double* __restrict__ coef,
                                                       int use_prev) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double m = use_prev ? fmax(coef[e], 0.0) : 0.0;
  for (int y = 0; y < Y; y++) m = fmax(m, part[(size_t)y * E + e]);
  coef[e] = m;
}

int drg_slices(const SegPlanView& p, int64_t nb, int n_cu) {
  // about sixteen wavefronts per compute unit: the gathers are latency bound
  const int64_t waves = (int64_t)p.B * DRG_WAVES + p.G + p.S;
  const int64_t want = ceil_div((int64_t)std::max(n_cu, 1) * 16, std::max<int64_t>(waves, 1));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, nb), 65535));
}

static unsigned drg_blocks(const SegPlanView& p) { return (unsigned)(p.B + ceil_div(p.G + p.S, DRG_WAVES)); }

void launch_drg_den(const DrgArgs& a, int Y, hipStream_t s) {
  if (drg_blocks(a.p) == 0 || a.nb == 0) return;
  hipLaunchKernelGGL((drg_gather_kernel<false>), dim3(drg_blocks(a.p), (unsigned)Y), dim3(DRG_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_drg_edges(const DrgArgs& a, int Y, hipStream_t s) {
  if (drg_blocks(a.p) == 0 || a.nb == 0) return;
  hipLaunchKernelGGL((drg_gather_kernel<true>), dim3(drg_blocks(a.p), (unsigned)Y), dim3(DRG_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_drgep_den(const DrgArgs& a, int Y, hipStream_t s) {
  if (drg_blocks(a.p) == 0 || a.nb == 0) return;
  hipLaunchKernelGGL((drg_gather_kernel<false, true>), dim3(drg_blocks(a.p), (unsigned)Y), dim3(DRG_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_drgep_edges(const DrgArgs& a, int Y, hipStream_t s) {
  if (drg_blocks(a.p) == 0 || a.nb == 0) return;
  hipLaunchKernelGGL((drg_gather_kernel<true, true>), dim3(drg_blocks(a.p), (unsigned)Y), dim3(DRG_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_pfa_split(const DrgArgs& a, int Y, hipStream_t s) {
  if (drg_blocks(a.p) == 0 || a.nb == 0) return;
  hipLaunchKernelGGL((drg_gather_kernel<true, true, true>), dim3(drg_blocks(a.p), (unsigned)Y), dim3(DRG_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

void launch_drg_max(int64_t E, int Y, const double* part, double* coef, int use_prev, hipStream_t s) {
  if (E == 0) return;
  hipLaunchKernelGGL(drg_max_kernel, dim3((unsigned)ceil_div(E, 256)), dim3(256), 0, s, (long long)E, Y, part, coef, use_prev);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
