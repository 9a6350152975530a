// Reaction importance, stage 3 (gfx950, wave64): from the per-state rates rates[nb][R] (stage 1, the flux sweep) and the
// denominators den[nb][N] (stage 2, the directed-relation-graph pass's denominator launch) of a block of states to
//   I_r = max over the states of  max over the selected species A of record(r) with nu_A != 0 of  (|nu_A| |w|) / den_A.
// One thread owns one REACTION: it keeps its partner and the record's four (species, |nu|) slots in registers and walks the
// states of its slice y. Per state it loads q = rates[b][r] (coalesced) and q' = rates[b][partner], forms |q - q'| - both
// members of a pair form the same bits, so nothing is expanded from records to reactions afterwards - and gathers den[b][A]
// of its slots through the caches: a workgroup needs at most 1 024 of the row's N values per state, so staging the row in LDS
// would move more than it saves and bound N. The product |nu| |w| is rounded once, exactly as the denominator launch rounds
// a row's only term, and every sum of non-negative terms is monotone: den_A >= fl(|nu_A| |w|), every quotient is in [0, 1],
// and a species' only record gets exactly 1.0. The maximum over the states is kept in a register and across the slices
// through part[Y][R] and drg_max_kernel: no atomics, the result does not depend on how the states are cut into blocks or slices.
#include "drg.hpp"

#include <algorithm>

namespace kin {

constexpr int RI_WG = 256;

// mask[id] = 1 for every listed id inside [0, N) (the others are passed over); mask was zeroed before. Several threads may
// store the same byte: they store the same value.
__global__ __launch_bounds__(RI_WG) void ri_mask_kernel(long long n_sel, const int64_t* __restrict__ sel, int N, uint8_t* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * RI_WG + threadIdx.x;
  if (i >= n_sel) return;
  const int64_t id = sel[i];
  if (id >= 0 && id < N) mask[id] = 1;
}

__global__ __launch_bounds__(RI_WG) void ri_kernel(RiArgs a) {
  const int r = (int)blockIdx.x * RI_WG + (int)threadIdx.x;
  const int Y = gridDim.y, y = blockIdx.y;
  const int R = a.R, N = a.N, nb = a.nb;
  if (r >= R) return;
  const int32_t partner = a.tab[r];
  const uint32_t co = (uint32_t)a.tab[(size_t)5 * R + r];
  int32_t sp[4]; double c[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    sp[j] = a.tab[(size_t)(1 + j) * R + r];
    c[j] = (double)(float)((co >> (8 * j)) & 0xffu);
    if (sp[j] >= 0 && a.mask && !a.mask[sp[j]]) sp[j] = -1;     // judged by the selected species only
  }
  double m = 0.0;
  for (int bl = y; bl < nb; bl += Y) {
    bool on = true;
    if (a.seg_n) {
      const int64_t gb = a.b0 + bl;
      on = gb % a.L < a.seg_n[gb / a.L];
    }
    double v = 0.0;
    if (on) {
      const double* rb = a.rates + (size_t)bl * R;
      const double* db = a.den + (size_t)bl * N;
      const double q = rb[r];
      const double qp = partner >= 0 ? rb[partner] : 0.0;
      double d[4];
#pragma unroll
      for (int j = 0; j < 4; j++) d[j] = sp[j] >= 0 ? db[sp[j]] : 0.0;
      const double w = fabs(q - qp);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const double t = __dmul_rn(c[j], w);
        v = fmax(v, d[j] > 0.0 ? t / d[j] : 0.0);
      }
      m = fmax(m, v);
    }
    if (a.per_state) a.per_state[(size_t)bl * R + r] = v;
  }
  a.part[(size_t)y * R + r] = m;
}

int ri_slices(int64_t R, int64_t nb, int n_cu) {
  // about sixteen wavefronts per compute unit, as the gather launches: the den reads are latency bound
  const int64_t waves = ceil_div(R, RI_WG) * (RI_WG / 64);
  const int64_t want = ceil_div((int64_t)std::max(n_cu, 1) * 16, std::max<int64_t>(waves, 1));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, nb), 65535));
}

void launch_ri_mask(int64_t n_sel, const int64_t* sel, int64_t N, uint8_t* mask, hipStream_t s) {
  KIN_HIP(hipMemsetAsync(mask, 0, (size_t)std::max<int64_t>(N, 1), s));
  if (n_sel <= 0 || N == 0) return;
  hipLaunchKernelGGL(ri_mask_kernel, dim3((unsigned)ceil_div(n_sel, RI_WG)), dim3(RI_WG), 0, s, (long long)n_sel, sel, (int)N, mask);
  KIN_HIP(hipGetLastError());
}

void launch_ri(const RiArgs& a, int Y, hipStream_t s) {
  if (a.R == 0 || a.nb == 0) return;
  hipLaunchKernelGGL(ri_kernel, dim3((unsigned)ceil_div(a.R, RI_WG), (unsigned)Y), dim3(RI_WG), 0, s, a);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
