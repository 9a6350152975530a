// Device-side pieces of the deterministic segmented gather-sum and its traversal of a plan by a grid (kernels.hip:
// segsum_kernel; ensemble_kernels.inc: e_segsum_kernel; solver_kernels.hip: the solve's last gather stage fused with the
// corrector update). Include from .hip files only.
#pragma once
#include "kernels.hpp"

namespace kin {

// The store operands that do not depend on the sum (old value, pivot, psi, d) are loaded by seg_pre
// BEFORE the gather loop: these kernels are a chain of dependent global loads on a few thousand rows,
// so every load taken off the critical path is ~1 us per launch. The same goes for the skip flag
// (blind-enqueued Newton iterations): it is loaded together with the row descriptors and tested when those
// are back - a skipped launch (47 % of the second iterations at C3) ends after ONE round of loads instead of
// three, an active one does not wait for the flag any longer than it waits for its descriptors anyway.
// (The pointer and plan-view types are template parameters: the grid kernels pass plain pointers and SegPlanView, the resident
// integrator address-space-qualified ones - pointers read from a context block are generic to the compiler and would turn
// every access into a flat instruction.)
struct SegPre { double o, a, b; };
template <int OP, class OutP, class SrcP, class EX>
__device__ __forceinline__ SegPre seg_pre(OutP out, SrcP src, int32_t dst, int32_t aux, const EX& ex) {
  SegPre q{0.0, 0.0, 0.0};
  if (dst < 0) return q;
  if (OP == SEG_PROD_SUB) q.o = out[dst];
  else if (OP == SEG_PROD_SUB_DIV) { q.o = out[dst]; q.a = src[aux]; }
  else if (OP == SEG_PROD_AUXSUB) q.o = src[aux];
  else if (OP == SEG_COEF_BDF) { q.a = ex.psi[aux]; q.b = ex.d[aux]; }
  return q;
}
template <int OP, class OutP, class EX>
__device__ __forceinline__ void seg_store(OutP out, int32_t dst, double acc, const SegPre& q, const EX& ex) {
  if (OP == SEG_COEF_SET) out[dst] = acc;
  else if (OP == SEG_PROD_SUB) out[dst] = q.o - acc;
  else if (OP == SEG_PROD_SUB_DIV) out[dst] = (q.o - acc) / q.a;
  else if (OP == SEG_PROD_AUXSUB) out[dst] = q.o - acc;
  else if (OP == SEG_PROD_SET) out[dst] = acc;
  else if (OP == SEG_PROD_NEG) out[dst] = -acc;
  else out[dst] = ex.cscal * acc - q.a - q.b;
}
template <int OP> struct seg_is_prod { static constexpr bool v = (OP == SEG_PROD_SUB || OP == SEG_PROD_SUB_DIV || OP == SEG_PROD_AUXSUB || OP == SEG_PROD_SET || OP == SEG_PROD_NEG); };

__device__ __forceinline__ double wave_sum(double v) {
  // fixed butterfly order -> bitwise reproducible
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One round of NX entries per lane: all index loads, then all gathers, then the sum in slot order (two dependent loads on
// the critical path). `idx_of(x)` = payload index of this lane's x-th entry, or -1. ELL = entries of an ELL group (padding
// inside the group is marked in the payload), else the contiguous payload of medium / long rows.
// srcA: the array the first factor (or the coefficient plans' operand) is read from, srcB: the second factor's - the same
// array in the grid kernels; in the resident integrator the factor values are in global memory and the solve vectors in LDS
template <int OP, int NX, bool ELL, class View, class SrcA, class SrcB, class EX, class F>
__device__ __forceinline__ double seg_gather2(const View& p, SrcA srcA, SrcB srcB, const EX& ex, bool impl, F idx_of) {
  constexpr bool PROD = seg_is_prod<OP>::v;
  const auto A = ELL ? p.ell_a : p.long_a;
  const auto Bp = ELL ? p.ell_b : p.long_b;
  const auto C = ELL ? p.ell_c : p.long_c;
  const int32_t vbase = ELL ? p.val_base : p.val_base + p.ell_total;
  float c[NX]; int32_t ia[NX], ib[NX]; double va[NX], vb[NX];
#pragma unroll
  for (int x = 0; x < NX; x++) {
    const int32_t e = idx_of(x);
    const bool ok = e >= 0;
    ib[x] = (PROD && ok) ? Bp[e] : -1;
    if (PROD && impl) ia[x] = vbase + e; else ia[x] = ok ? A[e] : 0;
    c[x] = PROD ? (ib[x] >= 0 ? 1.0f : 0.0f) : (ok ? C[e] : 0.0f);   // product plans carry no coefficients: padding = b < 0
  }
#pragma unroll
  for (int x = 0; x < NX; x++) {
    const bool on = c[x] != 0.0f;
    va[x] = on ? srcA[ia[x]] : 0.0;
    vb[x] = (PROD && on) ? srcB[ib[x]] : 0.0;
  }
  double acc = 0.0;
#pragma unroll
  for (int x = 0; x < NX; x++) {
    if (PROD) acc += va[x] * vb[x];
    else acc += (double)c[x] * va[x];
  }
  return acc;
}

template <int OP, int NX, bool ELL, class View, class SrcP, class EX, class F>
__device__ __forceinline__ double seg_gather(const View& p, SrcP src, const EX& ex, bool impl, F idx_of) {
  return seg_gather2<OP, NX, ELL>(p, src, src, ex, impl, idx_of);
}

// The traversal of a plan by a grid of SEG_WG-thread workgroups: the first p.B take one LONG row each (whole workgroup,
// BLK_PASS entries per pass, so that all but the very longest rows are ONE round of index loads + gathers), the others
// SEG_WG / 64 wavefront tasks each (an ELL group of 64 short rows, or one medium row)
// (plans without long rows are launched with 256-thread workgroups: small workgroups start ~1.5 us sooner).
// `pre(dst, aux)` requests what the row's store needs that does not depend on the sum (dst < 0: this lane stores nothing),
// `store(dst, aux, acc, q)` takes the row's sum and what pre returned; `tail(t)` gets the wavefront tasks behind the plan's
// (t = 0, 1, ...: the grid may be larger than the plan needs). *skip_flag (optional) is loaded with the row descriptors and
// tested when those are back, see above; it is uniform over the grid, and the result is false when it was set.
template <int OP, int SEG_WG, class SrcP, class EX, class Pre, class Store, class Tail>
__device__ __forceinline__ bool seg_traverse(const SegPlanView& p, SrcP src, const EX& ex, const int* skip_flag, Pre pre, Store store,
                                             Tail tail) {
  constexpr int SEG_WAVES = SEG_WG / 64, BLK_PER_THREAD = SegPlanHost::BLK_PASS / 1024;
  const int skip = skip_flag ? *skip_flag : 0;
  const int lane = threadIdx.x & 63;
  const bool impl = p.val_base >= 0;                    // value-ordered plan: first factor of slot q = src[val_base + q]
  if (SEG_WG == 1024 && (int)blockIdx.x < p.B) {
    __shared__ double sh[SEG_WAVES];
    const int r = blockIdx.x;
    const int32_t e0 = p.blk_beg[r], e1 = p.blk_end[r];
    const int32_t bdst = p.blk_dst[r];
    const int32_t baux = p.blk_aux[r];
    if (skip) return false;      // (whole workgroup: the flag is uniform) tested once the first round of loads is back
    const auto q = pre(threadIdx.x == 0 ? bdst : -1, baux);
    double acc = 0.0;
    for (int32_t base = e0; base < e1; base += SegPlanHost::BLK_PASS)
      acc += seg_gather<OP, BLK_PER_THREAD, false>(p, src, ex, impl, [&](int x) {
        const int32_t e = base + (int32_t)threadIdx.x + 1024 * x;
        return e < e1 ? e : -1;
      });
    acc = wave_sum(acc);
    if (lane == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
#pragma unroll
      for (int w = 0; w < SEG_WAVES; w++) tot += sh[w];     // fixed order
      store(bdst, baux, tot, q);
    }
    return true;
  }
  const int task = ((int)blockIdx.x - p.B) * SEG_WAVES + (threadIdx.x >> 6);
  if (task < p.G) {
    const int32_t dst = p.grp_dst[task * 64 + lane];
    const int32_t aux = p.grp_aux[task * 64 + lane];
    const int32_t c0 = p.grp_off[task], c1 = p.grp_off[task + 1];
    if (skip) return false;
    const auto q = pre(dst, aux);
    double acc = 0.0;
    for (int32_t col = c0; col < c1; col += 8)       // a whole ELL group in one round: rows have <= 8 entries
      acc += seg_gather<OP, 8, true>(p, src, ex, impl, [&](int x) { return col + x < c1 ? (col + x) * 64 + lane : -1; });
    if (dst >= 0) store(dst, aux, acc, q);
  } else if (task < p.G + p.S) {
    const int sidx = task - p.G;
    const int32_t e0 = p.seg_beg[sidx], e1 = p.seg_end[sidx];
    const int32_t sdst = p.seg_dst[sidx];
    const int32_t saux = p.seg_aux[sidx];
    if (skip) return false;
    const auto q = pre(lane == 0 ? sdst : -1, saux);
    // four entries per lane: ONE round of index loads and ONE round of gathers, all in flight together
    static_assert(SegPlanHost::SEG_LEN <= 256, "a medium row is one round of four entries per lane");
    double acc = seg_gather<OP, 4, false>(p, src, ex, impl, [&](int x) { const int32_t e = e0 + lane + 64 * x; return e < e1 ? e : -1; });
    acc = wave_sum(acc);
    if (lane == 0) store(sdst, saux, acc, q);
  } else {
    if (skip) return false;
    tail(task - p.G - p.S);
  }
  return true;
}

// ... with the plan's own store (seg_pre / seg_store of OP into `out`)
template <int OP, int SEG_WG, class OutP, class SrcP, class EX>
__device__ __forceinline__ void seg_traverse(const SegPlanView& p, SrcP src, OutP out, const EX& ex, const int* skip_flag) {
  seg_traverse<OP, SEG_WG>(
      p, src, ex, skip_flag, [&](int32_t dst, int32_t aux) { return seg_pre<OP>(out, src, dst, aux, ex); },
      [&](int32_t dst, int32_t, double acc, const SegPre& q) { seg_store<OP>(out, dst, acc, q, ex); }, [](int) {});
}

}  // namespace kin
