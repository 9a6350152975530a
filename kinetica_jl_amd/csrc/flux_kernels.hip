// Reaction-flux pass (gfx950, wave64): rate_r(u_b; k_b) = k_r u[x0_r] (x1_r >= 0 ? u[x1_r] : 1) for B states, written
// out per state and / or summed over the states with weights w_b. FP64, bandwidth shaped like the batched RHS sweep
// (kernels.hip) minus its accumulator: per state the k row streams once (16-byte non-temporal loads), u is staged in
// LDS (8 N bytes), nothing is scattered - no LDS atomics.
// Segmented form (flux_seg_kernel): one workgroup per (segment of states, part of the reactions) sums its segment itself and
// keeps the rate constants in registers while a segment's key does not change; seg_max_kernel / seg_dot_kernel next to it.
#include "flux_kernels.hpp"

#include "exp_tab.hpp"

#include <algorithm>
#include <cstdlib>

namespace kin {

FluxTables build_flux_tables(const NetworkHost& h) {
  FluxTables t;
  const int64_t R = h.R, N = h.N, P = (R + 1) / 2;
  const bool lds = N + 1 < 65536;
  t.idx32.assign((size_t)std::max<int64_t>(P, 1) * 4, 0);
  if (lds) t.idx16.assign((size_t)std::max<int64_t>(P, 1) * 2, (uint32_t)N | ((uint32_t)N << 16));
  for (int64_t j = 0; j < std::max<int64_t>(P, 1); j++)
    for (int e = 0; e < 2; e++) {
      const int64_t r = 2 * j + e;
      const int32_t a = r < R ? h.x0[r] : 0, b = r < R ? h.x1[r] : -1;
      t.idx32[4 * j + 2 * e] = a;
      t.idx32[4 * j + 2 * e + 1] = b;
      if (lds && r < R) t.idx16[2 * j + e] = (uint32_t)a | ((uint32_t)(b >= 0 ? b : N) << 16);
    }
  return t;
}

static int flux_env_int(const char* name, int dflt) {
  const char* e = getenv(name);   // (read per call: tests change it)
  return e ? atoi(e) : dflt;
}

constexpr int FLUX_BS = 1024;
constexpr size_t FLUX_LDS_MAX = 160 * 1024;
constexpr int FLUX_UPT2 = 5;     // double2 per thread of a staged state on path 0 (N <= 10 240)

FluxPlan flux_plan(int64_t B, int64_t R, int64_t N, int n_cu, bool temperature_form, bool u_aligned, int max_rows) {
  FluxPlan p;
  const int64_t P = std::max<int64_t>((R + 1) / 2, 1);
  const bool lds = flux_env_int("KIN_FLUX_LDS", 1) != 0 && (size_t)(N + 2) * 8 <= FLUX_LDS_MAX && N + 1 < 65536;
  p.path = !lds ? 2 : ((N % 2 == 0 && N >= 2 && N <= 2 * FLUX_BS * FLUX_UPT2 && u_aligned) ? 0 : 1);
  // register budget (1024 threads: 128 VGPRs per lane): a row costs 4 accumulator registers, 2 (LDS labels) or 4 (32-bit
  // ids) index registers and 4 for its rate constants in flight; the temperature form also keeps (Ea, A) of its reactions -
  // 8 more per row - and the exponential's temporaries. The caps are the largest counts that compile without scratch
  // (DESIGN 3.1c has the resource report).
  // (max_rows: the segmented pass also keeps its rate constants across states and stops at 4 rows)
  const int cap = std::min(max_rows, temperature_form ? 2 : (p.path != 0 ? 4 : 8));
  const int64_t need = ceil_div(P, (int64_t)FLUX_BS);   // rows that cover every pair
  int rows = flux_env_int("KIN_FLUX_ROWS", 0);
  if (rows <= 0) rows = (int)ceil_div(need, ceil_div(need, (int64_t)cap));   // fewest parts, then the fewest rows for them
  rows = std::min(rows, cap);
  p.rows = rows <= 1 ? 1 : rows <= 2 ? 2 : rows <= 4 ? 4 : 8;
  p.parts = (int)ceil_div(need, (int64_t)p.rows);
  // one 1024-thread workgroup per compute unit (at 128 VGPRs a SIMD holds four waves)
  p.G = (int)std::max<int64_t>(1, std::min<int64_t>(B, std::max<int64_t>(1, n_cu / p.parts)));
  return p;
}

FluxModes flux_modes(int64_t R, bool temperature_form, int64_t k_stride, unsigned k_bits, bool want_rates, unsigned rates_bits) {
  FluxModes m;
  m.k_mode = FLUX_T;
  if (!temperature_form) m.k_mode = (R % 2 == 0 && (k_stride % 2 == 0) && ((k_bits & 15) == 0)) ? FLUX_K16 : FLUX_K8;
  if (!want_rates) m.rates_mode = 0;
  else if (R % 2 == 0 && (rates_bits & 15) == 0) m.rates_mode = 1;
  else m.rates_mode = 2;
  return m;
}

static __device__ const double kFluxOne[1] = {1.0};
typedef double flux_d2 __attribute__((ext_vector_type(2)));

// A workgroup = (slice g of the states, part y of the reactions). A thread owns ROWS pairs of adjacent reactions for
// the whole launch: their operand labels and their accumulators stay in registers across its states.
// Every global load is unconditional and no loaded VALUE decides an address (the rule of sweep_reg_kernel): pairs
// beyond the last are clamped onto it (address arithmetic only); their accumulators are never written out.
// RATES: 0 = no per-state rates, 1 = written as double2 (R even, aligned), 2 = as doubles. Like the loads, the stores are
// unconditional: a pair beyond the last is clamped onto the last and stores the same values to the same place again.
template <int ROWS, int MODE, int PATH, int RATES>
__global__ __launch_bounds__(FLUX_BS) void flux_sweep_kernel(FluxArgs a) {
  constexpr int BS = FLUX_BS;
  constexpr bool LDS = PATH != 2;
  constexpr int NU = FLUX_UPT2;
  extern __shared__ double u_s[];
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  const int N = a.N, R = a.R, P = a.P, B = a.B, Pm1 = P - 1, Bm1 = B - 1, Rm1 = R - 1;
  const int j0 = (int)blockIdx.y * ROWS * BS + tid;     // pair of row i: j0 + i * BS
  uint2 ix[LDS ? ROWS : 1];
  int4 jx[LDS ? 1 : ROWS];
  double2 ea[MODE == FLUX_T ? ROWS : 1], aa[MODE == FLUX_T ? ROWS : 1];
#pragma unroll
  for (int i = 0; i < ROWS; i++) {
    const int jc = min(j0 + i * BS, Pm1);
    if (LDS) ix[i] = a.idx16[jc]; else jx[i] = a.idx32[jc];
    if (MODE == FLUX_T) {
      const int r0 = min(2 * jc, Rm1), r1 = min(2 * jc + 1, Rm1);
      ea[i] = make_double2(a.Ea[r0], a.Ea[r1]);
      aa[i] = make_double2(a.A[r0], a.A[r1]);
    }
  }
  double2 acc[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; i++) acc[i] = make_double2(0.0, 0.0);
  if (LDS && tid == 0) u_s[N] = 1.0;     // the dummy operand: serves x1 < 0, so the loop below has no branch
  // the next state's u travels global -> registers while this state's reactions are processed
  double2 un2[PATH == 0 ? NU : 1];
  (void)un2;
  auto request = [&](int b) {
    const double* ub = a.u + (size_t)min(b, Bm1) * N;
    if (PATH == 0) {
#pragma unroll
      for (int x = 0; x < NU; x++) {
        // (component-wise: a whole-vector assignment leaves the array in scratch memory, as in sweep_reg_kernel)
        const double2 t = *reinterpret_cast<const double2*>(ub + min((tid + x * BS) * 2, N - 2));
        un2[x].x = t.x; un2[x].y = t.y;
      }
    }
  };
  request(g);
  for (int b = g; b < B; b += G) {
    if (PATH == 0) {
#pragma unroll
      for (int x = 0; x < NU; x++) { const int i = (tid + x * BS) * 2; if (i < N) *reinterpret_cast<double2*>(u_s + i) = un2[x]; }
    }
    const double* ub = a.u + (size_t)b * N;
    if (PATH == 1) for (int i = tid; i < N; i += BS) u_s[i] = ub[i];    // any N that fits, any alignment: staged as it comes
    if (LDS) __syncthreads();
    request(b + G);
    const double w = *(a.w ? a.w + b : kFluxOne);
    const double* kb = MODE == FLUX_T ? nullptr : a.k + (size_t)(a.k_row ? a.k_row[b] : (int64_t)b) * (size_t)a.k_stride;
    const double RT = MODE == FLUX_T ? 8.314462618 * a.T[b] : 0.0;
    double* rb = RATES ? a.rates + (size_t)b * R : nullptr;
    // (the lane's row offsets do not depend on the state: opaque, or they are hoisted out of the state loop and held in
    // registers, one per row)
    int jl = j0;
    asm volatile("" : "+v"(jl));
    // the k row of this part: every load of a batch is requested before the first one is used
    // (all rows of the part; with eight rows AND the rates written out the registers only take four at a time)
    constexpr int KB = (ROWS <= 4 || RATES == 0) ? ROWS : 4;
#pragma unroll
    for (int i0 = 0; i0 < ROWS; i0 += KB) {
      double2 kk[KB];
#pragma unroll
      for (int x = 0; x < KB; x++) {
        if (i0 + x >= ROWS) continue;
        const int jc = min(jl + (i0 + x) * BS, Pm1);
        if (MODE == FLUX_K16) {
          // (unsigned 32-bit byte offset from the row, a wave-uniform base: no 64-bit address pair per row in flight)
          const flux_d2 v = __builtin_nontemporal_load(reinterpret_cast<const flux_d2*>(reinterpret_cast<const char*>(kb) + (uint32_t)jc * 16u));
          kk[x].x = v.x; kk[x].y = v.y;
        } else if (MODE == FLUX_K8) {
          kk[x].x = __builtin_nontemporal_load(kb + min(2 * jc, Rm1));
          kk[x].y = __builtin_nontemporal_load(kb + min(2 * jc + 1, Rm1));
        } else {
          kk[x].x = arrhenius_one(ea[i0 + x].x, aa[i0 + x].x, RT, a.has_kmax, a.k_max, a.t_mult);
          kk[x].y = arrhenius_one(ea[i0 + x].y, aa[i0 + x].y, RT, a.has_kmax, a.k_max, a.t_mult);
        }
      }
#pragma unroll
      for (int x = 0; x < KB; x++) {
        if (i0 + x >= ROWS) continue;
        const int i = i0 + x;
        double ua0, ub0, ua1, ub1;
        if (LDS) {
          uint2 q = ix[i];
          // opaque to the optimiser: the loop-invariant decode would otherwise be hoisted out of the state loop (four
          // LDS addresses per row instead of two packed words)
          asm volatile("" : "+v"(q.x), "+v"(q.y));
          ua0 = u_s[q.x & 0xffffu]; ub0 = u_s[q.x >> 16];
          ua1 = u_s[q.y & 0xffffu]; ub1 = u_s[q.y >> 16];
        } else {
          const int4 q = jx[i];
          ua0 = ub[q.x]; ub0 = *(q.y >= 0 ? ub + q.y : kFluxOne);
          ua1 = ub[q.z]; ub1 = *(q.w >= 0 ? ub + q.w : kFluxOne);
        }
        const double r0 = kk[x].x * ua0 * ub0, r1 = kk[x].y * ua1 * ub1;
        acc[i].x = __builtin_fma(w, r0, acc[i].x);
        acc[i].y = __builtin_fma(w, r1, acc[i].y);
        if (RATES) {     // touched once: non-temporal, like the k stream
          const int jc = min(jl + i * BS, Pm1);
          if (RATES == 1) {
            flux_d2 t; t.x = r0; t.y = r1;
            __builtin_nontemporal_store(t, reinterpret_cast<flux_d2*>(reinterpret_cast<char*>(rb) + (uint32_t)jc * 16u));
          } else {
            __builtin_nontemporal_store(r0, rb + 2 * jc);
            __builtin_nontemporal_store(2 * jc + 1 <= Rm1 ? r1 : r0, rb + min(2 * jc + 1, Rm1));   // R odd: the last pair has one reaction
          }
        }
      }
    }
    if (LDS) __syncthreads();    // u_s is overwritten at the top of the next trip
  }
  if (a.part) {
    double* pg = a.part + (size_t)g * R;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
      const int j = j0 + i * BS;
      if (2 * j < R) pg[2 * j] = acc[i].x;
      if (2 * j + 1 < R) pg[2 * j + 1] = acc[i].y;
    }
  }
}

// flux[r] = sum of the G partials of reaction r in slice order (fixed: bitwise reproducible, no atomics)
__global__ __launch_bounds__(256) void flux_reduce_kernel(int R, int G, const double* __restrict__ part, double* __restrict__ flux) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double s = 0.0;
  int g = 0;
  for (; g + 8 <= G; g += 8) {
    double v[8];
#pragma unroll
    for (int x = 0; x < 8; x++) v[x] = part[(size_t)(g + x) * R + r];
#pragma unroll
    for (int x = 0; x < 8; x++) s += v[x];
  }
  for (; g < G; g++) s += part[(size_t)g * R + r];
  flux[r] = s;
}

// ---- segmented pass ---------------------------------------------------------------------------------------------------
// A workgroup = (segment s, part y of the reactions); it walks the segment's rows j = 0 .. seg_n[s] - 1 in order and writes
// flux[s][.] of its part itself. Staging, labels, clamping and the rate are flux_sweep_kernel's. What the per-state pass cannot do:
// the lane's rate constants stay in registers from row to row and are loaded (k rows) or evaluated (temperatures) again
// only when the row's key - k_row[b], or the bits of T[b] - differs from the previous row's. The key is read through an address
// that depends on (s, j) only, so every lane of the workgroup takes the same side of that branch. The first row always
// loads. Rows j >= seg_n[s] are never read (the prefetch of the row behind the last is clamped onto the last).
template <int ROWS, int MODE, int PATH>
__global__ __launch_bounds__(FLUX_BS) void flux_seg_kernel(FluxSegArgs a) {
  constexpr int BS = FLUX_BS;
  constexpr bool LDS = PATH != 2;
  constexpr int NU = FLUX_UPT2;
  extern __shared__ double u_s[];
  const int tid = threadIdx.x;
  const int N = a.N, R = a.R, P = a.P, Pm1 = P - 1, Rm1 = R - 1;
  const int64_t L = a.L;
  const size_t b0 = (size_t)blockIdx.x * (size_t)L;      // first state of the segment
  int64_t n64 = a.seg_n ? a.seg_n[blockIdx.x] : L;
  n64 = n64 < 0 ? 0 : (n64 > L ? L : n64);
  const int n = (int)n64;
  const int j0 = (int)blockIdx.y * ROWS * BS + tid;     // pair of row i: j0 + i * BS
  uint2 ix[LDS ? ROWS : 1];
  int4 jx[LDS ? 1 : ROWS];
  double2 ea[MODE == FLUX_T ? ROWS : 1], aa[MODE == FLUX_T ? ROWS : 1];
#pragma unroll
  for (int i = 0; i < ROWS; i++) {
    const int jc = min(j0 + i * BS, Pm1);
    if (LDS) ix[i] = a.idx16[jc]; else jx[i] = a.idx32[jc];
    if (MODE == FLUX_T) {
      const int r0 = min(2 * jc, Rm1), r1 = min(2 * jc + 1, Rm1);
      // (the segment's own parameters: blockIdx.x par_stride doubles behind the base; stride 0: the shared rows)
      const double* Ea = a.Ea + (size_t)blockIdx.x * (size_t)a.par_stride;
      const double* A = a.A + (size_t)blockIdx.x * (size_t)a.par_stride;
      ea[i] = make_double2(Ea[r0], Ea[r1]);
      aa[i] = make_double2(A[r0], A[r1]);
    }
  }
  double2 acc[ROWS], kk[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; i++) { acc[i] = make_double2(0.0, 0.0); kk[i] = make_double2(0.0, 0.0); }
  if (LDS && tid == 0) u_s[N] = 1.0;     // the dummy operand: serves x1 < 0
  double2 un2[PATH == 0 ? NU : 1];
  (void)un2;
  auto request = [&](int j) {           // row j of the segment, j < n (the caller clamps)
    const double* ub = a.u + (b0 + (size_t)j) * N;
    if (PATH == 0) {
#pragma unroll
      for (int x = 0; x < NU; x++) {
        const double2 t = *reinterpret_cast<const double2*>(ub + min((tid + x * BS) * 2, N - 2));
        un2[x].x = t.x; un2[x].y = t.y;
      }
    }
  };
  if (n > 0) request(0);
  long long key_prev = 0;
  for (int j = 0; j < n; j++) {
    const size_t b = b0 + (size_t)j;
    if (PATH == 0) {
#pragma unroll
      for (int x = 0; x < NU; x++) { const int i = (tid + x * BS) * 2; if (i < N) *reinterpret_cast<double2*>(u_s + i) = un2[x]; }
    }
    const double* ub = a.u + b * N;
    if (PATH == 1) for (int i = tid; i < N; i += BS) u_s[i] = ub[i];
    if (LDS) __syncthreads();
    request(min(j + 1, n - 1));
    const double w = *(a.w ? a.w + b : kFluxOne);
    // the row's key (the same address in every lane)
    long long key;
    if (MODE == FLUX_T) key = __double_as_longlong(a.T[b]);
    else key = a.k_stride == 0 ? 0ll : (a.k_row ? (long long)a.k_row[b] : (long long)b);
    if (j == 0 || key != key_prev) {
      int jl = j0;
      asm volatile("" : "+v"(jl));     // (the row offsets: not hoisted out of the loop into one register per row)
      if (MODE == FLUX_T) {
        const double RT = 8.314462618 * __longlong_as_double(key);
#pragma unroll
        for (int i = 0; i < ROWS; i++) {
          kk[i].x = arrhenius_one(ea[i].x, aa[i].x, RT, a.has_kmax, a.k_max, a.t_mult);
          kk[i].y = arrhenius_one(ea[i].y, aa[i].y, RT, a.has_kmax, a.k_max, a.t_mult);
        }
      } else {
        const double* kb = a.k + (size_t)key * (size_t)a.k_stride;
#pragma unroll
        for (int i = 0; i < ROWS; i++) {    // every load of the part is requested before the first one is used
          const int jc = min(jl + i * BS, Pm1);
          if (MODE == FLUX_K16) {
            const flux_d2 v = __builtin_nontemporal_load(reinterpret_cast<const flux_d2*>(reinterpret_cast<const char*>(kb) + (uint32_t)jc * 16u));
            kk[i].x = v.x; kk[i].y = v.y;
          } else {
            kk[i].x = __builtin_nontemporal_load(kb + min(2 * jc, Rm1));
            kk[i].y = __builtin_nontemporal_load(kb + min(2 * jc + 1, Rm1));
          }
        }
      }
    }
    key_prev = key;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
      double ua0, ub0, ua1, ub1;
      if (LDS) {
        uint2 q = ix[i];
        asm volatile("" : "+v"(q.x), "+v"(q.y));   // (the loop-invariant decode stays two packed words, as in flux_sweep_kernel)
        ua0 = u_s[q.x & 0xffffu]; ub0 = u_s[q.x >> 16];
        ua1 = u_s[q.y & 0xffffu]; ub1 = u_s[q.y >> 16];
      } else {
        const int4 q = jx[i];
        ua0 = ub[q.x]; ub0 = *(q.y >= 0 ? ub + q.y : kFluxOne);
        ua1 = ub[q.z]; ub1 = *(q.w >= 0 ? ub + q.w : kFluxOne);
      }
      const double r0 = kk[i].x * ua0 * ub0, r1 = kk[i].y * ua1 * ub1;
      acc[i].x = __builtin_fma(w, r0, acc[i].x);
      acc[i].y = __builtin_fma(w, r1, acc[i].y);
    }
    if (LDS) __syncthreads();    // u_s is overwritten at the top of the next trip
  }
  double* fs = a.flux + (size_t)blockIdx.x * R;
#pragma unroll
  for (int i = 0; i < ROWS; i++) {
    const int j = j0 + i * BS;
    if (2 * j < R) fs[2 * j] = acc[i].x;
    if (2 * j + 1 < R) fs[2 * j + 1] = acc[i].y;
  }
}

// umax[s][i]: one thread per species, the segment's rows in order (colmax_kernel per segment); an empty segment gives zeros
__global__ __launch_bounds__(256) void seg_max_kernel(int N, long long L, const int64_t* __restrict__ seg_n, const double* __restrict__ U,
                                                       double* __restrict__ out) {
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i >= N) return;
  long long n = seg_n ? seg_n[blockIdx.x] : L;
  n = n < 0 ? 0 : (n > L ? L : n);
  const double* us = U + (size_t)blockIdx.x * (size_t)L * N;
  double v = 0.0;
  if (n > 0) {
    v = us[i];
    for (long long t = 1; t < n; t++) v = fmax(v, us[(size_t)t * N + i]);
  }
  out[(size_t)blockIdx.x * N + i] = v;
}

// dot[b] = sum_i w[i] U[b][i] for the rows of a segment, zeros beyond them: one 256-thread workgroup per state, the summation
// order of rowdot_kernel (lane sums, a shuffle tree per wavefront, the four wavefronts in order)
__global__ __launch_bounds__(256) void seg_dot_kernel(int N, long long L, const int64_t* __restrict__ seg_n, const double* __restrict__ U,
                                                       const double* __restrict__ w, double* __restrict__ out) {
  __shared__ double sh[4];
  const long long s = blockIdx.x / L, j = blockIdx.x % L;
  long long n = seg_n ? seg_n[s] : L;
  if (j >= n) {                       // (the same in every lane)
    if (threadIdx.x == 0) out[blockIdx.x] = 0.0;
    return;
  }
  const double* row = U + (size_t)blockIdx.x * N;
  double acc = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) acc += w[i] * row[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

template <int ROWS, int MODE, int PATH, int RATES>
static void flux_go_t(const FluxPlan& p, const FluxArgs& a, hipStream_t s) {
  const size_t smem = PATH == 2 ? 0 : (size_t)(a.N + 2) * 8;
  // per launch, not cached: the attribute belongs to the (function, device) pair and costs ~1 us
  if (PATH != 2) KIN_HIP(hipFuncSetAttribute((const void*)flux_sweep_kernel<ROWS, MODE, PATH, RATES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLUX_LDS_MAX));
  hipLaunchKernelGGL((flux_sweep_kernel<ROWS, MODE, PATH, RATES>), dim3((unsigned)p.G, (unsigned)p.parts), dim3(FLUX_BS), smem, s, a);
}

template <int ROWS, int MODE, int PATH>
static void flux_go(const FluxPlan& p, const FluxArgs& a, int rates_mode, hipStream_t s) {
  if (rates_mode == 0) return flux_go_t<ROWS, MODE, PATH, 0>(p, a, s);
  if (rates_mode == 1) return flux_go_t<ROWS, MODE, PATH, 1>(p, a, s);
  flux_go_t<ROWS, MODE, PATH, 2>(p, a, s);
}

template <int MODE, int PATH>
static void flux_go_rows(const FluxPlan& p, const FluxArgs& a, int rates_mode, hipStream_t s) {
  if (p.rows == 1) return flux_go<1, MODE, PATH>(p, a, rates_mode, s);
  if (p.rows == 2) return flux_go<2, MODE, PATH>(p, a, rates_mode, s);
  if constexpr (MODE != FLUX_T) {   // (flux_plan: the temperature form stops at 2 rows, paths 1 and 2 at 4)
    if (p.rows == 4) return flux_go<4, MODE, PATH>(p, a, rates_mode, s);
    if constexpr (PATH == 0) if (p.rows == 8) return flux_go<8, MODE, PATH>(p, a, rates_mode, s);
  }
  throw KinError(ERR_INVALID_ARG, "flux sweep: no instantiation for this row count");
}

static unsigned flux_low_bits(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); }

void launch_flux_sweep(const FluxPlan& p, const FluxArgs& a, hipStream_t s) {
  if (a.B == 0 || a.R == 0) return;
  const FluxModes m = flux_modes(a.R, a.T != nullptr, a.k_stride, flux_low_bits(a.k), a.rates != nullptr, flux_low_bits(a.rates));
  const int mode = m.k_mode;
#define KIN_FLUX_PATHS(MODE)                                        \
  do {                                                              \
    if (p.path == 0) flux_go_rows<MODE, 0>(p, a, m.rates_mode, s);  \
    else if (p.path == 1) flux_go_rows<MODE, 1>(p, a, m.rates_mode, s); \
    else flux_go_rows<MODE, 2>(p, a, m.rates_mode, s);              \
  } while (0)
  if (mode == FLUX_K16) KIN_FLUX_PATHS(FLUX_K16);
  else if (mode == FLUX_K8) KIN_FLUX_PATHS(FLUX_K8);
  else KIN_FLUX_PATHS(FLUX_T);
#undef KIN_FLUX_PATHS
  KIN_HIP(hipGetLastError());
}

void launch_flux_reduce(int64_t R, int G, const double* part, double* flux, hipStream_t s) {
  if (R == 0) return;
  hipLaunchKernelGGL(flux_reduce_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, s, (int)R, G, part, flux);
  KIN_HIP(hipGetLastError());
}

template <int ROWS, int MODE, int PATH>
static void flux_seg_go(const FluxPlan& p, const FluxSegArgs& a, hipStream_t s) {
  const size_t smem = PATH == 2 ? 0 : (size_t)(a.N + 2) * 8;
  if (PATH != 2) KIN_HIP(hipFuncSetAttribute((const void*)flux_seg_kernel<ROWS, MODE, PATH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLUX_LDS_MAX));
  hipLaunchKernelGGL((flux_seg_kernel<ROWS, MODE, PATH>), dim3((unsigned)a.S, (unsigned)p.parts), dim3(FLUX_BS), smem, s, a);
}

template <int MODE, int PATH>
static void flux_seg_go_rows(const FluxPlan& p, const FluxSegArgs& a, hipStream_t s) {
  if (p.rows == 1) return flux_seg_go<1, MODE, PATH>(p, a, s);
  if (p.rows == 2) return flux_seg_go<2, MODE, PATH>(p, a, s);
  if constexpr (MODE != FLUX_T) {   // (flux_plan with FLUX_SEG_MAX_ROWS: the temperature form stops at 2 rows, the others at 4)
    if (p.rows == 4) return flux_seg_go<4, MODE, PATH>(p, a, s);
  }
  throw KinError(ERR_INVALID_ARG, "segmented flux pass: no instantiation for this row count");
}

void launch_flux_seg(const FluxPlan& p, const FluxSegArgs& a, hipStream_t s) {
  if (a.S == 0 || a.R == 0) return;
  const int mode = flux_modes(a.R, a.T != nullptr, a.k_stride, flux_low_bits(a.k), false, 0).k_mode;
#define KIN_FLUX_SEG_PATHS(MODE)                                    \
  do {                                                              \
    if (p.path == 0) flux_seg_go_rows<MODE, 0>(p, a, s);            \
    else if (p.path == 1) flux_seg_go_rows<MODE, 1>(p, a, s);       \
    else flux_seg_go_rows<MODE, 2>(p, a, s);                        \
  } while (0)
  if (mode == FLUX_K16) KIN_FLUX_SEG_PATHS(FLUX_K16);
  else if (mode == FLUX_K8) KIN_FLUX_SEG_PATHS(FLUX_K8);
  else KIN_FLUX_SEG_PATHS(FLUX_T);
#undef KIN_FLUX_SEG_PATHS
  KIN_HIP(hipGetLastError());
}

void launch_seg_max(int N, int64_t S, int64_t L, const int64_t* seg_n, const double* u, double* umax, hipStream_t s) {
  if (S == 0 || N == 0) return;
  hipLaunchKernelGGL(seg_max_kernel, dim3((unsigned)S, (unsigned)ceil_div(N, 256)), dim3(256), 0, s, N, (long long)L, seg_n, u, umax);
  KIN_HIP(hipGetLastError());
}

void launch_seg_dot(int N, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* w, double* dot, hipStream_t s) {
  if (S * L == 0) return;
  hipLaunchKernelGGL(seg_dot_kernel, dim3((unsigned)(S * L)), dim3(256), 0, s, N, (long long)L, seg_n, u, w, dot);
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
