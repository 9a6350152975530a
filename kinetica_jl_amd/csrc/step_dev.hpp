// Device-side bodies of the step kernels, written once for the host-driven integrator (solver_kernels.hip, kernels.hip) and
// the lockstep ensemble (ensemble_kernels.inc): the arithmetic of one reaction, one GEMV row, the vector operations of a BDF
// step element by element, the corrector update with its five sums, and the reduction hand-over behind it up to the
// decision. The kernels choose the operands (kernel arguments, or the member and entry of a round's list) and call these.
// Include from .hip files only.
#pragma once
#include "kernels.hpp"
#include "segsum_dev.hpp"
#include "solver_kernels.hpp"

namespace kin {

// ------------------------------------------------------------------------------------------
// per-reaction rate and operand derivatives (make_rs mass action, solve_utils.jl:318-334): a = x0[r], b = x1[r] (< 0: none)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double mass_action_rate(double k, const double* u, int32_t a, int32_t b) {
  const double ub = b >= 0 ? u[b] : 1.0;
  return k * u[a] * ub;
}
// (d rate / d u[a], d rate / d u[b]); 2A: 2 k u in the first, single column
__device__ __forceinline__ double2 mass_action_drates(double k, const double* u, int32_t a, int32_t b) {
  double d0, d1 = 0.0;
  if (b < 0) d0 = k;
  else if (b == a) d0 = 2.0 * k * u[a];
  else { d0 = k * u[b]; d1 = k * u[a]; }
  return make_double2(d0, d1);
}

// *x_row = a[0:m] . y[0:m] by one wavefront; `sk` = the skip flag's value, requested by the caller in front of this call
__device__ __forceinline__ void gemv_row(const double* __restrict__ a, const double* __restrict__ y, int m, int sk, double* x_row) {
  const int lane = threadIdx.x & 63;
  // four independent partial sums per lane: all loads of a trip are in flight together (the row is read once,
  // the kernel is one dependent-latency chain per row otherwise); fixed order -> bitwise reproducible
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  int j = lane;
  if (j + 192 < m) {   // first trip issued before the flag is tested: an active launch does not wait for the flag alone
    const double a0 = a[j], a1 = a[j + 64], a2 = a[j + 128], a3 = a[j + 192];
    const double y0 = y[j], y1 = y[j + 64], y2 = y[j + 128], y3 = y[j + 192];
    if (sk) return;
    acc0 += a0 * y0; acc1 += a1 * y1; acc2 += a2 * y2; acc3 += a3 * y3;
    j += 256;
  } else if (sk) return;
  for (; j + 192 < m; j += 256) {
    const double a0 = a[j], a1 = a[j + 64], a2 = a[j + 128], a3 = a[j + 192];
    const double y0 = y[j], y1 = y[j + 64], y2 = y[j + 128], y3 = y[j + 192];
    acc0 += a0 * y0; acc1 += a1 * y1; acc2 += a2 * y2; acc3 += a3 * y3;
  }
  for (; j < m; j += 64) acc0 += a[j] * y[j];
  double acc = (acc0 + acc1) + (acc2 + acc3);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) *x_row = acc;
}

// ------------------------------------------------------------------------------------------
// reductions over a workgroup and over a grid
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_1024(double v, double* sh) {
  // fixed-order reduction over a 1024-thread workgroup
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < 16; i++) t += sh[i];
    sh[16] = t;
  }
  __syncthreads();
  return sh[16];
}

// the same shape for a maximum of non-negative values (NaN entries are ignored: the callers report them separately)
__device__ __forceinline__ double block_max_1024(double v, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 16; i++) t = fmax(t, sh[i]);
    sh[16] = t;
  }
  __syncthreads();
  return sh[16];
}

// Reductions over the state are spread over ceil(N / 1024) workgroups of 256 threads (four elements per
// thread, all loads in flight): each workgroup stores its partial sums, the last one to arrive (ticket in
// BdfCtrl) adds them in workgroup order - bitwise reproducible - and takes the decision. A single
// 1024-thread workgroup walking the whole state took 17 us at N = 10k, most of it load latency.
#ifndef KIN_RED_ELEMS
#define KIN_RED_ELEMS 1024
#endif
constexpr int RED_ELEMS = KIN_RED_ELEMS;   // elements per workgroup
constexpr int RED_PT = RED_ELEMS / 256;     // per thread

__device__ __forceinline__ double block_sum_256(double v, double* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// Hand-over of the per-workgroup partial sums to the workgroup that arrives last, without a cache-flushing fence
// (`__threadfence()` = buffer_wbl2 + buffer_inv, ~3.5 us on gfx950 - a third of these kernels' duration): the partials
// are stored write-through past L2 (relaxed agent-scope stores = `sc1`), the storing lane drains them (`s_waitcnt
// vmcnt(0)`) and then takes its ticket with an agent-scope atomic; the workgroup whose ticket is the last one reads
// the partials with `sc1` loads (sum_partials) after its atomic has returned. One storing lane per workgroup, 8-byte
// granules, one workgroup per CU: the form MI355X_MICROARCH.md lists as valid for inter-workgroup hand-offs.
__device__ __forceinline__ void store_partial(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// true in exactly one workgroup per launch: the one that arrives last, after every partial is visible.
// Call from all threads; thread 0 must be the one that stored the partials (store_partial).
__device__ __forceinline__ bool last_block_arrives(BdfCtrl* ctrl, int* flag) {
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = __hip_atomic_fetch_add(&ctrl->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = (t == (int)gridDim.x - 1);
    if (*flag) __hip_atomic_store(&ctrl->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
  }
  __syncthreads();
  return *flag != 0;
}

__device__ __forceinline__ double sum_partials(const double* part, int n) {
  double t = 0.0;
  for (int g = 0; g < n; g++) t += __hip_atomic_load(part + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // past this CU's L1
  return t;
}

// A workgroup's five partial sums sit in ONE 128-byte line of their own (RED_SLOT doubles apart): write-through stores of 60
// workgroups into shared lines serialise at the memory side - 325 stores took ~45 us of a 55 us launch with the sums of all
// workgroups interleaved (part[q * G + g]), and ~7 of the 10.7 us of the 10-workgroup launch before it.
constexpr int RED_SLOT = 16;
// The five sums of a corrector launch from the workgroups' partial sums: by the first wavefront of the workgroup that arrived
// last, one partial per lane and round (all loads in flight together), fixed butterfly order - bitwise reproducible. (A
// single thread adding them one `sc1` load after the other was fine for 10 workgroups and is ~0.2-1 us per partial: the
// fused launch below has 60 workgroups at 10k species.)
__device__ __forceinline__ void newton_totals(const double* part, int G, double (&tot)[5]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 5; q++) {
    double v = 0.0;
    for (int g = lane; g < G; g += 64) v += __hip_atomic_load(part + g * RED_SLOT + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot[q] = wave_sum(v);
  }
}

// The decision of a corrector iteration, taken by ONE thread of the workgroup that arrived last (all partial sums are
// visible to it): norm of the update, contraction rate, converged / diverged / go on, and - when converged - the step's
// error-test norms; publishes the control block to the host when the attempt is decided (or `publish_always`).
struct NewtonDecide {
  int N, iter, maxit;
  double tol, rate_max, crate0, tol_first, dy_first_max;
  int crate_from_ctrl, ban_negatives;
  BdfCtrl* ctrl; const double* tot;   // tot[5]: the launch's sums (update, error test of order / -1 / +1, negative entries)
  BdfCtrl* host_ctrl; unsigned long long* host_seq; unsigned long long seq; int publish_always;
};
__device__ __forceinline__ void newton_decide(const NewtonDecide& a) {
  const int N = a.N, iter = a.iter, maxit = a.maxit, publish_always = a.publish_always;
  const double tol = a.tol, rate_max = a.rate_max, tol_first = a.tol_first, dy_first_max = a.dy_first_max;
  BdfCtrl* ctrl = a.ctrl; BdfCtrl* host_ctrl = a.host_ctrl;
  const double crate0 = (a.crate_from_ctrl && iter == 0) ? ctrl->crate : a.crate0;
  unsigned long long* host_seq = a.host_seq; const unsigned long long seq = a.seq;
  {
    const double tot = a.tot[0];
    const double old = ctrl->dy_norm_old;
    const double dy_norm = sqrt(tot / (double)N);
    const bool nonfinite = !isfinite(tot);
    const bool have_rate = iter > 0;
    const double rate = have_rate ? dy_norm / old : 0.0;
    // CVODE's carried convergence rate: every factorisation keeps the contraction it has shown (crate <- max(0.3 crate,
    // rate) after each iteration with a rate; 1 = unknown, set by the host when the factorisation is made). It lets the
    // FIRST iteration of a step be judged like the later ones instead of always being followed by a second one.
    double crate = iter == 0 ? crate0 : ctrl->crate;
    if (have_rate && !nonfinite) crate = fmax(0.3 * crate, rate);
    ctrl->crate = crate;
    bool diverged = nonfinite;
    // rate_max < 1 (a reused factorisation): a contraction slower than that means the matrix no longer matches the
    // Jacobian well enough for the error of the iteration to be judged from two or three corrections
    if (!diverged && have_rate) {
      double rp = rate;                                     // rate^(maxit - iter), 1 <= maxit - iter <= 3
      for (int e = 1; e < maxit - iter; e++) rp *= rate;
      if (rate >= rate_max || rp / (1.0 - rate) * dy_norm > tol) diverged = true;
    }
    ctrl->n_iter = iter + 1;
    ctrl->dy_norm = dy_norm;
    bool done = true, converged = false;
    if (diverged) { ctrl->nonfinite = nonfinite; }
    else if (dy_norm == 0.0 || (have_rate && rate / (1.0 - rate) * dy_norm < tol) ||
             (!have_rate && (dy_norm < tol || (crate0 < 1.0 && dy_norm <= dy_first_max && crate0 / (1.0 - crate0) * dy_norm < tol_first)))) {
      converged = true;                             // (first-iteration acceptance as in ode15s / CVODE)
    }
    else {
      ctrl->dy_norm_old = dy_norm;
      done = iter == maxit - 1;
    }
    if (converged) {
      const double te = a.tot[1];
      ctrl->err_norm = sqrt(te / (double)N);
      ctrl->err_m_norm = sqrt(a.tot[2] / (double)N);
      ctrl->err_p_norm = sqrt(a.tot[3] / (double)N);
      ctrl->any_negative = a.tot[4] > 0.0 ? (a.tot[4] >= BDF_NEG_MARK ? 3 : 1) : 0;   // bit 1: a species below -BDF_NEG_DEEP weights
      if (!isfinite(te)) ctrl->nonfinite = 1;
    }
    ctrl->converged = converged ? 1 : 0;
    ctrl->newton_done = done ? 1 : 0;
    // the verdict the host will reach from the same numbers (solver.cpp, step()): an accepted step with nothing that makes
    // the next one more than a continuation (every allowed iteration used = the host may drop the factorisation)
    ctrl->spec_go = (done && converged && !ctrl->nonfinite && !ctrl->lu_bad && !(a.ban_negatives && ctrl->any_negative) && !(ctrl->any_negative & 2) &&
                     !(ctrl->err_norm > 1.0) && iter + 1 < maxit) ? 1 : 0;
    if ((done || publish_always) && host_ctrl) {
      *host_ctrl = *ctrl;
      __threadfence_system();
      *(volatile unsigned long long*)host_seq = seq;
    }
  }
}

// ------------------------------------------------------------------------------------------
// The corrector update of one species and the five sums it feeds. `F` names the operands (NewtonFuse, or NewtonOps below):
// N, order, scale, y, d, D, atol, rtol and the error constants ec, ec_m, ec_p of order, order - 1, order + 1.
// ------------------------------------------------------------------------------------------
struct NewtonOps { int N, order; const double* scale; double* y; double* d; const double* D; double atol, rtol, ec, ec_m, ec_p; };
struct NewtonElem { double sc, yy, dd, dm, dp; };
struct NewtonSums { double s = 0.0, se = 0.0, sm = 0.0, sp = 0.0, neg = 0.0; };

// everything the update needs of species sp (< 0: none), requested together
template <class F>
__device__ __forceinline__ NewtonElem newton_pre(const F& f, int32_t sp) {
  NewtonElem e{1.0, 0.0, 0.0, 0.0, 0.0};
  if (sp < 0) return e;
  e.sc = f.scale[sp]; e.yy = f.y[sp]; e.dd = f.d[sp];
  if (f.order > 1) e.dm = f.D[(size_t)f.order * f.N + sp];
  if (f.order < 5) e.dp = f.D[(size_t)(f.order + 1) * f.N + sp];
  return e;
}
// y += dy, d += dy in `e`, and the species' terms of the sums: the update's norm and the error test of the state after this
// iteration (a non-finite update or state makes its sum non-finite: one reduction carries both the norm and the flag)
template <class F>
__device__ __forceinline__ void newton_apply(const F& f, double dy, NewtonElem& e, NewtonSums& t) {
  const double q = dy / e.sc;
  t.s += q * q;
  e.yy += dy; e.dd += dy;
  const double sce = f.atol + f.rtol * fabs(e.yy);
  if (e.yy < 0.0) t.neg = fmax(t.neg, e.yy < -BDF_NEG_DEEP * sce ? BDF_NEG_MARK : 1.0);
  const double er = f.ec * e.dd / sce;
  t.se += er * er + (isfinite(e.yy) ? 0.0 : INFINITY);
  if (f.order > 1) { const double em = f.ec_m * (e.dm + e.dd) / sce; t.sm += em * em; }
  if (f.order < 5) { const double ep = f.ec_p * (e.dd - e.dp) / sce; t.sp += ep * ep; }
}
template <class F>
__device__ __forceinline__ void newton_store(const F& f, int32_t sp, const NewtonElem& e) {
  f.y[sp] = e.yy; f.d[sp] = e.dd;
}

// What follows the element loop in every corrector launch: the five sums over the workgroup (one pair of barriers), the
// workgroup's partials into its slot of `part`, the ticket, and in the workgroup that arrived last the totals and the
// decision. `between()` runs behind the ticket: the state update of the unfused kernels is off the critical path of the
// decision, its stores go out while the ticket travels. PAIRED: the four wavefronts' sums as (0 + 1) + (2 + 3) - the unfused
// kernels -, else one after the other from 0.0 - the fused launch, with 4 or 16 wavefronts; the two roundings differ.
template <int WAVES, bool PAIRED, class Between>
__device__ __forceinline__ void newton_finish(NewtonSums t, double* part, NewtonDecide dec, Between between) {
  static_assert(!PAIRED || WAVES == 4, "the paired order is written for four wavefronts");
  __shared__ double sh[5 * WAVES];
  __shared__ int last;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    t.s += __shfl_down(t.s, off, 64); t.se += __shfl_down(t.se, off, 64); t.sm += __shfl_down(t.sm, off, 64);
    t.sp += __shfl_down(t.sp, off, 64); t.neg += __shfl_down(t.neg, off, 64);
  }
  if (lane == 0) { sh[5 * wv] = t.s; sh[5 * wv + 1] = t.se; sh[5 * wv + 2] = t.sm; sh[5 * wv + 3] = t.sp; sh[5 * wv + 4] = t.neg; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 5; q++) {
      double tot = 0.0;
      if (PAIRED) tot = (sh[q] + sh[5 + q]) + (sh[10 + q] + sh[15 + q]);
      else {
#pragma unroll
        for (int w = 0; w < WAVES; w++) tot += sh[5 * w + q];     // fixed order
      }
      store_partial(part + blockIdx.x * RED_SLOT + q, tot);
    }
  }
  const bool is_last = last_block_arrives(dec.ctrl, &last);
  between();
  if (!is_last || threadIdx.x >= 64) return;
  double tot[5];
  newton_totals(part, gridDim.x, tot);
  dec.tot = tot;
  if (threadIdx.x == 0) newton_decide(dec);
}

// The unfused corrector launch of one trajectory: RED_ELEMS elements of the state per 256-thread workgroup, four per thread,
// all loads of a thread in flight together; `decided` is tested when they are back. dy = upd * W[xloc[i]] (upd = 2 / (1 + c /
// c_fact): reused factorisation).
__device__ __forceinline__ void newton_rows(const NewtonOps& f, const int32_t* __restrict__ xloc, const double* __restrict__ W, double upd,
                                            int decided, double* part, const NewtonDecide& dec) {
  const int i0 = blockIdx.x * RED_ELEMS + threadIdx.x;
  int32_t xl[RED_PT]; double dy[RED_PT]; NewtonElem e[RED_PT];
#pragma unroll
  for (int x = 0; x < RED_PT; x++) {
    const int i = i0 + 256 * x;
    xl[x] = i < f.N ? xloc[i] : -1;
    e[x] = newton_pre(f, i < f.N ? i : -1);
  }
  if (decided) return;
#pragma unroll
  for (int x = 0; x < RED_PT; x++) dy[x] = xl[x] >= 0 ? upd * W[xl[x]] : 0.0;
  NewtonSums t;
#pragma unroll
  for (int x = 0; x < RED_PT; x++)
    if (i0 + 256 * x < f.N) newton_apply(f, dy[x], e[x], t);
  newton_finish<4, true>(t, part, dec, [&] {
#pragma unroll
    for (int x = 0; x < RED_PT; x++)
      if (i0 + 256 * x < f.N) newton_store(f, i0 + 256 * x, e[x]);
  });
}

// ------------------------------------------------------------------------------------------
// BDF vector operations, one element (algorithm: solver.cpp). D is the backward-difference array [BDF_D_ROWS][N].
// ------------------------------------------------------------------------------------------
// the predictor opens a corrector attempt: it also clears the attempt's control block (what a separate one-thread launch
// used to do); done = 1: a predictor on its own, the iterations behind it stay no-ops
__device__ __forceinline__ void open_attempt(BdfCtrl* ctrl, int done) {
  ctrl->newton_done = done; ctrl->converged = 0; ctrl->n_iter = 0; ctrl->nonfinite = 0; ctrl->any_negative = 0; ctrl->ticket = 0;
  ctrl->dy_norm_old = 0.0; ctrl->dy_norm = 0.0; ctrl->err_norm = 0.0; ctrl->err_m_norm = 0.0; ctrl->err_p_norm = 0.0;
}

struct PredictOut { double* y; double* psi; double* d; double* scale; double alpha_o, atol, rtol; };
// what the predictor leaves of element i: yp = sum_j D[j], ps = sum_j gamma[j] D[j] over j <= order
__device__ __forceinline__ void predict_store(const PredictOut& o, int i, double yp, double ps) {
  o.y[i] = yp;
  o.psi[i] = ps / o.alpha_o;
  o.d[i] = 0.0;
  o.scale[i] = o.atol + o.rtol * fabs(yp);
}
__device__ __forceinline__ void predict_elem(const double* D, int N, int i, int order, const double* gamma, const PredictOut& o) {
  double yp = D[i], ps = 0.0;
  for (int j = 1; j <= order; j++) {
    const double dj = D[(size_t)j * N + i];
    yp += dj;
    ps += dj * gamma[j];
  }
  predict_store(o, i, yp, ps);
}

// accept of a step of `order` with correction di: the new differences; returns the new state D[0]
__device__ __forceinline__ double accept_elem(double* D, int N, int i, int order, double di) {
  D[(size_t)(order + 2) * N + i] = di - D[(size_t)(order + 1) * N + i];
  D[(size_t)(order + 1) * N + i] = di;
  double carry = di;
  for (int j = order; j >= 0; j--) {
    carry += D[(size_t)j * N + i];
    D[(size_t)j * N + i] = carry;
  }
  return carry;
}

__device__ __forceinline__ void init_D_elem(double* D, int N, int i, int nrows, double y0, double f0h) {
  D[i] = y0;
  D[(size_t)N + i] = f0h;
  for (int j = 2; j < nrows; j++) D[(size_t)j * N + i] = 0.0;
}

// dense output: D[0] + sum_j p[j] D[j]
__device__ __forceinline__ double interp_elem(const double* D, int N, int i, int order, const double* p) {
  double v = D[i];
  for (int j = 1; j <= order; j++) v += p[j] * D[(size_t)j * N + i];
  return v;
}

// norms for the initial step size, by one 1024-thread workgroup: rms(y0/sc), rms(f0/sc), rms((f1-f0)/sc),
// max |f0| / (0.1 |y0| + sc), sc = atol + rtol |y0|; f1 may be null. Also reports non-finite f.
__device__ __forceinline__ void norms_body(int N, const double* y0, const double* f0, const double* f1, double atol, double rtol,
                                           BdfCtrl* ctrl) {
  __shared__ double sh[17];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, vm = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const double yi = y0[i], fi = f0[i];
    const double sc = atol + rtol * fabs(yi);
    const double a = yi / sc, b = fi / sc;
    s0 += a * a; s1 += b * b;
    vm = fmax(vm, fabs(fi) / (0.1 * fabs(yi) + sc));
    if (!isfinite(fi)) bad = 1;
    if (f1) { const double gi = f1[i]; const double c = (gi - fi) / sc; s2 += c * c; if (!isfinite(gi)) bad = 1; }
  }
  const double t0 = block_sum_1024(s0, sh), t1 = block_sum_1024(s1, sh), t2 = block_sum_1024(s2, sh);
  const double tb = block_sum_1024((double)bad, sh);
  const double tm = block_max_1024(vm, sh);
  if (threadIdx.x == 0) {
    ctrl->scratch[0] = sqrt(t0 / (double)N);
    ctrl->scratch[1] = sqrt(t1 / (double)N);
    ctrl->scratch[2] = sqrt(t2 / (double)N);
    ctrl->scratch[3] = tm;
    ctrl->nonfinite = tb > 0.0;
  }
}

}  // namespace kin
