// Batched kernels of the large-network ensemble (ensemble.hpp): the single-trajectory kernels of solver_kernels.hip and of
// kernels.hip with a second grid dimension - blockIdx.y = entry of the round's list (EnsOp), which names the member (EnsRep)
// and carries what the single-trajectory launch takes as kernel arguments. Every kernel here chooses its operands and calls
// the body the single-trajectory kernel calls (step_dev.hpp, segsum_dev.hpp). Included at the end of solver_kernels.hip
// (inside namespace kin).

#define ENS_ENTRY                                   \
  const EnsOp& o = ops[blockIdx.y];                 \
  const EnsRep& r = reps[o.rep]

__global__ __launch_bounds__(256) void e_vec_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  switch (o.i0) {
    case EV_LOAD_U0: r.y[i] = o.out[i]; break;
    case EV_CS_FROM_Y: r.cs[i] = r.y[i]; break;
    case EV_Y_FROM_CS_CLIPPED: { const double v = r.cs[i]; r.y[i] = v < 0.0 ? 0.0 : v; } break;
    case EV_Y_FROM_D0: r.y[i] = r.D[i]; break;
    case EV_YTMP_FROM_D0: r.ytmp[i] = r.D[i]; break;
    case EV_YTMP_AXPY: r.ytmp[i] = r.y[i] + o.d0 * r.f0[i]; break;
    case EV_SAVE_Y: o.out[i] = r.y[i]; break;
    case EV_INTERP: o.out[i] = interp_elem(r.D, N, i, o.i1, o.p); break;
    default: break;
  }
}

__global__ __launch_bounds__(256) void e_accept_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  accept_elem(r.D, N, i, o.i0, r.d[i]);
}

// D[0..5] <- M^T D[0..5] with the 6 x 6 matrix of the entry (identity outside the orders involved; bdf_change_D_kernel loops to
// the order instead: the two differ in signed zeros and in non-finite rows above the order, each keeps its form)
__global__ __launch_bounds__(256) void e_change_D_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double v[6], w[6];
#pragma unroll
  for (int j = 0; j < 6; j++) v[j] = r.D[(size_t)j * N + i];
#pragma unroll
  for (int a = 0; a < 6; a++) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 6; q++) t += o.ru[q * 6 + a] * v[q];
    w[a] = t;
  }
#pragma unroll
  for (int j = 0; j < 6; j++) r.D[(size_t)j * N + i] = w[j];
}

__global__ __launch_bounds__(256) void e_init_D_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  init_D_elem(r.D, N, i, BDF_D_ROWS, o.i0 ? r.ytmp[i] : r.y[i], r.f0[i] * o.d0);
}

// norms for the initial step size (bdf_norms_kernel), one 1024-thread workgroup per entry
__global__ __launch_bounds__(1024) void e_norms_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  norms_body(N, r.y, r.f0, o.i0 != 0 ? r.f1 : nullptr, o.d0, o.d1, r.ctrl);
}

// mass-action rates of the entry's state: SRC 0: y, 1: ytmp when i0 != 0 (right-hand sides), 2: y with the corrector's skip flag
template <int SRC>
__global__ __launch_bounds__(256) void e_rates_kernel(int R, const int32_t* __restrict__ x0, const int32_t* __restrict__ x1,
                                                      const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  const int32_t a = x0[q], b = x1[q];
  const double kr = r.k[q];
  if (SRC == 2 && r.ctrl->newton_done) return;
  r.rate[q] = mass_action_rate(kr, (SRC == 1 && o.i0 != 0) ? r.ytmp : r.y, a, b);
}

__global__ __launch_bounds__(256) void e_drates_kernel(int R, const int32_t* __restrict__ x0, const int32_t* __restrict__ x1,
                                                       const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  reinterpret_cast<double2*>(r.dr)[q] = mass_action_drates(r.k[q], r.y, x0[q], x1[q]);
}

__global__ __launch_bounds__(256) void e_apply_rates_kernel(int R, int has_kmax,
                                                            double k_max, double t_mult, const EnsRep* __restrict__ reps,
                                                            const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  if (o.i0 == 1) r.k[q] = o.out[q];
  else r.k[q] = arrhenius_one(r.Ea[q], r.A[q], 8.314462618 * o.d0, has_kmax, k_max, t_mult);
}

// segmented gather-sum of the entry (kernels.hip: segsum_kernel). SEL 0: rates -> f0 / f1 (i0 == 1: f1); 1: operand
// derivatives -> Jacobian values; 2: Newton residual rates -> W (psi, d, c of the entry; corrector's skip flag); 3: a stage
// of the solve, W -> W (skip flag)
template <int OP, int SEG_WG, int SEL>
__global__ __launch_bounds__(SEG_WG) void e_segsum_kernel(SegPlanView p, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const double* src; double* out;
  SegExtra ex;
  if (SEL == 0) { src = r.rate; out = o.i0 == 1 ? r.f1 : r.f0; }
  else if (SEL == 1) { src = r.dr; out = r.jv; }
  else if (SEL == 2) { src = r.rate; out = o.W; ex.psi = r.psi; ex.d = r.d; ex.cscal = o.in.c; }
  else { src = o.W; out = o.W; }
  seg_traverse<OP, SEG_WG>(p, src, out, ex, SEL >= 2 ? &r.ctrl->newton_done : nullptr);
}

template <int OP, int SEL>
static void launch_e_segsum(const SegPlanView& p, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  const int tasks = p.G + p.S;
  if (tasks + p.B == 0 || n == 0) return;
  if (segsum_wg(p) == 1024) hipLaunchKernelGGL((e_segsum_kernel<OP, 1024, SEL>), dim3((unsigned)(p.B + ceil_div(tasks, 16)), (unsigned)n), dim3(1024), 0, s, p, reps, d_ops);
  else hipLaunchKernelGGL((e_segsum_kernel<OP, 256, SEL>), dim3((unsigned)ceil_div(tasks, 4), (unsigned)n), dim3(256), 0, s, p, reps, d_ops);
  KIN_HIP(hipGetLastError());
}

// x2 = S^-1 y2 of the entry: one wavefront per row (gemv_kernel)
__global__ __launch_bounds__(256) void e_gemv_kernel(int ld, int m, long long off_y2, long long off_x, const EnsRep* __restrict__ reps,
                                                     const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int sk = r.ctrl->newton_done;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  gemv_row(o.sinv + (size_t)row * ld, o.W + off_y2, m, sk, o.W + off_x + row);
}

// predictor of the entry (bdf_predict_kernel): clears the attempt's control block
__global__ __launch_bounds__(256) void e_predict_kernel(int N, BdfCoef cf, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  // i0 == 1: a predictor on its own (the state a Jacobian is refreshed at): no iterations
  if (i == 0) open_attempt(r.ctrl, o.i0 == 1 ? 1 : 0);
  if (i >= N) return;
  predict_elem(r.D, N, i, o.in.order, cf.gamma, PredictOut{r.y, r.psi, r.d, r.scale, o.in.alpha_o, o.in.atol, o.in.rtol});
}

// update + decision of one corrector iteration of the entry (bdf_newton_kernel; no publication to the host: the round ends
// with a stream synchronisation and the control blocks are copied then)
__global__ __launch_bounds__(256) void e_newton_kernel(int N, int iter, const int32_t* __restrict__ xloc, BdfCoef cf,
                                                       const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const ResCorrIn& in = o.in;
  const int decided = r.ctrl->newton_done;      // tested when the first round of loads is back (newton_rows)
  const NewtonOps f{N, in.order, r.scale, r.y, r.d, r.D, in.atol, in.rtol, in.ec, in.ec_m, in.ec_p};
  newton_rows(f, xloc, o.W, in.upd, decided, r.part,
              NewtonDecide{N, iter, BDF_NEWTON_MAXITER, in.newton_tol, in.rate_max, in.crate0, in.tol_first, in.dy_first_max, 0, 0, r.ctrl,
                           nullptr, nullptr, nullptr, 0ull, 0});
}

#undef ENS_ENTRY

#define ENS_GRID(n_el, n) dim3((unsigned)ceil_div((n_el), 256), (unsigned)(n)), dim3(256)
void ens_vec(int N, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_vec_kernel, ENS_GRID(N, n), 0, s, N, reps, d_ops);
}
void ens_accept(int N, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_accept_kernel, ENS_GRID(N, n), 0, s, N, reps, d_ops);
}
void ens_change_D(int N, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_change_D_kernel, ENS_GRID(N, n), 0, s, N, reps, d_ops);
}
void ens_init_D(int N, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_init_D_kernel, ENS_GRID(N, n), 0, s, N, reps, d_ops);
}
void ens_norms(int N, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_norms_kernel, dim3(1, (unsigned)n), dim3(1024), 0, s, N, reps, d_ops);
}
void ens_rhs(int N, int R, const int32_t* x0, const int32_t* x1, const SegPlanView& rhs_plan, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n <= 0) return;
  (void)N;
  hipLaunchKernelGGL((e_rates_kernel<1>), ENS_GRID(R, n), 0, s, R, x0, x1, reps, d_ops);
  launch_e_segsum<SEG_COEF_SET, 0>(rhs_plan, reps, d_ops, n, s);
}
void ens_jac(int R, const int32_t* x0, const int32_t* x1, const SegPlanView& jac_plan, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(e_drates_kernel, ENS_GRID(R, n), 0, s, R, x0, x1, reps, d_ops);
  launch_e_segsum<SEG_COEF_SET, 1>(jac_plan, reps, d_ops, n, s);
}
void ens_apply_rates(int R, int has_kmax, double k_max, double t_mult, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_apply_rates_kernel, ENS_GRID(R, n), 0, s, R, has_kmax, k_max, t_mult, reps, d_ops);
}
void ens_predict(const EnsSolveTables& T, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_predict_kernel, ENS_GRID(T.N, n), 0, s, T.N, T.cf, reps, d_ops);
}
void ens_newton(int N, int iter, const int32_t* xloc, const BdfCoef& cf, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_newton_kernel, dim3((unsigned)bdf_reduce_blocks(N), (unsigned)n), dim3(256), 0, s, N, iter, xloc, cf, reps, d_ops);
}
void ens_resid(int R, const int32_t* x0, const int32_t* x1, const SegPlanView& resid, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((e_rates_kernel<2>), ENS_GRID(R, n), 0, s, R, x0, x1, reps, d_ops);
  launch_e_segsum<SEG_COEF_BDF, 2>(resid, reps, d_ops, n, s);
}
void ens_iterations(const EnsSolveTables& T, const EnsRep* reps, const EnsOp* d_ops, int n, int it0, int iters, hipStream_t s) {
  if (n <= 0) return;
  for (int it = it0; it < it0 + iters; it++) {
    ens_resid(T.R, T.x0, T.x1, T.resid, reps, d_ops, n, s);
    launch_e_segsum<SEG_PROD_AUXSUB, 3>(T.stageA, reps, d_ops, n, s);
    hipLaunchKernelGGL(e_gemv_kernel, dim3((unsigned)ceil_div(T.m, 4), (unsigned)n), dim3(256), 0, s, T.mpad, T.m, (long long)(T.off_y + T.ns),
                       (long long)T.off_x, reps, d_ops);
    launch_e_segsum<SEG_PROD_SET, 3>(T.stageC, reps, d_ops, n, s);
    ens_newton(T.N, it, T.xloc, T.cf, reps, d_ops, n, s);
  }
  KIN_HIP(hipGetLastError());
}
int ens_reduce_doubles(int N) { return RED_SLOT * bdf_reduce_blocks(N); }
#undef ENS_GRID

// End of a round without a stream synchronisation: the members' control blocks go to coherent pinned host memory and a
// sequence number the host spins on follows them (the hand-over of the host-driven integrator, bdf_newton_kernel)
__global__ __launch_bounds__(256) void e_publish_kernel(const BdfCtrl* __restrict__ ctrl, BdfCtrl* host_ctrl, int n_words,
                                                        unsigned long long* host_seq, unsigned long long seq) {
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(ctrl);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(host_ctrl);
  for (int i = threadIdx.x; i < n_words; i += 256) dst[i] = src[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) { __threadfence_system(); *(volatile unsigned long long*)host_seq = seq; }
}
void ens_publish(const BdfCtrl* ctrl, BdfCtrl* host_ctrl, int K, unsigned long long* host_seq, unsigned long long seq, hipStream_t s) {
  static_assert(sizeof(BdfCtrl) % 8 == 0, "BdfCtrl is copied in 8-byte words");
  hipLaunchKernelGGL(e_publish_kernel, dim3(1), dim3(256), 0, s, ctrl, host_ctrl, (int)(K * sizeof(BdfCtrl) / 8), host_seq, seq);
}
