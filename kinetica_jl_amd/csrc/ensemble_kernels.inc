// Batched kernels of the large-network ensemble (ensemble.hpp): the single-trajectory kernels of this file and of kernels.hip
// with a second grid dimension - blockIdx.y = entry of the round's list (EnsOp), which names the member (EnsRep) and
// carries what the single-trajectory launch takes as kernel arguments. Included at the end of solver_kernels.hip (inside
// namespace kin): the reduction hand-over, the corrector's decision and the gather pieces are the ones defined above.

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
    case EV_INTERP: {
      double v = r.D[i];
      for (int j = 1; j <= o.i1; j++) v += o.p[j] * r.D[(size_t)j * N + i];
      o.out[i] = v;
    } break;
    default: break;
  }
}

__global__ __launch_bounds__(256) void e_accept_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int order = o.i0;
  double* D = r.D;
  const double di = r.d[i];
  D[(size_t)(order + 2) * N + i] = di - D[(size_t)(order + 1) * N + i];
  D[(size_t)(order + 1) * N + i] = di;
  double carry = di;
  for (int j = order; j >= 0; j--) {
    carry += D[(size_t)j * N + i];
    D[(size_t)j * N + i] = carry;
  }
}

// D[0..5] <- M^T D[0..5] with the 6 x 6 matrix of the entry (identity outside the orders involved)
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
  r.D[i] = o.i0 ? r.ytmp[i] : r.y[i];
  r.D[(size_t)N + i] = r.f0[i] * o.d0;
  for (int j = 2; j < BDF_D_ROWS; j++) r.D[(size_t)j * N + i] = 0.0;
}

// norms for the initial step size (bdf_norms_kernel), one 1024-thread workgroup per entry
__global__ __launch_bounds__(1024) void e_norms_kernel(int N, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  __shared__ double sh[17];
  ENS_ENTRY;
  const bool with_f1 = o.i0 != 0;
  const double atol = o.d0, rtol = o.d1;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, vm = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const double y0 = r.y[i], f0 = r.f0[i];
    const double sc = atol + rtol * fabs(y0);
    const double a = y0 / sc, b = f0 / sc;
    s0 += a * a; s1 += b * b;
    vm = fmax(vm, fabs(f0) / (0.1 * fabs(y0) + sc));
    if (!isfinite(f0)) bad = 1;
    if (with_f1) { const double f1 = r.f1[i]; const double c = (f1 - f0) / sc; s2 += c * c; if (!isfinite(f1)) bad = 1; }
  }
  const double t0 = block_sum_1024(s0, sh), t1 = block_sum_1024(s1, sh), t2 = block_sum_1024(s2, sh);
  const double tb = block_sum_1024((double)bad, sh);
  const double tm = block_max_1024(vm, sh);
  if (threadIdx.x == 0) {
    r.ctrl->scratch[0] = sqrt(t0 / (double)N);
    r.ctrl->scratch[1] = sqrt(t1 / (double)N);
    r.ctrl->scratch[2] = sqrt(t2 / (double)N);
    r.ctrl->scratch[3] = tm;
    r.ctrl->nonfinite = tb > 0.0;
  }
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
  const double* u = (SRC == 1 && o.i0 != 0) ? r.ytmp : r.y;
  const double ub = b >= 0 ? u[b] : 1.0;
  r.rate[q] = kr * u[a] * ub;
}

__global__ __launch_bounds__(256) void e_drates_kernel(int R, const int32_t* __restrict__ x0, const int32_t* __restrict__ x1,
                                                       const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  const int32_t a = x0[q], b = x1[q];
  const double kk = r.k[q];
  const double* u = r.y;
  double d0, d1 = 0.0;
  if (b < 0) d0 = kk;
  else if (b == a) d0 = 2.0 * kk * u[a];
  else { d0 = kk * u[b]; d1 = kk * u[a]; }
  reinterpret_cast<double2*>(r.dr)[q] = make_double2(d0, d1);
}

__global__ __launch_bounds__(256) void e_apply_rates_kernel(int R, const double* __restrict__ Ea, const double* __restrict__ A, int has_kmax,
                                                            double k_max, double t_mult, const EnsRep* __restrict__ reps,
                                                            const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= R) return;
  if (o.i0 == 1) r.k[q] = o.out[q];
  else r.k[q] = arrhenius_one(Ea[q], A[q], 8.314462618 * o.d0, has_kmax, k_max, t_mult);
}

// segmented gather-sum of the entry (kernels.hip: segsum_kernel). SEL 0: rates -> f0 / f1 (i0 == 1: f1); 1: operand
// derivatives -> Jacobian values; 2: Newton residual rates -> W (psi, d, c of the entry; corrector's skip flag); 3: a stage
// of the solve, W -> W (skip flag)
template <int OP, int SEG_WG, int SEL>
__global__ __launch_bounds__(SEG_WG) void e_segsum_kernel(SegPlanView p, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  constexpr int SEG_WAVES = SEG_WG / 64, BLK_PER_THREAD = SegPlanHost::BLK_PASS / 1024;
  ENS_ENTRY;
  const double* src; double* out;
  SegExtra ex;
  if (SEL == 0) { src = r.rate; out = o.i0 == 1 ? r.f1 : r.f0; }
  else if (SEL == 1) { src = r.dr; out = r.jv; }
  else if (SEL == 2) { src = r.rate; out = o.W; ex.psi = r.psi; ex.d = r.d; ex.cscal = o.in.c; }
  else { src = o.W; out = o.W; }
  const int skip = (SEL >= 2) ? r.ctrl->newton_done : 0;
  const int lane = threadIdx.x & 63;
  const bool impl = p.val_base >= 0;
  if (SEG_WG == 1024 && (int)blockIdx.x < p.B) {
    __shared__ double sh[SEG_WAVES];
    const int rr = blockIdx.x;
    const int32_t e0 = p.blk_beg[rr], e1 = p.blk_end[rr];
    const int32_t bdst = p.blk_dst[rr], baux = p.blk_aux[rr];
    if (skip) return;
    const SegPre pre = seg_pre<OP>(out, src, threadIdx.x == 0 ? bdst : -1, baux, ex);
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
      for (int w = 0; w < SEG_WAVES; w++) tot += sh[w];
      seg_store<OP>(out, bdst, tot, pre, ex);
    }
    return;
  }
  const int task = ((int)blockIdx.x - p.B) * SEG_WAVES + (threadIdx.x >> 6);
  if (task < p.G) {
    const int32_t dst = p.grp_dst[task * 64 + lane], aux = p.grp_aux[task * 64 + lane];
    const int32_t c0 = p.grp_off[task], c1 = p.grp_off[task + 1];
    if (skip) return;
    const SegPre pre = seg_pre<OP>(out, src, dst, aux, ex);
    double acc = 0.0;
    for (int32_t col = c0; col < c1; col += 8)
      acc += seg_gather<OP, 8, true>(p, src, ex, impl, [&](int x) { return col + x < c1 ? (col + x) * 64 + lane : -1; });
    if (dst >= 0) seg_store<OP>(out, dst, acc, pre, ex);
  } else if (task < p.G + p.S) {
    const int sidx = task - p.G;
    const int32_t e0 = p.seg_beg[sidx], e1 = p.seg_end[sidx];
    const int32_t sdst = p.seg_dst[sidx], saux = p.seg_aux[sidx];
    if (skip) return;
    const SegPre pre = seg_pre<OP>(out, src, lane == 0 ? sdst : -1, saux, ex);
    double acc = seg_gather<OP, 4, false>(p, src, ex, impl, [&](int x) { const int32_t e = e0 + lane + 64 * x; return e < e1 ? e : -1; });
    acc = wave_sum(acc);
    if (lane == 0) seg_store<OP>(out, sdst, acc, pre, ex);
  }
}

template <int OP, int SEL>
static void launch_e_segsum(const SegPlanView& p, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  const int tasks = p.G + p.S;
  if (tasks + p.B == 0 || n == 0) return;
  if (p.B > 0) hipLaunchKernelGGL((e_segsum_kernel<OP, 1024, SEL>), dim3((unsigned)(p.B + ceil_div(tasks, 16)), (unsigned)n), dim3(1024), 0, s, p, reps, d_ops);
  else hipLaunchKernelGGL((e_segsum_kernel<OP, 256, SEL>), dim3((unsigned)ceil_div(tasks, 4), (unsigned)n), dim3(256), 0, s, p, reps, d_ops);
  KIN_HIP(hipGetLastError());
}

// x2 = S^-1 y2 of the entry: one wavefront per row (gemv_kernel)
__global__ __launch_bounds__(256) void e_gemv_kernel(int ld, int m, long long off_y2, long long off_x, const EnsRep* __restrict__ reps,
                                                     const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  if (r.ctrl->newton_done) return;
  const double* a = o.sinv + (size_t)row * ld;
  const double* y = o.W + off_y2;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  int j = lane;
  for (; j + 192 < m; j += 256) {
    const double a0 = a[j], a1 = a[j + 64], a2 = a[j + 128], a3 = a[j + 192];
    const double y0 = y[j], y1 = y[j + 64], y2 = y[j + 128], y3 = y[j + 192];
    acc0 += a0 * y0; acc1 += a1 * y1; acc2 += a2 * y2; acc3 += a3 * y3;
  }
  for (; j < m; j += 64) acc0 += a[j] * y[j];
  double acc = (acc0 + acc1) + (acc2 + acc3);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) o.W[off_x + row] = acc;
}

// predictor of the entry (bdf_predict_kernel): clears the attempt's control block
__global__ __launch_bounds__(256) void e_predict_kernel(int N, BdfCoef cf, const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  ENS_ENTRY;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int order = o.in.order;
  BdfCtrl* ctrl = r.ctrl;
  if (i == 0) {
    ctrl->newton_done = o.i0 == 1 ? 1 : 0;   // i0 == 1: a predictor on its own (the state a Jacobian is refreshed at): no iterations
    ctrl->converged = 0; ctrl->n_iter = 0; ctrl->nonfinite = 0; ctrl->any_negative = 0; ctrl->ticket = 0;
    ctrl->dy_norm_old = 0.0; ctrl->dy_norm = 0.0; ctrl->err_norm = 0.0; ctrl->err_m_norm = 0.0; ctrl->err_p_norm = 0.0;
  }
  if (i >= N) return;
  double yp = r.D[i], ps = 0.0;
  for (int j = 1; j <= order; j++) {
    const double dj = r.D[(size_t)j * N + i];
    yp += dj;
    ps += dj * cf.gamma[j];
  }
  r.y[i] = yp;
  r.psi[i] = ps / o.in.alpha_o;
  r.d[i] = 0.0;
  r.scale[i] = o.in.atol + o.in.rtol * fabs(yp);
}

// update + decision of one corrector iteration of the entry (bdf_newton_kernel; no publication to the host: the round ends
// with a stream synchronisation and the control blocks are copied then)
__global__ __launch_bounds__(256) void e_newton_kernel(int N, int iter, const int32_t* __restrict__ xloc, BdfCoef cf,
                                                       const EnsRep* __restrict__ reps, const EnsOp* __restrict__ ops) {
  __shared__ double sh[20];
  __shared__ int last;
  ENS_ENTRY;
  BdfCtrl* ctrl = r.ctrl;
  if (ctrl->newton_done) return;
  const ResCorrIn& in = o.in;
  const int order = in.order;
  const int G = gridDim.x;
  const double* W = o.W;
  double s = 0.0, se = 0.0, sm = 0.0, sp = 0.0, neg = 0.0;
  const int i0 = blockIdx.x * RED_ELEMS + threadIdx.x;
  int32_t xl[RED_PT]; double dy[RED_PT], sc[RED_PT], yy[RED_PT], dd[RED_PT], dm[RED_PT], dp[RED_PT];
#pragma unroll
  for (int x = 0; x < RED_PT; x++) {
    const int i = i0 + 256 * x;
    const bool ok = i < N;
    xl[x] = ok ? xloc[i] : -1; sc[x] = ok ? r.scale[i] : 1.0;
    yy[x] = ok ? r.y[i] : 0.0; dd[x] = ok ? r.d[i] : 0.0;
    dm[x] = (ok && order > 1) ? r.D[(size_t)order * N + i] : 0.0;
    dp[x] = (ok && order < 5) ? r.D[(size_t)(order + 1) * N + i] : 0.0;
  }
#pragma unroll
  for (int x = 0; x < RED_PT; x++) dy[x] = xl[x] >= 0 ? in.upd * W[xl[x]] : 0.0;
#pragma unroll
  for (int x = 0; x < RED_PT; x++) {
    const double q = dy[x] / sc[x];
    s += q * q;
    yy[x] += dy[x]; dd[x] += dy[x];
    if (i0 + 256 * x >= N) continue;
    const double sce = in.atol + in.rtol * fabs(yy[x]);
    if (yy[x] < 0.0) neg = fmax(neg, yy[x] < -BDF_NEG_DEEP * sce ? BDF_NEG_MARK : 1.0);
    const double e = in.ec * dd[x] / sce;
    se += e * e + (isfinite(yy[x]) ? 0.0 : INFINITY);
    if (order > 1) { const double em = in.ec_m * (dm[x] + dd[x]) / sce; sm += em * em; }
    if (order < 5) { const double ep = in.ec_p * (dd[x] - dp[x]) / sce; sp += ep * ep; }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_down(s, off, 64); se += __shfl_down(se, off, 64); sm += __shfl_down(sm, off, 64);
    sp += __shfl_down(sp, off, 64); neg += __shfl_down(neg, off, 64);
  }
  {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[5 * w] = s; sh[5 * w + 1] = se; sh[5 * w + 2] = sm; sh[5 * w + 3] = sp; sh[5 * w + 4] = neg; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 5; q++) store_partial(r.part + blockIdx.x * RED_SLOT + q, (sh[q] + sh[5 + q]) + (sh[10 + q] + sh[15 + q]));
  }
  const bool is_last = last_block_arrives(ctrl, &last);
#pragma unroll
  for (int x = 0; x < RED_PT; x++) {
    const int i = i0 + 256 * x;
    if (i < N) { r.y[i] = yy[x]; r.d[i] = dd[x]; }
  }
  if (!is_last || threadIdx.x >= 64) return;
  double tot[5];
  newton_totals(r.part, G, tot);
  if (threadIdx.x == 0)
    newton_decide(NewtonDecide{N, iter, BDF_NEWTON_MAXITER, in.newton_tol, in.rate_max, in.crate0, in.tol_first, in.dy_first_max, 0, 0, ctrl, tot,
                               nullptr, nullptr, 0ull, 0});
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
void ens_apply_rates(int R, const double* Ea, const double* A, int has_kmax, double k_max, double t_mult, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_apply_rates_kernel, ENS_GRID(R, n), 0, s, R, Ea, A, has_kmax, k_max, t_mult, reps, d_ops);
}
void ens_predict(const EnsSolveTables& T, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_predict_kernel, ENS_GRID(T.N, n), 0, s, T.N, T.cf, reps, d_ops);
}
void ens_newton(int N, int iter, const int32_t* xloc, const BdfCoef& cf, const EnsRep* reps, const EnsOp* d_ops, int n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(e_newton_kernel, dim3((unsigned)bdf_reduce_blocks(N), (unsigned)n), dim3(256), 0, s, N, iter, xloc, cf, reps, d_ops);
}
void ens_iterations(const EnsSolveTables& T, const EnsRep* reps, const EnsOp* d_ops, int n, int it0, int iters, hipStream_t s) {
  if (n <= 0) return;
  for (int it = it0; it < it0 + iters; it++) {
    hipLaunchKernelGGL((e_rates_kernel<2>), ENS_GRID(T.R, n), 0, s, T.R, T.x0, T.x1, reps, d_ops);
    launch_e_segsum<SEG_COEF_BDF, 2>(T.resid, reps, d_ops, n, s);
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
