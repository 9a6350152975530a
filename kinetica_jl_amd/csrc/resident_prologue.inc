// The resident kernels' prologue (all threads): context block, parameters, split counts and the LDS task descriptors of the
// member's trajectory. Included as the first statements of resident_bdf_kernel and of the probe kernel (resident.hip, built as
// resident_probe.hip), so both set up alike. Text, not a function: an inlined call changed the product kernel's register
// allocation (gfx950: scratch 424 -> 440 bytes, VGPR spills 79 -> 83), the included text compiles to the same code as before.
// In scope: net_p, traj, par_p (the kernel's arguments).
  if (threadIdx.x == 0) {
    const ResNetDev& n = *net_p;
    g_par = *par_p;
    g_cx.T = traj[blockIdx.x];
    if (g_par.rate_mode == 3) { g_par.t_nodes = g_cx.T.t_nodes; g_par.T_nodes = g_cx.T.T_nodes; g_par.n_nodes = g_cx.T.n_nodes; }   // this member's profile
    if (g_par.rate_mode == 1 || g_par.rate_mode == 2) { g_par.tstops = g_cx.T.tstops; g_par.n_stops = (int32_t)g_cx.T.n_stops; }   // ... stops
    g_cx.net = net_p;
    g_cx.plan[PL_RHS] = n.rhs_plan; g_cx.plan[PL_JAC] = n.jac_plan; g_cx.plan[PL_RESID] = n.resid_plan;
    g_cx.plan[PL_LZ] = n.lz_build; g_cx.plan[PL_NVU] = n.nvu_build; g_cx.plan[PL_STAGEA] = n.stageA; g_cx.plan[PL_STAGEC] = n.stageC;
    g_cx.plan[PL_FWDZ] = n.fwdZ; g_cx.plan[PL_FWD_DENSE] = n.fwd_dense; g_cx.plan[PL_BWDT] = n.bwdT; g_cx.plan[PL_BWDV] = n.bwdV;
    for (int i = 0; i < PL_COUNT; i++) { g_cx.split[i][0] = 0; g_cx.split[i][1] = 0; }
    g_cx.profile = par_p->profile;
    g_cx.N = n.N; g_cx.R = n.R; g_cx.nnzJ = n.nnzJ; g_cx.ns = n.ns; g_cx.m = n.m; g_cx.m16 = (n.m + 15) / 16 * 16; g_cx.mpad = n.mpad;
    g_cx.nrounds = n.nrounds; g_cx.n_mono_ent = n.n_mono_ent; g_cx.solve_mode = n.solve_mode; g_cx.has_kmax = n.has_kmax;
    g_cx.n_slots = par_p->n_slots; g_cx.rate_mode = par_p->rate_mode;
    g_cx.off_diag = n.off_diag; g_cx.off_U = n.off_U; g_cx.off_L = n.off_L; g_cx.off_S = n.off_S; g_cx.off_y = n.off_y; g_cx.off_x = n.off_x;
    g_cx.off_dinv = n.off_dinv; g_cx.w_size = n.w_size;
    g_cx.k_max = n.k_max; g_cx.t_mult = n.t_mult;
    g_cx.off_vec_end = n.off_vec_end;
    const int win = (int)(n.off_vec_end - n.off_y);
    g_cx.l_y = 0; g_cx.l_d = n.N; g_cx.l_psi = 2 * n.N; g_cx.l_scale = 3 * n.N; g_cx.l_win = 4 * n.N; g_cx.l_rate = 4 * n.N + win;
    // task descriptors of the corrector's three plans behind the vectors (the host provisioned the LDS for them or did not)
    g_cx.desc_on = n.desc_in_lds;
    const int m16_ = (n.m + 15) / 16 * 16;
    const int tail = n.R > 16 * (m16_ + 1) ? n.R : 16 * (m16_ + 1);
    int off = 2 * (4 * n.N + win + tail);       // in int32
    g_cx.desc_off[0] = off; off += desc_ints(n.resid_plan);
    g_cx.desc_off[1] = off; off += desc_ints(n.stageA);
    g_cx.desc_off[2] = off;
  }
  if (threadIdx.x < 20) g_sh.prof[threadIdx.x] = 0;
  __syncthreads();
  for (int id = 0; id < PL_COUNT; id++) count_splits(id);
  __syncthreads();
  if (g_cx.desc_on) { stage_descriptors(0, PL_RESID); stage_descriptors(1, PL_STAGEA); stage_descriptors(2, PL_STAGEC); __syncthreads(); }
