// Resident integrator: device-visible tables and the launcher (resident.hip), host-side owner (resident.cpp).
// One 512-thread workgroup (8 wavefronts, 256 VGPRs each) integrates one trajectory from u0 to the end of the time span - chunk loop, rate updates,
// retries, BDF steps, Jacobians, factorisations and corrector iterations - without leaving the GPU (resident_core.hpp).
#pragma once
#include "kernels.hpp"
#include "resident_core.hpp"

namespace kin {

constexpr int RES_MAX_ROUNDS = 32;

// solve modes of the factorised Newton matrix (lu.hpp)
enum : int { RES_SOLVE_FUSED = 0, RES_SOLVE_EXPLICIT = 1, RES_SOLVE_PLAIN = 2 };

// immutable per network: reaction tables, gather plans, symbolic LU (device pointers)
struct ResNetDev {
  int32_t N, R, nnzJ, ns, m, mpad, nrounds, n_mono_ent, solve_mode, has_kmax;
  int32_t desc_in_lds, pad0_;      // the launch provisions LDS for the task descriptors of resid_plan / stageA / stageC
  int64_t off_diag, off_U, off_L, off_S, off_y, off_x, off_dinv, off_vec_end, w_size;
  double k_max, t_mult;
  const int32_t *x0, *x1, *jmap, *ent_pivot, *yloc, *xloc, *j_diag;
  const int32_t *mono_ent_ptr, *mono_ptr, *mono_fac, *mono_dst;
  const float* mono_sign;
  const double *Ea, *A;            // the handle's Arrhenius parameters (the kernel reads each member's ResTrajDev::Ea / A)
  const double* k_table;           // rate_mode 1 (rate_mode 2 reads each member's ResTrajDev::T_stops)
  int32_t round_e0[RES_MAX_ROUNDS + 1];   // first L entry of every elimination round
  SegPlanView rhs_plan, jac_plan, resid_plan, lz_build, nvu_build, stageA, stageC, fwdZ, fwd_dense, bwdT, bwdV;
  SegPlanView schur[RES_MAX_ROUNDS], fwd[RES_MAX_ROUNDS], bwd[RES_MAX_ROUNDS];
};

// per trajectory: inputs, work vectors, LU-cache slots, outputs
struct ResTrajDev {
  const double* u0;
  double *k, *D, *y, *psi, *d, *scale, *f0, *f1, *ytmp, *chunk_start, *jv, *rate, *dr;
  double* gj_scratch;   // mpad x mpad: second block of the dense inverse's ping-pong
  double* W;       // n_slots value arrays of w_size doubles
  double* jd;      // n_slots copies of diag(J) (drift guard of the LU cache)
  double *sol, *sol_t;
  ResResult* result;
  const double *t_nodes, *T_nodes;   // rate_mode 3: this member's temperature profile (ResParams::t_nodes ...)
  int64_t n_nodes;
  const double *tstops, *T_stops;    // rate_mode 1 / 2: this member's stops (ResParams::tstops, n_stops); T_stops: rate_mode 2
  int64_t n_stops;
  // rate_mode 2 / 3: this member's Arrhenius parameters - its rows of a per-member call's blocks, else the handle's arrays
  // (run_resident sets them for every member; appended, so code that fills the fields above stays as it is, and without
  // initialisers: the kernel keeps a copy of this struct in LDS, which takes no constructor)
  const double *Ea, *A;
};

// enqueues the solve of K trajectories (grid = K workgroups of RES_WG = 512 threads)
// `m`: dimension of the dense Schur block (sizes the dynamic LDS of its row panel; at most RES_MAX_DENSE)
constexpr int RES_MAX_DENSE = 512;
// dynamic LDS of the kernel: y, d, psi, scale (4 N), the solve-vector window of W, max(R, row panel of the dense inverse)
size_t resident_dyn_lds(int N, int R, int m, int64_t window);
size_t resident_desc_bytes(const SegPlanView& resid, const SegPlanView& stageA, const SegPlanView& stageC);   // ... + these, when they fit
constexpr size_t RES_LDS_BUDGET = 160 * 1024 - 16 * 1024;   // what is left of a CU's LDS next to the kernel's static blocks
void launch_resident(int K, size_t dyn_lds, const ResNetDev* d_net, const ResTrajDev* d_traj, const ResParams* d_par, hipStream_t s);
// the same kernel built with half the registers per lane: two workgroups share a compute unit (resident_w4.hip)
void launch_resident_shared_cu(int K, size_t dyn_lds, const ResNetDev* d_net, const ResTrajDev* d_traj, const ResParams* d_par, hipStream_t s);
size_t resident_static_lds();    // static LDS of the kernel (what two co-resident workgroups need twice, next to 2 x dyn_lds)
// diagnostic (resident_probe.hip: resident.hip built with RES_LINALG_PROBE): the phases of one Newton-matrix solve per member -
// f(u) into T.f0, J(u) into T.jv, M = I - c[m] J(u) into slot 0 of T.W, x[m] = M^-1 b[m], bad[m] = the vanished-pivot flag (mode
// RES_PROBE_NEWTON, the zero-initialised default).
// The cache modes (kin_cache_probe, path 1; one workgroup): RES_PROBE_DRIFT - n_slots slots made from jv_slots[n_slots][nnz] at
// c_fact[n_slots] (ph_factor with keep_diag), flags valid[n_slots], then DevBackend::drift_check(max_drift) against jv_now[nnz]:
// drift[n_slots] = g_sh.drift, out_i[n_slots] = the slot table's valid flags afterwards, out_i[RES_MAX_SLOTS] = its return value;
// RES_PROBE_RULES - the slot table valid / c_fact / stamps[3][n_slots] (jac_stamp, step_stamp, last_use), n_queries queries
// qd[q][2] = c, band, qi[q][5] = n_restarts, max_age, n_steps, step_age, slot count: out_i[q][2] = nearest_slot, victim_slot.
// The step mode (kin_step_probe, paths 3 and 4; one workgroup per member): RES_PROBE_STEP - ONE operation of the step on the member's
// block state[RES_STEP_ROWS][N] of the caller (kinetica_hip.h: rows 0-7 are T.D, 12-15 T.f0 / f1 / ytmp / chunk_start, 24-25 the two
// rows of T.sol, 26 T.u0 - the host points the member's ResTrajDev there; rows 8-11 are loaded into the LDS arrays y / psi / d /
// scale before the operation and stored back after it), run the way resident_bdf_kernel runs it: wavefronts 1-7 in worker_loop,
// wavefront 0 with a controller in g_ctl_mem calling the controller's or the backend's method. Results that are scalars go to the
// member's ctrl[RES_STEP_CTRL] (the fields of BdfCtrl as doubles); what an operation does not return stays as uploaded.
enum : int { RES_PROBE_NEWTON = 0, RES_PROBE_DRIFT = 1, RES_PROBE_RULES = 2, RES_PROBE_STEP = 3 };
constexpr int RES_STEP_ROWS = 28, RES_STEP_CTRL = 18, RES_STEP_ROW_Y = 8, RES_STEP_ROW_X = 23;
enum : int { RES_STEP_VEC = 0, RES_STEP_SAVE_Y, RES_STEP_SET_TIME, RES_STEP_NORMS, RES_STEP_INIT_D, RES_STEP_PREDICT, RES_STEP_ACCEPT,
             RES_STEP_CHANGE_D, RES_STEP_INTERP, RES_STEP_NEWTON, RES_STEP_CORRECTOR, RES_STEP_OP_COUNT };
// one member's arguments: aux = the VecOp / with_f1 / from_ytmp; row = the solution row; h = VEC's h0, INIT_D's h, CHANGE_D's factor;
// t, h_abs, ts: INTERP (t also the time of SAVE_Y / SET_TIME); c_fact: what slot 0 is factorised at (NEWTON, CORRECTOR: `in`)
struct ResStepArg { int32_t order, aux, row, pad; double atol, rtol, h, t, h_abs, ts, c_fact; ResCorrIn in; };
struct ResProbeIO {
  const double *c, *b; double* x; int32_t* bad;
  int32_t mode, n_slots, n_queries;
  const double *jv_slots, *jv_now, *c_fact; const int32_t* valid; double max_drift;
  const long long* stamps; const double* qd; const long long* qi;
  double* drift; int32_t* out_i;
  int32_t step_op, pad_; const ResStepArg* step_arg; double *state, *ctrl;   // RES_PROBE_STEP
};
void launch_resident_probe(int K, size_t dyn_lds, const ResNetDev* d_net, const ResTrajDev* d_traj, const ResParams* d_par, const ResProbeIO& io,
                           hipStream_t s);
// the same probe kernel in the shared-CU build (resident_probe_w4.hip: 128 VGPRs, phases inlined, as resident_w4.hip)
void launch_resident_probe_shared_cu(int K, size_t dyn_lds, const ResNetDev* d_net, const ResTrajDev* d_traj, const ResParams* d_par,
                                     const ResProbeIO& io, hipStream_t s);

}  // namespace kin
