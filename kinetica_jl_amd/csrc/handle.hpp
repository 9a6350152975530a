// The object behind the opaque kin_network handle of include/kinetica_hip.h, and what every extern "C" entry point that
// takes one is written with: require and the KIN_TRY / KIN_CATCH guard.
#pragma once
#include <memory>
#include <string>

#include "common.hpp"
#include "drg.hpp"
#include "kernels.hpp"
#include "network.hpp"
#include "observable_kernels.hpp"
#include "pfa.hpp"
#include "tiled.hpp"

namespace kin {
struct Solver; struct IntegratorState; struct ResidentSolver; struct EnsembleSolver;
struct ResidentDeleter { void operator()(ResidentSolver* p) const; };   // resident.cpp (the type is complete there only)
struct EnsembleDeleter { void operator()(EnsembleSolver* p) const; };   // ensemble.cpp

inline void require(bool c, int code, const char* msg) {
  if (!c) throw KinError(code, msg);
}
}

// The body of an entry point that has checked its handle: it runs on the handle's own device (the one current at
// kin_network_create), whatever the calling thread's current device is - K handles on K host threads can share one GPU or sit
// on different ones - and a KinError becomes its code, with the message left in the handle for kin_last_error.
#define KIN_TRY(h) try { KIN_HIP(hipSetDevice((h)->device));
#define KIN_CATCH(h)                                                        \
  }                                                                         \
  catch (const ::kin::KinError& e) { (h)->err = e.what(); return e.code; }  \
  catch (const std::exception& e) { (h)->err = e.what(); return ::kin::ERR_DEVICE; } \
  return ::kin::OK;

struct kin_network {
  kin::NetworkHost host;
  hipStream_t stream = nullptr;
  std::string err;

  // reaction tables
  kin::DevBuf<int32_t> x0, x1, sp_ptr, sp_rxn;
  kin::DevBuf<uint32_t> sweep_rec;   // 4 words per reversible pair (kernels.hip: SweepRec)
  kin::DevBuf<int32_t> sweep_k;      // (kf, kr) per pair
  kin::DevBuf<uint32_t> sweep_rec64; // 64-bit packed records (register-resident sweep)
  kin::DevBuf<uint32_t> gen_rec8;    // 8-byte fixed-role records of the general LDS sweep (host-padded)
  kin::DevBuf<int32_t> gen_k;        // (kf, kr) per record of that sweep (host-padded)
  kin::DevBuf<int32_t> gen_expl;     // its explicit-operand records (slow path)
  kin::DevBuf<int32_t> sweep_copy;   // species of the split hubs' extra accumulator entries
  kin::DevBuf<uint32_t> big_rec, big_rec8;   // large-N sweep: label-space records (16-byte slow-path and 8-byte stream format)
  kin::DevBuf<int32_t> big_spec, big_tptr, big_expl;
  kin::DevBuf<uint32_t> big_tent;    // (record, local label | coef << 24) pairs per tail tile
  kin::DevBuf<double> big_scratch;   // per-workgroup rows (tail u + net rates) of the large-N sweep (grown on demand)
  kin::DevBuf<float> sp_coef;
  kin::SegPlanDev rhs_plan, jac_plan;

  // rate constants / calculator
  kin::DevBuf<double> k, Ea, A, table, T_stops;
  bool has_rates = false, has_arrhenius = false, has_kmax = false;
  // Continuous-rate solves: a temperature whose rate constants have not been formed yet. The first kernel that reads k
  // (rates / operand derivatives / the corrector's rates) evaluates the Arrhenius law itself and stores k for the readers
  // behind it: no launch of its own per step attempt (the reference inlines k(T(t)) into the ODEs, methods.jl:389-419).
  bool k_pending = false;
  double T_pending = 0.0;
  void set_pending_T(double T) { T_pending = T; k_pending = true; has_rates = true; }
  kin::ArrheniusAt pending_at() const { return kin::ArrheniusAt{Ea.p, A.p, has_kmax ? 1 : 0, k_max, t_mult, T_pending}; }
  void flush_pending_T(hipStream_t s);   // forms k now if a temperature is still pending
  double k_max = 0.0, t_mult = 1.0;
  int64_t table_rows = 0;

  // single-state work vectors
  kin::DevBuf<double> u, du, rate, dr, jvals;

  // batched sweep workspace
  kin::DevBuf<double> b_u, b_k, b_du;

  // reaction-flux pass (flux_kernels.hpp, flux_api.cpp): index tables uploaded at the first call that needs them, the
  // partial sums part[G][R] and the staging buffers of the host entries grown on demand. The host entries of every analysis
  // pass stage through the same ones (flux_api.hpp): states f_u, rate-constant keys f_k / f_krow / f_T, a species list f_sel
  // and an accumulating result f_result
  bool flux_ready = false;
  kin::DevBuf<uint32_t> flux_idx16;
  kin::DevBuf<int32_t> flux_idx32;
  kin::DevBuf<double> flux_part, f_u, f_k, f_T, f_w, f_flux, f_rates, f_result;
  kin::DevBuf<int64_t> f_krow, f_segn, f_sel;

  // directed-relation-graph pass (drg.hpp, drg_api.cpp): host tables and device plans per pairing mode, built at the first
  // call that needs them; the block of per-state rates (stage 1), its denominators and the maxima per slice, grown on demand
  struct DrgMode {
    std::unique_ptr<kin::DrgTables> host;
    bool dev_ready = false;
    kin::SegPlanDev den_plan, edge_plan;
    kin::DevBuf<float> den_ell_c, den_long_c, edge_ell_c, edge_long_c;
    // DRGEP (drgep_api.cpp): the signed coefficients and the transposed pattern, uploaded at the first DRGEP call
    bool ep_ready = false;
    kin::DevBuf<float> den_ell_s, den_long_s, edge_ell_s, edge_long_s;
    kin::DevBuf<int32_t> in_ptr, in_src, in_edge, in_order;
  } drg[2];
  kin::DevBuf<double> drg_rates, drg_den, drg_part;
  // DRGEP: the block's coefficients r[nb][E], importances R[nb][N], the global form's work[nb][2][N], rounds[nb]
  kin::DevBuf<double> drgep_r, drgep_R, drgep_work;
  kin::DevBuf<int32_t> drgep_rounds;
  // reaction importance (drg.hpp, drg_api.cpp): the per-reaction table per pairing mode and, where the DRG pass has not
  // uploaded its plans yet, a denominator plan of its own (no edge plan is built for this pass); the species mask, the maxima
  // per slice and the block's per-state values when asked for
  struct RiMode {
    std::unique_ptr<kin::RiTables> host;
    std::unique_ptr<kin::DrgTables> den_host;
    bool dev_ready = false;
    kin::DevBuf<int32_t> tab;
    kin::SegPlanDev den_plan;
    kin::DevBuf<float> den_ell_c, den_long_c;
  } ri[2];
  kin::DevBuf<uint8_t> ri_mask;
  kin::DevBuf<double> ri_part, ri_state;

  // path flux analysis (pfa.hpp, pfa_api.cpp): the second-generation pattern per pairing mode and, on the device, both
  // patterns and the order of the rows; the block's rp[nb][E], rc[nb][E], the per-state r[nb][E2] when asked for and the
  // maxima per slice
  struct PfaMode {
    std::unique_ptr<kin::PfaTables> host;
    bool dev_ready = false;
    kin::DevBuf<int32_t> rowptr, colidx, rowptr2, colidx2, order;
  } pfa[2];
  kin::DevBuf<double> pfa_rp, pfa_rc, pfa_r, pfa_part;

  // timescale pass (timescale.hpp, timescale_api.cpp): the row pass's tables, uploaded at the first call that needs them; the
  // block's rates[nb][R], dr[nb][2R], jv[nb][nnz], g[nb][N], the extrema per slice part[Y][3][N] and the staging buffers of
  // the host entries' per-state outputs, grown on demand
  bool ts_ready = false;
  int32_t ts_G = 0, ts_S = 0, ts_Bl = 0;
  kin::DevBuf<int32_t> ts_rows;
  kin::DevBuf<double> ts_rates, ts_dr, ts_jv, ts_g, ts_part, ts_o_vals, ts_o_diag, ts_o_err, ts_o_norm;

  // tiled sweep in library order (tiled.hpp, tiled_api.cpp): built at the first call that needs it
  kin::TiledHost tiled;
  bool tiled_tried = false;
  kin::DevBuf<uint32_t> t_rec;
  kin::DevBuf<int32_t> t_copy, t_kf, t_kr, t_rxn_of_slot, t_spec_of_lib, t_lib_of_spec, t_kslot, t_stage_lib, t_stage_off;
  kin::DevBuf<double> t_par, t_T, t_u, t_du;   // Arrhenius parameters per record (4 doubles), temperatures, layout scratch
  bool t_par_valid = false;

  // the device this handle lives on (the one current at kin_network_create) and its compute units
  int device = 0, n_cu = 0;

  // solver + stored solution (solver.cpp)
  std::unique_ptr<kin::Solver> solver;
  std::unique_ptr<kin::IntegratorState> integ;   // return_integrator=true stepping state
  std::unique_ptr<kin::ResidentSolver, kin::ResidentDeleter> resident;   // one-workgroup-per-trajectory integrator (resident.cpp)
  std::unique_ptr<kin::EnsembleSolver, kin::EnsembleDeleter> ensemble;   // lockstep ensemble of large networks (ensemble.cpp)
  // solve-only copies of this handle (own stream, work vectors, Solver and LU cache; no sweep tables): a SMALL ensemble of a
  // large network is K independent kin_solve calls on K host threads (ensemble_routes.cpp: replica_ensemble)
  std::vector<kin_network*> replicas;
  size_t lu_budget_mb = 0;   // device memory of this handle's LU cache (0: KIN_LU_CACHE_MB, default 32768); set on replicas
  std::vector<double> sol_t, sol_u;
  kin::DevBuf<double> d_sol_u;   // saved states on the device, [n_saved][N]
  int64_t n_saved = 0;

  // The last ensemble call's saved states, where they live: sol[K][cap][N] (rows past n_saved[m] are zeros) in the resident
  // solver's or the lockstep ensemble's own buffer, or in ens_sol (thread route, lockstep calls of several blocks: the members'
  // rows copied device-to-device). Cleared when an ensemble call starts (run_ensemble), set when it succeeded (finish_ensemble,
  // both ensemble_routes.cpp); the buffers it may point to are reallocated by ensemble calls only (ResidentSolver::ensure with
  // own_sol, EnsembleSolver::prepare, replica_ensemble).
  struct EnsembleRecord {
    const double* sol = nullptr;
    int64_t K = 0, cap = 0;
    std::vector<int64_t> n_saved;
    // solved with per-member Arrhenius parameters (kin_solve_ensemble_*_params): Ea[K][R], A[K][R] on the device (ens_Ea / ens_A,
    // which only the next per-member call overwrites); null for a record of shared parameters
    const double *Ea = nullptr, *A = nullptr;
    // a record of observables (kin_ensemble_observables with store): its G, the columns that mean something - the others of
    // the N are zeros and no column is a species any more; 0 for a record of states
    int64_t observables = 0;
    bool valid() const { return sol != nullptr && K > 0; }
    bool member_params() const { return Ea != nullptr; }
    void clear() { sol = nullptr; K = 0; cap = 0; n_saved.clear(); Ea = nullptr; A = nullptr; observables = 0; }
  } ens;
  kin::DevBuf<double> ens_sol, ens_w, ens_out;   // handle-owned copy of the saved states; workspaces of kin_ensemble_max / _dot
  kin::DevBuf<double> ens_Ea, ens_A;             // the per-member parameter blocks of a kin_solve_ensemble_*_params call, reused across calls
  kin::DevBuf<int64_t> ens_segn;                 // n_saved[K] on the device
  // resampling (resample_api.cpp): the two buffers a resampled record lives in by turns (kin_ensemble_resample with store: the
  // result goes to the one the record is not in), and the host entries' staging of jc[S][Q] and w[S][Q]
  kin::DevBuf<double> ens_rs[2], rs_w;
  kin::DevBuf<int32_t> rs_jc;
  // observables (observable_api.cpp): the forms and observables of the last call as the caller gave them - a call that brings the
  // same ones finds its plan on the device - and the plan, on the host and uploaded
  std::vector<int64_t> ob_h_ptr, ob_h_idx, ob_h_num, ob_h_den;
  std::vector<double> ob_h_w;
  kin::ObsPlanHost ob_plan;
  bool ob_ready = false;
  kin::DevBuf<int32_t> ob_idx;
  kin::DevBuf<double> ob_w;
  kin::DevBuf<kin::ObsTask> ob_tasks;
  kin::DevBuf<kin::ObsPhase> ob_phases;
  void set_ensemble_record(const double* sol, int64_t K, int64_t cap, std::vector<int64_t> n_saved) {
    ens.sol = sol; ens.K = K; ens.cap = cap; ens.n_saved = std::move(n_saved);
  }

  // cross-member statistics (member_stats.hpp, member_stats_api.cpp): the index base kin_network_create was given (species
  // lists of these entries are in it); the participants, the selected species, the probabilities and the normalised inputs
  // on the device with the host copies the uploads read; the workspace Yhat[columns][n] of a block of columns; the staging
  // buffers of the host entries' states and outputs; the weights of the Sobol pass's participants
  int index_base = 0;
  std::vector<int32_t> ms_h_idx, ms_h_sel, ms_h_wt;
  std::vector<double> ms_h_p, ms_h_xhat;
  kin::DevBuf<int32_t> ms_idx, ms_sel, ms_wt;
  kin::DevBuf<double> ms_p, ms_xhat, ms_yhat, ms_u, ms_o[4];

  kin_network();
  ~kin_network();
  void rhs_dev(const double* d_u, double* d_du);        // du = f(u) with current k
  void jac_dev(const double* d_u, double* d_vals);      // CSR values with current k
  void sweep_dev(int64_t B, const double* d_u, const double* d_k, double* d_du, hipStream_t s);   // batched RHS
  // the launch plan sweep_dev executes for these buffers (d_k null: the handle's own rate constants)
  kin::SweepPlan sweep_plan_dev(int64_t B, const double* d_u, const double* d_k, const double* d_du) const;
};
