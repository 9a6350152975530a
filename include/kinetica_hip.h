/*
 * kinetica_hip.h - C ABI of libkinetica_hip.so, the MI355X (gfx950) implementation of
 * Kinetica.jl's kinetic-ODE solve path (src/solving in the reference).
 *
 * The reference has no FFI on this path (pure Julia multiple dispatch), so this
 * header DEFINES the boundary a `ccall` shim binds. Every entry
 * point cites the reference code it stands in for (paths relative to the reference
 * repository root). Conventions:
 *   - all entry points are extern "C", return an int status (KIN_OK == 0) and never throw;
 *   - plain pointers and sizes only; the caller owns every host buffer, the library
 *     never keeps a host pointer after a call returns;
 *   - Float64 / Int64 everywhere, as the reference (init_network(fType=Float64,
 *     iType=Int64), src/exploration/network.jl:491);
 *   - `index_base` is 1 when called from Julia (1-based species ids,
 *     src/exploration/network.jl:55-56) and 0 from C / Python;
 *   - one host thread per handle; handles are independent (one per GPU / stream);
 *   - a handle owns device memory; kin_network_destroy(NULL) is a no-op.
 * There is no CPU fallback: without a HIP device every compute call returns
 * KIN_ERR_DEVICE.
 */
#ifndef KINETICA_HIP_H
#define KINETICA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (error convention of SURVEY 8(b)) ------------------------------ */
enum {
  KIN_OK = 0,
  KIN_ERR_INVALID_ARG = 1,   /* ArgumentError in the reference (params.jl:77-104, calculator.jl:200-204) */
  KIN_ERR_UNSUPPORTED = 2,   /* molecularity > 2 on one side (network.jl:275-279) */
  KIN_ERR_DEVICE = 3,        /* HIP runtime error / no device */
  KIN_ERR_SOLVE_FAILED = 4,  /* ErrorException("ODE solution failed.") (solve_utils.jl:405-411) */
  KIN_ERR_CAPACITY = 5,      /* caller-provided output buffer too small */
  KIN_ERR_STATE = 6          /* call order violated (e.g. rates never set) */
};

/* ---- integrator return codes, 1:1 with SciMLBase.ReturnCode as consumed by
 *      successful_retcode (solve_utils.jl:391) and stored in the solution (methods.jl:862) */
enum {
  KIN_RETCODE_SUCCESS = 0,
  KIN_RETCODE_MAXITERS = 1,
  KIN_RETCODE_DTLESSTHANMIN = 2,
  KIN_RETCODE_UNSTABLE = 3     /* a non-finite state at (re)initialisation, or an accepted step that leaves a species below -1e3
                                * error weights (the blow-up of a negative concentration, given up before the step size has followed
                                * it down to dtmin; the tolerance retry of adaptive_tols treats it like any other failure) */
};

typedef struct kin_network kin_network; /* opaque */

/* ---- A1: CRN topology ------------------------------------------------------------- */
/* Replaces the four ragged vectors of RxData the solve reads (id_reacs, stoic_reacs,
 * id_prods, stoic_prods; src/exploration/network.jl:193-203) in flat CSR-like form:
 * reaction r consumes reac_idx[reac_ptr[r]..reac_ptr[r+1]) with stoichiometries reac_sto,
 * and likewise for products. ptr arrays are always 0-based offsets; idx uses index_base.
 * Rate law and ODEs are those of make_rs (src/solving/solve_utils.jl:318-334) with
 * combinatoric_ratelaws=false. */
int kin_network_create(int64_t n_species, int64_t n_reactions,
                       const int64_t* reac_ptr, const int64_t* reac_idx, const int64_t* reac_sto,
                       const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                       int index_base, kin_network** out);
int kin_network_destroy(kin_network* h);
int kin_network_sizes(const kin_network* h, int64_t* n_species, int64_t* n_reactions);
/* Last error text of this handle (or of the failed create when h == NULL). */
const char* kin_last_error(const kin_network* h);

/* ---- A6: rate constants ------------------------------------------------------------ */
/* DummyKineticCalculator / any external calculator: hand over k[R] directly
 * (calculator.jl:127-152 produces such a vector). */
int kin_set_rates(kin_network* h, const double* k);
int kin_get_rates(kin_network* h, double* k_out);
/* PrecalculatedArrheniusCalculator parameters (calculator.jl:164-198). k_max = NaN means
 * `k_max = nothing`, and so does k_max = +inf (1 / (0 + 1/k_r) = k_r; also in kin_arrhenius_eval); t_mult = tconvert(t_unit, "s") (calculator.jl:196, utils.jl:21-30). */
int kin_set_arrhenius(kin_network* h, const double* Ea, const double* A, double k_max, double t_mult);
/* k = calculator(; T) (calculator.jl:223-232) evaluated on the device; becomes the
 * handle's current rate vector; k_out (host, R doubles) may be NULL. */
int kin_rates_at(kin_network* h, double T, double* k_out);
/* Network-free form of the same functor, used by the host for get_max_rates /
 * apply_low_k_cutoff! (solve_utils.jl:19-54, 213-245) before a handle exists. */
int kin_arrhenius_eval(const double* Ea, const double* A, int64_t n, double k_max, double t_mult,
                       double T, double* k_out);
/* A8: calculate_discrete_rates (solve_utils.jl:91-109): table[s][r] = calculator(T[s])[r],
 * S x R doubles, row-major; generated on the device. out_table (host) may be NULL, in which
 * case the table only stays resident on the device for kin_solve. */
int kin_rate_table(kin_network* h, const double* T, int64_t n_stops, double* out_table);

/* ---- A2: mass-action right-hand side ------------------------------------------------ */
/* du = f(u; k) for the current rates: the generated f! of ODEProblem (methods.jl:157). */
int kin_rhs(kin_network* h, const double* u, double* du);
/* B states at once, host buffers in the reference's layout u[b][N], du[b][N] (sol.u is a
 * Vector of Vectors); k is per state k[b][R] or NULL (current rates for every state). */
int kin_rhs_batched(kin_network* h, int64_t B, const double* u, const double* k, double* du);
/* The same sweep on device-resident buffers (no PCIe), same state-major layouts u[b][N],
 * k[b][R] (or NULL), du[b][N]. `stream` is a hipStream_t (NULL = the handle's stream); the
 * call only enqueues (no allocation, no synchronisation: graph-capturable). The handle's stream is a non-blocking
 * stream of its own: work the caller has queued on OTHER streams (fills, arithmetic on these buffers) is not ordered
 * before the sweep - pass the stream that work runs on, or synchronise first. The same holds for every *_dev entry point. */
int kin_rhs_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, double* d_du, void* stream);
/* Which kernel instantiation and launch configuration kin_rhs_batched_dev takes for these buffers (nothing is launched, the
 * pointers are only inspected for their 16-byte alignment; d_k == NULL: the handle's own rate constants), and the same
 * without a device or a handle from the flat network lists (kin_network_create's), the compute units n_cu of a device
 * (kin_network_compute_units) and the low four address bits of u, of the rate constants in effect and of du.
 * info[KIN_SWEEP_PLAN_INFO]: kernel (0 register-resident records, 1 general, 2 coefficient records in LDS, 3 large-N hub /
 * tail, 4 the single-state kernels state after state: N >= 65535), workgroup size, register-resident record rows TR, record
 * rows per batch ILP, 1 if the block pairing (p, P + p) is read, 1 if rate constants travel as adjacent 16-byte pairs, 1 if
 * the state is staged in LDS, streamed batches of ILP rows n_a, of ILP + 1 rows n_b, grid, workgroups per compute unit,
 * split-accumulator entries, explicit-operand records, tail tiles, 1 if tail operands are addressed by species, dynamic LDS
 * bytes, species tiles, hubs, records (a reaction with its reverse, or a single reaction). Entries a kernel does not have are 0.
 * Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
#define KIN_SWEEP_PLAN_INFO 19
int kin_sweep_plan(kin_network* h, int64_t B, const double* d_u, const double* d_k, const double* d_du, int64_t* info);
int kin_sweep_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                        const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                        int index_base, int n_cu, int64_t B, int u_bits, int k_bits, int du_bits, int64_t* info);

/* ---- A2 in the library's own data layout ("library order"): the bandwidth path of the batched sweep --------------
 * The reference evaluates its RHS one state at a time inside the integrator; the batched sweep (ensembles, flux
 * analysis over sol.u) has no layout to inherit, so the library defines one in which ONE pass over a state's rate
 * constants needs random access to on-chip memory only (kinetica_jl_amd/csrc/tiled.hpp):
 *   species   [ hubs | window 0 | window 1 | ... ]   (the caller's order when the state fits on-chip memory, N <= 10 000)
 *   reactions every reaction next to its exact reverse, grouped by window; within a window the pairs first (two slots per
 *             record, 0.0 in the reverse slot of a reaction without one), then - when the network has lost a noticeable
 *             part of its reverses, as after the low-k cutoff (solve_utils.jl:213-245) - the reactions without a reverse
 *             at one slot each: a k row has k_len <= 2 x records doubles, reaction r at slot_of_reaction[r].
 * KIN_ERR_UNSUPPORTED (from every call of this block) when the network has no such layout: more than two product
 * molecules in a reaction, or rarely referenced species that do not fall apart into window-sized groups. */
/* k_len; species_of_lib[N] (library position -> species id, + index_base); slot_of_reaction[R] (+ index_base);
 * species_identity = 1 when the library species order is the caller's; info[6] = hubs, windows, records, on-chip
 * entries, split-accumulator entries, workgroup size. Any pointer may be NULL. */
int kin_lib_layout(kin_network* h, int index_base, int64_t* k_len, int64_t* species_of_lib, int64_t* slot_of_reaction,
                   int32_t* species_identity, int64_t* info);
/* The same layout computed on the host alone (no device, no handle): what the library-order tables contain, for tools
 * and for tests that replay the sweep's arithmetic on the CPU. `hubs` = 0 lets the library choose. info[10] = hubs,
 * windows, records, on-chip entries, split-accumulator entries, workgroup size, first window entry, iteration rows,
 * k_len, 1 if some window ends in one-slot records;
 * rec[records] = packed 64-bit records (four 14-bit on-chip labels with fixed roles + 3 flag bits at bit 56),
 * rowtab[2 x rows], seg_q[windows + 1], win_off / win_cnt[windows], copy_src[copies], seg_k[2 x windows] = slot of the
 * window's first record and the number of its records that have two slots (record i of the window: slot + 2 i below
 * that number n2, slot + n2 + i from it on). Call once with NULL arrays for the sizes. */
int kin_lib_layout_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                        const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                        int index_base, int hubs, int64_t* info, int64_t* species_of_lib, int64_t* slot_of_reaction,
                        uint64_t* rec, int32_t* rowtab, int32_t* seg_q, int32_t* win_off, int32_t* win_cnt, int32_t* copy_src,
                        int32_t* seg_k);
/* Which instantiation of the tiled sweep a call over B states takes (temperature_form != 0: rate constants formed in the
 * sweep; else the k stream), on the handle's device or - host variant, no device - on one of n_cu compute units.
 * info[KIN_TILED_PLAN_INFO]: workgroup size, 1 for the temperature form, staged doubles per thread UN (5 / 10), 1 for the
 * one-slot-record form SINGLES, record rows per batch NB, grid, workgroups per compute unit, dynamic LDS bytes, 1 if the
 * library species order is the caller's, windows, split-accumulator entries, 1 if some window ends in one-slot records.
 * The layout switches KIN_TILED_ENTRIES / KIN_TILED_SINGLES of the calling process are honoured, as when a handle builds
 * its layout. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
#define KIN_TILED_PLAN_INFO 12
int kin_tiled_sweep_plan(kin_network* h, int64_t B, int temperature_form, int64_t* info);
int kin_tiled_sweep_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                              const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                              int index_base, int n_cu, int64_t B, int temperature_form, int64_t* info);
/* Symbolic analysis of the Newton-matrix factorisation (I - c J; the reference's solver does this inside KLU,
 * docs/src/getting-started.md:69) WITHOUT a device: sizes only. Arguments <= 0 take the library's defaults.
 * info[0..11] = sparse pivots, dense block dimension, elimination rounds, nnz(U), nnz(L11^-1), nnz(U11^-1), nnz(L21 L11^-1),
 * nnz(U11^-1 U12), doubles per factorisation, symbolic products of the fused solve, gather-plan entries, wavefront tasks. */
int kin_lu_analyze_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                        const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                        int index_base, int hub_degree, int max_rounds, int max_tail_degree, int max_degree, int min_round,
                        int64_t* info);
/* Layout conversions on device buffers (each a coalesced write with a gather on the source side; enqueue only):
 * states u[b][N] caller order <-> library order, rate constants k[b][R] -> k_lib[b][k_len]. */
int kin_states_to_lib_dev(kin_network* h, int64_t B, const double* d_in, double* d_out, void* stream);
int kin_states_from_lib_dev(kin_network* h, int64_t B, const double* d_in, double* d_out, void* stream);
int kin_rates_to_lib_dev(kin_network* h, int64_t B, const double* d_k, double* d_k_lib, void* stream);
/* calculate_discrete_rates (solve_utils.jl:91-109) written directly in library order: d_out[s][k_len] (device). */
int kin_rate_table_lib_dev(kin_network* h, const double* T, int64_t n_stops, double* d_out);
/* The sweep: du_lib[b] = f(u_lib[b]; k) for b < B, device buffers in library order. Exactly one of d_k_lib
 * (k_lib[b][k_len], 16-byte aligned) and d_T (B temperatures) is non-NULL; with d_T the rate constants are formed
 * inside the sweep from the Arrhenius parameters - no k stream at all (SURVEY 8(d) M1'; the reference's continuous
 * path inlines k(T(t)) into every species ODE the same way, methods.jl:389-419 with calculator.jl:223-226).
 * HBM traffic per state: k_lib row (or nothing) + u row in, du row out. Enqueue only. */
int kin_rhs_tiled_dev(kin_network* h, int64_t B, const double* d_u_lib, const double* d_k_lib, const double* d_T,
                      double* d_du_lib, void* stream);
/* The temperature form on states in the CALLER's species order: u[b][N], T[b], du[b][N] (device). When the library
 * species order differs (species_identity == 0) the call converts the layout on the way in and out (16 N bytes per
 * state each way, workspace grown on demand). */
int kin_rhs_batched_T_dev(kin_network* h, int64_t B, const double* d_u, const double* d_T, double* d_du, void* stream);
/* The drop-in batched sweep for a caller whose RATE CONSTANTS come from this library (kin_rate_table_lib_dev, or converted once
 * by kin_rates_to_lib_dev): states u[b][N] and du[b][N] in the CALLER's species order - the reference's own sol.u layout -,
 * rate constants k_lib[b][k_len] in the slot order kin_lib_layout reports (16-byte aligned). The bandwidth-grade path at ANY
 * size and after the low-k cutoff (apply_low_k_cutoff!, solve_utils.jl:213-245, leaves reactions without their reverse):
 * hubs and windows in LDS, the k row streamed once; when the library species order differs from the caller's (N > ~10 000)
 * the states are permuted through LDS on the way in and out, one coalesced pass each (HBM traffic per state: 8 k_len + 16 N for
 * the sweep + 32 N for the two permutations). kin_rhs_batched_dev (rate constants in the caller's REACTION order) stays
 * correct at every size but cannot stream k once when the state does not fit LDS. Enqueue only. */
int kin_rhs_batched_klib_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k_lib, double* d_du, void* stream);

/* ---- N6: reaction-flux analysis (the "which reactions matter" companion of identify_next_seeds; the reference's
 *      analysis/ works on sol.u after the solve) -------------------------------------------------------------------
 * rate_r(u; k) = k_r u[x0_r] (x1_r >= 0 ? u[x1_r] : 1): the mass action of make_rs (solve_utils.jl:318-334) without 1/s!
 * (2A gives u_a^2, an inert collider is an ordinary operand). For B states u[b][N]:
 *   rates[b][r] = rate_r(u_b; k of state b)            (optional, unweighted)
 *   flux[r]     = sum_b w[b] rates[b][r]               (optional; w == NULL: weights 1; B == 0 writes zeros)
 * both in the caller's reaction order; at least one must be requested. State b's rate constants come from exactly one of
 *   - row k_row[b] of k[rows][R] (k_row == NULL: row b),
 *   - the handle's Arrhenius law at T[b] (evaluated as kin_rates_at does, inside the pass),
 *   - the handle's current rates, when neither k nor T is given (a pending continuous-rate temperature is formed first).
 * One pass over the states: per state the k row is streamed once, u is staged on chip, flux is reduced in a fixed order
 * (bitwise reproducible for given B, R, N and device). The partial sums live in the handle and are grown on demand: the
 * entry serves ONE stream per handle at a time and may allocate when B grows; afterwards it only enqueues.
 * KIN_ERR_INVALID_ARG: both k and T; k_row without a k source; a row index out of range (host entries); neither output;
 * B < 0. KIN_ERR_STATE: T without Arrhenius parameters; no rates at all; no stored solution; table rows asked for with no
 * resident table. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* device buffers (d_k_row: B int64 row indices, not validated); enqueue only once the workspace has its size */
int kin_flux_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                         const double* d_w, double* d_flux, double* d_rates, void* stream);
/* host buffers; k has n_k_rows rows (k_row validated against it; k_row == NULL needs n_k_rows == B) */
int kin_flux_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                     const double* T, const double* w, double* flux, double* rates);
/* the saved states of the last kin_solve / kin_solve_continuous / kin_solve_explicit, where they live (on the device):
 * no copy of the trajectory. w[n_saved], T_rows[n_saved], k_row[n_saved]. k == NULL with k_row != NULL reads rows of the
 * device-resident rate table (what kin_solve(k_table) / kin_rate_table left there). */
int kin_solution_flux(kin_network* h, const double* w, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T_rows, double* flux, double* rates);
/* Which kernel instantiation and grid a flux call takes, without a device or a handle: the launch plan of the per-state pass
 * (segmented == 0) or of the segmented pass (segmented != 0, B = S L) for a network of n_species x n_reactions on a device of
 * n_cu compute units (kin_network_compute_units). temperature_form != 0: temperatures given; else k rows k_stride doubles
 * apart (0: one shared row; n_reactions for the entries above). u_bits, k_bits, rates_bits: the low four address bits of
 * the state, rate-constant and per-state-rates buffers (rates_bits < 0: no rates asked for; the segmented pass has none).
 * The KIN_FLUX_LDS / KIN_FLUX_ROWS switches of the calling process are honoured, as in a real call.
 * info[6]: path (0 state staged in LDS as 16-byte words, 1 staged as it comes, 2 gathered from global memory), rows of
 * reaction pairs per thread, reaction parts, state slices G, k mode (0 16-byte loads, 1 8-byte loads, 2 Arrhenius law in the
 * kernel), rates mode (0 none, 1 16-byte stores, 2 8-byte stores). KIN_ERR_INVALID_ARG for sizes < 1 or bits outside 0 .. 15.
 * Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
int kin_flux_plan_host(int64_t n_species, int64_t n_reactions, int64_t B, int n_cu, int temperature_form, int segmented,
                       int64_t k_stride, int u_bits, int k_bits, int rates_bits, int64_t* info);
/* Compute units of the device the handle lives on (what its launch plans are sized by). */
int kin_network_compute_units(const kin_network* h, int* n_cu);

/* ---- A3: analytic sparse Jacobian ---------------------------------------------------- */
/* Replaces ODEProblem(...; jac=true, sparse=true) (methods.jl:157-158): pattern (CSR,
 * sorted columns, diagonal always present) and values for the current rates. The reference
 * stores SparseMatrixCSC; CSR of J is CSC of transpose(J), the shim picks what it needs. */
int kin_jac_nnz(kin_network* h, int64_t* nnz);
int kin_jac_pattern(kin_network* h, int64_t* rowptr, int64_t* colidx, int index_base);
int kin_jac_values(kin_network* h, const double* u, double* vals);

/* ---- A12: ODESimulationParams (src/solving/params.jl:3-27, defaults :55-75) ---------- */
typedef struct kin_params {
  double tspan0, tspan1;     /* tspan */
  double abstol;             /* 1e-10 */
  double reltol;             /* 1e-8  */
  int32_t adaptive_tols;     /* true  */
  int32_t update_tols;       /* false */
  int32_t solve_chunks;      /* true (1): chunkwise in local time, the integrator re-initialised at every chunk start as the
                              * reference does (methods.jl:819); 0: complete timespan; 2 (EXTENSION): chunkwise with difference
                              * history, order and step size carried across chunk starts whose rate constants did not change
                              * (a StaticODESolve's chunk boundaries are not events); rate updates still re-initialise */
  int32_t ban_negatives;     /* false: isoutofdomain = any(u < 0) (methods.jl:169-171) */
  double solve_chunkstep;    /* 1e-3  */
  int64_t maxiters;          /* 100000 */
  double save_interval;      /* < 0 means `nothing` */
  double dtmin;              /* minimum step size handed to the integrator; <= 0 selects the reference's own choice:
                              * eps(solve_chunkstep) for chunkwise solves (methods.jl:232, 770), eps(tspan[end]) for
                              * complete-timespan solves (methods.jl:164, 694). A step that merely STARTS below dtmin is
                              * raised to it (CVodeSetMinStep semantics); a step pushed below it by the corrector or
                              * the error test ends the attempt with KIN_RETCODE_DTLESSTHANMIN, which the retry loop
                              * (adaptive_solve!, solve_utils.jl:376-424) answers with tighter tolerances. */
  /* `solver`, `jac`, `sparse`, `progress`, `u0`, `low_k_*`, `allow_short_u0` are consumed
   * by the host layer (the integrator is always the library's BDF with the analytic
   * sparse Jacobian). */
} kin_params;

typedef struct kin_stats {
  int64_t n_steps, n_rejected, n_rhs, n_jac, n_factor, n_linsolve, n_newton_fail;
  /* n_rhs / n_linsolve: corrector iterations the device executed (launches enqueued ahead of a decision that turn into
   * no-ops are not counted), plus the right-hand sides of restarts */
  int64_t n_chunks, n_restarts, n_retries;
  double final_abstol, final_reltol; /* what update_tols writes back (solve_utils.jl:397-401) */
  double wall_seconds;
  int64_t lu_dense_dim, lu_sparse_rows, lu_rounds, lu_nnz;
  int64_t n_lu_reused;   /* step attempts that started on a cached factorisation (the solver's LU cache) */
  int64_t lu_slots;      /* size of that cache */
  int64_t n_bad_pivot;   /* factorisations dropped because a pivot vanished (answered by a fresh Jacobian and half the step) */
  int64_t n_lu_dropped;  /* cached factorisations dropped at a restart because the Jacobian's diagonal had drifted */
} kin_stats;

/* ---- A4/A5/A9/A10: the solve --------------------------------------------------------- */
/* Integrates du/dt = f(u; k) over params->tspan from u0 with the library's variable-order
 * BDF (orders 1-5, modified Newton, analytic sparse Jacobian, on-device sparse LU), standing
 * in for init/solve!/reinit! of the user-supplied stiff solver (methods.jl:174, 241, 260,
 * 779, 819; solve_utils.jl:389) including:
 *   - chunkwise local-time solving and output stitching (methods.jl:185-303, 717-865),
 *   - complete-timespan solving (methods.jl:132-183, 655-714) when solve_chunks == 0,
 *   - discrete rate-constant updates at `tstops` (solve_utils.jl:435-509): k is held
 *     piecewise constant and switched at every tstop; rates come from k_table[s][R] (host,
 *     any calculator) or, when k_table == NULL, from the Arrhenius parameters at T_stops[s];
 *     n_stops == 0 means static rates (StaticODESolve),
 *   - the tolerance-tightening retry loop adaptive_solve! (solve_utils.jl:376-424).
 * Results stay in the handle; fetch them with kin_solution_size / kin_solution_copy.
 * Returns KIN_ERR_SOLVE_FAILED (with *retcode set) when adaptive_solve! would throw. */
int kin_solve(kin_network* h, const kin_params* params, const double* u0,
              const double* tstops, const double* T_stops, const double* k_table, int64_t n_stops,
              int64_t* n_saved, int32_t* retcode, kin_stats* stats);
/* An ENSEMBLE of K independent trajectories of one network in ONE call (the reference leaves ensembles to the user:
 * docs/src/tutorials/ode-solution.md:190 solves member after member through solve_network, exploration/methods.jl:221).
 * Every member is integrated by the same algorithm as kin_solve (csrc/resident_core.hpp is the controller of all paths):
 *   - a network that fits one compute unit's LDS (up to ~1 000 species): ONE launch, one workgroup owns one member from u0 to
 *     the end of the span; a member's result is bit-identical to a K = 1 call with its inputs;
 *   - larger networks, up to 12 members (KIN_ENSEMBLE_THREADS): K kin_solve calls on K host threads, each on a solve-only copy
 *     of the handle (kept with the handle for later calls); bit-identical to kin_solve on the member's inputs;
 *   - larger networks, more members: the members advance in lockstep rounds, every launch of a round carries all members
 *     that need that kind of work (csrc/ensemble.cpp); a member's result equals its solo kin_solve within the step-sequence
 *     tolerance.
 *   u0[K][N]; rate constants per member k[K][R], or temperatures T[K] (Arrhenius parameters of the handle), or neither
 *   (the handle's current rates for all); discrete rate updates (tstops / T_stops / k_table as in kin_solve) are shared
 *   by all members and exclude k / T. `params` needs a save grid (solve_chunks or save_interval).
 * Outputs (any may be NULL): *n_rows = rows of the save grid; out_t[n_rows]: the save times of the member that got furthest
 * (most saved rows, the first of them), 0.0 from its n_saved on - so all of n_rows times when one member completed the grid;
 * out_u[K][n_rows][N]; n_saved[K] rows a member actually wrote (the rows of out_u beyond them - a member that failed early -
 * are zero); retcodes[K] (KIN_RETCODE_*); stats[K].
 * A call with out_u == NULL and n_saved == NULL only reports *n_rows.
 * Returns KIN_OK when the call ran, whatever the members' retcodes; KIN_ERR_UNSUPPORTED for a network that fits neither
 * path (too large for the resident kernel and without a dense Schur block): solve those member by member with kin_solve. */
int kin_solve_ensemble(kin_network* h, const kin_params* params, int64_t K, const double* u0, const double* k, const double* T,
                       const double* tstops, const double* T_stops, const double* k_table, int64_t n_stops, int64_t* n_rows,
                       double* out_t, double* out_u, int64_t* n_saved, int32_t* retcodes, kin_stats* stats);
/* Same call with an explicit integrator: `pars.solver` may be any SciML algorithm (params.jl:9); BASELINE config 2
 * exercises the RHS kernel with an explicit one. The pair is Dormand-Prince 5(4) with FSAL and 4th-order dense
 * output, step-size control as in SciPy's RK45 (which is the oracle, step for step); no Jacobian, no linear solve.
 * Orchestration (chunks, save grid, discrete rate updates, tolerance retries) is kin_solve's. */
int kin_solve_explicit(kin_network* h, const kin_params* params, const double* u0, const double* tstops, const double* T_stops,
                       const double* k_table, int64_t n_stops, int64_t* n_saved, int32_t* retcode, kin_stats* stats);

/* N3: continuous rate updates (reference: methods.jl:363-653, where k(t) = calculator(T(t)) is inlined
 * symbolically into every species ODE). Here the integrator is simply non-autonomous: the Arrhenius
 * rates are re-evaluated on the device at T(t_new) for every step attempt; T(t) is the linear
 * interpolation of the profile solution (t_nodes, T_nodes), as the reference's DiffEqArray functor does
 * (src/utils.jl:135-139). Chunking / save grid / retry semantics as kin_solve; no restarts at all. */
int kin_solve_continuous(kin_network* h, const kin_params* params, const double* u0, const double* t_nodes,
                         const double* T_nodes, int64_t n_nodes, int64_t* n_saved, int32_t* retcode, kin_stats* stats);
/* An ENSEMBLE of K trajectories under continuous rate updates, one temperature profile per member (reference: a
 * VariableODESolve whose ConditionSet has no ts_update, methods.jl:363-653; the obvious sweep is a set of heating rates or
 * start temperatures). Member m's rates are re-evaluated at T(t) of every step attempt, T(t) the linear interpolation of its
 * profile (t_nodes, T_nodes)[node_ptr[m] .. node_ptr[m + 1]) in global time (src/utils.jl:135-139); node counts may differ.
 *   - a network the resident kernel takes (as in kin_solve_ensemble): ONE launch, one workgroup per member, the profiles
 *     uploaded once; a member's result is bit-identical to a K = 1 call with its inputs and equals its kin_solve_continuous
 *     within the step-sequence tolerance;
 *   - larger networks: kin_solve_continuous calls on host threads (KIN_ENSEMBLE_THREADS; beyond it a thread takes several
 *     members), bit-identical to kin_solve_continuous on the member's inputs. There is no lockstep form:
 *     KIN_ENSEMBLE_ROUTE=lockstep returns KIN_ERR_UNSUPPORTED.
 * Per member as kin_solve_continuous: >= 2 nodes, non-decreasing t (else KIN_ERR_INVALID_ARG), Arrhenius parameters set on
 * the handle (else KIN_ERR_STATE). u0, the save-grid requirement, the outputs, the size query and the return value are those
 * of kin_solve_ensemble. */
int kin_solve_ensemble_continuous(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                  const int64_t* node_ptr, const double* t_nodes, const double* T_nodes,
                                  int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved,
                                  int32_t* retcodes, kin_stats* stats);
/* An ENSEMBLE of K trajectories under discrete rate updates, one stop schedule per member (reference: a VariableODESolve whose
 * ConditionSet has ts_update, solve_utils.jl:435-509, swept over heating rates / start temperatures). Member m's rates are the
 * Arrhenius rates (handle's parameters) at T_stops[j], held from tstops[j] on, j in [stop_ptr[m], stop_ptr[m + 1]) -
 * exactly kin_solve's zero-order hold with that member's (tstops, T_stops). Stop counts may differ.
 * Per member as kin_solve: >= 1 stop, strictly increasing tstops (else KIN_ERR_INVALID_ARG), Arrhenius parameters set on the
 * handle (else KIN_ERR_STATE); a null stop_ptr / tstops / T_stops is KIN_ERR_INVALID_ARG. u0, the save-grid requirement, the
 * outputs, the size query and the return value are those of kin_solve_ensemble. Added without a KIN_ABI_VERSION change
 * (purely additive, structs unchanged): a binding detects it by symbol lookup. */
int kin_solve_ensemble_discrete(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                const int64_t* stop_ptr, const double* tstops, const double* T_stops,
                                int64_t* n_rows, double* out_t, double* out_u, int64_t* n_saved,
                                int32_t* retcodes, kin_stats* stats);
/* The two calls above with Arrhenius parameters of each member's own (uncertain barriers and prefactors under a temperature
 * programme: a design over rate parameters in ONE ensemble call). Ea[K][R], A[K][R]: member m's rates are
 * arrhenius_one(Ea[m][r], A[m][r], R T, ...) with has_kmax / k_max / t_mult of the handle, so kin_set_arrhenius is still
 * required (else KIN_ERR_STATE); the handle's own Ea / A are neither read nor changed. Ea == NULL and A == NULL: exactly the
 * call above (same code path, same bits); exactly one of them NULL: KIN_ERR_INVALID_ARG. Every route takes them: the resident
 * kernel reads each member's rows (a member is bit-identical to a K = 1 call on a handle set to its parameters), the thread
 * route solves member m on a replica holding its parameters (bit-identical to kin_solve / kin_solve_continuous on such a
 * handle), the lockstep rounds (discrete only) form each member's rates from its rows. The blocks cost 16 K R bytes on the
 * device, stay with the stored ensemble and are reused by later calls (a failed allocation: KIN_ERR_DEVICE, the size in
 * kin_last_error). The stored ensemble remembers it was solved this way: kin_ensemble_flux with T_rows evaluates every
 * member's rate constants from its own rows; kin_ensemble_drg / _drgep / _pfa / _reaction_importance / _timescale with T_rows
 * return KIN_ERR_UNSUPPORTED on such a record (they would use the handle's one pair) - give them k / k_row, one
 * kin_arrhenius_eval row per member and temperature; everything that reads states only (kin_ensemble_max / _dot / _moments /
 * _quantiles / _correlate / _sobol) works on either record. A later shared call leaves a shared record again. All other
 * arguments, the size query and the return values are those of the calls above. Added without a KIN_ABI_VERSION change
 * (purely additive, structs unchanged): a binding detects them by symbol lookup. */
int kin_solve_ensemble_continuous_params(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                         const double* Ea, const double* A, const int64_t* node_ptr, const double* t_nodes,
                                         const double* T_nodes, int64_t* n_rows, double* out_t, double* out_u,
                                         int64_t* n_saved, int32_t* retcodes, kin_stats* stats);
int kin_solve_ensemble_discrete_params(kin_network* h, const kin_params* params, int64_t K, const double* u0,
                                       const double* Ea, const double* A, const int64_t* stop_ptr, const double* tstops,
                                       const double* T_stops, int64_t* n_rows, double* out_t, double* out_u,
                                       int64_t* n_saved, int32_t* retcodes, kin_stats* stats);
/* N1: return_integrator=true (methods.jl:105-106, 175-178, 242-246, 706-709): `init(oprob, solver; kwargs...)`
 * without solve!. The integrator spans the whole tspan (solve_chunks = 0) or the first chunk
 * [0, solve_chunkstep] (solve_chunks = 1, what the reference hands back); tstops / T_stops / k_table as
 * in kin_solve (n_stops = 0: the rates set on the handle). Save grid and the tolerance retry loop are
 * not part of an integrator (they belong to adaptive_solve!, solve_utils.jl:376-424). */
int kin_integrator_init(kin_network* h, const kin_params* params, const double* u0, const double* tstops,
                        const double* T_stops, const double* k_table, int64_t n_stops);
/* The same for continuous rate updates (methods.jl:363-458 with :445-449, and :461-653): the integrator re-evaluates
 * the Arrhenius rates at T(t) of every step attempt, T(t) as in kin_solve_continuous. */
int kin_integrator_init_continuous(kin_network* h, const kin_params* params, const double* u0, const double* t_nodes,
                                   const double* T_nodes, int64_t n_nodes);
/* step!(integ) x max_steps accepted steps (max_steps <= 0: solve!(integ), run to the end of the span);
 * rate updates fire when the time reaches a tstop (solve_utils.jl:435-509). steps_taken < max_steps
 * means the end of the span was reached or the integrator failed (see kin_integrator_state). */
int kin_integrator_step(kin_network* h, int64_t max_steps, int64_t* steps_taken);
/* integ.t, integ.u[N], the integrator's KIN_RETCODE_* and counters; any pointer may be NULL. */
int kin_integrator_state(kin_network* h, double* t, double* u, int32_t* retcode, kin_stats* stats);
int kin_solution_size(const kin_network* h, int64_t* n_saved, int64_t* n_species);
/* out_t[n_saved], out_u[n_saved][N] (sol.t / sol.u of ODESolveOutput, analysis/io.jl:3-11). */
int kin_solution_copy(const kin_network* h, double* out_t, double* out_u);
/* N2: max over saved times of each species (what identify_next_seeds reads,
 * src/exploration/explore_utils.jl:344-351), reduced on the device. */
int kin_solution_max(const kin_network* h, double* out_umax);

/* ---- multi-GPU building blocks (one process per GPU; the collectives themselves are RCCL calls of the host layer) -- */
/* kin_solution_max into a caller-owned DEVICE buffer of N doubles: what an ensemble of replicas all-gathers. */
int kin_solution_max_dev(const kin_network* h, double* d_out);
/* kin_rate_table for a slice of time stops straight into a caller-owned DEVICE buffer [n_stops][R] (T on the host):
 * ranks generate disjoint slices of the table; an all-gather follows only if sol_k is wanted. */
int kin_rate_table_dev(kin_network* h, const double* T, int64_t n_stops, double* d_out);
/* Partial right-hand side of reactions [r_lo, r_hi) only: du_partial = sum over the block of nu * rate (device buffers,
 * enqueue only). Summed over a partition of the reactions (an all-reduce of N doubles) it is kin_rhs: the reaction-block
 * decomposition of ONE trajectory. */
int kin_rhs_block_dev(kin_network* h, int64_t r_lo, int64_t r_hi, const double* d_u, double* d_du, void* stream);

/* out[t] = sum_i w[i] * u_i(t) for every saved time, reduced on the device: conserved quantities of the network
 * (element or mass balances - what a caller checks before trusting a long run) without copying the trajectory. */
int kin_solution_dot(const kin_network* h, const double* w, double* out);
/* Selected rows of the device-resident rate table (k_precalc[s] of calculate_discrete_rates, solve_utils.jl:91-109):
 * out[i][R] = table[rows[i]][:]. The full table (5.6 GB at 14 001 stops x 50 000 reactions) never has to cross PCIe
 * for a caller that wants sol_k at a few stops. */
int kin_rate_table_rows(kin_network* h, const int64_t* rows, int64_t n_rows, double* out);

/* Diagnostic: one Newton-matrix solve on the device, (I - c*J(u)) x = b with the current rates,
 * through exactly the factorisation / substitution kernels kin_solve uses (what KLU does for
 * CVODE in the reference's documented setup, docs/src/getting-started.md:69). */
int kin_newton_solve(kin_network* h, double c, const double* u, const double* b, double* x);
/* Diagnostic: K Newton-matrix solves through the host-driven factorisation and solve kernels (kin_solve's path above the resident
 * kernel's size, and every thread / lockstep ensemble), with the current rates and the handle's own analysis (the KIN_LU_EXPLICIT /
 * KIN_LU_FUSED switches are read when that analysis first runs). Member i (arrays row-major): I - c[i] J(u[i]) is factorised into a
 * slot of its own, x[i] = (I - c[i] J(u[i]))^-1 b[i]; bad[i] = 1 when a pivot of that factorisation vanished (the call still returns
 * KIN_OK, x[i] is then meaningless). batched = 0: every dense Schur block is inverted by the single-matrix Gauss-Jordan chain, as in
 * kin_solve; batched = 1: the dense blocks of up to 16 members at a time are inverted by ONE batched chain, as in the lockstep
 * ensemble. info (8 + n_species entries): sparse rows ns, dense block size m, its padded size, elimination rounds, solve form
 * (0 fused, 1 explicit, 2 round by round), Gauss-Jordan block steps (padded size / 32), whole-workgroup gather rows over all
 * plans, longest gather row over all plans; then the species at dense positions 0 .. m-1. KIN_ERR_STATE without rates,
 * KIN_ERR_INVALID_ARG for K < 1 or a null buffer. Added under KIN_ABI_VERSION 6: look the symbol up before calling it. */
int kin_newton_probe(kin_network* h, int64_t K, int32_t batched, const double* u, const double* c, const double* b,
                     double* x, int32_t* bad, int64_t* info);
/* Diagnostic: the resident integrator's own phases (one workgroup per trajectory, kin_solve's path for small networks and every
 * one-launch ensemble), run once for K members in one launch with the current rates. Member m (arrays row-major, m-th row):
 * du[m] = f(u[m]); jac[m] = J(u[m]) in kin_jac_pattern order; x[m] = (I - c[m] J(u[m]))^-1 b[m] through the kernel's
 * factorisation and its solve form; bad[m] = 1 when a pivot of that factorisation vanished (x[m] is then meaningless).
 * info (8 + n_species entries): dense Schur block size m, sparse rows ns, elimination rounds, solve form (0 fused,
 * 1 explicit, 2 plain), task descriptors in LDS (0/1), dynamic LDS bytes, padded dense size, 0; then the species at dense
 * positions 0 .. m-1. KIN_ERR_UNSUPPORTED when the network does not fit the resident kernel, KIN_ERR_STATE without rates. */
int kin_resident_probe(kin_network* h, int64_t K, const double* u, const double* c, const double* b, double* du, double* jac,
                       double* x, int32_t* bad, int64_t* info);
/* Diagnostic: ONE operation of the BDF / Dormand-Prince step, run ONCE on the caller's state through the integrators' own launchers
 * and kernels; everything the operation may write comes back (and everything it must not touch, so that can be checked too).
 * path 0: the host-driven kernels (launch_bdf_*, launch_rk_*), K = n_entries = 1, n is the caller's (the handle gives the device
 * and the stream); path 1: the corrector update fused into the solve's last gather launch (SparseLU::solve_newton), K = 1, n = the
 * handle's species count, op = NEWTON only; path 2: the lockstep ensemble's batched kernels, K members and n_entries list entries
 * in one launch (the list may permute the members or leave some out), n is the caller's; paths 3 and 4: the resident kernel (one
 * 512-thread workgroup per member, K members in one launch, n_entries = K, n = the handle's species count, the network must fit
 * the kernel) in its default build (3: 256 registers per lane, phases as functions) and its shared-CU build (4: 128 registers,
 * phases inlined), through the kernel's real dispatch - wavefront 0 builds the controller and calls ITS method (predict, change_D
 * and interpolate form their coefficients and matrices on the device), the other seven wavefronts decode the posted command in
 * worker_loop. See "Paths 3 and 4" below.
 *   state[K][KIN_STEP_ROWS][n], rows: 0-7 D; 8 y; 9 psi; 10 d; 11 scale; 12 f0; 13 f1; 14 ytmp; 15 cs; 16-22 the stage array
 *     K[7]; 23 x (solution vector); 24 out; 25 y_new; 26 u; 27 b. Uploaded, operated on, downloaded whole.
 *   ctrl[K][KIN_STEP_CTRL]: BdfCtrl as doubles - dy_norm_old, dy_norm, err_norm, err_m_norm, err_p_norm, crate, scratch[0..3],
 *     newton_done, converged, n_iter, nonfinite, any_negative, ticket, lu_bad, spec_go. In and out.
 *   iarg[n_entries][KIN_STEP_IARGS]: 0 member; 1 order; 2 aux (ACCEPT_PREDICT: order of the accepted step; INIT_D: 1 = from
 *     ytmp; NORMS: 1 = with f1; RK_COMBINE: stages; VEC: the EnsVecOp; PREDICT on path 2: 1 = a predictor on its own);
 *     3 copy_out (ACCEPT, ACCEPT_PREDICT: the new state also into row 24); 4 go (ACCEPT_PREDICT: 1 = the launch is given
 *     &ctrl->spec_go as its go flag); 5 iter; 6 maxit; 7 publish_always; 8 crate_from_ctrl; 9 ban_negatives; 10 seq; 11 row (paths
 *     3 and 4: the solution row, 0 or 1, of INTERP and of VEC's save_y / set_time).
 *     (NEWTON on path 2 takes iter from entry 0 and the ensemble's fixed iteration limit.)
 *   darg[n_entries][KIN_STEP_DARGS]: 0 atol; 1 rtol; 2 h (INIT_D) / factor (CHANGE_D: the matrix is built by
 *     bdf_change_D_matrix(order, factor)) / the scalar of VEC's axpy; 3 upd; 4 tol; 5 rate_max; 6 crate0; 7 tol_first;
 *     8 dy_first_max; 9 c (path 1); 10-12 ts, t, h_abs (INTERP: weights from bdf_interp_weights); 13-19 stage weights
 *     (RK_COMBINE, RK_ERROR); paths 3 and 4: 9 c; 20 c_fact; 21-23 ec, ec_m, ec_p (error constants of order, order - 1, order + 1).
 *   xloc[n] (NEWTON on paths 0 and 2): a permutation of 0 .. n-1; row 23 is scattered into the W buffer through it.
 *   Operands: INIT_D y (or ytmp), f0 -> D; PREDICT / ACCEPT / ACCEPT_PREDICT / CHANGE_D as the integrators call them; INTERP
 *     -> row 24; NORMS y, f0, f1 -> ctrl; NEWTON row 23, scale, y, d, D -> y, d, ctrl; RK_COMBINE y, K -> row 24; RK_ERROR
 *     y, row 25, K -> ctrl; VEC: `out` is row 24. Path 1: I - c J(u) (row 26, current rates) is factorised, b (row 27) placed, the
 *     solve and the update run in solve_newton; the x that launch produced is returned in row 23.
 *   pub[KIN_STEP_CTRL + 1] (paths 0 and 1, NEWTON and RK_ERROR): the block the launch published to pinned host memory and the
 *     sequence word; unpublished: every integer field -1, every double NaN, sequence word 0.
 *   info[8], path 1: the stage-C plan's ELL groups, one-wavefront rows, of those with more than 256 entries, whole-workgroup
 *     rows, its longest row, the dense block size m, the launch's grid size and workgroup size. Other paths: zeros.
 *   Paths 3 and 4. Rows 0-7 ARE the member's T.D, 12-15 its f0 / f1 / ytmp / chunk_start, 24-25 rows 0 / 1 of its solution buffer,
 *     26 its u0; rows 8-11 are loaded into the kernel's LDS arrays y / psi / d / scale before the operation and stored back after
 *     it. Operations: VEC (aux: 0 load_u0 .. 5 ytmp_axpy with h; 6 save_y(row, t); 8 set_time(row, t)), NORMS (aux: with f1),
 *     INIT_D (aux: from ytmp), PREDICT (ctl->predict()), ACCEPT, CHANGE_D (ctl->change_D(order, factor)), INTERP
 *     (ctl->interpolate(ts, row) with t, h_abs, order from the entry, then set_time(row, ts)), NEWTON and CORRECTOR: the Jacobian
 *     at the state in row 26 with the handle's rates, I - c_fact J factorised into slot 0 (the vanished-pivot flag comes back in
 *     lu_bad), then NEWTON: ONE iteration of the corrector (residual from y, psi, d at c; solve; update with upd), the x it used
 *     in row 23; CORRECTOR (paths 3 and 4 only): the whole attempt b.corrector(in) - predictor from D, up to four iterations and
 *     their decisions -, `in` from order, c, upd, rate_max, crate0, tol_first, tol, dy_first_max, ec*, atol, rtol.
 *     ctrl: NORMS -> scratch0-3 = rms(y/w), rms(f0/w), rms((f1-f0)/w), max |f0|/(0.1|y|+w), nonfinite; NEWTON -> dy_norm,
 *     err_norm, err_m_norm, err_p_norm = the RAW SUMS s, se, sm, sp of the iteration (not norms), any_negative = 0 / 1 shallow /
 *     3 deep; CORRECTOR -> newton_done, converged, n_iter, nonfinite, any_negative (0 / 1 / 3), err_norm, err_m_norm, err_p_norm
 *     (norms; 0 unless converged), crate; VEC's save_y / set_time and INTERP: scratch0 / scratch1 carry the times of solution rows
 *     0 / 1 in and out. Every other field comes back as given. pub: unpublished.
 *     info[8]: species N, trips of a 512-stride loop and wavefronts that own a species - all three counted by the kernel (-1:
 *     the members disagree) -, dense block size
 *     m, solve form (0 fused, 1 explicit, 2 plain), task descriptors in LDS (0/1), dynamic LDS bytes, waves per SIMD (2 or 4).
 * KIN_ERR_UNSUPPORTED: path 1 on a handle whose analysis has no fused solve or m = 0, an op a path does not have (CORRECTOR on
 * paths 0-2), a network that does not fit the resident kernel (paths 3 and 4);
 * KIN_ERR_INVALID_ARG: sizes, orders, members or xloc out of range; KIN_ERR_STATE: path 1 without rates. The handle is usable
 * afterwards (a later solve is bit for bit that of a fresh handle). Added under KIN_ABI_VERSION 6: look the symbol up. */
#define KIN_STEP_ROWS 28
#define KIN_STEP_CTRL 18
#define KIN_STEP_IARGS 12
#define KIN_STEP_DARGS 24
enum { KIN_STEP_INIT_D = 0, KIN_STEP_PREDICT, KIN_STEP_ACCEPT, KIN_STEP_ACCEPT_PREDICT, KIN_STEP_CHANGE_D, KIN_STEP_INTERP,
       KIN_STEP_NORMS, KIN_STEP_NEWTON, KIN_STEP_RK_COMBINE, KIN_STEP_RK_ERROR, KIN_STEP_VEC, KIN_STEP_CORRECTOR };
int kin_step_probe(kin_network* h, int32_t path, int32_t op, int64_t n, int64_t K, int64_t n_entries, const int32_t* iarg,
                   const double* darg, const int32_t* xloc, double* state, double* ctrl, double* pub, int64_t* info);

/* Diagnostic: the right-hand side, the Jacobian values or the Newton residual of a BDF step, formed ONCE on the caller's states
 * through the integrators' own launchers and kernels, every value of the output returned (and what must not be touched, so that
 * can be checked too).
 * path 0: the single-state kernels as kin_rhs / kin_jac_values and the host-driven corrector launch them, with the handle's rate
 *   constants (k must be NULL), K = n_entries = 1. T > 0: that temperature is made pending first, so the evaluation runs the
 *   kernels that form k from it on the spot and store it (kin_get_rates reads it afterwards); needs kin_set_arrhenius.
 * path 2: the lockstep ensemble's batched kernels: K members (1 .. 64) with buffers of the probe's own and rate constants
 *   k[K][R] per member, members[n_entries] of them (distinct) in one launch; members not named keep their buffers.
 * op KIN_EVAL_RHS: u[K][N] -> out. Path 0: out[N]. Path 2: mode is the source mode of ens_rhs (0: y -> f0, 1: ytmp -> f1,
 *     2: ytmp -> f0; the state is placed in the source the mode reads, the other source holds the sentinel),
 *     out[K][out_len] = f0 | f1 of each member (out_len >= 2 N); rate[K][R], when given, the members' rate buffers.
 *   KIN_EVAL_JAC: out[K][out_len], out_len >= nnz: the values in kin_jac_pattern order. Path 2: rate[K][2 R], when given, the
 *     members' operand-derivative buffers (filled with the sentinel first).
 *   KIN_EVAL_RESID: the rates with the corrector's skip flag, then c f(u) - psi - d gathered into the permuted solve vector through
 *     the solver's (path 0) or the ensemble's (path 2) own residual plan. c[K], psi[K][N], d[K][N]; done[K]: the value of
 *     newton_done the kernels find (non-zero: both launches are no-ops). The rate buffer and the window of W that holds the solve
 *     vectors are filled with `sentinel` first and come back as they stand: rate[K][R], out[K][out_len] (out_len >= the window's
 *     length), with yloc[N]: the position of species i's residual inside that window (the analysis's yloc less the window's start).
 *   KIN_EVAL_SIZES: no launch; info only (the residual plan of the path).
 * Output buffers of RHS and JAC are the probe's own on the device, pre-filled with NaN: an entry no kernel wrote comes back NaN.
 * info[8]: of the gather plan the operation used - ELL groups G, one-wavefront rows S, whole-workgroup rows B, its longest row,
 *   the rows in the ELL groups, the workgroup size the launcher takes for the plan (segsum_wg: 256 / 1024); RESID and SIZES: the solve-vector window's length,
 *   else 0; the Jacobian's nnz.
 * KIN_ERR_INVALID_ARG: sizes, members, mode or T out of range, k given on path 0 or missing on path 2; KIN_ERR_CAPACITY: out_len too
 * small; KIN_ERR_STATE: no rates, or T without Arrhenius parameters; a refused call leaves the handle as it was. Path 0 works in the
 * handle's own buffers: the residual overwrites the host-driven solver's step vectors y, psi, d (slot 0's solve vectors and the control
 * block are restored), and T > 0 replaces the handle's rate constants for good. A later kin_solve is bit for bit that of a fresh handle
 * with those rates; an integrator opened with kin_integrator_init does NOT survive a path 0 call and has to be initialised again.
 * Added under KIN_ABI_VERSION 6: look the symbol up before calling it. */
enum { KIN_EVAL_RHS = 0, KIN_EVAL_JAC, KIN_EVAL_RESID, KIN_EVAL_SIZES };
int kin_eval_probe(kin_network* h, int32_t path, int32_t op, int32_t mode, int64_t K, int64_t n_entries, const int32_t* members,
                   const double* u, const double* k, double T, const double* c, const double* psi, const double* d,
                   const int32_t* done, double sentinel, double* out, int64_t out_len, double* rate, int32_t* yloc, int64_t* info);

/* Diagnostic: the LU cache's drift guard and slot rules, run ONCE on the caller's values through the integrators' own launchers,
 * kernels and backends. The probe computes nothing itself, and every index array the kernels use is the handle's own.
 * mode KIN_CACHE_DRIFT: n_slots slots are made from the Jacobian value arrays jv_slots[n_slots][nnz] (kin_jac_pattern order) at
 *   c_fact[n_slots], with flags valid[n_slots] (0: the slot counts as unused), and tested against today's values jv_now[nnz] with
 *   the threshold max_drift.
 *   path 0 (host-driven: Solver::restart / resume_chunk and the lockstep ensemble), n_slots 1 .. 128: each slot's diagonal by
 *     launch_jac_diag; launch_drift_test once with the pinned host target and once without (the ensemble's form: results at a
 *     member's offset of a larger buffer, copied afterwards); then drop_drifted. jd[n_slots][N]: the saved diagonals;
 *     drift[2][n_slots]: the results of the two forms; out_i[n_slots]: the slots' valid flags afterwards; info[0]: the number
 *     drop_drifted dropped, info[1]: the number of slots launch_drift_test tested, info[2]: the number dropped on the second
 *     form's results, info[6]: 1 when nothing outside the slots' results was written.
 *   path 1 (the resident kernel, its diagnostic build), n_slots 1 .. 64: slot s by ph_factor(s, c_fact[s], keep_diag) on
 *     jv_slots[s], then today's values and DevBackend::drift_check(max_drift) by wavefront 0 with ph_drift on all eight.
 *     jd as above; drift[n_slots]: the kernel's per-slot results (-7: ph_drift wrote none); out_i[n_slots]: the slot table's
 *     valid flags afterwards; info[0] (= info[2]): drift_check's return value; info[1] = n_slots.
 * mode KIN_CACHE_RULES (path 1 only): the slot table valid[n_slots], c_fact[n_slots], stamps[3][n_slots] = jac_stamp, step_stamp,
 *   last_use (n_slots 0 .. 64; the kernel's other slots are unused), and n_queries queries qd[q][2] = c, band;
 *   qi[q][5] = n_restarts, max_age, n_steps, step_age (-1: off), the launch's slot count (0 .. 64). out_i[q][2] =
 *   DevBackend::nearest_slot and DevBackend::victim_slot as the controller calls them.
 * info has 8 entries; path 1 also returns the dense block size, the sparse rows and the dynamic LDS bytes in info[3 .. 5].
 * KIN_ERR_INVALID_ARG: path, mode, n_slots, n_queries or a query's slot count out of range, a null buffer;
 * KIN_ERR_UNSUPPORTED: path 1 on a network the resident kernel does not take. Needs no rate constants; a later solve on the handle
 * is that of a fresh handle. Added under KIN_ABI_VERSION 6: look the symbol up before calling it. */
enum { KIN_CACHE_DRIFT = 0, KIN_CACHE_RULES = 1 };
int kin_cache_probe(kin_network* h, int32_t path, int32_t mode, int64_t n_slots, const double* jv_slots, const double* c_fact,
                    const int32_t* valid, const double* jv_now, double max_drift, const int64_t* stamps, int64_t n_queries,
                    const double* qd, const int64_t* qi, double* jd, double* drift, int32_t* out_i, int64_t* info);

/* ---- segmented flux pass and the analysis of a stored ensemble --------------------------------------------------- */
/* The flux pass over S SEGMENTS of up to L states each (an ensemble's members, the chunks of a long trajectory): state
 * b = s L + j at u[b][N], flux[s][r] = sum over j < seg_n[s] of w[b] rate_r(u_b; k of state b), rate_r as in kin_flux_batched,
 * in the caller's reaction order. ONE launch: a workgroup owns (segment, part of the reactions), walks the segment's rows in
 * order and writes flux[s][.] itself - a segment's result depends on its own rows only: it is bit-identical whatever other
 * segments the call holds and whatever S is, and repeats bit for bit. Rows j >= seg_n[s] are never read (their u, k_row, T and
 * w entries need not be valid); seg_n == NULL: every segment has L rows; seg_n[s] == 0 gives zeros. Rate constants of state b,
 * exactly the rules of kin_flux_batched_dev: row k_row[b] of k (k_row NULL: row b), or the Arrhenius law at T[b], or the
 * handle's current rates. A lane keeps its rate constants in registers from row to row of a segment and loads / evaluates
 * them again only when k_row[b] (the bits of T[b]) differs from the previous row's - the same function of the same inputs:
 * no bit changes. Statuses as kin_flux_batched: KIN_ERR_INVALID_ARG for both k and T, k_row without k, S or L < 0, a null
 * output (host entry: a k_row of a row j < seg_n[s] outside [0, n_k_rows), a seg_n outside [0, L], k without k_row and
 * n_k_rows != S L); KIN_ERR_STATE for T without Arrhenius parameters or no rates at all; S L = 0 or R = 0 writes zeros.
 * The device entry only enqueues (d_seg_n: S int64 on the device, or NULL); one stream per handle at a time, as for the
 * per-state pass. Added under KIN_ABI_VERSION 6: look the symbols up. */
int kin_flux_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u,
                           const double* d_k, const int64_t* d_k_row, const double* d_T, const double* d_w,
                           double* d_flux /* [S][R] */, void* stream);
int kin_flux_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* k,
                       int64_t n_k_rows, const int64_t* k_row, const double* T, const double* w, double* flux /* [S][R] */);
/* After a successful kin_solve_ensemble* call the handle remembers where the members' saved states live on the device,
 * [K][n_rows][N] with zeros past n_saved[m] - whether or not out_u was given (out_u == NULL with n_saved != NULL is a
 * solve that downloads no trajectory). The next ensemble call on the handle replaces the record; a failed one leaves
 * none; kin_solve and the other entries leave it alone. Without a stored ensemble the four calls return KIN_ERR_STATE. */
int kin_ensemble_size(const kin_network* h, int64_t* K, int64_t* n_rows, int64_t* n_species, int64_t* n_saved /* [K] or NULL */);
/* out_umax[m][i] = max over member m's saved rows of species i (kin_solution_max per member; the zero rows past n_saved take no
 * part; a member without saved rows gives zeros). One launch. */
int kin_ensemble_max(kin_network* h, double* out_umax /* [K][N] */);
/* out[m][j] = sum_i w[i] u_m(t_j)[i] for j < n_saved[m], zeros beyond (kin_solution_dot per member). One launch. */
int kin_ensemble_dot(kin_network* h, const double* w /* [N] */, double* out /* [K][n_rows] */);
/* kin_flux_segmented over the stored ensemble (S = K, L = n_rows, seg_n = n_saved), read where it lives: flux[m][R] of every
 * member. w, k_row and T_rows have one entry per (member, row of the save grid); entries of rows j >= n_saved[m] are ignored.
 * k without k_row needs n_k_rows == K n_rows. */
int kin_ensemble_flux(kin_network* h, const double* w /* [K*n_rows] or NULL */, const double* k, int64_t n_k_rows,
                      const int64_t* k_row /* [K*n_rows] */, const double* T_rows /* [K*n_rows] */, double* flux /* [K][R] */);

/* ---- directed relation graph (Lu & Law) of the network over batched states: which species matter for which ------------- */
/* Reaction rates are the flux pass's, q_r = k_r u[x0_r] (x1_r >= 0 ? u[x1_r] : 1). RECORDS group the reactions: with
 * pairing != 0 a record is a reaction kf together with its exact reverse kr as the network compiler pairs them for the
 * batched sweep (reactions in order; a reaction whose operands and products are another, earlier, still unpaired one's
 * products and operands joins the latest such reaction; reactions with a species on both sides stay alone) and progresses
 * at w = q_kf - q_kr; with pairing == 0 every reaction is a record, w = q_r. nu_A is the net stoichiometric coefficient of
 * species A in the record's forward reaction, S the species on either side of it (a collider with zero net coefficient
 * belongs to S). For a state b
 *   den_A(b)  = sum over records with nu_A != 0                    of |nu_A| |w(b)|
 *   num_AB(b) = sum over records with nu_A != 0, B in S, B != A    of |nu_A| |w(b)|
 *   r_AB(b)   = num_AB / den_A  (exactly 0.0 where den_A == 0: never NaN or Inf for finite inputs)
 *   coef_AB   = max over the B states of r_AB(b)
 * The EDGES are the pairs (A, B) that have a contribution to num_AB: a CSR over A with sorted columns and no diagonal that
 * depends on the topology and on pairing only (a collider M of A + M -> B + M is the head of edges A -> M and B -> M and the
 * tail of none). coef has one entry per edge, in CSR order. Sums are formed in a fixed order and the maximum is exact: the
 * result is bit-identical from call to call and does not depend on how the states are cut into blocks (a workspace of at
 * most 256 MB of per-state rates; KIN_DRG_BLOCK_STATES=n forces blocks of at most n states). accumulate != 0: the current
 * contents of coef take part in the maximum (several solves or conditions folded into one graph). Rate constants and
 * statuses are exactly kin_flux_batched[_dev]'s; B == 0 writes zeros, or leaves coef alone when accumulating.
 * KIN_ERR_UNSUPPORTED for pairing != 0 on a network without pair records (n_species >= 65535).
 * Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* Pattern and plan sizes without a device or a handle. rowptr[n_species + 1] / colidx[edges], both may be NULL (sizes only).
 * info[9]: edges, denominator contributions, edge contributions, then the rows of the denominator plan with <= 8, 9 .. 256 and
 * > 256 contributions and the edges of the edge plan in the same three classes. */
int kin_drg_pattern_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                         const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                         int index_base, int pairing, int64_t* info, int64_t* rowptr, int64_t* colidx);
/* The handle's pattern (built at the first call per pairing mode; no device call). Any of nnz / rowptr / colidx may be NULL. */
int kin_drg_pattern(kin_network* h, int pairing, int index_base, int64_t* nnz, int64_t* rowptr, int64_t* colidx);
/* Device pointers; only enqueues on `stream` (NULL: the handle's); allocates when the workspace has to grow. */
int kin_drg_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                        const double* d_T, int accumulate, double* d_coef /* [edges] */, void* stream);
int kin_drg_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef /* [edges] */);
/* Over the saved states of the last kin_solve, read where they live (arguments as kin_solution_flux). */
int kin_solution_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef /* [edges] */);
/* Over the stored ensemble, all members and rows at once (arguments as kin_ensemble_flux; the rows past n_saved[m] and their
 * k_row / T_rows entries take no part). */
int kin_ensemble_drg(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row /* [K*n_rows] */,
                     const double* T_rows /* [K*n_rows] */, int accumulate, double* coef /* [edges] */);

/* ---- DRG with error propagation (DRGEP, Pepiot-Desjardins & Pitsch 2008): one importance per species ------------------- */
/* Rates q_r, records, pairing, nu_A and S are exactly those of the "directed relation graph" block above.
 * With pairing, w = q_kf - q_kr; without pairing, w = q_r.
 *
 * For one state:
 *
 *   P_A   = sum over records with nu_A != 0 of max( nu_A w, 0)
 *   C_A   = sum over records with nu_A != 0 of max(-nu_A w, 0)
 *   den_A = max(P_A, C_A)
 *   s_AB  = sum over records with nu_A != 0, B in S, B != A of nu_A w          (signed)
 *   r_AB  = min(1, |s_AB| / den_A), exactly 0.0 where den_A == 0
 *   R_t   = 1 for every target t
 *   R_B   = max over edges (A, B) of fl(R_A * r_AB), iterated to the fixed point (R_B = 0 if unreachable)
 *
 * Over the states, importance_B is the exact maximum over the counted states of R_B.
 *
 * The edge set and its CSR order are those of kin_drg_pattern(pairing); no new pattern is defined.
 *
 * Floating-point multiplication by a number in [0, 1] is monotone.
 * Hence the fixed point is unique: R_B is the maximum over paths of the left-to-right product along the path.
 * It does not depend on relaxation order, on Jacobi versus in-place updates, or on the number of rounds beyond convergence.
 * Given r, R is therefore bit-identical to any correct CPU search doing the same multiplications.
 *
 * The sums of r are formed in the fixed order of the DRG pass; the search runs per state on that state's r, one workgroup
 * per state, at most n_species rounds (rounds counts the last one, which changes nothing). States are taken in blocks as in
 * the DRG pass (no per-state array of a block above 256 MB; KIN_DRG_BLOCK_STATES=n); the result does not depend on the
 * blocks, nor on where the search keeps R (LDS up to 4080 species, else global memory; KIN_DRGEP_LDS_SPECIES=n forces the
 * global form above n species; KIN_DRGEP_STAGES=1 or 2 ends every block after that stage and leaves importance alone - a knob
 * for timing the stages, never for results). accumulate != 0: the current contents of importance take part in the maximum. targets:
 * n_targets >= 1 species ids (index_base as given; the device entry: 0-based int64 on the device, ids outside [0, N) are
 * passed over there), duplicates allowed; a target outside [0, N) or n_targets < 1: KIN_ERR_INVALID_ARG. Rate constants
 * and statuses are exactly kin_flux_batched[_dev]'s and kin_drg_batched's; B == 0 writes zeros, or leaves importance alone
 * when accumulating. For finite inputs every output is finite and in [0, 1], and a target's importance is exactly 1.0
 * whenever at least one state counts. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* Device pointers; only enqueues on `stream` (NULL: the handle's) once the workspace has its size. */
int kin_drgep_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                          const double* d_T, const int64_t* d_targets, int64_t n_targets, int accumulate,
                          double* d_importance /* [N] */, void* stream);
/* Host arrays. The optional outputs show every stage: r_out[b][e] the coefficients, R_out[b][i] the per-state importances,
 * rounds_out[b] the rounds of the search. */
int kin_drgep_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T, const int64_t* targets, int64_t n_targets, int index_base, int accumulate,
                      double* importance /* [N] */, double* r_out /* [B][edges] or NULL */, double* R_out /* [B][N] or NULL */,
                      int32_t* rounds_out /* [B] or NULL */);
/* The path stage alone on the caller's coefficients r[B][edges] (CSR order of kin_drg_pattern(pairing)).
 * KIN_ERR_INVALID_ARG for an r outside [0, 1] or non-finite. */
int kin_drgep_paths(kin_network* h, int pairing, int64_t B, const double* r, const int64_t* targets, int64_t n_targets, int index_base,
                    int accumulate, double* importance /* [N] */, double* R_out /* [B][N] or NULL */, int32_t* rounds_out /* [B] or NULL */);
/* Over the saved states of the last kin_solve / over the stored ensemble, read where they live: arguments and statuses of
 * kin_solution_drg / kin_ensemble_drg, plus the targets. Rows past n_saved[m] take no part. */
int kin_solution_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                       const int64_t* targets, int64_t n_targets, int index_base, int accumulate, double* importance /* [N] */);
int kin_ensemble_drgep(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row /* [K*n_rows] */,
                       const double* T_rows /* [K*n_rows] */, const int64_t* targets, int64_t n_targets, int index_base, int accumulate,
                       double* importance /* [N] */);

/* ---- reaction elimination (Lu & Law 2008): one importance index per reaction -------------------------------------------- */
/* Rates q_r, records, pairing, nu_A and den_A are exactly those of the "directed relation graph" block above: with pairing a
 * record is a reaction with its exact reverse and w = q_kf - q_kr, without pairing every reaction is a record and w = q_r;
 * den_A = sum over records with nu_A != 0 of |nu_A| |w|.
 *
 * For one state b and a record rho:
 *
 *   I_rho(b)      = max over species A with nu_A(rho) != 0 and A selected of  fl(fl(|nu_A| * |w(b)|) / den_A(b))
 *                   (a species with den_A == 0 contributes exactly 0.0; no selected species with nu != 0: 0.0)
 *   importance[r] = max over the counted states of I_rho(b),  for every reaction r of record rho
 *
 * The output has one entry per REACTION, in the caller's reaction order; the two reactions of a pair record carry the same
 * bits. The species reduction passes above say which species to keep; this one says which reactions among the survivors
 * carry a share >= eps of the turnover of at least one species the caller cares about.
 *
 * "Selected" means every species when no list is given (species == NULL), else the listed ids - the convention of DRGEP's
 * targets: index_base as given on the host entries, 0-based int64 on the device; ids outside [0, N) are KIN_ERR_INVALID_ARG
 * on the host and passed over on the device; duplicates allowed; a non-null list with n_sel < 1: KIN_ERR_INVALID_ARG. The
 * denominators are always those of the WHOLE network: the list only restricts which species a reaction is judged by. A
 * collider with zero net coefficient never counts.
 *
 * Every floating-point sum of non-negative terms is monotone, so den_A >= fl(|nu_A| |w|) whatever order the denominator pass
 * uses: for finite inputs every output is finite and in [0, 1], and a record that is a selected species' only record gets
 * exactly 1.0 whenever its |w| > 0 in at least one counted state. The maximum over the states is exact, there are no
 * atomics, and the result is bit-identical from call to call and independent of how the states are cut into blocks (the
 * workspace of at most 256 MB of per-state rates and KIN_DRG_BLOCK_STATES=n of the DRG pass). accumulate != 0: the current
 * contents of importance take part in the maximum. B == 0 writes zeros, or leaves importance alone when accumulating. Rate
 * constants and statuses are exactly kin_flux_batched[_dev]'s and kin_drg_batched's, KIN_ERR_UNSUPPORTED for pairing != 0 on a
 * network without pair records included. The pass has no size limit beyond the DRG pass's and builds no edge plan.
 * Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* The per-reaction table the kernel reads, without a device or a handle; any output may be NULL. The outputs are 0-based whatever
 * index_base the network was given in. partner[r]: the other reaction of r's pair record or -1; always -1 with pairing == 0.
 * species[4 r + j], nu[4 r + j]: the record's up to four slots - species or -1, signed net coefficient (0 beside -1) - taken
 * from the record's forward reaction, the sign flipped for the reverse member. info[3]: records, reactions that have a partner,
 * reactions without any non-zero slot (their importance is always 0.0). */
int kin_reaction_importance_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                                      const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                                      int index_base, int pairing, int64_t* info /* [3] */, int64_t* partner /* [R] or NULL */,
                                      int64_t* species /* [4R] or NULL */, int64_t* nu /* [4R] or NULL */);
/* Device pointers; only enqueues on `stream` (NULL: the handle's) once the workspace has its size. */
int kin_reaction_importance_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                                        const double* d_T, const int64_t* d_species /* [n_sel] or NULL */, int64_t n_sel, int accumulate,
                                        double* d_importance /* [R] */, void* stream);
/* Host arrays. per_state[b][r] = I_rho(b) of every state, for tests that check more than the maximum. */
int kin_reaction_importance_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows,
                                    const int64_t* k_row, const double* T, const int64_t* species /* [n_sel] or NULL */, int64_t n_sel,
                                    int index_base, int accumulate, double* importance /* [R] */, double* per_state /* [B][R] or NULL */);
/* Over the saved states of the last kin_solve / over the stored ensemble, read where they live: arguments and statuses of
 * kin_solution_drg / kin_ensemble_drg, plus the species list. Rows past n_saved[m] take no part. */
int kin_solution_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row,
                                     const double* T_rows, const int64_t* species, int64_t n_sel, int index_base, int accumulate,
                                     double* importance /* [R] */);
int kin_ensemble_reaction_importance(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row /* [K*n_rows] */,
                                     const double* T_rows /* [K*n_rows] */, const int64_t* species, int64_t n_sel, int index_base,
                                     int accumulate, double* importance /* [R] */);

/* ---- path flux analysis (PFA, Sun, Chen, Gou & Ju 2010): second-generation species coupling --------------------------- */
/* The rates q, the records, pairing, the signed nu_A and the set S are exactly those of the "directed relation graph" block
 * above. Per state, with w = q_kf - q_kr (pairing) or q_r:
 *
 *   P_A  = sum of max( nu_A w, 0)            C_A  = sum of max(-nu_A w, 0)      over the records with nu_A != 0
 *   P_AB = the part of P_A whose records hold B (B in S, B != A)                C_AB likewise
 *   den_A = max(P_A, C_A)
 *   rp_AB = P_AB / den_A        rc_AB = C_AB / den_A        (0.0 where den_A == 0, never NaN)
 *   rp2_AB = sum over M not in {A, B} with (A, M) and (M, B) in E of rp_AM * rp_MB         rc2_AB likewise with rc
 *   r_AB  = rp_AB + rc_AB + rp2_AB + rc2_AB           coef_AB = max over the states of r_AB
 *
 * E is the DRG pattern of that pairing mode (kin_drg_pattern). The PFA pattern E2 holds (A, B), A != B, when (A, B) is in E
 * or some M not in {A, B} has (A, M) in E and (M, B) in E; it is stored as CSR with sorted columns and no diagonal, and coef
 * has one entry per pair of E2 in that order. r is not clipped: a reversible pair without pairing gives 1.5. Production and
 * consumption never mix: rp_AM * rc_MB contributes nothing. States past n_saved[m] of a stored ensemble do not count.
 *
 * No floating-point atomics: P_AB and C_AB are formed in the fixed order of the DRG pass, the second-generation sums with M
 * in pattern order, one writer per value, and the maximum is exact. The result is bit-identical from call to call and does
 * not depend on how the states are cut into blocks or slices, on accumulate against one call, or on which rows a workgroup
 * and which a single wavefront takes (the rows whose cost sum over M in out(A) of deg(M) is above 65536, and every row of a
 * network above 2366 species, go to a workgroup; KIN_PFA_WG_COST=n sets the cost instead - a knob for timing, never for results). States are taken in blocks as in the DRG
 * pass: none of rates[nb][R], rp[nb][E] + rc[nb][E] and, when asked for, r[nb][E2] above 256 MB; KIN_DRG_BLOCK_STATES=n forces
 * blocks of at most n states; KIN_PFA_STAGES=1 or 2 ends every block after the rates or after the split stage and leaves
 * coef alone - for timing the stages. accumulate != 0: the current contents of coef take part in the maximum. Rate
 * constants and statuses are exactly kin_flux_batched[_dev]'s and kin_drg_batched's; B == 0 writes zeros, or leaves coef
 * alone when accumulating. Size limit: the second-generation stage keeps one row of n_species doubles in LDS, which fits the
 * 160 KB of a compute unit up to 20286 species; above that every entry but the two pattern ones returns KIN_ERR_UNSUPPORTED
 * and kin_last_error names the limit. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* E2 and its sizes from the topology alone, no device or handle. rowptr[n_species + 1] / colidx[pairs], both may be NULL
 * (sizes only). info[4]: the edges of E, the pairs of E2, the products per state (sum over the edges (A, M) of M's out-degree:
 * each is two multiply-adds) and the largest row of E. */
int kin_pfa_pattern_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                         const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                         int index_base, int pairing, int64_t* info /* [4] */, int64_t* rowptr, int64_t* colidx);
/* The handle's E2 (built at the first call per pairing mode; no device call). Any of nnz / rowptr / colidx may be NULL. */
int kin_pfa_pattern(kin_network* h, int pairing, int index_base, int64_t* nnz, int64_t* rowptr, int64_t* colidx);
/* Device pointers; only enqueues on `stream` (NULL: the handle's) once the workspace has its size. */
int kin_pfa_batched_dev(kin_network* h, int pairing, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row,
                        const double* d_T, int accumulate, double* d_coef /* [pairs] */, void* stream);
/* Host arrays. The optional outputs show every stage per state: rp_out[b][e] and rc_out[b][e] over the edges of E, r_out[b][z]
 * over the pairs of E2. */
int kin_pfa_batched(kin_network* h, int pairing, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                    const double* T, int accumulate, double* coef /* [pairs] */, double* rp_out /* [B][edges] or NULL */,
                    double* rc_out /* [B][edges] or NULL */, double* r_out /* [B][pairs] or NULL */);
/* The second-generation stage alone on the caller's coefficients rp[B][edges], rc[B][edges] (CSR order of
 * kin_drg_pattern(pairing)). KIN_ERR_INVALID_ARG for a coefficient that is negative or not finite. */
int kin_pfa_paths(kin_network* h, int pairing, int64_t B, const double* rp, const double* rc, int accumulate,
                  double* coef /* [pairs] */, double* r_out /* [B][pairs] or NULL */);
/* Over the saved states of the last kin_solve / over the stored ensemble, read where they live: arguments and statuses of
 * kin_solution_drg / kin_ensemble_drg. Rows past n_saved[m] take no part. */
int kin_solution_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                     int accumulate, double* coef /* [pairs] */);
int kin_ensemble_pfa(kin_network* h, int pairing, const double* k, int64_t n_k_rows, const int64_t* k_row /* [K*n_rows] */,
                     const double* T_rows /* [K*n_rows] */, int accumulate, double* coef /* [pairs] */);

/* ---- timescale analysis: batched Jacobians, species lifetimes, quasi-steady-state error --------------------------------- */
/* For a state u_b with rate constants k_b, chosen exactly as kin_flux_batched[_dev] chooses them (rows of k, the Arrhenius
 * law at T[b], or the handle's current rates):
 *   q_r, dq_r/du   the mass-action rate and its operand derivatives: 2A has ONE operand column with 2 k u, a collider is an
 *                  ordinary operand
 *   f_i  = sum_r nu_ir q_r                          (the right-hand side)
 *   J_ij                                            the CSR pattern of kin_jac_pattern (sorted columns, diagonal always present)
 *   d_i  = J_ii
 *   g_i  = sum_j |J_ij|                             over the stored entries of row i, diagonal included
 *   norm(b) = max_i g_i = ||J(u_b)||_inf            (bounds the spectral radius: the stiffness along a run)
 *   e_i(b)  = |f_i| / |d_i|                         the instantaneous quasi-steady-state error (Turanyi, Tomlin & Pilling 1993):
 *             exactly 0.0 where f_i == 0 (0/0 included), +Inf where d_i == 0 and f_i != 0 (a species nothing consumes is
 *             never quasi-steady); never NaN for finite inputs
 * and over the states that count, summary[3][N]:
 *   row 0: decay_max_i = max_b (-d_i)     (1 / decay_max: the shortest lifetime tau_i = -1 / J_ii, Turanyi & Tomlin)
 *   row 1: decay_min_i = min_b (-d_i)
 *   row 2: qss_err_i   = max_b e_i(b)
 * Maxima and minima are exact. With no counting state and accumulate == 0 the rows hold the identities -Inf, +Inf, 0.0;
 * accumulate != 0: the current contents of summary take part (several solves folded into one summary, as in kin_drg_*).
 * Every sum is formed in a fixed order and there are no atomics: results are bit-identical from call to call and do not
 * depend on how the states are cut into blocks or slices (a per-state workspace of at most 256 MB per block;
 * KIN_TS_BLOCK_STATES=n forces blocks of at most n states; KIN_TS_STAGES=1 or 2 ends every block after the rates or after
 * the Jacobian entries and leaves the outputs behind that stage alone - a knob for timing the stages, never for results).
 * At least one output must be requested; statuses and argument
 * checks are those of kin_flux_batched[_dev] / kin_drg_*. B == 0 writes the identities, or leaves summary alone when
 * accumulating. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
/* The Jacobian values of B states, vals[b][nnz] in the CSR order of kin_jac_pattern (kin_jac_values for many states, each
 * with its own rate constants). Device pointers: only enqueues on `stream` (NULL: the handle's) once the workspace has its
 * size; one stream per handle at a time. */
int kin_jac_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                        double* d_vals /* [B][nnz] */, void* stream);
int kin_jac_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T,
                    double* vals /* [B][nnz] */);
/* summary[3][N], diag[b][i] = d_i(b), err[b][i] = e_i(b), norm[b]: any of them may be NULL, not all. */
int kin_timescale_batched_dev(kin_network* h, int64_t B, const double* d_u, const double* d_k, const int64_t* d_k_row, const double* d_T,
                              int accumulate, double* d_summary /* [3][N] or NULL */, double* d_diag /* [B][N] or NULL */,
                              double* d_err /* [B][N] or NULL */, double* d_norm /* [B] or NULL */, void* stream);
int kin_timescale_batched(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T, int accumulate, double* summary /* [3][N] or NULL */, double* diag /* [B][N] or NULL */,
                          double* err /* [B][N] or NULL */, double* norm /* [B] or NULL */);
/* Over the saved states of the last kin_solve / over the stored ensemble, read where they live (arguments and statuses of
 * kin_solution_drg / kin_ensemble_drg). row_begin leaves out the induction period: saved rows with an index below it take no
 * part (in an ensemble: of every member), nor do the rows past n_saved[m]; the norm entries of rows that take no part are
 * written as 0.0. row_begin < 0: KIN_ERR_INVALID_ARG. */
int kin_solution_timescale(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                           int64_t row_begin, int accumulate, double* summary /* [3][N] or NULL */, double* norm /* [n_saved] or NULL */);
int kin_ensemble_timescale(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row /* [K*n_rows] */,
                           const double* T_rows /* [K*n_rows] */, int64_t row_begin, int accumulate, double* summary /* [3][N] or NULL */,
                           double* norm /* [K*n_rows] or NULL */);
/* Plan sizes without a device or a handle. info[4]: the stored entries of J, then the rows of J with <= 8, 9 .. 256 and > 256
 * stored entries: the three classes of the row pass (a lane, a wavefront, a workgroup per row). */
int kin_timescale_plan_host(int64_t n_species, int64_t n_reactions, const int64_t* reac_ptr, const int64_t* reac_idx,
                            const int64_t* reac_sto, const int64_t* prod_ptr, const int64_t* prod_idx, const int64_t* prod_sto,
                            int index_base, int64_t* info /* [4] */);

/* ---- cross-member statistics of an ensemble: moments, quantiles, correlations with the sampled inputs --------------------- */
/* The passes above reduce along a member's rows. These reduce ACROSS the members of a block of states u[K][L][N] (member, row
 * of the save grid, species: the stored ensemble's layout) - what a Monte-Carlo run over uncertain rate parameters, a sweep
 * of heating rates or a set of start compositions is made for: mean and spread of every species at every saved time, the
 * 5 / 50 / 95 % envelope, and which sampled input drives which species (Pearson and Spearman correlation: the sampling-based
 * global sensitivity).
 *
 * PARTICIPANTS. use[K] is int32; member m takes part iff use[m] != 0; the n participants are the same for every row and
 * species and are always visited in member order. use == NULL: all K members (kin_members_*), the members that completed
 * the save grid, n_saved[m] == n_rows (kin_ensemble_*). Over the stored ensemble use[m] != 0 for a member with
 * n_saved[m] < n_rows is KIN_ERR_INVALID_ARG: rows past n_saved are never read, as in the other ensemble entries.
 *
 * MOMENTS per (row j, species i) over the participants' x = u[m][j][i]:
 *   count = n;  mean = sum x / n;  var = sum (x - mean)^2 / (n - 1) (two passes, unbiased; exactly 0.0 for n == 1);  min and
 *   max exact. n == 0 writes zeros everywhere.
 * QUANTILES for probabilities p[Q] in [0, 1] (anything else, NaN included: KIN_ERR_INVALID_ARG) over the sorted participant
 * values x[0..n):  h = (n - 1) p, lo = floor(h), g = h - lo;  the value is x[lo] when g == 0, else x[lo] + (x[lo+1] - x[lo]) g
 * with a separately rounded multiply and add (no fused multiply-add) - numpy.quantile's "linear" method up to the form of the
 * interpolation. n == 0 gives 0.0.
 * RANKS are 1-based, ties get the average rank (multiples of 0.5: exact); -0.0 and +0.0 tie.
 * CORRELATION with the inputs X[K][P] (one row per member: a log-multiplier of a rate constant, a temperature, a heating rate,
 * a u0 entry ...), for every row j, selected species i and input p, over the participants' y = u[m][j][i] and x = X[m][p]:
 *   r = sum (x - xbar)(y - ybar) / sqrt(sum (x - xbar)^2 sum (y - ybar)^2)
 * rank != 0: both sides are replaced by their ranks among the participants (Spearman's coefficient). r is exactly 0.0 where
 * either sum of squares is 0 or n < 2, never NaN or Inf for finite inputs (sums of squares that under- or overflow the double
 * range count as 0 / Inf: value correlations of subnormal columns come out 0.0; rank correlations have no such limit).
 * NON-FINITE VALUES: a NaN among the participating values of a (row, species) makes every statistic of that (row, species)
 * NaN; +-Inf sort as the extremes they are and otherwise follow IEEE arithmetic (a mean of Inf, a NaN variance).
 *
 * How it is computed, and the order of every sum (member_stats.hpp): the moments in one launch, lanes along the species, the
 * participants split over the eight wavefronts of a workgroup (wave w adds q = w, w + 8, ... in order, the eight partial sums
 * are added in the order of w). The selected columns (j, i) are gathered tile by tile into LDS and sorted there; quantiles
 * come from the sorted column, ranks from two binary searches in it. A correlation is out[j][i][p] = sum over the
 * participants, in order, of Xhat[q][p] Yhat[(j, i)][q], with Xhat = (x - xbar) / sqrt(sum (x - xbar)^2) (or the same of the
 * ranks) from kin_members_inputs_host and Yhat the same of y, written by the column pass to a workspace of at most 256 MB;
 * larger requests are cut into blocks of columns (KIN_MEMBERS_BLOCK_COLUMNS=n forces blocks of at most n columns). Every
 * statistic is a function of its own column with one fixed order of operations: results are bit-identical from call to
 * call, between a kin_ensemble_* entry and the kin_members_* entry fed the downloaded states, and under any blocking.
 * The sorted passes (quantiles, rank correlation) take at most KIN_MEMBERS_MAX_SORTED participants (KIN_ERR_UNSUPPORTED
 * beyond, with the limit in the message); moments and value correlations have no limit on K.
 *
 * species[n_sel]: the selected species in the index base the handle was created with (kin_network_create's index_base);
 * NULL: all N (n_sel is ignored). Statuses: KIN_ERR_INVALID_ARG for K, L, n_sel, Q or P < 0, a species outside the network,
 * a null u with K L > 0, a null output (moments: every output null), a null p with Q > 0 or X with P > 0;
 * KIN_ERR_STATE from the kin_ensemble_* entries without a stored ensemble. In the _dev entries u and the outputs are device
 * pointers and the call only enqueues on `stream` (NULL: the handle's) once the workspace has its size; use, species, p, X
 * and count are HOST pointers, read (count: written) before the call returns. One stream per handle at a time. Added under
 * KIN_ABI_VERSION 6: look the symbols up before calling them. */
#define KIN_MEMBERS_MAX_SORTED 4096
/* The inputs' side of a correlation, on the host (no handle, no device): *n = the participants, Xhat[q][p] for the q-th
 * participant in member order = (x - xbar) / sqrt(sum (x - xbar)^2) of input p over the participants, x replaced by its
 * average-tie rank when rank != 0; a column whose sum of squares is 0, and any column for n < 2, gives zeros; a column
 * holding a NaN gives NaNs. Sums are carried in extended precision: the values are within a few ulp of the exact ones.
 * Xhat may be NULL (only *n is wanted); K or P < 0, a null X with K P > 0: KIN_ERR_INVALID_ARG. */
int kin_members_inputs_host(int64_t K, int64_t P, const double* X /* [K][P] */, const int32_t* use /* [K] or NULL */, int rank,
                            int64_t* n, double* Xhat /* [n][P] (at most [K][P]) or NULL */);
int kin_members_moments(kin_network* h, int64_t K, int64_t L, const double* u /* [K][L][N] */, const int32_t* use, int64_t* count,
                        double* mean, double* var, double* min, double* max /* [L][N] each; any may be NULL, not all five */);
int kin_members_moments_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, int64_t* count, double* d_mean,
                            double* d_var, double* d_min, double* d_max, void* stream);
int kin_members_quantiles(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, const int64_t* species,
                          int64_t n_sel, const double* p /* [Q] */, int64_t Q, double* out /* [Q][L][n_sel] */);
int kin_members_quantiles_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, const int64_t* species,
                              int64_t n_sel, const double* p, int64_t Q, double* d_out, void* stream);
int kin_members_correlate(kin_network* h, int64_t K, int64_t L, const double* u, const int32_t* use, const int64_t* species,
                          int64_t n_sel, const double* X /* [K][P] */, int64_t P, int rank, double* out /* [L][n_sel][P] */);
int kin_members_correlate_dev(kin_network* h, int64_t K, int64_t L, const double* d_u, const int32_t* use, const int64_t* species,
                              int64_t n_sel, const double* X, int64_t P, int rank, double* d_out, void* stream);
/* The same over the stored ensemble, read where it lives (K, L = n_rows of kin_ensemble_size); host outputs. */
int kin_ensemble_moments(kin_network* h, const int32_t* use, int64_t* count, double* mean, double* var, double* min, double* max);
int kin_ensemble_quantiles(kin_network* h, const int32_t* use, const int64_t* species, int64_t n_sel, const double* p, int64_t Q,
                           double* out /* [Q][n_rows][n_sel] */);
int kin_ensemble_correlate(kin_network* h, const int32_t* use, const int64_t* species, int64_t n_sel, const double* X /* [K][P] */,
                           int64_t P, int rank, double* out /* [n_rows][n_sel][P] */);

/* ---- Sobol sensitivity indices across the members of a Saltelli design ------------------------------------------------------ */
/* A correlation measures monotone, additive influence. The variance-based indices answer what a Monte-Carlo run over uncertain
 * inputs is set up for: how much of the variance of species i at time t does input p carry alone (first order, S1) and with
 * its interactions (total effect, ST).
 *
 * DESIGN LAYOUT. K = M (P + 2) members, M >= 1 base samples, P >= 1 inputs. Member b M + m is sample m of block b: block 0 is
 * A, block 1 is B, block 2 + p is AB_p - A with input p taken from B. For one column (row j, species i) a_m, b_m and c_pm are
 * the values of sample m in A, B and AB_p.
 *
 * WEIGHTS. w[M] is int32: values >= 0 are multiplicities - 0: the sample takes no part, above 1: a bootstrap replicate; a
 * negative entry is KIN_ERR_INVALID_ARG. w == NULL: all ones (kin_members_sobol*); over the stored ensemble 1 where all P + 2
 * members of sample m completed the save grid (n_saved == n_rows), else 0, and w[m] != 0 for a sample with an incomplete
 * member is KIN_ERR_INVALID_ARG (rows past n_saved are never read). The participants are the samples with w > 0, always
 * visited in ascending m; n = sum w.
 *
 * QUANTITIES per column, sums over the participants:
 *   mu   = (sum w a + sum w b) / (2 n)
 *   V    = (sum w (a - mu)^2 + sum w (b - mu)^2) / (2 n)      the population variance over A u B (Saltelli et al. 2010)
 *   S1_p = (sum w (b - mu)(c_p - a) / n) / V                  (Saltelli et al. 2010)
 *   ST_p = (sum w (a - c_p)^2 / (2 n)) / V                    (Jansen 1999)
 * EDGE RULES. n < 2 or V == 0 gives exactly 0.0 for S1 and ST; V is exactly 0.0 for a column whose participating a and b are
 * all equal (whatever the sum of n equal values rounds to). n == 0 writes zeros everywhere, mu and V included. Otherwise IEEE
 * arithmetic: a NaN in a participating a or b makes the column's mu, V and every S1_p, ST_p NaN (n >= 2), a NaN in c_p that
 * p's two values (V != 0); never NaN or Inf for finite inputs with V > 0 short of overflow. Squares that
 * underflow the double range count as 0, as for the correlations: a column of values near 1e-160 or below has V == 0.
 *
 * How it is computed, and the order of every sum (member_stats.hpp): one launch, lanes along the species, the participants
 * split over the eight wavefronts of a workgroup (wave w adds q = w, w + 8, ... in order, the partials are added in the order
 * of w); mu first, then the centred sums by fused multiply-add; the weight enters as one multiplication, exact for w = 1; P is
 * taken eight inputs per workgroup. Results are bit-identical from call to call, between kin_ensemble_sobol and
 * kin_members_sobol fed the downloaded states, and a 0/1 weight vector gives the bits of the call on the block with the
 * dropped samples removed.
 *
 * Outputs S1, ST [L][n_sel][P], mean (mu), var (V) [L][n_sel]; any may be NULL, not all four. species as above. Statuses as
 * kin_members_correlate: KIN_ERR_INVALID_ARG for M or P < 1, L or n_sel < 0, a negative weight, a species outside the
 * network, a null u with L N > 0, every output null, and from kin_ensemble_sobol a stored K != M (P + 2);
 * KIN_ERR_UNSUPPORTED for M (P + 2) >= 2^31; KIN_ERR_STATE from kin_ensemble_sobol without a stored ensemble. In the _dev
 * entry u and the outputs are device pointers and the call only enqueues on `stream`; w and species are HOST pointers read
 * before it returns. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
int kin_members_sobol(kin_network* h, int64_t M, int64_t P, int64_t L, const double* u /* [M (P + 2)][L][N] */,
                      const int32_t* w /* [M] or NULL */, const int64_t* species, int64_t n_sel, double* S1, double* ST,
                      double* mean, double* var);
int kin_members_sobol_dev(kin_network* h, int64_t M, int64_t P, int64_t L, const double* d_u, const int32_t* w, const int64_t* species,
                          int64_t n_sel, double* d_S1, double* d_ST, double* d_mean, double* d_var, void* stream);
int kin_ensemble_sobol(kin_network* h, int64_t M, int64_t P, const int32_t* w, const int64_t* species, int64_t n_sel, double* S1,
                       double* ST, double* mean, double* var /* L = n_rows */);

/* ---- event times: per-species peak and level-crossing times of stored trajectories ---------------------------------------- */
/* The questions asked of a kinetics run are timing questions - when does an intermediate peak, how long is the induction
 * period before a product reaches 10 % of its final value, what is the half-life of the feed, how wide is a radical's pulse at
 * half of its maximum - and over an ensemble their spread. This pass answers them where the states live.
 *
 * SEGMENTS. A segment s is a member of an ensemble, or the one trajectory of kin_solve: rows j = row_begin .. n_s - 1 of its
 * block of L rows, states u[s][j][i], times t[j] (t[L] shared by all segments, or t[S][L] with t_per_segment != 0). With
 * row_begin >= n_s the segment is empty. Rows at or past n_s are never read, neither their states nor their times.
 *
 * For every segment and species i:
 *   u_peak[s][i]   the maximum over the segment's rows: seg_max's fmax chain, so with row_begin == 0 it equals kin_ensemble_max /
 *                  kin_solution_max bit for bit. An empty segment gives 0.0.
 *   t_peak[s][i]   t[j*], j* the first row that holds the peak. An empty segment gives `never`.
 *   t_cross[s][i]  the time at which the species first crosses the level l:
 *                    level_kind KIN_LEVEL_ABS       l = level[i]
 *                               KIN_LEVEL_OF_PEAK   l = level[i] * u_peak[s][i]
 *                               KIN_LEVEL_OF_START  l = level[i] * u[s][row_begin][i]      (one multiplication, rounded once)
 *                  The search starts at row j0 = row_begin (start KIN_FROM_BEGIN) or j0 = j* (KIN_FROM_PEAK). jc is the first row
 *                  j >= j0 with u[j] >= l (direction > 0, rising) or u[j] <= l (direction < 0, falling). No such row: `never`.
 *                  jc == j0: t[j0]. Otherwise, with a = u[jc - 1] and b = u[jc], the chord
 *                    t[jc - 1] + ((l - a) / (b - a)) * (t[jc] - t[jc - 1])
 *                  evaluated in exactly this order in IEEE double arithmetic, every operation rounded on its own: the kernel is
 *                  compiled with floating-point contraction off (#pragma clang fp contract(off) over event_kernels.hip, which
 *                  is what __dsub_rn / __ddiv_rn / __dmul_rn / __dadd_rn would spell operation by operation), so no
 *                  multiplication fuses with an addition. By construction a < l <= b (a > l >= b): b - a is never zero.
 *                  An empty segment gives `never`.
 * `never` is the caller's: NaN marks "no such time"; the last saved time censors instead.
 * A NaN among the rows that take part: u_peak follows fmax (a NaN row is passed over unless every row is NaN); nothing else
 * is specified for that species. Zeros of both signs among the rows that hold the peak: the device's fmax orders them, u_peak
 * is +0.0 if any such row holds +0.0 (whatever the decomposition) and t_peak the time of the first row that holds a zero.
 *
 * Every output is an extremum or a first index, never a sum: the result is exactly defined whatever the decomposition, and is
 * the same bits from call to call, between the host and the device entry, and whatever else the call holds. How it is
 * computed (event_kernels.hip): one launch, no atomics; a workgroup owns (segment, 64 species), lanes along the species, its 4
 * to 16 wavefronts take the parts of the segment's rows in turn and combine by "larger value, then smaller row" (peak) and
 * "smaller row" (crossing); KIN_LEVEL_ABS and KIN_LEVEL_OF_START from KIN_FROM_BEGIN read the states once, a level or start
 * that depends on the peak a second time in the same workgroup. KIN_EVENT_PART_ROWS caps the rows of a part and
 * KIN_EVENT_WAVES sets the wavefronts (read per call; test knobs: results do not depend on them).
 *
 * Outputs [S][N]; any may be NULL, not all three; level may be NULL when t_cross is. Statuses: KIN_ERR_INVALID_ARG for S or
 * L < 0, a null u or t with S L > 0, every output null, t_cross without level, direction == 0, an unknown level_kind or start,
 * row_begin < 0, and from the host entries a seg_n outside [0, L] or a t that is not strictly increasing over the rows read;
 * KIN_ERR_UNSUPPORTED for S or L >= 2^31 or N > 64 * 65535; KIN_ERR_STATE from kin_ensemble_events / kin_solution_events without
 * a stored ensemble / solution. S L = 0 writes the empty-segment values; N = 0 writes nothing. A refused call leaves the
 * handle as it was. The device entry only enqueues (d_seg_n: S int64 on the device, or NULL: L rows each); one stream per handle
 * at a time. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
enum { KIN_LEVEL_ABS = 0, KIN_LEVEL_OF_PEAK = 1, KIN_LEVEL_OF_START = 2 };
enum { KIN_FROM_BEGIN = 0, KIN_FROM_PEAK = 1 };
int kin_events_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u /* [S][L][N] */,
                             const double* d_t /* [L] or [S][L] */, int t_per_segment, const double* d_level /* [N] */, int level_kind,
                             int direction, int start, int64_t row_begin, double never, double* d_u_peak, double* d_t_peak,
                             double* d_t_cross /* [S][N] each */, void* stream);
int kin_events_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* t, int t_per_segment,
                         const double* level, int level_kind, int direction, int start, int64_t row_begin, double never,
                         double* u_peak, double* t_peak, double* t_cross);
/* kin_events_segmented over the stored ensemble (S = K, L = n_rows, seg_n = n_saved), read where it lives. t: the save grid
 * [n_rows], or with t_per_member != 0 every member's own [K][n_rows] (entries of rows j >= n_saved[m] are ignored). */
int kin_ensemble_events(kin_network* h, const double* t, int t_per_member, const double* level, int level_kind, int direction, int start,
                        int64_t row_begin, double never, double* u_peak, double* t_peak, double* t_cross /* [K][N] each */);
/* The same over the stored states of the last kin_solve (S = 1, L = n_saved) and its saved times. */
int kin_solution_events(kin_network* h, const double* level, int level_kind, int direction, int start, int64_t row_begin, double never,
                        double* u_peak, double* t_peak, double* t_cross /* [N] each */);

/* ---- resampling: stored trajectories on a common axis --------------------------------------------------------------------- */
/* Row j of every member of an ensemble is "the state at time t[j]". Members of a heating-rate or start-temperature sweep sit at
 * different temperatures at one saved time, so a mean, an envelope or a Sobol index "at row j" compares different stages of the
 * programme. This pass evaluates every segment's stored trajectory at query points of an axis of its own - its temperature, a
 * normalised time, the save grid - where the states live; its result can take the place of the stored ensemble, so that every
 * kin_ensemble_* pass runs on rows of equal temperature.
 *
 * SEGMENTS. As in kin_events_segmented: segment s has rows j = row_begin .. n_s - 1 of its block of L rows, states u[s][j][i].
 * AXIS. x[L] shared by all segments, or x[S][L] with x_per_segment != 0: non-decreasing over the rows read (plateaus are allowed:
 *   a ramp that reaches its end value and holds), no NaN. Rows at or past n_s are never read, neither states nor axis.
 * QUERIES. xq[Q] shared, or xq[S][Q] with xq_per_segment != 0; any order, repeats allowed.
 * BRACKET of (s, q). jc is the first row j in [row_begin, n_s) with x[j] >= xq. The query is INSIDE iff the segment is not empty,
 *   xq is not NaN and x[row_begin] <= xq <= x[n_s - 1]. A query that is not inside has the code jc = -1 below the range, -2 above
 *   it, -3 for a NaN query or an empty segment.
 * VALUE of an inside query. x[jc] == xq: u[s][jc][i], copied bit for bit (resampling at a segment's own axis returns its own
 *   rows, -0.0 included; on a plateau the first row that holds the value). Otherwise, with a = u[s][jc - 1][i], b = u[s][jc][i]:
 *     w = (xq - x[jc - 1]) / (x[jc] - x[jc - 1]),      result = a + w * (b - a)
 *   evaluated in exactly this order in IEEE double arithmetic, every operation rounded on its own: the kernel is compiled with
 *   floating-point contraction off (#pragma clang fp contract(off) over resample_kernels.hip, as event_kernels.hip is), so no
 *   multiplication fuses with an addition. x[jc - 1] < xq <= x[jc]: the denominator is never zero. w depends on (s, q) only.
 * OUTSIDE queries. mode KIN_RESAMPLE_FILL: every species gets `fill`, the caller's value (NaN marks "no such state").
 *   KIN_RESAMPLE_HOLD: a query below the range gets row row_begin, one above it row n_s - 1, bit for bit; a NaN query or an
 *   empty segment still gets `fill`. Such a held query counts as COVERED; under KIN_RESAMPLE_FILL covered means inside.
 * OUTPUTS. u_q[S][Q][N]; optionally jc[S][Q] (int32, the codes above whatever the mode) and w[S][Q] (0.0 where the value is a
 *   copy or the query is outside).
 *
 * Every output is a function of its own (s, q, i) with one order of operations: the same bits from call to call, between the
 * host and the device entry, and under any decomposition. How it is computed (resample_kernels.hip): one launch, no atomics; a
 * workgroup owns (segment, a tile of queries, 1024 species); its threads search one query each by bisection and leave (jc, w)
 * in LDS, after one barrier its wavefronts take the tile's queries in turn with the lanes along the species, reading at most
 * two rows and writing one per query. KIN_RESAMPLE_TILE_QUERIES sets the tile (1 .. 256) and KIN_RESAMPLE_WAVES the wavefronts
 * (1 .. 16) (read per call; test knobs: results do not depend on them).
 *
 * Statuses: KIN_ERR_INVALID_ARG for S, L, Q or row_begin < 0, a null u or x with S L > 0, a null xq with S Q > 0, a null output,
 * an unknown mode, and from the host entries a seg_n outside [0, L] or an axis that decreases or holds a NaN over the rows read;
 * KIN_ERR_UNSUPPORTED for S, L or Q >= 2^31, S ceil(Q / 4) >= 2^31 or N > 64 * 65535; KIN_ERR_STATE from kin_ensemble_resample /
 * kin_solution_resample without a stored ensemble / solution. S Q = 0 or N = 0 writes nothing. A refused call leaves the handle
 * as it was. The device entry only enqueues (d_seg_n: S int64 on the device, or NULL: L rows each); one stream per handle at a
 * time. Added under KIN_ABI_VERSION 6: look the symbols up before calling them. */
enum { KIN_RESAMPLE_FILL = 0, KIN_RESAMPLE_HOLD = 1 };
/* The bracket alone, on host arrays: no handle, no device. The normative restatement of (jc, w) above; either output may be
 * NULL, not both. */
int kin_resample_bracket_host(int64_t S, int64_t L, const int64_t* seg_n, const double* x, int x_per_segment, int64_t Q, const double* xq,
                              int xq_per_segment, int64_t row_begin, int32_t* jc /* [S][Q] */, double* w /* [S][Q] */);
int kin_resample_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u /* [S][L][N] */,
                               const double* d_x /* [L] or [S][L] */, int x_per_segment, int64_t Q, const double* d_xq /* [Q] or [S][Q] */,
                               int xq_per_segment, int mode, double fill, int64_t row_begin, double* d_out /* [S][Q][N] */,
                               int32_t* d_jc, double* d_w /* [S][Q] each, or NULL */, void* stream);
int kin_resample_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, const double* x, int x_per_segment,
                           int64_t Q, const double* xq, int xq_per_segment, int mode, double fill, int64_t row_begin, double* out,
                           int32_t* jc, double* w);
/* The same over the stored states of the last kin_solve (S = 1, L = n_saved); x NULL: its saved times. out[Q][N]. */
int kin_solution_resample(kin_network* h, const double* x /* [n_saved] or NULL */, int64_t Q, const double* xq, int mode, double fill,
                          int64_t row_begin, double* out);
/* The same over the stored ensemble (S = K, L = n_rows, seg_n = n_saved), read where it lives; x[n_rows], or x[K][n_rows] with
 * x_per_member != 0 (entries of rows j >= n_saved[m] are ignored). out[K][Q][N] may be NULL when store != 0.
 * With store != 0 THE RESULT BECOMES THE STORED ENSEMBLE (Q >= 1, else KIN_ERR_INVALID_ARG): the block goes to a handle-owned
 * buffer and the record is (K, n_rows = Q, n_saved'), n_saved'[m] the length of the leading run of covered queries of member m -
 * its first uncovered query ends the run, and from that query on the member's rows in the stored block are zeros, the record's
 * invariant, whatever `fill` is (`out` holds the pass's plain result). The per-member Ea / A of a kin_solve_ensemble_*_params
 * record stay attached. Every kin_ensemble_* entry then reads this record unchanged: kin_ensemble_size reports Q rows, and the
 * statistics passes take by default the members that cover the whole query axis. A resampled record may be resampled again
 * (source and destination are two handle buffers used in turn); the next kin_solve_ensemble* call replaces the record as always. */
int kin_ensemble_resample(kin_network* h, const double* x, int x_per_member, int64_t Q, const double* xq, int xq_per_member, int mode,
                          double fill, int64_t row_begin, int store, double* out);

/* ---- observables: weighted species sums and ratios of stored states -------------------------------------------------------- */
/* What a kinetics run is judged by is seldom one species: mole fractions u_i / sum u, lumped product classes, element totals, a
 * selectivity, an ignition delay on a radical pool. This pass reads every stored state once, evaluates H linear forms over the
 * species and G observables built from them, and writes them in the species' place; its result can take the place of the stored
 * ensemble, so that every kin_ensemble_* pass that treats columns as columns runs on observables unchanged. With singleton forms
 * and a compact output it is also the "download only these species" entry.
 *
 * SEGMENTS. As in kin_resample_segmented: segment s has rows j = 0 .. n_s - 1 of its block of L rows, states u[s][j][i], i < N.
 *   Rows at or past n_s are never read. seg_n == NULL: L rows each.
 * FORMS. H >= 0 linear forms in CSR: form_ptr[H + 1] (int64, starts at 0, non-decreasing), form_idx[nnz] (int64 species, in the
 *   index base the handle was created with), form_w[nnz] (double). A species may repeat inside a form; its entries are separate
 *   terms. For one state the terms of form f are t_e = form_w[e] * u[form_idx[e]], each rounded on its own; n is their number.
 *     n == 0: the value is +0.0.
 *     1 <= n <= 64 (short): acc = t_0, then acc = acc + t_e for e = 1 .. n - 1 in entry order. A singleton with weight 1.0 copies
 *       the species, -0.0 included.
 *     n > 64 (long): 64 chains; v[l] is the short rule over the entries e = l, l + 64, l + 128, ... (every chain has at least one
 *       entry). Then for off = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + off] for every l < off. The value is v[0].
 *   The class of a form depends on n only, never on how the launch is shaped.
 * OBSERVABLES. G >= 0 outputs, each a pair (num[g], den[g]) with num[g] in [0, H). den[g] == -1: y_g = F[num[g]], copied bit for
 *   bit. den[g] in [0, H): y_g = F[num[g]] / F[den[g]], one IEEE division; x / 0 and 0 / 0 are what IEEE says.
 * OUTPUT. out[(s L + j) * pitch + c], pitch >= G. Column c < G of a row j < n_s is y_c; every column c >= G is 0.0; every column
 *   of a row j >= n_s is 0.0 (the stored record's invariant). pitch == G is the compact form, pitch == N a block that every
 *   [S][L][N] pass accepts.
 *
 * The kernel and the host restatement are compiled with floating-point contraction off (#pragma clang fp contract(off), as
 * resample_kernels.hip and event_kernels.hip are). Every output is a function of its own (s, j, g) with one order of operations:
 * the same bits from call to call, between kin_observables_host, the host entry and the device entry, and under any tiling. How
 * it is computed (observable_kernels.hip): one launch, no atomics; a 256-thread workgroup owns a few consecutive rows of the flat
 * (s, j) axis and stages them into LDS (a row that does not fit LDS - more than 16 384 species - is gathered from global memory
 * instead: no species limit); a host-built plan, cached in the handle with the forms it was built from, deals short numerators one
 * per lane and long ones one per wavefront, the forms that serve as denominators first, into a table of 64 per row and phase.
 * KIN_OBSERVABLES_ROWS (1 .. 16) sets the rows a workgroup keeps and KIN_OBSERVABLES_LDS=0 forces the gather path (read per call;
 * test knobs: results do not depend on them).
 *
 * Statuses: KIN_ERR_INVALID_ARG for a negative size, a null buffer where data is due (form_ptr with H > 0, form_idx / form_w with
 * entries, num / den with G > 0, states with S L N > 0, the output with S L pitch > 0), a form_ptr that does not start at 0 or
 * decreases, a species outside the network, num outside [0, H), den outside [-1, H), pitch < G, and from the host entries a seg_n
 * outside [0, L]; KIN_ERR_UNSUPPORTED from the entries that launch the kernel for S L >= 2^31 or N, pitch, H, G or nnz >= 2^30;
 * KIN_ERR_STATE from kin_solution_observables / kin_ensemble_observables / kin_ensemble_observable_count without a stored solution
 * / ensemble. S L = 0 or pitch = 0 writes nothing. A refused call leaves the handle as it was. Added under KIN_ABI_VERSION 6: look
 * the symbols up before calling them. */
/* The definition above in plain loops on host arrays: no handle, no device. The normative restatement. */
int kin_observables_host(int64_t N, int index_base, int64_t S, int64_t L, const int64_t* seg_n, const double* u /* [S][L][N] */, int64_t H,
                         const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                         const int64_t* den, int64_t pitch, double* out /* [S][L][pitch] */);
/* States and output on the device; the forms and observables are host arrays, read before the call returns. Only enqueues
 * (d_seg_n: S int64 on the device, or NULL); one stream per handle at a time. */
int kin_observables_segmented_dev(kin_network* h, int64_t S, int64_t L, const int64_t* d_seg_n, const double* d_u /* [S][L][N] */, int64_t H,
                                  const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                                  const int64_t* den, int64_t pitch, double* d_out /* [S][L][pitch] */, void* stream);
int kin_observables_segmented(kin_network* h, int64_t S, int64_t L, const int64_t* seg_n, const double* u, int64_t H,
                              const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G, const int64_t* num,
                              const int64_t* den, int64_t pitch, double* out);
/* The same over the stored states of the last kin_solve (S = 1, L = n_saved). out[n_saved][pitch]. */
int kin_solution_observables(kin_network* h, int64_t H, const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G,
                             const int64_t* num, const int64_t* den, int64_t pitch, double* out);
/* The same over the stored ensemble (S = K, L = n_rows, seg_n = n_saved), read where it lives. out[K][n_rows][pitch] may be NULL
 * when store != 0. With store != 0 THE RESULT BECOMES THE STORED ENSEMBLE, as with kin_ensemble_resample: it needs pitch == N
 * (hence G <= N) and G >= 1, else KIN_ERR_INVALID_ARG; K, n_rows and n_saved are unchanged, the block goes to the one of the two
 * handle buffers of the resampling pass the record is not in, the per-member Ea / A stay attached, and the record is marked as a
 * record of observables (kin_ensemble_observable_count). The passes that treat columns as columns take such a record unchanged -
 * kin_ensemble_size / _max / _dot / _moments / _quantiles / _correlate / _sobol / _events / _resample (with store it keeps the mark)
 * and kin_ensemble_observables itself, whose species then number the observables; the passes that need species and reactions -
 * kin_ensemble_flux / _drg / _drgep / _pfa / _reaction_importance / _timescale - return KIN_ERR_STATE with a message that says
 * so. There is no way back to the states: the next kin_solve_ensemble* call replaces the record as always. */
int kin_ensemble_observables(kin_network* h, int64_t H, const int64_t* form_ptr, const int64_t* form_idx, const double* form_w, int64_t G,
                             const int64_t* num, const int64_t* den, int64_t pitch, int store, double* out);
/* G of a stored record of observables, 0 for a record of states. */
int kin_ensemble_observable_count(const kin_network* h, int64_t* G);

/* ---- device / build information ------------------------------------------------------- */
int kin_device_count(int* n);
/* Selects the device for handles created afterwards by this thread; a handle remembers the device it was created on
 * and every later call on it runs there, whatever the calling thread's current device is. Handles are independent:
 * K handles driven by K host threads may share one GPU (concurrent replicas of an ensemble) or sit on different ones. */
int kin_set_device(int device);
const char* kin_version(void);
/* Layout version of this header's structs and argument lists. A binding compares it (and, if it wants certainty, the
 * struct sizes) with the values it was written against before the first call: kin_params / kin_stats have grown between
 * versions (1: round 1; 2: + dtmin and the LU-cache counters; 3: + the library-order sweep entry points; 4: + kin_solve_ensemble,
 * kin_lu_analyze_host - structs unchanged; 5: + kin_rhs_batched_klib_dev - structs unchanged; 6: + kin_solve_ensemble_continuous -
 * structs unchanged; kin_solve_ensemble_discrete, kin_resident_probe, kin_newton_probe, kin_step_probe, kin_eval_probe, kin_cache_probe, the flux pass (kin_flux_*, kin_solution_flux) and
 * kin_ensemble_size / _max / _dot / _flux and the directed relation graph (kin_drg_*, kin_solution_drg, kin_ensemble_drg) came
 * later under 6, found by symbol lookup; so did DRGEP: kin_drgep_*, kin_solution_drgep, kin_ensemble_drgep, and the timescale analysis:
 * kin_jac_batched*, kin_timescale_*, kin_solution_timescale, kin_ensemble_timescale, and path flux analysis: kin_pfa_*,
 * kin_solution_pfa, kin_ensemble_pfa, and reaction elimination: kin_reaction_importance_*, kin_solution_reaction_importance,
 * kin_ensemble_reaction_importance, and the cross-member statistics: kin_members_*, kin_ensemble_moments / _quantiles /
 * _correlate, and the Sobol indices: kin_members_sobol, kin_members_sobol_dev, kin_ensemble_sobol, and the
 * per-member Arrhenius parameters: kin_solve_ensemble_continuous_params, kin_solve_ensemble_discrete_params, and the event
 * times: kin_events_segmented, kin_events_segmented_dev, kin_ensemble_events, kin_solution_events, and the resampling:
 * kin_resample_bracket_host, kin_resample_segmented, kin_resample_segmented_dev, kin_solution_resample, kin_ensemble_resample, and the observables:
 * kin_observables_host, kin_observables_segmented, kin_observables_segmented_dev, kin_solution_observables,
 * kin_ensemble_observables, kin_ensemble_observable_count). */
#define KIN_ABI_VERSION 6
int kin_abi_version(void);
int64_t kin_struct_size(int which); /* 0: sizeof(kin_params), 1: sizeof(kin_stats), else -1 */

#ifdef __cplusplus
}
#endif
#endif /* KINETICA_HIP_H */
