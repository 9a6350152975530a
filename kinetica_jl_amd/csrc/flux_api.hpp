// What the host side of every analysis pass over a batch of states is written with (flux_api.cpp defines it; the passes:
// flux_api.cpp, drg_api.cpp, drgep_api.cpp, pfa_api.cpp, timescale_api.cpp): where a batch's states and rate constants come
// from - host arrays, the stored solution, the stored ensemble - the block loop over its states, and the staging of a host
// entry's species list and accumulating result. What only the DRG family shares sits in drg_api.hpp.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "handle.hpp"

namespace kin {

// where a call's rate constants come from: rows of k (k_stride doubles apart; 0 = one shared row) or the Arrhenius law at T[b]
struct FluxSource {
  const double* k; int64_t k_stride; const int64_t* k_row; const double* T;
  FluxSource at(int64_t b0) const {      // the source of the states from b0 on
    FluxSource s = *this;
    if (s.k && !s.k_row) s.k += (size_t)b0 * (size_t)s.k_stride;
    if (s.k_row) s.k_row += b0;
    if (s.T) s.T += b0;
    return s;
  }
};

// B states u[B][N] on the device and their rate constants; state b counts only when b % L < seg_n[b / L] (seg_n null: all do)
struct StateBatch { int64_t B; const double* u; FluxSource src; const int64_t* seg_n; int64_t L; };

// The argument and state checks of a pass (have_k: a rate-constant array or the resident table); throws KinError. Every pass
// has one of this shape - flux_check, drg_check, ts_check - and the stored forms below take the caller's.
using PassCheck = void (*)(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out);
void flux_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out);
// flux_check, a null output and the limit on N: the DRG family's check, and what the kin_solution_* / kin_ensemble_* entries
// of the timescale pass have applied from the start
void drg_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out);
void drg_limit(const kin_network* h);   // N below 2^30 (the DRG family's 32-bit offsets)
// every k_row[b] in [0, n_rows); throws KinError
void flux_check_rows(const int64_t* k_row, int64_t B, int64_t n_rows);

// The three ways to a batch, each behind the caller's own check. Host arrays (the *_batched host entries): checked, then
// uploaded into f_u, f_k, f_krow, f_T.
StateBatch host_batch(kin_network* h, int64_t B, const double* u, const double* k, int64_t n_k_rows, const int64_t* k_row,
                      const double* T, hipStream_t s);
// The stored solution h->d_sol_u [n_saved][N] and the stored ensemble h->ens.sol [K n_rows][N] (its n_saved into ens_segn):
// `check`, the form's own checks, then the upload of the keys. The ensemble form looks only at the keys of the rows a member
// saved and replaces the others by harmless ones; it refuses T_rows on a record of per-member Arrhenius parameters.
StateBatch solution_batch(kin_network* h, PassCheck check, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T_rows, bool have_out, hipStream_t s);
StateBatch ensemble_batch(kin_network* h, PassCheck check, const double* k, int64_t n_k_rows, const int64_t* k_row,
                          const double* T_rows, bool have_out, hipStream_t s);
// what ensemble_batch and kin_ensemble_flux answer, with KIN_ERR_STATE, on a record of observables (kin_ensemble_observables
// with store): the passes that need species and reactions have none to work on
constexpr const char* OBSERVABLES_RECORD_MSG =
    "the stored ensemble is a record of observables (kin_ensemble_observables with store): its columns are no species, and this "
    "pass needs species and reactions; solve the ensemble again";
// the keys alone into f_k, f_krow, f_T (host_batch and solution_batch; the segmented entries of the flux pass)
FluxSource stage_source(kin_network* h, int64_t B, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T, hipStream_t s);

// The flux pass on device buffers: flux[R] (weights d_w) and / or rates[B][R]; grows the handle's workspace, then enqueues on s.
void flux_run(kin_network* h, int64_t B, const double* d_u, const FluxSource& src, const double* d_w, double* d_flux,
              double* d_rates, hipStream_t s);

// A species list of a host entry (DRGEP's targets, reaction importance's selection): checked, made 0-based and uploaded into
// f_sel; the two messages are the entry's own.
const int64_t* species_list(kin_network* h, const int64_t* list, int64_t n, int index_base, const char* none_msg, const char* range_msg,
                            hipStream_t s);

constexpr size_t BLOCK_BYTES = (size_t)256 << 20;   // bound of every per-state workspace of a block of states
// States per block of a pass whose largest workspace holds doubles_per_state per state; the environment variable env_name
// (read per call: tests change it) lowers it, values below 1 are ignored.
inline int64_t block_states(size_t doubles_per_state, int64_t B, const char* env_name) {
  int64_t nb = std::max<int64_t>(1, (int64_t)(BLOCK_BYTES / (std::max<size_t>(doubles_per_state, 1) * sizeof(double))));
  if (const char* e = getenv(env_name)) {
    const int64_t v = atoll(e);
    if (v >= 1) nb = std::min(nb, v);
  }
  return std::min(nb, B);
}

// body(b0, nb, use_prev) for the blocks of B states; use_prev: the result so far - the caller's or an earlier block's - takes part
template <class F>
void for_blocks(int64_t B, int64_t nb_max, int accumulate, F body) {
  for (int64_t b0 = 0; b0 < B; b0 += nb_max) body(b0, std::min(nb_max, B - b0), (accumulate || b0 > 0) ? 1 : 0);
}

// the empty-batch rule of an accumulating pass: without a state the result is zeros, or the caller's left alone; true when B == 0
inline bool empty_batch(int64_t B, double* d_out, int64_t n, int accumulate, hipStream_t s) {
  if (B > 0) return false;
  if (!accumulate) KIN_HIP(hipMemsetAsync(d_out, 0, (size_t)n * sizeof(double), s));
  return true;
}

// The accumulating result host[n] of a host entry, staged through f_result: uploaded first when it takes part, run(device
// pointer), downloaded, and the stream waited for. host null (an optional result): run(nullptr) and the wait.
template <class F>
void staged_result(kin_network* h, int64_t n, double* host, int accumulate, hipStream_t s, F run) {
  if (host) {
    h->f_result.alloc((size_t)n);
    if (accumulate) h->f_result.upload(host, (size_t)n, s);
  }
  run(host ? h->f_result.p : nullptr);
  if (host) h->f_result.download(host, (size_t)n, s);
  KIN_HIP(hipStreamSynchronize(s));
}

// KIN_SLICES_MAX (read per call: tests change it) caps the slices Y a pass cuts a block's states into - launches and part[Y][...]
// alike - so that a task walks several states of a small batch; values below 1 are ignored. A test knob: results do not depend on Y.
inline int slices_cap(int Y) {
  if (const char* e = getenv("KIN_SLICES_MAX")) {
    const long long v = atoll(e);
    if (v >= 1) Y = (int)std::min<long long>(Y, v);
  }
  return Y;
}

}  // namespace kin
