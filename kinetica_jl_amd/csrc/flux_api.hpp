// What the entry points of the flux pass (flux_api.cpp) share with the passes built on it (drg_api.cpp).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "common.hpp"

struct kin_network;

namespace kin {

// where a call's rate constants come from: rows of k (k_stride doubles apart; 0 = one shared row) or the Arrhenius law at T[b]
struct FluxSource { const double* k; int64_t k_stride; const int64_t* k_row; const double* T; };

// argument and state checks of kin_flux_batched* (have_k: a rate-constant array or the resident table); throws KinError
void flux_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out);
// every k_row[b] in [0, n_rows); throws KinError
void flux_check_rows(const int64_t* k_row, int64_t B, int64_t n_rows);
// The pass on device buffers: flux[R] (weights d_w) and / or rates[B][R]; grows the handle's workspace, then enqueues on s.
void flux_run(kin_network* h, int64_t B, const double* d_u, const FluxSource& src, const double* d_w, double* d_flux,
              double* d_rates, hipStream_t s);

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
