// What the entry points of the directed-relation-graph pass (drg_api.cpp) share with DRGEP's (drgep_api.cpp).
#pragma once
#include "drg.hpp"
#include "flux_api.hpp"
#include "handle.hpp"

namespace kin {

constexpr size_t DRG_RATES_BYTES = (size_t)256 << 20;   // bound of the stage-1 workspace rates[nb][R]

// the handle's tables of a pairing mode, built at the first call (throws KinError), and their device side
DrgTables& drg_host(kin_network* h, int pairing);
kin_network::DrgMode& drg_dev(kin_network* h, int pairing, hipStream_t s);
// ... with the signed coefficients and the transposed pattern as well (DRGEP and PFA; drgep_api.cpp)
kin_network::DrgMode& drgep_dev(kin_network* h, int pairing, hipStream_t s);
// flux_check plus the pass's own limits; throws KinError
void drg_check(kin_network* h, int64_t B, bool have_k, bool have_row, bool have_T, bool have_out);
// Checks of the solution / ensemble forms and the upload of their rate-constant keys (f_k, f_krow, f_T; the ensemble's
// n_saved into ens_segn): the source of the saved states h->d_sol_u [n_saved][N] / h->ens.sol [K n_rows][N]. Throws KinError.
FluxSource drg_solution_source(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                               bool have_out, hipStream_t s);
FluxSource drg_ensemble_source(kin_network* h, const double* k, int64_t n_k_rows, const int64_t* k_row, const double* T_rows,
                               bool have_out, hipStream_t s);

}  // namespace kin
