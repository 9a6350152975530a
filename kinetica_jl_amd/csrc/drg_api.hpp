// What the entry points of the DRG family (drg_api.cpp: DRG and reaction importance; drgep_api.cpp; pfa_api.cpp) share beyond
// the batch-of-states layer of flux_api.hpp: the tables of a pairing mode and the first two launches of a block.
#pragma once
#include "drg.hpp"
#include "flux_api.hpp"

namespace kin {

constexpr const char* DRG_BLOCK_ENV = "KIN_DRG_BLOCK_STATES";   // block_states' knob of the whole family

// the handle's tables of a pairing mode, built at the first call (throws KinError), and their device side
DrgTables& drg_host(kin_network* h, int pairing);
kin_network::DrgMode& drg_dev(kin_network* h, int pairing, hipStream_t s);
// ... with the signed coefficients and the transposed pattern as well (DRGEP and PFA; drgep_api.cpp)
kin_network::DrgMode& drgep_dev(kin_network* h, int pairing, hipStream_t s);

// a denominator or edge plan on the device with its coefficient tables
struct DrgPlan {
  SegPlanView p; const float* ell_c; const float* long_c;
  void into(DrgArgs& a) const { a.p = p; a.ell_c = ell_c; a.long_c = long_c; }
};
// the two plans of a mode with the signed coefficients (after drgep_dev)
inline DrgPlan signed_den_plan(const kin_network::DrgMode& m) { return DrgPlan{m.den_plan.view(), m.den_ell_s.p, m.den_long_s.p}; }
inline DrgPlan signed_edge_plan(const kin_network::DrgMode& m) { return DrgPlan{m.edge_plan.view(), m.edge_ell_s.p, m.edge_long_s.p}; }

// Stage 1 and the denominators of the block [b0, b0 + nb) of a batch: the flux sweep writes the block's rates into
// h->drg_rates, then launch_drg_den (DRG, reaction importance) or, signed, launch_drgep_den (DRGEP, PFA) den[nb][N] into
// h->drg_den. `a` comes with the pass's own fields (E, part, r, rc) and leaves with the block's filled in, for the launches
// behind. stages 1: the sweep alone (the passes' stage knobs). drg_stage_alloc grows the two buffers for blocks of nb_max.
void drg_stage_alloc(kin_network* h, int64_t nb_max);
void drg_rates_den(kin_network* h, const StateBatch& b, int64_t b0, int64_t nb, const DrgPlan& den, bool signed_den, int stages,
                   DrgArgs& a, hipStream_t s);

}  // namespace kin
