// TEST INFRASTRUCTURE - not a product path, never loaded by kinetica_jl_amd.
// CPU replay of the resident integrator's continuous rate mode (ResParams::rate_mode 3: the rates re-formed at T(t) of every
// step attempt, resident_core.hpp): the sequential backend of tests/native/resident_host.cpp, unchanged, extended by the
// operation that mode needs - apply_T (the Arrhenius rates at one temperature, what resident.hip's ph_apply_T does). The
// LU-cache lookup with the bound on the age of a slot's Jacobian in accepted steps is the shared slot_nearest already.
#include "../native/resident_host.cpp"

namespace {

struct ContBackend : HostBackend {
  using HostBackend::HostBackend;
  void apply_T(double T) {
    const double RT = 8.314462618 * T;
    for (int r = 0; r < R; r++) {
      const double kr = net.A[r] * std::exp(-net.Ea[r] / RT) * 6.02214076e23 * net.t_mult;
      k[r] = net.has_kmax ? 1.0 / (1.0 / net.k_max + 1.0 / kr) : kr;
    }
  }
};
static_assert(ResHasApplyT<ContBackend>::value, "the continuous backend is detected");
static_assert(!ResHasApplyT<HostBackend>::value, "the plain replay backend runs without apply_T");

}  // namespace

extern "C" {

// a continuous solve: kin_solve_continuous's arguments (the handle made by res_host_create, Arrhenius parameters set by
// res_host_set_arrhenius); out_t / out_u sized by res_host_rows
int res_cont_solve(void* hv, const kin_params* p, const double* u0, const double* t_nodes, const double* T_nodes, int64_t n_nodes,
                   int n_slots, double* out_t, double* out_u, int64_t* n_saved, ResResult* result) {
  HostNet* n = (HostNet*)hv;
  const ResGrid g = make_res_grid(*p);
  ResParams P{};
  res_fill_params(P, *p, g);
  res_default_settings(P, n_slots > 0 ? n_slots : RES_MAX_SLOTS);
  P.save_local = g.save_local.data();
  P.n_stops = 0;
  P.rate_mode = 3;
  P.t_nodes = t_nodes; P.T_nodes = T_nodes; P.n_nodes = n_nodes;
  ContBackend B(*n, P);
  B.u0 = u0;
  ResidentBdf<ContBackend> ctl(B, P);
  const ResResult r = ctl.run();
  const int64_t rows = std::min<int64_t>(r.n_saved, g.cap);
  if (out_t) std::copy(B.sol_t.begin(), B.sol_t.begin() + rows, out_t);
  if (out_u) std::copy(B.sol.begin(), B.sol.begin() + (size_t)rows * n->H.N, out_u);
  if (n_saved) *n_saved = rows;
  if (result) *result = r;
  return r.retcode;
}

}  // extern "C"
