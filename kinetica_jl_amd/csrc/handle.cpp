// kin_network's launches of the single-state and batched right-hand side and of the Jacobian (handle.hpp), with the rate
// constants of a temperature still pending formed on the way.
#include "handle.hpp"
#include "solver_kernels.hpp"

using namespace kin;

void kin_network::flush_pending_T(hipStream_t s) {
  if (!k_pending) return;
  launch_arrhenius(host.R, Ea.p, A.p, has_kmax, k_max, t_mult, T_pending, k.p, s);
  k_pending = false;
}

void kin_network::rhs_dev(const double* d_u, double* d_du) {
  if (k_pending) { launch_rates_T(host.R, pending_at(), k.p, d_u, x0.p, x1.p, rate.p, stream); k_pending = false; }
  else launch_rates(host.R, k.p, d_u, x0.p, x1.p, rate.p, stream);
  launch_segsum(rhs_plan.view(), SEG_COEF_SET, rate.p, d_du, SegExtra{}, stream);
}

SweepPlan kin_network::sweep_plan_dev(int64_t B, const double* d_u, const double* d_k, const double* d_du) const {
  const auto bits = [](const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); };
  return sweep_plan(sweep_net_info(host), n_cu, B, SweepAlign{bits(d_u), bits(d_k ? d_k : k.p), bits(d_du)});
}

void kin_network::sweep_dev(int64_t B, const double* d_u, const double* d_k, double* d_du, hipStream_t s) {
  if (!d_k) flush_pending_T(s);   // the handle's own k is about to be read: a temperature still pending is formed first
  const SweepPlan plan = sweep_plan_dev(B, d_u, d_k, d_du);
  if (plan.kernel == SWEEP_PER_STATE) {
    // (sweep_plan.hpp: species ids beyond 16 bits) the single-state kernels, state after state on the same stream
    for (int64_t b = 0; b < B; b++) {
      launch_rates(host.R, d_k ? d_k + b * host.R : k.p, d_u + b * host.N, x0.p, x1.p, rate.p, s);
      launch_segsum(rhs_plan.view(), SEG_COEF_SET, rate.p, d_du + b * host.N, SegExtra{}, s);
    }
  } else if (plan.kernel == SWEEP_BIG) {
    big_scratch.alloc((size_t)plan.grid * (size_t)(host.N - host.big_H + host.n_pairs()));
    launch_sweep_big(plan, host.N, host.R, host.n_pairs(), B, big_rec8.p, big_rec.p, big_expl.p, sweep_k.p, big_spec.p, big_tptr.p,
                     big_tent.p, big_scratch.p, d_u, d_k, k.p, d_du, s);
  } else
    launch_sweep(plan, host.N, host.R, host.n_pairs(), B, sweep_rec.p, sweep_k.p, host.pair_rec64.empty() ? nullptr : sweep_rec64.p,
                 sweep_copy.p, host.gen_rec8.empty() ? nullptr : gen_rec8.p, gen_k.p, gen_expl.p, d_u, d_k, k.p, d_du, s);
}

void kin_network::jac_dev(const double* d_u, double* d_vals) {
  if (k_pending) { launch_drates_T(host.R, pending_at(), k.p, d_u, x0.p, x1.p, dr.p, stream); k_pending = false; }
  else launch_drates(host.R, k.p, d_u, x0.p, x1.p, dr.p, stream);
  launch_segsum(jac_plan.view(), SEG_COEF_SET, dr.p, d_vals, SegExtra{}, stream);
}
