// The scalar step-control rules of the BDF integrator, defined ONCE for every implementation inside the library: the
// host-driven integrator's explicit mode (solver.cpp), the controller ResidentBdf<B> (resident_core.hpp: on the device, on the host
// threads of the lockstep ensemble, in the CPU replays under tests/native*) and the set-up of EnsembleSolver (ensemble.cpp).
// Plain C++17, no HIP headers; every function is KIN_HD, so the same text compiles in the device pass, in hipcc's host pass
// and with a plain host compiler. The expressions are kept operation by operation as the integrators had them (a fused
// multiply-add appearing or disappearing changes bits). oracle/ (bdf.py, cpu_bdf.cpp) restates these rules independently -
// the tests compare against it, it must not include this header.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KIN_HD __host__ __device__
#else
#define KIN_HD
#endif

namespace kin {

constexpr int BDF_MAX_ORDER = 5;
constexpr int BDF_NEWTON_MAXITER = 4;
constexpr int BDF_D_ROWS = BDF_MAX_ORDER + 3;
// continuous rate updates: k(t) moves inside a segment and no restart re-validates the LU-cache slots - the Jacobian behind
// a reused slot is at most this many accepted steps old (CVODE's bound on the age of its Jacobian)
constexpr int64_t BDF_CONT_JAC_AGE = 50;

// An ACCEPTED step (corrector converged, error test passed) that leaves a species below -BDF_NEG_DEEP error weights ends the
// segment as Unstable. The error test bounds what ONE step can do to one species at sqrt(N) / error constant weights in the worst
// case (~300 at 1 000 species; more only if a step's whole error sat on a single species of a larger network), so such a state
// has been growing over many accepted steps: it is the negative excursion of DESIGN 4 - below zero some species are unstable
// under mass-action kinetics, |u| grows with an e-folding time of ~0.1 ms and h follows it down for 500-1 400 more steps until
// dtmin or a non-finite state ends the attempt anyway. The chunk's tolerance retry (negative entries of its start state zeroed)
// carries the solve in either case; a false alarm costs one such retry (docs/DESIGN_HISTORY.md R5.12 has the measurements). The flag
// rides in the sum that counts negative entries: a thread contributes 1 for a negative entry, BDF_NEG_MARK for a deep one.
constexpr double BDF_NEG_DEEP = 1e3;
constexpr double BDF_NEG_MARK = 4294967296.0;   // 2^32 > any count of species

struct BdfCoef {  // passed to kernels by value
  double gamma[BDF_MAX_ORDER + 1];
  double alpha[BDF_MAX_ORDER + 1];
  double error_const[BDF_MAX_ORDER + 2];
};
struct BdfMat { double v[BDF_MAX_ORDER + 1][BDF_MAX_ORDER + 1]; };
struct BdfVec { double v[BDF_MAX_ORDER + 1]; };

KIN_HD inline double bdf_inf() { return HUGE_VAL; }
// spacing of the doubles above x (x >= 0, finite): what std::nextafter(x, inf) - x gives on the host
KIN_HD inline double bdf_ulp_above(double x) { return nextafter(x, bdf_inf()) - x; }

// method coefficients of the NDF variant (Shampine & Reichelt 1997, orders 1-5): gamma_j = sum 1 / i, alpha_j = (1 - kappa_j)
// gamma_j, error constants kappa_j gamma_j + 1 / (j + 1); gamma / alpha hold BDF_MAX_ORDER + 1 entries, error_const one more
KIN_HD inline void bdf_fill_coef(double* gamma, double* alpha, double* error_const) {
  const double KAPPA[6] = {0.0, -0.1850, -1.0 / 9.0, -0.0823, -0.0415, 0.0};
  gamma[0] = 0.0;
  for (int j = 1; j <= BDF_MAX_ORDER; j++) gamma[j] = gamma[j - 1] + 1.0 / j;
  for (int j = 0; j <= BDF_MAX_ORDER; j++) alpha[j] = (1.0 - KAPPA[j]) * gamma[j];
  for (int j = 0; j <= BDF_MAX_ORDER; j++) error_const[j] = KAPPA[j] * gamma[j] + 1.0 / (j + 1);
  error_const[BDF_MAX_ORDER + 1] = 0.0;
}

// largest power of ten <= h, by exact IEEE operations only (the same double on the host, on the device and in the oracle's
// Python and C); h <= 0 or not below 1e300: h itself. (The host-driven integrator used to guard with !std::isfinite(h), the
// resident controller with !(h < 1e300) - the device-safe form kept here; they differ only for h >= 1e300, which no step
// size reaches.)
KIN_HD inline double bdf_decade_floor(double h) {
  if (!(h > 0.0) || !(h < 1e300)) return h;
  double p = 1.0;
  while (p > h) p /= 10.0;
  while (p * 10.0 <= h) p *= 10.0;
  return p;
}

// Corrector tolerance as a fraction of the error weight atol + rtol |y| (the estimated iteration error must get below it), in
// the style of ode15s / CVODE - a fixed fraction, not RADAU5's sqrt(rtol); ode15s uses 0.05, CVODE 0.1 (nlscoef). Here
// 0.03 at the default relative tolerance 1e-8 and looser ones, 0.1 from 1e-9 down, 1e-10 / rtol between.
// What it rests on (profiles/r05_newton_tol_ab.txt, one MI355X):
//  * at rtol <= 1e-9 an iteration asked to converge to 0.03 of the weight asks for less than the rounding of the right-hand
//    side's sums leaves (~1e-10 relative on these networks): it fails, and every failure restarts the step at a quarter. With 0.1
//    the 200-species solve at 1e-12 / 1e-10 ends 2-7 x closer to its Radau truth in half the steps (resident kernel rms 385 -> 55
//    tight units, host-driven 885 -> 394, CPU port 153 -> 61), C3 at 1e-11 / 1e-9 takes 0.60 s instead of 0.90 s;
//  * at 1e-8 a flat 0.1 is 7 % faster on C3 (0.350 -> 0.325 s) and passes every sweep with the default switches, but over the 140
//    solves of tools/robustness_sweep.py wide under four perturbed configurations (corrector fused, reuse band 0.3, 8 and 1
//    factorisation slots) 10 of 560 needed a tolerance retry after a step-size collapse, against 3 of 560 at 0.03 and 5 at 0.05
//    (ode15s) - all on 1 000-species networks, the ones that collapsed under 0.05 in round 2: not adopted there.
KIN_HD inline double bdf_newton_frac(double rtol) { return fmin(0.1, fmax(0.03, 1e-10 / rtol)); }
// ... and the tolerance itself: that fraction (`pinned_frac` > 0: a value a test pins instead), but at least 10 ulp / rtol
KIN_HD inline double bdf_newton_tol(double rtol, double pinned_frac = -1.0) {
  const double lo = 10.0 * 2.220446049250313e-16 / rtol;
  const double frac = pinned_frac > 0.0 ? pinned_frac : bdf_newton_frac(rtol);
  return lo > frac ? lo : frac;
}

// Rescaling of the difference array when the step size changes by `factor` at order `ord` (Shampine & Reichelt): D <- (R U)^T D
// with R = R(factor), U = R(1). M, R, U are the caller's work matrices (the resident controller keeps them as members: its
// object lives in LDS, locals indexed dynamically would go to scratch).
KIN_HD inline void bdf_compute_R(int ord, double factor, double (&M)[6][6], double (&R)[6][6]) {
  for (int i = 0; i <= ord; i++)
    for (int j = 0; j <= ord; j++) M[i][j] = 0.0;
  for (int j = 0; j <= ord; j++) M[0][j] = 1.0;
  for (int i = 1; i <= ord; i++)
    for (int j = 1; j <= ord; j++) M[i][j] = ((double)i - 1.0 - factor * (double)j) / (double)i;
  for (int j = 0; j <= ord; j++) {
    double p = 1.0;
    for (int i = 0; i <= ord; i++) { p *= M[i][j]; R[i][j] = p; }
  }
}
KIN_HD inline void bdf_change_D_matrix(int ord, double factor, double (&M)[6][6], double (&R)[6][6], double (&U)[6][6], double (&RU)[6][6]) {
  bdf_compute_R(ord, factor, M, R);
  bdf_compute_R(ord, 1.0, M, U);
  for (int a = 0; a <= ord; a++)
    for (int q2 = 0; q2 <= ord; q2++) {
      double v = 0.0;
      for (int q = 0; q <= ord; q++) v += R[a][q] * U[q][q2];
      RU[a][q2] = v;
    }
}

// Initial step of a (re)start = CVODE's (cvode.c: cvHin, cvUpperBoundH0, cvYddNorm - the documented solver of the reference,
// docs/src/getting-started.md:69, re-initialised at every chunk start and rate update, methods.jl:260, 819): the h with
// ||h^2 y'' / 2||_WRMS = 1, y'' from a difference quotient of f along the Euler direction, iterated (at most BDF_H0_EVALS
// evaluations) until two successive estimates agree within a factor of 2, halved (H_BIAS), kept inside [hlb, hub]: hlb = 100 ulp
// of the segment's largest time `tmax`, hub = a tenth of the segment but no step over which ANY component moves by more than a
// tenth of itself plus its error weight (`dmax` = max |f0| / (0.1 |y| + w)). Then rounded DOWN to a power of ten: the step size
// climbs through the same values after every restart, so the iteration matrices of the previous segment's climb are found in the
// LU cache again (C3, 100 chunks: 363 -> 269 factorisations, profiles/r04_h0_decade_ab.txt - the rms deviations from
// the truths do not move).
constexpr int BDF_H0_EVALS = 4;
struct BdfFirstStep {
  double hlb, hub, hg, hnew;
  KIN_HD bool iterate() const { return hub >= hlb; }   // else: the geometric mean of the bounds as it stands
};
KIN_HD inline BdfFirstStep bdf_h0_begin(double tmax, double interval, double dmax) {
  BdfFirstStep f;
  f.hlb = 100.0 * 2.220446049250313e-16 * tmax;
  f.hub = 0.1 * interval;
  if (f.hub * dmax > 1.0) f.hub = 1.0 / dmax;
  f.hg = sqrt(f.hlb * f.hub);
  f.hnew = f.hg;
  return f;
}
// evaluation `count` (1-based) gave d2 = rms((f(y + hg f0) - f0) / w): the next estimate; true when the iteration is over
KIN_HD inline bool bdf_h0_update(BdfFirstStep& f, int count, double d2) {
  const double ydd = d2 / f.hg;
  f.hnew = ydd * f.hub * f.hub > 2.0 ? sqrt(2.0 / ydd) : sqrt(f.hg * f.hub);
  if (count == BDF_H0_EVALS) return true;
  const double hrat = f.hnew / f.hg;
  if (hrat > 0.5 && hrat < 2.0) return true;
  if (count > 1 && hrat > 2.0) { f.hnew = f.hg; return true; }
  f.hg = f.hnew;
  return false;
}
// (h0 is finite: the bounds are, and the callers leave on a non-finite norm before they update)
KIN_HD inline double bdf_h0_finish(const BdfFirstStep& f, double interval) {
  double h0 = 0.5 * f.hnew;
  h0 = h0 < f.hlb ? f.hlb : h0;
  h0 = h0 > f.hub ? f.hub : h0;
  h0 = h0 < interval ? h0 : interval;
  return bdf_decade_floor(h0);
}

// smallest step at time t: the user's dtmin, but not below the resolution of the time variable
KIN_HD inline double bdf_min_step(double dtmin, double t) {
  const double ulp10 = 10.0 * bdf_ulp_above(t);
  return dtmin > ulp10 ? dtmin : ulp10;
}

// safety factor of the step-size selection from the corrector's iteration count; factor of an error-test rejection (>= 0.2)
KIN_HD inline double bdf_safety(int n_iter) { return 0.9 * (2.0 * BDF_NEWTON_MAXITER + 1.0) / (2.0 * BDF_NEWTON_MAXITER + n_iter); }
KIN_HD inline double bdf_reject_factor(double safety, double err_norm, int order) {
  const double f0 = safety * pow(err_norm, -1.0 / (order + 1));
  return f0 > 0.2 ? f0 : 0.2;
}

// Order / step-size selection after order + 1 equal steps: the order (one down, the same, one up) whose error norm allows the
// largest step; an order that is not on offer carries the norm inf. Growth cap 1e4 at the first selection after a
// (re)initialisation, 10 afterwards (CVODE: ETAMX1, ETAMX2 / ETAMX3).
struct BdfOrderChoice { int d_order; double factor; };
KIN_HD inline BdfOrderChoice bdf_select_order(int order, double err_m, double err_o, double err_p, double safety, bool first_selection) {
  const double norms[3] = {err_m, err_o, err_p};
  double best = -1.0;
  int arg = 1;
  for (int i = 0; i < 3; i++) {
    double f;
    if (norms[i] == 0.0) f = bdf_inf();
    else if (norms[i] == bdf_inf()) f = 0.0;
    else f = pow(norms[i], -1.0 / (order + i));
    if (f > best) { best = f; arg = i; }
  }
  const double f1 = safety * best;
  const double cap = first_selection ? 1e4 : 10.0;
  return BdfOrderChoice{arg - 1, f1 < cap ? f1 : cap};
}

// dense output at ts of the step that ended at t (step size h_abs, differences of `order`): y(ts) = D0 + sum_j p[j] D_j
KIN_HD inline void bdf_interp_weights(int order, double ts, double t, double h_abs, double (&p)[BDF_MAX_ORDER + 1]) {
  double prod = 1.0;
  p[0] = 0.0;
  for (int j = 0; j < order; j++) {
    prod *= (ts - (t - h_abs * j)) / (h_abs * (1.0 + j));
    p[j + 1] = prod;
  }
}

// ---- LU-cache slot lookup over a contiguous array of slot records (fields valid, c_fact, jac_stamp, step_stamp, last_use).
// The slot whose c_fact is closest (in ratio) to c and within the band, lowest index on ties; -1: none. A slot is offered for
// max_age restarts after its Jacobian was evaluated and, with step_age >= 0 (continuous rates), step_age accepted steps.
template <class S>
KIN_HD int slot_nearest(const S* sl, int n, double c, double band, long long n_restarts, long long max_age, long long n_steps = 0,
                        long long step_age = -1) {
  int best = -1;
  double bd = 1e300;
  for (int i = 0; i < n; i++) {
    const S& q = sl[i];
    if (!q.valid || n_restarts - q.jac_stamp > max_age) continue;
    if (step_age >= 0 && n_steps - q.step_stamp > step_age) continue;
    const double r = fabs(log(c / q.c_fact));
    if (r < bd && fabs(c / q.c_fact - 1.0) <= band) { bd = r; best = i; }
  }
  return best;
}
// a slot for a new factorisation: the first unused or expired one (-1: none), else the least recently used
template <class S>
KIN_HD int slot_first_free(const S* sl, int n, long long n_restarts, long long max_age) {
  for (int i = 0; i < n; i++)
    if (!sl[i].valid || n_restarts - sl[i].jac_stamp > max_age) return i;
  return -1;
}
template <class S>
KIN_HD int slot_lru(const S* sl, int n) {
  int v = 0;
  for (int i = 1; i < n; i++)
    if (sl[i].last_use < sl[v].last_use) v = i;
  return v;
}

}  // namespace kin
