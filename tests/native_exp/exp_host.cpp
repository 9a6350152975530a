// Host replay of exp_tab.hpp - TEST INFRASTRUCTURE: the product header compiled for the CPU, entered the way the kernels
// enter it (rate_table_kernel's per-reaction and per-row prologue for the fast form).
#include <cmath>
#include <cstdint>
#define __device__
#define __forceinline__ inline
using std::exp; using std::fma; using std::fmin; using std::fmax; using std::ldexp; using std::rint;
#include "../../kinetica_jl_amd/csrc/exp_tab.hpp"

namespace {

template <int TAB>
void fill_tab(double* tab) {
  for (int i = 0; i < TAB; i++) tab[i] = kin::kExp2Tab[i * (512 / TAB)];
}

template <int TAB>
void exp_tab_n(const double* x, int64_t n, double* out) {
  double tab[TAB];
  fill_tab<TAB>(tab);
  for (int64_t i = 0; i < n; i++) out[i] = kin::exp_tab_t<TAB>(x[i], tab);
}

template <int TAB>
void fast_n(const double* Ea, const double* A, int64_t n, double T, int has_kmax, double k_max, double t_mult, double* out) {
  double tab[TAB];
  fill_tab<TAB>(tab);
  const double RT = 8.314462618 * T, inv_RT = kin::arrhenius_inv_RT(RT), inv_kmax = 1.0 / k_max;
  for (int64_t i = 0; i < n; i++) {
    const double c = A[i] * 6.02214076e23 * t_mult, ic = 1.0 / c;
    out[i] = kin::arrhenius_fast_t<TAB>(Ea[i], c, ic, RT, inv_RT, has_kmax, inv_kmax, tab);
  }
}

}  // namespace

extern "C" {
void exp2_table(double* out) { fill_tab<512>(out); }
void exp_tab_512(const double* x, int64_t n, double* out) { exp_tab_n<512>(x, n, out); }
void exp_tab_128(const double* x, int64_t n, double* out) { exp_tab_n<128>(x, n, out); }
void arrhenius_fast_512(const double* Ea, const double* A, int64_t n, double T, int has_kmax, double k_max, double t_mult, double* out) {
  fast_n<512>(Ea, A, n, T, has_kmax, k_max, t_mult, out);
}
void arrhenius_fast_128(const double* Ea, const double* A, int64_t n, double T, int has_kmax, double k_max, double t_mult, double* out) {
  fast_n<128>(Ea, A, n, T, has_kmax, k_max, t_mult, out);
}
void arrhenius_literal(const double* Ea, const double* A, int64_t n, double T, int has_kmax, double k_max, double t_mult, double* out) {
  for (int64_t i = 0; i < n; i++) out[i] = kin::arrhenius_one(Ea[i], A[i], 8.314462618 * T, has_kmax, k_max, t_mult);
}
}
