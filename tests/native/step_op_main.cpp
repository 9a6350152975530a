// TEST INFRASTRUCTURE: a stand-alone program over the replay's single-operation entries (resident_host.cpp: res_host_step_op,
// res_host_corrector_loop), for a sanitizer build of that host code (`make asan` compiles both files with
// -fsanitize=address,undefined and runs this). Every operation at every order on the pair networks of 2 and of 513 species (one
// pair; two trips' worth of species plus the inert one), on state blocks of the probe's layout filled with mixed-sign values.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
void* res_host_create(int64_t n_species, int64_t n_reactions, const int64_t* rp, const int64_t* ri, const int64_t* rs, const int64_t* pp,
                      const int64_t* pi, const int64_t* ps, int index_base, const int* lu_opt, int64_t* info);
void res_host_destroy(void* h);
int res_host_step_op(void* hv, int op, const int32_t* ia, const double* da, const double* k, double* state, double* ctrl);
void res_host_corrector_loop(int n_species, int n_sums, const double* sums, const double* cin, double* out);
}

int main() {
  int launches = 0;
  for (int n : {2, 513}) {
    const int p = n / 2, R = 2 * p;
    // A_i -> B_i, B_i -> A_i
    std::vector<int64_t> rp(R + 1), ri(R), rs(R, 1), pp(R + 1), pi(R), ps(R, 1);
    for (int r = 0; r <= R; r++) rp[r] = pp[r] = r;
    for (int i = 0; i < p; i++) { ri[i] = 2 * i; pi[i] = 2 * i + 1; ri[p + i] = 2 * i + 1; pi[p + i] = 2 * i; }
    int64_t info[8] = {};
    void* h = res_host_create(n, R, rp.data(), ri.data(), rs.data(), pp.data(), pi.data(), ps.data(), 0, nullptr, info);
    if (!h) { std::printf("res_host_create failed\n"); return 1; }
    std::vector<double> k(R, 1024.0), state((size_t)28 * n), ctrl(18);
    uint64_t seed = 12345u + n;
    auto rnd = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    for (int order = 1; order <= 5; order++)
      for (int op = 0; op <= 10; op++)
        for (int aux = 0; aux <= (op == 0 ? 5 : (op == 3 || op == 4 ? 1 : 0)); aux++)
          for (int row = 0; row <= (op == 1 || op == 2 || op == 8 ? 1 : 0); row++) {
            for (double& v : state) v = (rnd() - 0.4) * 1e-3;
            for (int i = 0; i < n; i++) {
              state[8 * n + i] = 0.1 + rnd();                          // y > 0
              state[11 * n + i] = 1e-14 + 1e-8 * state[8 * n + i];     // scale
              state[26 * n + i] = state[8 * n + i];
              state[i] = state[8 * n + i]; state[n + i] = 1e-9 * (rnd() - 0.5);
            }
            for (double& v : ctrl) v = 0.5;
            const int32_t ia[3] = {order, aux, row};
            const double da[17] = {1e-14, 1e-8, 0.375, 1.0, 0.125, 0.96875, 0.75 / 1024, 1.0 / 1024, 0.8, 1.0, 0.5, 0.03, 0.03, 0.2, 0.3, 0.2, 0.1};
            if (res_host_step_op(h, op, ia, da, k.data(), state.data(), ctrl.data()) != 0) { std::printf("operation %d refused\n", op); return 1; }
            launches++;
          }
    const int32_t bad[3] = {6, 0, 0};
    const double da0[17] = {};
    if (res_host_step_op(h, 6, bad, da0, k.data(), state.data(), ctrl.data()) != -1) { std::printf("order 6 accepted\n"); return 1; }
    res_host_destroy(h);
  }
  const double sums[3][5] = {{64.0, 1, 1, 1, 0}, {0.64, 1, 1, 1, 4294967296.0}, {0.0064, 1, 1, 1, 4294967296.0}};
  const double cin[8] = {3, 1, 1, 1, 1, -1, 0.03, 0.2};
  double out[12];
  res_host_corrector_loop(64, 3, &sums[0][0], cin, out);
  if (out[0] != 1 || out[1] != 1 || out[5] != 2 || out[4] != 1) { std::printf("scripted attempt: unexpected result\n"); return 1; }
  std::printf("ok: %d operations\n", launches);
  return 0;
}
