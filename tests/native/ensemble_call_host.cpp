// TEST INFRASTRUCTURE - not a product path, never loaded by kinetica_jl_amd.
// The host parts of the ensemble call layer (kinetica_jl_amd/csrc/solver.hpp), which need no device: EnsembleCall::block, the
// thread route's member assignment, the finishing layer's host part and the member-thread runner. Part of
// libkin_resident_host.so (tests/native/Makefile); tests/test_ensemble_call_host.py drives it.
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../kinetica_jl_amd/csrc/solver.hpp"

using namespace kin;

extern "C" {

// EnsembleCall::block(N, R, m0, n) of a call of K members over arrays made here, seen through the block's member j. The call has
// per-member stops (stop_ptr), or per-member profiles (node_ptr), or neither (static: per-member k and T); the first two carry
// per-member Ea / A with stand-ins for their device copies (never dereferenced). out[24], every pointer as its offset in elements
// from the whole call's (-1: null): 0 K, 1 u0, 2 k, 3 T, 4 stop_ptr, 5 node_ptr, 6 tstops, 7 T_stops, 8 t_nodes, 9 T_nodes,
// 10 Ea, 11 A, 12 out_t, 13 out_u, 14 n_saved, 15 retcodes, 16 stats, 17 cap, and of member j: 18 / 19 member_stops' tstops /
// T_stops, 20 its count, 21 / 22 member_arrhenius' Ea / A from the device stand-ins, 23 its first node's offset in t_nodes
void ens_host_block(const kin_params* p, int64_t K, int64_t N, int64_t R, const int64_t* stop_ptr, const int64_t* node_ptr, int64_t m0,
                    int64_t n, int64_t j, int64_t* out) {
  const int64_t cap = make_res_grid(*p).cap;
  const bool member_form = stop_ptr || node_ptr;
  const int64_t n_all = stop_ptr ? stop_ptr[K] : node_ptr ? node_ptr[K] : 1;
  std::vector<double> u0(K * N), k(K * R), T(K), ts(n_all), Ts(n_all), Ea(K * R), A(K * R), dEa(K * R), dA(K * R), out_t(cap), out_u(K * cap * N);
  std::vector<int64_t> ns(K);
  std::vector<int32_t> rc(K);
  std::vector<kin_stats> st(K);
  EnsembleCall c{*p, K, u0.data(), member_form ? nullptr : k.data(), member_form ? nullptr : T.data(), stop_ptr ? ts.data() : nullptr,
                 stop_ptr ? Ts.data() : nullptr, nullptr, 0, stop_ptr, node_ptr, node_ptr ? ts.data() : nullptr, node_ptr ? Ts.data() : nullptr,
                 nullptr, out_t.data(), out_u.data(), ns.data(), rc.data(), st.data()};
  if (member_form) { c.Ea = Ea.data(); c.A = A.data(); c.d_Ea = dEa.data(); c.d_A = dA.data(); }
  const EnsembleCall b = c.block(N, R, m0, n);
  const auto off = [](const auto* q, const auto* base) { return q ? (int64_t)(q - base) : (int64_t)-1; };
  kin_network net;
  net.host.N = N; net.host.R = R;
  const EnsembleCall::Stops ms = b.member_stops(j);
  const EnsembleCall::Arrhenius pm = b.member_arrhenius(&net, j);
  const int64_t v[24] = {b.K, off(b.u0, c.u0), off(b.k, c.k), off(b.T, c.T), off(b.stop_ptr, c.stop_ptr), off(b.node_ptr, c.node_ptr),
                         off(b.tstops, c.tstops), off(b.T_stops, c.T_stops), off(b.t_nodes, c.t_nodes), off(b.T_nodes, c.T_nodes),
                         off(b.Ea, c.Ea), off(b.A, c.A), off(b.out_t, c.out_t), off(b.out_u, c.out_u), off(b.n_saved, c.n_saved),
                         off(b.retcodes, c.retcodes), off(b.stats, c.stats), cap, off(ms.tstops, c.tstops), off(ms.T_stops, c.T_stops), ms.n,
                         member_form ? off(pm.Ea, c.d_Ea) : -1, member_form ? off(pm.A, c.d_A) : -1,
                         b.node_ptr ? off(b.t_nodes + b.node_ptr[j], c.t_nodes) : -1};
  std::memcpy(out, v, sizeof v);
}

// replica_thread_share(K, limit): out[2] = (per, threads), thread_of[K]
void ens_host_thread_share(int64_t K, int64_t limit, int64_t* out, int64_t* thread_of) {
  const ThreadShare s = replica_thread_share(K, limit);
  out[0] = s.per; out[1] = s.threads;
  for (int64_t m = 0; m < K; m++) thread_of[m] = s.thread_of(m);
}

// finish_members over K results (n_saved_in, ret_in, stats.n_steps = steps_in) into the outputs given (each may be null). times:
// every member's save times [K][cap] on the host, or null (the furthest member's are elsewhere). rows[K]: the clamped rows;
// returns the furthest member
int64_t ens_host_finish(int64_t K, int64_t cap, const int64_t* n_saved_in, const int32_t* ret_in, const int64_t* steps_in, const double* times,
                        double* out_t, int64_t* n_saved, int32_t* retcodes, kin_stats* stats, int64_t* rows) {
  std::vector<MemberResult> res((size_t)K);
  std::vector<std::vector<double>> tt((size_t)K);
  for (int64_t m = 0; m < K; m++) {
    res[m].n_saved = n_saved_in[m]; res[m].retcode = ret_in[m]; res[m].stats.n_steps = steps_in[m];
    if (times) tt[m].assign(times + m * cap, times + (m + 1) * cap);
  }
  EnsembleCall c{};
  c.K = K; c.out_t = out_t; c.n_saved = n_saved; c.retcodes = retcodes; c.stats = stats;
  const EnsembleRows f = finish_members(c, cap, res.data(), times ? tt.data() : nullptr);
  std::copy(f.n_saved.begin(), f.n_saved.end(), rows);
  return f.best;
}

// run_member_threads over n bodies: body i throws "boom" if i == throw_at, else marks ran[i] from its own thread. Returns 0, or the
// KinError's code with its text in msg; never_started: calls of the hook
int ens_host_runner(int64_t n, int64_t throw_at, int32_t* ran, int64_t* never_started, char* msg, int64_t msg_len) {
  const std::thread::id caller = std::this_thread::get_id();
  *never_started = 0;
  try {
    run_member_threads(n, [&](int64_t i) {
      if (i == throw_at) throw std::runtime_error("boom");
      ran[i] = std::this_thread::get_id() != caller ? 1 : -1;
    }, [&](int64_t) { ++*never_started; });
  } catch (const KinError& e) {
    snprintf(msg, (size_t)msg_len, "%s", e.what());
    return e.code;
  }
  return 0;
}

}  // extern "C"
