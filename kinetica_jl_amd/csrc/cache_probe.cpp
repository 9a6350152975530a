// kin_cache_probe (declaration and argument layout: include/kinetica_hip.h): the LU cache's drift guard once, on the caller's
// Jacobian values, through the launchers the integrators use - launch_jac_diag, launch_drift_test and drop_drifted of HostBackend::drift_launch / drift_collect
// and the lockstep ensemble (path 0), ph_factor's saved diagonal, DevBackend::drift_check / ph_drift and the slot lookups of the
// resident kernel (path 1: resident.cpp, resident_probe.hip). Nothing here computes: the probe uploads, fills the launchers'
// arguments the way HostBackend / EnsembleSolver fill them, launches, downloads. Every index array is the handle's own.
#include "../../include/kinetica_hip.h"

#include <algorithm>
#include <vector>

#include "handle.hpp"
#include "lu.hpp"
#include "resident.hpp"
#include "solver.hpp"

using namespace kin;

namespace {

constexpr double SENTINEL = -7.0;   // fills the drift results before a launch: a slot no workgroup wrote shows

struct Pinned {   // the drift test's host target (HostBackend::h_drift is pinned as well)
  double* p = nullptr;
  explicit Pinned(size_t n) { KIN_HIP(hipHostMalloc((void**)&p, n * sizeof(double), hipHostMallocDefault)); }
  ~Pinned() { if (p) (void)hipHostFree(p); }
};

void host_drift(kin_network* h, int64_t n_slots, const double* jv_slots, const double* c_fact, const int32_t* valid, const double* jv_now,
                double max_drift, double* jd, double* drift, int32_t* out_i, int64_t* info) {
  const int64_t N = h->host.N, nnz = h->host.nnz();
  const int n = (int)n_slots;
  hipStream_t s = h->stream;
  DevBuf<int32_t> d_jdiag;
  DevBuf<double> d_jvs, d_now, d_drift, d_drift_k;
  d_jdiag.upload(h->host.j_diag, s);
  d_jvs.upload(jv_slots, (size_t)(n_slots * nnz), s);
  d_now.upload(jv_now, (size_t)nnz, s);
  // slots as HostBackend::factor leaves them: the diagonal of the Jacobian behind each by launch_jac_diag (an unused slot's too, so
  // that every row can be compared; launch_drift_test hands the kernel no pointer for it)
  std::vector<SparseLU::Slot> slots((size_t)n);
  for (int i = 0; i < n; i++) {
    slots[i].jd.alloc((size_t)N);
    launch_jac_diag((int)N, d_jvs.p + (size_t)i * nnz, d_jdiag.p, slots[i].jd.p, s);
    slots[i].c_fact = c_fact[i];
    slots[i].valid = valid[i] != 0;
  }
  KIN_HIP(hipGetLastError());
  for (int i = 0; i < n; i++) slots[i].jd.download(jd + (size_t)i * N, (size_t)N, s);
  // (a) HostBackend::drift_launch: results copied to the pinned host target by the launcher
  Pinned pin((size_t)LU_MAX_SLOTS + 1);
  std::vector<double> fill((size_t)2 * LU_MAX_SLOTS, SENTINEL);
  std::copy(fill.begin(), fill.begin() + LU_MAX_SLOTS + 1, pin.p);
  d_drift.upload(fill.data(), (size_t)LU_MAX_SLOTS + 1, s);
  const int n_checked = launch_drift_test((int)N, slots, d_now.p, d_jdiag.p, d_drift.p, pin.p, s);
  KIN_HIP(hipGetLastError());
  // (b) the lockstep ensemble: no host target, the member's results at an offset of the ensemble's buffer (member 1 of 2 here),
  // one copy of the whole buffer afterwards
  d_drift_k.upload(fill.data(), fill.size(), s);
  launch_drift_test((int)N, slots, d_now.p, d_jdiag.p, d_drift_k.p + LU_MAX_SLOTS, nullptr, s);
  KIN_HIP(hipGetLastError());
  std::vector<double> h_k((size_t)2 * LU_MAX_SLOTS);
  d_drift_k.download(h_k.data(), h_k.size(), s);
  KIN_HIP(hipStreamSynchronize(s));
  std::copy(pin.p, pin.p + n, drift);
  std::copy(h_k.begin() + LU_MAX_SLOTS, h_k.begin() + LU_MAX_SLOTS + n, drift + n);
  std::vector<SparseLU::Slot> flags((size_t)n);   // (drop_drifted looks at the flags and the results only)
  for (int i = 0; i < n; i++) flags[i].valid = slots[i].valid;
  std::fill(info, info + 8, (int64_t)0);
  info[0] = drop_drifted(slots, n_checked, pin.p, max_drift);
  info[1] = n_checked;
  info[2] = drop_drifted(flags, n, h_k.data() + LU_MAX_SLOTS, max_drift);
  // what lies outside the slots' results stayed as it was
  bool clean = pin.p[LU_MAX_SLOTS] == SENTINEL;
  for (int i = 0; i < LU_MAX_SLOTS; i++) clean = clean && h_k[i] == SENTINEL && (i < n || (h_k[LU_MAX_SLOTS + i] == SENTINEL && pin.p[i] == SENTINEL));
  info[6] = clean ? 1 : 0;
  for (int i = 0; i < n; i++) out_i[i] = slots[i].valid ? 1 : 0;
}

}  // namespace

extern "C" int kin_cache_probe(kin_network* h, int32_t path, int32_t mode, int64_t n_slots, const double* jv_slots, const double* c_fact,
                               const int32_t* valid, const double* jv_now, double max_drift, const int64_t* stamps, int64_t n_queries,
                               const double* qd, const int64_t* qi, double* jd, double* drift, int32_t* out_i, int64_t* info) {
  if (!h) return KIN_ERR_INVALID_ARG;
  try {
    KIN_HIP(hipSetDevice(h->device));
    require((path == 0 || path == 1) && (mode == KIN_CACHE_DRIFT || mode == KIN_CACHE_RULES), ERR_INVALID_ARG, "unknown path or mode");
    require(out_i && info, ERR_INVALID_ARG, "null buffer");
    if (mode == KIN_CACHE_DRIFT) {
      require(n_slots >= 1 && n_slots <= (path == 0 ? LU_MAX_SLOTS : RES_MAX_SLOTS), ERR_INVALID_ARG,
              "n_slots outside 1 .. 128 (path 0) / 1 .. 64 (path 1)");
      require(jv_slots && c_fact && valid && jv_now && jd && drift, ERR_INVALID_ARG, "null buffer");
      if (path == 0) host_drift(h, n_slots, jv_slots, c_fact, valid, jv_now, max_drift, jd, drift, out_i, info);
      else resident_cache_probe(h, RES_PROBE_DRIFT, n_slots, jv_slots, c_fact, valid, jv_now, max_drift, nullptr, 0, nullptr, nullptr, jd, drift,
                                out_i, info);
    } else {
      require(path == 1, ERR_INVALID_ARG, "the slot-rule mode belongs to path 1 (the host paths share the templates of bdf_rules.hpp)");
      require(n_slots >= 0 && n_slots <= RES_MAX_SLOTS && n_queries >= 1 && n_queries <= 4096, ERR_INVALID_ARG, "n_slots outside 0 .. 64 or n_queries outside 1 .. 4096");
      require((n_slots == 0 || (c_fact && valid && stamps)) && qd && qi, ERR_INVALID_ARG, "null buffer");
      for (int64_t q = 0; q < n_queries; q++)
        require(qi[5 * q + 4] >= 0 && qi[5 * q + 4] <= RES_MAX_SLOTS, ERR_INVALID_ARG, "a query's slot count outside 0 .. 64");
      resident_cache_probe(h, RES_PROBE_RULES, n_slots, nullptr, c_fact, valid, nullptr, 0.0, stamps, n_queries, qd, qi, nullptr, nullptr, out_i, info);
    }
  } catch (const KinError& e) {
    h->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    h->err = e.what();
    return KIN_ERR_DEVICE;
  }
  return KIN_OK;
}
