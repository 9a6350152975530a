// TEST INFRASTRUCTURE - not a product path, never loaded by kinetica_jl_amd.
// The launch plans of the event-time and the resampling pass (kin::event_plan, kin::resample_plan: pure host functions of the
// product library, which read their KIN_* knobs per call) and a download of the stored ensemble record as it lies on the device,
// the rows past a member's n_saved included, which no entry of the library reads. Part of libkin_resident_host.so
// (tests/native/Makefile); tests/test_pass_plans_host.py and tests/test_gpu_ensemble_resample.py drive it.
#include <cstdint>

#include "../../kinetica_jl_amd/csrc/event_kernels.hpp"
#include "../../kinetica_jl_amd/csrc/handle.hpp"
#include "../../kinetica_jl_amd/csrc/resample_kernels.hpp"

using namespace kin;

extern "C" {

// out[6]: EVENT_LANES, EVENT_WAVES_MAX, EVENT_ROWS_IN_FLIGHT, RESAMPLE_SLICE, RESAMPLE_WAVES_MAX, RESAMPLE_TILE_MAX
void plan_host_constants(int32_t* out) {
  const int32_t v[6] = {EVENT_LANES, EVENT_WAVES_MAX, EVENT_ROWS_IN_FLIGHT, RESAMPLE_SLICE, RESAMPLE_WAVES_MAX, RESAMPLE_TILE_MAX};
  for (int i = 0; i < 6; i++) out[i] = v[i];
}

// out[2] = (waves, part_rows)
void plan_host_event(int64_t S, int64_t L, int64_t N, int n_cu, int32_t* out) {
  const EventPlan p = event_plan(S, L, N, n_cu);
  out[0] = p.waves; out[1] = p.part_rows;
}

// out[2] = (tile, waves)
void plan_host_resample(int64_t S, int64_t Q, int64_t N, int n_cu, int32_t* out) {
  const ResamplePlan p = resample_plan(S, Q, N, n_cu);
  out[0] = p.tile; out[1] = p.waves;
}

// the stored ensemble record [K][n_rows][N] as it lies on the device into out[len]; returns 0, -1 without a record or with a
// len that is not the record's, else the runtime's error
int plan_host_record_download(kin_network* h, double* out, int64_t len) {
  if (!h || !h->ens.valid() || len != h->ens.K * h->ens.cap * h->host.N) return -1;
  if (hipError_t e = hipStreamSynchronize(h->stream)) return (int)e;
  return (int)hipMemcpy(out, h->ens.sol, (size_t)len * sizeof(double), hipMemcpyDeviceToHost);
}

}  // extern "C"
