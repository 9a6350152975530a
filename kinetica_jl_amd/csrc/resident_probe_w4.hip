// The diagnostic build of the resident integrator (resident_probe.hip) with the shared-CU build's register budget and inlined
// phases (resident_w4.hip): kin_step_probe's path 4 runs the step's operations through it.
#define RES_LINALG_PROBE
#define RES_WAVES_PER_EU 4
#define RES_PHASE __device__ __forceinline__
#include "resident.hip"
