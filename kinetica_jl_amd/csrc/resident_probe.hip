// The resident integrator's phases run once on given inputs (kin_resident_probe: tests compare each with a reference). Built
// from the same source as the product kernel with its one-workgroup-per-CU register budget; the probe kernel takes the place of
// resident_bdf_kernel, so the product's translation units (resident.hip, resident_w4.hip) compile as they would without it.
#define RES_LINALG_PROBE
#include "resident.hip"
