// Observables of stored states: for every row of the flat (segment, row) axis H linear forms over the species and G outputs
// built from them - a form, or the ratio of two - written pitch doubles per row (definitions: include/kinetica_hip.h).
//
// One launch, no atomics. A 256-thread workgroup owns `rows` consecutive rows of the flat axis. It stages the rows a segment
// really has into LDS with 16-byte loads (a row of odd N starts 8 bytes off a 16-byte boundary: every row is read as its own
// head element, aligned pairs and tail element), or - the gather path, for a row that does not fit LDS - reads them from global
// memory, the same layout behind another pointer. Then it walks the host-built plan once: per phase the forms that serve as
// denominators go into a table of OBS_DEN_SLOTS values per row in LDS, and after a barrier the outputs are evaluated, divided
// where they have a denominator and stored. A short form (at most 64 terms) is one lane's sequential sum, consecutive columns
// on consecutive lanes, so the stores of a row coalesce; a long form is one wavefront's: lane l sums the entries l, l + 64, ...
// in order and the 64 chains are folded by the butterfly of wave_sum (segsum_dev.hpp). A lane carries the sums of
// OBS_ROWS_REG rows through one walk over a form's entries: an entry is fetched once per four rows, from L2. No [rows][H]
// array exists anywhere. At last the columns from G on and every column of a row past its segment's end are written as zeros.
//
// Every sum is evaluated in the documented order with every operation rounded on its own: the file is compiled with
// floating-point contraction off (the pragma below), so w * u + acc does not become a fused multiply-add; the division is
// hipcc's IEEE double division. A singleton of weight 1.0 is one exact multiplication: the species' bits, -0.0 included. The
// class of a form depends on its length only, never on the launch.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../include/kinetica_hip.h"
#include "observable_kernels.hpp"

#pragma clang fp contract(off)

namespace kin {

namespace {

// the LDS of a workgroup: the denominator table [rows][OBS_DEN_SLOTS], then (LDS path) the rows [rows][N]; one dynamic
// region, every offset a multiple of 16 bytes
extern __shared__ __attribute__((aligned(16))) double obs_lds[];

// what a task's value becomes: slot `col` of the row's table in a denominator stage, else column `col` of the row's output,
// divided by its denominator's slot first where it has one
template <bool DEN>
__device__ __forceinline__ void obs_store(const ObsArgs& a, const ObsTask& t, int64_t row0, int r, double v) {
  if (DEN) { obs_lds[r * OBS_DEN_SLOTS + t.col] = v; return; }
  if (t.den >= 0) v = v / obs_lds[r * OBS_DEN_SLOTS + t.den];
  a.out[(size_t)(row0 + r) * (size_t)a.pitch + (size_t)t.col] = v;
}

// short tasks [t0, t1): one per lane
template <bool DEN>
__device__ __forceinline__ void obs_short(const ObsArgs& a, const double* ub, int t0, int t1, int64_t row0, int nrows, unsigned live) {
  for (int ti = t0 + (int)threadIdx.x; ti < t1; ti += OBS_THREADS) {
    const ObsTask t = a.tasks[ti];
    for (int r0 = 0; r0 < nrows; r0 += OBS_ROWS_REG) {
      if (!((live >> r0) & ((1u << OBS_ROWS_REG) - 1u))) continue;      // (none of these rows is real: no walk over the entries)
      double acc[OBS_ROWS_REG];
#pragma unroll
      for (int c = 0; c < OBS_ROWS_REG; c++) acc[c] = 0.0;
      for (int e = 0; e < t.n; e++) {
        const int i = a.idx[t.e0 + e];
        const double w = a.w[t.e0 + e];
#pragma unroll
        for (int c = 0; c < OBS_ROWS_REG; c++) {
          if (!((live >> (r0 + c)) & 1u)) continue;      // (a row past its segment's end is never read)
          const double p = w * ub[(size_t)(r0 + c) * a.N + i];
          acc[c] = e == 0 ? p : acc[c] + p;
        }
      }
#pragma unroll
      for (int c = 0; c < OBS_ROWS_REG; c++)
        if ((live >> (r0 + c)) & 1u) obs_store<DEN>(a, t, row0, r0 + c, acc[c]);
    }
  }
}

// long tasks [t0, t1): one per wavefront, 64 chains and the butterfly
template <bool DEN>
__device__ __forceinline__ void obs_long(const ObsArgs& a, const double* ub, int t0, int t1, int64_t row0, int nrows, unsigned live) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int ti = t0 + wv; ti < t1; ti += OBS_THREADS / 64) {
    const ObsTask t = a.tasks[ti];
    for (int r0 = 0; r0 < nrows; r0 += OBS_ROWS_REG) {
      if (!((live >> r0) & ((1u << OBS_ROWS_REG) - 1u))) continue;      // (none of these rows is real: no walk over the entries)
      double acc[OBS_ROWS_REG];
#pragma unroll
      for (int c = 0; c < OBS_ROWS_REG; c++) acc[c] = 0.0;
      for (int e = lane; e < t.n; e += 64) {      // (n > 64: every lane has a first entry)
        const int i = a.idx[t.e0 + e];
        const double w = a.w[t.e0 + e];
#pragma unroll
        for (int c = 0; c < OBS_ROWS_REG; c++) {
          if (!((live >> (r0 + c)) & 1u)) continue;
          const double p = w * ub[(size_t)(r0 + c) * a.N + i];
          acc[c] = e == lane ? p : acc[c] + p;
        }
      }
#pragma unroll
      for (int c = 0; c < OBS_ROWS_REG; c++) {
        double v = acc[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);      // (wave_sum's order)
        if (lane == 0 && ((live >> (r0 + c)) & 1u)) obs_store<DEN>(a, t, row0, r0 + c, v);
      }
    }
  }
}

}  // namespace

template <bool STAGE>
__global__ __launch_bounds__(OBS_THREADS) void observables_kernel(ObsArgs a) {
  const int64_t row0 = (int64_t)blockIdx.x * a.rows;
  const int nrows = (int)min((int64_t)a.rows, a.rows_total - row0);
  // the rows of the workgroup that their segments really have (the same in every thread)
  unsigned live = 0;
  for (int r = 0; r < nrows; r++) {
    const int64_t seg = (row0 + r) / a.L, j = (row0 + r) % a.L;
    const long long n = a.seg_n ? a.seg_n[seg] : a.L;
    if (j < n) live |= 1u << r;
  }
  const double* ug = a.u + (size_t)row0 * (size_t)a.N;
  double* sh_u = obs_lds + OBS_ROWS_MAX * OBS_DEN_SLOTS;
  if (STAGE) {
    // slot c of a row: the elements 2c - head and 2c - head + 1, head = 1 for a row that starts 8 bytes off a 16-byte boundary
    const int per = a.N / 2 + 1;
    for (int t = threadIdx.x; t < nrows * per; t += OBS_THREADS) {
      const int r = t / per, c = t % per;
      if (!((live >> r) & 1u)) continue;
      const double* p = ug + (size_t)r * a.N;
      double* q = sh_u + (size_t)r * a.N;
      const int head = (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1u);
      const int lo = 2 * c - head, hi = lo + 1;
      if (lo >= 0 && hi < a.N) {
        const double2 v = *reinterpret_cast<const double2*>(p + lo);
        q[lo] = v.x; q[hi] = v.y;
      } else if (lo >= 0 && lo < a.N) {
        q[lo] = p[lo];
      } else if (lo < 0 && hi < a.N) {
        q[hi] = p[hi];
      }
    }
    __syncthreads();
  }
  const double* ub = STAGE ? sh_u : ug;

  // (live is the same in every thread; a workgroup without a real row goes straight to the zeros)
  for (int ph = 0; live != 0 && ph < a.n_phases; ph++) {
    const ObsPhase P = a.phases[ph];
    if (P.den_long > P.begin) {
      if (ph > 0) __syncthreads();      // (the outputs of the phase before have read the table)
      obs_short<true>(a, ub, P.begin, P.den_short, row0, nrows, live);
      obs_long<true>(a, ub, P.den_short, P.den_long, row0, nrows, live);
      __syncthreads();
    }
    obs_short<false>(a, ub, P.den_long, P.out_short, row0, nrows, live);
    obs_long<false>(a, ub, P.out_short, P.end, row0, nrows, live);
  }

  // the columns from G on, and every column of a row past its segment's end
  for (int r = 0; r < nrows; r++) {
    double* o = a.out + (size_t)(row0 + r) * (size_t)a.pitch;
    for (int c = (((live >> r) & 1u) ? a.G : 0) + (int)threadIdx.x; c < a.pitch; c += OBS_THREADS) o[c] = 0.0;
  }
}

ObsPlanHost observable_plan(const int64_t* form_ptr, const std::vector<int32_t>& idx0, const double* form_w, int64_t G,
                            const int64_t* num, const int64_t* den) {
  ObsPlanHost p;
  p.idx = idx0;
  p.w.assign(form_w, form_w + idx0.size());
  auto form_task = [&](int64_t f, int32_t slot, int32_t col) {
    return ObsTask{(int32_t)form_ptr[f], (int32_t)(form_ptr[f + 1] - form_ptr[f]), slot, col};
  };
  // the distinct denominator forms in the order the outputs first name them: table slot d % OBS_DEN_SLOTS of phase d / OBS_DEN_SLOTS
  std::map<int64_t, int32_t> slot_of;
  std::vector<int64_t> den_forms;
  for (int64_t g = 0; g < G; g++)
    if (den[g] >= 0 && slot_of.emplace(den[g], (int32_t)den_forms.size()).second) den_forms.push_back(den[g]);
  const int64_t n_ph = std::max<int64_t>(1, ceil_div((int64_t)den_forms.size(), OBS_DEN_SLOTS));
  std::vector<std::vector<ObsTask>> out_short((size_t)n_ph), out_long((size_t)n_ph);
  for (int64_t g = 0; g < G; g++) {      // (ascending g: a phase's tasks of one class are sorted by column)
    const int32_t d = den[g] >= 0 ? slot_of[den[g]] : -1;
    const ObsTask t = form_task(num[g], d < 0 ? -1 : d % OBS_DEN_SLOTS, (int32_t)g);
    (t.n <= OBS_SHORT_MAX ? out_short : out_long)[(size_t)(d < 0 ? 0 : d / OBS_DEN_SLOTS)].push_back(t);
  }
  for (int64_t ph = 0; ph < n_ph; ph++) {
    ObsPhase P{};
    P.begin = (int32_t)p.tasks.size();
    const int64_t d0 = ph * OBS_DEN_SLOTS, d1 = std::min<int64_t>(d0 + OBS_DEN_SLOTS, (int64_t)den_forms.size());
    for (int pass = 0; pass < 2; pass++) {
      for (int64_t d = d0; d < d1; d++) {
        const ObsTask t = form_task(den_forms[(size_t)d], -1, (int32_t)(d - d0));
        if ((t.n <= OBS_SHORT_MAX) == (pass == 0)) p.tasks.push_back(t);
      }
      (pass == 0 ? P.den_short : P.den_long) = (int32_t)p.tasks.size();
    }
    p.tasks.insert(p.tasks.end(), out_short[(size_t)ph].begin(), out_short[(size_t)ph].end());
    P.out_short = (int32_t)p.tasks.size();
    p.tasks.insert(p.tasks.end(), out_long[(size_t)ph].begin(), out_long[(size_t)ph].end());
    P.end = (int32_t)p.tasks.size();
    p.phases.push_back(P);
  }
  return p;
}

ObsLaunch observable_launch_plan(int64_t N) {
  const size_t row = (size_t)std::max<int64_t>(N, 1) * sizeof(double);
  int rows = OBS_ROWS_DEFAULT;
  if (const char* e = getenv("KIN_OBSERVABLES_ROWS")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= OBS_ROWS_MAX) rows = (int)v;
  }
  bool lds = row <= OBS_LDS_MAX_BYTES;
  if (const char* e = getenv("KIN_OBSERVABLES_LDS"))
    if (strcmp(e, "0") == 0) lds = false;      // (the one documented value; anything else leaves the choice alone)
  // fewer rows while they do not fit the share of LDS that leaves room for four workgroups per compute unit; a single row may
  // take more than that share
  if (lds) while (rows > 1 && (size_t)rows * row > OBS_LDS_ROWS_BYTES) rows--;
  return ObsLaunch{rows, lds};
}

void launch_observables(const ObsLaunch& plan, const ObsArgs& a, hipStream_t s) {
  if (a.rows_total == 0 || a.pitch == 0) return;
  ObsArgs b = a;
  b.rows = plan.rows;
  const unsigned grid = (unsigned)ceil_div(a.rows_total, plan.rows);
  const size_t table = (size_t)OBS_ROWS_MAX * OBS_DEN_SLOTS * sizeof(double);
  if (plan.lds) {
    // (rows N doubles, rounded up to 16 bytes)
    const size_t lds = table + (((size_t)plan.rows * (size_t)a.N * sizeof(double) + 15) & ~(size_t)15);
    KIN_HIP(hipFuncSetAttribute((const void*)observables_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(observables_kernel<true>, dim3(grid), dim3(OBS_THREADS), lds, s, b);
  } else {
    hipLaunchKernelGGL(observables_kernel<false>, dim3(grid), dim3(OBS_THREADS), table, s, b);
  }
  KIN_HIP(hipGetLastError());
}

}  // namespace kin
