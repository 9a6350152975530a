// Observables of stored states (observable_kernels.hip; entry points: observable_api.cpp; definitions:
// include/kinetica_hip.h): per row H linear forms over the species and G outputs built from them - a form, or the ratio of
// two - written in the species' place, pitch doubles per row.
#pragma once
#include <cstdint>
#include <vector>

#include "common.hpp"

namespace kin {

constexpr int OBS_SHORT_MAX = 64;         // terms of a short form: one sequential sum; longer forms: 64 chains and the butterfly
constexpr int OBS_ROWS_MAX = 16;          // rows a workgroup keeps
constexpr int OBS_ROWS_DEFAULT = 4;
constexpr int OBS_ROWS_REG = 4;           // rows whose sums a lane carries through one walk over a form's entries
constexpr int OBS_THREADS = 256;
constexpr int OBS_DEN_SLOTS = 64;         // denominator forms whose values a workgroup keeps per row and phase
constexpr size_t OBS_LDS_ROWS_BYTES = (size_t)32 << 10;    // the rows of a workgroup where several fit: four workgroups per CU
constexpr size_t OBS_LDS_MAX_BYTES = (size_t)128 << 10;    // one row at the most: beyond it the gather path

// One task: the form entries e0 .. e0 + n - 1 evaluated for every row of the workgroup. In a denominator stage the value goes
// to slot `col` of the row's table; in an output stage it is divided by slot `den` of that table (den < 0: as it is) and goes to
// column `col` of the row.
struct ObsTask { int32_t e0, n, den, col; };

// One phase: the tasks [begin, den_short) are short denominator forms, [den_short, den_long) long ones, then after a barrier
// [den_long, out_short) short outputs and [out_short, end) long outputs. The next phase begins at `end`.
struct ObsPhase { int32_t begin, den_short, den_long, out_short, end; };

// The plan of a call on the host: the forms' entries 0-based, the tasks and the phases. Observables are dealt to phases by the
// table slot of their denominator (OBS_DEN_SLOTS distinct denominator forms per phase; outputs without one go to phase 0),
// inside a phase by the class of their numerator and then by column, so that the stores of a row coalesce.
struct ObsPlanHost {
  std::vector<int32_t> idx;
  std::vector<double> w;
  std::vector<ObsTask> tasks;
  std::vector<ObsPhase> phases;
};
ObsPlanHost observable_plan(const int64_t* form_ptr, const std::vector<int32_t>& idx0, const double* form_w, int64_t G,
                            const int64_t* num, const int64_t* den);

struct ObsArgs {
  int N, L, G, pitch;
  int64_t rows_total;             // S L
  int rows;                       // rows of a workgroup
  int n_phases;
  const int64_t* seg_n;           // rows a segment really has (null: L)
  const double* u;                // [S][L][N]
  const int32_t* idx;             // the forms' entries
  const double* w;
  const ObsTask* tasks;
  const ObsPhase* phases;
  double* out;                    // [S][L][pitch]
};

// How the launcher cuts the work: `rows` consecutive rows of the flat (s, j) axis per workgroup, staged into LDS or (lds false)
// gathered from global memory. Results do not depend on either; KIN_OBSERVABLES_ROWS (1 .. 16) and KIN_OBSERVABLES_LDS=0
// (read per call: tests change them) force them.
struct ObsLaunch { int rows; bool lds; };
ObsLaunch observable_launch_plan(int64_t N);

// one launch over S L rows: S L >= 1, pitch >= 1, S L < 2^31, N, pitch, the entries and the tasks below 2^31
void launch_observables(const ObsLaunch& plan, const ObsArgs& a, hipStream_t s);

}  // namespace kin
