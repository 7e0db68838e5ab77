// psm_rows.h -- launchers of the "rows -> scalars + columns" stage in front of the evaluators' frame steps (see psm_rows.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the recipes (PSM_ROWS_* of include/psm.h) and their column counts
constexpr int PSM_ROWS_KIND_DELTAS = 0, PSM_ROWS_KIND_POISSON = 1, PSM_ROWS_KIND_GRADP = 2;
constexpr int PSM_ROWS_PARTS = 256;           // capacity of one frame's row of partial maxima: every finish workgroup folds a row
constexpr int PSM_ROWS_CHUNK = 256;           // cells per workgroup and pass (one per thread)
constexpr int PSM_ROWS_SCALARS = 8;           // doubles per frame in `scalars`
inline int psm_rows_cols(int kind) { return kind == PSM_ROWS_KIND_DELTAS ? 3 : kind == PSM_ROWS_KIND_POISSON ? 8 : kind == PSM_ROWS_KIND_GRADP ? 5 : 0; }
inline int psm_rows_min_width(int kind) { return kind == PSM_ROWS_KIND_GRADP ? 8 : 11; }
inline int psm_rows_parts(int64_t n_cells) {
  const int64_t c = (n_cells + PSM_ROWS_CHUNK - 1) / PSM_ROWS_CHUNK;
  return (int)(c < 1 ? 1 : c > PSM_ROWS_PARTS ? PSM_ROWS_PARTS : c);
}

struct PsmRowsArgs {
  const float* rows;            // [n_frames][n_cells][width] the dataset frame cut at `indice`, float32 as stored
  float* part;                  // [n_frames][3][n_parts] partial maxima (U, dU, c)
  double* cols;                 // [n_frames][n_cells][k] the columns the frame entries take
  double* scalars;              // [n_frames][8]: U, dU, c, relevant, U^2, out-scale, 0, 0
  // where the step's kernels read the frame's scalars (each nullptr: not written)
  float* row_scale;             // [n_frames * B] the decode's row scale
  double* u2;                   // [n_frames] the deltas pack's U^2
  double* lu;                   // [n_frames][2] (L, U) of the feature launches
  int64_t n_cells;
  double base, phi;             // out-scale = base U^2; L of the features
  float ex, ey;                 // gradP: max_x - min_x, max_y - min_y (float32, as EvaluationGradP holds them)
  int width, kind, n_frames, n_parts, B;
};
hipError_t psm_launch_rows_partial(const PsmRowsArgs& a, hipStream_t st);
hipError_t psm_launch_rows_finish(const PsmRowsArgs& a, hipStream_t st);
