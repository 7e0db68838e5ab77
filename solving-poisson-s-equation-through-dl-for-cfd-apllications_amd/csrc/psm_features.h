// psm_features.h -- launcher of the pressureSM_Poisson input features (see psm_features.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// ---- pressureSM_Poisson input features (SMP:588-711), case-batched: one launch per stage, see psm_features.hip
struct PsmFeatureArgs {
  const double *ux, *uy, *dux, *duy, *sdf;   // case 0: [ny][nx] float64 (dimensional grids, zero outside the flow; raw SDF)
  double* term;                              // [n_cases][ny][nx] scratch: the Poisson source term
  double* partial;                           // [n_cases][2 * workgroups per case] (sum, sum of squares)
  float* grid;                               // [n_cases][ny][nx][4] float32 NHWC
  int ny, nx;
  double L, U, k;                            // L, U: read when lu == nullptr (the host entry's single case)
  double max_abs[4];                         // Poisson_term_1, delta_Ux, delta_Uy, dist
  const double* lu;                          // [n_cases][2] (L, U) per case in device memory: a captured launch reads new values on replay
  int n_cases;                               // launch dimension y; 0 counts as 1
  int64_t vel_stride, sdf_stride;            // doubles from one case's velocity planes / SDF plane to the next case's
};
hipError_t psm_launch_poisson_features(const PsmFeatureArgs& a, hipStream_t st);
