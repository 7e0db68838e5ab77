// psm_filter.h -- launcher of the Gaussian post-steps (see psm_filter.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// ---- Gaussian post-steps (SMD:353-363, UGP:366-367), case-batched: one launch per separable pass, see psm_filter.hip
struct PsmGaussJob {
  const float* in;           // [n_cases][ny][nx][c]
  const float* w;            // [2 * radius + 1] normalised taps
  int radius;
};
struct PsmGaussArgs {
  PsmGaussJob job[2];        // axis 0: n_jobs independent inputs (blockIdx.z); axis 1 with epilogue 1: field (in == nullptr: not filtered) and weighting input
  float* out[2];             // axis 0: one per job; axis 1 without an epilogue: out[0]
  const float* prev;         // epilogues 1 and 2: [n_cases][ny][nx]
  const float* fields;       // epilogue 1 without job 0: the unfiltered field
  float* result; float* t;   // epilogue 1: result (may be nullptr), t = (result - prev) * w
  float* change; float* next;   // epilogue 2: either may be nullptr
  int ny, nx, c, n_cases, n_jobs;
  int tap_chunk;             // taps staged at a time (psm_gauss_tap_chunk of the widest table of the launch)
  int tiles_x;               // set by the launcher
};
void psm_gauss_init();
int psm_gauss_tap_chunk(int max_radius);
// axis 0: along y, no epilogue.  axis 1: along x, epilogue 0 (none), 1 or 2 (c == 1 only)
hipError_t psm_launch_gauss(PsmGaussArgs a, int axis, int epi, hipStream_t st);
