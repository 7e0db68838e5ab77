// psm_trust.h -- launchers of the input-trust score (see psm_trust.hip): per block row of the last solve the squared norm of the
// centred input block and the reconstruction residual of its PCA round trip (the SPE / Q statistic), both float64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#define PSM_TRUST_BAND_ROWS 8      // block rows one workgroup of the norm launch sums
#define PSM_TRUST_MAX_P 1024       // p_in the finish launch holds in LDS
#define PSM_TRUST_MAX_K 65536      // S * S * c_in of the basis

inline int psm_trust_bands(int S) { return (S + PSM_TRUST_BAND_ROWS - 1) / PSM_TRUST_BAND_ROWS; }

// G = C C^T in float64 from the natural-order float32 basis comp [P][K]; gram [P][P].  Once per bind.
struct PsmTrustGramArgs { const float* comp; double* gram; int P, K; };
hipError_t psm_launch_trust_gram(const float* comp, double* gram, int P, int K, hipStream_t st);

// sum_k (x_k - mu_k)^2 over a band of rows of one block of one case: part [n_cases][B][bands]
struct PsmTrustNormArgs {
  const float* grid;               // [n_cases][Ny][Nx][c_in] the image the last solve ran on
  const float* mean;               // [S][S][c_in] natural order
  const int32_t* blk_y0x0;         // [B][2] block origins
  double* part;                    // [n_cases][B][bands]
  int S, c_in, Nx, B, bands, n_cases;
  int64_t case_stride;             // floats from one case's image to the next
  int aligned;                     // every band row of the image and of the mean starts on 16 bytes and holds whole float4
};
hipError_t psm_launch_trust_norm(const PsmTrustNormArgs& a, hipStream_t st);

// (n, spe) per block row m = case * B + b: out [n_cases * B][2]
struct PsmTrustFinishArgs {
  const double* part;              // [M][bands]
  const float* xin;                // [Mpad][ld_in] the scaled coefficients the encode left
  const float *ia, *ib;            // [ld_in] the model's input scaler: xin = z * ia + ib
  const double* gram;              // [P][P]
  double* out;                     // [M][2]
  int M, bands, P, ld_in;
};
hipError_t psm_launch_trust_finish(const PsmTrustFinishArgs& a, hipStream_t st);
