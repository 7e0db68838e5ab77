// psm_trust.hip -- the input-trust score of the last solve (psm_bind_trust / psm_trust_last*, psm_api_trust.cpp): per block row
//   n   = sum_k (x_k - mu_k)^2                      the centred input block, float32 image and mean, summed in float64
//   spe = n - 2 sum_p z_p^2 + z^T G z               with G = C C^T and z the coefficients the encode of that solve left in ws0.d_xin,
//                                                     the model's input scaler undone: |x - mu - C^T z|^2 at z = C (x - mu), any basis C
// Three kernels, launchers in psm_trust.h: the Gram matrix once per bind (gram), then per call a reduction over the image (norm:
// band partials) and one workgroup per block row that finishes both values (finish).  Like the error-sum kernels of psm_eval.hip
// they are overloads of psm_block_error_kernel, the library's family of per-block evaluation sums, told apart by their argument
// struct (PsmTrustGramArgs / PsmTrustNormArgs / PsmTrustFinishArgs): a trace shows them under that name with the struct's.
// Float64 throughout, no atomics, every sum one fixed tree (thread -> lane -> wave -> workgroup -> band): the same solve gives the
// same bits on every call.
#include "psm_trust.h"

namespace {

// 64 lanes -> lane 0, then the four waves of a 256-thread workgroup in wave order; the total is valid in thread 0
__device__ __forceinline__ double fold_workgroup(double v, double* sw) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int t = threadIdx.x;
  if ((t & 63) == 0) sw[t >> 6] = v;
  __syncthreads();
  return (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

}  // namespace

// G[p][q] = sum_k C[p][k] C[q][k]: a 32 x 32 tile per workgroup, 2 x 2 entries per thread, the K range staged through LDS 32 columns
// at a time.  A product of two float32 is exact in float64 and every entry sums its products in k order, so G is symmetric to the bit.
// Bind time only: not tuned (p_in = 128, K = 49152: 16 tiles x 8e8 multiply-adds).
__global__ __launch_bounds__(256) void psm_block_error_kernel(PsmTrustGramArgs a) {
  constexpr int T = 32, KC = 32;
  const float* __restrict__ comp = a.comp;
  double* __restrict__ gram = a.gram;
  const int P = a.P, K = a.K;
  __shared__ float sa[T][KC + 1], sb[T][KC + 1];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int p0 = blockIdx.y * T, q0 = blockIdx.x * T;
  double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = t & 31, k = k0 + kc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (t >> 5) + 8 * i;
      sa[r][kc] = (p0 + r < P && k < K) ? comp[(int64_t)(p0 + r) * K + k] : 0.f;
      sb[r][kc] = (q0 + r < P && k < K) ? comp[(int64_t)(q0 + r) * K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < KC; ++kk) {
      const double a0 = sa[ty][kk], a1 = sa[ty + 16][kk], b0 = sb[tx][kk], b1 = sb[tx + 16][kk];
      g00 += a0 * b0; g01 += a0 * b1; g10 += a1 * b0; g11 += a1 * b1;
    }
    __syncthreads();
  }
  const int p = p0 + ty, q = q0 + tx;
  if (p < P && q < P) gram[(int64_t)p * P + q] = g00;
  if (p < P && q + 16 < P) gram[(int64_t)p * P + q + 16] = g01;
  if (p + 16 < P && q < P) gram[(int64_t)(p + 16) * P + q] = g10;
  if (p + 16 < P && q + 16 < P) gram[(int64_t)(p + 16) * P + q + 16] = g11;
}

hipError_t psm_launch_trust_gram(const float* comp, double* gram, int P, int K, hipStream_t st) {
  if (P < 1 || P > PSM_TRUST_MAX_P || K < 1 || K > PSM_TRUST_MAX_K) return hipErrorInvalidValue;
  const int tiles = (P + 31) / 32;
  hipLaunchKernelGGL(psm_block_error_kernel, dim3(tiles, tiles), dim3(256), 0, st, PsmTrustGramArgs{comp, gram, P, K});
  return hipGetLastError();
}

// Grid (B, bands, cases): a workgroup sums (x - mu)^2 over PSM_TRUST_BAND_ROWS rows of one block.  A block row is S * c_in
// consecutive floats of the image ([r][c][ch], the column order of comp_in) and of the mean: lanes read consecutive addresses,
// 16 bytes each where the plan's origins allow it.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void psm_block_error_kernel(PsmTrustNormArgs a) {
  const int b = blockIdx.x, band = blockIdx.y, cs = blockIdx.z, t = threadIdx.x;
  const int y0 = a.blk_y0x0[2 * b], x0 = a.blk_y0x0[2 * b + 1];
  const int W = a.S * a.c_in;
  const int r0 = band * PSM_TRUST_BAND_ROWS, r1 = min(r0 + PSM_TRUST_BAND_ROWS, a.S);
  const float* img = a.grid + (int64_t)cs * a.case_stride;
  double acc = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float* xr = img + ((int64_t)(y0 + r) * a.Nx + x0) * a.c_in;
    const float* mr = a.mean + (int64_t)r * W;
    if (ALIGNED) {
      for (int j = 4 * t; j < W; j += 1024) {
        const float4 x = *reinterpret_cast<const float4*>(xr + j), m = *reinterpret_cast<const float4*>(mr + j);
        const double d0 = (double)x.x - (double)m.x, d1 = (double)x.y - (double)m.y, d2 = (double)x.z - (double)m.z, d3 = (double)x.w - (double)m.w;
        acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
      }
    } else {
      for (int j = t; j < W; j += 256) {
        const double d = (double)xr[j] - (double)mr[j];
        acc += d * d;
      }
    }
  }
  __shared__ double sw[4];
  const double total = fold_workgroup(acc, sw);
  if (t == 0) a.part[((int64_t)cs * a.B + b) * a.bands + band] = total;
}

hipError_t psm_launch_trust_norm(const PsmTrustNormArgs& a, hipStream_t st) {
  if (a.B < 1 || a.n_cases < 1 || a.n_cases > 65535 || a.bands != psm_trust_bands(a.S) || a.bands > 65535) return hipErrorInvalidValue;
  const dim3 grid(a.B, a.bands, a.n_cases);
  if (a.aligned) {
    if ((a.S * a.c_in) % 4 != 0 || ((reinterpret_cast<uintptr_t>(a.grid) | reinterpret_cast<uintptr_t>(a.mean)) & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(psm_block_error_kernel<true>, grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(psm_block_error_kernel<false>, grid, dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

// One workgroup per block row: the band partials in band order, z = (xin - ib) / ia in float64, then sum z^2 and z^T G z -- thread p
// walks column p of G (= its row p: lanes read consecutive addresses) against z in LDS.  n == 0 stores spe = 0; nothing is clamped.
__global__ __launch_bounds__(256) void psm_block_error_kernel(PsmTrustFinishArgs a) {
  __shared__ double z[PSM_TRUST_MAX_P];
  __shared__ double sw[2][4];
  const int m = blockIdx.x, t = threadIdx.x;
  for (int p = t; p < a.P; p += 256) z[p] = ((double)a.xin[(int64_t)m * a.ld_in + p] - (double)a.ib[p]) / (double)a.ia[p];
  __syncthreads();
  double zz = 0.0, zgz = 0.0;
  for (int p = t; p < a.P; p += 256) {
    double s = 0.0;
    for (int q = 0; q < a.P; ++q) s += a.gram[(int64_t)q * a.P + p] * z[q];
    zz += z[p] * z[p];
    zgz += z[p] * s;
  }
  const double ZZ = fold_workgroup(zz, sw[0]), ZGZ = fold_workgroup(zgz, sw[1]);
  if (t == 0) {
    double n = 0.0;
    for (int k = 0; k < a.bands; ++k) n += a.part[(int64_t)m * a.bands + k];
    a.out[2 * (int64_t)m] = n;
    a.out[2 * (int64_t)m + 1] = n == 0.0 ? 0.0 : n - 2.0 * ZZ + ZGZ;
  }
}

hipError_t psm_launch_trust_finish(const PsmTrustFinishArgs& a, hipStream_t st) {
  if (a.M < 1 || a.P < 1 || a.P > PSM_TRUST_MAX_P || a.P > a.ld_in || a.bands < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(psm_block_error_kernel, dim3(a.M), dim3(256), 0, st, a);
  return hipGetLastError();
}
