// psm_mesh_dev.h -- device-side helpers that the mesh ends of every path share (psm_mesh.hip: the PCA paths; psm_unet_mesh.hip: the
// convolutional path): U_max out of a row of partial maxima, and the NumPy-exact add of the delta tails.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double sqrt_rn(double x) {
  double r = sqrt(x);
  const unsigned long long eb = __double_as_longlong(r) & 0x7ff0000000000000ull;
  if (eb > (53ull << 52) && eb < 0x7ff0000000000000ull) {                       // normal, finite, not NaN
    const double u = __longlong_as_double(eb - (52ull << 52));                  // ulp(r)
    const double e = fma(-r, r, x);                                             // x - r^2, exact
    const double lim = r * u;                                                   // |sqrt(x) - r| <= u / 2  <=>  |e| <= r u (to 2nd order)
    if (e > lim) r += u; else if (e < -lim) r -= u;
  }
  return r;
}

// np.max semantics on doubles: NaN propagates
__device__ __forceinline__ double nanmax2(double a, double b) { return (b > a || b != b) ? b : a; }

// U_max from a row of <= 256 partial maxima of the SQUARED speed, folded by every thread of a 256-thread workgroup: sqrt_rn last
__device__ __forceinline__ double umax_of_partials(const double* partials, int n_partials) {
  __shared__ double um_s[4];
  double m = partials[min((int)threadIdx.x, n_partials - 1)];
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) um_s[threadIdx.x >> 6] = m;
  __syncthreads();
  return sqrt_rn(nanmax2(nanmax2(um_s[0], um_s[1]), nanmax2(um_s[2], um_s[3])));
}

// p(t-1) + dp as NumPy adds them: one rounding, never folded into the multiplications in front of it
__device__ __forceinline__ double add_np(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
typedef double psm_uv2 __attribute__((ext_vector_type(2)));   // one row of u_prev [N][2]: 16 bytes, 16-byte aligned
