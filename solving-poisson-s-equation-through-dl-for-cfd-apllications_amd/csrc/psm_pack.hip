// psm_pack.hip -- the image packs of the evaluators' frame batches: what a timeStep body does on the host between the mesh -> grid
// interpolation and the solve, per pixel and in its order -- NaN -> 0, the division by the channel's max_abs in float64, then the
// float32 cast of the solve's entry -- plus the frame's label / truth planes.  One IEEE division per value and no addition: nothing
// for the compiler to contract, so every output holds the bits of the NumPy statements (deltas: pressureSM_deltas/SM_call.py:439-445,
// :580; gradp: Eval_dual_Dense_onlycil.py:461-467; chapter4: M_u :215-225, M_fU :213-223).  Overloads of psm_to_grid_kernel by
// argument struct.  HBM-bound streams with one access pattern: frame blockIdx.y, a thread takes 4 consecutive pixels of every plane
// in 16-byte accesses where the frame's plane or image starts 16-byte aligned; else (odd plane sizes, shifted destinations, the tail)
// one access per element.  The values do not depend on the path.
// Shared: nan0, the 4-pixel load, the image store and the truth store.  The statements that fill the image floats stay with each
// kernel, and the Chapter-4 kernel keeps its image store written out: behind a common pack_image<C_IN> body the deltas and the gradP
// kernel compile to another instruction mix, and behind pack_store_image the C_IN = 2 kernel takes two more VGPRs
// (tools/kernel_isa_diff.py --same-work against the kernels as they were; profiles/r21_boundary_refactor.txt).
#include "psm_pack.h"

typedef float psm_pack_f4 __attribute__((ext_vector_type(4)));
typedef double psm_pack_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double nan0(double v) { return v != v ? 0.0 : v; }     // grid[np.isnan(grid)] = 0

__device__ __forceinline__ bool pack_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// pixels pix .. pix + 3 of plane p (n < 4 in the tail: the rest 0.0)
__device__ __forceinline__ void pack_load4(const double* p, int64_t pix, int n, double (&v)[4]) {
  if (n == 4 && pack_aligned(p)) {
    const psm_pack_d2 q0 = *reinterpret_cast<const psm_pack_d2*>(p + pix), q1 = *reinterpret_cast<const psm_pack_d2*>(p + pix + 2);
    v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = e < n ? p[pix + e] : 0.0;
}

// the 4 * C_IN image floats of a thread's pixels to go[0 .. C_IN * n)
template <int C_IN>
__device__ __forceinline__ void pack_store_image(float* go, const float (&g)[4 * C_IN], int n) {
  if (n == 4 && pack_aligned(go)) {
#pragma unroll
    for (int q = 0; q < C_IN; ++q) reinterpret_cast<psm_pack_f4*>(go)[q] = psm_pack_f4{g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]};
  } else {
    for (int e = 0; e < C_IN * n; ++e) go[e] = g[e];
  }
}

// 4 doubles of a truth plane to to[0 .. n)
__device__ __forceinline__ void pack_store_truth(double* to, const double (&t)[4], int n) {
  if (n == 4 && pack_aligned(to)) {
    reinterpret_cast<psm_pack_d2*>(to)[0] = psm_pack_d2{t[0], t[1]};
    reinterpret_cast<psm_pack_d2*>(to)[1] = psm_pack_d2{t[2], t[3]};
  } else {
    for (int e = 0; e < n; ++e) to[e] = t[e];
  }
}

// deltas: the label is the image's third plane once more, as float32 and, dimensional again, as the float64 truth -- two float64
// multiplications in a row, left to right.  The label plane is loaded whether or not an output asks for it.
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmDeltasPackArgs a) {
  const int64_t frame = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * PSM_DELTAS_PACK_SPAN + threadIdx.x * 4;
  if (pix >= a.npix) return;
  const int n = (int)min((int64_t)4, a.npix - pix);
  const double* pl = a.planes + frame * 3 * a.npix;
  double v0[4], v1[4], v2[4], sd[4];
  pack_load4(pl, pix, n, v0);
  pack_load4(pl + a.npix, pix, n, v1);
  pack_load4(pl + 2 * a.npix, pix, n, v2);
  pack_load4(a.sdn, pix, n, sd);
  float g[12], lb[4];
  double tr[4];
  const double u2 = a.truth ? a.u2[frame] : 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double x = nan0(v0[e]) / a.max_abs_ux, y = nan0(v1[e]) / a.max_abs_uy, p = nan0(v2[e]) / a.max_abs_p;
    g[3 * e] = (float)x; g[3 * e + 1] = (float)y; g[3 * e + 2] = (float)sd[e];
    lb[e] = (float)p;
    const double pm = p * a.max_abs_p;
    tr[e] = pm * u2;
  }
  pack_store_image<3>(a.grid + (frame * a.npix + pix) * 3, g, n);
  if (a.label) {
    float* lo = a.label + frame * a.npix + pix;
    if (n == 4 && pack_aligned(lo)) *reinterpret_cast<psm_pack_f4*>(lo) = psm_pack_f4{lb[0], lb[1], lb[2], lb[3]};
    else for (int e = 0; e < n; ++e) lo[e] = lb[e];
  }
  if (a.truth) pack_store_truth(a.truth + frame * a.npix + pix, tr, n);
}

hipError_t psm_launch_deltas_pack(const PsmDeltasPackArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.npix < 1 || !a.planes || !a.sdn || !a.grid || (a.truth && !a.u2)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmDeltasPackArgs)>(psm_to_grid_kernel),
                     dim3((unsigned)((a.npix + PSM_DELTAS_PACK_SPAN - 1) / PSM_DELTAS_PACK_SPAN), (unsigned)a.n_frames), dim3(256), 0, st, a);
  return hipGetLastError();
}

// gradp: the label channels 3-5 stay float64, the pressure label undivided
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmGradpPackArgs a) {
  const int64_t frame = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * PSM_DELTAS_PACK_SPAN + threadIdx.x * 4;
  if (pix >= a.npix) return;
  const int n = (int)min((int64_t)4, a.npix - pix);
  const double* pl = a.planes + frame * 5 * a.npix;
  double v0[4], v1[4], sd[4];
  pack_load4(pl, pix, n, v0);
  pack_load4(pl + a.npix, pix, n, v1);
  pack_load4(a.sdn, pix, n, sd);
  float g[12];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double x = nan0(v0[e]) / a.m0, y = nan0(v1[e]) / a.m1;
    g[3 * e] = (float)x; g[3 * e + 1] = (float)y; g[3 * e + 2] = (float)sd[e];
  }
  pack_store_image<3>(a.grid + (frame * a.npix + pix) * 3, g, n);
  if (!a.truth) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double mc = c == 0 ? a.m3 : c == 1 ? a.m4 : 1.0;
    double v[4], t[4];
    pack_load4(pl + (2 + c) * a.npix, pix, n, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = c < 2 ? nan0(v[e]) / mc : nan0(v[e]);
    pack_store_truth(a.truth + (frame * 3 + c) * a.npix + pix, t, n);
  }
}

hipError_t psm_launch_gradp_pack(const PsmGradpPackArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.npix < 1 || !a.planes || !a.sdn || !a.grid) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmGradpPackArgs)>(psm_to_grid_kernel),
                     dim3((unsigned)((a.npix + PSM_DELTAS_PACK_SPAN - 1) / PSM_DELTAS_PACK_SPAN), (unsigned)a.n_frames), dim3(256), 0, st, a);
  return hipGetLastError();
}

// chapter4: C_IN is the image width (M_u 3, M_fU 2), a template parameter so that the 4 * C_IN image floats of a thread go out as
// C_IN 16-byte stores; the pressure label, plane C_IN - 1, stays float64
template <int C_IN>
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmChapter4PackArgs a) {
  const int64_t frame = blockIdx.y;
  const int64_t pix = (int64_t)blockIdx.x * PSM_DELTAS_PACK_SPAN + threadIdx.x * 4;
  if (pix >= a.npix) return;
  const int n = (int)min((int64_t)4, a.npix - pix);
  const double* pl = a.planes + frame * C_IN * a.npix;
  float g[4 * C_IN];
#pragma unroll
  for (int c = 0; c < C_IN - 1; ++c) {
    double v[4];
    pack_load4(pl + c * a.npix, pix, n, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[C_IN * e + c] = (float)(nan0(v[e]) / a.m[c]);
  }
  {
    double sd[4];
    pack_load4(a.sdn, pix, n, sd);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[C_IN * e + C_IN - 1] = (float)sd[e];
  }
  float* go = a.grid + (frame * a.npix + pix) * C_IN;
  if (n == 4 && pack_aligned(go)) {
#pragma unroll
    for (int q = 0; q < C_IN; ++q) reinterpret_cast<psm_pack_f4*>(go)[q] = psm_pack_f4{g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]};
  } else {
    for (int e = 0; e < C_IN * n; ++e) go[e] = g[e];
  }
  if (!a.truth) return;
  double v[4], t[4];
  pack_load4(pl + (C_IN - 1) * a.npix, pix, n, v);
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = nan0(v[e]) / a.m_p;
  pack_store_truth(a.truth + frame * a.npix + pix, t, n);
}

hipError_t psm_launch_chapter4_pack(const PsmChapter4PackArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.npix < 1 || !a.planes || !a.sdn || !a.grid || (a.c_in != 2 && a.c_in != 3)) return hipErrorInvalidValue;
  const dim3 wgs((unsigned)((a.npix + PSM_DELTAS_PACK_SPAN - 1) / PSM_DELTAS_PACK_SPAN), (unsigned)a.n_frames);
  if (a.c_in == 3) hipLaunchKernelGGL(static_cast<void (*)(PsmChapter4PackArgs)>(psm_to_grid_kernel<3>), wgs, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(static_cast<void (*)(PsmChapter4PackArgs)>(psm_to_grid_kernel<2>), wgs, dim3(256), 0, st, a);
  return hipGetLastError();
}
