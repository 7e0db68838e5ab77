// psm_mesh.hip -- mesh <-> uniform-grid ends of the per-step call:
// the solver hands over cells[N,5] = (Ux, Uy, Cx, Cy, p) in float64 (PythonComm.H:2-9) and
// reads back p[N] float64 (PythonComm.H:31-36).
//
//   umax     : U_max = max sqrt(Ux^2 + Uy^2)                               [PM:270]
//   to_grid  : barycentric mesh->grid interpolation, scatter into the image, normalisation,
//              SDF channel, NaN -> 0                                        [PM:272-297]
//   to_mesh  : gather at `indices`, barycentric grid->mesh interpolation with fill,
//              dimensionalise, near-wall / NaN fallback to the previous p   [PM:481-496]
//
// All of them are HBM-bound gathers; interpolation is done in float64 like the reference.
#include "psm_mesh.h"

#include <algorithm>

// U_max = max sqrt(Ux^2 + Uy^2) as NumPy takes it (PM:270), bit for bit, and bit for bit what the host pass of psm_solve takes
// (psm_api_mesh.cpp: max of the squares, one sqrt).  Found by tests/test_embed_host.py (round 6): the device reduction and the host
// pass gave U_max one ulp apart on 2 of 7 velocity scales -- and with it every pressure of those steps -- because hipcc contracts
// ux * ux + uy * uy into an fma in device code.  The squares and their sum are computed under `fp contract(off)`; the kernels
// reduce the SQUARED speed like the host does and take one square root at the end (sqrt_rn: the device's sqrt with a
// round-to-nearest correction from the exact residual -- a guard, no last-bit difference of sqrt itself was observed).
__device__ __forceinline__ double speed2_np(double ux, double uy) {
#pragma clang fp contract(off)               // (__dmul_rn / __dadd_rn are plain operators in this toolchain's headers and get contracted too)
  const double xx = ux * ux, yy = uy * uy;
  return xx + yy;
}
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

__global__ __launch_bounds__(1024) void psm_umax_kernel(const double* cells, int64_t n, double* umax) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m = 0.0;
  for (int64_t i = tid; i < n; i += 1024) {
    const double ux = cells[i * 5], uy = cells[i * 5 + 1];
    const double v = speed2_np(ux, uy);
    m = (v > m || v != v) ? v : m;          // np.max propagates NaN
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_down(m, o, 64);
    m = (other > m || other != other) ? other : m;
  }
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) {
    double r = red[0];
    for (int w = 1; w < 16; ++w) r = (red[w] > r || red[w] != red[w]) ? red[w] : r;
    *umax = sqrt_rn(r);
  }
}

// np.max semantics on doubles: NaN propagates
__device__ __forceinline__ double nanmax2(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(const double* cells, int64_t n, double* partials) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + tid; i < n; i += (int64_t)gridDim.x * 1024) {
    const double ux = cells[i * 5], uy = cells[i * 5 + 1];
    m = nanmax2(m, speed2_np(ux, uy));
  }
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) {
    double r = red[0];
    for (int w = 1; w < 16; ++w) r = nanmax2(r, red[w]);
    partials[blockIdx.x] = r;
  }
}

// First kernel of the one-graph psm_solve (registered caller buffers): reads the solver's cells[N,5] array STRAIGHT from host
// memory (the device-side address of the registered pages) -- every row requested at once over PCIe, no DMA-engine copy and no
// copy -> kernel dependency in front of the first kernel --, stores it to the device copy the gathers read, and takes the
// per-workgroup partial maxima of sqrt(Ux^2 + Uy^2) on the way (PM:270; reduced by every psm_to_grid workgroup).
typedef double psm_d2 __attribute__((ext_vector_type(2)));
// A workgroup owns 512 rows = 20480 bytes = 1280 16-byte pieces, five per thread, all five requested up front as fully
// coalesced 16-byte loads (a wave reads 1 KB of consecutive host memory per instruction: whole PCIe read requests, each line
// asked for once); the pieces go to the device copy from the registers and through LDS to the threads that own the rows'
// (Ux, Uy) for the maximum.  ALIGNED = false (a host array that is not 16-byte aligned): 8-byte pieces, same structure.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void psm_stage_cells_kernel(const double* host_cells, double* cells, int64_t n, double* partials) {
  constexpr int ROWS = 512, NP = ROWS * 5 / 2 / 256;        // 5 pieces of 16 bytes per thread
  __shared__ double row[ROWS * 5];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t dn = n * 5, n_chunks = (n + ROWS - 1) / ROWS;              // in doubles; chunks of 512 rows
  double m = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {  // more than 256 chunks (131 072 cells): a second round
    const int64_t d0 = chunk * ROWS * 5;
    if (ALIGNED) {
      psm_d2 v[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int64_t e = d0 + 2 * (int64_t)(j * 256 + tid);
        v[j] = (e + 1 < dn) ? __builtin_nontemporal_load(reinterpret_cast<const psm_d2*>(host_cells + e))
                            : (psm_d2){e < dn ? __builtin_nontemporal_load(host_cells + e) : 0.0, 0.0};
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int64_t e = d0 + 2 * (int64_t)(j * 256 + tid);
        const int l = 2 * (j * 256 + tid);
        row[l] = v[j].x; row[l + 1] = v[j].y;
        if (e + 1 < dn) *reinterpret_cast<psm_d2*>(cells + e) = v[j];
        else if (e < dn) cells[e] = v[j].x;
      }
    } else {
      double v[2 * NP];
#pragma unroll
      for (int j = 0; j < 2 * NP; ++j) {
        const int64_t e = d0 + (int64_t)(j * 256 + tid);
        v[j] = e < dn ? __builtin_nontemporal_load(host_cells + e) : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 2 * NP; ++j) {
        const int64_t e = d0 + (int64_t)(j * 256 + tid);
        row[j * 256 + tid] = v[j];
        if (e < dn) cells[e] = v[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROWS / 256; ++k) {
      const int r = k * 256 + tid;
      if (chunk * ROWS + r < n) {
        const double ux = row[r * 5], uy = row[r * 5 + 1];
        m = nanmax2(m, speed2_np(ux, uy));
      }
    }
    __syncthreads();                                         // the rows are consumed: the next round may overwrite them
  }
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) partials[blockIdx.x] = nanmax2(nanmax2(red[0], red[1]), nanmax2(red[2], red[3]));
}

hipError_t psm_launch_stage_cells(const double* host_cells, double* cells, int64_t n, double* partials, int* n_partials, hipStream_t st) {
  if (n < 1) return hipErrorInvalidValue;
  const int64_t wgs = std::min<int64_t>(256, (n + 511) / 512);   // the partials array holds 256: larger meshes take further rounds
  *n_partials = (int)wgs;
  const bool aligned = ((reinterpret_cast<uintptr_t>(host_cells) | reinterpret_cast<uintptr_t>(cells)) & 15) == 0;
  if (aligned) hipLaunchKernelGGL(psm_stage_cells_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, st, host_cells, cells, n, partials);
  else hipLaunchKernelGGL(psm_stage_cells_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, st, host_cells, cells, n, partials);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmToGridArgs a) {
  __shared__ double um_s[4];
  double umax_v = a.umax ? *a.umax : a.umax_val;
  if (a.umax_partials) {                      // uniform: every workgroup reduces the <= 256 partial maxima itself
    double m = a.umax_partials[min((int)threadIdx.x, a.n_partials - 1)];
    for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) um_s[threadIdx.x >> 6] = m;
    __syncthreads();
    umax_v = sqrt_rn(nanmax2(nanmax2(um_s[0], um_s[1]), nanmax2(um_s[2], um_s[3])));      // the partials are maxima of the SQUARED speed
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.umax_out = umax_v;
  }
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.n_grid) return;
  const int src = a.src_of_cell[cell];     // grid point whose value lands in this cell (-1: never written -> 0)
  float ux = 0.f, uy = 0.f;
  if (src >= 0) {
    const double inv = 1.0 / umax_v;
    const int32_t* v = a.vtx + (int64_t)src * 3;
    const double* w = a.wts + (int64_t)src * 3;
    double sx = 0.0, sy = 0.0;
    bool neg = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* c = a.cells + (int64_t)v[j] * 5;
      sx += (c[0] * inv) * w[j];           // interpolate(Ux / U_max)  (PM:272,280)
      sy += (c[1] * inv) * w[j];
      neg = neg || (w[j] < 0.0);
    }
    if (a.fill && neg) { sx = NAN; sy = NAN; }   // interpolate_fill (SMD:421-423): NaN, then NaN -> 0
    sx /= a.max_abs_ux;                    // PM:290-291
    sy /= a.max_abs_uy;
    ux = (sx != sx) ? 0.f : (float)sx;     // grid[np.isnan(grid)] = 0  (PM:297)
    uy = (sy != sy) ? 0.f : (float)sy;
  }
  const double sd = a.sdf[cell] * a.sdf_scale;   // PM:292 (raw) / SMD:443 (divided by max_abs_dist)
  float* g = a.grid + cell * a.c_in;
  g[0] = ux;
  g[1] = uy;
  g[2] = (sd != sd) ? 0.f : (float)sd;
}

__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmToMeshArgs a) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_cells) return;
  const int32_t* v = a.vtx + n * 3;
  const double* w = a.wts + n * 3;
  double acc = 0.0;
  bool neg = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int cell = a.cell_of_point[v[j]];                         // p_adim_unif = result[indices]  (PM:481)
    acc += (double)a.field[(int64_t)cell * a.c_out] * w[j];
    neg = neg || (w[j] < 0.0);
  }
  const double um = a.umax ? *a.umax : a.umax_val;
  double p = acc * a.max_abs_p * (um * um);                         // PM:490
  const double prev = a.cells[n * 5 + 4];
  if (a.near_wall[n] || neg || acc != acc) p = prev;                // PM:494, 496 (interpolate_fill -> NaN)
  a.p_out[n] = p;
}

hipError_t psm_launch_umax_partial(const double* cells, int64_t n, double* partials, int* n_partials, hipStream_t st) {
  const int nwg = (int)std::min<int64_t>(256, (n + 4095) / 4096);
  *n_partials = nwg;
  hipLaunchKernelGGL(psm_umax_partial_kernel, dim3(nwg), dim3(1024), 0, st, cells, n, partials);
  return hipGetLastError();
}

hipError_t psm_launch_umax(const double* cells, int64_t n, double* umax, hipStream_t st) {
  hipLaunchKernelGGL(psm_umax_kernel, dim3(1), dim3(1024), 0, st, cells, n, umax);
  return hipGetLastError();
}
hipError_t psm_launch_to_grid(const PsmToGridArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(psm_to_grid_kernel, dim3((unsigned)((a.n_grid + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
// k columns of mesh values -> grid image, float64: out[cell][c] = interpolate(_fill)(values[:, c]) of the
// grid point that NumPy's fancy assignment leaves in that cell (last writer), 0 for cells never written
// (np.zeros base image); NaNs of interpolate_fill are kept (the caller's `grid[np.isnan(grid)] = 0`).
__global__ __launch_bounds__(256) void psm_interp_to_grid_kernel(const double* values, int k, const int32_t* vtx, const double* wts,
                                                                 const int32_t* src_of_cell, int fill, double* out, int64_t n_grid) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= n_grid) return;
  const int src = src_of_cell[cell];
  if (src < 0) {
    for (int c = 0; c < k; ++c) out[cell * k + c] = 0.0;
    return;
  }
  const int32_t* v = vtx + (int64_t)src * 3;
  const double* w = wts + (int64_t)src * 3;
  const bool neg = (w[0] < 0.0) || (w[1] < 0.0) || (w[2] < 0.0);
  for (int c = 0; c < k; ++c) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) s += values[(int64_t)v[j] * k + c] * w[j];      // np.einsum('nj,nj->n', take(values, vtx), wts)
    out[cell * k + c] = (fill && neg) ? NAN : s;
  }
}

hipError_t psm_launch_interp_to_grid(const double* values, int k, const int32_t* vtx, const double* wts, const int32_t* src_of_cell,
                                     int fill, double* out, int64_t n_grid, hipStream_t st) {
  hipLaunchKernelGGL(psm_interp_to_grid_kernel, dim3((unsigned)((n_grid + 255) / 256)), dim3(256), 0, st, values, k, vtx, wts,
                     src_of_cell, fill, out, n_grid);
  return hipGetLastError();
}

// The same step for n_frames arrays of cell columns at once (PsmFrameArgs in psm_mesh.h), every column into a plane of its own:
// frame blockIdx.y, one thread per image cell.  A thread reads its cell's source point, simplex and weights once -- they are the
// frames' common tables -- and then repeats the statements of the kernel above per column: the sum over the three vertices in the
// same order from s = 0, NaN for a negative weight under `fill`, 0 for a cell nobody writes (in EVERY stored plane, so the planes
// need no memset and a replay over reused buffers is complete).  A float64 plane therefore holds the bits of that kernel's column;
// a float32 plane holds their plain cast.  The k descriptors are kernel arguments: nothing is copied for a launch.
__global__ __launch_bounds__(256) void psm_interp_to_grid_kernel(PsmFrameArgs a) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.n_grid) return;
  const int64_t frame = blockIdx.y;
  const int k = a.k;
  const double* values = a.cols + frame * a.n_cells * k;
  const int src = a.src_of_cell[cell];
  int32_t v[3] = {0, 0, 0};
  double w[3] = {0.0, 0.0, 0.0};
  if (src >= 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { v[j] = a.vtx[(int64_t)src * 3 + j]; w[j] = a.wts[(int64_t)src * 3 + j]; }
  }
  const bool neg = (w[0] < 0.0) || (w[1] < 0.0) || (w[2] < 0.0);
  for (int c = 0; c < k; ++c) {
    const PsmFramePlane o = a.out[c];
    if (!o.dst) continue;
    double r = 0.0;
    if (src >= 0) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) s += values[(int64_t)v[j] * k + c] * w[j];
      r = (a.fill && neg) ? NAN : s;
    }
    const int64_t at = frame * o.frame_stride + cell;
    if (o.as_f32) static_cast<float*>(o.dst)[at] = (float)r;
    else static_cast<double*>(o.dst)[at] = r;
  }
}

hipError_t psm_launch_frames_to_grid(const PsmFrameArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.k < 1 || a.k > PSM_FRAME_MAX_COLS || a.n_grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmFrameArgs)>(psm_interp_to_grid_kernel), dim3((unsigned)((a.n_grid + 255) / 256), (unsigned)a.n_frames),
                     dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t psm_launch_to_mesh(const PsmToMeshArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(psm_to_mesh_kernel, dim3((unsigned)((a.n_cells + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The mesh ends of a case batch (psm_solve_cases*, PsmMeshCasesArgs in psm_mesh.h): K meshes with their own obstacles on one
// planned grid.  Three launches around the batched solve, the case is launch dimension y everywhere; a workgroup reads its
// case's range from cell_off and its case's tables only, so a case's result does not depend on what the other slots hold.
// The per-thread arithmetic is that of the single-mesh kernels above, statement for statement: one case through these
// kernels gives the bits of psm_solve (tests/test_mesh_cases.py holds them to that).

// U_max, level one: the maximum of the SQUARED speed over part blockIdx.x of case blockIdx.y.  The partition is fixed by the
// launch (n_parts parts, cell c of a case belongs to part (c / 1024) % n_parts); a maximum does not depend on it anyway.
__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(PsmMeshCasesArgs a) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cs = blockIdx.y;
  const int64_t c0 = a.cell_off[cs], n = a.cell_off[cs + 1] - c0;
  const double* cells = a.cells + c0 * 5;
  double m = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + tid; i < n; i += (int64_t)gridDim.x * 1024) {
    const double ux = cells[i * 5], uy = cells[i * 5 + 1];
    m = nanmax2(m, speed2_np(ux, uy));
  }
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) {
    double r = red[0];
    for (int w = 1; w < 16; ++w) r = nanmax2(r, red[w]);
    a.umax_part[(int64_t)cs * a.n_parts + blockIdx.x] = r;
  }
}

// Level two + mesh -> grid: every workgroup folds its case's row of partials (like psm_to_grid_kernel does with the single
// mesh's), workgroup 0 of the case leaves U_max[case] for the batched psm_to_mesh_kernel; then the body of psm_to_grid_kernel on
// the case's tables, into image `case` of the staging grid.
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmMeshCasesArgs a) {
  __shared__ double um_s[4];
  const int cs = blockIdx.y;
  double m = a.umax_part[(int64_t)cs * a.n_parts + min((int)threadIdx.x, a.n_parts - 1)];
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) um_s[threadIdx.x >> 6] = m;
  __syncthreads();
  const double umax_v = sqrt_rn(nanmax2(nanmax2(um_s[0], um_s[1]), nanmax2(um_s[2], um_s[3])));
  if (blockIdx.x == 0 && threadIdx.x == 0) a.umax[cs] = umax_v;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.n_grid) return;
  const int64_t g0 = (int64_t)cs * a.n_grid;
  const double* cells = a.cells + a.cell_off[cs] * 5;
  const int src = a.src_of_cell[g0 + cell];
  float ux = 0.f, uy = 0.f;
  if (src >= 0) {
    const double inv = 1.0 / umax_v;
    const int32_t* v = a.vtx_m2g + (g0 + src) * 3;
    const double* w = a.wts_m2g + (g0 + src) * 3;
    double sx = 0.0, sy = 0.0;
    bool neg = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double* c = cells + (int64_t)v[j] * 5;
      sx += (c[0] * inv) * w[j];
      sy += (c[1] * inv) * w[j];
      neg = neg || (w[j] < 0.0);
    }
    if (a.fill && neg) { sx = NAN; sy = NAN; }
    sx /= a.max_abs_ux;
    sy /= a.max_abs_uy;
    ux = (sx != sx) ? 0.f : (float)sx;
    uy = (sy != sy) ? 0.f : (float)sy;
  }
  const double sd = a.sdf[g0 + cell] * a.sdf_scale;
  float* g = a.grid + (g0 + cell) * a.c_in;
  g[0] = ux;
  g[1] = uy;
  g[2] = (sd != sd) ? 0.f : (float)sd;
}

// grid -> mesh for all sum n_i cells in one launch.  The case is launch dimension y (x covers the largest case) and not a
// search of cell_off per thread: a workgroup then reads its range with two uniform loads and gathers from one case's image
// only, and what it costs is the workgroups beyond a shorter case's end, which return at once -- the cases of an ensemble
// are meshes of one channel with different obstacles, a few per cent apart in size.
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmMeshCasesArgs a) {
  const int cs = blockIdx.y;
  const int64_t c0 = a.cell_off[cs], local = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (local >= a.cell_off[cs + 1] - c0) return;
  const int64_t n = c0 + local, g0 = (int64_t)cs * a.n_grid;
  const int32_t* v = a.vtx_g2m + n * 3;
  const double* w = a.wts_g2m + n * 3;
  double acc = 0.0;
  bool neg = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int cell = a.cell_of_point[g0 + v[j]];
    acc += (double)a.field[(g0 + cell) * a.c_out] * w[j];
    neg = neg || (w[j] < 0.0);
  }
  const double um = a.umax[cs];
  double p = acc * a.max_abs_p * (um * um);
  const double prev = a.cells[n * 5 + 4];
  if (a.near_wall[n] || neg || acc != acc) p = prev;
  a.p_out[n] = p;
}

typedef void (*PsmCasesKernel)(PsmMeshCasesArgs);
hipError_t psm_launch_umax_cases(const PsmMeshCasesArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(static_cast<PsmCasesKernel>(psm_umax_partial_kernel), dim3(a.n_parts, a.n_cases), dim3(1024), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_to_grid_cases(const PsmMeshCasesArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(static_cast<PsmCasesKernel>(psm_to_grid_kernel), dim3((unsigned)((a.n_grid + 255) / 256), a.n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_to_mesh_cases(const PsmMeshCasesArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(static_cast<PsmCasesKernel>(psm_to_mesh_kernel), dim3((unsigned)((a.max_cells + 255) / 256), a.n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// a8 (evaluation only): label blocks with the per-block mean over the flow cells removed --
//   y_array[step, ..., c][x_array[step, ..., sdf] != 0] -= mean(y_array[step, ..., c][x_array[step, ..., sdf] != 0])
// (SM_call.py:487-488; Eval_dual_Dense_onlycil.py:509-511).  One workgroup per (block, channel); float64 sums like the
// float64 grid of the reference.  A block without flow cells keeps its values (the reference's empty-slice mean is
// NaN but is assigned to an empty selection).
__global__ __launch_bounds__(256) void psm_label_blocks_kernel(const float* grid, const float* labels, const int32_t* blk_y0x0,
                                                               float* out, int S, int c_in, int c_out, int sdf_ch, int Nx) {
  const int b = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
  const int y0 = blk_y0x0[2 * b], x0 = blk_y0x0[2 * b + 1];
  __shared__ double ssum[256];
  __shared__ double scnt[256];
  double sum = 0.0, cnt = 0.0;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * Nx + x0 + i % S;
    if (grid[pix * c_in + sdf_ch] != 0.f) { sum += (double)labels[pix * c_out + c]; cnt += 1.0; }
  }
  ssum[t] = sum; scnt[t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { ssum[t] += ssum[t + s]; scnt[t] += scnt[t + s]; }
    __syncthreads();
  }
  const double mean = scnt[0] > 0.0 ? ssum[0] / scnt[0] : 0.0;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * Nx + x0 + i % S;
    const double v = (double)labels[pix * c_out + c];
    out[((int64_t)b * S * S + i) * c_out + c] = (float)(grid[pix * c_in + sdf_ch] != 0.f ? v - mean : v);
  }
}

hipError_t psm_launch_label_blocks(const float* grid, const float* labels, const int32_t* blk_y0x0, float* out, int B, int S,
                                   int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st) {
  hipLaunchKernelGGL(psm_label_blocks_kernel, dim3(B, c_out), dim3(256), 0, st, grid, labels, blk_y0x0, out, S, c_in, c_out, sdf_ch, Nx);
  return hipGetLastError();
}

// compute_in_block_error (pressureSM_deltas/utils.py:210-243; called at SM_call.py:555-557 on the decoded blocks BEFORE the
// reassembly): partial sums per workgroup over the flow cells of one block -- count and sum / sum of squares of the
// non-NaN differences pred - true, extrema of true and pred, count of NaN truths (np.max then gives NaN) -- float64 like
// the reference's arrays; `true` = label block * row_scale[b] (SM_call.py:555: y_array * max_abs_p * U_max_norm^2, the scale
// the decoded blocks already carry).  Partials [B][8] doubles, summed on the host.
__global__ __launch_bounds__(256) void psm_block_error_kernel(const float* grid, const float* pred, const float* label_blocks,
                                                              const float* row_scale, const int32_t* blk_y0x0, double* part,
                                                              int S, int c_in, int c_out, int sdf_ch, int Nx) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int y0 = blk_y0x0[2 * b], x0 = blk_y0x0[2 * b + 1];
  const double sc = (double)row_scale[b];
  double n = 0.0, s1 = 0.0, s2 = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, tnan = 0.0;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * Nx + x0 + i % S;
    if (!(grid[pix * c_in + sdf_ch] != 0.f)) continue;
    for (int c = 0; c < c_out; ++c) {
      const int64_t e = ((int64_t)b * S * S + i) * c_out + c;
      const double tr = (double)label_blocks[e] * sc, pr = (double)pred[e];
      if (tr != tr) tnan += 1.0; else { tmin = fmin(tmin, tr); tmax = fmax(tmax, tr); }
      if (pr == pr) { pmin = fmin(pmin, pr); pmax = fmax(pmax, pr); }
      const double d = pr - tr;
      if (d == d) { n += 1.0; s1 += d; s2 += d * d; }
    }
  }
  __shared__ double sh[8][256];
  sh[0][t] = n; sh[1][t] = s1; sh[2][t] = s2; sh[3][t] = tmin; sh[4][t] = tmax; sh[5][t] = pmin; sh[6][t] = pmax; sh[7][t] = tnan;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sh[0][t] += sh[0][t + s]; sh[1][t] += sh[1][t + s]; sh[2][t] += sh[2][t + s]; sh[7][t] += sh[7][t + s];
      sh[3][t] = fmin(sh[3][t], sh[3][t + s]); sh[4][t] = fmax(sh[4][t], sh[4][t + s]);
      sh[5][t] = fmin(sh[5][t], sh[5][t + s]); sh[6][t] = fmax(sh[6][t], sh[6][t + s]);
    }
    __syncthreads();
  }
  if (t < 8) part[(int64_t)b * 8 + t] = sh[t][0];
}

hipError_t psm_launch_block_error(const float* grid, const float* pred, const float* label_blocks, const float* row_scale,
                                  const int32_t* blk_y0x0, double* part, int B, int S, int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st) {
  hipLaunchKernelGGL(psm_block_error_kernel, dim3(B), dim3(256), 0, st, grid, pred, label_blocks, row_scale, blk_y0x0, part, S, c_in, c_out, sdf_ch, Nx);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The same eight sums for ASSEMBLED fields (psm_field_errors_device; PsmFieldErrorArgs in psm_mesh.h): the three error blocks the
// Poisson evaluator prints per frame (pressureSM_Poisson/SM_call.py:962-1043) without the fields leaving the device.  HBM-bound:
// a pair reads up to five planes once.  Launch 1, grid (workgroups over pixels, pair, frame): a thread takes 4 consecutive pixels
// per round -- one 16-byte load per float32 plane, two per float64 plane where the frame's plane is dense and 16-byte aligned,
// else one load per pixel (result [npix][c_out], odd plane offsets, the tail) --, sums in float64 like the reference's arrays,
// then wave shuffle -> LDS -> 8 doubles per workgroup.  Launch 2 folds a row of partials.  No atomics; pixel -> thread -> lane ->
// wave -> workgroup is a fixed tree, the same on either load path: a result depends on the inputs alone, bit for bit.
typedef float psm_f4 __attribute__((ext_vector_type(4)));

struct PsmErrSrc { const char* base; int64_t es; bool f32, dense; };   // one frame's plane (base == nullptr: absent)

__device__ __forceinline__ PsmErrSrc err_src(const PsmErrPlane& p, int64_t frame) {
  PsmErrSrc s;
  s.f32 = p.as_f32 != 0; s.es = p.elem_stride;
  s.base = p.ptr ? static_cast<const char*>(p.ptr) + frame * p.frame_stride * (s.f32 ? 4 : 8) : nullptr;
  s.dense = s.base && s.es == 1 && (reinterpret_cast<uintptr_t>(s.base) & 15) == 0;
  return s;
}

// pixels pix .. pix + 3 (pix a multiple of 4) as doubles; a pixel beyond the image or of an absent plane reads as 0
__device__ __forceinline__ void err_load4(const PsmErrSrc& s, int64_t pix, int64_t npix, double (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.0;
  if (!s.base) return;
  if (s.dense && pix + 3 < npix) {
    if (s.f32) {
      const psm_f4 q = *reinterpret_cast<const psm_f4*>(s.base + pix * 4);
      v[0] = (double)q.x; v[1] = (double)q.y; v[2] = (double)q.z; v[3] = (double)q.w;
    } else {
      const psm_d2 q0 = *reinterpret_cast<const psm_d2*>(s.base + pix * 8), q1 = *reinterpret_cast<const psm_d2*>(s.base + pix * 8 + 16);
      v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (pix + e >= npix) continue;
    const int64_t at = (pix + e) * s.es;
    v[e] = s.f32 ? (double)reinterpret_cast<const float*>(s.base)[at] : reinterpret_cast<const double*>(s.base)[at];
  }
}

__device__ __forceinline__ double nan0(double x) { return x != x ? 0.0 : x; }

__global__ __launch_bounds__(256) void psm_block_error_kernel(PsmFieldErrorArgs a) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, pi = blockIdx.y;
  const int64_t frame = blockIdx.z;
  const PsmFieldErrorPair& pr = a.pair[pi];
  const PsmErrSrc mask = err_src(a.mask, frame), pred = err_src(pr.pred, frame), truth = err_src(pr.truth, frame),
                  add = err_src(pr.add, frame), sub = err_src(pr.sub, frame);
  const bool t0 = pr.truth_nan_to_zero != 0;
  double n = 0.0, s1 = 0.0, s2 = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, tnan = 0.0;
#pragma unroll
  for (int j = 0; j < PSM_FIELD_ERR_SPAN / 1024; ++j) {
    const int64_t pix = (int64_t)blockIdx.x * PSM_FIELD_ERR_SPAN + j * 1024 + t * 4;
    if (pix >= a.npix) continue;
    double m[4], p[4], tr[4], ad[4], sb[4];
    err_load4(mask, pix, a.npix, m); err_load4(pred, pix, a.npix, p); err_load4(truth, pix, a.npix, tr);
    err_load4(add, pix, a.npix, ad); err_load4(sub, pix, a.npix, sb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!(m[e] != 0.0 && m[e] == m[e])) continue;          // no flow, and every pixel beyond the image (its mask read as 0)
      const double tv = t0 ? nan0(tr[e]) : tr[e];
      const double pe = (nan0(ad[e]) - nan0(sb[e])) + p[e];
      if (tv != tv) tnan += 1.0; else { tmin = fmin(tmin, tv); tmax = fmax(tmax, tv); }
      if (pe == pe) { pmin = fmin(pmin, pe); pmax = fmax(pmax, pe); }
      const double d = pe - tv;
      if (d == d) { n += 1.0; s1 += d; s2 += d * d; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o, 64); s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); tnan += __shfl_down(tnan, o, 64);
    tmin = fmin(tmin, __shfl_down(tmin, o, 64)); tmax = fmax(tmax, __shfl_down(tmax, o, 64));
    pmin = fmin(pmin, __shfl_down(pmin, o, 64)); pmax = fmax(pmax, __shfl_down(pmax, o, 64));
  }
  __shared__ double red[4][8];
  if (lane == 0) {
    double* r = red[wave];
    r[0] = n; r[1] = s1; r[2] = s2; r[3] = tmin; r[4] = tmax; r[5] = pmin; r[6] = pmax; r[7] = tnan;
  }
  __syncthreads();
  if (t < 8) {
    double r = red[0][t];
    for (int w = 1; w < 4; ++w) r = (t == 3 || t == 5) ? fmin(r, red[w][t]) : (t == 4 || t == 6) ? fmax(r, red[w][t]) : r + red[w][t];
    a.part[((frame * a.n_pairs + pi) * a.n_wg + blockIdx.x) * 8 + t] = r;
  }
}

// one wave per (pair, frame): lane l folds partials l, l + 64, ... in order, then the same shuffle tree
__global__ __launch_bounds__(64) void psm_block_error_kernel(PsmFieldErrorFinalArgs a) {
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;        // frame * n_pairs + pair
  const double* part = a.part + row * a.n_wg * 8;
  double n = 0.0, s1 = 0.0, s2 = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, tnan = 0.0;
  for (int w = lane; w < a.n_wg; w += 64) {
    const double* q = part + (int64_t)w * 8;
    n += q[0]; s1 += q[1]; s2 += q[2]; tnan += q[7];
    tmin = fmin(tmin, q[3]); tmax = fmax(tmax, q[4]); pmin = fmin(pmin, q[5]); pmax = fmax(pmax, q[6]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_down(n, o, 64); s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); tnan += __shfl_down(tnan, o, 64);
    tmin = fmin(tmin, __shfl_down(tmin, o, 64)); tmax = fmax(tmax, __shfl_down(tmax, o, 64));
    pmin = fmin(pmin, __shfl_down(pmin, o, 64)); pmax = fmax(pmax, __shfl_down(pmax, o, 64));
  }
  if (lane == 0) {
    double* r = a.raw + row * 8;
    r[0] = n; r[1] = s1; r[2] = s2; r[3] = tmin; r[4] = tmax; r[5] = pmin; r[6] = pmax; r[7] = tnan;
  }
}

hipError_t psm_launch_field_errors(const PsmFieldErrorArgs& a, hipStream_t st) {
  if (a.npix < 1 || a.n_pairs < 1 || a.n_pairs > PSM_FIELD_ERR_MAX_PAIRS || a.n_frames < 1 || a.n_wg != psm_field_error_workgroups(a.npix) || !a.part)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmFieldErrorArgs)>(psm_block_error_kernel), dim3((unsigned)a.n_wg, (unsigned)a.n_pairs, (unsigned)a.n_frames),
                     dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_field_errors_final(const PsmFieldErrorFinalArgs& a, int n_pairs, int n_frames, hipStream_t st) {
  if (n_pairs < 1 || n_frames < 1 || a.n_wg < 1 || !a.part || !a.raw) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmFieldErrorFinalArgs)>(psm_block_error_kernel), dim3((unsigned)n_pairs, (unsigned)n_frames), dim3(64), 0, st, a);
  return hipGetLastError();
}
