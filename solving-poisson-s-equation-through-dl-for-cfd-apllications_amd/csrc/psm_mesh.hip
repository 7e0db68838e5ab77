// psm_mesh.hip -- mesh <-> uniform-grid ends of the per-step call:
// the solver hands over cells[N,5] = (Ux, Uy, Cx, Cy, p) in float64 (PythonComm.H:2-9) and
// reads back p[N] float64 (PythonComm.H:31-36).
//
//   umax     : U_max = max sqrt(Ux^2 + Uy^2)                               [PM:270]
//   to_grid  : barycentric mesh->grid interpolation, scatter into the image, normalisation,
//              SDF channel, NaN -> 0                                        [PM:272-297]
//   to_mesh  : gather at `indices`, barycentric grid->mesh interpolation with fill,
//              dimensionalise, near-wall / NaN fallback to the previous p   [PM:481-496]
//   both ends also in DELTA form (psm_solve_delta*): U - U(t-1) in, p(t-1) + dp out, U(t-1) := U   [SMD:389-391]
//   and as the ends of the Poisson-model step (psm_solve_poisson*, at the end of this file): six columns from cells + a two-frame
//   state in, p(t-1) + dp out, the state turned over; for a case set too (psm_solve_cases_poisson*)  [SMP:549-556, 842-847]
//   and the tail of the gradient-model step (psm_solve_gradp*, at the end of this file): the outlet level of the integrated plane,
//   grid -> mesh, p = acc U^2; for a case set too (psm_solve_cases_gradp*)                          [PM:472, 481-496; UGP:537-538]
//
// All of them are HBM-bound gathers; interpolation is done in float64 like the reference.
#include "psm_mesh.h"
#include "psm_mesh_dev.h"   // sqrt_rn, nanmax2, umax_of_partials, add_np, psm_uv2: shared with psm_unet_mesh.hip

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
__global__ __launch_bounds__(1024) void psm_umax_kernel(const double* cells, int64_t n, double* umax) {
  __shared__ double red[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m = 0.0;
  for (int64_t i = tid; i < n; i += 1024) {
    const double ux = cells[i * 5], uy = cells[i * 5 + 1];
    m = nanmax2(m, speed2_np(ux, uy));
  }
  for (int o = 32; o > 0; o >>= 1) m = nanmax2(m, __shfl_down(m, o, 64));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) {
    double r = red[0];
    for (int w = 1; w < 16; ++w) r = nanmax2(r, red[w]);
    *umax = sqrt_rn(r);
  }
}

// ---------------------------------------------------------------------------
// One body per stage, called by the single-mesh kernel and by the case-batch kernel (PsmMeshCasesArgs) alike: a kernel is where
// U_max comes from and the offsetting of its case's base pointers, then the body.

// The maximum of the SQUARED speed over the cells blockIdx.x * 1024 + tid, + gridDim.x * 1024, ... of cells[n,5], wave fold, LDS
// fold; thread 0 stores it to *out.
__device__ __forceinline__ void umax2_partial(const double* cells, int64_t n, double* out) {
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
    *out = r;
  }
}

// image cell `cell` of the mesh whose tables `a` points at.  DELTA (psm_solve_delta*, the deltas model at the solver boundary):
// the gathered value is U(t) - U(t-1), formed in float64 per vertex in front of the chain (SM_call.py:389-391), with U(t-1) from
// u_prev [N][2]; U_max stays that of the current cells (:404, :418-419).
template <bool DELTA>
__device__ __forceinline__ void to_grid_cell(const PsmToGridArgs& a, const double* u_prev, double umax_v, int64_t cell) {
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
      double cx = c[0], cy = c[1];
      if (DELTA) {
        const psm_uv2 q = *reinterpret_cast<const psm_uv2*>(u_prev + (int64_t)v[j] * 2);
        cx -= q.x; cy -= q.y;
      }
      sx += (cx * inv) * w[j];             // interpolate(Ux / U_max)  (PM:272,280)
      sy += (cy * inv) * w[j];
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

// mesh cell n of the mesh whose tables `a` points at.  DELTA: the field is dp, so p = p(t-1) + dp and p(t-1) itself where the body
// falls back (PM:494-496 applied to dp); the thread then leaves its cell's (Ux, Uy) in u_prev[n] -- the state turns over in the
// step's last launch, behind every reader of the old one in stream order.  `prime` (uniform): no field yet, p = p(t-1) everywhere.
template <bool DELTA>
__device__ __forceinline__ void to_mesh_cell(const PsmToMeshArgs& a, double* u_prev, int prime, double um, int64_t n) {
  const int32_t* v = a.vtx + n * 3;
  const double* w = a.wts + n * 3;
  double acc = 0.0;
  bool neg = false;
  if (!(DELTA && prime)) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int cell = a.cell_of_point[v[j]];                       // p_adim_unif = result[indices]  (PM:481)
      acc += (double)a.field[(int64_t)cell * a.c_out] * w[j];
      neg = neg || (w[j] < 0.0);
    }
  }
  double p = acc * a.max_abs_p * (um * um);                         // PM:490
  const double prev = a.cells[n * 5 + 4];
  if (DELTA) p = add_np(prev, p);
  if ((DELTA && prime) || a.near_wall[n] || neg || acc != acc) p = prev;   // PM:494, 496 (interpolate_fill -> NaN)
  a.p_out[n] = p;
  if (DELTA) *reinterpret_cast<psm_uv2*>(u_prev + n * 2) = psm_uv2{a.cells[n * 5], a.cells[n * 5 + 1]};
}

__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(const double* cells, int64_t n, double* partials) {
  umax2_partial(cells, n, partials + blockIdx.x);
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

// ---------------------------------------------------------------------------
// One wrapper per end and batch form: where U_max comes from, the bounds check, the cell body.  The kernels below are a call of
// one of them each.  The argument structs go BY VALUE: behind a reference the uniform load of *a.umax becomes a load per lane.
template <bool DELTA>
__device__ __forceinline__ void to_grid_single(PsmToGridArgs a, const double* u_prev) {
  double umax_v = a.umax ? *a.umax : a.umax_val;
  if (a.umax_partials) {                      // uniform: every workgroup reduces the <= 256 partial maxima itself
    umax_v = umax_of_partials(a.umax_partials, a.n_partials);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.umax_out = umax_v;
  }
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.n_grid) return;
  to_grid_cell<DELTA>(a, u_prev, umax_v, cell);
}

// `prime` (delta only): nothing is scaled, U_max is not read
template <bool DELTA>
__device__ __forceinline__ void to_mesh_single(PsmToMeshArgs a, double* u_prev, int prime) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_cells) return;
  to_mesh_cell<DELTA>(a, u_prev, prime, prime ? 0.0 : (a.umax ? *a.umax : a.umax_val), n);
}

// The single mesh, absolute and delta (PsmDeltaGridArgs / PsmDeltaMeshArgs in psm_mesh.h): the same launch shapes and the same
// three sources of U_max.
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmToGridArgs a) { to_grid_single<false>(a, nullptr); }
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmToMeshArgs a) { to_mesh_single<false>(a, nullptr, 0); }
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmDeltaGridArgs d) { to_grid_single<true>(d.g, d.u_prev); }
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmDeltaMeshArgs d) { to_mesh_single<true>(d.m, d.u_prev, d.prime); }

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
  hipLaunchKernelGGL(static_cast<void (*)(PsmToGridArgs)>(psm_to_grid_kernel), dim3((unsigned)((a.n_grid + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_to_grid_delta(const PsmDeltaGridArgs& d, hipStream_t st) {
  if (!d.u_prev || d.g.n_grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmDeltaGridArgs)>(psm_to_grid_kernel), dim3((unsigned)((d.g.n_grid + 255) / 256)), dim3(256), 0, st, d);
  return hipGetLastError();
}
// One column of one image cell, the statements the two kernels below share: np.einsum('nj,nj->n', take(values, vtx), wts) over the
// three vertices in order from 0.0; NaN where interpolate_fill finds a negative weight.
__device__ __forceinline__ double interp_column(const double* values, int k, int c, const int32_t* v, const double* w, int fill, bool neg) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) s += values[(int64_t)v[j] * k + c] * w[j];
  return (fill && neg) ? NAN : s;
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
  for (int c = 0; c < k; ++c) out[cell * k + c] = interp_column(values, k, c, v, w, fill, neg);
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
    if (src >= 0) r = interp_column(values, k, c, v, w, a.fill, neg);
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
  hipLaunchKernelGGL(static_cast<void (*)(PsmToMeshArgs)>(psm_to_mesh_kernel), dim3((unsigned)((a.n_cells + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_to_mesh_delta(const PsmDeltaMeshArgs& d, hipStream_t st) {
  if (!d.u_prev || d.m.n_cells < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmDeltaMeshArgs)>(psm_to_mesh_kernel), dim3((unsigned)((d.m.n_cells + 255) / 256)), dim3(256), 0, st, d);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The mesh ends of a case batch (psm_solve_cases*, PsmMeshCasesArgs in psm_mesh.h): K meshes with their own obstacles on one
// planned grid.  Three launches around the batched solve, the case is launch dimension y everywhere; a workgroup reads its
// case's range from cell_off and its case's tables only, so a case's result does not depend on what the other slots hold.
// The per-thread arithmetic is the bodies above, on the case's slices of the concatenated tables.

// U_max, level one: the maximum of the SQUARED speed over part blockIdx.x of case blockIdx.y.  The partition is fixed by the
// launch (n_parts parts, cell c of a case belongs to part (c / 1024) % n_parts); a maximum does not depend on it anyway.
__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(PsmMeshCasesArgs a) {
  const int cs = blockIdx.y;
  const int64_t c0 = a.cell_off[cs];
  umax2_partial(a.cells + c0 * 5, a.cell_off[cs + 1] - c0, a.umax_part + (int64_t)cs * a.n_parts + blockIdx.x);
}

// A case's slices of the concatenated tables, as the single-mesh bodies take them (U_max is the wrapper's)
__device__ __forceinline__ PsmToGridArgs case_grid_slice(const PsmMeshCasesArgs& a, int cs) {
  const int64_t g0 = (int64_t)cs * a.n_grid;
  PsmToGridArgs g{};
  g.cells = a.cells + a.cell_off[cs] * 5;
  g.vtx = a.vtx_m2g + g0 * 3; g.wts = a.wts_m2g + g0 * 3; g.src_of_cell = a.src_of_cell + g0;
  g.sdf = a.sdf + g0; g.grid = a.grid + g0 * a.c_in;
  g.max_abs_ux = a.max_abs_ux; g.max_abs_uy = a.max_abs_uy; g.sdf_scale = a.sdf_scale; g.c_in = a.c_in; g.fill = a.fill;
  return g;
}
__device__ __forceinline__ PsmToMeshArgs case_mesh_slice(const PsmMeshCasesArgs& a, int cs, int64_t c0) {
  const int64_t g0 = (int64_t)cs * a.n_grid;
  PsmToMeshArgs m{};
  m.cells = a.cells + c0 * 5;
  m.vtx = a.vtx_g2m + c0 * 3; m.wts = a.wts_g2m + c0 * 3; m.cell_of_point = a.cell_of_point + g0;
  m.field = a.field + g0 * a.c_out; m.near_wall = a.near_wall + c0; m.p_out = a.p_out + c0;
  m.max_abs_p = a.max_abs_p; m.c_out = a.c_out;
  return m;
}

// Level two + mesh -> grid: every workgroup folds its case's row of partials, workgroup 0 of the case leaves U_max[case] for the
// batched psm_to_mesh_kernel; then the cell body on the case's tables, into image `case` of the staging grid.  DELTA: u_prev
// [sum n_i][2] is sliced like the cells.
template <bool DELTA>
__device__ __forceinline__ void to_grid_case(PsmMeshCasesArgs a, const double* u_prev) {
  const int cs = blockIdx.y;
  const double umax_v = umax_of_partials(a.umax_part + (int64_t)cs * a.n_parts, a.n_parts);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.umax[cs] = umax_v;
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.n_grid) return;
  to_grid_cell<DELTA>(case_grid_slice(a, cs), DELTA ? u_prev + a.cell_off[cs] * 2 : nullptr, umax_v, cell);
}

// grid -> mesh for all sum n_i cells in one launch.  The case is launch dimension y (x covers the largest case) and not a
// search of cell_off per thread: a workgroup then reads its range with two uniform loads and gathers from one case's image
// only, and what it costs is the workgroups beyond a shorter case's end, which return at once -- the cases of an ensemble
// are meshes of one channel with different obstacles, a few per cent apart in size.
template <bool DELTA>
__device__ __forceinline__ void to_mesh_case(PsmMeshCasesArgs a, double* u_prev, int prime) {
  const int cs = blockIdx.y;
  const int64_t c0 = a.cell_off[cs], local = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (local >= a.cell_off[cs + 1] - c0) return;
  to_mesh_cell<DELTA>(case_mesh_slice(a, cs, c0), DELTA ? u_prev + c0 * 2 : nullptr, prime, prime ? 0.0 : a.umax[cs], local);
}

__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmMeshCasesArgs a) { to_grid_case<false>(a, nullptr); }
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmMeshCasesArgs a) { to_mesh_case<false>(a, nullptr, 0); }
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmDeltaCasesArgs d) { to_grid_case<true>(d.c, d.u_prev); }
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmDeltaCasesArgs d) { to_mesh_case<true>(d.c, d.u_prev, d.prime); }

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
typedef void (*PsmDeltaCasesKernel)(PsmDeltaCasesArgs);
hipError_t psm_launch_to_grid_cases_delta(const PsmDeltaCasesArgs& d, hipStream_t st) {
  if (!d.u_prev || d.c.n_cases < 1 || d.c.n_grid < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<PsmDeltaCasesKernel>(psm_to_grid_kernel), dim3((unsigned)((d.c.n_grid + 255) / 256), d.c.n_cases), dim3(256), 0, st, d);
  return hipGetLastError();
}
hipError_t psm_launch_to_mesh_cases_delta(const PsmDeltaCasesArgs& d, hipStream_t st) {
  if (!d.u_prev || d.c.n_cases < 1 || d.c.max_cells < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<PsmDeltaCasesKernel>(psm_to_mesh_kernel), dim3((unsigned)((d.c.max_cells + 255) / 256), d.c.n_cases), dim3(256), 0, st, d);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The mesh ends of the Poisson-model step at the solver boundary (psm_solve_poisson*, PsmPoissonCellsArgs / PsmPoissonMeshArgs in
// psm_mesh.h): three launches around the chain of psm_poisson_step_device, overloads of the kernels of the same purpose above.
// What a cell's columns are made of is float64 and rounded operation by operation (`fp contract(off)`); the interpolation of a
// column is the statement of interp_column, so that a plane holds the bits psm_poisson_frames leaves on host-made columns.

// c_cell = np.abs(delta_U - delta_U_prev).sum(axis=-1)  (SMP:549)
__device__ __forceinline__ double poisson_change(double dux, double duy, double dpx, double dpy) {
#pragma clang fp contract(off)
  const double d0 = dux - dpx, d1 = duy - dpy;
  return fabs(d0) + fabs(d1);
}

// The six columns of mesh cell i: (Ux, Uy, dUx, dUy, c_cell / c, dp_prev); the last two only with the weighting.  A skipped step: zeros.
struct PoissonCols { double v[6]; };
__device__ __forceinline__ PoissonCols poisson_cols(const PsmPoissonCellsArgs& a, int64_t i, double c, bool skip) {
#pragma clang fp contract(off)
  PoissonCols o;
#pragma unroll
  for (int q = 0; q < 6; ++q) o.v[q] = 0.0;
  if (skip) return o;
  const double* r = a.cells + i * 5;
  const psm_uv2 up = *reinterpret_cast<const psm_uv2*>(a.u_prev + i * 2);
  const double ux = r[0], uy = r[1];
  const double dux = ux - up.x, duy = uy - up.y;
  o.v[0] = ux; o.v[1] = uy; o.v[2] = dux; o.v[3] = duy;
  if (a.weighting) {
    const psm_uv2 dq = *reinterpret_cast<const psm_uv2*>(a.du_prev + i * 2);
    const double cc = poisson_change(dux, duy, dq.x, dq.y);
    o.v[4] = (c == 0.0) ? 0.0 : cc / c;                    // deltaU_changed / deltaU_changed.max()  (SMP:550); 0 where nothing changed at all
    o.v[5] = r[4] - a.p_prev[i];
  }
  return o;
}

// One body per launch, called by the single-mesh kernel and by the case-set kernel (PsmPoissonCasesArgs) alike: a kernel is the
// offsetting of its case's base pointers, then the body.  The argument structs go BY VALUE, as above.

// Head, level one: workgroup b leaves the maxima of the squared speed and of c_cell over its cells (b * 1024 + tid, + gridDim.x *
// 1024, ...) in partials[b] and partials[PSM_POISSON_PARTS + b].  cells and the state are read once.  A workgroup that owns no cell
// (a shorter case of a set) stores 0.0, the start value of the fold.
__device__ __forceinline__ void poisson_partial(PsmPoissonCellsArgs a) {
  __shared__ double red[2][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double m = 0.0, mc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + tid; i < a.n_cells; i += (int64_t)gridDim.x * 1024) {
    const double ux = a.cells[i * 5], uy = a.cells[i * 5 + 1];
    const psm_uv2 up = *reinterpret_cast<const psm_uv2*>(a.u_prev + i * 2);
    const psm_uv2 dq = *reinterpret_cast<const psm_uv2*>(a.du_prev + i * 2);
    m = nanmax2(m, speed2_np(ux, uy));
    mc = nanmax2(mc, poisson_change(ux - up.x, uy - up.y, dq.x, dq.y));
  }
  for (int o = 32; o > 0; o >>= 1) { m = nanmax2(m, __shfl_down(m, o, 64)); mc = nanmax2(mc, __shfl_down(mc, o, 64)); }
  if (lane == 0) { red[0][wave] = m; red[1][wave] = mc; }
  __syncthreads();
  if (tid < 2) {
    double r = red[tid][0];
    for (int w = 1; w < 16; ++w) r = nanmax2(r, red[tid][w]);
    a.partials[tid * PSM_POISSON_PARTS + blockIdx.x] = r;
  }
}

// Head, level two + mesh -> grid: every workgroup folds both rows of partials itself, workgroup 0 stores the step's scalars -- into
// `scalars` and into the device arrays the chain reads, as psm_rows.hip's finish launch does --; then one thread per image cell
// gathers the columns of the three vertices of its source point and writes the six planes: 0 where nobody writes, NaN for a negative
// weight (interpolate_fill) in the four velocity planes, NaN -> 0 in the two float32 planes.
__device__ __forceinline__ void poisson_to_grid(PsmPoissonCellsArgs a) {
  __shared__ double fold_s[2][4];
  const int tid = threadIdx.x;
  const int p = min(tid, a.n_partials - 1);
  double m = a.partials[p], mc = a.partials[PSM_POISSON_PARTS + p];
  for (int o = 32; o > 0; o >>= 1) { m = nanmax2(m, __shfl_down(m, o, 64)); mc = nanmax2(mc, __shfl_down(mc, o, 64)); }
  if ((tid & 63) == 0) { fold_s[0][tid >> 6] = m; fold_s[1][tid >> 6] = mc; }
  __syncthreads();
  double U = sqrt_rn(nanmax2(nanmax2(fold_s[0][0], fold_s[0][1]), nanmax2(fold_s[0][2], fold_s[0][3])));
  const double c = nanmax2(nanmax2(fold_s[1][0], fold_s[1][1]), nanmax2(fold_s[1][2], fold_s[1][3]));
  const bool skip = !(U > 0.0 && U < INFINITY) || (a.weighting && c != c);
  if (skip) U = 1.0;
  if (blockIdx.x == 0) {
#pragma clang fp contract(off)
    const double U2 = U * U;
    const double scale = skip ? 0.0 : a.max_abs_dp * U2;
    if (tid == 0) {
      double* o = a.scalars;
      o[0] = U; o[1] = c; o[2] = U2; o[3] = scale; o[4] = skip ? 1.0 : 0.0; o[5] = (double)a.frames; o[6] = 0.0; o[7] = 0.0;
      a.lu[0] = a.phi; a.lu[1] = U;
    }
    for (int b = tid; b < a.B; b += 256) a.row_scale[b] = (float)scale;
  }
  const int64_t cell = (int64_t)blockIdx.x * 256 + tid;
  if (cell >= a.n_grid) return;
  const int src = a.src_of_cell[cell];
  double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (src >= 0) {
    const int32_t* v = a.vtx + (int64_t)src * 3;
    const double* w = a.wts + (int64_t)src * 3;
    const double w0 = w[0], w1 = w[1], w2 = w[2];
    const bool neg = (w0 < 0.0) || (w1 < 0.0) || (w2 < 0.0);
    const PoissonCols c0 = poisson_cols(a, v[0], c, skip), c1 = poisson_cols(a, v[1], c, skip), c2 = poisson_cols(a, v[2], c, skip);
#pragma unroll
    for (int q = 0; q < 6; ++q) {                          // (without the weighting columns 4 and 5 are zeros and are not stored)
      double s = 0.0;                                      // the statements of interp_column, vertex by vertex
      s += c0.v[q] * w0;
      s += c1.v[q] * w1;
      s += c2.v[q] * w2;
      r[q] = neg ? NAN : s;                                // interpolate_fill
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) a.vel[q * a.n_grid + cell] = r[q];
  if (a.weighting) {
    a.w_plane[cell] = (r[4] != r[4]) ? 0.f : (float)r[4];  // a solver's tables carry negative weights (PM:210, no IDW fallback): a NaN here
    a.prev_plane[cell] = (r[5] != r[5]) ? 0.f : (float)r[5];   // would spread through the sigma_weight filter over its whole radius
  }
}
__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(PsmPoissonCellsArgs a) { poisson_partial(a); }
__global__ __launch_bounds__(256) void psm_interp_to_grid_kernel(PsmPoissonCellsArgs a) { poisson_to_grid(a); }

// Tail, grid -> mesh: dp[n] = sum_j field[cell_of_point[vtx[n][j]]] * wts[n][j] in float64, p = p(t-1) + dp, p(t-1) itself bit for
// bit where psm_to_mesh_kernel falls back (near-wall cell, negative weight, NaN: PM:494-496) and everywhere on a skipped step; then
// the same thread turns its cell's state over.  prime (uniform): the push alone -- no field, p = p(t-1), block 0 stores the scalars.
__device__ __forceinline__ void poisson_to_mesh(PsmPoissonMeshArgs a) {
#pragma clang fp contract(off)
  const bool skip = a.prime ? true : (a.scalars[4] != 0.0);
  if (a.prime && blockIdx.x == 0 && threadIdx.x == 0) {
    for (int q = 0; q < PSM_POISSON_SCALARS; ++q) a.scalars[q] = 0.0;
    a.scalars[5] = (double)a.frames;
  }
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_cells) return;
  const double* r = a.cells + n * 5;
  const double ux = r[0], uy = r[1], prev = r[4];
  double p = prev;
  if (!skip) {
    const int32_t* v = a.vtx + n * 3;
    const double* w = a.wts + n * 3;
    double acc = 0.0;
    bool neg = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double f = (double)a.field[a.cell_of_point[v[j]]];
      const double t = f * w[j];
      acc = acc + t;
      neg = neg || (w[j] < 0.0);
    }
    if (!(a.near_wall[n] || neg || acc != acc)) p = prev + acc;
  }
  a.p_out[n] = p;
  psm_uv2 du = psm_uv2{0.0, 0.0};
  if (a.frames > 0) {
    const psm_uv2 up = *reinterpret_cast<const psm_uv2*>(a.u_prev + n * 2);
    du = psm_uv2{ux - up.x, uy - up.y};
  }
  *reinterpret_cast<psm_uv2*>(a.du_prev + n * 2) = du;
  *reinterpret_cast<psm_uv2*>(a.u_prev + n * 2) = psm_uv2{ux, uy};
  a.p_prev[n] = prev;
}
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmPoissonMeshArgs a) { poisson_to_mesh(a); }

// ---- the case set (psm_solve_cases_poisson*, PsmPoissonCasesArgs in psm_mesh.h): the case is launch dimension y of all three
// launches; a workgroup reads its case's range from cell_off and runs the body above on the case's slices, so that a case of a set
// holds the bits the single mesh gives on the same tables, decides on its own whether its step is skipped and stores its own
// scalars, (phi, U) and row scales.  No atomics: a step is bit-reproducible.
__device__ __forceinline__ PsmPoissonCellsArgs case_poisson_cells(const PsmPoissonCasesArgs& a, int cs) {
  const int64_t c0 = a.cell_off[cs], g0 = (int64_t)cs * a.n_grid;
  PsmPoissonCellsArgs s{};
  s.cells = a.cells + c0 * 5; s.u_prev = a.u_prev + c0 * 2; s.du_prev = a.du_prev + c0 * 2; s.p_prev = a.p_prev + c0;
  s.n_cells = a.cell_off[cs + 1] - c0;
  s.partials = a.partials + (int64_t)cs * 2 * PSM_POISSON_PARTS; s.n_partials = a.n_parts;
  s.vtx = a.vtx_m2g + g0 * 3; s.wts = a.wts_m2g + g0 * 3; s.src_of_cell = a.src_of_cell + g0; s.n_grid = a.n_grid;
  s.vel = a.vel + g0 * 4;
  if (a.weighting) { s.w_plane = a.w_plane + g0; s.prev_plane = a.prev_plane + g0; }
  s.scalars = a.scalars + (int64_t)cs * PSM_POISSON_SCALARS; s.lu = a.lu + 2 * cs; s.row_scale = a.row_scale + (int64_t)cs * a.B; s.B = a.B;
  s.phi = a.phi; s.max_abs_dp = a.max_abs_dp; s.weighting = a.weighting; s.frames = a.frames;
  return s;
}
__device__ __forceinline__ PsmPoissonMeshArgs case_poisson_mesh(const PsmPoissonCasesArgs& a, int cs) {
  const int64_t c0 = a.cell_off[cs], g0 = (int64_t)cs * a.n_grid;
  PsmPoissonMeshArgs m{};
  m.cells = a.cells + c0 * 5; m.vtx = a.vtx_g2m + c0 * 3; m.wts = a.wts_g2m + c0 * 3; m.cell_of_point = a.cell_of_point + g0;
  m.field = a.prime ? nullptr : a.field + g0; m.near_wall = a.near_wall + c0; m.p_out = a.p_out + c0; m.n_cells = a.cell_off[cs + 1] - c0;
  m.u_prev = a.u_prev + c0 * 2; m.du_prev = a.du_prev + c0 * 2; m.p_prev = a.p_prev + c0;
  m.scalars = a.scalars + (int64_t)cs * PSM_POISSON_SCALARS; m.prime = a.prime; m.frames = a.frames;
  return m;
}
// head, level one: part blockIdx.x of case blockIdx.y; every (part, case) slot is written, 0.0 where a shorter case has no cell there
__global__ __launch_bounds__(1024) void psm_umax_partial_kernel(PsmPoissonCasesArgs a) { poisson_partial(case_poisson_cells(a, blockIdx.y)); }
// head, level two + mesh -> grid: workgroup 0 of a case stores that case's scalars
__global__ __launch_bounds__(256) void psm_interp_to_grid_kernel(PsmPoissonCasesArgs a) { poisson_to_grid(case_poisson_cells(a, blockIdx.y)); }
// tail: x covers the largest case, the workgroups beyond a shorter case's end return at once (as to_mesh_case)
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmPoissonCasesArgs a) { poisson_to_mesh(case_poisson_mesh(a, blockIdx.y)); }

hipError_t psm_launch_poisson_partial(const PsmPoissonCellsArgs& a, hipStream_t st) {
  if (a.n_cells < 1 || a.n_partials < 1 || a.n_partials > PSM_POISSON_PARTS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmPoissonCellsArgs)>(psm_umax_partial_kernel), dim3((unsigned)a.n_partials), dim3(1024), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_poisson_to_grid(const PsmPoissonCellsArgs& a, hipStream_t st) {
  if (a.n_grid < 1 || a.n_partials < 1 || a.n_partials > PSM_POISSON_PARTS || (a.weighting && (!a.w_plane || !a.prev_plane))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmPoissonCellsArgs)>(psm_interp_to_grid_kernel), dim3((unsigned)((a.n_grid + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_poisson_to_mesh(const PsmPoissonMeshArgs& a, hipStream_t st) {
  if (a.n_cells < 1 || !a.u_prev || !a.du_prev || !a.p_prev || !a.scalars || (!a.prime && !a.field)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmPoissonMeshArgs)>(psm_to_mesh_kernel), dim3((unsigned)((a.n_cells + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

typedef void (*PsmPoissonCasesKernel)(PsmPoissonCasesArgs);
static bool poisson_cases_ok(const PsmPoissonCasesArgs& a) {
  return a.n_cases >= 1 && a.cell_off && a.cells && a.u_prev && a.du_prev && a.p_prev && a.scalars;
}
hipError_t psm_launch_poisson_partial_cases(const PsmPoissonCasesArgs& a, hipStream_t st) {
  if (!poisson_cases_ok(a) || a.n_parts < 1 || a.n_parts > PSM_POISSON_PARTS || !a.partials) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<PsmPoissonCasesKernel>(psm_umax_partial_kernel), dim3((unsigned)a.n_parts, (unsigned)a.n_cases), dim3(1024), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_poisson_to_grid_cases(const PsmPoissonCasesArgs& a, hipStream_t st) {
  if (!poisson_cases_ok(a) || a.n_grid < 1 || a.n_parts < 1 || a.n_parts > PSM_POISSON_PARTS || !a.partials || !a.vel || !a.lu || !a.row_scale ||
      (a.weighting && (!a.w_plane || !a.prev_plane))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<PsmPoissonCasesKernel>(psm_interp_to_grid_kernel), dim3((unsigned)((a.n_grid + 255) / 256), (unsigned)a.n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_poisson_to_mesh_cases(const PsmPoissonCasesArgs& a, hipStream_t st) {
  if (!poisson_cases_ok(a) || a.max_cells < 1 || !a.p_out || (!a.prime && !a.field)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<PsmPoissonCasesKernel>(psm_to_mesh_kernel), dim3((unsigned)((a.max_cells + 255) / 256), (unsigned)a.n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The tail of the gradient-model step at the solver boundary (psm_solve_gradp*, PsmGradpMeshArgs in psm_mesh.h): grid -> mesh of the
// integrated plane q = p / U^2, an overload of the kernels of the same purpose above.  Float64, rounded operation by operation
// (`fp contract(off)`), so that NumPy restates a cell's p bit for bit.

// s = mean_y(3 q[y][nx-1] - q[y][nx-2]) / 3 over all ny rows (PM:472 on the integrated plane), by every thread of a 256-thread
// workgroup: rows tid, tid + 256, ... in order, wave fold, LDS fold in one fixed tree -- the chain idiom of psm_integ_cols_kernel.
// The 2 ny floats come out of L2; no atomics, so every workgroup of every run holds the same bits.
__device__ __forceinline__ double gradp_outlet_level(const float* q, int ny, int nx) {
#pragma clang fp contract(off)
  __shared__ double lvl_s[4];
  double t = 0.0;
  for (int y = threadIdx.x; y < ny; y += 256) {
    const float* r = q + (int64_t)y * nx + (nx - 2);
    const double last = (double)r[1], before = (double)r[0];
    const double three = 3.0 * last;
    t = t + (three - before);
  }
  for (int o = 32; o > 0; o >>= 1) t = t + __shfl_down(t, o, 64);
  if ((threadIdx.x & 63) == 0) lvl_s[threadIdx.x >> 6] = t;
  __syncthreads();
  const double sum = (lvl_s[0] + lvl_s[1]) + (lvl_s[2] + lvl_s[3]);
  return (sum / (double)ny) / 3.0;
}

// One body, called by the single-mesh kernel and by the case-set kernel alike.  A workgroup beyond the mesh's end (a shorter case of
// a set) returns as a whole, in front of the barrier of the level; workgroup 0 stores the scalars.
__device__ __forceinline__ void gradp_to_mesh(PsmGradpMeshArgs a) {
#pragma clang fp contract(off)
  if ((int64_t)blockIdx.x * 256 >= a.n_cells) return;                // uniform per workgroup
  const double s = a.reference == PSM_GRADP_LEVEL_OUTLET ? gradp_outlet_level(a.q, a.ny, a.nx) : 0.0;
  const double U = *a.umax;
  const double U2 = U * U;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* o = a.scalars;
    o[0] = U; o[1] = U2; o[2] = s; o[3] = a.sx; o[4] = a.sy; o[5] = 0.0; o[6] = 0.0; o[7] = 0.0;
  }
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.n_cells) return;
  const int32_t* v = a.vtx + n * 3;
  const double* w = a.wts + n * 3;
  double acc = 0.0;
  bool neg = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double d = (double)a.q[a.cell_of_point[v[j]]] - s;         // p_adim_unif = (q - s)[indices]  (PM:481)
    const double t = d * w[j];
    acc = acc + t;
    neg = neg || (w[j] < 0.0);
  }
  double p = acc * U2;                                               // PM:490 with max_abs_p = 1
  const double prev = a.cells[n * 5 + 4];
  if (a.near_wall[n] || neg || acc != acc) p = prev;                 // PM:494, 496 (interpolate_fill -> NaN)
  a.p_out[n] = p;
}
__device__ __forceinline__ PsmGradpMeshArgs case_gradp_mesh(const PsmGradpCasesArgs& a, int cs) {
  const int64_t c0 = a.cell_off[cs], g0 = (int64_t)cs * a.ny * a.nx;
  PsmGradpMeshArgs m{};
  m.cells = a.cells + c0 * 5; m.umax = a.umax + cs; m.vtx = a.vtx_g2m + c0 * 3; m.wts = a.wts_g2m + c0 * 3; m.cell_of_point = a.cell_of_point + g0;
  m.q = a.q + g0; m.near_wall = a.near_wall + c0; m.p_out = a.p_out + c0; m.n_cells = a.cell_off[cs + 1] - c0;
  m.ny = a.ny; m.nx = a.nx; m.reference = a.reference;
  m.scalars = a.scalars + (int64_t)cs * PSM_GRADP_SCALARS; m.sx = a.sx; m.sy = a.sy;
  return m;
}
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmGradpMeshArgs a) { gradp_to_mesh(a); }
// the case is launch dimension y, x covers the largest case (as to_mesh_case)
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmGradpCasesArgs a) { gradp_to_mesh(case_gradp_mesh(a, blockIdx.y)); }

static bool gradp_level_ok(int reference, int ny, int nx) {
  return (reference == PSM_GRADP_LEVEL_NONE || reference == PSM_GRADP_LEVEL_OUTLET) && ny >= 1 && nx >= 2;
}
hipError_t psm_launch_gradp_to_mesh(const PsmGradpMeshArgs& a, hipStream_t st) {
  if (a.n_cells < 1 || !a.cells || !a.umax || !a.vtx || !a.wts || !a.cell_of_point || !a.q || !a.near_wall || !a.p_out || !a.scalars ||
      !gradp_level_ok(a.reference, a.ny, a.nx)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmGradpMeshArgs)>(psm_to_mesh_kernel), dim3((unsigned)((a.n_cells + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_gradp_to_mesh_cases(const PsmGradpCasesArgs& a, hipStream_t st) {
  if (a.n_cases < 1 || a.max_cells < 1 || !a.cells || !a.cell_off || !a.umax || !a.vtx_g2m || !a.wts_g2m || !a.cell_of_point || !a.q || !a.near_wall ||
      !a.p_out || !a.scalars || !gradp_level_ok(a.reference, a.ny, a.nx)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmGradpCasesArgs)>(psm_to_mesh_kernel), dim3((unsigned)((a.max_cells + 255) / 256), (unsigned)a.n_cases), dim3(256), 0,
                     st, a);
  return hipGetLastError();
}
