// psm_unet_mesh.hip -- mesh <-> canvas ends of the convolutional path at the solver boundary (psm_unet_solve*, include/psm_unet.h):
// the two launches around psm_unet_forward_device that take K meshes' cells [sum n_i, 5] = (Ux, Uy, Cx, Cy, p) float64 to the
// network's input images and its output fields back to p [sum n_i] float64.  The per-cell arithmetic is that of psm_mesh.hip's
// to_grid_cell / to_mesh_cell, statement by statement (float64, the same operation order, the same fallbacks: PM:272-297, 481-496;
// delta form SMD:389-391), so that the NumPy oracle's mesh_to_grid / grid_to_mesh restate both ends; what differs is the addressing:
// the image of case k lies at CANVAS pitch -- rows [0, ny) x columns [0, nx) of canvas k [ny_c][nx_c] (PsmUnetMeshArgs in
// psm_unet_mesh.h) -- and the pixels outside it are never written.  The first launch of a step, the partial maxima of the squared
// speed per case, is psm_launch_umax_cases of psm_mesh.hip as it is.  The two kernels carry the names of their family in
// psm_mesh.hip (psm_to_grid_kernel, psm_to_mesh_kernel: "mesh <-> grid" in the kernel tables of the tests) and are told apart by
// their argument type, like that file's overloads: psm_to_grid_kernel<DELTA>(PsmUnetMeshArgs) is the mesh -> CANVAS end.
//
// Both kernels are gathers through 16 k-cell tables that sit in L2 between steps; a step's cost is its launches.  A thread reads
// its table rows ([3] int32 + [3] float64, 12- and 24-byte rows: neighbouring threads read neighbouring rows, so a wave's loads
// cover one contiguous range) and gathers 3 x 2 (3 x 4 in delta form) doubles; the image's 12-byte pixels leave through LDS so that
// every store instruction of a wave writes 256 consecutive bytes.
#include "psm_unet_mesh.h"

#include "psm_mesh_dev.h"

// mesh -> canvas.  Launch: x covers the ny * nx image cells in row-major order, 256 per workgroup; y is the case.  Every workgroup
// folds its case's row of partial maxima (the barrier inside is reached by all 256 threads: nobody returns before it), workgroup 0
// of the case leaves U_max[case] for the tail.  Then one thread per image cell: the value of the grid point NumPy's fancy
// assignment leaves in that cell (src_of_cell: last writer, -1 = nobody -> 0), U / U_max (DELTA: (U - U(t-1)) / U_max, U_max of the
// CURRENT cells) interpolated over the point's three vertices, interpolate_fill's NaN for a negative weight, / max_abs_*, NaN -> 0,
// and the SDF channel.  The three floats go to LDS, and the workgroup stores its 768 floats in three rounds of 256 consecutive
// ones: float f of the workgroup belongs to pixel f / 3, whose cell gives (ii, jj) and with it the address at canvas pitch.
template <bool DELTA>
__global__ __launch_bounds__(256) void psm_to_grid_kernel(PsmUnetMeshArgs a) {
  __shared__ float px[256 * 3];
  const int cs = blockIdx.y, tid = threadIdx.x;
  const double umax_v = umax_of_partials(a.umax_part + (int64_t)cs * a.n_parts, a.n_parts);
  if (blockIdx.x == 0 && tid == 0) a.umax[cs] = umax_v;
  const int64_t n_grid = (int64_t)a.ny * a.nx, g0 = (int64_t)cs * n_grid;
  const int64_t cell0 = (int64_t)blockIdx.x * 256, cell = cell0 + tid;
  float ux = 0.f, uy = 0.f, sdv = 0.f;
  if (cell < n_grid) {
    const int src = a.src_of_cell[g0 + cell];
    if (src >= 0) {
      const int64_t c0 = a.cell_off[cs];
      const double* cells = a.cells + c0 * 5;
      const double inv = 1.0 / umax_v;
      const int32_t* v = a.vtx_m2g + (g0 + src) * 3;
      const double* w = a.wts_m2g + (g0 + src) * 3;
      double sx = 0.0, sy = 0.0;
      bool neg = false;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double* c = cells + (int64_t)v[j] * 5;
        double cx = c[0], cy = c[1];
        if (DELTA) {
          const psm_uv2 q = *reinterpret_cast<const psm_uv2*>(a.u_prev + (c0 + v[j]) * 2);
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
    const double sd = a.sdf[g0 + cell] * a.sdf_scale;   // PM:292 (raw) / SMD:443 (divided by max_abs_dist)
    sdv = (sd != sd) ? 0.f : (float)sd;
  }
  px[tid * 3] = ux; px[tid * 3 + 1] = uy; px[tid * 3 + 2] = sdv;
  __syncthreads();
  float* canvas = a.canvas + (int64_t)cs * a.ny_c * a.nx_c * 3;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int f = r * 256 + tid, q = f / 3;
    const int64_t cq = cell0 + q;
    if (cq >= n_grid) continue;              // the last workgroup's tail: no pixel, nothing stored
    const int ii = (int)(cq / a.nx), jj = (int)(cq - (int64_t)ii * a.nx);
    canvas[((int64_t)ii * a.nx_c + jj) * 3 + (f - q * 3)] = px[f];
  }
}

// canvas -> mesh.  Launch: x covers the largest case, 256 cells per workgroup, y is the case; the workgroups beyond a shorter
// case's end return at once.  One thread per mesh cell: the field at the three vertices' pixels (pixel_of_point: `indices` at
// canvas pitch), acc in float64, p = acc * max_abs_p * U_max^2, and cells[:,4] where the reference falls back (near-wall cell,
// negative weight, NaN: PM:494-496).  DELTA: the field is dp, p = p(t-1) + dp by one rounded add, p(t-1) itself where it falls
// back; `prime` (uniform): no field and no U_max are read, p = p(t-1) everywhere; then the thread leaves its cell's (Ux, Uy) in
// u_prev -- the state turns over in the step's last launch, behind every reader of the old one in stream order.
template <bool DELTA>
__global__ __launch_bounds__(256) void psm_to_mesh_kernel(PsmUnetMeshArgs a) {
  const int cs = blockIdx.y;
  const int64_t c0 = a.cell_off[cs], local = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (local >= a.cell_off[cs + 1] - c0) return;
  const int64_t n = c0 + local;
  const bool prime = DELTA && a.prime;
  const double* row = a.cells + n * 5;
  double acc = 0.0, um = 0.0;
  bool neg = false;
  if (!prime) {
    const int32_t* v = a.vtx_g2m + n * 3;
    const double* w = a.wts_g2m + n * 3;
    const int32_t* pix = a.pixel_of_point + (int64_t)cs * a.ny * a.nx;
    const float* field = a.field + (int64_t)cs * a.ny_c * a.nx_c;
    um = a.umax[cs];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc += (double)field[pix[v[j]]] * w[j];                        // p_adim_unif = result[indices]  (PM:481)
      neg = neg || (w[j] < 0.0);
    }
  }
  double p = acc * a.max_abs_p * (um * um);                          // PM:490
  const double prev = row[4];
  if (DELTA) p = add_np(prev, p);
  if (prime || a.near_wall[n] || neg || acc != acc) p = prev;        // PM:494, 496 (interpolate_fill -> NaN)
  a.p_out[n] = p;
  if (DELTA) *reinterpret_cast<psm_uv2*>(a.u_prev + n * 2) = psm_uv2{row[0], row[1]};
}

static bool unet_mesh_ok(const PsmUnetMeshArgs& a, bool delta) {
  return a.n_cases >= 1 && a.cells && a.cell_off && a.ny >= 1 && a.nx >= 1 && a.ny_c >= a.ny && a.nx_c >= a.nx && (!delta || a.u_prev);
}
hipError_t psm_launch_unet_to_canvas(const PsmUnetMeshArgs& a, bool delta, hipStream_t st) {
  if (!unet_mesh_ok(a, delta) || a.n_parts < 1 || a.n_parts > 256 || !a.umax_part || !a.umax || !a.vtx_m2g || !a.wts_m2g || !a.src_of_cell || !a.sdf ||
      !a.canvas) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)a.ny * a.nx + 255) / 256), (unsigned)a.n_cases);
  if (delta) hipLaunchKernelGGL(psm_to_grid_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(psm_to_grid_kernel<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_unet_to_mesh(const PsmUnetMeshArgs& a, bool delta, hipStream_t st) {
  const bool prime = delta && a.prime;
  if (!unet_mesh_ok(a, delta) || a.max_cells < 1 || !a.near_wall || !a.p_out ||
      (!prime && (!a.umax || !a.vtx_g2m || !a.wts_g2m || !a.pixel_of_point || !a.field))) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.max_cells + 255) / 256), (unsigned)a.n_cases);
  if (delta) hipLaunchKernelGGL(psm_to_mesh_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(psm_to_mesh_kernel<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
