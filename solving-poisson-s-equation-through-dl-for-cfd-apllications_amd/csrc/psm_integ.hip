// psm_integ.hip -- U_to_gradP: integration of the assembled (dp/dx, dp/dy) into p, for a whole case batch in two launches.
//
// Semantics: integrate_field (UGP:371-416) on four quadrants cut at (cy, cx) and the stitching of the left quadrants onto the
// right ones (UGP:597-628).  For a quadrant with reference corner column `ij` and row `ii` the reference's double loop reduces to
//     Phat[a,b] = (SdPy[a,ij] - SdPy[ii,ij]) + (SdPx[a,b] - SdPx[a,ij])
// i.e. one row-wise cumulative sum per quadrant row -- with the reference's "reset at the obstacle" index quirk, precomputed per
// quadrant-local row on the host as (v, u) pairs: aaa[v] = -(ccc[v] - ccc[u]) -- and ONE column-wise cumulative sum per side
// (column 0 for the left quadrants, column nx-1 for the right ones), restarted at the cut row.
//
// Launch 1, psm_integ_rows_kernel: one WAVE per (case, row, side).  The row of a side is scanned in chunks of 64 pixels (one
//   float2 per lane: both channels of a pixel in one request; __shfl_up scan over the 64 lanes, carry between chunks in a
//   register, the next chunk's load issued before the current chunk's scan).  The left side runs forwards from column 0
//   (SdPx[a,b] - SdPx[a,0]); the right side runs BACKWARDS from column nx-1, so that SdPx[a,b] - SdPx[a,nx-1] is minus the
//   exclusive scan and no row total is needed first.  The scaled scan goes straight into p (column cx-1 belongs to the left
//   side, as in the reference's order of assignments).  What launch 2 needs of a row is left in aux [case][row] (16 bytes):
//   dp/dy at columns 0 and nx-1 and both sides' scan values at column cx-1.
// Launch 2, psm_integ_cols_kernel: one workgroup per (case, PSM_INTEG_ROWS rows).  Every workgroup recomputes its case's four
//   column scans (left / right x top / bottom; the bottom half backwards from row ny-1, its reference row) and the two stitching
//   means from aux -- ny float4 out of L2, the idiom psm_assemble_kernel uses for the offset chain -- and adds yl[y] - corr /
//   yr[y] to its rows of p.  The mean over the paired flow cells of the two cut columns is taken as (sum over the left list -
//   sum over the right list) / n: the lists have equal length (checked by the bind), so the pairing itself does not matter.
//   An empty selection gives 0 / 0 = NaN like np.mean.
// No thread loops serially over a row or a column, no intermediate image; no LDS in launch 1, 0.2 KiB in launch 2.
#include "psm_launch.h"
#include "psm_integ.h"

namespace {

__device__ __forceinline__ float psm_wave_scan(float v, int lane) {      // inclusive scan over the 64 lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void psm_integ_rows_kernel(PsmIntegArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cs = blockIdx.y, y = blockIdx.x * 2 + (wave >> 1), side = wave & 1;
  if (y >= a.ny) return;                                          // whole waves; the kernel has no barrier
  const int2 cut = a.cuts[cs];
  const int cy = cut.x, cx = cut.y;
  const int x0 = side ? cx - 1 : 0, w = side ? a.nx - cx + 1 : cx;      // left block [0,cx), right block [cx-1,nx)
  const int64_t row = (int64_t)cs * a.ny + y;
  const float2* g = reinterpret_cast<const float2*>(a.gradp) + row * a.nx + x0;
  float* prow = a.p + row * a.nx + x0;
  float* aux = reinterpret_cast<float*>(a.aux + row);
  const int2* fx = a.fixups + ((int64_t)cs * a.ny + (y < cy ? y : y - cy)) * PSM_INTEG_MAX_FIX;   // quadrant-local row

  // "aaa[nn] = -dd": element v becomes -(ccc[v] - ccc[u]) with ccc the plain cumulative sum of the block row from its left end
  int fv[PSM_INTEG_MAX_FIX], fu[PSM_INTEG_MAX_FIX];
  float cv[PSM_INTEG_MAX_FIX], cu[PSM_INTEG_MAX_FIX];
  int last = -1;
#pragma unroll
  for (int e = 0; e < PSM_INTEG_MAX_FIX; ++e) {
    const int2 f = fx[e];
    fv[e] = (f.x >= 0 && f.x < w) ? f.x : -1;
    fu[e] = fv[e] >= 0 ? f.y : -1;
    cv[e] = cu[e] = 0.f;
    last = max(last, max(fv[e], fu[e]));
  }
  last = min(last, w - 1);
  float carry = 0.f;
  for (int base = 0; base <= last; base += 64) {                  // usually one chunk: the indices are int(sdf) values
    const int j = base + lane;
    const float s = psm_wave_scan(j < w ? g[j].x : 0.f, lane) + carry;
#pragma unroll
    for (int e = 0; e < PSM_INTEG_MAX_FIX; ++e) {
      if (fv[e] >= base && fv[e] < base + 64) cv[e] = __shfl(s, fv[e] - base, 64);
      if (fu[e] >= base && fu[e] < base + 64) cu[e] = __shfl(s, fu[e] - base, 64);
    }
    carry = __shfl(s, 63, 64);
  }

  const int n_chunks = (w + 63) / 64;
  auto load = [&](int c) {
    const int r = c * 64 + lane;
    return r < w ? g[side ? w - 1 - r : r] : make_float2(0.f, 0.f);
  };
  float2 cur = load(0);
  float first = 0.f;
  carry = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const float2 nxt = c + 1 < n_chunks ? load(c + 1) : make_float2(0.f, 0.f);
    const int r = c * 64 + lane;
    const bool valid = r < w;
    const int j = side ? w - 1 - r : r;                            // block column
    float x = cur.x;
#pragma unroll
    for (int e = 0; e < PSM_INTEG_MAX_FIX; ++e)
      if (valid && j == fv[e]) x = -(cv[e] - cu[e]);
    const float incl = psm_wave_scan(x, lane) + carry;
    float out;
    if (side == 0) {                                               // (SdPx[j] - SdPx[0]) * dx
      if (c == 0) first = __shfl(incl, 0, 64);
      out = (incl - first) * a.dx;
    } else {                                                       // (SdPx[j] - SdPx[w-1]) * dx = -(sum over the columns right of j) * dx
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = carry;
      out = -excl * a.dx;
    }
    carry = __shfl(incl, 63, 64);
    if (valid) {
      if (side == 0) {
        prow[j] = out;
        if (j == 0) aux[0] = cur.y;                                // dp/dy at column 0
        if (j == w - 1) aux[2] = out;                              // p2[:, -1] / p4[:, -1] without the column part
      } else {
        if (j > 0) prow[j] = out;
        else aux[3] = out;                                         // p1[:, 0] / p3[:, 0] without the column part
        if (j == w - 1) aux[1] = cur.y;                            // dp/dy at column nx-1
      }
    }
    cur = nxt;
  }
}

__global__ __launch_bounds__(256) void psm_integ_cols_kernel(PsmIntegArgs a) {
  __shared__ float4 wsum[4];
  __shared__ float red[2][4];
  __shared__ float addl[PSM_INTEG_ROWS], addr[PSM_INTEG_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cs = blockIdx.y, y0 = blockIdx.x * PSM_INTEG_ROWS;
  const int ny = a.ny;
  const int2 cut = a.cuts[cs];
  const int cy = cut.x, cx = cut.y;
  const float4* aux = a.aux + (int64_t)cs * ny;
  const uint8_t* mask = a.rowmask + (int64_t)cs * ny;
  const float4 row0 = aux[0];                                      // SdPy[0, ij] of the top quadrants
  float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);                  // (left top, left bottom, right top, right bottom)
  float acc_top = 0.f, acc_bot = 0.f;
  // scan position i: rows 0 .. cy-1 forwards, then rows ny-1 .. cy backwards (each half from its reference row)
  for (int base = 0; base < ny; base += 256) {
    const int i = base + tid;
    const bool valid = i < ny, top = i < cy;
    const int y = top ? i : ny - 1 - (i - cy);
    const float4 v = valid ? aux[y] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int m = valid ? mask[y] : 0;
    const float4 own = make_float4(top ? v.x : 0.f, top ? 0.f : v.x, top ? v.y : 0.f, top ? 0.f : v.y);
    float4 s;
    s.x = psm_wave_scan(own.x, lane); s.y = psm_wave_scan(own.y, lane);
    s.z = psm_wave_scan(own.z, lane); s.w = psm_wave_scan(own.w, lane);
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    float4 off = carry, tot = carry;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = wsum[q];
      if (q < wave) { off.x += t.x; off.y += t.y; off.z += t.z; off.w += t.w; }
      tot.x += t.x; tot.y += t.y; tot.z += t.z; tot.w += t.w;
    }
    carry = tot;
    // top: (SdPy[y] - SdPy[0]) * dy; bottom: (SdPy[y] - SdPy[ny-1]) * dy = -(sum over the rows below y) * dy
    const float yl = top ? (s.x + off.x - row0.x) * a.dy : -(s.y + off.y - own.y) * a.dy;
    const float yr = top ? (s.z + off.z - row0.y) * a.dy : -(s.w + off.w - own.w) * a.dy;
    if (valid) {
      const float d = ((m & 1) ? yl + v.z : 0.f) - ((m & 2) ? yr + v.w : 0.f);
      if (top) acc_top += d; else acc_bot += d;
      if (y >= y0 && y < y0 + PSM_INTEG_ROWS) { addl[y - y0] = yl; addr[y - y0] = yr; }
    }
    __syncthreads();                                               // wsum is rewritten by the next chunk
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    float t = q == 0 ? acc_top : acc_bot;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) red[q][wave] = t;
  }
  __syncthreads();
  const int2 np = a.npair[cs];
  const float corr_top = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)np.x;   // mean of an empty selection -> NaN like NumPy
  const float corr_bot = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (float)np.y;
  for (int r = wave; r < PSM_INTEG_ROWS && y0 + r < ny; r += 4) {
    const int y = y0 + r;
    const float al = addl[r] - (y < cy ? corr_top : corr_bot), ar = addr[r];
    float* prow = a.p + ((int64_t)cs * ny + y) * a.nx;
    for (int x = lane; x < a.nx; x += 64) prow[x] += x < cx ? al : ar;
  }
}

hipError_t psm_launch_integrate(const PsmIntegArgs& a, hipStream_t st) {
  PSM_LAUNCH(psm_integ_rows_kernel, dim3((a.ny + 1) / 2, a.n_cases), dim3(256), 0, st, a);
  PSM_LAUNCH(psm_integ_cols_kernel, dim3((a.ny + PSM_INTEG_ROWS - 1) / PSM_INTEG_ROWS, a.n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}
