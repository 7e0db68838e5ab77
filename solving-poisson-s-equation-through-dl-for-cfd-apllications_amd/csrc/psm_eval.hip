// psm_eval.hip -- evaluator kernels on the grid (evaluation only, nothing of a solve): label blocks with the flow-cell mean removed,
// and the eight error sums of compute_in_block_error -- per decoded block (psm_block_error) and for assembled fields
// (psm_field_errors_device).  Launchers in psm_eval.h.
#include "psm_eval.h"

// The eight sums of compute_in_block_error (pressureSM_deltas/utils.py:210-243) over a set of flow cells -- count and sum / sum of
// squares of the non-NaN differences pred - true, extrema of true and pred, count of NaN truths (np.max then gives NaN) -- float64
// like the reference's arrays.  Slots of the 8 doubles: psm_errors.h.  Every kernel below keeps its own pixel -> thread -> lane ->
// wave -> workgroup tree; this is what a node of any of them does.
struct PsmErrSums {
  double n = 0.0, s1 = 0.0, s2 = 0.0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, tnan = 0.0;
  __device__ __forceinline__ void add(double pr, double tr) {          // one element
    if (tr != tr) tnan += 1.0; else { tmin = fmin(tmin, tr); tmax = fmax(tmax, tr); }
    if (pr == pr) { pmin = fmin(pmin, pr); pmax = fmax(pmax, pr); }
    const double d = pr - tr;
    if (d == d) { n += 1.0; s1 += d; s2 += d * d; }
  }
  __device__ __forceinline__ void fold(const PsmErrSums& o) {          // this (+) o
    n += o.n; s1 += o.s1; s2 += o.s2; tnan += o.tnan;
    tmin = fmin(tmin, o.tmin); tmax = fmax(tmax, o.tmax); pmin = fmin(pmin, o.pmin); pmax = fmax(pmax, o.pmax);
  }
  __device__ __forceinline__ void fold_wave() {                        // 64 lanes -> lane 0
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      PsmErrSums d;
      d.n = __shfl_down(n, o, 64); d.s1 = __shfl_down(s1, o, 64); d.s2 = __shfl_down(s2, o, 64); d.tnan = __shfl_down(tnan, o, 64);
      d.tmin = __shfl_down(tmin, o, 64); d.tmax = __shfl_down(tmax, o, 64); d.pmin = __shfl_down(pmin, o, 64); d.pmax = __shfl_down(pmax, o, 64);
      fold(d);
    }
  }
  __device__ __forceinline__ void store(double* r, int stride = 1) const {
    r[0] = n; r[stride] = s1; r[2 * stride] = s2; r[3 * stride] = tmin; r[4 * stride] = tmax; r[5 * stride] = pmin; r[6 * stride] = pmax; r[7 * stride] = tnan;
  }
  static __device__ __forceinline__ PsmErrSums load(const double* r, int stride = 1) {
    PsmErrSums s;
    s.n = r[0]; s.s1 = r[stride]; s.s2 = r[2 * stride]; s.tmin = r[3 * stride]; s.tmax = r[4 * stride]; s.pmin = r[5 * stride]; s.pmax = r[6 * stride]; s.tnan = r[7 * stride];
    return s;
  }
};

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

// compute_in_block_error (called at SM_call.py:555-557 on the decoded blocks BEFORE the reassembly): the sums per workgroup over
// the flow cells of one block; `true` = label block * row_scale[b] (SM_call.py:555: y_array * max_abs_p * U_max_norm^2, the scale
// the decoded blocks already carry).  Partials [B][8] doubles, summed on the host.
__global__ __launch_bounds__(256) void psm_block_error_kernel(const float* grid, const float* pred, const float* label_blocks,
                                                              const float* row_scale, const int32_t* blk_y0x0, double* part,
                                                              int S, int c_in, int c_out, int sdf_ch, int Nx) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int y0 = blk_y0x0[2 * b], x0 = blk_y0x0[2 * b + 1];
  const double sc = (double)row_scale[b];
  PsmErrSums sums;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * Nx + x0 + i % S;
    if (!(grid[pix * c_in + sdf_ch] != 0.f)) continue;
    for (int c = 0; c < c_out; ++c) {
      const int64_t e = ((int64_t)b * S * S + i) * c_out + c;
      sums.add((double)pred[e], (double)label_blocks[e] * sc);
    }
  }
  __shared__ double sh[8][256];
  sums.store(&sh[0][t], 256);
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
// The same eight sums for ASSEMBLED fields (psm_field_errors_device; PsmFieldErrorArgs in psm_eval.h): the three error blocks the
// Poisson evaluator prints per frame (pressureSM_Poisson/SM_call.py:962-1043) without the fields leaving the device.  HBM-bound:
// a pair reads up to five planes once.  Launch 1, grid (workgroups over pixels, pair, frame): a thread takes 4 consecutive pixels
// per round -- one 16-byte load per float32 plane, two per float64 plane where the frame's plane is dense and 16-byte aligned,
// else one load per pixel (result [npix][c_out], odd plane offsets, the tail) --, sums in float64 like the reference's arrays,
// then wave shuffle -> LDS -> 8 doubles per workgroup.  Launch 2 folds a row of partials.  No atomics; pixel -> thread -> lane ->
// wave -> workgroup is a fixed tree, the same on either load path: a result depends on the inputs alone, bit for bit.
typedef float psm_f4 __attribute__((ext_vector_type(4)));

typedef double psm_d2 __attribute__((ext_vector_type(2)));
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
  PsmErrSums sums;
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
      sums.add((nan0(ad[e]) - nan0(sb[e])) + p[e], t0 ? nan0(tr[e]) : tr[e]);
    }
  }
  sums.fold_wave();
  __shared__ double red[4][8];
  if (lane == 0) sums.store(red[wave]);
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
  PsmErrSums sums;
  for (int w = lane; w < a.n_wg; w += 64) sums.fold(PsmErrSums::load(part + (int64_t)w * 8));
  sums.fold_wave();
  if (lane == 0) sums.store(a.raw + row * 8);
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

// ---------------------------------------------------------------------------
// compute_in_block_error for a batch of frames (psm_block_errors_device; PsmBlockErrorBatchArgs in psm_eval.h): workgroup (block,
// frame) does what psm_label_blocks_kernel and the first psm_block_error_kernel above do for case 0 in two launches, without the
// label block in between.  Pass 1 is the mean of psm_label_blocks_kernel -- its pixel -> thread partition (i = t, t + 256, ...), its
// float64 sums, its LDS tree --, so (float)(label - mean) holds the bits that kernel stores; pass 2 is the first kernel's loop and
// tree on (double)pred against (double)that float * row_scale[frame * B + block].  A frame's row of B partials therefore holds the
// bits psm_block_error sums for that frame.  The partition is kept for that reason: a wave reads 64 consecutive pixels of a block
// row per access (the image channel at a stride of c_in floats); pass 2 reads the block's label and mask a second time, from L2.
__global__ __launch_bounds__(256) void psm_block_error_kernel(PsmBlockErrorBatchArgs a) {
  const int b = blockIdx.x, t = threadIdx.x, S = a.S;
  const int64_t frame = blockIdx.y;
  const int y0 = a.blk_y0x0[2 * b], x0 = a.blk_y0x0[2 * b + 1];
  const float* grid = a.grid + frame * a.npix * a.c_in;
  const float* labels = a.label + frame * a.npix;
  const int64_t row = frame * a.B + b;
  const float* pred = a.pred + row * S * S;
  __shared__ double sh[8][256];
  double sum = 0.0, cnt = 0.0;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * a.Nx + x0 + i % S;
    if (grid[pix * a.c_in + a.sdf_ch] != 0.f) { sum += (double)labels[pix]; cnt += 1.0; }
  }
  sh[0][t] = sum; sh[1][t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) { sh[0][t] += sh[0][t + s]; sh[1][t] += sh[1][t + s]; }
    __syncthreads();
  }
  const double mean = sh[1][0] > 0.0 ? sh[0][0] / sh[1][0] : 0.0;
  __syncthreads();                                      // every thread has read the mean before the tree's rows are written again
  const double sc = (double)a.row_scale[row];
  PsmErrSums sums;
  for (int i = t; i < S * S; i += 256) {
    const int64_t pix = (int64_t)(y0 + i / S) * a.Nx + x0 + i % S;
    if (!(grid[pix * a.c_in + a.sdf_ch] != 0.f)) continue;
    const float lb = (float)((double)labels[pix] - mean);
    sums.add((double)pred[i], (double)lb * sc);
  }
  sums.store(&sh[0][t], 256);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sh[0][t] += sh[0][t + s]; sh[1][t] += sh[1][t + s]; sh[2][t] += sh[2][t + s]; sh[7][t] += sh[7][t + s];
      sh[3][t] = fmin(sh[3][t], sh[3][t + s]); sh[4][t] = fmax(sh[4][t], sh[4][t + s]);
      sh[5][t] = fmin(sh[5][t], sh[5][t + s]); sh[6][t] = fmax(sh[6][t], sh[6][t + s]);
    }
    __syncthreads();
  }
  if (t < 8) a.part[row * 8 + t] = sh[t][0];
}

// One workgroup per frame: thread q < 8 adds slot q of the frame's B partial rows in block order -- the statements of
// psm_block_error's host loop (sums from 0, std::min / std::max from +-inf) -- into the frame's block row of raw; threads 8-15
// copy the frame's field row in front of it where there is one.
__global__ __launch_bounds__(64) void psm_block_error_kernel(PsmBlockErrorFoldArgs a) {
  const int t = threadIdx.x;
  const int64_t frame = blockIdx.x;
  const int rows = a.field_raw ? 2 : 1;
  if (t < 8) {
    const double* q = a.part + frame * a.B * 8 + t;
    const bool lo = t == 3 || t == 5, hi = t == 4 || t == 6;
    double r = lo ? INFINITY : hi ? -INFINITY : 0.0;
    for (int b = 0; b < a.B; ++b) {
      const double v = q[(int64_t)b * 8];
      r = lo ? (v < r ? v : r) : hi ? (r < v ? v : r) : r + v;
    }
    a.raw[(frame * rows + rows - 1) * 8 + t] = r;
  } else if (t < 16 && a.field_raw) {
    a.raw[frame * 16 + t - 8] = a.field_raw[frame * 8 + t - 8];
  }
}

hipError_t psm_launch_block_error_batch(const PsmBlockErrorBatchArgs& a, hipStream_t st) {
  if (a.n_frames < 1 || a.B < 1 || a.S < 1 || a.npix < 1 || !a.grid || !a.label || !a.pred || !a.row_scale || !a.blk_y0x0 || !a.part)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmBlockErrorBatchArgs)>(psm_block_error_kernel), dim3((unsigned)a.B, (unsigned)a.n_frames), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t psm_launch_block_error_fold(const PsmBlockErrorFoldArgs& a, int n_frames, hipStream_t st) {
  if (n_frames < 1 || a.B < 1 || !a.part || !a.raw) return hipErrorInvalidValue;
  hipLaunchKernelGGL(static_cast<void (*)(PsmBlockErrorFoldArgs)>(psm_block_error_kernel), dim3((unsigned)n_frames), dim3(64), 0, st, a);
  return hipGetLastError();
}
