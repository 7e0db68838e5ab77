// psm_rows.hip -- the head of the evaluators' frame steps on the device: a frame's dataset rows as stored (float32, row-major, cut at
// `indice`) -> the per-frame scalars and the float64 columns the frame entries take.  Two launches for the batch, the frame is
// launch dimension y:
//   partial : psm_umax_partial_kernel(PsmRowsArgs) -- maxima per (frame, part) of |U| = sqrt(r0^2 + r1^2), |dU| = sqrt(r5^2 + r6^2) and c = |r5 - r8| + |r6 - r9|
//   finish  : psm_stage_cells_kernel(PsmRowsArgs) -- every workgroup folds its frame's <= 256 partials itself (as psm_to_grid_kernel folds umax_partials), derives the
//             scalars and writes its 256 cells' columns; workgroup 0 of a frame stores the frame's scalars -- into `scalars` and
//             into the device arrays the step's kernels read (row scale, U^2 of the deltas pack, (L, U) of the features)
// The arithmetic is NumPy's on float32 operands, statement by statement (Evaluation.timeSteps, EvaluationPoisson.timeSteps,
// EvaluationGradP.timeSteps in surrogate.py): every product, sum, square root and quotient is rounded on its own, in float32, and
// only then widened -- so `#pragma clang fp contract(off)` around all of it (hipcc contracts a * a + b * b into an fma otherwise; what
// that costs is in the comment on speed2_np, psm_mesh.hip).  A maximum is np.max: a NaN anywhere makes it NaN.  No atomics; a
// maximum does not depend on the order of its fold, so the scalars are bit-reproducible.
// A row is width * 4 bytes, with width 11 neither 8- nor 16-byte aligned: the columns are read with scalar float loads.
#include "psm_rows.h"

namespace {

__device__ __forceinline__ float nanmax2f(float a, float b) { return (b > a || b != b) ? b : a; }

// np.sqrt(np.square(x) + np.square(y)) on float32
__device__ __forceinline__ float norm2_np(float x, float y) {
#pragma clang fp contract(off)
  const float xx = x * x, yy = y * y;
  const float s = xx + yy;
  return sqrtf(s);
}

// np.abs(delta_U - delta_U_prev).sum(axis=-1) on float32
__device__ __forceinline__ float change_np(float a5, float a6, float a8, float a9) {
#pragma clang fp contract(off)
  const float d0 = a5 - a8, d1 = a6 - a9;
  return fabsf(d0) + fabsf(d1);
}

__device__ __forceinline__ float wave_nanmax(float m) {
  for (int o = 32; o > 0; o >>= 1) m = nanmax2f(m, __shfl_down(m, o, 64));
  return m;
}

// What a frame's three maxima make of it.  u / u2: what the columns are divided by; U_out ... scale: the frame's scalars.
struct RowScalars {
  float u, u2;
  double U_out, U2_out, scale;
  float scale32;
  bool relevant;
};

__device__ __forceinline__ RowScalars row_scalars(const PsmRowsArgs& a, float U, float dU) {
#pragma clang fp contract(off)
  RowScalars s;
  s.u = U;
  s.u2 = U * U;                                            // pow(U_max_norm, 2.0) on a float32
  s.relevant = true;
  if (a.kind == PSM_ROWS_KIND_DELTAS) {
    const float q = dU / U;
    s.relevant = !(q < 1e-4f);                             // the skip rule of Evaluation.timeSteps -- a NaN compares false: relevant
    s.scale32 = (float)a.base * s.u2;                      // max_abs_p * U ** 2: a Python float times a float32 is a float32
    s.scale = (double)s.scale32;
  } else if (a.kind == PSM_ROWS_KIND_POISSON) {
    const float q = dU / U;
    s.relevant = !(q < 1e-4f || dU < 1e-6f || U < 1e-6f);  // the skip rule of EvaluationPoisson.timeSteps
    const double Ud = (double)U;
    const double Ud2 = Ud * Ud;                            // U is a Python float there: float64, and exact
    s.scale = a.base * Ud2;
    s.scale32 = (float)s.scale;                            // the cast of the row-scale upload
  } else {
    s.scale = 1.0;
    s.scale32 = 1.0f;
  }
  s.U_out = (double)U;
  s.U2_out = (double)s.u2;
  if (!s.relevant) { s.u = s.u2 = 1.0f; s.U_out = s.U2_out = 1.0; s.scale = 0.0; s.scale32 = 0.0f; }
  return s;
}

}  // namespace

// The two kernels are overloads of the solver boundary's kernels of the same purpose (psm_mesh.hip: partial maxima of the speed; cells
// staged for the mesh -> grid launch), on a batch of float32 frames.
__global__ __launch_bounds__(256) void psm_umax_partial_kernel(PsmRowsArgs a) {
  __shared__ float red[3][4];
  const int tid = threadIdx.x, frame = blockIdx.y;
  const float* rows = a.rows + (int64_t)frame * a.n_cells * a.width;
  float mU = 0.f, mD = 0.f, mC = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * PSM_ROWS_CHUNK + tid; i < a.n_cells; i += (int64_t)gridDim.x * PSM_ROWS_CHUNK) {
    const float* r = rows + i * a.width;
    mU = nanmax2f(mU, norm2_np(r[0], r[1]));
    if (a.kind != PSM_ROWS_KIND_GRADP) mD = nanmax2f(mD, norm2_np(r[5], r[6]));
    if (a.kind == PSM_ROWS_KIND_POISSON) mC = nanmax2f(mC, change_np(r[5], r[6], r[8], r[9]));
  }
  mU = wave_nanmax(mU); mD = wave_nanmax(mD); mC = wave_nanmax(mC);
  if ((tid & 63) == 0) { red[0][tid >> 6] = mU; red[1][tid >> 6] = mD; red[2][tid >> 6] = mC; }
  __syncthreads();
  if (tid < 3)
    a.part[((int64_t)frame * 3 + tid) * a.n_parts + blockIdx.x] = nanmax2f(nanmax2f(red[tid][0], red[tid][1]), nanmax2f(red[tid][2], red[tid][3]));
}

__global__ __launch_bounds__(256) void psm_stage_cells_kernel(PsmRowsArgs a) {
#pragma clang fp contract(off)
  __shared__ float red[3][4];
  const int tid = threadIdx.x, frame = blockIdx.y;
  const float* part = a.part + (int64_t)frame * 3 * a.n_parts;
  const int p = min(tid, a.n_parts - 1);
  const float fU = wave_nanmax(part[p]), fD = wave_nanmax(part[a.n_parts + p]), fC = wave_nanmax(part[2 * a.n_parts + p]);
  if ((tid & 63) == 0) { red[0][tid >> 6] = fU; red[1][tid >> 6] = fD; red[2][tid >> 6] = fC; }
  __syncthreads();
  const float U = nanmax2f(nanmax2f(red[0][0], red[0][1]), nanmax2f(red[0][2], red[0][3]));
  const float dU = nanmax2f(nanmax2f(red[1][0], red[1][1]), nanmax2f(red[1][2], red[1][3]));
  const float c = nanmax2f(nanmax2f(red[2][0], red[2][1]), nanmax2f(red[2][2], red[2][3]));
  const RowScalars s = row_scalars(a, U, dU);
  if (blockIdx.x == 0) {
    if (tid == 0) {
      double* o = a.scalars + (int64_t)frame * PSM_ROWS_SCALARS;
      o[0] = s.U_out; o[1] = (double)dU; o[2] = (double)c; o[3] = s.relevant ? 1.0 : 0.0;
      o[4] = s.U2_out; o[5] = s.scale; o[6] = 0.0; o[7] = 0.0;
      if (a.u2) a.u2[frame] = s.U2_out;
      if (a.lu) { a.lu[2 * frame] = a.phi; a.lu[2 * frame + 1] = s.U_out; }
    }
    if (a.row_scale)
      for (int b = tid; b < a.B; b += 256) a.row_scale[(int64_t)frame * a.B + b] = s.scale32;
  }
  const int64_t cell = (int64_t)blockIdx.x * PSM_ROWS_CHUNK + tid;
  if (cell >= a.n_cells) return;
  const float* r = a.rows + ((int64_t)frame * a.n_cells + cell) * a.width;
  if (a.kind == PSM_ROWS_KIND_DELTAS) {
    double* o = a.cols + ((int64_t)frame * a.n_cells + cell) * 3;
    if (!s.relevant) { o[0] = o[1] = o[2] = 0.0; return; }
    const float v0 = r[5] / s.u, v1 = r[6] / s.u, v2 = r[7] / s.u2;     // delta_U / U, delta_p / pow(U, 2.0)
    o[0] = (double)v0; o[1] = (double)v1; o[2] = (double)v2;
  } else if (a.kind == PSM_ROWS_KIND_POISSON) {
    double* o = a.cols + ((int64_t)frame * a.n_cells + cell) * 8;
    if (!s.relevant) { for (int q = 0; q < 8; ++q) o[q] = 0.0; return; }
    const float w = change_np(r[5], r[6], r[8], r[9]) / c;              // deltaU_changed / deltaU_changed.max()
    o[0] = (double)r[0]; o[1] = (double)r[1]; o[2] = (double)r[5]; o[3] = (double)r[6];      // the order of the concatenate
    o[4] = (double)r[7]; o[5] = (double)r[2]; o[6] = (double)w; o[7] = (double)r[10];
  } else {
    double* o = a.cols + ((int64_t)frame * a.n_cells + cell) * 5;
    const float gx = r[6] * a.ex, gy = r[7] * a.ey;                     // dPdx * (max_x - min_x): a float32 array times a float32 scalar
    const float v0 = r[0] / s.u, v1 = r[1] / s.u, v2 = gx / s.u2, v3 = gy / s.u2, v4 = r[2] / s.u2;
    o[0] = (double)v0; o[1] = (double)v1; o[2] = (double)v2; o[3] = (double)v3; o[4] = (double)v4;
  }
}

hipError_t psm_launch_rows_partial(const PsmRowsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(psm_umax_partial_kernel, dim3((unsigned)a.n_parts, (unsigned)a.n_frames), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t psm_launch_rows_finish(const PsmRowsArgs& a, hipStream_t st) {
  const unsigned wgs = (unsigned)((a.n_cells + PSM_ROWS_CHUNK - 1) / PSM_ROWS_CHUNK);
  hipLaunchKernelGGL(psm_stage_cells_kernel, dim3(wgs, (unsigned)a.n_frames), dim3(256), 0, st, a);
  return hipGetLastError();
}
