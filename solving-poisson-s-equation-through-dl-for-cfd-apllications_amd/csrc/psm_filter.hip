// psm_filter.hip -- the Gaussian post-steps of assemble_prediction (SM_call.py:352-363, UGP:366-367) for a case batch.
//
// Semantics: scipy.ndimage.gaussian_filter(order=0, mode='reflect', truncate=4) = correlate1d along axis 0, then along axis 1,
// with weights exp(-x^2 / 2 sigma^2) / sum over |x| <= int(4 sigma + 0.5) (computed in double on the host, rounded to float) and
// half-sample-symmetric boundaries ("reflect": d c b a | a b c d | d c b a; the radius may exceed the extent many times over).
//
// One pass = one launch of psm_gauss1d_kernel<AXIS, EPI> over [n_cases][ny][nx][c] float32:
//   AXIS 0  the image is ny rows of W = nx * c floats (the channels are just more columns).  A workgroup owns a strip of 64
//           columns x 16 output rows and stages rows y0 - r .. y0 + 15 + r of the strip into LDS, row by row: a wave loads 64
//           consecutive floats of one row (coalesced along x), and the reflection of that row's index is one wave-uniform modulo.
//           blockIdx.z also selects one of up to two jobs (field and weighting input, each with its own table and radius).
//   AXIS 1  a workgroup owns 256 pixels of 4 lines (a line = one row of one channel; the channels are de-interleaved while
//           staging) and stages x0 - r .. x0 + 255 + r of each, the reflection resolved per staged element.
// The taps of a pass are staged next to the data.  After the barrier the tap loop is LDS reads and FMAs only: a thread owns FOUR
// consecutive outputs along the filtered axis and walks the staged span in groups of four values, so one value read from LDS
// feeds up to four outputs (16 FMAs per 4 data reads + one broadcast read of 4 taps).  Every output is the plain sum over its
// taps in ascending order -- no atomics, no dependence on the batch size: case i of a batch is bit-identical to the same field
// alone, and an output is NaN exactly where a NaN lies under its taps (taps outside an output's window are never multiplied).
// A radius whose span does not fit the LDS budget is walked in chunks of `tap_chunk` taps, the span re-staged per chunk, the
// accumulators carried: the summation order stays the same.
//
// Epilogues of the AXIS 1 pass (c == 1):
//   EPI 1  result = filtered field (or the field itself without job 0), w = filtered weighting input (job 1);
//          t = (result - prev) * w is written next to result
//   EPI 2  change = filtered t; next = prev + change is written next to change
// so the whole tail with the weighting is 4 launches: AXIS 0 {field, dU} -> AXIS 1 EPI 1 -> AXIS 0 {t} -> AXIS 1 EPI 2.
#include <algorithm>

#include "psm_launch.h"
#include "psm_filter.h"

namespace {

constexpr int G0_COLS = 64, G0_ROWS = 16;      // AXIS 0 tile: 4 waves x 4 rows per thread
constexpr int G1_PIX = 256, G1_LINES = 4;      // AXIS 1 tile: one line per wave, 4 pixels per thread
constexpr int G_SLACK = 8;                     // staged-span slack: the last value group of a thread may reach past the span (never multiplied)

__device__ __forceinline__ int psm_reflect(int i, int n) {
  const int p = 2 * n;
  int j = i % p;
  if (j < 0) j += p;
  return j < n ? j : p - 1 - j;
}

// acc[j] += sum_t sw[4 + t] * sp[(j + t) * ES], t = 0 .. nt-1 ascending, for the thread's outputs j = 0..3
template <int ES>
__device__ __forceinline__ void psm_gauss_taps(const float* sp, const float* sw, int nt, float (&acc)[4]) {
  auto edge = [&](int m) {                     // a group at either end of the span: some of the 16 products lie outside the window
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = sp[(4 * m + i) * ES];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = 4 * m + i - j;
        if (t >= 0 && t < nt) acc[j] = fmaf(sw[4 + t], v[i], acc[j]);
      }
  };
  const int ng = (nt + 6) / 4, nfull = nt / 4;  // groups cover value offsets 0 .. nt+2; groups 1 .. nfull-1 hold all 16 products
  edge(0);
  const float4* sw4 = reinterpret_cast<const float4*>(sw);
  float4 wp = sw4[1];                          // taps 4m-4 .. 4m-1 of the group before
#pragma unroll 2
  for (int m = 1; m < nfull; ++m) {
    const float4 wc = sw4[m + 1];              // taps 4m .. 4m+3
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = sp[(4 * m + i) * ES];
    const float wt[7] = {wp.y, wp.z, wp.w, wc.x, wc.y, wc.z, wc.w};     // taps 4m-3 .. 4m+3
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(wt[3 + i - j], v[i], acc[j]);
    wp = wc;
  }
  for (int m = nfull > 1 ? nfull : 1; m < ng; ++m) edge(m);
}

// One filter of the workgroup's tile: stage (per tap chunk) and accumulate.  `src` is the case's plane(s).
template <int AXIS>
__device__ __forceinline__ void psm_gauss_tile(float* lds, int woff, const float* __restrict__ src, const float* __restrict__ w,
                                               int radius, int tap_chunk, int ny, int nx, int c, int y0, int x0, float (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntaps = 2 * radius + 1;
  float* sw = lds;
  float* sd = lds + woff;
  for (int t0 = 0; t0 < ntaps; t0 += tap_chunk) {
    const int nt = min(tap_chunk, ntaps - t0);
    __syncthreads();                           // the reads of the chunk (or of the filter) before are done
    for (int t = tid; t < nt; t += 256) sw[4 + t] = w[t0 + t];
    if (AXIS == 0) {
      const int W = nx * c, E = G0_ROWS + nt - 1, x = x0 + lane;
      for (int e = wave; e < E; e += 4) {
        const int y = psm_reflect(y0 + e + t0 - radius, ny);
        sd[e * G0_COLS + lane] = x < W ? src[(int64_t)y * W + x] : 0.f;
      }
      __syncthreads();
      psm_gauss_taps<G0_COLS>(sd + 4 * wave * G0_COLS + lane, sw, nt, acc);
    } else {
      const int E = G1_PIX + nt - 1, LP = (G1_PIX + tap_chunk + G_SLACK + 3) & ~3, line = y0 + wave;
      if (line < ny * c) {
        const int row = line / c, ch = line - row * c;
        const float* sl = src + (int64_t)row * nx * c + ch;
        for (int e = lane; e < E; e += 64) sd[wave * LP + e] = sl[(int64_t)psm_reflect(x0 + e + t0 - radius, nx) * c];
      }
      __syncthreads();
      psm_gauss_taps<1>(sd + wave * LP + 4 * lane, sw, nt, acc);
    }
  }
}

}  // namespace

template <int AXIS, int EPI>
__global__ __launch_bounds__(256) void psm_gauss1d_kernel(PsmGaussArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int job = blockIdx.z / a.n_cases, cs = blockIdx.z - job * a.n_cases;
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
  const int64_t plane = (int64_t)a.ny * a.nx * a.c, off = cs * plane;
  const int woff = (a.tap_chunk + G_SLACK + 3) & ~3;
  if (AXIS == 0) {
    const int x0 = tx * G0_COLS, y0 = ty * G0_ROWS, W = a.nx * a.c;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    psm_gauss_tile<0>(lds, woff, a.job[job].in + off, a.job[job].w, a.job[job].radius, a.tap_chunk, a.ny, a.nx, a.c, y0, x0, acc);
    const int x = x0 + lane;
    float* out = a.out[job] + off;
    if (x < W) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int y = y0 + 4 * wave + j;
        if (y < a.ny) out[(int64_t)y * W + x] = acc[j];
      }
    }
  } else {
    const int x0 = tx * G1_PIX, l0 = ty * G1_LINES;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, acw[4] = {0.f, 0.f, 0.f, 0.f};
    const bool filt = a.job[0].in != nullptr;
    if (filt) psm_gauss_tile<1>(lds, woff, a.job[0].in + off, a.job[0].w, a.job[0].radius, a.tap_chunk, a.ny, a.nx, a.c, l0, x0, acc);
    if (EPI == 1) psm_gauss_tile<1>(lds, woff, a.job[1].in + off, a.job[1].w, a.job[1].radius, a.tap_chunk, a.ny, a.nx, a.c, l0, x0, acw);
    const int line = l0 + wave;
    if (line >= a.ny * a.c) return;
    const int row = line / a.c, ch = line - row * a.c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + 4 * lane + j;
      if (x >= a.nx) break;
      const int64_t i = off + ((int64_t)row * a.nx + x) * a.c + ch;
      if (EPI == 0) {
        a.out[0][i] = acc[j];
      } else if (EPI == 1) {
        const float r = filt ? acc[j] : a.fields[i], pv = a.prev[i];
        if (a.result) a.result[i] = r;
        a.t[i] = (r - pv) * acw[j];
      } else {
        const float pv = a.next ? a.prev[i] : 0.f;
        if (a.change) a.change[i] = acc[j];
        if (a.next) a.next[i] = pv + acc[j];
      }
    }
  }
}

// ---- launcher ------------------------------------------------------------------------------------------------------
namespace {
int g_lds_cap = 64 * 1024;     // dynamic LDS a launch may ask for (psm_gauss_init raises it)

size_t gauss_lds_bytes(int axis, int tap_chunk) {
  const size_t woff = (size_t)((tap_chunk + G_SLACK + 3) & ~3);
  const size_t data = axis == 0 ? (size_t)(G0_ROWS + tap_chunk + G_SLACK) * G0_COLS
                                : (size_t)G1_LINES * ((G1_PIX + tap_chunk + G_SLACK + 3) & ~3);
  return (woff + data) * sizeof(float);
}
}  // namespace

// Once per process, outside any stream capture: allow the kernels the CU's whole LDS, so that a 64-wide strip with a radius-200
// halo either side (111 KB) is staged once.  Where the runtime refuses, the 64 KB default stays and wide spans go in tap chunks.
void psm_gauss_init() {
  static bool done = false;
  if (done) return;
  done = true;
  const int want = 160 * 1024;
  const void* k[4] = {(const void*)psm_gauss1d_kernel<0, 0>, (const void*)psm_gauss1d_kernel<1, 0>, (const void*)psm_gauss1d_kernel<1, 1>,
                      (const void*)psm_gauss1d_kernel<1, 2>};
  bool ok = true;
  for (auto f : k) ok = (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess) && ok;
  if (ok) g_lds_cap = want; else (void)hipGetLastError();
}

// taps per staged chunk: all of the widest table where the strip of the AXIS 0 pass fits the LDS budget
int psm_gauss_tap_chunk(int max_radius) {
  int fit = (g_lds_cap / (int)sizeof(float) - (G0_ROWS + G_SLACK) * G0_COLS - G_SLACK - 4) / (G0_COLS + 1);
  fit &= ~3;
  return std::min(2 * max_radius + 1, fit);
}

hipError_t psm_launch_gauss(PsmGaussArgs a, int axis, int epi, hipStream_t st) {
  if (a.n_cases < 1 || a.n_jobs < 1 || a.n_jobs > 2 || a.ny < 1 || a.nx < 1 || a.c < 1 || a.tap_chunk < 1) return hipErrorInvalidValue;
  if (axis == 1 && epi != 0 && a.c != 1) return hipErrorInvalidValue;
  const size_t lds = gauss_lds_bytes(axis, a.tap_chunk);
  if (lds > (size_t)g_lds_cap) return hipErrorInvalidValue;
  const int64_t tx = axis == 0 ? ((int64_t)a.nx * a.c + G0_COLS - 1) / G0_COLS : (a.nx + G1_PIX - 1) / G1_PIX;
  const int64_t ty = axis == 0 ? (a.ny + G0_ROWS - 1) / G0_ROWS : ((int64_t)a.ny * a.c + G1_LINES - 1) / G1_LINES;
  const int64_t nz = (int64_t)a.n_cases * (axis == 0 ? a.n_jobs : 1);
  if (tx * ty > 0x7fffffff || nz > 65535) return hipErrorInvalidValue;
  a.tiles_x = (int)tx;
  const dim3 grid((unsigned)(tx * ty), 1, (unsigned)nz);
  if (axis == 0) PSM_LAUNCH((psm_gauss1d_kernel<0, 0>), grid, dim3(256), lds, st, a);
  else if (epi == 0) PSM_LAUNCH((psm_gauss1d_kernel<1, 0>), grid, dim3(256), lds, st, a);
  else if (epi == 1) PSM_LAUNCH((psm_gauss1d_kernel<1, 1>), grid, dim3(256), lds, st, a);
  else PSM_LAUNCH((psm_gauss1d_kernel<1, 2>), grid, dim3(256), lds, st, a);
  return hipGetLastError();
}
