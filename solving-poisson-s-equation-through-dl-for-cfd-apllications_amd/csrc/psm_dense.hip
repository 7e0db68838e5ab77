// psm_dense.hip -- the network between the two PCA contractions, hand-written for gfx950 (CDNA4, wave64): kernels and launchers.
//
//   reduce  : split-K slab reduction + affine input scaler         [PM:351, SMD:505-523]
//   dense   : Keras Dense (x@W+b, ReLU / linear head + inverse scaler) [PM:121-134, SMD:532-539]
//
// psm_reduce_kernel, psm_reduce_dense1_kernel (reduce + first layer in one launch), psm_conv1d_kernel (conv1D_PCA head),
// psm_dense_kernel (with the strip-dot and geometry-guard riders of the bound path), psm_layernorm_kernel, and the strip dots
// as launches of their own (psm_act_dots_kernel, psm_res_dots_kernel).
#include "psm_kernels.h"
#include "psm_devutil.h"
#include "psm_mfma.h"
#include "psm_stamps.h"

// ---------------------------------------------------------------------------
// reduce (+ input scaler): 16 waves x 16 slabs in flight per lane, one round trip
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void psm_reduce_kernel(PsmReduceArgs a) {
  __shared__ float red[16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t total = (int64_t)a.Mpad * a.ldp;
  const int64_t o = (int64_t)blockIdx.x * 64 + lane;
  const int per = (a.n_slices + 15) / 16;
  const int s0 = wave * per, s1 = min(a.n_slices, s0 + per);
  const float* p = a.part + o;
  PSM_STAMP(0, 16);
  float acc = 0.f;
  int s = s0;
  for (; s + 16 <= s1; s += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(int64_t)(s + u) * total];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += v[u];       // fixed order: deterministic
  }
  for (; s + 4 <= s1; s += 4) {                     // fewer than 16 slabs per wave (K groups, slice pairs): still every load of a batch in flight together
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = p[(int64_t)(s + u) * total];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += v[u];
  }
  for (; s < s1; ++s) acc += p[(int64_t)s * total];
  red[wave][lane] = acc;
  __syncthreads();
  PSM_STAMP(0, 17);
  if (wave == 0) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) v += red[w][lane];
    const int col = (int)(o % a.ldp);
    a.xin[o] = v * a.ia[col] + a.ib[(o / a.ldp) * a.ib_stride + col];
  }
}

hipError_t psm_launch_reduce(const PsmReduceArgs& a, hipStream_t st) {
  const int64_t total = (int64_t)a.Mpad * a.ldp;
  PSM_LAUNCH(psm_reduce_kernel, dim3((unsigned)(total / 64)), dim3(1024), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// reduce + first dense layer in one launch (small row counts): one workgroup per block row
// (and column half of the layer) sums the row's split-K slabs, applies the input scaler and,
// having the WHOLE coefficient row in LDS, finishes x@W1+b1, ReLU for its columns on the
// VALU -- the contraction is only p_in (<= 512) long.  Saves a launch (~5 us) over
// psm_reduce_kernel + psm_dense_kernel; slab summation order is that of psm_reduce_kernel.
// ---------------------------------------------------------------------------
template <bool BF16>
__global__ __launch_bounds__(1024) void psm_reduce_dense1_kernel(PsmReduceArgs r, PsmDenseArgs d) {
  __shared__ float red[16][512];
  __shared__ __attribute__((aligned(16))) float xrow[512];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = blockIdx.x;
  const int64_t total = (int64_t)r.Mpad * r.ldp;
  const int per = (r.n_slices + 15) / 16;
  const int s0 = wave * per, s1 = min(r.n_slices, s0 + per);
  PSM_STAMP(0, 8);
  // first-layer weights of this thread's first column / K quarter: independent of the slabs, so
  // they are requested first and arrive under the slab reduction.  Addresses are a wave-uniform
  // row base plus a 32-bit lane offset.
  const int ncols = d.ld_w / gridDim.y, n0 = blockIdx.y * ncols;
  const int kp = wave >> 2, kq = d.Kpad / 4;               // 4 waves (256 columns) per K quarter
  const int nl0 = tid & 255;
  const int ncol0 = n0 + min(nl0, ncols - 1);
  float wv0[32];
  if (!BF16) {
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const float* wrow = d.W + (int64_t)(kp * kq + min(u, kq - 1)) * d.ld_w;     // uniform
      wv0[u] = wrow[ncol0];
    }
  }
  // input-scaler operands of the coefficient this thread finishes below
  const int pfin = min(tid, r.ldp - 1);
  const float ia_v = r.ia[pfin], ib_v = r.ib[(int64_t)m * r.ib_stride + pfin];
  const float bias0 = d.bias[n0 + min(tid, ncols - 1)];
  __builtin_amdgcn_sched_barrier(0);
  // slab sums: wave w adds slabs [16w, 16w+16) for two 64-column groups per pass, all 32 loads
  // of a pass in flight together (n_slices == 256: per == 16)
  for (int p0 = 0; p0 < r.ldp; p0 += 128) {
    const int pc0 = p0 + lane, pc1 = p0 + 64 + lane;
    const int o0 = m * r.ldp + min(pc0, r.ldp - 1), o1 = m * r.ldp + min(pc1, r.ldp - 1);
    float acc0 = 0.f, acc1 = 0.f;
    int s = s0;
    for (; s + 16 <= s1; s += 16) {
      float v0[16], v1[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float* slab = r.part + (int64_t)(s + u) * total;                     // uniform
        v0[u] = slab[o0];
        v1[u] = slab[o1];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) acc0 += v0[u];     // fixed order: that of psm_reduce_kernel
#pragma unroll
      for (int u = 0; u < 16; ++u) acc1 += v1[u];
    }
    for (; s + 8 <= s1; s += 8) {                  // 128 slabs (slice pairs): 8 per wave, all 16 loads in flight together
      float v0[8], v1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float* slab = r.part + (int64_t)(s + u) * total;                     // uniform
        v0[u] = slab[o0];
        v1[u] = slab[o1];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc0 += v0[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc1 += v1[u];
    }
    for (; s < s1; ++s) { const float* slab = r.part + (int64_t)s * total; acc0 += slab[o0]; acc1 += slab[o1]; }
    if (pc0 < r.ldp) red[wave][pc0] = acc0;
    if (pc1 < r.ldp) red[wave][pc1] = acc1;
  }
  __syncthreads();
  PSM_STAMP(0, 9);
  float x_keep = 0.f;
  if (tid < r.ldp) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) v += red[w][tid];
    x_keep = v * ia_v + ib_v;
    xrow[tid] = BF16 ? (float)(__bf16)x_keep : x_keep;
  }
  __syncthreads();
  // ---- x @ W1 + b1, ReLU: thread = (column, quarter of K); K = d.Kpad (multiple of 32)
  float* part4 = &red[0][0];                                           // [4][ncols <= 512]
  for (int nl = nl0; nl < ncols; nl += 256) {
    const int n = n0 + nl;
    float acc = 0.f;
    if (BF16) {
      const __bf16* w = reinterpret_cast<const __bf16*>(d.W) + (int64_t)(kp * kq) * d.ld_w + n;
      for (int k = 0; k < kq; ++k) acc = fmaf(xrow[kp * kq + k], (float)w[(int64_t)k * d.ld_w], acc);
    } else {
      // kq is a multiple of 8; up to 32 weight rows in flight per thread (one round trip for
      // p_in <= 128), k ascending.  Branch-free: rows beyond kq are clamped loads with a zero
      // weight, so that the LDS reads and FMAs of a chunk are one straight line.
      for (int k = 0; k < kq; k += 32) {
        float wv[32];
        if (k == 0 && nl == nl0) {
#pragma unroll
          for (int u = 0; u < 32; ++u) wv[u] = wv0[u];
        } else {
#pragma unroll
          for (int u = 0; u < 32; ++u) {
            const float* wrow = d.W + (int64_t)(kp * kq + min(k + u, kq - 1)) * d.ld_w;
            wv[u] = wrow[n];
          }
        }
        f32x4 xv[8];
#pragma unroll
        for (int u4 = 0; u4 < 8; ++u4)
          xv[u4] = *reinterpret_cast<const f32x4*>(&xrow[kp * kq + min(k + 4 * u4, kq - 4)]);
#pragma unroll
        for (int u4 = 0; u4 < 8; ++u4) {
          const bool in = (k + 4 * u4 < kq);                     // uniform; kq is a multiple of 4
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = fmaf(xv[u4][j], in ? wv[4 * u4 + j] : 0.f, acc);
        }
      }
    }
    part4[kp * 512 + nl] = acc;
  }
  __syncthreads();
  PSM_STAMP(0, 10);
  for (int nl = tid; nl < ncols; nl += 1024) {
    const int n = n0 + nl;
    float v = ((part4[nl] + part4[512 + nl]) + (part4[1024 + nl] + part4[1536 + nl])) + (nl == tid ? bias0 : d.bias[n]);
    if (d.relu) v = fmaxf(v, 0.f);
    if (d.head) v = v * d.sa[n] + d.sb[n];
    d.out[(int64_t)m * d.ld_out + n] = v;
  }
  // scaled coefficients, kept for psm_read_stage: stored last so that no barrier waits for them
  if (blockIdx.y == 0 && tid < r.ldp) r.xin[(int64_t)m * r.ldp + tid] = x_keep;
  PSM_STAMP(0, 11);
}

hipError_t psm_launch_reduce_dense1(const PsmReduceArgs& r, const PsmDenseArgs& d, hipStream_t st) {
  if (r.ldp > 512 || d.ld_w > 1024 || (d.ld_w / 2) % 1 != 0) return hipErrorInvalidValue;
  const dim3 grid(r.Mpad, 2);                        // (4 or 8 column workgroups per row: 4.64-4.76 us against 4.72 -- no difference)
  if (d.bf16) PSM_LAUNCH((psm_reduce_dense1_kernel<true>), grid, dim3(1024), 0, st, r, d);
  else PSM_LAUNCH((psm_reduce_dense1_kernel<false>), grid, dim3(1024), 0, st, r, d);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Conv1D over the PCA coefficients (conv1D_PCA head, NNs.py:75-124; the reference's 'conv1D' architecture has 7 layers of
// 128-64-32-16-32-64-128 filters, kernel 3, utils.py:452-454).  A rarely used head on <= a few hundred block rows of
// <= 128 positions: plain float32 FMAs, a thread owns 4 consecutive positions of one output channel (one weight load
// feeds 4 FMAs; lanes run over the output channels, so weight loads are coalesced and activation loads broadcast).
__global__ __launch_bounds__(256) void psm_conv1d_kernel(PsmConv1dArgs a) {
  const int m = blockIdx.y;
  const int items = ((a.P + 3) / 4) * a.c_out;
  const int item = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (item >= items) return;
  const int pt = item / a.c_out, co = item - pt * a.c_out;
  const int p0 = 4 * pt - (a.k - 1) / 2;                    // Keras 'same': (k - 1) / 2 zeros in front
  const float* in = a.in + (int64_t)m * a.in_stride;
  const float bv = a.bias[co];
  float acc[4] = {bv, bv, bv, bv};
  for (int t = 0; t < a.k; ++t) {
    const float* w = a.W + (int64_t)t * a.c_in * a.c_out + co;
    int pos[4]; float keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + t + j;
      keep[j] = (p >= 0 && p < a.P) ? 1.f : 0.f;
      pos[j] = min(max(p, 0), a.P - 1) * a.c_in;
    }
    for (int ci = 0; ci < a.c_in; ++ci) {
      const float wv = w[(int64_t)ci * a.c_out];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(in[pos[j] + ci] * keep[j], wv, acc[j]);
    }
  }
  float* out = a.out + (int64_t)m * a.out_stride;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int p = 4 * pt + j;
    if (p < a.P) out[(int64_t)p * a.c_out + co] = a.relu ? fmaxf(acc[j], 0.f) : acc[j];
  }
}

hipError_t psm_launch_conv1d(const PsmConv1dArgs& a, hipStream_t st) {
  if (a.M < 1 || a.P < 1 || a.k < 1 || a.k > 15 || a.c_in < 1 || a.c_out < 1) return hipErrorInvalidValue;
  const int items = ((a.P + 3) / 4) * a.c_out;
  PSM_LAUNCH(psm_conv1d_kernel, dim3((items + 255) / 256, a.M), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// dense layer: v_mfma_f32_16x16x4_f32, one 16-column tile x 32 rows per workgroup,
// K split over 8 waves, operands prefetched to registers in one round trip.
//   A: lane l holds A[i = l&15][k = l>>4];  B: lane l holds B[k = l>>4][j = l&15]
//   D: lane l, reg r holds D[4*(l>>4) + r][l&15]
// k order inside a group of 16: step j uses k = 16g + 4*(l>>4) + j (one float4 of A per lane).
// ---------------------------------------------------------------------------
// BF16: weights stored as bf16, activations rounded to bf16 on load; products are then exact
// and the f32 MFMA accumulates them exactly like v_mfma_*_bf16 would (this layer is latency
// bound, the bf16 storage only halves its weight bytes).
//
// Weights come MFMA-packed (psm_api_model.cpp, pack_dense): the four k of a lane's group are one
// 16-byte (bf16: 8-byte) piece and a wave's group is 1 KiB contiguous, so the whole operand set
// of a wave (NGC groups: 2*NGC + NGC loads per lane) is requested up front, unconditionally, and
// the MFMAs wait on it with counted vmcnt -- one memory round trip per pass.  Columns of the
// activation row beyond ld_in are clamped (their weights are zero rows).
// ROWS = 16 (few block rows: twice the workgroups, each pulling 2/3 of the bytes -- the layer
// is bound by what ONE CU can pull per round trip) or 32 (weights read once per 32 rows).

// DOTS (head layer of the geometry-bound path): workgroups with blockIdx.z > 0 do not compute the layer but the
// strip dot products of psm_kernels.h (PsmDotsArgs) from the same input activation: one wave per two table rows,
// every load issued up front (clamped), out[row] = scale * (act . g2[row] + c2[row]) / cnt[row]  (0/0 = NaN for an
// empty strip, like np.mean([])).
// LNIN (hidden layers of densePCA_attention): the input carries a pending LayerNormalization (PsmDenseArgs::ln_*) -- moments of
// the workgroup's own rows in a prologue, operands normalised on their way into the MFMAs, optional residual in the epilogue.
// float4 number q (columns 4 q .. 4 q + 3) of row `row` of a Dense input: rows of ld_in floats, or the packed form of PsmDenseArgs
__device__ __forceinline__ f32x4 psm_act_q(const PsmDenseArgs& a, int row, int q) {
  if (a.in_rows) return reinterpret_cast<const f32x4*>(a.in_rows + (int64_t)row * a.ld_in)[q];
  if (a.in_packed) return reinterpret_cast<const f32x4*>(a.in)[((int64_t)(row >> 4) * (a.ld_in >> 4) + (q >> 2)) * 64 + (q & 3) * 16 + (row & 15)];
  return reinterpret_cast<const f32x4*>(a.in + (int64_t)row * a.ld_in)[q];
}

template <int NGC, bool BF16, int ROWS, bool DOTS, bool LNIN = false>   // NGC: groups of 16 k per wave per pass
__global__ __launch_bounds__(512) void psm_dense_kernel(PsmDenseArgs a, PsmDotsArgs d) {
  psm_warm_kernargs<sizeof(PsmDenseArgs) + sizeof(PsmDotsArgs)>();
  // (One column tile of 16 per workgroup.  Two, for 576 block rows x 512 columns = 576 workgroups on 512 slots, measured no gain: 7.7 / 8.7 us
  // either way -- the layer is 4.3 us of latency + 147 456 float32 MFMAs of 32 cycles on 1024 SIMDs; profiles/r05_case_batch.txt (6a).)
  if (!DOTS && blockIdx.z > 0) {                       // guard riders behind a hidden layer (large case batches)
    const int wg = ((int)(blockIdx.z - 1) * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
    psm_guard_wg<8>(d.guard, wg, threadIdx.x >> 6, threadIdx.x & 63);
    return;
  }
  if (DOTS && blockIdx.z > 0) {
    constexpr int RPW = 2, NQ = 4;                     // rows per wave; float4 per lane and row (Kh <= 1024)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wg = ((int)(blockIdx.z - 1) * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
    const bool wave_rows = d.n_src > 1 && d.n_rows > PSM_DOTS_WG_ROWS;      // closed form, many rows: two rows per workgroup
    const int n_dot_wgs = d.n_src > 1 ? (wave_rows ? (d.n_rows + 1) / 2 : d.n_rows) : (d.n_rows + 8 * RPW - 1) / (8 * RPW);
    if (wg >= n_dot_wgs) {                               // guard riders behind the dots workgroups (uniform per workgroup)
      psm_guard_wg<8>(d.guard, wg - n_dot_wgs, wave, lane);
      return;
    }
    const int nq = d.Kh / 4;
    if (wave_rows) {
      // closed form, case batches of more than PSM_DOTS_WG_ROWS rows: TWO rows per workgroup -- four waves per row, wave q of a
      // row takes the source blocks q, q + 4, ... (four per batch, all loads of a batch up front; up to 16 blocks are one round
      // trip), the partial sums meet in LDS.  64 cases x 9 rows: 288 workgroups instead of 576 behind the head's 144.
      __shared__ float lsum2[8];
      const int rsel = wave >> 2, q4 = wave & 3;
      const int row = wg * 2 + rsel, rc = min(row, d.n_rows - 1);
      const int cs = rc / d.rows_per_case;
      const f32x4* gp = reinterpret_cast<const f32x4*>(d.g2) + (int64_t)rc * d.n_src * nq;
      const int arow_base = cs * d.n_src;
      const float rsv = d.row_scale[cs * d.n_src];
      float acc = 0.f;
      for (int b0 = q4; b0 < d.n_src; b0 += 16) {
        f32x4 gg[4][NQ], xx[4][NQ];
        float cc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int blk = min(b0 + 4 * t, d.n_src - 1);
          cc[t] = d.c2[(int64_t)rc * d.n_src + blk];
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            const int q = min(lane + 64 * u, nq - 1);
            gg[t][u] = gp[(int64_t)blk * nq + q];
            xx[t][u] = psm_act_q(a, arow_base + blk, q);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool on = b0 + 4 * t < d.n_src;
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            const float s4 = (gg[t][u].x * xx[t][u].x + gg[t][u].y * xx[t][u].y) + (gg[t][u].z * xx[t][u].z + gg[t][u].w * xx[t][u].w);
            acc += (on && lane + 64 * u < nq) ? s4 : 0.f;
          }
          acc += (on && lane == 0) ? cc[t] : 0.f;
        }
      }
      const float tot = wave_sum(acc);
      if (lane == 0) lsum2[wave] = tot;
      __syncthreads();
      if (lane == 0 && q4 == 0 && row < d.n_rows) d.out[row] = rsv * ((lsum2[4 * rsel] + lsum2[4 * rsel + 1]) + (lsum2[4 * rsel + 2] + lsum2[4 * rsel + 3]));
      return;
    }
    if (d.n_src > 1) {
      // closed form: one WORKGROUP per row -- wave w takes the source blocks w, w + 8, ... (four per batch, all loads of a
      // batch up front), the eight partial sums meet in LDS
      __shared__ float lsum[8];
      const int row = wg, rc = min(row, d.n_rows - 1);
      const int cs = rc / d.rows_per_case;
      const f32x4* gp = reinterpret_cast<const f32x4*>(d.g2) + (int64_t)rc * d.n_src * nq;
      const int arow_base = cs * d.n_src;
      const float rsv = d.row_scale[cs * d.n_src];
      float acc = 0.f;
      for (int b0 = wave; b0 < d.n_src; b0 += 32) {
        f32x4 gg[4][NQ], xx[4][NQ];
        float cc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int blk = min(b0 + 8 * t, d.n_src - 1);
          cc[t] = d.c2[(int64_t)rc * d.n_src + blk];
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            const int q = min(lane + 64 * u, nq - 1);
            gg[t][u] = gp[(int64_t)blk * nq + q];
            xx[t][u] = psm_act_q(a, arow_base + blk, q);
          }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool on = b0 + 8 * t < d.n_src;
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            const float s4 = (gg[t][u].x * xx[t][u].x + gg[t][u].y * xx[t][u].y) + (gg[t][u].z * xx[t][u].z + gg[t][u].w * xx[t][u].w);
            acc += (on && lane + 64 * u < nq) ? s4 : 0.f;
          }
          acc += (on && lane == 0) ? cc[t] : 0.f;
        }
      }
      const float tot = wave_sum(acc);
      if (lane == 0) lsum[wave] = tot;
      __syncthreads();
      if (threadIdx.x == 0 && row < d.n_rows) {
        float t8 = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) t8 += lsum[w8];
        d.out[row] = rsv * t8;
      }
      return;
    }
    f32x4 g[RPW][NQ], x[RPW][NQ];
    float c2[RPW], cn[RPW], rs[RPW];
    int row[RPW];
#pragma unroll
    for (int t = 0; t < RPW; ++t) {
      row[t] = (wg * 8 + wave) * RPW + t;
      const int rc = min(row[t], d.n_rows - 1);
      const int blk = d.row_of[rc];
      c2[t] = d.c2[rc]; cn[t] = d.cnt[rc]; rs[t] = d.row_scale[blk];
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int q = min(lane + 64 * u, nq - 1);
        g[t][u] = reinterpret_cast<const f32x4*>(d.g2)[(int64_t)rc * nq + q];
        x[t][u] = psm_act_q(a, blk, q);
      }
    }
#pragma unroll
    for (int t = 0; t < RPW; ++t) {
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const float s4 = (g[t][u].x * x[t][u].x + g[t][u].y * x[t][u].y) + (g[t][u].z * x[t][u].z + g[t][u].w * x[t][u].w);
        acc += (lane + 64 * u < nq) ? s4 : 0.f;
      }
      const float tot = wave_sum(acc);
      if (lane == 0 && row[t] < d.n_rows) d.out[row[t]] = rs[t] * (tot + c2[t]) / cn[t];
    }
    return;
  }
  __shared__ float red[8][2][16 * 17];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x, mt = blockIdx.y;
  const int i = lane & 15, kq = lane >> 4;
  const int groups = a.Kp / 16;                      // all waves
  const int ng = groups / 8;                         // per wave: a multiple of NGC
  PSM_STAMP(0, 44 + 4 * (a.layer & 3));
  // epilogue operands of this thread's output column: in flight from the start
  const int n_out = nt * 16 + (tid & 15);
  const float bias_v = a.bias[n_out];
  const float sa_v = a.head ? a.sa[n_out] : 1.f, sb_v = a.head ? a.sb[n_out] : 0.f;
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  const float* arow0 = a.in + (int64_t)(mt * ROWS + i) * a.ld_in;
  const float* arow1 = arow0 + (int64_t)16 * a.ld_in;
  const int g_first = wave * ng;
  const int kmax = a.ld_in - 4;
  auto rnd = [](float v) { return BF16 ? (float)(__bf16)v : v; };
  // ---- operand loads, normalisation and matrix step of NGC groups (one pass of the contraction)
  auto load_a = [&](int g0, f32x4 (&a0)[NGC], f32x4 (&a1)[NGC]) {
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      const int kcol = min(16 * (g_first + g0 + g) + 4 * kq, kmax);
      a0[g] = *reinterpret_cast<const f32x4*>(arow0 + kcol);
      if (ROWS == 32) a1[g] = *reinterpret_cast<const f32x4*>(arow1 + kcol);
    }
  };
  auto load_gb = [&](int g0, f32x4 (&gm)[NGC], f32x4 (&bt)[NGC]) {       // columns beyond ln_n carry gamma = beta = 0 (and zero weight rows)
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      const int kcol = min(16 * (g_first + g0 + g) + 4 * kq, kmax);
      gm[g] = *reinterpret_cast<const f32x4*>(a.ln_gamma + kcol);
      bt[g] = *reinterpret_cast<const f32x4*>(a.ln_beta + kcol);
    }
  };
  auto load_w = [&](int g0, f32x4 (&w)[NGC]) {
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      const int64_t widx = ((int64_t)nt * groups + g_first + g0 + g) * 64 + lane;
      if (BF16) {
        const uint2 u = reinterpret_cast<const uint2*>(a.Wp)[widx];
        w[g] = (f32x4){__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                       __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
      } else {
        w[g] = reinterpret_cast<const f32x4*>(a.Wp)[widx];
      }
    }
  };
  auto load_aw = [&](int g0, f32x4 (&a0)[NGC], f32x4 (&a1)[NGC], f32x4 (&w)[NGC]) {
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      const int kcol = min(16 * (g_first + g0 + g) + 4 * kq, kmax);
      if (!LNIN && !BF16 && ROWS == 32 && a.in_packed) {                 // uniform: one contiguous KiB per wave and row tile
        const int gin = a.ld_in >> 4;
        const f32x4* pk = reinterpret_cast<const f32x4*>(a.in) + ((int64_t)(2 * mt) * gin + min(g_first + g0 + g, gin - 1)) * 64 + lane;
        a0[g] = pk[0];
        a1[g] = pk[(int64_t)gin * 64];
      } else {
        a0[g] = *reinterpret_cast<const f32x4*>(arow0 + kcol);
        if (ROWS == 32) a1[g] = *reinterpret_cast<const f32x4*>(arow1 + kcol);
      }
      const int64_t widx = ((int64_t)nt * groups + g_first + g0 + g) * 64 + lane;
      if (BF16) {
        const uint2 u = reinterpret_cast<const uint2*>(a.Wp)[widx];
        w[g] = (f32x4){__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                       __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
      } else {
        w[g] = reinterpret_cast<const f32x4*>(a.Wp)[widx];
      }
      __builtin_amdgcn_sched_barrier(0);               // keeps the groups' requests in this order (the scheduler clusters the row loads otherwise)
    }
  };
  auto mma = [&](const f32x4 (&a0)[NGC], const f32x4 (&a1)[NGC], const f32x4 (&w)[NGC]) {
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      acc0 = MFMA16(rnd(a0[g].x), w[g].x, acc0); if (ROWS == 32) acc1 = MFMA16(rnd(a1[g].x), w[g].x, acc1);
      acc0 = MFMA16(rnd(a0[g].y), w[g].y, acc0); if (ROWS == 32) acc1 = MFMA16(rnd(a1[g].y), w[g].y, acc1);
      acc0 = MFMA16(rnd(a0[g].z), w[g].z, acc0); if (ROWS == 32) acc1 = MFMA16(rnd(a1[g].z), w[g].z, acc1);
      acc0 = MFMA16(rnd(a0[g].w), w[g].w, acc0); if (ROWS == 32) acc1 = MFMA16(rnd(a1[g].w), w[g].w, acc1);
    }
  };
  // ---- pending LayerNormalization of the input: moments of rows i (and i + 16) over the first ln_n columns, two passes like
  // tf.nn.moments.  Lane (i, kq) of wave w owns columns 16 (g_first + g) + 4 kq + j; the four kq lanes of a row meet through
  // two shuffles, the eight waves through LDS (the `red` buffer, free until the MFMA results are written).  A contraction of
  // one pass (K <= 512: ng == NGC) takes the moments from its operand registers -- the row is loaded once, with the weights
  // and gamma / beta already in flight; longer rows are read from L2 again for each pass.
  __shared__ float ln_stat[2][32];
  float mean0 = 0.f, rstd0 = 1.f, mean1 = 0.f, rstd1 = 1.f, res_raw = 0.f, res_g = 0.f, res_b = 0.f;
  f32x4 p0[NGC], p1[NGC], pw[NGC], pg[NGC], pb[NGC];
  const bool single = LNIN && ng == NGC;                 // uniform
  if constexpr (LNIN) {
    if (single) { load_a(0, p0, p1); load_gb(0, pg, pb); load_w(0, pw); }
    if (a.ln_residual && tid < ROWS * 16) {              // the epilogue's residual operands: in flight from here
      const int row = tid >> 4;
      res_raw = a.in[(int64_t)(mt * ROWS + row) * a.ld_in + n_out];
      res_g = a.ln_gamma[n_out]; res_b = a.ln_beta[n_out];
    }
    const float inv_n = 1.f / (float)a.ln_n;
    auto meet = [&](float s0, float s1, float& o0, float& o1) {
      s0 += __shfl_xor(s0, 16, 64); s0 += __shfl_xor(s0, 32, 64);
      s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
      if (kq == 0) { red[wave][0][i] = s0; red[wave][1][i] = s1; }
      __syncthreads();
      float t0 = 0.f, t1 = 0.f;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) { t0 += red[w8][0][i]; t1 += red[w8][1][i]; }
      __syncthreads();                                   // everyone has read the partials: `red` may be rewritten
      o0 = t0 * inv_n; o1 = t1 * inv_n;
    };
    auto row_moment = [&](float m0, float m1, bool second, float& o0, float& o1) {
      float s0 = 0.f, s1 = 0.f;
      if (single) {
#pragma unroll
        for (int g = 0; g < NGC; ++g) {
          const int k0 = 16 * (g_first + g) + 4 * kq;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < a.ln_n;
            const float d0 = p0[g][j] - m0, d1 = (ROWS == 32 ? p1[g][j] : p0[g][j]) - m1;
            s0 += in ? (second ? d0 * d0 : d0) : 0.f;
            s1 += in ? (second ? d1 * d1 : d1) : 0.f;
          }
        }
      } else {
        for (int g = 0; g < ng; ++g) {
          const int k0 = 16 * (g_first + g) + 4 * kq, kc = min(k0, kmax);
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(arow0 + kc);
          f32x4 v1 = v0;
          if (ROWS == 32) v1 = *reinterpret_cast<const f32x4*>(arow1 + kc);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bool in = k0 + j < a.ln_n;
            const float d0 = v0[j] - m0, d1 = v1[j] - m1;
            s0 += in ? (second ? d0 * d0 : d0) : 0.f;
            s1 += in ? (second ? d1 * d1 : d1) : 0.f;
          }
        }
      }
      meet(s0, s1, o0, o1);
    };
    float q0, q1;
    row_moment(0.f, 0.f, false, mean0, mean1);
    row_moment(mean0, mean1, true, q0, q1);
    rstd0 = rsqrtf(q0 + a.ln_eps); rstd1 = rsqrtf(q1 + a.ln_eps);
    if (wave == 0 && kq == 0) {
      ln_stat[0][i] = mean0; ln_stat[1][i] = rstd0;
      if (ROWS == 32) { ln_stat[0][16 + i] = mean1; ln_stat[1][16 + i] = rstd1; }
    }
  }
  auto normalise = [&](f32x4 (&a0)[NGC], f32x4 (&a1)[NGC], const f32x4 (&gm)[NGC], const f32x4 (&bt)[NGC]) {
#pragma unroll
    for (int g = 0; g < NGC; ++g) {
      a0[g] = (a0[g] - mean0) * rstd0 * gm[g] + bt[g];
      if (ROWS == 32) a1[g] = (a1[g] - mean1) * rstd1 * gm[g] + bt[g];
    }
  };
  if (single) {
    normalise(p0, p1, pg, pb);
    mma(p0, p1, pw);
  } else {
    for (int g0 = 0; g0 < ng; g0 += NGC) {
      f32x4 a0[NGC], a1[NGC], w[NGC];
      if constexpr (LNIN) {
        f32x4 gm[NGC], bt[NGC];
        load_a(g0, a0, a1);
        load_gb(g0, gm, bt);
        load_w(g0, w);
        normalise(a0, a1, gm, bt);
      } else {
        // requests in the order the MFMAs consume them -- (rows, weights) of k group 0, then of group 1, ...: loads return in issue
        // order, so the first group's MFMAs need vmcnt(3 (NGC - 1)) instead of everything but the last weight groups, and the
        // matrix steps of group g run while groups g + 1 ... are still arriving (round 6; was: all rows, then all weights)
        load_aw(g0, a0, a1, w);
      }
      __builtin_amdgcn_sched_barrier(0);               // every request of the pass before its first MFMA (the scheduler had sunk half of them behind it: two round trips)
      mma(a0, a1, w);
    }
  }
  PSM_STAMP(0, 45 + 4 * (a.layer & 3));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wave][0][(4 * kq + r) * 17 + i] = acc0[r];
    if (ROWS == 32) red[wave][1][(4 * kq + r) * 17 + i] = acc1[r];
  }
  __syncthreads();
  if (tid < ROWS * 16) {
    const int row = tid >> 4, col = tid & 15;          // ROWS rows x 16 cols
    const int half = row >> 4, r16 = row & 15;
    float v = 0.f;
#pragma unroll
    for (int w8 = 0; w8 < 8; ++w8) v += red[w8][half][r16 * 17 + col];
    v += bias_v;
    if (a.relu) v = fmaxf(v, 0.f);
    if constexpr (LNIN) {
      if (a.ln_residual) v += (res_raw - ln_stat[0][row]) * ln_stat[1][row] * res_g + res_b;     // x + LN(input) (NNs.py:64)
    }
    if (a.head) v = v * sa_v + sb_v;
    if (!LNIN && !BF16 && ROWS == 32 && a.out_packed) {
      a.out[psm_packed_offset(mt * ROWS + row, n_out, a.ld_out >> 4)] = v;
      if (a.out_rows) a.out_rows[(int64_t)(mt * ROWS + row) * a.ld_out + n_out] = v;
    } else a.out[(int64_t)(mt * ROWS + row) * a.ld_out + n_out] = v;
  }
  PSM_STAMP(0, 46 + 4 * (a.layer & 3));
}

hipError_t psm_launch_dense(const PsmDenseArgs& a, hipStream_t st, const PsmGuardArgs* riders) {
  const int ng = a.Kp / 128;                       // groups of 16 k per wave
  if (!a.Wp || a.Kp % 128 != 0 || (ng > 2 && ng % 4 != 0) || a.ld_in < 4) return hipErrorInvalidValue;
  const bool r16 = a.Mpad <= 128;     // up to 128 block rows: 16-row tiles keep >= 64 workgroups pulling <= 64 KB each
  if ((a.in_packed || a.out_packed) && (r16 || a.bf16 || a.ln_gamma || (a.in_packed && (a.ld_in % 16 != 0 || a.Kp > a.ld_in)) || (a.out_packed && a.ld_out % 16 != 0)))
    return hipErrorInvalidValue;       // packed activations: float32 layers on 32-row tiles, no pending LayerNormalization
  const int gx = a.ld_w / 16, gy = a.Mpad / (r16 ? 16 : 32);
  PsmDotsArgs rd{};
  int gz = 1;
  if (riders && riders->sdf && riders->wg_count > 0) { rd.guard = *riders; gz = 1 + (riders->wg_count + gx * gy - 1) / (gx * gy); }
  const dim3 grid(gx, gy, gz), blk(512);
#define DENSE2(N, L)                                                                        \
  do {                                                                                      \
    if (r16) {                                                                              \
      if (a.bf16) PSM_LAUNCH((psm_dense_kernel<N, true, 16, false, L>), grid, blk, 0, st, a, rd); \
      else PSM_LAUNCH((psm_dense_kernel<N, false, 16, false, L>), grid, blk, 0, st, a, rd);       \
    } else {                                                                                \
      if (a.bf16) PSM_LAUNCH((psm_dense_kernel<N, true, 32, false, L>), grid, blk, 0, st, a, rd); \
      else PSM_LAUNCH((psm_dense_kernel<N, false, 32, false, L>), grid, blk, 0, st, a, rd);       \
    }                                                                                       \
  } while (0)
#define DENSE(N) do { if (a.ln_gamma) DENSE2(N, true); else DENSE2(N, false); } while (0)
  if (psm_launch_probe) psm_launch_probe->tag = a.layer;          // every Dense layer is its own entry of psm_time_kernels
  if (a.ln_gamma && (!a.ln_beta || a.ln_n < 1 || a.ln_n > a.ld_in || (a.ln_residual && a.ln_n > a.ld_w))) return hipErrorInvalidValue;
  if (ng == 1) DENSE(1); else if (ng == 2) DENSE(2); else DENSE(4);
  if (psm_launch_probe) psm_launch_probe->tag = -1;
#undef DENSE
#undef DENSE2
  return hipGetLastError();
}

hipError_t psm_launch_dense_dots(const PsmDenseArgs& a, const PsmDotsArgs& d, hipStream_t st) {
  const int ng = a.Kp / 128;
  if (!a.Wp || a.Kp % 128 != 0 || (ng > 2 && ng % 4 != 0) || a.ld_in < 4 || a.bf16) return hipErrorInvalidValue;
  if (d.Kh < 4 || d.Kh % 4 != 0 || d.Kh > 1024 || d.Kh > a.ld_in || d.n_rows < 1) return hipErrorInvalidValue;
  const bool r16 = a.Mpad <= 128;                   // same tile choice as psm_launch_dense
  if (a.out_packed || (a.in_packed && (r16 || a.ld_in % 16 != 0 || a.Kp > a.ld_in))) return hipErrorInvalidValue;
  const int gx = a.ld_w / 16, gy = a.Mpad / (r16 ? 16 : 32);
  // z planes > 0: ceil(n_rows / 16) dots workgroups (8 waves x 2 rows), then ceil(guard waves / 8) guard workgroups
  const int extra = (d.n_src > 1 ? (d.n_rows > PSM_DOTS_WG_ROWS ? (d.n_rows + 1) / 2 : d.n_rows) : (d.n_rows + 15) / 16) + (d.guard.sdf ? d.guard.wg_count : 0);
  const dim3 grid(gx, gy, 1 + (extra + gx * gy - 1) / (gx * gy)), blk(512);
#define DD(N)                                                                                          \
  do {                                                                                                 \
    if (r16) PSM_LAUNCH((psm_dense_kernel<N, false, 16, true>), grid, blk, 0, st, a, d);       \
    else PSM_LAUNCH((psm_dense_kernel<N, false, 32, true>), grid, blk, 0, st, a, d);           \
  } while (0)
  if (psm_launch_probe) psm_launch_probe->tag = a.layer;
  if (ng == 1) DD(1); else if (ng == 2) DD(2); else DD(4);
  if (psm_launch_probe) psm_launch_probe->tag = -1;
#undef DD
  return hipGetLastError();
}

// LayerNormalization (+ residual) of the densePCA_attention stack, see psm_kernels.h.  Two-pass moments like
// tf.nn.moments (mean, then the mean of squared deviations; biased variance), float32.
// NPL > 0: the row (n <= 64 * NPL) is read ONCE into NPL registers per lane, every load issued up front, and both moments come
// from the registers (one memory round trip); NPL == 0: any n, three passes over a row that sits in L2.
template <int NPL>
__global__ __launch_bounds__(256) void psm_layernorm_kernel(PsmLayerNormArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = (int)blockIdx.x * 4 + wave;
  if (row >= a.rows) return;                          // wave-uniform
  float* x = a.act + (int64_t)row * a.ld_act;
  const float* r = a.res ? a.res + (int64_t)row * a.ld_res : nullptr;
  const float inv_n = 1.f / (float)a.n;
  if constexpr (NPL > 0) {
    float v[NPL], rv[NPL], g[NPL], b[NPL];
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
      const int k = min(lane + 64 * u, a.n - 1);
      v[u] = x[k]; rv[u] = r ? r[k] : 0.f; g[u] = a.gamma[k]; b[u] = a.beta[k];
    }
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NPL; ++u) { v[u] += rv[u]; s += (lane + 64 * u < a.n) ? v[u] : 0.f; }
    const float mean = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < NPL; ++u) { const float d = v[u] - mean; q += (lane + 64 * u < a.n) ? d * d : 0.f; }
    const float inv = rsqrtf(wave_sum(q) * inv_n + a.eps);
#pragma unroll
    for (int u = 0; u < NPL; ++u)
      if (lane + 64 * u < a.n) x[lane + 64 * u] = (v[u] - mean) * inv * g[u] + b[u];
    return;
  }
  float s = 0.f;
  for (int k = lane; k < a.n; k += 64) s += x[k] + (r ? r[k] : 0.f);
  const float mean = wave_sum(s) * inv_n;
  float q = 0.f;
  for (int k = lane; k < a.n; k += 64) { const float d = x[k] + (r ? r[k] : 0.f) - mean; q += d * d; }
  const float inv = rsqrtf(wave_sum(q) * inv_n + a.eps);
  for (int k = lane; k < a.n; k += 64) x[k] = (x[k] + (r ? r[k] : 0.f) - mean) * inv * a.gamma[k] + a.beta[k];
}

hipError_t psm_launch_layernorm(const PsmLayerNormArgs& a, hipStream_t st) {
  if (!a.act || !a.gamma || !a.beta || a.rows < 1 || a.n < 1 || a.n > a.ld_act || (a.res && a.n > a.ld_res)) return hipErrorInvalidValue;
  const dim3 grid((a.rows + 3) / 4), blk(256);
  if (a.n <= 512) PSM_LAUNCH(psm_layernorm_kernel<8>, grid, blk, 0, st, a);
  else if (a.n <= 1024) PSM_LAUNCH(psm_layernorm_kernel<16>, grid, blk, 0, st, a);
  else PSM_LAUNCH(psm_layernorm_kernel<0>, grid, blk, 0, st, a);
  return hipGetLastError();
}
// table dots from any activation [rows][ld_act] (one wave per table row; d.Kh <= ld_act): introspection under the closed
// form (the strip means the chain would have consumed)
__global__ __launch_bounds__(256) void psm_act_dots_kernel(PsmDotsArgs d, const float* act, int ld_act, int round_bf16, int packed) {
  const int lane = threadIdx.x & 63, row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int rc = min(row, d.n_rows - 1);
  const int blk = d.row_of[rc];
  float acc = 0.f;
  for (int k = lane; k < d.Kh; k += 64) {
    float x = packed ? act[psm_packed_offset(blk, k, ld_act >> 4)] : act[(int64_t)blk * ld_act + k];
    if (round_bf16) x = (float)(__bf16)x;
    acc += x * d.g2[(int64_t)rc * d.Kh + k];
  }
  const float tot = wave_sum(acc);
  if (lane == 0 && row < d.n_rows) d.out[row] = d.row_scale[blk] * (tot + d.c2[rc]) / d.cnt[rc];
}
hipError_t psm_launch_act_dots(const PsmDotsArgs& d, const float* act, int ld_act, int round_bf16, hipStream_t st, int packed) {
  if (d.n_rows < 1 || d.Kh < 1 || d.Kh > ld_act || (packed && ld_act % 16 != 0)) return hipErrorInvalidValue;
  PSM_LAUNCH(psm_act_dots_kernel, dim3((d.n_rows + 3) / 4), dim3(256), 0, st, d, act, ld_act, round_bf16, packed);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void psm_res_dots_kernel(PsmDotsArgs d, const float* res, int ld_res) {
  const int lane = threadIdx.x & 63, row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_dot_wgs = d.n_src > 1 ? d.n_rows : (d.n_rows + 3) / 4;
  if ((int)blockIdx.x >= n_dot_wgs) {                    // guard riders (PsmGuardArgs)
    psm_guard_wg<4>(d.guard, (int)blockIdx.x - n_dot_wgs, (int)(threadIdx.x >> 6), lane);
    return;
  }
  const int rc = min(row, d.n_rows - 1);
  if (d.n_src > 1) {                                     // closed form: one workgroup per row, wave w takes the source blocks w, w + 4, ...
    __shared__ float lsum[4];
    const int wave = threadIdx.x >> 6;
    const int rowl = (int)blockIdx.x, rl = min(rowl, d.n_rows - 1);
    const int cs = rl / d.rows_per_case;
    float acc = 0.f;
    for (int b0 = wave; b0 < d.n_src; b0 += 16) {
      float xv[4][2], gv[4][2], cc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int blk = min(b0 + 4 * t, d.n_src - 1);
        cc[t] = d.c2[(int64_t)rl * d.n_src + blk];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int k = min(lane + 64 * u, ld_res - 1);
          xv[t][u] = res[((int64_t)cs * d.n_src + blk) * ld_res + k];
          gv[t][u] = d.g2[((int64_t)rl * d.n_src + blk) * ld_res + k];
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const bool on = b0 + 4 * t < d.n_src;
#pragma unroll
        for (int u = 0; u < 2; ++u) acc += (on && lane + 64 * u < ld_res) ? (float)(__bf16)xv[t][u] * gv[t][u] : 0.f;
        acc += (on && lane == 0) ? cc[t] : 0.f;
      }
    }
    const float tot = wave_sum(acc);
    if (lane == 0) lsum[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0 && rowl < d.n_rows) d.out[rowl] = d.row_scale[cs * d.n_src] * ((lsum[0] + lsum[1]) + (lsum[2] + lsum[3]));
    return;
  }
  const int blk = d.row_of[rc];
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {                        // ld_res <= 128
    const int k = min(lane + 64 * u, ld_res - 1);
    const float x = (float)(__bf16)res[(int64_t)blk * ld_res + k];
    const float g = d.g2[(int64_t)rc * ld_res + k];
    acc += (lane + 64 * u < ld_res) ? x * g : 0.f;
  }
  const float tot = wave_sum(acc);
  if (lane == 0 && row < d.n_rows) d.out[row] = d.row_scale[blk] * (tot + d.c2[rc]) / d.cnt[rc];
}

hipError_t psm_launch_res_dots(const PsmDotsArgs& d, const float* res, int ld_res, hipStream_t st) {
  if (ld_res > 128 || ld_res < 1 || d.n_rows < 1) return hipErrorInvalidValue;
  const int nwg = (d.n_src > 1 ? d.n_rows : (d.n_rows + 3) / 4) + (d.guard.sdf ? d.guard.wg_count : 0);
  PSM_LAUNCH(psm_res_dots_kernel, dim3(nwg), dim3(256), 0, st, d, res, ld_res);
  return hipGetLastError();
}
