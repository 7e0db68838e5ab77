// psm_decode.hip -- decode stage of the general solve path, hand-written for gfx950 (CDNA4, wave64): kernels and launcher.
//
//   decode  : f32 MFMA GEMM  blocks = res @ comp_out + mean, out_scale fused [PM:365-366, SMD:541-551]
//
// psm_decode128_kernel (<= 128 output components) and psm_decode_kernel (any count).  The geometry-bound path decodes and pastes
// in one kernel (psm_bound.hip); the bf16-operand decode is in psm_bf16.hip.  MFMA operand maps: psm_mfma.h.
#include "psm_kernels.h"
#include "psm_devutil.h"
#include "psm_mfma.h"
#include "psm_stamps.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
// Fast path: <= 128 output components (ld_res == 128, 16 groups of 8 k): the whole weight
// slice of a wave (16 x 16 B per lane) is issued behind the activation-tile loads and stays in
// flight under the first MFMAs (counted vmcnt).
template <int MTC>
__global__ __launch_bounds__(256) void psm_decode128_kernel(PsmDecodeArgs a, int m_first, int m_end) {
  constexpr int LDR = 128, LDA = LDR + 4, Q = LDR / 4, GD = LDR / 8, NA = MTC * 32 * Q / 256;
  m_first += (int)blockIdx.y * MTC * 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int ct = min(blockIdx.x * 4 + wave, a.n_coltiles - 1);
  const bool live = (blockIdx.x * 4 + wave) < a.n_coltiles;
  auto load_tile = [&](f32x4 (&x)[NA], int m_base) {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = tid + 256 * u, row = idx / Q, q = idx - row * Q;
      const int m = min(m_base + row, a.Mpad - 1);
      x[u] = *reinterpret_cast<const f32x4*>(a.res + (int64_t)m * LDR + 4 * q);
    }
  };
  auto write_tile = [&](const f32x4 (&x)[NA]) {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = tid + 256 * u, row = idx / Q, q = idx - row * Q;
      *reinterpret_cast<f32x4*>(&lds[row * LDA + 4 * q]) = x[u];
    }
  };
  PSM_STAMP(0, 20);
  f32x4 x[NA];
  load_tile(x, m_first);
  float rs = a.row_scale[min(m_first + min(tid, MTC * 32 - 1), a.Mpad - 1)];
  __builtin_amdgcn_sched_barrier(0);
  float4 b[GD];                                  // this wave's weight slice: loaded once, kept for every row chunk
  const float4* bp = a.bpack + ((int64_t)ct * GD) * 64 + lane;
#pragma unroll
  for (int g = 0; g < GD; ++g) b[g] = stream_load(bp + g * 64);
  const int col = ct * 32 + i;
  const float mu_raw = a.mean[col];
  __builtin_amdgcn_sched_barrier(0);
  const float mu = psm_settled(mu_raw);
  float* lrs = lds + MTC * 32 * LDA;             // [MTC*32] out_scale per block row
  const int m_step = MTC * 32 * (int)gridDim.y;    // row chunks are dealt round-robin to the gridDim.y row groups
  for (int m_base = m_first; m_base < m_end; m_base += m_step) {
    if (m_base != m_first) {                     // later chunks (many block rows): only the activation tile is new
      __syncthreads();                           // every wave is done with the previous tile
      load_tile(x, m_base);
      rs = a.row_scale[min(m_base + min(tid, MTC * 32 - 1), a.Mpad - 1)];
    }
    write_tile(x);
    if (tid < MTC * 32) lrs[tid] = rs;
    __syncthreads();
    PSM_STAMP(0, 21);
    f32x16 acc[MTC];
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt) {
      acc[mt] = (f32x16){0};
      const float* arow = &lds[(mt * 32 + i) * LDA + 4 * h];
      float4 av = *reinterpret_cast<const float4*>(arow);
#pragma unroll
      for (int g = 0; g < GD; ++g) {
        const float4 an = *reinterpret_cast<const float4*>(arow + 8 * (g + 1 < GD ? g + 1 : g));
        acc[mt] = MFMA32(av.x, b[g].x, acc[mt]);
        acc[mt] = MFMA32(av.y, b[g].y, acc[mt]);
        acc[mt] = MFMA32(av.z, b[g].z, acc[mt]);
        acc[mt] = MFMA32(av.w, b[g].w, acc[mt]);
        av = an;
      }
    }
    PSM_STAMP(0, 22);
    if (live) {
#pragma unroll
      for (int mt = 0; mt < MTC; ++mt) {
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const int rr = mt * 32 + acc_row(rg, h);
          const int m = m_base + rr;
          if (m < a.M) a.pred[(int64_t)m * a.K_out + col] = (acc[mt][rg] + mu) * lrs[rr];
        }
      }
    }
  }
  PSM_STAMP(0, 23);
}

template <int MTC, int GCH>   // GCH: groups of 8 k whose weights are prefetched together
__global__ __launch_bounds__(256) void psm_decode_kernel(PsmDecodeArgs a, int m_base) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int LDA = a.ld_res + 4, Q = a.ld_res / 4;
  const int ct = min(blockIdx.x * 4 + wave, a.n_coltiles - 1);
  const bool live = (blockIdx.x * 4 + wave) < a.n_coltiles;
  const float4* bp = a.bpack + ((int64_t)ct * a.Gd) * 64 + lane;
  // activation tile first (needed first), then the weight stream
  for (int idx = tid; idx < MTC * 32 * Q; idx += 256) {
    const int row = idx / Q, q = idx - row * Q;
    const int m = m_base + row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m < a.Mpad) v = *reinterpret_cast<const float4*>(a.res + (int64_t)m * a.ld_res + 4 * q);
    *reinterpret_cast<float4*>(&lds[row * LDA + 4 * q]) = v;
  }
  float4 b[GCH];
#pragma unroll
  for (int g = 0; g < GCH; ++g) b[g] = bp[(int64_t)min(g, a.Gd - 1) * 64];
  const int col = ct * 32 + i;
  const float mu = a.mean[col];
  __syncthreads();
  f32x16 acc[MTC];
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) acc[mt] = (f32x16){0};
  for (int g0 = 0; g0 < a.Gd; g0 += GCH) {   // Gd is a multiple of 4; GCH in {4, 16}
    if (g0 > 0) {
#pragma unroll
      for (int g = 0; g < GCH; ++g) b[g] = bp[(int64_t)min(g0 + g, a.Gd - 1) * 64];
    }
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt) {
      const float* arow = &lds[(mt * 32 + i) * LDA + 4 * h + 8 * g0];
#pragma unroll
      for (int g = 0; g < GCH; ++g) {
        if (g0 + g < a.Gd) {
          const float4 av = *reinterpret_cast<const float4*>(arow + 8 * g);
          acc[mt] = MFMA32(av.x, b[g].x, acc[mt]);
          acc[mt] = MFMA32(av.y, b[g].y, acc[mt]);
          acc[mt] = MFMA32(av.z, b[g].z, acc[mt]);
          acc[mt] = MFMA32(av.w, b[g].w, acc[mt]);
        }
      }
    }
  }
  if (!live) return;
  const float mu_r = psm_settled(mu);
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) {
    float rsv[16];                                   // the tile's row scales first, straight-line (see psm_settled)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) rsv[rg] = a.row_scale[min(m_base + mt * 32 + acc_row(rg, h), a.M - 1)];
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) rsv[rg] = psm_settled(rsv[rg]);
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int m = m_base + mt * 32 + acc_row(rg, h);
      if (m < a.M) a.pred[(int64_t)m * a.K_out + col] = (acc[mt][rg] + mu_r) * rsv[rg];
    }
  }
}

hipError_t psm_launch_decode(const PsmDecodeArgs& a, hipStream_t st) {
  const int nwg = (a.n_coltiles + 3) / 4;
  if (a.ld_res == 128) {
    // <= 128 components: ONE launch for any number of block rows; a workgroup keeps its weight slice in
    // registers and walks the rows in chunks of MTC*32 (chunk size chosen to waste the fewest padded tiles)
    // one output channel gives only 128 column workgroups: the row tiles are then spread over up to 512 / nwg row groups,
    // one chunk each where possible, so that all 256 CUs work (each group re-reads the weight slice: 8 MB more traffic
    // per group; same rule as psm_launch_decode_paste_batch, where it was measured)
    const int tiles = a.Mpad / 32;
    int mtc, groups;
    if (nwg >= 256) {
      const int iters = (tiles + 3) / 4;
      mtc = (tiles + iters - 1) / iters; groups = 1;
    } else {
      const int cap = std::max(1, 512 / nwg);
      mtc = std::min(4, std::max(1, (tiles + cap - 1) / cap));
      groups = std::min((tiles + mtc - 1) / mtc, cap);
    }
    const size_t lds128 = (size_t)mtc * 32 * (a.ld_res + 4) * sizeof(float) + (size_t)mtc * 32 * sizeof(float);
    const dim3 grid(nwg, groups);
    if (mtc == 4) PSM_LAUNCH((psm_decode128_kernel<4>), grid, dim3(256), lds128, st, a, 0, a.Mpad);
    else if (mtc == 3) PSM_LAUNCH((psm_decode128_kernel<3>), grid, dim3(256), lds128, st, a, 0, a.Mpad);
    else if (mtc == 2) PSM_LAUNCH((psm_decode128_kernel<2>), grid, dim3(256), lds128, st, a, 0, a.Mpad);
    else PSM_LAUNCH((psm_decode128_kernel<1>), grid, dim3(256), lds128, st, a, 0, a.Mpad);
    return hipGetLastError();
  }
  int m_base = 0;
  while (m_base < a.Mpad) {
    const int tiles = (a.Mpad - m_base) / 32;
    const int mtc = tiles >= 4 ? 4 : (tiles >= 2 ? 2 : 1);
    const size_t lds = (size_t)mtc * 32 * (a.ld_res + 4) * sizeof(float);
    const bool g16 = (a.Gd % 16 == 0);
#define DEC(M_, G_) PSM_LAUNCH((psm_decode_kernel<M_, G_>), dim3(nwg), dim3(256), lds, st, a, m_base)
    if (mtc == 4) { if (g16) DEC(4, 16); else DEC(4, 4); }
    else if (mtc == 2) { if (g16) DEC(2, 16); else DEC(2, 4); }
    else { if (g16) DEC(1, 16); else DEC(1, 4); }
#undef DEC
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    m_base += mtc * 32;
  }
  return hipSuccess;
}
