// psm_encode.hip -- encode stage of one surrogate solve, hand-written for gfx950 (CDNA4, wave64): kernels and their launchers.
//
//   encode  : split-K f32 MFMA GEMM  coeff = (blocks - mean) @ comp_in^T, the block
//             operand gathered straight from the grid image (blocks are never
//             materialised), centring fused into the LDS fill      [PM:303-349]
//
// Four forms of the same contraction (psm_launch_encode picks one): psm_encode_kernel (one slab per K slice, float32 MFMA),
// psm_encode_pair_kernel (two slices per workgroup), psm_encode_x6_kernel (bf16 pipe at float32 accuracy) and
// psm_encode_x6_mt_kernel (M-tiled, large case batches; its basis comes from psm_split_basis_kernel).  The slabs go to the
// reduce of psm_dense.hip.  MFMA operand maps and the x6 split: psm_mfma.h.
#include "psm_kernels.h"
#include "psm_devutil.h"
#include "psm_mfma.h"
#include "psm_stamps.h"

#include <cstdlib>

// ---------------------------------------------------------------------------
// SDF fold (PsmEncodeArgs::fold; bound geometry, SDF channel last): the contraction runs over the CH = C_IN - 1 leading channels
// only.  A row is still loaded as the 16-byte pieces of its C_IN interleaved channels (same addresses, same aligned loads); on
// the way into LDS the piece's elements of the leading channels are centred and written COMPACTED -- element e = 4 lane + j of
// the slice (pixel e / C_IN, channel e % C_IN) goes to float (e / C_IN) CH + e % C_IN of the row, LDS row stride 64 CH + 4 --
// and its SDF elements go to the row's four padding floats, which no MFMA operand read touches (no predicated store).
// ---------------------------------------------------------------------------
template <int C_IN, int CH>
__device__ __forceinline__ void psm_fold_slots(int lane, int (&dst)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = 4 * lane + j, pix = e / C_IN, ch = e - pix * C_IN;
    dst[j] = ch < CH ? pix * CH + ch : PSM_PIX_PER_SLICE * CH + j;
  }
}

// One row tile (<= 32 block rows), one slab per slice, SDF channel folded: the straight-line form of psm_encode_kernel's common
// case (rows requested before the basis slice, counted waits) over CH channels.
template <int C_IN, bool ALIGNED>
__device__ __forceinline__ void psm_encode_tile_fold(const PsmEncodeArgs& a, float* lds) {
  constexpr int CH = C_IN > 1 ? C_IN - 1 : 1;
  constexpr int KS = PSM_PIX_PER_SLICE * C_IN;  // K elements of a slice in the grid
  constexpr int KC = PSM_PIX_PER_SLICE * CH;    // ... contracted
  constexpr int G = KC / 8, LDA = KC + 4, Q = KS / 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x;
  const int runs = a.S / PSM_PIX_PER_SLICE;
  const int r = s / runs, c0 = (s - r * runs) * PSM_PIX_PER_SLICE;
  const int64_t src_off = (int64_t)r * a.row_stride + (int64_t)c0 * C_IN;
  const int NT = a.NT;
  const int i = lane & 31, h = lane >> 5;
  const int ql = lane < Q ? lane : Q - 1;
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + (int64_t)s * KS + 4 * ql);
  int dst[4];
  psm_fold_slots<C_IN, CH>(ql, dst);
  const int t = min(wave, NT - 1);
  int64_t rb[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) rb[u] = psm_row_base(a.row_base, min(wave + 4 * u, a.M - 1));   // wave-uniform: scalar loads
  float4 x[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float* src = a.grid + rb[u] + src_off + 4 * ql;
    if (ALIGNED) x[u] = *reinterpret_cast<const float4*>(src);
    else x[u] = make_float4(src[0], src[1], src[2], src[3]);
  }
  __builtin_amdgcn_sched_barrier(0);
  float4 b[G];
  {
    const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < 8; ++u) {                 // waits for the activation rows only (counted vmcnt)
    const int row = wave + 4 * u;
    const float keep = row < a.M ? 1.f : 0.f;   // padding rows -> 0 (no branch)
    if (lane < Q) {
      float* o = &lds[row * LDA];
      o[dst[0]] = (x[u].x - mu.x) * keep; o[dst[1]] = (x[u].y - mu.y) * keep;
      o[dst[2]] = (x[u].z - mu.z) * keep; o[dst[3]] = (x[u].w - mu.w) * keep;
    }
  }
  __syncthreads();
  f32x16 acc = {0};
  const float* arow = &lds[i * LDA + 4 * h];
  float4 av = *reinterpret_cast<const float4*>(arow);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float4 an = *reinterpret_cast<const float4*>(arow + 8 * (g + 1 < G ? g + 1 : g));   // next group in flight
    acc = MFMA32(av.x, b[g].x, acc);
    acc = MFMA32(av.y, b[g].y, acc);
    acc = MFMA32(av.z, b[g].z, acc);
    acc = MFMA32(av.w, b[g].w, acc);
    av = an;
  }
  if (wave < NT) {
    float* out = a.part + ((int64_t)s * a.Mpad) * a.ldp + t * 32 + i;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) out[(int64_t)acc_row(rg, h) * a.ldp] = acc[rg];
  }
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
template <int C_IN, bool ALIGNED>
__global__ __launch_bounds__(256) void psm_encode_kernel(PsmEncodeArgs a) {
  psm_warm_kernargs<sizeof(PsmEncodeArgs)>();
  constexpr int KS = PSM_PIX_PER_SLICE * C_IN;  // K elements per workgroup
  constexpr int G = KS / 8;                     // groups of 8 k
  constexpr int LDA = KS + 4;                   // LDS row stride (floats): 16-B slots rotate by one per row
  constexpr int Q = KS / 4;                     // 16-byte pieces per activation row (<= 64)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (C_IN > 1 && a.fold) { psm_encode_tile_fold<C_IN, ALIGNED>(a, lds); return; }   // uniform; the launcher sets it for one row tile, NT <= 4 only
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x;
  const int runs = a.S / PSM_PIX_PER_SLICE;
  const int r = s / runs, c0 = (s - r * runs) * PSM_PIX_PER_SLICE;
  const int64_t src_off = (int64_t)r * a.row_stride + (int64_t)c0 * C_IN;
  const int NT = a.NT;
  const int i = lane & 31, h = lane >> 5;
  const int ql = lane < Q ? lane : Q - 1;       // lanes >= Q idle in the staging (C_IN < 4)
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + (int64_t)s * KS + 4 * ql);

  // One activation row per wave and step: the row's origin is wave-uniform (scalar load),
  // the lanes read 16 contiguous bytes each.  All loads of a batch are issued before any use.
  auto load_rows = [&](float4 (&x)[8], int m0, int row0) {    // rows row0 + wave + 4u (u < 8) of chunk m0
    int64_t rb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) rb[u] = psm_row_base(a.row_base, min(m0 + row0 + wave + 4 * u, a.M - 1));   // wave-uniform: scalar loads
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* src = a.grid + rb[u] + src_off + 4 * ql;
      if (ALIGNED) x[u] = *reinterpret_cast<const float4*>(src);
      else x[u] = make_float4(src[0], src[1], src[2], src[3]);
    }
  };
  auto write_rows = [&](const float4 (&x)[8], int m0, int row0) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = row0 + wave + 4 * u;
      const float keep = (m0 + row) < a.M ? 1.f : 0.f;          // padding rows -> 0 (no branch)
      const float4 v = make_float4((x[u].x - mu.x) * keep, (x[u].y - mu.y) * keep, (x[u].z - mu.z) * keep, (x[u].w - mu.w) * keep);
      if (lane < Q) *reinterpret_cast<float4*>(&lds[row * LDA + 4 * lane]) = v;
    }
  };
  auto stage_rows = [&](int m0, int row0) {
    float4 x[8];
    load_rows(x, m0, row0);
    write_rows(x, m0, row0);
  };
  auto gemm_tile = [&](const float4 (&b)[G], int mt, int t, int m0, bool store) {
    f32x16 acc = {0};
    const float* arow = &lds[(mt * 32 + i) * LDA + 4 * h];
    float4 av = *reinterpret_cast<const float4*>(arow);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float4 an = *reinterpret_cast<const float4*>(arow + 8 * (g + 1 < G ? g + 1 : g));   // next group in flight
      acc = MFMA32(av.x, b[g].x, acc);
      acc = MFMA32(av.y, b[g].y, acc);
      acc = MFMA32(av.z, b[g].z, acc);
      acc = MFMA32(av.w, b[g].w, acc);
      av = an;
    }
    if (store) {
      float* out = a.part + ((int64_t)s * a.Mpad + m0 + mt * 32) * a.ldp + t * 32 + i;
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) out[(int64_t)acc_row(rg, h) * a.ldp] = acc[rg];
    }
  };

  if (NT <= 4 && a.Mpad > 32 && a.Mpad <= 32 * PSM_MT_CHUNK && a.whole) {
    // 33..128 block rows (a per-GPU shard of a case batch: 8 cases x 9 blocks = 72 rows): ALL rows and the weight slice
    // are requested in one go -- one memory round trip in front of the MFMAs instead of one per 64-row chunk --, staged
    // (rows beyond M as zeros, always 128 of them: no conditional stores), then the 2-4 row tiles run back to back with
    // the partial-sum stores of tile mt under the MFMAs of tile mt + 1.
    // The first row tile and the weight slice are requested first; the first tile's MFMAs start as soon as its rows and
    // the first weight group have landed (counted vmcnt) and run under the rest of the stream; the other tiles are
    // staged after them (their own LDS rows: no hazard with tile 0 being read).
    const int t = min(wave, NT - 1);
    PSM_STAMP(0, 0);
    float4 x[PSM_MT_CHUNK][8];
    load_rows(x[0], 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    float4 b[G];
    {
      const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
      for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    write_rows(x[0], 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    PSM_STAMP(0, 1);
    // the other row tiles are requested only now: asked for up front, together with everything else, they delayed the
    // first tile's rows (5.3 us to the first MFMA instead of ~3); they land under the first tile's 3 us of MFMAs
#pragma unroll
    for (int q = 1; q < PSM_MT_CHUNK; ++q) load_rows(x[q], 0, 32 * q);
    __builtin_amdgcn_sched_barrier(0);
    gemm_tile(b, 0, t, 0, wave < NT);
    PSM_STAMP(0, 3);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 1; q < PSM_MT_CHUNK; ++q) write_rows(x[q], 0, 32 * q);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    PSM_STAMP(0, 4);
    for (int mt = 1; mt < a.Mpad / 32; ++mt) gemm_tile(b, mt, t, 0, wave < NT);
    PSM_STAMP(0, 2);
    return;
  }

  if (NT <= 4 && a.Mpad > 32) {
    // many block rows (case batches): 64-row chunks double-buffered in LDS.  The rows of chunk c+1 are
    // requested before the MFMAs of chunk c and written to the other buffer after them, so the
    // staging round trip hides under the matrix work; the weight slice stays in registers throughout.
    // Barriers are LDS-only (the partial-sum stores need not drain between chunks).
    constexpr int CH = 64;
    // wave -> (component tile t, first row tile, row-tile step): with one or two component tiles (<= 64 components, e.g.
    // the reference's 45-component network) the waves split the two 32-row tiles of a chunk between them instead of
    // recomputing the last component tile (which halved the useful MFMA rate of this path)
    int t, mt_first, mt_step;
    bool store;
    if (NT == 2) { t = wave & 1; mt_first = wave >> 1; mt_step = 2; store = true; }
    else if (NT == 1) { t = 0; mt_first = wave & 1; mt_step = 2; store = wave < 2; }
    else { t = min(wave, NT - 1); mt_first = 0; mt_step = 1; store = wave < NT; }
    float4 xa[8], xb[8];
    load_rows(xa, 0, 0);
    load_rows(xb, 0, 32);
    __builtin_amdgcn_sched_barrier(0);
    float4 b[G];
    {
      const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
      for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    write_rows(xa, 0, 0);
    write_rows(xb, 0, 32);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    int buf = 0;
    for (int m0 = 0; m0 < a.Mpad; m0 += CH) {
      const bool more = m0 + CH < a.Mpad;
      if (more) { load_rows(xa, m0 + CH, 0); load_rows(xb, m0 + CH, 32); }
      const int tiles = min(2, (a.Mpad - m0) / 32);
      for (int mt = mt_first; mt < tiles; mt += mt_step) {
        f32x16 acc = {0};
        const float* arow = &lds[(buf * CH + mt * 32 + i) * LDA + 4 * h];
        float4 av = *reinterpret_cast<const float4*>(arow);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 an = *reinterpret_cast<const float4*>(arow + 8 * (g + 1 < G ? g + 1 : g));
          acc = MFMA32(av.x, b[g].x, acc);
          acc = MFMA32(av.y, b[g].y, acc);
          acc = MFMA32(av.z, b[g].z, acc);
          acc = MFMA32(av.w, b[g].w, acc);
          av = an;
        }
        if (store) {
          float* out = a.part + ((int64_t)s * a.Mpad + m0 + mt * 32) * a.ldp + t * 32 + i;
#pragma unroll
          for (int rg = 0; rg < 16; ++rg) out[(int64_t)acc_row(rg, h) * a.ldp] = acc[rg];
        }
      }
      if (more) {
        // rows of the next chunk into the other buffer (row index relative to that buffer)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = wave + 4 * u;
          const float k0 = (m0 + CH + row) < a.M ? 1.f : 0.f, k1 = (m0 + CH + 32 + row) < a.M ? 1.f : 0.f;
          const float4 v0 = make_float4((xa[u].x - mu.x) * k0, (xa[u].y - mu.y) * k0, (xa[u].z - mu.z) * k0, (xa[u].w - mu.w) * k0);
          const float4 v1 = make_float4((xb[u].x - mu.x) * k1, (xb[u].y - mu.y) * k1, (xb[u].z - mu.z) * k1, (xb[u].w - mu.w) * k1);
          if (lane < Q) {
            *reinterpret_cast<float4*>(&lds[((buf ^ 1) * CH + row) * LDA + 4 * lane]) = v0;
            *reinterpret_cast<float4*>(&lds[((buf ^ 1) * CH + 32 + row) * LDA + 4 * lane]) = v1;
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      buf ^= 1;
    }
    return;
  }

  if (NT <= 4 && a.Mpad <= 32 * PSM_MT_CHUNK) {
    // common case (<= 128 components, <= 128 block rows): straight-line so that the weight
    // stream stays in flight behind the first MFMAs (counted vmcnt).  Every wave computes (a
    // wave without a tile of its own recomputes the last one and stores nothing): keeps the
    // weight loads unconditional, ahead of the barrier.
    const int t = min(wave, NT - 1);
    PSM_STAMP(0, 0);
    float4 x0[8];
    load_rows(x0, 0, 0);                        // first 32 rows: loads issued BEFORE the weights
    __builtin_amdgcn_sched_barrier(0);
    float4 b[G];
    {
      const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
      for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
    }
    __builtin_amdgcn_sched_barrier(0);
    write_rows(x0, 0, 0);                       // waits for the activation rows only (counted vmcnt)
    for (int row0 = 32; row0 < a.Mpad; row0 += 32) stage_rows(0, row0);
    __syncthreads();
    PSM_STAMP(0, 1);
    gemm_tile(b, 0, t, 0, wave < NT);           // peeled: counted waits on the weight stream
    for (int mt = 1; mt < a.Mpad / 32; ++mt) gemm_tile(b, mt, t, 0, wave < NT);
    PSM_STAMP(0, 2);
    return;
  }

  // general case: any number of component tiles / row chunks
  float4 b[G];
  int cur_t = -1;
  for (int m0 = 0; m0 < a.Mpad; m0 += 32 * PSM_MT_CHUNK) {
    const int rows = min(32 * PSM_MT_CHUNK, a.Mpad - m0);
    for (int row0 = 0; row0 < rows; row0 += 32) stage_rows(m0, row0);
    __syncthreads();
    for (int t = wave; t < NT; t += 4) {
      if (t != cur_t) {
        const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
        for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
        cur_t = t;
      }
      for (int mt = 0; mt < rows / 32; ++mt) gemm_tile(b, mt, t, m0, true);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// encode of ONE row tile (a single case, <= 32 block rows) with four component tiles: a workgroup owns TWO consecutive K
// slices and one HALF of the components -- waves (slice 0 | 1) x (component tile 2 half + (0 | 1)) -- and adds the two
// slices' partial sums through LDS before it stores: n_slices / 2 slabs instead of n_slices.  Same basis bytes, same
// MFMAs per wave (one slice x one component tile, the whole basis slice in registers, counted waits) as the one-slice
// form above; what halves is the slab traffic (4.2 -> 2.1 MB written) and, above all, what the ONE workgroup per block row
// of psm_reduce_dense1_kernel has to pull in front of the first Dense layer (128 -> 64 KB: that launch's longest phase).
// ---------------------------------------------------------------------------
// The body is a template over the CONTRACTED channel count CH: C_IN (every channel), or C_IN - 1 with the SDF channel folded
// (PsmEncodeArgs::fold, see psm_fold_slots): fewer basis groups in registers, fewer MFMAs, a narrower LDS row; the row loads, the
// request order and the pair sum are the same.
template <int C_IN, int CH, bool ALIGNED>
__device__ __forceinline__ void psm_encode_pair_body(const PsmEncodeArgs& a, float* lds) {
  constexpr int KS = PSM_PIX_PER_SLICE * C_IN;  // K elements per slice in the grid
  constexpr int KC = PSM_PIX_PER_SLICE * CH;    // ... contracted
  constexpr int G = KC / 8;                     // groups of 8 k
  constexpr int LDA = KC + 4;                   // LDS row stride (floats): 16-B slots rotate by one per row
  constexpr int Q = KS / 4;                     // 16-byte pieces per activation row (<= 64)
  constexpr bool FOLD = CH != C_IN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sl = wave >> 1, j = wave & 1;       // this wave's slice of the pair; its row parity in the staging and its component tile of the half
  const int pair = (int)blockIdx.x >> 1, half = (int)blockIdx.x & 1;
  const int s = 2 * pair + sl, t = 2 * half + j;
  const int runs = a.S / PSM_PIX_PER_SLICE;
  const int r = s / runs, c0 = (s - r * runs) * PSM_PIX_PER_SLICE;
  const int64_t src_off = (int64_t)r * a.row_stride + (int64_t)c0 * C_IN;
  const int NT = a.NT;
  const int i = lane & 31, h = lane >> 5;
  const int ql = lane < Q ? lane : Q - 1;       // lanes >= Q idle in the staging (C_IN < 4)
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + (int64_t)s * KS + 4 * ql);
  int dst[4];
  if (FOLD) psm_fold_slots<C_IN, CH>(ql, dst);
  // Request order (round 6): the block-row offsets are a dependent table lookup in front of the activation rows.  They are
  // wave-uniform, so they come through the scalar cache (address space 4: s_load_dwordx2, its own counter) instead of sixteen
  // wave-wide vector loads, and the FIRST HALF of the basis stream is requested before anything waits for them: the lookup's round
  // trip hides behind it.  Then the rows, then the second half of the stream; the staging below waits for the rows (and, the counter
  // being in order, the first half of the stream, which was requested earlier anyway), the MFMAs of k group g for groups <= g.
  float4 b[G];
  const float4* bp = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
  int64_t rb[16];
  {
#pragma unroll
    for (int u = 0; u < 16; ++u) rb[u] = psm_row_base(a.row_base, min(j + 2 * u, a.M - 1));              // wave-uniform
  }
  __builtin_amdgcn_sched_barrier(0);             // (the scheduler sinks the scalar loads behind the stream's first half otherwise)
#pragma unroll
  for (int g = 0; g < G / 2; ++g) b[g] = stream_load(bp + g * 64);
  __builtin_amdgcn_sched_barrier(0);
  // staging: the two waves of a slice take its even / odd rows (16 each); every request before any use
  float4 x[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const float* src = a.grid + rb[u] + src_off + 4 * ql;
    if (ALIGNED) x[u] = *reinterpret_cast<const float4*>(src);
    else x[u] = make_float4(src[0], src[1], src[2], src[3]);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = G / 2; g < G; ++g) b[g] = stream_load(bp + g * 64);
  __builtin_amdgcn_sched_barrier(0);
  float* tile = lds + sl * 32 * LDA;
#pragma unroll
  for (int u = 0; u < 16; ++u) {                // waits for the activation rows only (counted vmcnt)
    const int row = j + 2 * u;
    const float keep = row < a.M ? 1.f : 0.f;   // padding rows -> 0 (no branch)
    const float4 v = make_float4((x[u].x - mu.x) * keep, (x[u].y - mu.y) * keep, (x[u].z - mu.z) * keep, (x[u].w - mu.w) * keep);
    if (FOLD) {
      float* o = &tile[row * LDA];
      if (lane < Q) { o[dst[0]] = v.x; o[dst[1]] = v.y; o[dst[2]] = v.z; o[dst[3]] = v.w; }
    } else if (lane < Q) *reinterpret_cast<float4*>(&tile[row * LDA + 4 * lane]) = v;
  }
  __syncthreads();
  f32x16 acc = {0};
  {
    const float* arow = &tile[i * LDA + 4 * h];
    float4 av = *reinterpret_cast<const float4*>(arow);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float4 an = *reinterpret_cast<const float4*>(arow + 8 * (g + 1 < G ? g + 1 : g));   // next group in flight
      acc = MFMA32(av.x, b[g].x, acc);
      acc = MFMA32(av.y, b[g].y, acc);
      acc = MFMA32(av.z, b[g].z, acc);
      acc = MFMA32(av.w, b[g].w, acc);
      av = an;
    }
  }
  // slice 1's partial sums meet slice 0's through LDS ([tile j][register][lane]: conflict-free both ways); fixed order s0 + s1
  float* red = lds + 2 * 32 * LDA + j * 16 * 64;
  if (sl == 1) {
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) red[rg * 64 + lane] = acc[rg];
  }
  __syncthreads();
  if (sl == 0) {
    float* out = a.part + ((int64_t)pair * a.Mpad) * a.ldp + t * 32 + i;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) out[(int64_t)acc_row(rg, h) * a.ldp] = acc[rg] + red[rg * 64 + lane];
  }
}

template <int C_IN, bool ALIGNED>
__global__ __launch_bounds__(256) void psm_encode_pair_kernel(PsmEncodeArgs a) {
  psm_warm_kernargs<sizeof(PsmEncodeArgs)>();
  extern __shared__ __attribute__((aligned(16))) float lds[];                  // [2 slices][32 rows][LDA], then [2 tiles][64 lanes][16]
  if (C_IN > 1 && a.fold) psm_encode_pair_body<C_IN, (C_IN > 1 ? C_IN - 1 : 1), ALIGNED>(a, lds);   // uniform
  else psm_encode_pair_body<C_IN, C_IN, ALIGNED>(a, lds);
}

// ---------------------------------------------------------------------------
// encode, "x6" arithmetic: the same contraction on the bf16 matrix pipe at float32 accuracy.
// Every float32 operand is split EXACTLY into three bf16 terms, x = hi + mid + lo (8 + 8 + 8 significant bits: the two
// remainders x - hi and (x - hi) - mid are exact in float32), and a product a * w is taken as the six terms whose
// weight is >= 2^-16 of it -- hh, hm, mh, hl, lh, mm -- by v_mfma_f32_32x32x16_bf16 (products of bf16 pairs are exact in
// float32; accumulation in float32).  The three dropped terms are <= 2^-23 of the product, the size of one float32
// rounding.  Six MFMAs of 32 cycles cover 16 k where the float32 instruction (v_mfma_f32_32x32x2_f32, 64 cycles) needs
// eight: 192 vs 512 cycles, and the matrix phase is the longest serial phase of this kernel for case batches.
// The basis stays float32 in memory (same packing, same bytes): a wave splits its slice in registers while the rest of
// the stream is in flight; the activation rows are split once, on their way into LDS (three bf16 planes).
// k order inside a 16-step: lane half h holds k = 16 s + 4 h + (0..3) and 16 s + 8 + 4 h + (0..3) in both operands.

template <int C_IN, bool ALIGNED>
__global__ __launch_bounds__(256) void psm_encode_x6_kernel(PsmEncodeArgs a) {
  psm_warm_kernargs<sizeof(PsmEncodeArgs)>();
  constexpr int KS = PSM_PIX_PER_SLICE * C_IN;  // K elements per workgroup
  constexpr int G = KS / 8;                     // float4 groups of the packed basis per lane
  constexpr int NS = KS / 16;                   // MFMA steps
  constexpr int LDB = KS + 4;                   // plane row stride in bf16: KS / 2 + 2 dwords = 2 * odd -> ds_read_b64 of 32 rows conflict-free
  constexpr int Q = KS / 4;
  extern __shared__ __attribute__((aligned(16))) __bf16 ldsx[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x;
  const int runs = a.S / PSM_PIX_PER_SLICE;
  const int r = s / runs, c0 = (s - r * runs) * PSM_PIX_PER_SLICE;
  const int64_t src_off = (int64_t)r * a.row_stride + (int64_t)c0 * C_IN;
  const int NT = a.NT;
  const int i = lane & 31, h = lane >> 5;
  const int ql = lane < Q ? lane : Q - 1;
  // rows per plane (as the launcher sized the LDS).  33 ... 128 block rows run as TWO workgroups per slice (gridDim.y == 2),
  // 64 rows each: half the LDS, so two workgroups share a CU and one's matrix phase covers the other's load latency
  const int R = a.Mpad <= 32 ? 32 : (gridDim.y == 2 ? 64 : 32 * PSM_MT_CHUNK);
  const int PL = R * LDB;                                    // plane stride
  const int mrow0 = gridDim.y == 2 ? 64 * (int)blockIdx.y : 0;   // first block row of this workgroup
  const float4 mu = *reinterpret_cast<const float4*>(a.mean + (int64_t)s * KS + 4 * ql);

  auto load_rows = [&](float4 (&x)[8], int m0, int row0) {
    int64_t rb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) rb[u] = psm_row_base(a.row_base, min(m0 + row0 + wave + 4 * u, a.M - 1));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* src = a.grid + rb[u] + src_off + 4 * ql;
      if (ALIGNED) x[u] = *reinterpret_cast<const float4*>(src);
      else x[u] = make_float4(src[0], src[1], src[2], src[3]);
    }
  };
  auto write_rows = [&](const float4 (&x)[8], int m0, int row0, int buf_row0) {   // rows row0 + wave + 4u of chunk m0 -> LDS rows buf_row0 + ...
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = wave + 4 * u;
      const float keep = (m0 + row0 + row) < a.M ? 1.f : 0.f;
      const f32x4 v = {(x[u].x - mu.x) * keep, (x[u].y - mu.y) * keep, (x[u].z - mu.z) * keep, (x[u].w - mu.w) * keep};
      bf16x4 vh, vm, vl;
      psm_split3(v, vh, vm, vl);
      if (lane < Q) {
        __bf16* dst = &ldsx[(buf_row0 + row) * LDB + 4 * lane];
        *reinterpret_cast<bf16x4*>(dst) = vh;
        *reinterpret_cast<bf16x4*>(dst + PL) = vm;
        *reinterpret_cast<bf16x4*>(dst + 2 * PL) = vl;
      }
    }
  };
  bf16x8 Bh[NS], Bm[NS], Bl[NS];
  // one 32-row tile against this wave's 32 components.  SPLIT: the basis registers b[] are split on the way (first tile:
  // each step waits only for the two groups it needs, the rest of the stream stays in flight)
  auto gemm_tile = [&](const float4 (&b)[G], bool split, int lds_row0, int out_row0, int t, bool store) {
    f32x16 acc = {0};
    const __bf16* arow = &ldsx[(lds_row0 + i) * LDB + 4 * h];
#pragma unroll
    for (int st = 0; st < NS; ++st) {
      if (split) {
        bf16x4 h0, m0, l0, h1, m1, l1;
        psm_split3((f32x4){b[2 * st].x, b[2 * st].y, b[2 * st].z, b[2 * st].w}, h0, m0, l0);
        psm_split3((f32x4){b[2 * st + 1].x, b[2 * st + 1].y, b[2 * st + 1].z, b[2 * st + 1].w}, h1, m1, l1);
        Bh[st] = psm_cat4(h0, h1); Bm[st] = psm_cat4(m0, m1); Bl[st] = psm_cat4(l0, l1);
      }
      const bf16x8 ah = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 16 * st + 8));
      const bf16x8 am = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + PL + 16 * st), *reinterpret_cast<const bf16x4*>(arow + PL + 16 * st + 8));
      const bf16x8 al = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 2 * PL + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 2 * PL + 16 * st + 8));
      acc = MFMA_BF16(am, Bm[st], acc);            // small terms first
      acc = MFMA_BF16(al, Bh[st], acc);
      acc = MFMA_BF16(ah, Bl[st], acc);
      acc = MFMA_BF16(am, Bh[st], acc);
      acc = MFMA_BF16(ah, Bm[st], acc);
      acc = MFMA_BF16(ah, Bh[st], acc);
    }
    if (store) {
      float* out = a.part + ((int64_t)s * a.Mpad + out_row0) * a.ldp + t * 32 + i;
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) out[(int64_t)acc_row(rg, h) * a.ldp] = acc[rg];
    }
  };
  auto load_basis = [&](float4 (&b)[G], int t) {
    const float4* p = a.bpack + (((int64_t)s * NT + t) * G) * 64 + lane;
#pragma unroll
    for (int g = 0; g < G; ++g) b[g] = stream_load(p + g * 64);
  };

  if (a.Mpad <= 32 * PSM_MT_CHUNK) {
    // up to 128 block rows: every row staged once; the first tile's rows and the basis slice are requested first, the
    // other tiles' rows land under the first tile's matrix work
    const int t = min(wave, NT - 1);
    const int tiles = min(a.Mpad - mrow0, R) / 32;           // row tiles of this workgroup (>= 1)
    float4 x0[8];
    load_rows(x0, mrow0, 0);
    __builtin_amdgcn_sched_barrier(0);
    float4 b[G];
    load_basis(b, t);
    __builtin_amdgcn_sched_barrier(0);
    write_rows(x0, mrow0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float4 x1[8], x2[8], x3[8];
    if (tiles > 1) load_rows(x1, mrow0, 32);
    if (tiles > 2) load_rows(x2, mrow0, 64);
    if (tiles > 3) load_rows(x3, mrow0, 96);
    __builtin_amdgcn_sched_barrier(0);
    gemm_tile(b, true, 0, mrow0, t, wave < NT);
    if (tiles > 1) {
      __builtin_amdgcn_sched_barrier(0);
      write_rows(x1, mrow0, 32, 32);
      if (tiles > 2) write_rows(x2, mrow0, 64, 64);
      if (tiles > 3) write_rows(x3, mrow0, 96, 96);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      for (int mt = 1; mt < tiles; ++mt) gemm_tile(b, false, mt * 32, mrow0 + mt * 32, t, wave < NT);
    }
    return;
  }

  // many block rows: 64-row chunks double-buffered in LDS (rows of chunk c + 1 requested before the matrix work of chunk
  // c, written to the other buffer after it); with one or two component tiles the waves split the chunk's two row tiles
  constexpr int CH = 64;
  int t, mt_first, mt_step;
  bool store;
  if (NT == 2) { t = wave & 1; mt_first = wave >> 1; mt_step = 2; store = true; }
  else if (NT == 1) { t = 0; mt_first = wave & 1; mt_step = 2; store = wave < 2; }
  else { t = min(wave, NT - 1); mt_first = 0; mt_step = 1; store = wave < NT; }
  float4 xa[8], xb[8];
  load_rows(xa, 0, 0);
  load_rows(xb, 0, 32);
  __builtin_amdgcn_sched_barrier(0);
  float4 b[G];
  load_basis(b, t);
  __builtin_amdgcn_sched_barrier(0);
  write_rows(xa, 0, 0, 0);
  write_rows(xb, 0, 32, 32);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  int buf = 0;
  bool first = true;
  for (int m0 = 0; m0 < a.Mpad; m0 += CH) {
    const bool more = m0 + CH < a.Mpad;
    if (more) { load_rows(xa, m0 + CH, 0); load_rows(xb, m0 + CH, 32); }
    const int tiles = min(2, (a.Mpad - m0) / 32);
    for (int mt = mt_first; mt < tiles; mt += mt_step) {
      if (first) gemm_tile(b, true, buf * CH + mt * 32, m0 + mt * 32, t, store);
      else gemm_tile(b, false, buf * CH + mt * 32, m0 + mt * 32, t, store);
      first = false;
    }
    if (more) {
      write_rows(xa, m0 + CH, 0, (buf ^ 1) * CH);
      write_rows(xb, m0 + CH, 32, (buf ^ 1) * CH + 32);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    buf ^= 1;
  }
}

// ---------------------------------------------------------------------------
// encode, x6 arithmetic, M-TILED, for large case batches (>= 32 cases per step; BASELINE configs[3] on one card runs 64).
// psm_encode_x6_kernel gives every K slice of 192 its own workgroup, whatever the row count: at 576 block rows that is 256 slabs
// of 576 x 128 floats = 75 MB written by the launch and read again by the reduce.  Here a workgroup owns a GROUP of consecutive K
// slices x 64 block rows (two MFMA row tiles) x all components and keeps its accumulators in registers across the group: one slab
// per K group (56 groups at 64 cases: 16.5 MB), the activations are read exactly once, the basis once per row group -- from the
// XCD's L2 for all but the first (XCD-aware workgroup mapping below).
//   wave w = component tile w (32 components), as in psm_encode_x6_kernel.  Its basis comes PRE-SPLIT (three bf16 planes in MFMA
//   fragment order, psm_split_basis_kernel, 1.5 x the bytes): half a slice (96 k) at a time in 72 registers, loads and MFMAs only --
//   splitting the float32 pack in the kernel cost 344 vector instructions per half-slice and the registers for the raw copy.  The
//   activation rows of a (half-slice, row tile) step go through LDS (three bf16 planes, 32 rows, one buffer per row tile: 38 KB,
//   two workgroups per CU).  Round 6 (stamps: tools/encode_stamps.py; record: profiles/r06_case_batch.txt (6)): the next step's rows are
//   split and written to the OTHER tile's buffer in the shadow of the step's MFMA chain (sched_group_barrier: one MFMA, six vector
//   instructions, in turn) -- behind the chain the same instructions cost ~1 us of every 2.1 us step; rows are requested two steps
//   ahead, a half-slice's basis planes as the previous half-slice's second tile releases them, step by step.
// Measured at 64 cases (one box): 49 us + 6 us reduce against 60 + 12 us for the one-slab-per-slice form.  Built and measured on
// the way, none faster (profiles/r05_case_batch.txt): three row tiles with the float32 basis split in the kernel (49-56 us), an
// eight-wave form with four multiplying and four staging waves per workgroup (57-64 us: the staging wave of a SIMD runs its ~260
// instructions per step at half speed beside the multiplying wave), three workgroups per CU at 168 registers (spills: 64-82 us).
// Summation order: k ascending inside a K group (MFMA accumulators), then the groups in slab order (psm_reduce_kernel) --
// deterministic, but not the order of the one-slab-per-slice form (float32 rounding differs in the last bits).
// ---------------------------------------------------------------------------
template <int C_IN, bool ALIGNED>
__global__ __launch_bounds__(256, 2) void psm_encode_x6_mt_kernel(PsmEncodeArgs a) {
  psm_warm_kernargs<sizeof(PsmEncodeArgs)>();
  ESTAMP(0);
  constexpr int KS = PSM_PIX_PER_SLICE * C_IN;  // K elements per slice
  constexpr int KH = KS / 2;                    // ... per half-slice
  constexpr int NSH = KH / 16;                  // MFMA steps per half-slice
  constexpr int LDB = KH + 8;                   // plane row stride in bf16: a multiple of 16 bytes, an odd number of 16-byte slots (13 at C_in = 3)
                                                // -- the 16 lanes of a ds_read_b128 group fall on 16 different slots.  Inside every 16 k the four
                                                // 4-element groups are stored 0, 2, 1, 3: lane half h's MFMA operand (k 4h.. and 8 + 4h.., the order
                                                // of the basis pack) is ONE 16-byte read (as two 8-byte reads the compiler emitted ds_read2_b64:
                                                // 16 LDS cycles for what ds_read_b128 moves in 4, MI355X_MICROARCH.md LDS table)
  constexpr int QH = KH / 4;                    // float4 per activation row and half-slice
  constexpr int NX = (32 * QH + 255) / 256;     // float4 per thread and step
  constexpr int MT = PSM_ENC_MT_ROWS / 32;
  constexpr int PL = 32 * LDB;                  // plane stride (bf16)
  constexpr int MAXG = 8;                       // slices per K group, at most
  static_assert(KH % 16 == 0 && MT == 2, "whole MFMA steps per half-slice; two named row tiles");
  __shared__ __attribute__((aligned(16))) __bf16 ldsx[2 * 3 * PL];
  __shared__ __attribute__((aligned(16))) float mean_l[MAXG * KS];       // the workgroup's K range of the mean
  __shared__ int hs_off[2 * MAXG + 2];                                    // float offset of half-slice hs within a block row (read two ahead)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_slices = a.S * a.S / PSM_PIX_PER_SLICE;
  // Workgroup -> (K group g, row group): the row groups of ONE K group read the same basis slices, so they get consecutive slots of
  // ONE XCD (workgroup i runs on XCD i % 8, tools/attic/xcc_probe.hip): id = ((g / 8) * row_groups + rg) * 8 + g % 8 -- the basis then comes
  // from memory once per K group and from that XCD's L2 for the other row groups.  Placement is a speed matter only.  Ids whose K
  // group does not exist (the last, partial block of eight) leave at once.
  const int n_groups = a.kgroup, row_groups = (a.Mpad + PSM_ENC_MT_ROWS - 1) / PSM_ENC_MT_ROWS;
  const int slot = blockIdx.x >> 3, g_blk = slot / row_groups, rg = slot - g_blk * row_groups;
  const int grp = g_blk * 8 + (blockIdx.x & 7);
  if (grp >= n_groups) return;
  const int s_first = (int)(((long long)grp * n_slices) / n_groups);
  const int s_end = (int)(((long long)(grp + 1) * n_slices) / n_groups);
  const int n_hs = 2 * (s_end - s_first);                    // half-slices of this workgroup (2 .. 2 MAXG)
  const int m0 = rg * PSM_ENC_MT_ROWS;
  const int runs = a.S / PSM_PIX_PER_SLICE;
  for (int k = tid; k < (s_end - s_first) * KS; k += 256) mean_l[k] = a.mean[(int64_t)s_first * KS + k];
  if (tid < n_hs) {
    const int s = s_first + (tid >> 1), r = s / runs, c0 = (s - r * runs) * PSM_PIX_PER_SLICE;
    hs_off[tid] = (int)((int64_t)r * a.row_stride + (int64_t)c0 * C_IN + (tid & 1) * KH);
  }
  const int NT = a.NT;
  const int t = min(wave, NT - 1);
  const int i = lane & 31, h = lane >> 5;
  // staging: 256 threads move one step's 32 rows x KH floats, float4 idx = tid + 256 u -> (row, q), fixed over the steps.  Everything a
  // request needs is ONE 32-bit float offset per (row tile, piece) -- row base (a case batch of grids is < 2^31 floats) + column --
  // plus the half-slice's scalar offset from LDS; padding rows are one bit each
  static_assert(32 * QH == 256 * NX, "every thread moves exactly NX pieces of a step");
  int ldst[NX], mq[NX];
  unsigned o0[NX], o1[NX];                                                 // BYTE offsets (the launcher keeps a case batch of grids under 4 GiB)
  unsigned keep_bits = 0;
#pragma unroll
  for (int u = 0; u < NX; ++u) {
    const int idx = tid + 256 * u;
    const int xrow = idx / QH, xq = idx - xrow * QH;
    const int m = m0 + xrow;
    o0[u] = 4u * (unsigned)((int)a.row_base[min(m, a.M - 1)] + 4 * xq);
    o1[u] = 4u * (unsigned)((int)a.row_base[min(m + 32, a.M - 1)] + 4 * xq);
    ldst[u] = xrow * LDB + psm_x6_group_pos(xq);             // bf16 offset within a plane
    mq[u] = 4 * xq;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) keep_bits |= (m + 32 * mt) < a.M ? (1u << (mt * NX + u)) : 0u;
  }
  // one register set per row tile: a tile's rows are requested TWO steps ahead of their split (stamps, tools/encode_stamps.py: with one
  // step of lead the staging phase waited ~0.6 us per step for rows that come from HBM / MALL exactly once)
  float4 xr0[NX], xr1[NX];
  auto load_x = [&](int off, auto mt_tag) {                               // off = hs_off[hs] as a wave-uniform value: scalar base + 32-bit lane offset
    constexpr int MTI = decltype(mt_tag)::value;
    const char* base = reinterpret_cast<const char*>(a.grid + off);
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      const float* src = reinterpret_cast<const float*>(base + (MTI == 0 ? o0[u] : o1[u]));
      float4& dst = MTI == 0 ? xr0[u] : xr1[u];
      if (ALIGNED) dst = *reinterpret_cast<const float4*>(src);
      else dst = make_float4(src[0], src[1], src[2], src[3]);
    }
  };
  float4 mu_r[NX];                                                         // the step's mean pieces, read at the top of its matrix phase
  auto read_mean = [&](int hs) {
#pragma unroll
    for (int u = 0; u < NX; ++u) mu_r[u] = *reinterpret_cast<const float4*>(&mean_l[hs * KH + mq[u]]);
  };
  auto write_piece = [&](auto mt_tag, int buf, int u) {
    constexpr int MTI = decltype(mt_tag)::value;
    const uint32_t k = ((keep_bits >> (MTI * NX + u)) & 1u) ? 0xffffffffu : 0u;   // padding rows: zeros (a bit mask: as a float factor the
    const float4 mu = mu_r[u];                                                     // compiler packed the multiplies -- v_pk_mul_f32 is slow beside MFMAs)
    const float4 x = MTI == 0 ? xr0[u] : xr1[u];
    const f32x4 v = {__uint_as_float(__float_as_uint(x.x - mu.x) & k), __uint_as_float(__float_as_uint(x.y - mu.y) & k),
                     __uint_as_float(__float_as_uint(x.z - mu.z) & k), __uint_as_float(__float_as_uint(x.w - mu.w) & k)};
    bf16x4 vh, vm, vl;
    psm_split3(v, vh, vm, vl);
    __bf16* dst = &ldsx[buf * 3 * PL + ldst[u]];
    *reinterpret_cast<bf16x4*>(dst) = vh;
    *reinterpret_cast<bf16x4*>(dst + PL) = vm;
    *reinterpret_cast<bf16x4*>(dst + 2 * PL) = vl;
  };
  auto write_x = [&](int hs, auto mt_tag, int buf) {
    read_mean(hs);
#pragma unroll
    for (int u = 0; u < NX; ++u) write_piece(mt_tag, buf, u);
  };
  // basis planes of a half-slice: [step][plane h, m, l] fragments as they lie in a.bpack_x6 (psm_split_basis_kernel): loads and
  // MFMAs only.  ONE register set (72), refilled step by step (mfma_tile's `next`)
  bf16x8 P[NSH][3];
  auto b_ptr = [&](int hs) { return a.bpack_x6 + ((((int64_t)(s_first + (hs >> 1)) * NT + t) * (2 * NSH) + (hs & 1) * NSH) * 3) * 64 + lane; };
  auto load_b = [&](int hs) {
    const uint4* p = b_ptr(hs);
#pragma unroll
    for (int st = 0; st < NSH; ++st)
#pragma unroll
      for (int q = 0; q < 3; ++q) P[st][q] = __builtin_bit_cast(bf16x8, p[(st * 3 + q) * 64]);
  };
  f32x16 acc0 = {0}, acc1 = {0};
  // `next` != nullptr: the planes of step st are dead after its six MFMAs in a half-slice's SECOND row tile -- the next half-slice's
  // planes of that step are requested right there (a whole matrix phase + staging ahead of their first use instead of behind the
  // last MFMA of the phase)
  // `stage(u)`: piece u of the NEXT step's rows (split + LDS writes into the other tile's buffer, which nobody reads during this step) rides
  // in the shadow of MFMA groups 2u, 2u + 1: one MFMA, then a few of its vector instructions, in turn (the MFMAs are one dependent chain of
  // 32 cycles each; behind the phase the same instructions cost ~1 us per step, tools/encode_stamps.py)
  auto mfma_tile = [&](f32x16& c, int buf, const uint4* next, int stamp, int hs_stage, auto&& stage) {
    const __bf16* arow = &ldsx[buf * 3 * PL + i * LDB + 8 * h];
    if (hs_stage >= 0) read_mean(hs_stage);
    bf16x8 A[2][3];
    auto rd = [&](int st, int sl) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        A[sl][pl] = *reinterpret_cast<const bf16x8*>(arow + pl * PL + 16 * st);
    };
    rd(0, 0);
#pragma unroll
    for (int st = 0; st < NSH; ++st) {
      const int sl = st & 1;
      if (st + 1 < NSH) rd(st + 1, sl ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      if ((st & 1) == 0) stage(st >> 1);
      c = MFMA_BF16(A[sl][1], P[st][1], c);            // small terms first: mm, lh, hl, mh, hm, hh
      c = MFMA_BF16(A[sl][2], P[st][0], c);
      c = MFMA_BF16(A[sl][0], P[st][2], c);
      c = MFMA_BF16(A[sl][1], P[st][0], c);
      c = MFMA_BF16(A[sl][0], P[st][1], c);
      c = MFMA_BF16(A[sl][0], P[st][0], c);
#pragma unroll
      for (int k6 = 0; k6 < 6; ++k6) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
      }
      if (st == 0) ESTAMP(stamp);
      if (next) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 3; ++q) P[st][q] = __builtin_bit_cast(bf16x8, next[(st * 3 + q) * 64]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  typedef std::integral_constant<int, 0> T0; typedef std::integral_constant<int, 1> T1;
  __syncthreads();                                            // mean_l, hs_off
  load_x(__builtin_amdgcn_readfirstlane(hs_off[0]), T0{});
  load_b(0);
  load_x(__builtin_amdgcn_readfirstlane(hs_off[0]), T1{});
  int off_next = __builtin_amdgcn_readfirstlane(hs_off[1]);    // hs_off[hs + 1] at the top of run_hs(hs); the one after is read a half-slice ahead
  __builtin_amdgcn_sched_barrier(0);
  write_x(0, T0{}, 0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  ESTAMP(1);
  // steps (half-slice hs, row tile): buffer = tile (two steps per half-slice).  The rows a step splits and writes beside its MFMAs (those
  // of the NEXT step) were requested before the PREVIOUS step's MFMAs; what it requests itself is for the step after next.  (The last
  // half-slice is a second compile-time copy: behind a run-time "is there a next one" the plane registers became a conditional
  // assignment and spilled.)
  auto run_hs = [&](int hs, auto more_tag) {
    constexpr bool more = decltype(more_tag)::value;
    if (more) load_x(off_next, T0{});
    const int off_raw = hs_off[hs + 2];
    __builtin_amdgcn_sched_barrier(0);
    mfma_tile(acc0, 0, nullptr, 2 + 6 * hs, hs, [&](int u) { write_piece(T1{}, 1, u); });
    ESTAMP(3 + 6 * hs);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ESTAMP(4 + 6 * hs);
    if (more) load_x(off_next, T1{});
    __builtin_amdgcn_sched_barrier(0);
    if (more) mfma_tile(acc1, 1, b_ptr(hs + 1), 5 + 6 * hs, hs + 1, [&](int u) { write_piece(T0{}, 0, u); });
    else mfma_tile(acc1, 1, nullptr, 5 + 6 * hs, -1, [](int) {});
    off_next = __builtin_amdgcn_readfirstlane(off_raw);
    ESTAMP(6 + 6 * hs);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ESTAMP(7 + 6 * hs);
  };
  for (int hs = 0; hs + 1 < n_hs; ++hs) run_hs(hs, std::true_type{});
  run_hs(n_hs - 1, std::false_type{});
  if (wave < NT) {
    float* out = a.part + ((int64_t)grp * a.Mpad + m0) * a.ldp + t * 32 + i;
#pragma unroll
    for (int q = 0; q < 16; ++q) out[(int64_t)acc_row(q, h) * a.ldp] = acc0[q];
    if (m0 + 32 < a.Mpad) {
#pragma unroll
      for (int q = 0; q < 16; ++q) out[(int64_t)(32 + acc_row(q, h)) * a.ldp] = acc1[q];
    }
  }
  ESTAMP(63);
}

// x6 covers <= 128 components (NT <= 4) and an LDS footprint of three bf16 planes
static bool psm_encode_x6_fits(const PsmEncodeArgs& a, int row_wgs, size_t* lds) {
  const int rows = a.Mpad <= 32 ? 32 : (row_wgs == 2 ? 64 : 32 * PSM_MT_CHUNK);
  *lds = (size_t)3 * rows * (PSM_PIX_PER_SLICE * a.c_in + 4) * 2;
  return a.NT <= 4 && *lds <= 156 * 1024 && a.Mpad % 32 == 0;
}

// the two-slices-per-workgroup form (psm_encode_pair_kernel): one row tile, exactly four component tiles, float32 MFMA, an even
// number of slices; a predicate of the arguments alone (pairs_ok carries the route's say).  The slab count the reduce launches must use: n_slices / 2 when psm_encode_pairs(args) (launch_all, psm_api_solve.cpp).
bool psm_encode_pairs(const PsmEncodeArgs& a) {
  const int n_slices = a.S * a.S / PSM_PIX_PER_SLICE;
  return a.pairs_ok && !a.x6 && a.kgroup <= 1 && a.Mpad == 32 && a.NT == 4 && n_slices % 2 == 0;
}
hipError_t psm_launch_encode(const PsmEncodeArgs& a, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop, int row_wgs) {
  const int n_slices = a.S * a.S / PSM_PIX_PER_SLICE;
  const int rows = a.Mpad <= 32 ? 32 : 32 * PSM_MT_CHUNK;        // one tile, or 2 x 64-row buffers / a 128-row chunk
  size_t lds = (size_t)rows * (PSM_PIX_PER_SLICE * a.c_in + 4) * sizeof(float);
  size_t lds_x6 = 0;
  // two workgroups per slice (the route's choice): only where the kernel has the 64-row form, more than two and at most four row tiles
  if (row_wgs != 1 && !(row_wgs == 2 && a.Mpad > 64 && a.Mpad <= 32 * PSM_MT_CHUNK)) return hipErrorInvalidValue;
  // SDF fold: only the float32 forms of one row tile have the arm (choose_route, psm_api_solve.cpp, asks for nothing else)
  if (a.fold && (a.x6 || a.kgroup > 1 || a.Mpad != 32 || a.NT > 4 || a.c_in < 2)) return hipErrorInvalidValue;
  if (a.x6 && a.kgroup > 1) {
    // kgroup = number of K GROUPS here (the slab count); a group holds n_slices / kgroup slices, rounded either way, at most 8
    if (a.NT > 4 || a.Mpad % 32 != 0 || a.kgroup > n_slices || (n_slices + a.kgroup - 1) / a.kgroup > 8 || !a.bpack_x6) return hipErrorInvalidValue;
    const int row_groups = (a.Mpad + PSM_ENC_MT_ROWS - 1) / PSM_ENC_MT_ROWS;
    const dim3 grid((unsigned)(((a.kgroup + 7) / 8) * row_groups * 8));      // XCD-aware 1-D mapping, see the kernel
    PSM_LAUNCH_ENCODE_FAMILY(psm_encode_x6_mt_kernel, grid, 0, st, ev_start, ev_stop, a);
    return hipGetLastError();
  }
  if (a.x6 && psm_encode_x6_fits(a, row_wgs, &lds_x6)) {
    lds = lds_x6;
    PSM_LAUNCH_ENCODE_FAMILY(psm_encode_x6_kernel, dim3(n_slices, row_wgs), lds, st, ev_start, ev_stop, a);
    return hipGetLastError();
  }
  if (psm_encode_pairs(a)) {                       // one row tile, four component tiles: two slices per workgroup, n_slices / 2 slabs
    const size_t lds_p = ((size_t)2 * 32 * (PSM_PIX_PER_SLICE * a.c_in + 4) + 2 * 16 * 64) * sizeof(float);
    PSM_LAUNCH_ENCODE_FAMILY(psm_encode_pair_kernel, dim3(n_slices), lds_p, st, ev_start, ev_stop, a);
    return hipGetLastError();
  }
  PSM_LAUNCH_ENCODE_FAMILY(psm_encode_kernel, dim3(n_slices), lds, st, ev_start, ev_stop, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// basis of the large-batch encode: the float32 pack (pack_comp_in: [slice][ntile][KS/8 groups][64 lanes] float4) split exactly into
// three bf16 planes in the fragment order of the MFMA's second operand: [slice][ntile][KS/16 steps][plane h, m, l][64 lanes] x 8 bf16
// (step st = groups 2 st and 2 st + 1 of the same lane).  Once per handle (psm_api_solve.cpp, ensure_encode_aux).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psm_split_basis_kernel(const float4* bpack, uint4* out, long long n_frag, int NS) {
  const long long f = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // fragment = (slice, ntile, step)
  const int lane = threadIdx.x & 63;
  if (f >= n_frag) return;
  const long long tile = f / NS; const int st = (int)(f - tile * NS);
  const float4 g0 = bpack[(tile * (2 * NS) + 2 * st) * 64 + lane], g1 = bpack[(tile * (2 * NS) + 2 * st + 1) * 64 + lane];
  bf16x4 h0, m0, l0, h1, m1, l1;
  psm_split3((f32x4){g0.x, g0.y, g0.z, g0.w}, h0, m0, l0);
  psm_split3((f32x4){g1.x, g1.y, g1.z, g1.w}, h1, m1, l1);
  out[(f * 3 + 0) * 64 + lane] = __builtin_bit_cast(uint4, psm_cat4(h0, h1));
  out[(f * 3 + 1) * 64 + lane] = __builtin_bit_cast(uint4, psm_cat4(m0, m1));
  out[(f * 3 + 2) * 64 + lane] = __builtin_bit_cast(uint4, psm_cat4(l0, l1));
}
hipError_t psm_launch_split_basis(const float4* bpack, uint4* out, int n_slices, int NT, int KS, hipStream_t st) {
  if (KS % 16 != 0) return hipErrorInvalidValue;
  const long long n_frag = (long long)n_slices * NT * (KS / 16);
  PSM_LAUNCH(psm_split_basis_kernel, dim3((unsigned)((n_frag + 3) / 4)), dim3(256), 0, st, bpack, out, n_frag, KS / 16);
  return hipGetLastError();
}
