// psm_bound.hip -- geometry-bound fast path of one surrogate solve (psm_bind_geometry), hand-written for gfx950 (CDNA4,
// wave64): kernels and launchers.  Bind time: psm_bind_rows / _fold / _own / _copy_kernel and psm_pair_fold_kernel build the
// tables that fold strips and shift through the basis (and the head layer).  Solve time: psm_decode_paste_kernel (one case) and
// psm_chain_dots_kernel + psm_decode_paste_batch_kernel (case batches) decode, run the offset chain and paste in one pass.
//
//   decode  : f32 MFMA GEMM  blocks = res @ comp_out + mean, out_scale fused [PM:365-366, SMD:541-551]
//   chain   : serial per-block offset recurrence + global shift    [PM:391-445, 472; SMD:233-316, 350; UGP:300-340, 359-361]
//   paste   : owner-map gather of the corrected blocks into the field [PM:449-467, SMD:334-348, UGP:345-356]
//
// MFMA operand maps and the x6 split: psm_mfma.h; chain, guard and predicated-store helpers: psm_devutil.h.
#include "psm_kernels.h"
#include "psm_devutil.h"
#include "psm_mfma.h"
#include "psm_stamps.h"

#include <algorithm>
#include <cstdlib>

// ---------------------------------------------------------------------------
// geometry-bound fast path (psm_bind_geometry; structs in psm_kernels.h)
// ---------------------------------------------------------------------------
// Table build, once per geometry.  Row layout: [c_out][nst] strips, then [c_out][B] shift rows.
//   strip row (f, s):  G[k] = sum over the rectangle of block `data`, cells that are flow cells of block `mask`,
//                      of comp[k][(r*S + c)*C + f];  M = the same sum of mean;  cnt = number of such cells
//   shift row (f, b):  G[k] = sum_i 3 comp[k][A_i] - sum_i comp[k][B_i] over the shift-list entries owned by block b
// One workgroup per row, thread = component k (double accumulation: this runs once, not per solve).
__global__ __launch_bounds__(128) void psm_bind_rows_kernel(PsmBindArgs a) {
  const int C = a.c_out, S = a.S, SS = S * S, K_out = SS * C;
  const int row = blockIdx.x, n_strip_rows = C * a.nst;
  const int tid = threadIdx.x;
  double acc[4] = {0, 0, 0, 0};                       // components tid, tid+128, ... (ld_out <= 512)
  double msum = 0.0, cnt = 0.0;
  int blk_of;
  if (row < n_strip_rows) {
    const int f = row / a.nst, s = row - f * a.nst;
    const int32_t* st = a.strips + 6 * s;
    const int data = st[0], mask = st[1], r0 = st[2], r1 = st[3], c0 = st[4], c1 = st[5];
    blk_of = data;
    const int my0 = mask >= 0 ? a.blk_y0x0[2 * mask] : 0, mx0 = mask >= 0 ? a.blk_y0x0[2 * mask + 1] : 0;
    for (int r = r0; r < r1; ++r)
      for (int c = c0; c < c1; ++c) {
        const bool on = mask < 0 || a.grid[((int64_t)(my0 + r) * a.Nx + (mx0 + c)) * a.c_in + a.sdf_ch] != 0.f;
        if (!on) continue;                              // uniform
        const int col = (r * S + c) * C + f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (tid + 128 * u < a.ld_out) acc[u] += (double)a.comp[(int64_t)(tid + 128 * u) * K_out + col];
        msum += (double)a.mean[col];
        cnt += 1.0;
      }
  } else {
    const int q = row - n_strip_rows, f = q / a.B, b = q - f * a.B;
    blk_of = b;
    cnt = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
      const int32_t* list = (pass == 0 ? a.shiftOwnA : a.shiftOwnB) + (int64_t)f * a.Lmax;
      const double w = pass == 0 ? 3.0 : -1.0;
      for (int i = 0; i < a.shiftL[f]; ++i) {
        const int o = list[i];
        if (o < 0 || o / SS != b) continue;            // uniform
        const int col = (o - b * SS) * C + f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (tid + 128 * u < a.ld_out) acc[u] += w * (double)a.comp[(int64_t)(tid + 128 * u) * K_out + col];
        msum += w * (double)a.mean[col];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (tid + 128 * u < a.ld_out) a.G[(int64_t)row * a.ld_out + tid + 128 * u] = acc[u];
  if (tid == 0) { a.Mrow[row] = msum; a.cnt[row] = (float)cnt; a.row_of[row] = a.row_base + blk_of; }
}

// fold the head layer into the rows:  g2[row][j] = sum_k Wh[j][k] sa[k] G[row][k];
// c2[row] = sum_k (bh[k] sa[k] + sb[k]) G[row][k] + M[row]   (head: out = (act @ Wh + bh) * sa + sb)
__global__ __launch_bounds__(256) void psm_bind_fold_kernel(PsmBindArgs a) {
  extern __shared__ double gs[];                        // [ld_out] G row scaled by sa
  const int row = blockIdx.x, tid = threadIdx.x;
  double part = 0.0;
  for (int k = tid; k < a.ld_out; k += 256) {
    const double g = a.G[(int64_t)row * a.ld_out + k];
    gs[k] = g * (double)a.sa[k];
    part += ((double)a.bh[k] * (double)a.sa[k] + (double)a.sb[k]) * g;
  }
  __shared__ double red[256];
  red[tid] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
  if (tid == 0) a.c2[row] = (float)(red[0] + a.Mrow[row]);
  for (int j = tid; j < a.Kh; j += 256) {
    const float* w = a.Wh + (int64_t)j * a.ldw;
    double acc = 0.0;
    for (int k = 0; k < a.ld_out; ++k) acc += (double)w[k] * gs[k];
    a.g2[(int64_t)row * a.Kh + j] = (float)acc;
  }
}

__global__ __launch_bounds__(256) void psm_bind_own_kernel(PsmBindArgs a) {
  const int SS = a.S * a.S, wpb = SS / 32;
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= a.B * wpb) return;
  const int b = w / wpb, p0 = (w - b * wpb) * 32;
  const int y0 = a.blk_y0x0[2 * b], x0 = a.blk_y0x0[2 * b + 1];
  uint32_t bits = 0;
  for (int t = 0; t < 32; ++t) {
    const int px = p0 + t, r = px / a.S, c = px - r * a.S;
    if (a.owner[(int64_t)(y0 + r) * a.Nx + (x0 + c)] == b * SS + px) bits |= 1u << t;
  }
  a.ownbits[w] = bits;
}

hipError_t psm_launch_bind(const PsmBindArgs& a, hipStream_t st) {
  if (a.ld_out > 512 || a.ld_out < 1 || (a.S * a.S) % 32 != 0) return hipErrorInvalidValue;
  const int rows = a.c_out * a.nst + a.c_out * a.B;
  PSM_LAUNCH(psm_bind_rows_kernel, dim3(rows), dim3(128), 0, st, a);
  PSM_LAUNCH(psm_bind_fold_kernel, dim3(rows), dim3(256), (size_t)a.ld_out * sizeof(double), st, a);
  PSM_LAUNCH(psm_bind_own_kernel, dim3((a.B * (a.S * a.S / 32) + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}

// decode + offset chain + paste.  Waves 0-3: the decode tile of psm_decode128_kernel (one row chunk); waves 4, 5: the
// offset chain of field 0 / 1 from the strip means the head launch left in `dots`, and the global shift
// (shift_f = sum_b dots_shift[f][b] / (3 L_f) - sum_b w_b offs_b).  Both run while the other's loads are in flight;
// the epilogue writes value - offset - shift for the block pixels that own their cell (ownership bits) straight
// into the field -- the decoded blocks are never stored.
// BF (bf16 handles): the tile is rounded to bf16 on its way into LDS and multiplied with the bf16 basis by
// v_mfma_f32_32x32x16_bf16, exactly like psm_decode_bf16_kernel (psm_bf16.hip) -- same rounding points.
template <int MTC, int C, int LDR, int MODE>     // LDR = ld_res: output components padded to 32, 64, 96 or 128; MODE 0 f32, 1 bf16 handle, 2 x6
__global__ __launch_bounds__(384) void psm_decode_paste_kernel(PsmDecodeArgs a, PsmBoundArgs p) {
  constexpr bool BF = MODE == 1, X6 = MODE == 2;
  constexpr int LDX = LDR + 4;                         // x6: plane row stride in bf16
  constexpr int LDA = X6 ? 3 * LDX / 2 : (BF ? (LDR + 8) / 2 : LDR + 4);    // tile floats per row (bf16: LDR + 8 halves; x6: three planes)
  constexpr int Q = LDR / 4, GD = BF ? LDR / 16 : LDR / 8, NA = MTC * 32 * Q / 256;
  constexpr int WPB = (128 / C) / 32;                  // ownership words per block for this workgroup's 128 columns
  constexpr int NST = 8;                               // staging rounds of 384 floats (C*nst + nst <= 3072)
  constexpr int R = MTC * 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  psm_warm_kernargs<sizeof(PsmDecodeArgs) + sizeof(PsmBoundArgs)>();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int B = p.B, nst = p.n_strips, S = p.cp.S;
  // per block row, one 32-byte record for the epilogue: {element offset of the block's first cell (bits), -, out_scale, -, ownership words (WPB <= 4)}
  float* rec = lds + R * LDA;                          // [R][8]
  float* smean = rec + R * 8;                          // [C][nst]
  float* scnt = smean + C * nst;                       // [nst]
  float* offs = scnt + nst;                            // [C][B]
  float* wred = offs + C * B;                          // [4] shift per field
  const bool dec = wave < 4;                           // uniform per wave
  const int i = lane & 31, h = lane >> 5;
  const int ct = min((int)blockIdx.x * 4 + min(wave, 3), a.n_coltiles - 1);
  const bool live = dec && ((int)blockIdx.x * 4 + wave) < a.n_coltiles;
  PSM_STAMP(0, 20);
  // The FIRST HALF of the basis stream is requested before anything else (round 6): its addresses need nothing but the column tile,
  // while the small operands below cost ~250 instructions of address arithmetic and branches before the stream could start.  They
  // return behind that half (the counter is in order), which is still well before the second half has landed.
  float4 b[GD];                                        // bf16: 8 halves per 16-byte piece
  const float4* bp = a.bpack + ((int64_t)ct * GD) * 64 + lane;
#pragma unroll
  for (int g = 0; g < GD / 2; ++g) b[g] = stream_load(bp + g * 64);
  __builtin_amdgcn_sched_barrier(0);
  // ---- every load of the prologue, clamped and unconditional
  const int n_stage = p.cf ? 1 : C * nst + nst;
  float sv[NST];
  if (!p.cf) {                                         // (closed form: nothing to stage -- eight clamped loads and their address chains less)
#pragma unroll
    for (int u = 0; u < NST; ++u) {
      const int idx = min(tid + 384 * u, n_stage - 1);
      const float* src = idx < C * nst ? p.dots + idx : p.scnt + (idx - C * nst);
      sv[u] = *src;
    }
  } else {
#pragma unroll
    for (int u = 0; u < NST; ++u) sv[u] = 0.f;
  }
  // closed form of the chain: offset + shift of block b = a0 + the long dot the head launch left (one thread per value)
  const int cfi = min(tid, C * B - 1);
  // (the two terms are added where they are written to LDS: added here, the sum waited vmcnt(0) for both -- a full round trip to
  // what the head launch has just written -- BEFORE the basis stream below was requested)
  float cfa = 0.f, cfb = 0.f;
  if (p.cf) { cfa = p.cf_a0[cfi]; cfb = p.cf_dots[cfi]; }
  const int rb = min(tid, B - 1);                      // threads < B: the record of block row tid
  uint32_t ow[WPB];
#pragma unroll
  for (int w = 0; w < WPB; ++w) ow[w] = p.ownbits[(int64_t)rb * (S * S / 32) + (int)blockIdx.x * WPB + w];
  const int y0v = p.blk_y0x0[2 * rb], x0v = p.blk_y0x0[2 * rb + 1];
  const float rs = a.row_scale[min(rb, a.Mpad - 1)];
  const int cf = min(max(wave - 4, 0), C - 1);         // chain waves: their field
  const float w_shift = p.shiftW[cf * B + min(lane, B - 1)];
  const float s_raw = p.cf ? 0.f : p.dots[C * nst + cf * B + min(lane, B - 1)];
  const float gf0 = p.gflags[min(lane, p.n_gwaves - 1)], gf1 = p.gflags[min(lane + 64, p.n_gwaves - 1)];   // guard flags (0 / NaN)
  f32x4 x[NA];
#pragma unroll
  for (int u = 0; u < NA; ++u) {                       // (the two chain waves load a clamped duplicate: 384 threads, 256 slots)
    const int idx = min(tid, 255) + 256 * u, row = idx / Q, q = idx - row * Q;
    x[u] = *reinterpret_cast<const f32x4*>(a.res + (int64_t)min(row, a.Mpad - 1) * LDR + 4 * q);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int g = GD / 2; g < GD; ++g) b[g] = stream_load(bp + g * 64);
  const int col = ct * 32 + i;
  const float mu = a.mean[col];
  __builtin_amdgcn_sched_barrier(0);
  PSM_STAMP(0, 24);
  // ---- LDS staging; the barrier drains LDS traffic only, so the basis loads above stay in flight behind it
#pragma unroll
  for (int u = 0; u < NST; ++u)
    if (!p.cf && tid + 384 * u < n_stage) smean[tid + 384 * u] = sv[u];       // smean and scnt are contiguous
  if (p.cf && tid < C * B) offs[tid] = cfa + cfb;
  if (tid < B) {
    float* rr = rec + tid * 8;
    rr[0] = __uint_as_float((uint32_t)((y0v * p.Nx + x0v) * C)); rr[1] = 0.f; rr[2] = rs; rr[3] = 0.f;   // element offset of the block's first cell (one case: < 2^31)
#pragma unroll
    for (int w = 0; w < WPB; ++w) rr[4 + w] = __uint_as_float(ow[w]);
  }
  if (tid < 256) {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = tid + 256 * u, row = idx / Q, q = idx - row * Q;
      if constexpr (X6) {
        bf16x4 vh, vm, vl;
        psm_split3(x[u], vh, vm, vl);
        __bf16* dst = reinterpret_cast<__bf16*>(lds) + row * LDX + 4 * q;
        *reinterpret_cast<bf16x4*>(dst) = vh;
        *reinterpret_cast<bf16x4*>(dst + R * LDX) = vm;
        *reinterpret_cast<bf16x4*>(dst + 2 * R * LDX) = vl;
      } else if constexpr (BF) {
        bf16x4 v;
        v[0] = (__bf16)x[u][0]; v[1] = (__bf16)x[u][1]; v[2] = (__bf16)x[u][2]; v[3] = (__bf16)x[u][3];
        *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(&lds[row * LDA]) + 4 * q) = v;
      } else {
        *reinterpret_cast<f32x4*>(&lds[row * LDA + 4 * q]) = x[u];
      }
    }
  }
  PSM_STAMP(0, 25);
  PSM_LDS_BARRIER();
  PSM_STAMP(0, 21);
  f32x16 acc[MTC];
  bf16x8 Bh[X6 ? LDR / 16 : 1], Bm[X6 ? LDR / 16 : 1], Bl[X6 ? LDR / 16 : 1];
  if (dec) {
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt) {
      acc[mt] = (f32x16){0};
      if constexpr (X6) {
        const __bf16* arow = reinterpret_cast<const __bf16*>(lds) + (mt * 32 + i) * LDX + 4 * h;
#pragma unroll
        for (int st = 0; st < LDR / 16; ++st) {
          if (mt == 0) {                               // the basis slice is split on the way: each step waits for its two groups only
            bf16x4 h0, m0, l0, h1, m1, l1;
            psm_split3((f32x4){b[2 * st].x, b[2 * st].y, b[2 * st].z, b[2 * st].w}, h0, m0, l0);
            psm_split3((f32x4){b[2 * st + 1].x, b[2 * st + 1].y, b[2 * st + 1].z, b[2 * st + 1].w}, h1, m1, l1);
            Bh[st] = psm_cat4(h0, h1); Bm[st] = psm_cat4(m0, m1); Bl[st] = psm_cat4(l0, l1);
          }
          const bf16x8 ah = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 16 * st + 8));
          const bf16x8 am = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + R * LDX + 16 * st), *reinterpret_cast<const bf16x4*>(arow + R * LDX + 16 * st + 8));
          const bf16x8 al = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 2 * R * LDX + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 2 * R * LDX + 16 * st + 8));
          acc[mt] = MFMA_BF16(am, Bm[st], acc[mt]);
          acc[mt] = MFMA_BF16(al, Bh[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bl[st], acc[mt]);
          acc[mt] = MFMA_BF16(am, Bh[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bm[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bh[st], acc[mt]);
        }
      } else if constexpr (BF) {
        const __bf16* arow = reinterpret_cast<const __bf16*>(&lds[(mt * 32 + i) * LDA]) + 8 * h;
#pragma unroll
        for (int g = 0; g < GD; ++g) {
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(arow + 16 * g);
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, b[g]), acc[mt], 0, 0, 0);
        }
      } else {
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
    }
  } else if (wave - 4 < C) {
    const int f = wave - 4;
    const float guard = psm_guard_sum(p.gflags, p.n_gwaves, lane, gf0, gf1);   // NaN when the grid is not the bound geometry
    if (p.cf) {                                // closed form: the staged values already hold offset + shift
      if (lane == 0) wred[f] = guard;
    } else {
      // (the chain shares its SIMD with an MFMA wave and in effect runs after that wave's 2 us of MFMAs -- 3.7 us to the
      // chain's end instead of 1.6 alone; s_setprio(3) here changes nothing: the vector ALU itself is taken)
      psm_chain_wave(p.cp, smean + f * nst, scnt, p.blocks, f, lane, offs + f * B);
      const float t = (lane < B && w_shift != 0.f) ? w_shift * offs[f * B + lane] : 0.f;   // same-wave LDS writes are visible
      const float t_shift = wave_sum(t);
      const float raw = wave_sum(lane < B ? s_raw : 0.f);
      if (lane == 0) wred[f] = raw / (float)p.shiftL[f] / 3.f - t_shift + guard;
    }
    if (blockIdx.x == 0 && f == 0 && lane == 0) {
#if defined(PSM_STAMPS) && !defined(PSM_STAMPS_ENC)
      g_psm_stamps[39] = __builtin_amdgcn_s_memrealtime();
#endif
    }
  }
  PSM_STAMP(0, 22);
  PSM_LDS_BARRIER();
  if (blockIdx.x == 0 && !p.cf) {       // introspection copies (psm_read_stage; under the closed form it runs the chain itself)
    for (int idx = tid; idx < C * B; idx += 384) p.offs[idx] = offs[idx];
    if (tid < C) p.shift[tid] = wred[tid];
  }
  if (!live) return;
  const float mu_r = psm_settled(mu);
  const int px = col / C, f = col - px * C;
  const int pxl = px - (int)blockIdx.x * (128 / C);
  const int r = px / S, c = px - r * S;
  const float sh = wred[f];
  const uint32_t pix_off = (uint32_t)((r * p.Nx + c) * C + f);       // this lane's cell within a block's window, in elements
  // epilogue in two passes so that the LDS reads of all 16 rows are in flight together: records and offsets first
  // (straight-line), then the owned values are stored
#pragma unroll
  for (int mt = 0; mt < MTC; ++mt) {
    f32x4 ra[16], rb4[16];
    float of[16];
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int mc = min(mt * 32 + acc_row(rg, h), B - 1);
      ra[rg] = *reinterpret_cast<const f32x4*>(rec + mc * 8);
      rb4[rg] = *reinterpret_cast<const f32x4*>(rec + mc * 8 + 4);
      of[rg] = offs[f * B + mc];
    }
    auto paste = [&](auto buffered) {
      const __amdgpu_buffer_rsrc_t frs = psm_store_rsrc(p.fields, p.field_bytes);
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int m = mt * 32 + acc_row(rg, h);
        const uint32_t word = __float_as_uint(rb4[rg][pxl >> 5]);
        const bool mine = m < B && ((word >> (pxl & 31)) & 1u);
        const float val = (acc[mt][rg] + mu_r) * ra[rg][2] - of[rg] - sh;
        if constexpr (decltype(buffered)::value) psm_store_if(frs, __float_as_uint(ra[rg][0]) + pix_off, mine, val);
        else if (mine) p.fields[(size_t)(__float_as_uint(ra[rg][0]) + pix_off)] = val;
      }
    };
    if (p.field_bytes) paste(std::true_type{}); else paste(std::false_type{});        // uniform
  }
  PSM_STAMP(0, 23);
}

hipError_t psm_launch_decode_paste(const PsmDecodeArgs& a, const PsmBoundArgs& p, int c_out, hipStream_t st, int bf16) {
  if (a.ld_res > 128 || a.ld_res % 32 != 0 || a.Mpad > 64 || a.Mpad % 32 != 0 || p.B > 64 || p.B < 1 || a.M != p.B) return hipErrorInvalidValue;
  if ((c_out != 1 && c_out != 2) || c_out * p.n_strips + p.n_strips > 8 * 384) return hipErrorInvalidValue;
  const int nwg = (a.n_coltiles + 3) / 4, mtc = a.Mpad / 32, wpb = (128 / c_out) / 32;
  (void)wpb;
  const bool x6 = a.x6 && !bf16;
  const size_t tile_floats = x6 ? (size_t)mtc * 32 * (a.ld_res + 4) * 3 / 2 : (size_t)mtc * 32 * (a.ld_res + 4);
  const size_t lds = (tile_floats + (size_t)mtc * 32 * 8 + (size_t)c_out * p.n_strips + p.n_strips + (size_t)c_out * p.B + 4) * sizeof(float);
#define DP(M_, C_, L_)                                                                                              \
  do {                                                                                                              \
    if (bf16) PSM_LAUNCH((psm_decode_paste_kernel<M_, C_, L_, 1>), dim3(nwg), dim3(384), lds, st, a, p);    \
    else if (x6) PSM_LAUNCH((psm_decode_paste_kernel<M_, C_, L_, 2>), dim3(nwg), dim3(384), lds, st, a, p); \
    else PSM_LAUNCH((psm_decode_paste_kernel<M_, C_, L_, 0>), dim3(nwg), dim3(384), lds, st, a, p);         \
  } while (0)
#define DPL(L_)                                                        \
  do {                                                                 \
    if (mtc == 1) { if (c_out == 1) DP(1, 1, L_); else DP(1, 2, L_); } \
    else { if (c_out == 1) DP(2, 1, L_); else DP(2, 2, L_); }          \
  } while (0)
  if (a.ld_res == 32) DPL(32); else if (a.ld_res == 64) DPL(64); else if (a.ld_res == 96) DPL(96); else DPL(128);
#undef DPL
#undef DP
  return hipGetLastError();
}

// ---- case batches on a bound geometry: the chain of every case in one small launch (one workgroup per case, wave f =
// field f), then decode + paste for all block rows (row chunks like psm_decode128_kernel)
template <int C>
__global__ __launch_bounds__(256) void psm_chain_dots_kernel(PsmBoundBatchArgs p) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cs = blockIdx.x;
  const int B = p.B, nst = p.n_strips;
  float* smean = sm;                                   // [C][nst]
  float* scnt = smean + C * nst;                       // [nst]
  float* offs = scnt + nst;                            // [C][B]
  const float* dots = p.dots + (int64_t)cs * p.rows_pc;
  const float* cnt = p.scnt + (int64_t)cs * p.rows_pc;
  const int n_stage = C * nst + nst;
  const float gpart = psm_guard_part(p.gflags, p.n_gwaves, lane, 0);   // guard flags of this solve (0 / NaN): in flight with the staging loads
  for (int base = 0; base < n_stage; base += 256 * 8) {            // 8 loads in flight per thread and round
    float sv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = min(base + tid + 256 * u, n_stage - 1);
      sv[u] = idx < C * nst ? dots[idx] : cnt[idx - C * nst];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (base + tid + 256 * u < n_stage) smean[base + tid + 256 * u] = sv[u];
  }
  __syncthreads();
  if (wave < C) {
    psm_chain_wave(p.cp, smean + wave * nst, scnt, p.blocks, wave, lane, offs + wave * B);
    float t = 0.f, raw = 0.f;
    for (int b = lane; b < B; b += 64) {                            // same-wave LDS writes above are visible
      const float w = p.shiftW[wave * B + b];
      t += w != 0.f ? w * offs[wave * B + b] : 0.f;                   // skipped blocks have NaN offsets and weight 0
      raw += dots[C * nst + wave * B + b];
      p.offs[((int64_t)cs * C + wave) * B + b] = offs[wave * B + b];
    }
    const float t_shift = wave_sum(t), raw_all = wave_sum(raw);
    const float guard = wave_sum(gpart);                              // NaN when a grid of this batch is not its bound geometry
    if (lane == 0) p.shift[cs * C + wave] = raw_all / (float)p.shiftL[wave] / 3.f - t_shift + guard;
  }
}

hipError_t psm_launch_chain_dots(const PsmBoundBatchArgs& p, int c_out, hipStream_t st) {
  const size_t lds = ((size_t)c_out * p.n_strips + p.n_strips + (size_t)c_out * p.B) * sizeof(float);
  if ((c_out != 1 && c_out != 2) || lds > 60 * 1024 || p.B < 1) return hipErrorInvalidValue;
  if (c_out == 1) PSM_LAUNCH((psm_chain_dots_kernel<1>), dim3(p.n_cases), dim3(256), lds, st, p);
  else PSM_LAUNCH((psm_chain_dots_kernel<2>), dim3(p.n_cases), dim3(256), lds, st, p);
  return hipGetLastError();
}

template <int MTC, int C, int LDR, int MODE>           // MODE 0: exact-f32 MFMA, 1: bf16 handle (operands rounded), 2: x6 (float32 accuracy on the bf16 pipe)
__global__ __launch_bounds__(256) void psm_decode_paste_batch_kernel(PsmDecodeArgs a, PsmBoundBatchArgs p, int m_end) {
  psm_warm_kernargs<sizeof(PsmDecodeArgs) + sizeof(PsmBoundBatchArgs)>();
  DSTAMP(0);
  constexpr bool BF = MODE == 1, X6 = MODE == 2;
  constexpr int LDX = LDR + 4;                         // x6: plane row stride in bf16 (LDR / 2 + 2 dwords = 2 * odd: ds_read_b64 conflict-free)
  constexpr int LDA = X6 ? 3 * LDX / 2 : (BF ? (LDR + 8) / 2 : LDR + 4);    // tile floats per row (bf16: LDR + 8 halves; x6: three planes)
  constexpr int Q = LDR / 4, GD = BF ? LDR / 16 : LDR / 8, NA = MTC * 32 * Q / 256;
  constexpr int WPB = (128 / C) / 32, R = MTC * 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int B = p.B, S = p.cp.S, wps = S * S / 32;
  // per-row operands of the epilogue, ONE 16-byte LDS read per output value: {out_scale, offset + shift of field 0, of field 1,
  // element offset of the block's first cell in `fields` (bits)}; ownership words beside them (rows >= M own nothing)
  float4* lrow = reinterpret_cast<float4*>(lds + R * LDA);          // [R]
  uint32_t* lown = reinterpret_cast<uint32_t*>(lrow + R);           // [R][WPB]
  float* lg = reinterpret_cast<float*>(lown + R * WPB);             // [4] guard partial per wave
  const int ct = min((int)blockIdx.x * 4 + wave, a.n_coltiles - 1);
  const bool live = ((int)blockIdx.x * 4 + wave) < a.n_coltiles;
  const int m_first = (int)blockIdx.y * R, m_step = R * (int)gridDim.y;
  auto load_tile = [&](f32x4 (&x)[NA], int m_base) {
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = tid + 256 * u, row = idx / Q, q = idx - row * Q;
      x[u] = *reinterpret_cast<const f32x4*>(a.res + (int64_t)min(m_base + row, a.Mpad - 1) * LDR + 4 * q);
    }
  };
  // per-row operands of the epilogue (thread = row of the chunk): scale, offset + shift, ownership words
  struct RowOps { float rs, sa[C], sb[C]; uint32_t own[WPB]; int cs, b, y0, x0; bool in; };    // offset + shift = sa + sb, added when the row is written (the prefetch must not wait)
  auto load_rows = [&](RowOps& o, int m_base) {
    const int mr = m_base + min(tid, R - 1), m = min(mr, a.M - 1);
    o.in = mr < a.M;
    o.cs = m / B; o.b = m - o.cs * B;
    o.rs = a.row_scale[m];
    o.y0 = p.blk_y0x0[2 * o.b]; o.x0 = p.blk_y0x0[2 * o.b + 1];
#pragma unroll
    for (int w = 0; w < WPB; ++w) o.own[w] = p.ownbits[((int64_t)o.cs * B + o.b) * wps + (int)blockIdx.x * WPB + w];
  };
  // offset + shift of the row's block: requested AFTER the basis stream has been issued (first chunk), so that the sums'
  // wait does not sit in front of it
  auto load_sub = [&](RowOps& o) {
#pragma unroll
    for (int f = 0; f < C; ++f) {
      if (p.cf) {                                      // closed form: a0 + the B pair dots of this (case, field, block)
        o.sa[f] = p.cf_a0[((int64_t)o.cs * C + f) * B + o.b]; o.sb[f] = p.cf_dots[((int64_t)o.cs * C + f) * B + o.b];
      } else {
        o.sa[f] = p.offs[((int64_t)o.cs * C + f) * B + o.b]; o.sb[f] = p.shift[o.cs * C + f];
      }
    }
  };
  f32x4 x[NA];
  RowOps ro;
  load_tile(x, m_first);
  load_rows(ro, m_first);
  // guard flags of this solve (0, or NaN after a geometry mismatch): with the closed form there is no chain launch to fold
  // them into the shift, so every workgroup sums them itself.  The first 1024 (64 cases) are requested HERE, in front of the
  // basis stream: as a loop behind it they were a round trip of their own after everything else had landed.
  float gv0[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) gv0[u] = p.gflags[min(tid + 256 * u, p.n_gwaves - 1)];     // (unconditional: never null, >= 1 entry)
  __builtin_amdgcn_sched_barrier(0);
  float4 b[GD];
  const float4* bp = a.bpack + ((int64_t)ct * GD) * 64 + lane;
#pragma unroll
  for (int g = 0; g < GD; ++g) b[g] = stream_load(bp + g * 64);
  const int col = ct * 32 + i;
  const float mu = a.mean[col];
  __builtin_amdgcn_sched_barrier(0);
  load_sub(ro);
  float gpart = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) gpart += (p.cf && tid + 256 * u < p.n_gwaves) ? gv0[u] : 0.f;
  if (p.cf) {
    for (int k0 = tid + 1024; k0 < p.n_gwaves; k0 += 256 * 4) {      // more than 64 cases' worth of flags
      float gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = p.gflags[min(k0 + 256 * u, p.n_gwaves - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) gpart += (k0 + 256 * u < p.n_gwaves) ? gv[u] : 0.f;
    }
  }
  {
    const float gw = wave_sum(gpart);
    if (lane == 0) lg[wave] = gw;
  }
  // x6: this wave's basis slice split once into three bf16 planes (registers); reused by every row chunk
  bf16x8 Bh[X6 ? LDR / 16 : 1], Bm[X6 ? LDR / 16 : 1], Bl[X6 ? LDR / 16 : 1];
  if constexpr (X6) {
#pragma unroll
    for (int st = 0; st < LDR / 16; ++st) {
      bf16x4 h0, m0, l0, h1, m1, l1;
      psm_split3((f32x4){b[2 * st].x, b[2 * st].y, b[2 * st].z, b[2 * st].w}, h0, m0, l0);
      psm_split3((f32x4){b[2 * st + 1].x, b[2 * st + 1].y, b[2 * st + 1].z, b[2 * st + 1].w}, h1, m1, l1);
      Bh[st] = psm_cat4(h0, h1); Bm[st] = psm_cat4(m0, m1); Bl[st] = psm_cat4(l0, l1);
    }
  }
  const int px = col / C, f = col - px * C;
  const int pxl = px - (int)blockIdx.x * (128 / C);
  const int r = px / S, c = px - r * S;
  const uint32_t pix_off = (uint32_t)((r * p.Nx + c) * C + f);       // this lane's cell within a block's window, in elements
  const int own_w = pxl >> 5;
  const uint32_t own_bit = 1u << (pxl & 31);
  const float mu_r = psm_settled(mu);                  // (64 cases: 4.6 us per chunk for 0.6 us of MFMAs before this)
  // Row chunks.  The NEXT chunk's activation tile and row operands are requested as soon as the current tile sits in LDS and
  // land during its MFMAs and stores (they were a full exposed round trip per chunk: 64 cases are 4-5 chunks per workgroup).
  DSTAMP(1);
  int dchunk = 0;
  for (int m_base = m_first; m_base < m_end; m_base += m_step, ++dchunk) {
    if (m_base != m_first) __syncthreads();            // every wave is done with the previous chunk's tile and row operands
    DSTAMP(2 + 5 * dchunk);
#pragma unroll
    for (int u = 0; u < NA; ++u) {
      const int idx = tid + 256 * u, row = idx / Q, q = idx - row * Q;
      if constexpr (X6) {                            // exact three-way split, one bf16 plane each
        bf16x4 vh, vm, vl;
        psm_split3(x[u], vh, vm, vl);
        __bf16* dst = reinterpret_cast<__bf16*>(lds) + row * LDX + 4 * q;
        *reinterpret_cast<bf16x4*>(dst) = vh;
        *reinterpret_cast<bf16x4*>(dst + R * LDX) = vm;
        *reinterpret_cast<bf16x4*>(dst + 2 * R * LDX) = vl;
      } else if constexpr (BF) {
        bf16x4 v;
        v[0] = (__bf16)x[u][0]; v[1] = (__bf16)x[u][1]; v[2] = (__bf16)x[u][2]; v[3] = (__bf16)x[u][3];
        *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(&lds[row * LDA]) + 4 * q) = v;
      } else {
        *reinterpret_cast<f32x4*>(&lds[row * LDA + 4 * q]) = x[u];
      }
    }
    if (tid < R) {
      const uint32_t off = (uint32_t)(((int64_t)ro.cs * p.npix + (int64_t)ro.y0 * p.Nx + ro.x0) * C);
      lrow[tid] = make_float4(ro.rs, ro.sa[0] + ro.sb[0], ro.sa[C - 1] + ro.sb[C - 1], __uint_as_float(off));
#pragma unroll
      for (int w = 0; w < WPB; ++w) lown[tid * WPB + w] = ro.in ? ro.own[w] : 0u;
    }
    __syncthreads();
    DSTAMP(3 + 5 * dchunk);
    if (m_base + m_step < m_end) {                     // uniform
      load_tile(x, m_base + m_step);
      load_rows(ro, m_base + m_step);
      load_sub(ro);
    }
    __builtin_amdgcn_sched_barrier(0);
    DSTAMP(4 + 5 * dchunk);
    f32x16 acc[MTC];
#pragma unroll
    for (int mt = 0; mt < MTC; ++mt) {
      acc[mt] = (f32x16){0};
      if constexpr (X6) {
        const __bf16* arow = reinterpret_cast<const __bf16*>(lds) + (mt * 32 + i) * LDX + 4 * h;
#pragma unroll
        for (int st = 0; st < LDR / 16; ++st) {
          const bf16x8 ah = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 16 * st + 8));
          const bf16x8 am = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + R * LDX + 16 * st), *reinterpret_cast<const bf16x4*>(arow + R * LDX + 16 * st + 8));
          const bf16x8 al = psm_cat4(*reinterpret_cast<const bf16x4*>(arow + 2 * R * LDX + 16 * st), *reinterpret_cast<const bf16x4*>(arow + 2 * R * LDX + 16 * st + 8));
          acc[mt] = MFMA_BF16(am, Bm[st], acc[mt]);
          acc[mt] = MFMA_BF16(al, Bh[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bl[st], acc[mt]);
          acc[mt] = MFMA_BF16(am, Bh[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bm[st], acc[mt]);
          acc[mt] = MFMA_BF16(ah, Bh[st], acc[mt]);
        }
      } else if constexpr (BF) {
        const __bf16* arow = reinterpret_cast<const __bf16*>(&lds[(mt * 32 + i) * LDA]) + 8 * h;
#pragma unroll
        for (int g = 0; g < GD; ++g) {
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(arow + 16 * g);
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, b[g]), acc[mt], 0, 0, 0);
        }
      } else {
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
    }
    DSTAMP(5 + 5 * dchunk);
    if (live) {
      const __amdgpu_buffer_rsrc_t frs = psm_store_rsrc(p.fields, p.field_bytes);
      const float gsum = (lg[0] + lg[1]) + (lg[2] + lg[3]);            // written before the barrier above
      auto paste = [&](auto buffered) {
#pragma unroll
        for (int mt = 0; mt < MTC; ++mt) {
#pragma unroll
          for (int rg = 0; rg < 16; ++rg) {
            const int rr = mt * 32 + acc_row(rg, h);
            const float4 ro4 = lrow[rr];
            const bool mine = (lown[rr * WPB + own_w] & own_bit) != 0u;
            const float val = (acc[mt][rg] + mu_r) * ro4.x - (C == 2 && f ? ro4.z : ro4.y) - gsum;
            if constexpr (decltype(buffered)::value) psm_store_if(frs, __float_as_uint(ro4.w) + pix_off, mine, val);
            else if (mine) p.fields[(size_t)(__float_as_uint(ro4.w) + pix_off)] = val;
          }
        }
      };
      if (p.field_bytes) paste(std::true_type{}); else paste(std::false_type{});      // uniform
    }
    DSTAMP(6 + 5 * dchunk);
  }
}

hipError_t psm_launch_decode_paste_batch(const PsmDecodeArgs& a, const PsmBoundBatchArgs& p, int c_out, hipStream_t st, int mtc, int wg_target, int bf16) {
  if (a.ld_res > 128 || a.ld_res % 32 != 0 || a.Mpad % 32 != 0 || p.B > 4096 || p.B < 1 || a.M != p.B * p.n_cases) return hipErrorInvalidValue;
  if (c_out != 1 && c_out != 2) return hipErrorInvalidValue;
  if (mtc < 1 || mtc > 3) return hipErrorInvalidValue;     // row tiles per chunk: the 4-tile form of this kernel spills (acc + tile + row operands)
  const int nwg = (a.n_coltiles + 3) / 4;
  // mtc row tiles per chunk, the chunks spread over up to `wg_target / nwg` row groups (grid.y): the route's choice, measured there
  const int tiles = a.Mpad / 32, wpb = (128 / c_out) / 32;
  const int groups = std::min((tiles + mtc - 1) / mtc, std::max(1, wg_target / nwg));
  const int R = mtc * 32;
  const bool x6 = a.x6 && !bf16;
  const size_t tile_floats = x6 ? (size_t)R * (a.ld_res + 4) * 3 / 2 : (size_t)R * (a.ld_res + 4);
  const size_t lds = (tile_floats + 4 * (size_t)R + (size_t)R * wpb + 4) * sizeof(float);
  if ((int64_t)p.n_cases * p.npix * c_out >= (int64_t)1 << 32) return hipErrorInvalidValue;   // cell offsets are 32-bit element counts
  const dim3 grid(nwg, groups);
#define DP(M_, C_, L_)                                                                                                          \
  do {                                                                                                                          \
    if (bf16) PSM_LAUNCH((psm_decode_paste_batch_kernel<M_, C_, L_, 1>), grid, dim3(256), lds, st, a, p, a.Mpad);      \
    else if (x6) PSM_LAUNCH((psm_decode_paste_batch_kernel<M_, C_, L_, 2>), grid, dim3(256), lds, st, a, p, a.Mpad);   \
    else PSM_LAUNCH((psm_decode_paste_batch_kernel<M_, C_, L_, 0>), grid, dim3(256), lds, st, a, p, a.Mpad);           \
  } while (0)
#define DPM(C_, L_)                                                                 \
  do {                                                                              \
    if (mtc == 3) DP(3, C_, L_); else if (mtc == 2) DP(2, C_, L_); else DP(1, C_, L_); \
  } while (0)
#define DPL(L_) do { if (c_out == 1) DPM(1, L_); else DPM(2, L_); } while (0)
  if (a.ld_res == 32) DPL(32); else if (a.ld_res == 64) DPL(64); else if (a.ld_res == 96) DPL(96); else DPL(128);
#undef DPL
#undef DPM
#undef DP
  return hipGetLastError();
}

// ---- bf16 handles on a bound geometry: the decode rounds `res` to bf16, which is not linear, so the strip dots
// cannot be folded through the head layer; they are taken from the rounded `res` itself in a small launch of their
// own (one wave per table row):  out[row] = scale * (bf16(res[b]) . G[row] + M[row]) / cnt[row]
// pair rows of the closed form (bind time): g2p[pair] = sum_e coef_e g2[src_e], c2p likewise
__global__ __launch_bounds__(256) void psm_pair_fold_kernel(PsmPairFoldArgs a) {
  const int pr = blockIdx.x;
  const int e0 = a.ptr[pr], e1 = a.ptr[pr + 1];
  for (int k = threadIdx.x; k < a.Kh; k += 256) {
    double acc = 0.0;
    for (int e = e0; e < e1; ++e) acc += (double)a.coef[e] * (double)a.g2[(int64_t)a.src[e] * a.Kh + k];
    a.g2p[(int64_t)pr * a.Kh + k] = (float)acc;
  }
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int e = e0; e < e1; ++e) acc += (double)a.coef[e] * (double)a.c2[a.src[e]];
    a.c2p[pr] = (float)acc;
  }
}
hipError_t psm_launch_pair_fold(const PsmPairFoldArgs& a, hipStream_t st) {
  if (a.n_pairs < 1 || a.Kh < 1) return hipErrorInvalidValue;
  PSM_LAUNCH(psm_pair_fold_kernel, dim3(a.n_pairs), dim3(256), 0, st, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void psm_bind_copy_kernel(PsmBindArgs a) {   // un-folded tables: g2 = G, c2 = M
  const int row = blockIdx.x;
  for (int k = threadIdx.x; k < a.ld_out; k += 256) a.g2[(int64_t)row * a.ld_out + k] = (float)a.G[(int64_t)row * a.ld_out + k];
  if (threadIdx.x == 0) a.c2[row] = (float)a.Mrow[row];
}

hipError_t psm_launch_bind_unfolded(const PsmBindArgs& a, hipStream_t st) {
  if (a.ld_out > 512 || a.ld_out < 1 || (a.S * a.S) % 32 != 0) return hipErrorInvalidValue;
  const int rows = a.c_out * a.nst + a.c_out * a.B;
  PSM_LAUNCH(psm_bind_rows_kernel, dim3(rows), dim3(128), 0, st, a);
  PSM_LAUNCH(psm_bind_copy_kernel, dim3(rows), dim3(256), 0, st, a);
  PSM_LAUNCH(psm_bind_own_kernel, dim3((a.B * (a.S * a.S / 32) + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}
