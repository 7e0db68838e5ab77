// psm_assemble.hip -- from decoded blocks to the field on the general solve path, hand-written for gfx950 (CDNA4, wave64):
// kernels and launchers, and the ring's stage-in kernel.
//
//   strips  : masked overlap-strip sums of the raw decoded blocks  [PM:391-445, SMD:233-316, UGP:300-340]
//   chain   : serial per-block offset recurrence + global shift    [same lines; PM:472, SMD:350, UGP:359-361]
//   paste   : owner-map gather of the corrected blocks into the field [PM:449-467, SMD:334-348, UGP:345-356]
//
// psm_strips_kernel, psm_chain_kernel, psm_assemble_kernel (chain + shift + paste in one launch), psm_paste_kernel,
// psm_stage_in_kernel.  The recurrence itself (psm_chain_rows / psm_chain_wave) is in psm_devutil.h: the bound path runs it too.
#include "psm_kernels.h"
#include "psm_devutil.h"
#include "psm_mfma.h"
#include "psm_stamps.h"

// ---------------------------------------------------------------------------
// strips: one workgroup per (block, band of 16 rows).  Every decoded value of the band
// (the block's own and the previous block's, the latter under THIS block's mask) is read
// once into registers; the band's contribution to each of the block's strip rectangles is
// reduced over the workgroup and stored as a partial (sum per field, count).
// ---------------------------------------------------------------------------
template <int C_OUT>
__global__ __launch_bounds__(256) void psm_strips_kernel(PsmStripArgs a) {
  constexpr int RB = PSM_STRIP_BAND;                 // rows per band
  constexpr int RPT = RB / 2;                        // rows per thread (two half-bands of 128 columns)
  __shared__ float2 colred[2][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, band = blockIdx.y, cs = blockIdx.z;
  const int S = a.S, SS = S * S;
  const int c = tid & 127, half = tid >> 7;
  const int rbase = band * RB + half * RPT;
  const float* self = a.pred + ((int64_t)(cs * a.B + b) * SS + (int64_t)rbase * S + c) * C_OUT;
  const float* prev = b > 0 ? self - (int64_t)SS * C_OUT : self;
  const float* gm = a.grid + (((int64_t)cs * a.Ny + a.blk_y0x0[2 * b] + rbase) * a.Nx + a.blk_y0x0[2 * b + 1] + c) * a.c_in + a.sdf_ch;
  PSM_STAMP(0, 28);
  __shared__ int32_t tab[C_NS * 6];                 // this block's strip rectangles
  float vs[RPT][C_OUT], vp[RPT][C_OUT];
  bool on[RPT];
  // decoded values and the rectangle table first: their addresses need nothing but the launch
  // arguments; the mask loads wait for the block's grid origin (a dependent scalar load)
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
#pragma unroll
    for (int f = 0; f < C_OUT; ++f) {
      vs[k][f] = self[(int64_t)k * S * C_OUT + f];
      vp[k][f] = prev[(int64_t)k * S * C_OUT + f];
    }
  }
  const int32_t tabv = a.strips[(int64_t)b * a.NS * 6 + min(tid, a.NS * 6 - 1)];
  __builtin_amdgcn_sched_barrier(0);
  float gv[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) gv[k] = gm[(int64_t)k * a.Nx * a.c_in];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < RPT; ++k) on[k] = gv[k] != 0.f;
  if (tid < a.NS * 6) tab[tid] = tabv;
  const int NS = a.NS;
  // per-thread totals over its RPT rows (flow cells only / all cells), then per-COLUMN totals of
  // the band in LDS: a rectangle covering the band's rows completely (the usual case) is then a
  // sum of column totals over [c0, c1), done by ONE wave per slot
  constexpr int NQ = 3 * C_OUT + 1;                  // masked self [C], masked prev [C], unmasked self [C], flow-cell count
  __shared__ float colT[NQ][2][128];
  __shared__ float fin[C_NS][3];
  __shared__ float wsum[4][C_NS][3];
  float tot_s[C_OUT], tot_p[C_OUT], tot_cnt = 0.f, all_s[C_OUT];
#pragma unroll
  for (int f = 0; f < C_OUT; ++f) { tot_s[f] = 0.f; tot_p[f] = 0.f; all_s[f] = 0.f; }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
#pragma unroll
    for (int f = 0; f < C_OUT; ++f) {
      tot_s[f] += on[k] ? vs[k][f] : 0.f;
      tot_p[f] += on[k] ? vp[k][f] : 0.f;
      all_s[f] += vs[k][f];
    }
    tot_cnt += on[k] ? 1.f : 0.f;
  }
#pragma unroll
  for (int f = 0; f < C_OUT; ++f) {
    colT[f][half][c] = tot_s[f];
    colT[C_OUT + f][half][c] = tot_p[f];
    colT[2 * C_OUT + f][half][c] = all_s[f];
  }
  colT[3 * C_OUT][half][c] = tot_cnt;
  __syncthreads();
  PSM_STAMP(0, 29);                                  // loads landed, column totals in LDS
  const int32_t* st = tab;
  float4* outp = a.spart + (((int64_t)cs * a.B + b) * a.n_bands + band) * NS;
  static_assert(C_NS <= 12, "three slots per wave");
  // slots whose rectangle cuts this band (row tests needed): found once, by every wave
  unsigned long long pmask;
  {
    const int sl = min(lane, NS - 1);
    const int r0 = st[6 * sl + 2], r1 = st[6 * sl + 3], c0 = st[6 * sl + 4], c1 = st[6 * sl + 5];
    const bool live = !(r1 <= band * RB || r0 >= (band + 1) * RB || c1 <= c0);
    const bool whole = (r0 <= band * RB && r1 >= (band + 1) * RB);
    pmask = __ballot(lane < NS && live && !whole);
  }
  // every other slot is a sum of column totals over [c0, c1): wave w takes slots w, w+4, w+8 --
  // straight-line (selects, no branches), nine wave sums interleaved
  float rs[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int s = wave + 4 * j, sv = min(s, NS - 1);
    const int data = st[6 * sv], mask = st[6 * sv + 1], r0 = st[6 * sv + 2], r1 = st[6 * sv + 3], c0 = st[6 * sv + 4], c1 = st[6 * sv + 5];
    const bool live = !(r1 <= band * RB || r0 >= (band + 1) * RB || c1 <= c0);
    const bool whole = (r0 <= band * RB && r1 >= (band + 1) * RB);
    const bool ok = (s < NS) && live && whole;
    const int qb = mask < 0 ? 2 * C_OUT : (data != b ? C_OUT : 0);
    float s0 = 0.f, s1 = 0.f, cnt = 0.f;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int cc = lane + 64 * h2;
      const bool in = ok && (cc >= c0 && cc < c1);
      const float t0 = colT[qb][0][cc] + colT[qb][1][cc];
      const float t1 = colT[qb + C_OUT - 1][0][cc] + colT[qb + C_OUT - 1][1][cc];
      const float tc = colT[3 * C_OUT][0][cc] + colT[3 * C_OUT][1][cc];
      s0 += in ? t0 : 0.f;
      s1 += in ? t1 : 0.f;
      cnt += in ? (mask < 0 ? (float)RB : tc) : 0.f;
    }
    rs[j][0] = s0; rs[j][1] = s1; rs[j][2] = cnt;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    rs[j][0] = wave_sum(rs[j][0]);
    if (C_OUT > 1) rs[j][1] = wave_sum(rs[j][1]); else rs[j][1] = rs[j][0];
    rs[j][2] = wave_sum(rs[j][2]);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = wave + 4 * j;
      if (s < C_NS) { fin[s][0] = rs[j][0]; fin[s][1] = rs[j][1]; fin[s][2] = rs[j][2]; }
    }
  }
  for (unsigned long long pm = pmask; pm; pm &= pm - 1) {     // band cut by the rectangle: row tests, whole workgroup
    const int s = __ffsll((long long)pm) - 1;
    const int data = st[6 * s], mask = st[6 * s + 1], r0 = st[6 * s + 2], r1 = st[6 * s + 3], c0 = st[6 * s + 4], c1 = st[6 * s + 5];
    const bool use_prev = (data != b);
    float s0 = 0.f, s1 = 0.f, cnt = 0.f;
    if (c >= c0 && c < c1) {
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const int r = rbase + k;
        if (r >= r0 && r < r1 && (mask < 0 || on[k])) {
          s0 += use_prev ? vp[k][0] : vs[k][0];
          if (C_OUT > 1) s1 += use_prev ? vp[k][C_OUT - 1] : vs[k][C_OUT - 1];
          cnt += 1.f;
        }
      }
    }
    s0 = wave_sum(s0); if (C_OUT > 1) s1 = wave_sum(s1); cnt = wave_sum(cnt);
    if (lane == 0) { wsum[wave][s][0] = s0; wsum[wave][s][1] = s1; wsum[wave][s][2] = cnt; }
  }
  __syncthreads();
  PSM_STAMP(0, 30);
  if (tid < NS) {
    const int s = tid;
    if ((pmask >> s) & 1ull)
      outp[s] = make_float4((wsum[0][s][0] + wsum[1][s][0]) + (wsum[2][s][0] + wsum[3][s][0]),
                            (wsum[0][s][1] + wsum[1][s][1]) + (wsum[2][s][1] + wsum[3][s][1]),
                            (wsum[0][s][2] + wsum[1][s][2]) + (wsum[2][s][2] + wsum[3][s][2]), 0.f);
    else
      outp[s] = make_float4(fin[s][0], fin[s][1], fin[s][2], 0.f);
  }
  // gradp: per-column sums of block 0, field 0 (first column holding a flow cell, UGP:294-300)
  if (a.colpart && b == 0) {
    float s0 = 0.f, cnt = 0.f;
#pragma unroll
    for (int k = 0; k < RPT; ++k)
      if (on[k]) { s0 += vs[k][0]; cnt += 1.f; }
    colred[half][c] = make_float2(s0, cnt);
    __syncthreads();
    if (half == 0) {
      const float2 u = colred[0][c], v = colred[1][c];
      a.colpart[((int64_t)cs * a.n_bands + band) * 128 + c] = make_float2(u.x + v.x, u.y + v.y);
    }
  }
}

hipError_t psm_launch_strips(const PsmStripArgs& a, int n_cases, hipStream_t st) {
  if (a.S != 128) return hipErrorInvalidValue;
  if (a.c_out == 1) PSM_LAUNCH((psm_strips_kernel<1>), dim3(a.B, a.n_bands, n_cases), dim3(256), 0, st, a);
  else PSM_LAUNCH((psm_strips_kernel<2>), dim3(a.B, a.n_bands, n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// chain (+ global shift): one workgroup per case.  All strip partials are combined into
// LDS by the whole workgroup, lane 0 of wave f runs the serial recurrence of field f.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512) void psm_chain_kernel(PsmChainArgs a) {
  constexpr int NB = 128 / PSM_STRIP_BAND;            // bands per block
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cs = blockIdx.x;
  const int B = a.cp.B, SS = a.cp.S * a.cp.S, NS = a.cp.NS, C = a.c_out;
  const int nst = a.n_strips;                         // B*NS (+128 column strips for gradp)
  float* smean = sm;                                  // [C][nst]  sum/count (0/0 -> NaN like np.mean([]))
  float* scnt = smean + C * nst;                      // [nst]
  float* offs = scnt + nst;                           // [C][B]
  float* up = offs + C * B;                           // [C][PSM_MAX_COLS] (fallback path only)
  float* wred = up + C * PSM_MAX_COLS;                // [8]
  const float4* sp = a.spart + (int64_t)cs * B * NB * NS;
  for (int idx = tid; idx < B * NS; idx += 512) {
    const int b = idx / NS, s = idx - b * NS;
    float4 v[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) v[q] = sp[((int64_t)b * NB + q) * NS + s];   // all bands in flight
    float s0 = 0.f, s1 = 0.f, cn = 0.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) { s0 += v[q].x; s1 += v[q].y; cn += v[q].z; }
    smean[idx] = s0 / cn;
    if (C > 1) smean[nst + idx] = s1 / cn;
    scnt[idx] = cn;
  }
  if (a.colpart) {
    for (int c = tid; c < 128; c += 512) {
      float2 v[NB];
#pragma unroll
      for (int q = 0; q < NB; ++q) v[q] = a.colpart[((int64_t)cs * NB + q) * 128 + c];
      float s0 = 0.f, cn = 0.f;
#pragma unroll
      for (int q = 0; q < NB; ++q) { s0 += v[q].x; cn += v[q].y; }
      smean[B * NS + c] = s0 / cn;
      if (C > 1) smean[nst + B * NS + c] = 0.f;
      scnt[B * NS + c] = cn;
    }
  }
  for (int idx = tid; idx < C * PSM_MAX_COLS; idx += 512) up[idx] = 0.f;
  __syncthreads();
  if (wave < C) {
    if (a.cp.n_x + 2 <= 64) {
      psm_chain_wave(a.cp, smean + wave * nst, scnt, a.blocks, wave, lane, offs + wave * B);
    } else if (lane == 0) {
      PsmArrayChainCtx<float> cx{a.blocks, smean + wave * nst, scnt, NS, a.cp.col_base, a.cp.S, up + wave * PSM_MAX_COLS, offs + wave * B};
      psm_chain<float>(a.cp, cx, wave);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < C * B; idx += 512) a.offs[(int64_t)cs * C * B + idx] = offs[idx];
  for (int f = 0; f < C; ++f) {
    const int L = a.shiftL[f];
    const int32_t* la = a.shiftA + (int64_t)f * a.Lmax;
    const int32_t* lb = a.shiftB + (int64_t)f * a.Lmax;
    const float* pred = a.pred + ((int64_t)cs * B * SS) * C + f;
    float acc = 0.f;
    for (int k = tid; k < L; k += 512) {
      const int oa = a.owner[la[k]], ob = a.owner[lb[k]];
      const float va = oa >= 0 ? pred[(int64_t)oa * C] - offs[f * B + oa / SS] : 0.f;
      const float vb = ob >= 0 ? pred[(int64_t)ob * C] - offs[f * B + ob / SS] : 0.f;
      acc += 3.f * va - vb;
    }
    acc = wave_sum(acc);
    __syncthreads();
    if (lane == 0) wred[wave] = acc;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < 8; ++w) t += wred[w];
      a.shift[cs * C + f] = t / (float)L / 3.f;
    }
  }
}

hipError_t psm_launch_chain(const PsmChainArgs& a, int n_cases, hipStream_t st) {
  const size_t lds = ((size_t)a.c_out * a.n_strips + a.n_strips + (size_t)a.c_out * a.cp.B + (size_t)a.c_out * PSM_MAX_COLS + 8) * sizeof(float);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  PSM_LAUNCH(psm_chain_kernel, dim3(n_cases), dim3(512), lds, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// assemble = chain + shift + paste in one launch (small block counts): every paste
// workgroup re-runs the (cheap, register-resident) offset chain instead of waiting for a
// separate one-workgroup launch.  The global shift is split into a part that does not
// depend on the offsets (gathered while the strip partials are in flight) and a weighted
// sum of the offsets:  shift = sum_k(3 pred[A_k] - pred[B_k])/(3L) - sum_b w_b offs_b.
// ---------------------------------------------------------------------------

template <int C>
__global__ __launch_bounds__(256) void psm_assemble_kernel(PsmChainArgs a, PsmPasteArgs p) {
  constexpr int NB = 128 / PSM_STRIP_BAND;
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cs = blockIdx.y;
  const int B = a.cp.B, SS = a.cp.S * a.cp.S, NS = a.cp.NS;
  const int nst = a.n_strips;
  float* smean = sm;                                  // [C][nst]
  float* scnt = smean + C * nst;                      // [nst]
  float* offs = scnt + nst;                           // [C][B]
  float* wred = offs + C * B;                         // [C][4] + [C] shift
  PSM_STAMP(0, 36);
  // ---- phase 1a: every independent load (cell owner, shift-list owners, strip partials).
  // Straight-line: indices are clamped and results selected, so that all loads of a phase are
  // in flight together (a conditional load costs a branch and, with it, a drained vmcnt).
  const int pix = blockIdx.x * 256 + tid;
  const int o_raw = a.owner[min(pix, p.npix - 1)];
  int la[C], lb[C];                                  // one shift-list entry per thread and field (L <= 256 on this path)
#pragma unroll
  for (int f = 0; f < C; ++f) {
    const int kk = (int)((int64_t)f * a.Lmax) + min(tid, max(a.shiftL[f], 1) - 1);
    la[f] = a.shiftOwnA[kk];
    lb[f] = a.shiftOwnB[kk];
  }
  const float4* sp = a.spart + (int64_t)cs * B * NB * NS;
  const int idx0 = tid, idx1 = tid + 256;             // B*NS <= 64*11 = 704 -> at most 3 per thread
  f32x4 pv0[NB], pv1[NB];
  {
    const int b0 = min(idx0, B * NS - 1) / NS, s0 = min(idx0, B * NS - 1) - b0 * NS;
    const int b1 = min(idx1, B * NS - 1) / NS, s1 = min(idx1, B * NS - 1) - b1 * NS;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      pv0[q] = *reinterpret_cast<const f32x4*>(sp + ((int64_t)b0 * NB + q) * NS + s0);
      pv1[q] = *reinterpret_cast<const f32x4*>(sp + ((int64_t)b1 * NB + q) * NS + s1);
    }
  }
  float2 cp[NB];
  if (a.colpart) {                                    // uniform
#pragma unroll
    for (int q = 0; q < NB; ++q) cp[q] = a.colpart[((int64_t)cs * NB + q) * 128 + (tid & 127)];
  }
  const float w_shift = a.shiftW[min(wave, C - 1) * B + min(lane, B - 1)];   // used after the chain (waves < C)
  __builtin_amdgcn_sched_barrier(0);
  // ---- phase 1b: dependent gathers from the decoded blocks.  They are NOT waited for before the
  // chain: the barriers below are LDS-only (s_waitcnt lgkmcnt(0); s_barrier), so these loads land
  // while the offset chain runs.
  const int o = pix < p.npix ? o_raw : -1;
  const float* predc = a.pred + ((int64_t)cs * B * SS) * C;
  float src[C], ga[C], gb[C];
#pragma unroll
  for (int f = 0; f < C; ++f) {
    const bool in = tid < a.shiftL[f];
    la[f] = in ? la[f] : -1;
    lb[f] = in ? lb[f] : -1;
    src[f] = predc[(int64_t)max(o, 0) * C + f];
    ga[f] = predc[(int64_t)max(la[f], 0) * C + f];
    gb[f] = predc[(int64_t)max(lb[f], 0) * C + f];
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- strip partials -> means
  auto fold = [&](const f32x4 (&v)[NB], int idx) {
    float s0 = 0.f, s1 = 0.f, cn = 0.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) { s0 += v[q].x; s1 += v[q].y; cn += v[q].z; }
    const float m0 = s0 / cn, m1 = s1 / cn;
    if (idx < B * NS) {
      smean[idx] = m0;
      if (C > 1) smean[nst + idx] = m1;
      scnt[idx] = cn;
    }
  };
  fold(pv0, idx0);
  fold(pv1, idx1);
  for (int idx = tid + 512; idx < B * NS; idx += 256) {   // only for > 46 blocks
    const int b = idx / NS, s = idx - b * NS;
    f32x4 v[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) v[q] = *reinterpret_cast<const f32x4*>(sp + ((int64_t)b * NB + q) * NS + s);
    fold(v, idx);
  }
  if (a.colpart) {
    float s0 = 0.f, cn = 0.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) { s0 += cp[q].x; cn += cp[q].y; }
    const float m0 = s0 / cn;
    if (tid < 128) {
      smean[B * NS + tid] = m0;
      if (C > 1) smean[nst + B * NS + tid] = 0.f;
      scnt[B * NS + tid] = cn;
    }
  }
  PSM_LDS_BARRIER();
  PSM_STAMP(0, 37);
  float t_shift = 0.f;
  if (wave < C) {
    PSM_STAMP(0, 38);
    psm_chain_wave(a.cp, smean + wave * nst, scnt, a.blocks, wave, lane, offs + wave * B);
    PSM_STAMP(0, 39);
    // shift of this field: weighted sum of the offsets (B <= 64 on this path); same-wave LDS
    // writes above are visible to the wave's own later reads
    const float t = (lane < B && w_shift != 0.f) ? w_shift * offs[wave * B + lane] : 0.f;
    t_shift = wave_sum(t);
  }
  // offset-independent part of the shift (the gathers have landed under the chain)
  float pp[C];
#pragma unroll
  for (int f = 0; f < C; ++f) {
    float acc = 3.f * (la[f] >= 0 ? ga[f] : 0.f) - (lb[f] >= 0 ? gb[f] : 0.f);
    for (int k = tid + 256; k < a.shiftL[f]; k += 256) {   // lists longer than 256 (not on the small-grid path)
      const int ia = a.shiftOwnA[(int64_t)f * a.Lmax + k], ib = a.shiftOwnB[(int64_t)f * a.Lmax + k];
      acc += 3.f * (ia >= 0 ? predc[(int64_t)ia * C + f] : 0.f) - (ib >= 0 ? predc[(int64_t)ib * C + f] : 0.f);
    }
    pp[f] = wave_sum(acc);
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < C; ++f) wred[f * 4 + wave] = pp[f];
  }
  PSM_LDS_BARRIER();
  if (wave < C && lane == 0) {
    const float part = (wred[wave * 4 + 0] + wred[wave * 4 + 1]) + (wred[wave * 4 + 2] + wred[wave * 4 + 3]);
    wred[4 * C + wave] = part / (float)a.shiftL[wave] / 3.f - t_shift;
  }
  PSM_LDS_BARRIER();
  PSM_STAMP(0, 40);
  if (blockIdx.x == 0) {       // introspection copies (psm_read_stage)
    for (int idx = tid; idx < C * B; idx += 256) a.offs[(int64_t)cs * C * B + idx] = offs[idx];
    if (tid < C) a.shift[cs * C + tid] = wred[4 * C + tid];
  }
  if (pix >= p.npix) return;
  float* out = p.fields + ((int64_t)cs * p.npix + pix) * C;
  if (o < 0) {
#pragma unroll
    for (int f = 0; f < C; ++f) out[f] = 0.f;
    return;
  }
  const int b = o / SS;
#pragma unroll
  for (int f = 0; f < C; ++f) out[f] = src[f] - offs[f * B + b] - wred[4 * C + f];
  PSM_STAMP(0, 41);
}

hipError_t psm_launch_assemble(const PsmChainArgs& a, const PsmPasteArgs& p, int n_cases, hipStream_t st) {
  const size_t lds = ((size_t)a.c_out * a.n_strips + a.n_strips + (size_t)a.c_out * a.cp.B + 6 * a.c_out + 8) * sizeof(float);
  const dim3 grid((p.npix + 255) / 256, n_cases);
  if (a.c_out == 1) PSM_LAUNCH((psm_assemble_kernel<1>), grid, dim3(256), lds, st, a, p);
  else PSM_LAUNCH((psm_assemble_kernel<2>), grid, dim3(256), lds, st, a, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// paste
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void psm_paste_kernel(PsmPasteArgs a) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int cs = blockIdx.y;
  if (pix >= a.npix) return;
  const int o = a.owner[pix];
  const int SS = a.S * a.S;
  float* out = a.fields + ((int64_t)cs * a.npix + pix) * a.c_out;
  if (o < 0) {
    for (int f = 0; f < a.c_out; ++f) out[f] = 0.f;
    return;
  }
  const int b = o / SS;
  const float* src = a.pred + ((int64_t)cs * a.B * SS + o) * a.c_out;
  for (int f = 0; f < a.c_out; ++f)
    out[f] = src[f] - a.offs[((int64_t)cs * a.c_out + f) * a.B + b] - a.shift[cs * a.c_out + f];
}

hipError_t psm_launch_paste(const PsmPasteArgs& a, int n_cases, hipStream_t st) {
  PSM_LAUNCH(psm_paste_kernel, dim3((a.npix + 255) / 256, n_cases), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Ring stage-in: the grid of one ticket is pulled from (mapped) pinned host memory by the GPU itself -- 16-byte loads over
// PCIe, enough of them in flight to fill the link -- instead of a DMA-engine copy in front of the kernels: the whole
// ticket is then kernel nodes only (one cheap graph replay, no engine hand-over signals).  The same launch expands the
// per-case out_scale of the ticket (host, pinned) to the per-block-row scale the decode reads.
__global__ __launch_bounds__(256) void psm_stage_in_kernel(const float4* src, float4* dst, size_t n16, const float* tail_src,
                                                           float* tail_dst, int n_tail, const float* scale_host, float* row_scale,
                                                           int n_rows, int B) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  // four independent 16-byte loads per lane and round: 192 workgroups x 256 lanes x 64 B = 3 MiB in flight at most
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const float4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) dst[i] = src[i];
  if (blockIdx.x == 0) {
    for (int t = threadIdx.x; t < n_tail; t += 256) tail_dst[t] = tail_src[t];
    if (scale_host) for (int r = threadIdx.x; r < n_rows; r += 256) row_scale[r] = scale_host[r / B];
  }
}

hipError_t psm_launch_stage_in(const float* src_host, float* dst, size_t n_floats, const float* scale_host, float* row_scale,
                               int n_rows, int B, hipStream_t st) {
  const size_t n16 = n_floats / 4;
  const int n_tail = (int)(n_floats - 4 * n16);
  PSM_LAUNCH(psm_stage_in_kernel, dim3(192), dim3(256), 0, st, reinterpret_cast<const float4*>(src_host), reinterpret_cast<float4*>(dst), n16,
             src_host + 4 * n16, dst + 4 * n16, n_tail, scale_host, row_scale, n_rows, B);
  return hipGetLastError();
}
