// psm_devutil.h -- device-side helpers shared by the PCA-path kernel files (psm_encode / psm_dense / psm_decode / psm_assemble /
// psm_bound / psm_bf16 .hip).  Every function here is __device__ __forceinline__: what a kernel inlines does not depend on what
// else its translation unit holds, so a kernel compiles to the same code in whichever file it lives.
#pragma once
#include <cstdint>

#include "psm_kernels.h"

// One scalar load from every 64-byte line of the kernel-argument segment, all requested together at the top of a kernel.  hipcc
// fetches arguments lazily, in the basic block that first needs them: a kernel with 250-300 bytes of arguments (two argument
// structs) took three or four scalar-cache MISSES one after the other on its way to its first vector load (decode + paste: 1.9 us
// from entry to "all requests issued", 1.6 us with the lines warmed by one batch -- the later loads hit).  The convolution kernels
// (one argument struct, A/B on one box: 145.0 / 144.1 against 144.7 / 146.1 us per pass) do not use it.
// (-DPSM_NO_WARM_KERNARGS: diagnostic build without it, for A/B runs on one box.)
template <int BYTES>
__device__ __forceinline__ void psm_warm_kernargs() {
#ifdef PSM_NO_WARM_KERNARGS
  return;
#endif
  typedef const __attribute__((address_space(4))) int* kptr;
  kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
  int v[(BYTES + 63) / 64];
#pragma unroll
  for (int o = 0; o < (BYTES + 63) / 64; ++o) v[o] = ka[16 * o];
#pragma unroll
  for (int o = 0; o < (BYTES + 63) / 64; ++o) asm volatile("" ::"s"(v[o]));
}

// A wave-uniform element of a read-only table that was written before the launch (block-row offsets, descriptors): through the
// scalar cache (constant address space: s_load, its own wait counter) instead of a wave-wide vector load of one value -- hipcc
// cannot prove a kernel-argument pointer read-only and takes the vector path on its own (round 6: the encode kernels' sixteen
// row-offset lookups were sixteen 64-lane loads and a vector-memory round trip in front of the rows and the basis stream).
__device__ __forceinline__ long long psm_row_base(const int64_t* table, int m) {
  typedef const __attribute__((address_space(4))) long long* ktab;
  return ((ktab)(uintptr_t)table)[__builtin_amdgcn_readfirstlane(m)];
}

// Predicated 4-byte store without a branch: through a raw buffer descriptor over the whole destination, a lane that must not write
// gets the offset 0xffffffff, which the hardware's range check drops (round 6: the paste epilogues were sixteen s_and_saveexec /
// branch / 64-bit address / store sequences per row chunk -- half the instructions of a chunk of the batch decode).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t psm_store_rsrc(float* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
__device__ __forceinline__ void psm_store_if(__amdgpu_buffer_rsrc_t r, uint32_t elem, bool on, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, on ? elem * 4u : 0xffffffffu, 0, 0);
}

// streamed-once operands (PCA bases): -DPSM_NT_STREAM selects non-temporal loads (so that the 42 MB of basis data per
// solve do not displace the small tables and dense weights from the L2s).  Measured on MI355X: SLOWER, 44.1 vs
// 41.9 us per solve -- back-to-back solves re-read the bases from L2 / Infinity Cache, which nt gives up.  Off.
#ifdef PSM_NT_STREAM
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 stream_load(const float4* p) {
  const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
#else
__device__ __forceinline__ float4 stream_load(const float4* p) { return *p; }
#endif

// 64-lane sum on the VALU (DPP row shifts + row broadcasts, ~6 instructions) instead of
// __shfl_down, which lowers to ds_bpermute (an LDS round trip per step).  Every lane must be
// active; the total is returned in all lanes (readlane 63).
__device__ __forceinline__ float wave_sum(float v) {
#define PSM_DPP_ADD(ctrl, rmask)                                                                             \
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, true))
  PSM_DPP_ADD(0x111, 0xf);   // row_shr:1
  PSM_DPP_ADD(0x112, 0xf);   // row_shr:2
  PSM_DPP_ADD(0x114, 0xf);   // row_shr:4
  PSM_DPP_ADD(0x118, 0xf);   // row_shr:8  -> lane 15 of each row of 16 holds the row total
  PSM_DPP_ADD(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  PSM_DPP_ADD(0x143, 0xc);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave total
#undef PSM_DPP_ADD
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// A loaded value whose FIRST use would sit inside run-time predicated store blocks is consumed once before them, through an opaque
// move.  The wait-count pass cannot count the stores in flight behind run-time predicates, so with a load still pending at their
// first use it emits s_waitcnt vmcnt(0) in front of EVERY store: sixteen store round trips in series per epilogue (the decode
// kernels' `mean` value; tools/attic/isa_store_waits.py finds the pattern in a listing).
__device__ __forceinline__ float psm_settled(float v) {
  float r;
  asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "v"(v));
  return r;
}

// Workgroup barrier that only drains LDS traffic: __syncthreads() also waits for every outstanding
// global load (vmcnt(0)), which would serialise the gathers of psm_assemble_kernel with its chain.
#define PSM_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// ---- geometry guard and strip-dot riders (Dense head, psm_res_dots_kernel, both decode + paste kernels) ----
constexpr int PSM_DOTS_WG_ROWS = 256;   // closed-form dots: up to this many rows one workgroup per row, beyond it two rows per workgroup
// One guard wave (PsmGuardArgs): 8 ballots of 64 consecutive pixels each against the bound pattern.
__device__ __forceinline__ bool psm_guard_wave(const PsmGuardArgs& g, int gw, int lane) {
  constexpr int NB = PSM_GUARD_BALLOTS;
  float v[NB];
  unsigned long long want[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) {                       // all loads up front, clamped
    const long long pix = min((long long)(gw * NB + u) * 64 + lane, g.npix - 1);
    v[u] = g.sdf[pix * g.c_in];
    want[u] = g.bits[min(gw * NB + u, g.n_ballots - 1)];
  }
  bool bad = false;
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const unsigned long long got = __ballot(v[u] != 0.f);           // NaN != 0 is true, like NumPy's `!= 0`
    bad |= (gw * NB + u < g.n_ballots) && got != want[u];
  }
  if (g.sdf_ref) {                                     // uniform.  SDF fold: the bound VALUES (the pixels of the clamped tail compare a pixel with itself)
    float ref[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) ref[u] = g.sdf_ref[min((long long)(gw * NB + u) * 64 + lane, g.npix - 1)];
#pragma unroll
    for (int u = 0; u < NB; ++u) bad |= __ballot(!(v[u] == ref[u])) != 0ull;      // NaN == x is false: a mismatch
  }
  return bad;                                          // wave-uniform
}
// One guard workgroup (index gwg of this launch's range, uniform): PSM_GUARD_WG_WAVES guard waves' worth of pixels by the WAVES
// waves of the calling workgroup, one flag.  Every thread of the workgroup must call it (barriers).
template <int WAVES>
__device__ __forceinline__ void psm_guard_wg(const PsmGuardArgs& g, int gwg, int wave, int lane) {
  __shared__ int guard_bad[WAVES];
  if (gwg >= g.wg_count) return;                       // uniform
  const int wg = g.wg_first + gwg;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < PSM_GUARD_WG_WAVES / WAVES; ++k) {
    const int gw = wg * PSM_GUARD_WG_WAVES + wave * (PSM_GUARD_WG_WAVES / WAVES) + k;
    if (gw < g.n_waves) bad |= psm_guard_wave(g, gw, lane);
  }
  if (lane == 0) guard_bad[wave] = bad ? 1 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) any |= guard_bad[w];
    g.flags[wg] = any ? __int_as_float(0x7fc00000) : 0.f;
    if (any && g.host_flag) __hip_atomic_store(g.host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// sum of the guard flags of a solve (0, or NaN after a mismatch): one wave, every lane gets the total
__device__ __forceinline__ float psm_guard_part(const float* flags, int n, int lane, int first) {   // this lane's share from `first` on
  float gs = 0.f;
  for (int k0 = first + lane; k0 < n; k0 += 64 * 8) {  // 8 independent loads per round
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = flags[min(k0 + 64 * u, n - 1)];
#pragma unroll
    for (int u = 0; u < 8; ++u) gs += (k0 + 64 * u < n) ? v[u] : 0.f;
  }
  return gs;
}
__device__ __forceinline__ float psm_guard_sum(const float* flags, int n, int lane, float f0, float f1) {
  const float gs = (lane < n ? f0 : 0.f) + (lane + 64 < n ? f1 : 0.f) + psm_guard_part(flags, n, lane, 128);
  return wave_sum(gs);
}

// ---- offset chain (psm_chain_kernel, psm_assemble_kernel, psm_decode_paste_kernel, psm_chain_dots_kernel) ----
// Row-parallel form of the offset chain (one wave per field, lane = position of the block
// in its row).  Blocks of one row only depend on each other through the value handed from the
// previously enumerated block (c_prev in SMD/UGP, BC_ant_0 / BC_alter in PM); inside a row
// that hand-over is needed by the whole first row and, elsewhere, only by blocks whose
// BC_ups entry is NaN.  So every row is evaluated lane-parallel from the block above
// (BC_ups is lane-local), followed by an in-order fix-up loop over just the lanes that need
// the hand-over -- the same arithmetic, in the same order, as the serial recurrence
// (psm_chain_v in psm_plan.h, which stays the host replay and the fallback for > 64 columns).
template <int VARIANT>
__device__ __forceinline__ void psm_chain_rows(const PsmChainParams& P, const float* smean, const float* scnt,
                                               const PsmBlock* blk, int field, int lane, float* offs_out) {
  const int n_x = P.n_x, n_y = P.n_y;
  const int ncol = (VARIANT == PSMV_CHAPTER5) ? n_x + 2 : n_x + 1;
  const int nrow = n_y + 2;
  const bool act = lane < ncol;
  const int l = act ? lane : 0;
  int tj;
  if (VARIANT == PSMV_GRADP) tj = l;
  else if (VARIANT == PSMV_DELTAS) tj = n_x - l;
  else tj = (l <= n_x) ? n_x - l : -1;
  const float ref = P.ref_bc;
  float first_col = NAN;                                      // UGP:294-300
  if (VARIANT == PSMV_GRADP && field == 0)
    for (int c = 0; c < 128; ++c)
      if (scnt[P.col_base + c] > 0.f) { first_col = smean[P.col_base + c]; break; }
  float up = (VARIANT == PSMV_CHAPTER5 && tj == -1) ? NAN : 0.f;   // BC_ups[tj] / BC_up_
  float carry = (VARIANT == PSMV_CHAPTER5) ? NAN : 0.f;             // c_prev | BC_ant_0 / BC_alter
  auto rl = [](float v, int q) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), q)); };
  // The strip means of a row's blocks do not depend on the chain: all C_NS of them (plus one
  // count) are read a row ahead, unconditionally, so that the recurrence itself runs on registers.
  constexpr int NSV = (VARIANT == PSMV_DELTAS) ? (int)D_NS : (VARIANT == PSMV_GRADP ? (int)G_NS : (int)C_NS);   // == P.NS
  const int bmax = nrow * ncol - 1;
  auto fetch = [&](float (&M)[NSV], float& cnt_up, int r) {
    const float* mp = smean + min(r * ncol + l, bmax) * NSV;
#pragma unroll
    for (int s = 0; s < NSV; ++s) M[s] = mp[s];
    cnt_up = (VARIANT == PSMV_DELTAS) ? scnt[min(r * ncol + l, bmax) * NSV + D_ROWS_UP] : 0.f;
  };
  float M[NSV], cnt_up;
  fetch(M, cnt_up, 0);
  for (int r = 0; r < nrow; ++r) {
    float Mn[NSV], cnt_up_n;
    fetch(Mn, cnt_up_n, r + 1);                               // clamped on the last row
    const int b = r * ncol + l;
    const bool first = (r == 0), last = (r == n_y + 1);
    if (last && P.skip_last) {                                // duplicate last row left out (uniform)
      if (act) offs_out[b] = NAN;
      continue;
    }
    const float* mp = M;
    const bool unan = (up != up);
    float A, Bm = 0.f, L = 0.f, c;
    bool need;
    if (VARIANT == PSMV_DELTAS) {
      const bool lim = (tj == 0);
      A = lim ? mp[D_CUR_R_LIM] : mp[D_CUR_R_OV];
      Bm = lim ? mp[D_PREV_L_LIM] : mp[D_PREV_L_OV];
      if (first) { c = mp[D_COL_LAST] - ref; need = (lane != 0); }
      else if (!last) { c = mp[D_TOP] - up; need = unan && !(tj != 0 && tj == n_x); }
      else {
        const bool use_side = cnt_up / 16384.f > 0.9f;         // SMD:307
        c = (tj == n_x) ? mp[D_ROWS_UP] - up : mp[D_ROWS_HEAD] - up;
        need = (tj != n_x) && use_side;
      }
    } else if (VARIANT == PSMV_GRADP) {
      const bool lim = (tj == n_x);
      A = lim ? mp[G_CUR_L_LIM] : mp[G_CUR_L_OV];
      Bm = lim ? mp[G_PREV_R_LIM] : mp[G_PREV_R_OV];
      if (first) { c = (field == 0 ? first_col : mp[G_ROW1]) - ref; need = (lane != 0); }
      else { c = (last ? mp[G_ROWS_UP] : mp[G_TOP]) - up; need = unan; }
    } else {
      const bool m1 = (tj == -1), nx = (tj == n_x);
      A = (first && m1) ? mp[C_COLS_C] : mp[C_COLS_R];
      L = mp[C_COLS_0];
      if (first) { c = mp[C_COLS_R] - 0.f; need = !nx; }
      else if (!last) { c = (m1 ? mp[C_TOPC] : mp[C_TOP]) - up; need = !m1 && unan; }
      else { c = (m1 ? mp[C_TC] : mp[C_ROWS_T]) - up; need = !m1 && unan; }
    }
    unsigned long long todo = __ballot(need && act);
    while (todo) {                                            // in enumeration order
      const int q = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const float out_prev = (VARIANT == PSMV_CHAPTER5) ? L - c : c;
      const float cin = (q == 0) ? carry : rl(out_prev, q > 0 ? q - 1 : 0);
      const float cnew = (VARIANT == PSMV_CHAPTER5) ? A - cin : A - (Bm - cin);
      c = (lane == q) ? cnew : c;
    }
    carry = rl((VARIANT == PSMV_CHAPTER5) ? L - c : c, ncol - 1);
    if (VARIANT == PSMV_DELTAS) {
      if (!last) up = ((!first && r == n_y) ? mp[D_ROWS_PI] : mp[D_BOTTOM]) - c;
    } else if (VARIANT == PSMV_GRADP) {
      if (!last) up = ((!first && r == n_y) ? mp[G_ROWS_PI] : mp[G_BOTTOM]) - c;
    } else {
      const bool m1 = (tj == -1), nx = (tj == n_x);
      if (first) up = (nx ? mp[C_RR] : (m1 ? mp[C_RC] : mp[C_ROWS_R])) - c;
      else if (!last) up = (m1 ? mp[C_RC_UNMASKED] : mp[C_ROWS_R]) - c;
    }
    if (act) offs_out[b] = c;
#pragma unroll
    for (int s = 0; s < NSV; ++s) M[s] = Mn[s];
    cnt_up = cnt_up_n;
  }
}

__device__ __forceinline__ void psm_chain_wave(const PsmChainParams& P, const float* smean, const float* scnt,
                                               const PsmBlock* blk, int field, int lane, float* offs_out) {
  if (P.variant == PSMV_DELTAS) psm_chain_rows<PSMV_DELTAS>(P, smean, scnt, blk, field, lane, offs_out);
  else if (P.variant == PSMV_GRADP) psm_chain_rows<PSMV_GRADP>(P, smean, scnt, blk, field, lane, offs_out);
  else psm_chain_rows<PSMV_CHAPTER5>(P, smean, scnt, blk, field, lane, offs_out);
}
