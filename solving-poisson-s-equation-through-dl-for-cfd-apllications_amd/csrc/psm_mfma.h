// psm_mfma.h -- matrix-instruction vocabulary of the PCA-path kernel files (psm_encode / psm_dense / psm_decode / psm_assemble /
// psm_bound / psm_bf16 .hip): vector types, the MFMA builtins under short names, and the exact three-way bf16 split of "x6".
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_32x32x2_f32 (exact f32 fma chain).  Operand maps (wave64):
//   A: lane l holds A[i = l&31][k = l>>5];  B: lane l holds B[k = l>>5][j = l&31]
//   D: lane l, reg r holds D[(r&3) + 8*(r>>2) + 4*(l>>5)][l&31]
// The K order inside a group of 8 is permuted (step j of group g uses k = 8g + 4h + j for
// lane half h) so that one 16-byte read per lane feeds four MFMAs; both operands use it.
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
// v_mfma_f32_16x16x4_f32: operand maps with the Dense kernel (psm_dense.hip)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// v_mfma_f32_32x32x16_bf16 (wave64): lane l (r = l&31, h = l>>5) holds A[r][8h+j] and B[8h+j][r], j = 0..7 (one 16-byte
// register group each); D as for the f32 32x32 form.  Operands rounded to bf16 (psm_bf16.hip) or split exactly (x6, below).
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// row of the 32x32 accumulator tile that register `reg` of lane half `half` holds (the D map above)
__device__ __forceinline__ int acc_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// "x6" arithmetic: a float32 contraction on the bf16 matrix pipe at float32 accuracy (psm_encode_x6_kernel in psm_encode.hip has
// the full account).  Every float32 operand is split EXACTLY into three bf16 terms, x = hi + mid + lo (8 + 8 + 8 significant
// bits: the two remainders x - hi and (x - hi) - mid are exact in float32); a product is taken as the six terms hh, hm, mh, hl,
// lh, mm.  k order inside a 16-step: lane half h holds k = 16 s + 4 h + (0..3) and 16 s + 8 + 4 h + (0..3) in both operands.
__device__ __forceinline__ void psm_split3(f32x4 x, bf16x4& h, bf16x4& m, bf16x4& l) {
  h = __builtin_convertvector(x, bf16x4);                          // round to nearest even
  const f32x4 r1 = x - __builtin_convertvector(h, f32x4);          // exact
  m = __builtin_convertvector(r1, bf16x4);
  const f32x4 r2 = r1 - __builtin_convertvector(m, f32x4);         // exact, <= 8 significant bits
  l = __builtin_convertvector(r2, bf16x4);
}
__device__ __forceinline__ bf16x8 psm_cat4(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
// LDS image of x6 activation planes read as ONE ds_read_b128 per MFMA operand: rows a multiple of 16 bytes (an odd number of 16-byte slots),
// the four 4-element groups of every 16 k stored 0, 2, 1, 3 (lane half h holds k 4h.. and 8 + 4h..).  Position (bf16) of 4-element group q:
__device__ __forceinline__ int psm_x6_group_pos(int q) { const int g = q & 3; return 16 * (q >> 2) + 4 * (g == 1 ? 2 : (g == 2 ? 1 : g)); }
