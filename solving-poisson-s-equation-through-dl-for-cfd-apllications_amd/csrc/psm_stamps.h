// psm_stamps.h -- diagnostic stamps (100 MHz wall clock) of the PCA-path kernels: compiled only with -DPSM_STAMPS (make stamps),
// never in the shipped library, where every macro below is empty.  The slots are ONE __device__ array that kernels of several
// stage files write and psm_read_stamps reads; separate translation units cannot share a device global without relocatable
// device code, so the stamps build compiles the stage files as one unit (psm_stamps.hip includes them) and the shipped build
// never defines the array.
#pragma once
#ifdef PSM_STAMPS
__device__ unsigned long long g_psm_stamps[64];
#endif
#if defined(PSM_STAMPS) && !defined(PSM_STAMPS_ENC)      // -DPSM_STAMPS_ENC: all 64 slots belong to psm_encode_x6_mt_kernel (ESTAMP below)
#define PSM_STAMP(buf, k) do { if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) g_psm_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PSM_STAMP_T(tid_, k) do { if (blockIdx.x == 0 && threadIdx.x == (tid_) && (k) < 64) g_psm_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define DSTAMP(k) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && (k) < 40) g_psm_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)   // psm_decode_paste_batch_kernel
#else
#define PSM_STAMP(buf, k) do { } while (0)
#define PSM_STAMP_T(tid_, k) do { } while (0)
#define DSTAMP(k) do { } while (0)
#endif
#if defined(PSM_STAMPS) && defined(PSM_STAMPS_ENC)      // make stamps EXTRA=-DPSM_STAMPS_ENC: psm_encode_x6_mt_kernel's stamps instead of the decode's (tools/attic/encode_stamps.py)
#define ESTAMP(k) do { if (blockIdx.x == 0 && threadIdx.x == (PSM_STAMPS_ENC) && (k) < 64) g_psm_stamps[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ESTAMP(k) do { } while (0)
#endif
