// psm_integ.h -- launcher of the U_to_gradP integration (see psm_integ.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// ---- U_to_gradP integration (UGP:371-416, 592-628), case-batched and device-resident: see psm_integ.hip
constexpr int PSM_INTEG_MAX_FIX = 4;   // distinct indices the "reset" quirk may touch per row
constexpr int PSM_INTEG_ROWS = 8;      // rows of p one workgroup of the second launch finishes
struct PsmIntegArgs {
  const float* gradp;        // [n_cases][ny][nx][2], 8-byte aligned
  float* p;                  // [n_cases][ny][nx]
  float4* aux;               // [n_cases][ny]: dp/dy at column 0, dp/dy at column nx-1, left row scan at column cx-1, right row scan at column cx-1
  const int2* fixups;        // [n_cases][ny][PSM_INTEG_MAX_FIX] (v, u) by quadrant-local row, v = -1: unused
  const int2* cuts;          // [n_cases] (cy, cx)
  const uint8_t* rowmask;    // [n_cases][ny]: bit 0 = flow cell at column cx (mask2 / mask4), bit 1 = at column cx-1 (mask1 / mask3)
  const int2* npair;         // [n_cases] flow cells per cut column in the (top, bottom) half
  int ny, nx, n_cases;
  float dx, dy;
};
hipError_t psm_launch_integrate(const PsmIntegArgs& a, hipStream_t st);
