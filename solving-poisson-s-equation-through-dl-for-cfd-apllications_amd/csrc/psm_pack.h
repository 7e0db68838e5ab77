// psm_pack.h -- launchers of the evaluators' image packs (see psm_pack.hip): between the frame form of the mesh -> grid launch
// (psm_launch_frames_to_grid, psm_mesh.h) and the solve.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int PSM_DELTAS_PACK_SPAN = 1024;   // pixels per workgroup of every pack: 256 threads x 4 consecutive pixels

// ---- the image pack of the deltas evaluator's frame batch (psm_deltas_image_device): the float64 planes the frame launch leaves for
// columns 0-2 (dUx / U, dUy / U, dp / U^2; NaNs of interpolate_fill kept) -> the solve's image, the label plane and the truth plane,
// the statements of pressureSM_deltas/SM_call.py:439-445 and :580 per pixel.  One launch, the frame is launch dimension y.
struct PsmDeltasPackArgs {
  const double* planes;         // [n_frames][3][npix]
  const double* sdn;            // [npix] nan0(sdfunct) / max_abs_dist of the simulation, shared by the frames (float64, made at bind)
  const double* u2;             // [n_frames] U_max_norm^2 of the frame (read only with truth)
  float* grid;                  // [n_frames][npix][3] = (float)(nan0(v) / max_abs) per channel, channel 2 = (float)sdn
  float* label;                 // [n_frames][npix]    = (float)(nan0(v2) / max_abs_p); nullptr: not stored
  double* truth;                // [n_frames][npix]    = (nan0(v2) / max_abs_p) * max_abs_p * u2[f], left to right; nullptr: not stored
  int64_t npix;
  double max_abs_ux, max_abs_uy, max_abs_p;
  int n_frames;
};
hipError_t psm_launch_deltas_pack(const PsmDeltasPackArgs& a, hipStream_t st);

// ---- the image / label pack of the U_to_gradP evaluator's frame batch (psm_gradp_image_device): the float64 planes of columns 0-4
// (Ux / U, Uy / U, dPdx (max_x - min_x) / U^2, dPdy (max_y - min_y) / U^2, p / U^2; NaNs of interpolate_fill kept) -> the solve's
// image and the three float64 label planes, the statements of Eval_dual_Dense_onlycil.py:461-467 per pixel.  One launch, the frame
// is launch dimension y; 48 bytes in and 36 out per pixel (60 with the labels).
struct PsmGradpPackArgs {
  const double* planes;         // [n_frames][5][npix]
  const double* sdn;            // [npix] nan0(sdfunct) / max_abs[2] of the simulation, shared by the frames (float64, made at bind)
  float* grid;                  // [n_frames][npix][3] = ((float)(nan0(v0) / m0), (float)(nan0(v1) / m1), (float)sdn)
  double* truth;                // [n_frames][3][npix] = (nan0(v2) / m3, nan0(v3) / m4, nan0(v4)): grid channels 3-5; nullptr: not stored
  int64_t npix;
  double m0, m1, m3, m4;        // max_abs of channels 0, 1, 3, 4; the pressure label (channel 5) is not divided
  int n_frames;
};
hipError_t psm_launch_gradp_pack(const PsmGradpPackArgs& a, hipStream_t st);

// ---- the image / label pack of the Chapter-4 evaluators' frame batch (psm_chapter4_image_device): the float64 planes of columns
// 0 .. c_in - 1 (M_u: Ux / U, Uy / U, p / U^2; M_fU: f(U) / U^2, p / U^2; NaNs of interpolate_fill kept) -> the solve's c_in-channel
// image and the float64 truth plane, the statements of Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py:215-225 (M_fU/Evaluation/
// Eval.py:213-223) per pixel.  One launch, the frame is launch dimension y; (c_in + 1) * 8 bytes in and c_in * 4 + 8 out per pixel.
struct PsmChapter4PackArgs {
  const double* planes;         // [n_frames][c_in][npix]: the c_in - 1 input channels, then the pressure label
  const double* sdn;            // [npix] nan0(sdfunct) / max_abs_dist of the simulation, shared by the frames (float64, made at bind)
  float* grid;                  // [n_frames][npix][c_in] = ((float)(nan0(v_c) / m[c]) for c < c_in - 1, (float)sdn)
  double* truth;                // [n_frames][npix] = nan0(v_label) / m_p; nullptr: not stored
  int64_t npix;
  double m[2], m_p;             // max_abs of the input channels (m[1] is not read at c_in == 2) and of the pressure
  int c_in, n_frames;           // c_in: 2 or 3, the image width
};
hipError_t psm_launch_chapter4_pack(const PsmChapter4PackArgs& a, hipStream_t st);
