// psm_eval.h -- launchers of the evaluator's label / error kernels (see psm_eval.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// label blocks [B][S*S*c_out] with the per-block flow-cell mean removed (SM_call.py:487-488, UGP:509-511)
hipError_t psm_launch_label_blocks(const float* grid, const float* labels, const int32_t* blk_y0x0, float* out, int B, int S,
                                   int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st);
// compute_in_block_error (utils.py:210-243): per-block partial sums [B][8] doubles, see psm_eval.hip
hipError_t psm_launch_block_error(const float* grid, const float* pred, const float* label_blocks, const float* row_scale,
                                  const int32_t* blk_y0x0, double* part, int B, int S, int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st);

// ---- compute_in_block_error for a batch of frames on the device (psm_block_errors_device): the two launches above in one, per
// (block, frame), from the frame's label PLANE -- no label block is stored --, then a fold of every frame's B partial rows in block
// order, as psm_block_error's host loop adds them.  c_out == 1.  See psm_eval.hip.
struct PsmBlockErrorBatchArgs {
  const float* grid;            // [n_frames][npix][c_in] the solve's image (flow cell: its SDF channel != 0)
  const float* label;           // [n_frames][npix] label plane in the network's normalised output units
  const float* pred;            // [n_frames * B][S*S] decoded blocks
  const float* row_scale;       // [n_frames * B]
  const int32_t* blk_y0x0;      // [B][2]
  double* part;                 // [n_frames][B][8]
  int64_t npix;
  int S, c_in, sdf_ch, Nx, B, n_frames;
};
struct PsmBlockErrorFoldArgs {
  const double* part;           // [n_frames][B][8]
  const double* field_raw;      // [n_frames][8] sums of the assembled field, copied to row 0 of the frame (nullptr: raw holds the block row alone)
  double* raw;                  // field_raw ? [n_frames][2][8] : [n_frames][8]
  int B;
};
hipError_t psm_launch_block_error_batch(const PsmBlockErrorBatchArgs& a, hipStream_t st);
hipError_t psm_launch_block_error_fold(const PsmBlockErrorFoldArgs& a, int n_frames, hipStream_t st);

// ---- the same eight sums for assembled fields (psm_field_errors_device): whole images instead of decoded blocks, several
// (prediction, truth) pairs and frames per call, two launches, no atomics.  Launch 1: grid (workgroups over pixels, pair, frame),
// every workgroup leaves 8 doubles of partials over its PSM_FIELD_ERR_SPAN pixels; launch 2: one workgroup per (pair, frame) folds
// them in a fixed order into raw[n_frames][n_pairs][8].  See psm_eval.hip.
constexpr int PSM_FIELD_ERR_MAX_PAIRS = 4;
constexpr int PSM_FIELD_ERR_SPAN = 2048;   // pixels per workgroup of launch 1: 256 threads x 2 rounds x 4 consecutive pixels
inline int psm_field_error_workgroups(int64_t npix) { return (int)((npix + PSM_FIELD_ERR_SPAN - 1) / PSM_FIELD_ERR_SPAN); }
struct PsmErrPlane {
  const void* ptr;              // pixel 0 of frame 0; nullptr: the plane is absent (add / sub: counts as 0)
  int64_t frame_stride;         // elements of the plane's type from one frame to the next
  int64_t elem_stride;          // elements from one pixel to the next (1: a dense plane, read with 16-byte loads where aligned)
  int32_t as_f32;               // 0: float64; else float32, widened exactly
};
struct PsmFieldErrorPair {
  PsmErrPlane pred, truth, add, sub;   // pred_eff = (nan0(add) - nan0(sub)) + pred;  d = pred_eff - truth
  int32_t truth_nan_to_zero;    // truth = nan0(truth) (np.nan_to_num of the label plane); else a NaN truth on a flow cell counts in tnan
};
struct PsmFieldErrorArgs {
  PsmErrPlane mask;             // flow cell iff mask != 0 && mask == mask (a NaN SDF is no flow: nan_to_num(sdfunct) / max_abs_dist == 0)
  PsmFieldErrorPair pair[PSM_FIELD_ERR_MAX_PAIRS];
  int64_t npix;
  int n_pairs, n_frames, n_wg;  // n_wg = psm_field_error_workgroups(npix)
  double* part;                 // [n_frames][n_pairs][n_wg][8]
};
struct PsmFieldErrorFinalArgs {
  const double* part;
  double* raw;                  // [n_frames][n_pairs][8]
  int n_wg;
};
hipError_t psm_launch_field_errors(const PsmFieldErrorArgs& a, hipStream_t st);
hipError_t psm_launch_field_errors_final(const PsmFieldErrorFinalArgs& a, int n_pairs, int n_frames, hipStream_t st);
