// psm_mesh.h -- launchers of the mesh <-> grid kernels (see psm_mesh.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct PsmToGridArgs {
  const double* cells;          // [N,5] Ux,Uy,Cx,Cy,p
  const double* umax;           // device scalar, or nullptr: umax_val (computed by the host while the H2D copy runs)
  double umax_val;
  const double* umax_partials;  // large meshes: per-workgroup partial maxima of psm_umax_partial_kernel (reduced here by every
  int n_partials;               // workgroup; workgroup 0 also stores the result to umax_out for psm_to_mesh_kernel), or nullptr
  double* umax_out;
  const int32_t* vtx;           // [n_grid,3] mesh->grid simplices (interp_weights, PM:52-62)
  const double* wts;            // [n_grid,3]
  const int32_t* src_of_cell;   // [n_grid] last grid point scattered into each cell (NumPy fancy assignment order), -1 none
  const double* sdf;            // [n_grid] sdfunct
  float* grid;                  // [n_grid][c_in]
  int64_t n_grid;
  double max_abs_ux, max_abs_uy, sdf_scale;
  int c_in, fill;               // fill: 1 = interpolate_fill (NaN where a weight is negative), 0 = interpolate
};

struct PsmToMeshArgs {
  const double* cells;          // [N,5]
  const double* umax;           // device scalar, or nullptr: umax_val
  double umax_val;
  const int32_t* vtx;           // [N,3] grid->mesh simplices
  const double* wts;            // [N,3]
  const int32_t* cell_of_point; // [n_grid] flat cell index of indices[point]
  const float* field;           // [n_grid][c_out]
  const uint8_t* near_wall;     // [N] interpolated SDF < threshold (PM:492-494), constant per geometry
  double* p_out;                // [N]
  int64_t n_cells;
  double max_abs_p;
  int c_out;
};

hipError_t psm_launch_umax(const double* cells, int64_t n, double* umax, hipStream_t st);
// parallel form for large meshes: partials[0 .. *n_partials) (capacity 256), reduced by psm_to_grid_kernel
hipError_t psm_launch_umax_partial(const double* cells, int64_t n, double* partials, int* n_partials, hipStream_t st);
// registered caller buffers: host cells -> device copy + partial maxima (capacity 256) in one kernel, see psm_mesh.hip
hipError_t psm_launch_stage_cells(const double* host_cells, double* cells, int64_t n, double* partials, int* n_partials, hipStream_t st);
hipError_t psm_launch_to_grid(const PsmToGridArgs& a, hipStream_t st);
hipError_t psm_launch_to_mesh(const PsmToMeshArgs& a, hipStream_t st);
hipError_t psm_launch_interp_to_grid(const double* values, int k, const int32_t* vtx, const double* wts, const int32_t* src_of_cell,
                                     int fill, double* out, int64_t n_grid, hipStream_t st);

// ---- frame-batched, plane-writing form of psm_launch_interp_to_grid (psm_frames_to_grid_device): n_frames arrays of cell columns on
// the single mesh of psm_set_geometry, the frame is launch dimension y, every column goes to a plane of its own.
constexpr int PSM_FRAME_MAX_COLS = 16;
struct PsmFramePlane {
  void* dst;                    // plane of frame 0, nullptr: the column is not stored
  int64_t frame_stride;         // elements of the plane's type from one frame's plane to the next frame's
  int32_t as_f32;               // 0: float64; else float32 by a plain cast (NaN stays NaN)
};
struct PsmFrameArgs {
  const double* cols;           // [n_frames][n_cells][k] row-major, the layout psm_mesh_to_grid takes per frame
  const int32_t* vtx;           // [n_grid,3] mesh->grid simplices, shared by the frames
  const double* wts;            // [n_grid,3]
  const int32_t* src_of_cell;   // [n_grid]
  int64_t n_grid, n_cells;
  int k, fill, n_frames;
  PsmFramePlane out[PSM_FRAME_MAX_COLS];
};
hipError_t psm_launch_frames_to_grid(const PsmFrameArgs& a, hipStream_t st);

// ---- the mesh ends for a case batch (psm_set_geometry_cases): K meshes on one planned grid, the case is launch dimension y.
// Cell-side arrays are the cases' concatenated ([sum n_i, ...], case i at rows cell_off[i] .. cell_off[i + 1]), grid-side tables
// are [K][n_grid, ...]; vertex indices are case-local as the caller gave them (the kernels add the case's offset).
constexpr int PSM_MESH_CASE_PARTS = 256;   // capacity of one case's row of partial maxima (every to_grid workgroup folds a row)
struct PsmMeshCasesArgs {
  const double* cells;          // [sum n_i, 5]
  const int64_t* cell_off;      // [K + 1]
  double* umax_part;            // [K][n_parts] maxima of the SQUARED speed over a fixed partition of the case's cells
  double* umax;                 // [K] written by workgroup 0 of every case in to_grid, read by to_mesh
  int n_parts, n_cases;
  // to_grid
  const int32_t* vtx_m2g;       // [K][n_grid, 3]
  const double* wts_m2g;        // [K][n_grid, 3]
  const int32_t* src_of_cell;   // [K][n_grid]
  const double* sdf;            // [K][n_grid]
  float* grid;                  // [K][n_grid][c_in]
  int64_t n_grid;
  double max_abs_ux, max_abs_uy, sdf_scale;
  int c_in, fill;
  // to_mesh
  const int32_t* vtx_g2m;       // [sum n_i, 3]
  const double* wts_g2m;        // [sum n_i, 3]
  const int32_t* cell_of_point; // [K][n_grid]
  const float* field;           // [K][n_grid][c_out]
  const uint8_t* near_wall;     // [sum n_i]
  double* p_out;                // [sum n_i]
  int64_t max_cells;            // largest n_i: sizes launch dimension x of the two cell-side launches
  double max_abs_p;
  int c_out;
};
hipError_t psm_launch_umax_cases(const PsmMeshCasesArgs& a, hipStream_t st);
hipError_t psm_launch_to_grid_cases(const PsmMeshCasesArgs& a, hipStream_t st);
hipError_t psm_launch_to_mesh_cases(const PsmMeshCasesArgs& a, hipStream_t st);

// ---- Gaussian post-steps (SMD:353-363, UGP:366-367), case-batched: one launch per separable pass, see psm_filter.hip
struct PsmGaussJob {
  const float* in;           // [n_cases][ny][nx][c]
  const float* w;            // [2 * radius + 1] normalised taps
  int radius;
};
struct PsmGaussArgs {
  PsmGaussJob job[2];        // axis 0: n_jobs independent inputs (blockIdx.z); axis 1 with epilogue 1: field (in == nullptr: not filtered) and weighting input
  float* out[2];             // axis 0: one per job; axis 1 without an epilogue: out[0]
  const float* prev;         // epilogues 1 and 2: [n_cases][ny][nx]
  const float* fields;       // epilogue 1 without job 0: the unfiltered field
  float* result; float* t;   // epilogue 1: result (may be nullptr), t = (result - prev) * w
  float* change; float* next;   // epilogue 2: either may be nullptr
  int ny, nx, c, n_cases, n_jobs;
  int tap_chunk;             // taps staged at a time (psm_gauss_tap_chunk of the widest table of the launch)
  int tiles_x;               // set by the launcher
};
void psm_gauss_init();
int psm_gauss_tap_chunk(int max_radius);
// axis 0: along y, no epilogue.  axis 1: along x, epilogue 0 (none), 1 or 2 (c == 1 only)
hipError_t psm_launch_gauss(PsmGaussArgs a, int axis, int epi, hipStream_t st);

// label blocks [B][S*S*c_out] with the per-block flow-cell mean removed (SM_call.py:487-488, UGP:509-511)
hipError_t psm_launch_label_blocks(const float* grid, const float* labels, const int32_t* blk_y0x0, float* out, int B, int S,
                                   int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st);
// compute_in_block_error (utils.py:210-243): per-block partial sums [B][8] doubles, see psm_mesh.hip
hipError_t psm_launch_block_error(const float* grid, const float* pred, const float* label_blocks, const float* row_scale,
                                  const int32_t* blk_y0x0, double* part, int B, int S, int c_in, int c_out, int sdf_ch, int Nx, hipStream_t st);

// ---- the same eight sums for assembled fields (psm_field_errors_device): whole images instead of decoded blocks, several
// (prediction, truth) pairs and frames per call, two launches, no atomics.  Launch 1: grid (workgroups over pixels, pair, frame),
// every workgroup leaves 8 doubles of partials over its PSM_FIELD_ERR_SPAN pixels; launch 2: one workgroup per (pair, frame) folds
// them in a fixed order into raw[n_frames][n_pairs][8].  See psm_mesh.hip.
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

// ---- pressureSM_Poisson input features (SMP:588-711), case-batched: one launch per stage, see psm_features.hip
struct PsmFeatureArgs {
  const double *ux, *uy, *dux, *duy, *sdf;   // case 0: [ny][nx] float64 (dimensional grids, zero outside the flow; raw SDF)
  double* term;                              // [n_cases][ny][nx] scratch: the Poisson source term
  double* partial;                           // [n_cases][2 * workgroups per case] (sum, sum of squares)
  float* grid;                               // [n_cases][ny][nx][4] float32 NHWC
  int ny, nx;
  double L, U, k;                            // L, U: read when lu == nullptr (the host entry's single case)
  double max_abs[4];                         // Poisson_term_1, delta_Ux, delta_Uy, dist
  const double* lu;                          // [n_cases][2] (L, U) per case in device memory: a captured launch reads new values on replay
  int n_cases;                               // launch dimension y; 0 counts as 1
  int64_t vel_stride, sdf_stride;            // doubles from one case's velocity planes / SDF plane to the next case's
};
hipError_t psm_launch_poisson_features(const PsmFeatureArgs& a, hipStream_t st);
