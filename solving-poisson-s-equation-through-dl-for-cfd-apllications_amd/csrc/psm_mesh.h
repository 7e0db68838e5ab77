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

// ---- the delta form of the two ends (psm_solve_delta*: [U(t) - U(t-1)], SDF -> p(t) - p(t-1), pressureSM_deltas/SM_call.py:389-391):
// the same launches on the same tables plus the state u_prev [N][2] = (Ux, Uy) of the previous step, 16-byte aligned.  to_grid
// gathers U - u_prev per vertex; to_mesh stores p(t-1) + dp (p(t-1) where it falls back) and then cells[n][0:2] into u_prev[n].
struct PsmDeltaGridArgs {
  PsmToGridArgs g;
  const double* u_prev;         // [N][2] read at the three vertices of every written image cell
};
struct PsmDeltaMeshArgs {
  PsmToMeshArgs m;
  double* u_prev;               // [N][2] written, one row per thread, after p_out
  int prime;                    // 1: the priming step -- no field is read, p_out = cells[:,4], u_prev = cells[:,0:2]
};
hipError_t psm_launch_to_grid_delta(const PsmDeltaGridArgs& d, hipStream_t st);
hipError_t psm_launch_to_mesh_delta(const PsmDeltaMeshArgs& d, hipStream_t st);

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

// ---- the mesh ends of the Poisson-model step at the solver boundary (psm_solve_poisson*, pressureSM_Poisson/SM_call.py:549-556,
// 815-818, 842-847): three launches around the chain of psm_poisson_step_device on the single mesh of psm_set_geometry.  The state
// is two frames per mesh cell, every row 16-byte aligned: u_prev [N][2] = U of the previous call, du_prev [N][2] = its dU, and
// p_prev [N] = its column 4.  The head (partial maxima, then mesh -> grid) gathers the six columns (Ux, Uy, dUx, dUy, dU-change
// weight, dp_prev) per vertex straight from cells + state; the tail (grid -> mesh) stores p(t-1) + dp and turns the state over.
constexpr int PSM_POISSON_PARTS = 256;     // capacity of one row of partial maxima (every mesh -> grid workgroup folds both rows)
constexpr int PSM_POISSON_SCALARS = 8;     // U, c, U^2, out-scale, skip, frames held before the call, 0, 0
struct PsmPoissonCellsArgs {
  const double* cells;          // [N,5] Ux,Uy,Cx,Cy,p(t-1)
  const double *u_prev, *du_prev, *p_prev;   // the state, read only
  int64_t n_cells;
  double* partials;             // [2][PSM_POISSON_PARTS] maxima of the SQUARED speed and of c_cell = |dUx - du_prev_x| + |dUy - du_prev_y|
  int n_partials;
  // mesh -> grid
  const int32_t* vtx;           // [n_grid,3] mesh->grid simplices
  const double* wts;            // [n_grid,3]
  const int32_t* src_of_cell;   // [n_grid]
  int64_t n_grid;
  double* vel;                  // [4][n_grid] float64 planes (Ux, Uy, dUx, dUy): NaNs of interpolate_fill kept
  float *w_plane, *prev_plane;  // [n_grid] float32 planes of the weight and of dp_prev, NaN -> 0; both nullptr without the weighting
  double* scalars;              // [PSM_POISSON_SCALARS], stored by workgroup 0 ...
  double* lu;                   // ... with (phi, U) for the feature kernels
  float* row_scale;             // ... and the decode's row scale (float)(max_abs_dp * U^2), B rows
  int B;
  double phi, max_abs_dp;
  int weighting, frames;
};
struct PsmPoissonMeshArgs {
  const double* cells;          // [N,5]
  const int32_t* vtx;           // [N,3] grid->mesh simplices
  const double* wts;            // [N,3]
  const int32_t* cell_of_point; // [n_grid]
  const float* field;           // [n_grid] dp on the grid, dimensional (next with the weighting, else result); not read when prime
  const uint8_t* near_wall;     // [N]
  double* p_out;                // [N]
  int64_t n_cells;
  double *u_prev, *du_prev, *p_prev;   // the state, one row each per thread, written after p_out
  double* scalars;              // a step reads [4] (skip) of what the head stored; the push stores all eight
  int prime, frames;            // prime: the push alone, p_out = cells[:,4]; frames held before the call (0: du_prev := 0)
};
hipError_t psm_launch_poisson_partial(const PsmPoissonCellsArgs& a, hipStream_t st);   // a.n_partials: psm_poisson_parts(n_cells)
hipError_t psm_launch_poisson_to_grid(const PsmPoissonCellsArgs& a, hipStream_t st);
hipError_t psm_launch_poisson_to_mesh(const PsmPoissonMeshArgs& a, hipStream_t st);
inline int psm_poisson_parts(int64_t n_cells) { return (int)(n_cells + 1023 < (int64_t)PSM_POISSON_PARTS * 1024 ? (n_cells + 1023) / 1024 : PSM_POISSON_PARTS); }

// ---- the same three launches for a case set (psm_solve_cases_poisson*, psm_set_geometry_cases under a four-channel model): K meshes
// on one planned grid, the case is launch dimension y.  Cell-side arrays -- the cells, the grid -> mesh tables, the state, p -- are the
// cases' concatenated (case i at rows cell_off[i] .. cell_off[i + 1], vertex indices case-local); grid-side tables and planes are
// [K][n_grid, ...] at the strides of the feature and post-step bindings.  A workgroup takes its case's slices and runs the single
// mesh's body on them, so a case's result does not depend on what the other slots hold.
struct PsmPoissonCasesArgs {
  const double* cells;          // [sum n_i, 5]
  const int64_t* cell_off;      // [K + 1]
  int n_cases, n_parts;         // n_parts: psm_poisson_parts(largest n_i), launch dimension x of the partial launch
  int64_t max_cells;            // largest n_i: sizes launch dimension x of the tail
  double *u_prev, *du_prev, *p_prev;   // the state [sum n_i][2] | [sum n_i][2] | [sum n_i]: read by the head, turned over by the tail
  double* partials;             // [K][2][PSM_POISSON_PARTS]; every (part, case) slot below n_parts is written at every step
  // mesh -> grid
  const int32_t* vtx_m2g;       // [K][n_grid, 3]
  const double* wts_m2g;        // [K][n_grid, 3]
  const int32_t* src_of_cell;   // [K][n_grid]
  int64_t n_grid;
  double* vel;                  // [K][4][n_grid]
  float *w_plane, *prev_plane;  // [K][n_grid]; both nullptr without the weighting
  double* scalars;              // [K][PSM_POISSON_SCALARS]
  double* lu;                   // [K][2]
  float* row_scale;             // [K][B]
  int B;
  double phi, max_abs_dp;
  int weighting, frames, prime; // frames held before the call, the same for every case; prime: read by the tail only
  // grid -> mesh
  const int32_t* vtx_g2m;       // [sum n_i, 3]
  const double* wts_g2m;        // [sum n_i, 3]
  const int32_t* cell_of_point; // [K][n_grid]
  const float* field;           // [K][n_grid]; not read when prime
  const uint8_t* near_wall;     // [sum n_i]
  double* p_out;                // [sum n_i]
};
hipError_t psm_launch_poisson_partial_cases(const PsmPoissonCasesArgs& a, hipStream_t st);
hipError_t psm_launch_poisson_to_grid_cases(const PsmPoissonCasesArgs& a, hipStream_t st);
hipError_t psm_launch_poisson_to_mesh_cases(const PsmPoissonCasesArgs& a, hipStream_t st);

// ---- the tail of the gradient-model step at the solver boundary (psm_solve_gradp*, U_to_gradP): grid -> mesh of the integrated
// plane q = p / U^2 [ny][nx] float32 behind the two launches of psm_integ.hip.  The head of that step is psm_solve's own (partial
// maxima, psm_to_grid_kernel), whose U_max the tail reads from the device scalar.  OUTLET: every workgroup first takes the level
// s = mean_y(3 q[y][nx-1] - q[y][nx-2]) / 3 in float64 over all ny rows (python_module.py:472 on the integrated plane) by one fixed
// tree, so every workgroup holds the same bits; NONE: s = 0.0 and nothing is read for it.  Then per mesh cell
// acc = sum_j ((double)q[cell_of_point[vtx[n][j]]] - s) * wts[n][j], p = acc * (U * U), and cells[n][4] where psm_to_mesh_kernel
// falls back (near-wall cell, negative weight, NaN).  Every operation rounds on its own (`fp contract(off)`).
constexpr int PSM_GRADP_LEVEL_NONE = 0, PSM_GRADP_LEVEL_OUTLET = 1;   // PSM_GRADP_REF_* of psm.h
constexpr int PSM_GRADP_SCALARS = 8;       // U, U^2, s, sx, sy, 0, 0, 0
struct PsmGradpMeshArgs {
  const double* cells;          // [N,5]
  const double* umax;           // device scalar: U_max as the head's mesh -> grid launch left it
  const int32_t* vtx;           // [N,3] grid->mesh simplices
  const double* wts;            // [N,3]
  const int32_t* cell_of_point; // [n_grid]
  const float* q;               // [ny][nx] the integrated plane
  const uint8_t* near_wall;     // [N]
  double* p_out;                // [N]
  int64_t n_cells;
  int ny, nx, reference;
  double* scalars;              // [PSM_GRADP_SCALARS], stored by workgroup 0
  double sx, sy;                // the integration's spacings, recorded in the scalars only
};
hipError_t psm_launch_gradp_to_mesh(const PsmGradpMeshArgs& a, hipStream_t st);
// The same launch for a case set: the case is launch dimension y; cell-side arrays concatenated, grid-side [K][n_grid], scalars [K][8].
struct PsmGradpCasesArgs {
  const double* cells;          // [sum n_i, 5]
  const int64_t* cell_off;      // [K + 1]
  const double* umax;           // [K]
  int n_cases;
  int64_t max_cells;            // largest n_i: sizes launch dimension x
  const int32_t* vtx_g2m;       // [sum n_i, 3]
  const double* wts_g2m;        // [sum n_i, 3]
  const int32_t* cell_of_point; // [K][n_grid]
  const float* q;               // [K][ny][nx]
  const uint8_t* near_wall;     // [sum n_i]
  double* p_out;                // [sum n_i]
  int ny, nx, reference;
  double* scalars;              // [K][PSM_GRADP_SCALARS]
  double sx, sy;
};
hipError_t psm_launch_gradp_to_mesh_cases(const PsmGradpCasesArgs& a, hipStream_t st);

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
// the delta form of the case batch's two ends: u_prev [sum n_i][2], the cases' rows concatenated like the cells'
struct PsmDeltaCasesArgs {
  PsmMeshCasesArgs c;
  double* u_prev;
  int prime;                    // as in PsmDeltaMeshArgs; read by to_mesh only
};
hipError_t psm_launch_to_grid_cases_delta(const PsmDeltaCasesArgs& d, hipStream_t st);
hipError_t psm_launch_to_mesh_cases_delta(const PsmDeltaCasesArgs& d, hipStream_t st);
