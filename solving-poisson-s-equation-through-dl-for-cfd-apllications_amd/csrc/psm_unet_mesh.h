// psm_unet_mesh.h -- launchers of the mesh ends of the convolutional path (psm_unet_mesh.hip): K meshes <-> the U-Net's canvas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// One step of psm_unet_solve*: the layout of PsmMeshCasesArgs (psm_mesh.h) -- cell-side arrays concatenated with cell_off, grid-side
// tables [K][ny * nx, ...], vertex indices case-local, the case is launch dimension y -- with the image at CANVAS pitch: the network
// runs on (ny_c, nx_c) = (ny, nx) rounded up to multiples of 2^(levels - 1), the image sits in rows [0, ny) and columns [0, nx) of
// its case's canvas, and every other canvas pixel is +0.0 from bind time on (no kernel here writes one).
struct PsmUnetMeshArgs {
  const double* cells;          // [sum n_i, 5]
  const int64_t* cell_off;      // [K + 1]
  double* umax_part;            // [K][n_parts] maxima of the SQUARED speed (psm_launch_umax_cases)
  double* umax;                 // [K] written by workgroup 0 of every case in to_canvas, read by to_mesh
  int n_parts, n_cases;
  // mesh -> canvas
  const int32_t* vtx_m2g;       // [K][ny * nx, 3]
  const double* wts_m2g;        // [K][ny * nx, 3]
  const int32_t* src_of_cell;   // [K][ny * nx]
  const double* sdf;            // [K][ny * nx]
  float* canvas;                // [K][ny_c][nx_c][3]
  int ny, nx, ny_c, nx_c;
  double max_abs_ux, max_abs_uy, sdf_scale;
  int fill;
  // canvas -> mesh
  const int32_t* vtx_g2m;       // [sum n_i, 3]
  const double* wts_g2m;        // [sum n_i, 3]
  const int32_t* pixel_of_point;// [K][ny * nx]: cell_of_point at canvas pitch, ii * nx_c + jj (re-pitched on the host at bind time)
  const float* field;           // [K][ny_c][nx_c]; not read when prime
  const uint8_t* near_wall;     // [sum n_i]
  double* p_out;                // [sum n_i]
  int64_t max_cells;            // largest n_i: sizes launch dimension x of the tail
  double max_abs_p;
  // the delta step (null / 0 for the absolute one)
  double* u_prev;               // [sum n_i][2], 16-byte aligned: read by to_canvas, turned over by to_mesh
  int prime;                    // 1: the priming step -- the tail alone, p_out = cells[:,4], u_prev = cells[:,0:2]
};
hipError_t psm_launch_unet_to_canvas(const PsmUnetMeshArgs& a, bool delta, hipStream_t st);
hipError_t psm_launch_unet_to_mesh(const PsmUnetMeshArgs& a, bool delta, hipStream_t st);
