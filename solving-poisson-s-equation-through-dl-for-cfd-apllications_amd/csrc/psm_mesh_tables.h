// psm_mesh_tables.h -- host side of psm_set_geometry (one mesh) and psm_set_geometry_cases: validation of the K caller tables, the case offsets and the derived
// tables (last writer per image cell, near-wall flags, the SDF channel as the kernels write it), concatenated in the layout of
// PsmMeshCasesArgs (psm_mesh.h).  Pure host code without HIP: tests/native/mesh_cases_sanitized.cpp runs it under ASan / UBSan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct PsmMeshCaseInput {          // the tables of psm_set_geometry, per case
  int64_t n_cells;
  const int32_t* vtx_m2g;          // [ny*nx, 3]
  const double* wts_m2g;           // [ny*nx, 3]
  const int32_t* indices;          // [ny*nx, 2]
  const double* sdfunct;           // [ny*nx]
  const int32_t* vtx_g2m;          // [n_cells, 3]   the single mesh may come without this pair: both null
  const double* wts_g2m;           // [n_cells, 3]
};

struct PsmMeshCaseTables {
  int n_cases = 0;
  bool have_g2m = true;                                           // false: the single mesh came without grid->mesh tables (zero-filled, near_wall all 0)
  int64_t n_grid = 0, total = 0, max_cells = 0;
  std::vector<int64_t> cell_off;                                  // [K + 1]
  std::vector<int32_t> vtx_m2g, src_of_cell, cell_of_point;       // [K][n_grid, 3], [K][n_grid], [K][n_grid]
  std::vector<double> wts_m2g, sdf;                               // [K][n_grid, 3], [K][n_grid]
  std::vector<int32_t> vtx_g2m;                                   // [total, 3]
  std::vector<double> wts_g2m;                                    // [total, 3]
  std::vector<uint8_t> near_wall;                                 // [total]
  std::vector<float> sdf_image;                                   // [K][n_grid][3]: channels 0, 1 zero, channel 2 as psm_to_grid*_kernel writes it
};

// All-or-nothing: validates every case with the checks of psm_set_geometry and only then fills `out`.  A case set requires the
// grid->mesh tables and names the first bad case ("case k: ..."); `single` (n_cases == 1, psm_set_geometry) takes a mesh without
// them and names no case.  0, or PSM_ERR_ARG (-1).
int psm_build_mesh_case_tables(int n_cases, const PsmMeshCaseInput* cases, int32_t ny, int32_t nx, double sdf_scale,
                               double wall_threshold, PsmMeshCaseTables& out, std::string& why, bool single = false);
