// psm_mesh_tables.cpp -- see psm_mesh_tables.h.  Host only.
#include "psm_mesh_tables.h"

#include <algorithm>

// the checks of psm_set_geometry on one case's tables; false: `why` says what is wrong (without naming the case)
static bool psm_mesh_case_valid(const PsmMeshCaseInput& c, int32_t ny, int32_t nx, bool single, std::string& why) {
  if (!c.vtx_m2g || !c.wts_m2g || !c.indices || !c.sdfunct) { why = "null geometry table"; return false; }
  if (single && (c.vtx_g2m == nullptr) != (c.wts_g2m == nullptr)) { why = "vtx_g2m and wts_g2m go together"; return false; }
  if (!single && (!c.vtx_g2m || !c.wts_g2m)) { why = "the grid->mesh tables (vtx_g2m, wts_g2m) are missing"; return false; }
  if (c.n_cells < 1 || c.n_cells > (int64_t)1 << 30) { why = "bad cell count"; return false; }
  const int64_t ng = (int64_t)ny * nx;
  for (int64_t t = 0; t < ng; ++t) {
    for (int j = 0; j < 3; ++j)
      if (c.vtx_m2g[t * 3 + j] < 0 || c.vtx_m2g[t * 3 + j] >= c.n_cells) { why = "mesh->grid vertex index out of range"; return false; }
    if (c.indices[t * 2] < 0 || c.indices[t * 2] >= ny || c.indices[t * 2 + 1] < 0 || c.indices[t * 2 + 1] >= nx) {
      why = "indices outside the grid";
      return false;
    }
  }
  for (int64_t n = 0; c.vtx_g2m && n < c.n_cells; ++n)
    for (int j = 0; j < 3; ++j)
      if (c.vtx_g2m[n * 3 + j] < 0 || c.vtx_g2m[n * 3 + j] >= ng) { why = "grid->mesh vertex index out of range"; return false; }
  return true;
}

int psm_build_mesh_case_tables(int n_cases, const PsmMeshCaseInput* cases, int32_t ny, int32_t nx, double sdf_scale,
                               double wall_threshold, PsmMeshCaseTables& out, std::string& why, bool single) {
  if (n_cases < 1 || !cases || ny < 1 || nx < 1 || (single && n_cases != 1)) { why = "bad case set"; return -1; }
  const int64_t ng = (int64_t)ny * nx;
  for (int k = 0; k < n_cases; ++k) {
    std::string w;
    if (!psm_mesh_case_valid(cases[k], ny, nx, single, w)) { why = single ? w : "case " + std::to_string(k) + ": " + w; return -1; }
  }
  PsmMeshCaseTables t;
  t.n_cases = n_cases; t.n_grid = ng; t.have_g2m = cases[0].vtx_g2m != nullptr;
  t.cell_off.assign((size_t)n_cases + 1, 0);
  for (int k = 0; k < n_cases; ++k) {
    t.cell_off[k + 1] = t.cell_off[k] + cases[k].n_cells;
    t.max_cells = std::max(t.max_cells, cases[k].n_cells);
  }
  t.total = t.cell_off[n_cases];
  const size_t G = (size_t)n_cases * ng, N = (size_t)t.total;
  t.vtx_m2g.resize(G * 3); t.wts_m2g.resize(G * 3); t.src_of_cell.assign(G, -1); t.cell_of_point.resize(G); t.sdf.resize(G);
  t.vtx_g2m.assign(N * 3, 0); t.wts_g2m.assign(N * 3, 0.0); t.near_wall.assign(N, 0); t.sdf_image.assign(G * 3, 0.f);
  for (int k = 0; k < n_cases; ++k) {
    const PsmMeshCaseInput& c = cases[k];
    const size_t g0 = (size_t)k * ng, c0 = (size_t)t.cell_off[k];
    std::copy(c.vtx_m2g, c.vtx_m2g + ng * 3, t.vtx_m2g.begin() + g0 * 3);
    std::copy(c.wts_m2g, c.wts_m2g + ng * 3, t.wts_m2g.begin() + g0 * 3);
    std::copy(c.sdfunct, c.sdfunct + ng, t.sdf.begin() + g0);
    if (t.have_g2m) {
      std::copy(c.vtx_g2m, c.vtx_g2m + c.n_cells * 3, t.vtx_g2m.begin() + c0 * 3);
      std::copy(c.wts_g2m, c.wts_g2m + c.n_cells * 3, t.wts_g2m.begin() + c0 * 3);
    }
    // NumPy fancy assignment grid[...][tuple(indices.T)] = values writes in point order: last wins
    for (int64_t p = 0; p < ng; ++p) {
      const int64_t cell = (int64_t)c.indices[p * 2] * nx + c.indices[p * 2 + 1];
      t.src_of_cell[g0 + cell] = (int32_t)p;
      t.cell_of_point[g0 + p] = (int32_t)cell;
      const double sdv = c.sdfunct[p] * sdf_scale;
      t.sdf_image[(g0 + p) * 3 + 2] = (sdv != sdv) ? 0.f : (float)sdv;
    }
    // sdf_mesh = interpolate_fill(sdfunct.flatten(), vert_NPtoOF, weights_NPtoOF) < threshold  (PM:492-494)
    for (int64_t n = 0; t.have_g2m && n < c.n_cells; ++n) {
      double acc = 0.0; bool neg = false;
      for (int j = 0; j < 3; ++j) { acc += c.sdfunct[c.vtx_g2m[n * 3 + j]] * c.wts_g2m[n * 3 + j]; neg = neg || c.wts_g2m[n * 3 + j] < 0.0; }
      t.near_wall[c0 + n] = (!neg && acc < wall_threshold) ? 1 : 0;     // NaN (fill) compares false
    }
  }
  out = std::move(t);
  return 0;
}
