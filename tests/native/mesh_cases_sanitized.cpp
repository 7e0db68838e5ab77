// CPU-only check of the host side of psm_set_geometry_cases (csrc/psm_mesh_tables.cpp) under AddressSanitizer + UBSan:
// random case sets of unequal cell counts on small grids -- offsets, the concatenated layout, last-writer and near-wall
// tables against a straightforward restatement, every index the kernels follow inside its table -- and every class of bad
// table refused with a message that names the case, leaving the output untouched.  The single mesh of psm_set_geometry goes
// through the same builder (one case, `single`): with and without the grid->mesh tables, each against a plain loop written here.
// Built and run by tests/test_mesh_cases.py with g++ -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <random>

#include "psm_mesh_tables.h"

struct Case {
  int64_t n;
  std::vector<int32_t> v1, idx, v2;
  std::vector<double> w1, sdf, w2;
  PsmMeshCaseInput in() const { return {n, v1.data(), w1.data(), idx.data(), sdf.data(), v2.data(), w2.data()}; }
};

static Case make_case(std::mt19937& rng, int ny, int nx) {
  std::uniform_real_distribution<double> u(-0.2, 1.0);
  const int64_t ng = (int64_t)ny * nx;
  Case c;
  c.n = 5 + (int64_t)(rng() % 200);
  c.v1.resize(ng * 3); c.w1.resize(ng * 3); c.idx.resize(ng * 2); c.sdf.resize(ng); c.v2.resize(c.n * 3); c.w2.resize(c.n * 3);
  for (int64_t t = 0; t < ng; ++t) {
    for (int j = 0; j < 3; ++j) { c.v1[t * 3 + j] = (int32_t)(rng() % c.n); c.w1[t * 3 + j] = u(rng); }
    // most points land on their own cell, some collide (the last writer wins), some cells stay empty
    const bool own = rng() % 8 != 0;
    c.idx[t * 2] = own ? (int32_t)(t / nx) : (int32_t)(rng() % ny);
    c.idx[t * 2 + 1] = own ? (int32_t)(t % nx) : (int32_t)(rng() % nx);
    c.sdf[t] = rng() % 16 == 0 ? 0.0 : u(rng) * 0.3;
  }
  for (int64_t n = 0; n < c.n; ++n)
    for (int j = 0; j < 3; ++j) { c.v2[n * 3 + j] = (int32_t)(rng() % ng); c.w2[n * 3 + j] = u(rng); }
  return c;
}

#define REQUIRE(cond, msg) do { if (!(cond)) { std::printf("FAILED: %s (line %d)\n", msg, __LINE__); return 1; } } while (0)

// One mesh as psm_set_geometry hands it over, with (g2m) or without the grid->mesh pair: every table against the loops
// psm_set_geometry used to run inline; refusals carry no "case k: " prefix.
static int single_mesh(std::mt19937& rng, int ny, int nx, bool g2m, double scale, double wall) {
  const int64_t ng = (int64_t)ny * nx;
  const Case c = make_case(rng, ny, nx);
  PsmMeshCaseInput in = c.in();
  if (!g2m) { in.vtx_g2m = nullptr; in.wts_g2m = nullptr; }
  PsmMeshCaseTables t;
  std::string why;
  REQUIRE(psm_build_mesh_case_tables(1, &in, ny, nx, scale, wall, t, why, true) == 0, why.c_str());
  REQUIRE(t.n_cases == 1 && t.have_g2m == g2m && t.n_grid == ng && t.total == c.n && t.max_cells == c.n, "single: header");
  REQUIRE(t.cell_off == (std::vector<int64_t>{0, c.n}), "single: offsets");
  std::vector<int32_t> src(ng, -1), cop(ng);
  for (int64_t p = 0; p < ng; ++p) {
    const int64_t cell = (int64_t)c.idx[p * 2] * nx + c.idx[p * 2 + 1];
    src[cell] = (int32_t)p;
    cop[p] = (int32_t)cell;
  }
  REQUIRE(t.src_of_cell == src && t.cell_of_point == cop, "single: last writer / cell of point");
  REQUIRE(t.vtx_m2g == c.v1 && t.wts_m2g == c.w1 && t.sdf == c.sdf, "single: mesh->grid tables");
  REQUIRE(t.sdf_image.size() == (size_t)ng * 3, "single: image size");
  for (int64_t p = 0; p < ng; ++p) {
    const double sdv = c.sdf[p] * scale;
    REQUIRE(t.sdf_image[p * 3] == 0.f && t.sdf_image[p * 3 + 1] == 0.f && t.sdf_image[p * 3 + 2] == ((sdv != sdv) ? 0.f : (float)sdv), "single: bound image");
  }
  REQUIRE(t.vtx_g2m.size() == (size_t)c.n * 3 && t.wts_g2m.size() == (size_t)c.n * 3 && t.near_wall.size() == (size_t)c.n, "single: grid->mesh sizes");
  for (int64_t n = 0; n < c.n; ++n) {
    double acc = 0.0; bool neg = false;
    for (int j = 0; j < 3; ++j) {
      REQUIRE(t.vtx_g2m[n * 3 + j] == (g2m ? c.v2[n * 3 + j] : 0) && t.wts_g2m[n * 3 + j] == (g2m ? c.w2[n * 3 + j] : 0.0), "single: grid->mesh tables (absent: zero-filled)");
      acc += c.sdf[c.v2[n * 3 + j]] * c.w2[n * 3 + j]; neg = neg || c.w2[n * 3 + j] < 0.0;
    }
    REQUIRE(t.near_wall[n] == (g2m && !neg && acc < wall ? 1 : 0), "single: near wall (absent: all 0)");
  }
  // refusals: the texts of psm_set_geometry, no case named, the earlier result untouched
  Case b = c;
  b.v1[(rng() % ng) * 3 + 2] = (int32_t)b.n;
  in = b.in();
  REQUIRE(psm_build_mesh_case_tables(1, &in, ny, nx, scale, wall, t, why, true) == -1 && why == "mesh->grid vertex index out of range", "single: bad vertex");
  in = c.in(); in.wts_g2m = nullptr;
  REQUIRE(psm_build_mesh_case_tables(1, &in, ny, nx, scale, wall, t, why, true) == -1 && why == "vtx_g2m and wts_g2m go together", "single: half a pair");
  in = c.in();
  REQUIRE(psm_build_mesh_case_tables(1, &in, ny, 0, scale, wall, t, why, true) == -1 && why == "bad case set", "single: a shape no grid has");
  REQUIRE(t.cell_off == (std::vector<int64_t>{0, c.n}) && t.src_of_cell == src, "single: a refused mesh changed the output");
  return 0;
}

int main() {
  std::mt19937 rng(11);
  int sets = 0, refused = 0;
  for (int trial = 0; trial < 60; ++trial) {
    const int ny = 3 + (int)(rng() % 20), nx = 3 + (int)(rng() % 30), K = 1 + (int)(rng() % 5);
    const int64_t ng = (int64_t)ny * nx;
    const double scale = trial % 2 ? 1.0 / 0.999023 : 1.0, wall = 0.05;
    std::vector<Case> cs;
    std::vector<PsmMeshCaseInput> in;
    for (int k = 0; k < K; ++k) cs.push_back(make_case(rng, ny, nx));
    for (const Case& c : cs) in.push_back(c.in());
    PsmMeshCaseTables t;
    std::string why;
    REQUIRE(psm_build_mesh_case_tables(K, in.data(), ny, nx, scale, wall, t, why) == 0, why.c_str());
    REQUIRE(t.n_cases == K && t.n_grid == ng && (int)t.cell_off.size() == K + 1 && t.cell_off[0] == 0, "header");
    REQUIRE(t.vtx_m2g.size() == (size_t)K * ng * 3 && t.sdf_image.size() == (size_t)K * ng * 3 && t.near_wall.size() == (size_t)t.total, "sizes");
    int64_t mx = 0;
    for (int k = 0; k < K; ++k) {
      const Case& c = cs[k];
      REQUIRE(t.cell_off[k + 1] - t.cell_off[k] == c.n, "offsets");
      mx = std::max(mx, c.n);
      const int64_t g0 = (int64_t)k * ng, c0 = t.cell_off[k];
      std::vector<int32_t> src(ng, -1);
      for (int64_t p = 0; p < ng; ++p) src[(int64_t)c.idx[p * 2] * nx + c.idx[p * 2 + 1]] = (int32_t)p;
      for (int64_t p = 0; p < ng; ++p) {
        REQUIRE(t.src_of_cell[g0 + p] == src[p], "last writer");
        REQUIRE(t.cell_of_point[g0 + p] == c.idx[p * 2] * nx + c.idx[p * 2 + 1], "cell of point");
        REQUIRE(t.sdf[g0 + p] == c.sdf[p] && t.sdf_image[(g0 + p) * 3 + 2] == (float)(c.sdf[p] * scale), "sdf");
        REQUIRE(t.sdf_image[(g0 + p) * 3] == 0.f && t.sdf_image[(g0 + p) * 3 + 1] == 0.f, "velocity channels of the bound image");
        for (int j = 0; j < 3; ++j) {
          const int32_t v = t.vtx_m2g[(g0 + p) * 3 + j];
          REQUIRE(v == c.v1[p * 3 + j] && v >= 0 && c0 + v < t.cell_off[k + 1], "mesh->grid vertex stays inside its case");
          REQUIRE(t.wts_m2g[(g0 + p) * 3 + j] == c.w1[p * 3 + j], "mesh->grid weight");
        }
      }
      for (int64_t n = 0; n < c.n; ++n) {
        double acc = 0.0; bool neg = false;
        for (int j = 0; j < 3; ++j) {
          const int32_t v = t.vtx_g2m[(c0 + n) * 3 + j];
          REQUIRE(v == c.v2[n * 3 + j] && v >= 0 && v < ng, "grid->mesh vertex");
          REQUIRE(t.wts_g2m[(c0 + n) * 3 + j] == c.w2[n * 3 + j], "grid->mesh weight");
          acc += c.sdf[v] * c.w2[n * 3 + j]; neg = neg || c.w2[n * 3 + j] < 0.0;
        }
        REQUIRE(t.near_wall[c0 + n] == ((!neg && acc < wall) ? 1 : 0), "near wall");
      }
    }
    REQUIRE(t.total == t.cell_off[K] && t.max_cells == mx, "totals");
    ++sets;

    // one bad table in one case: refused, the case named, the earlier result untouched
    const int bad = (int)(rng() % K), what = trial % 6;
    Case b = cs[bad];
    if (what == 0) b.v1[(rng() % ng) * 3 + 1] = (int32_t)b.n;
    if (what == 1) b.v1[(rng() % ng) * 3] = -1;
    if (what == 2) b.idx[(rng() % ng) * 2] = ny;
    if (what == 3) b.idx[(rng() % ng) * 2 + 1] = -1;
    if (what == 4) b.v2[(rng() % b.n) * 3 + 2] = (int32_t)ng;
    in[bad] = b.in();
    if (what == 5) { in[bad].vtx_g2m = nullptr; in[bad].wts_g2m = nullptr; }
    const std::vector<int64_t> before = t.cell_off;
    REQUIRE(psm_build_mesh_case_tables(K, in.data(), ny, nx, scale, wall, t, why) != 0, "a bad table was accepted");
    REQUIRE(why.find("case " + std::to_string(bad) + ":") == 0, "the message does not name the case");
    REQUIRE(t.cell_off == before, "a refused set changed the output");
    ++refused;
  }
  PsmMeshCaseTables t;
  std::string why;
  REQUIRE(psm_build_mesh_case_tables(0, nullptr, 4, 4, 1.0, 0.05, t, why) != 0 && !why.empty(), "an empty set was accepted");
  int singles = 0;
  for (int trial = 0; trial < 20; ++trial, ++singles) {
    const int ny = 3 + (int)(rng() % 20), nx = 3 + (int)(rng() % 30);
    if (single_mesh(rng, ny, nx, trial % 2 == 1, trial % 4 < 2 ? 1.0 : 1.0 / 0.999023, 0.05)) return 1;
  }
  std::printf("case sets built: %d, refused: %d, single meshes: %d\n", sets, refused, singles);
  return 0;
}
