// The host logic of the rows stage (csrc/psm_rows.h, and RowsCall / StepCall in csrc/psm_handle.h) in a stand-alone host program: no HIP
// call, so it runs without a device.  Built with AddressSanitizer + UBSan by tests/test_rows_abi.py.
//   - the sizing helpers: columns and least width per kind, parts per frame (1 .. PSM_ROWS_PARTS) and the cells a part covers
//   - every field of RowsCall that the two launches hold is in the graph key: one GraphKey per field that differs in it alone
//   - the combinations of stages: rows need frames on the columns they write
#include "psm_handle.h"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double D[16];
static float F[16];

static GraphKey base_key() {
  GraphKey k{3, &F[0], &F[1], StepCall{}};
  RowsCall& r = k.step.rows;
  r.rows = &F[2]; r.kind = PSM_ROWS_KIND_POISSON; r.width = 11; r.cols = &D[0]; r.scalars = &D[1]; r.n_cells = 700;
  r.base = 0.047; r.phi = 0.16; r.ex = 1.5; r.ey = 0.6; r.wired = true;
  k.step.frames.cols = &D[0]; k.step.frames.k = 8;
  k.step.feat = FeatCall{&D[2], &F[3]};
  return k;
}

int main() {
  // ---- sizing
  CHECK(psm_rows_cols(PSM_ROWS_KIND_DELTAS) == 3 && psm_rows_cols(PSM_ROWS_KIND_POISSON) == 8 && psm_rows_cols(PSM_ROWS_KIND_GRADP) == 5, "columns per kind");
  CHECK(psm_rows_cols(-1) == 0 && psm_rows_cols(3) == 0, "an unknown kind has no columns");
  CHECK(psm_rows_min_width(PSM_ROWS_KIND_DELTAS) == 11 && psm_rows_min_width(PSM_ROWS_KIND_POISSON) == 11 && psm_rows_min_width(PSM_ROWS_KIND_GRADP) == 8, "least width per kind");
  const int64_t cells[] = {1, 255, 256, 257, 513, 4097, 65535, 65536, 65537, 65793, 1000000, (int64_t)1 << 33};
  for (int64_t n : cells) {
    const int parts = psm_rows_parts(n);
    CHECK(parts >= 1 && parts <= PSM_ROWS_PARTS, "%lld cells: %d parts", (long long)n, parts);
    // the partial launch strides over the cells with parts * PSM_ROWS_CHUNK: every part below the cap holds at least one cell
    CHECK((int64_t)(parts - 1) * PSM_ROWS_CHUNK < n, "%lld cells: the last of %d parts is empty", (long long)n, parts);
    if (parts < PSM_ROWS_PARTS) CHECK((int64_t)parts * PSM_ROWS_CHUNK >= n, "%lld cells: %d parts below the cap do not cover them in one pass", (long long)n, parts);
  }
  CHECK(psm_rows_parts(256) == 1 && psm_rows_parts(257) == 2 && psm_rows_parts(65536) == 256 && psm_rows_parts(65793) == 256, "part edges");

  // ---- the key
  std::vector<std::pair<std::string, GraphKey>> v;
  auto distinct = [&](const std::string& name, const std::function<void(RowsCall&)>& edit) {
    GraphKey k = base_key(); edit(k.step.rows); v.push_back({name, k});
  };
  distinct("base", [](RowsCall&) {});
  distinct("rows", [](RowsCall& r) { r.rows = &F[4]; });
  distinct("kind", [](RowsCall& r) { r.kind = PSM_ROWS_KIND_DELTAS; });
  distinct("width", [](RowsCall& r) { r.width = 12; });
  distinct("cols", [](RowsCall& r) { r.cols = &D[3]; });
  distinct("scalars", [](RowsCall& r) { r.scalars = &D[4]; });
  distinct("n_cells", [](RowsCall& r) { r.n_cells = 701; });
  distinct("base value", [](RowsCall& r) { r.base = 0.048; });
  distinct("phi", [](RowsCall& r) { r.phi = 0.2; });
  distinct("ex", [](RowsCall& r) { r.ex = 1.6; });
  distinct("ey", [](RowsCall& r) { r.ey = 0.7; });
  distinct("wired", [](RowsCall& r) { r.wired = false; });
  distinct("absent", [](RowsCall& r) { r = RowsCall{}; });
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t j = 0; j < v.size(); ++j) {
      const bool lt = v[i].second < v[j].second, gt = v[j].second < v[i].second;
      CHECK(!(lt && gt), "%s and %s are each below the other", v[i].first.c_str(), v[j].first.c_str());
      CHECK((!lt && !gt) == (i == j), "%s and %s: equivalent = %d", v[i].first.c_str(), v[j].first.c_str(), (int)(!lt && !gt));
    }
  const GraphKey a = base_key(), b = base_key();
  CHECK(!(a < b) && !(b < a), "two copies of one step are one key");

  // ---- scaled(): only a wired deltas / Poisson stage writes the solve's row scale
  RowsCall r = base_key().step.rows;
  CHECK(r.scaled(), "wired Poisson rows write the row scale");
  r.kind = PSM_ROWS_KIND_GRADP; CHECK(!r.scaled(), "gradP rows leave the row scale alone");
  r.kind = PSM_ROWS_KIND_DELTAS; r.wired = false; CHECK(!r.scaled(), "the stage alone writes no row scale");
  r = RowsCall{}; CHECK(!r.scaled(), "no rows stage");

  // ---- the combinations of stages
  StepCall s = base_key().step;
  CHECK(!s.fault(), "psm_poisson_rows*: %s", s.fault() ? s.fault() : "");
  s.rows.cols = &D[5]; CHECK(s.fault() != nullptr, "rows that write other columns than the frames read");
  s = base_key().step; s.frames = FrameCall{}; s.feat = FeatCall{}; CHECK(s.fault() != nullptr, "rows without frames");
  s = base_key().step; s.feat = FeatCall{}; s.deltas = DeltasCall{&D[6], &F[5], &F[6], &D[7], &F[7]}; CHECK(!s.fault(), "psm_deltas_rows*");
  s.deltas = DeltasCall{}; s.gradp = GradpCall{&D[8], &F[8], &D[9], &F[9]}; CHECK(!s.fault(), "psm_gradp_rows*");

  std::printf("rows host logic: %zu key variants, %d failures\n", v.size(), g_failures);
  return g_failures ? 1 : 0;
}
