// The graph cache key of the step around a solve (csrc/psm_handle.h: StepCall, GraphKey) and the combinations of stages the sequence
// defines (StepCall::fault), in a stand-alone host program: no HIP call, so it runs without a device.  Built with AddressSanitizer + UBSan.
//
// Every keyed field of every stage descriptor gets one GraphKey that differs from the base in that field alone; the ordering must
// be a strict weak order in which two keys are equivalent exactly when no keyed field differs -- a field that is in the sequence
// but not in the key would make two different steps replay one graph.
#include "psm_handle.h"

#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double D[64];     // addresses to point at: elements of one array, so that comparing them is defined
static float F[64];

struct Variant { std::string name; GraphKey key; int cls; };   // cls: keys of one class are equivalent

static GraphKey base_key() {
  GraphKey k{5, &F[0], &F[1], StepCall{}};
  StepCall& s = k.step;
  s.frames.cols = &D[0]; s.frames.k = 7; s.frames.fill = 1;
  for (int c = 0; c < PSM_FRAME_MAX_COLS; ++c) s.frames.out[c] = PsmFramePlane{&D[1 + c], 100 + c, c & 1};
  s.feat = FeatCall{&D[20], &F[2]};
  s.deltas = DeltasCall{&D[21], &F[3], &F[4], &D[22], &F[5]};
  s.gradp = GradpCall{&D[23], &F[6], &D[24], &F[7]};
  s.p = &F[8];
  s.post.apply_filter = 1; s.post.dU = &F[9]; s.post.prev = &F[10]; s.post.result = &F[11]; s.post.change = &F[12]; s.post.next = &F[13];
  return k;
}

int main() {
  std::vector<Variant> v;
  int next_cls = 0;
  auto distinct = [&](const std::string& name, const std::function<void(GraphKey&)>& edit) {
    GraphKey k = base_key(); edit(k); v.push_back({name, k, next_cls++});
  };
  auto same_as_base = [&](const std::string& name, const std::function<void(GraphKey&)>& edit) {
    GraphKey k = base_key(); edit(k); v.push_back({name, k, 0});
  };
  distinct("base", [](GraphKey&) {});
  // the solve's own part
  distinct("n", [](GraphKey& k) { k.n = 6; });
  distinct("g", [](GraphKey& k) { k.g = &F[40]; });
  distinct("f", [](GraphKey& k) { k.f = &F[41]; });
  // FrameCall: cols, k, fill and the three fields of each of the k planes
  distinct("frames.cols", [](GraphKey& k) { k.step.frames.cols = &D[40]; });
  distinct("frames.k", [](GraphKey& k) { k.step.frames.k = 6; });
  distinct("frames.fill", [](GraphKey& k) { k.step.frames.fill = 0; });
  for (int c = 0; c < 7; ++c) {
    distinct("frames.out[" + std::to_string(c) + "].dst", [c](GraphKey& k) { k.step.frames.out[c].dst = &D[41 + c]; });
    distinct("frames.out[" + std::to_string(c) + "].frame_stride", [c](GraphKey& k) { k.step.frames.out[c].frame_stride = 999; });
    distinct("frames.out[" + std::to_string(c) + "].as_f32", [c](GraphKey& k) { k.step.frames.out[c].as_f32 ^= 1; });
  }
  distinct("feat.vel", [](GraphKey& k) { k.step.feat.vel = &D[50]; });
  distinct("feat.grid", [](GraphKey& k) { k.step.feat.grid = &F[42]; });
  distinct("deltas.planes", [](GraphKey& k) { k.step.deltas.planes = &D[51]; });
  distinct("deltas.grid", [](GraphKey& k) { k.step.deltas.grid = &F[43]; });
  distinct("deltas.label", [](GraphKey& k) { k.step.deltas.label = &F[44]; });
  distinct("deltas.truth", [](GraphKey& k) { k.step.deltas.truth = &D[52]; });
  distinct("gradp.planes", [](GraphKey& k) { k.step.gradp.planes = &D[53]; });
  distinct("gradp.grid", [](GraphKey& k) { k.step.gradp.grid = &F[45]; });
  distinct("gradp.truth", [](GraphKey& k) { k.step.gradp.truth = &D[54]; });
  distinct("gradp.p", [](GraphKey& k) { k.step.gradp.p = &F[46]; });
  distinct("p", [](GraphKey& k) { k.step.p = &F[47]; });
  distinct("post.apply_filter", [](GraphKey& k) { k.step.post.apply_filter = 0; });
  distinct("post.dU", [](GraphKey& k) { k.step.post.dU = &F[48]; });
  distinct("post.prev", [](GraphKey& k) { k.step.post.prev = &F[49]; });
  distinct("post.result", [](GraphKey& k) { k.step.post.result = &F[50]; });
  distinct("post.change", [](GraphKey& k) { k.step.post.change = &F[51]; });
  distinct("post.next", [](GraphKey& k) { k.step.post.next = &F[52]; });
  // every stage absent: the plain solve
  distinct("no stages", [](GraphKey& k) { k.step = StepCall{}; });
  // equal pairs: a copy, the binding's row buffer (not part of the key: it is the same for every call of a binding), a plane beyond k
  same_as_base("copy", [](GraphKey&) {});
  same_as_base("deltas.res", [](GraphKey& k) { k.step.deltas.res = &F[53]; });
  same_as_base("frames.out[k].dst", [](GraphKey& k) { k.step.frames.out[7].dst = &D[60]; });
  same_as_base("frames.out[15].as_f32", [](GraphKey& k) { k.step.frames.out[15].as_f32 ^= 1; });

  const size_t n = v.size();
  std::vector<std::vector<char>> lt(n, std::vector<char>(n));
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) lt[i][j] = v[i].key < v[j].key;
  for (size_t i = 0; i < n; ++i) {
    CHECK(!lt[i][i], "%s < itself", v[i].name.c_str());
    for (size_t j = 0; j < n; ++j) {
      CHECK(!(lt[i][j] && lt[j][i]), "%s and %s are each below the other", v[i].name.c_str(), v[j].name.c_str());
      const bool equivalent = !lt[i][j] && !lt[j][i];
      CHECK(equivalent == (v[i].cls == v[j].cls), "%s and %s: equivalent = %d, expected %d", v[i].name.c_str(), v[j].name.c_str(),
            (int)equivalent, (int)(v[i].cls == v[j].cls));
      for (size_t k = 0; k < n; ++k)
        CHECK(!(lt[i][j] && lt[j][k]) || lt[i][k], "not transitive: %s < %s < %s", v[i].name.c_str(), v[j].name.c_str(), v[k].name.c_str());
    }
  }
  std::map<GraphKey, int> cache;
  for (const Variant& x : v) cache.emplace(x.key, x.cls);
  CHECK((int)cache.size() == next_cls, "the map holds %zu keys, expected %d", cache.size(), next_cls);
  for (const Variant& x : v) CHECK(cache.count(x.key) == 1 && cache.at(x.key) == x.cls, "%s finds another step's entry", x.name.c_str());

  // ---- the combinations of stages: what each C entry builds is defined, each rule of StepCall::fault refuses one call ----
  FrameCall fr; fr.cols = &D[0]; fr.k = 3;
  const FeatCall ft{&D[1], &F[0]};
  const DeltasCall dl{&D[2], &F[1], &F[2], &D[3], &F[3]};
  const GradpCall gp{&D[4], &F[4], &D[5], &F[5]};
  PostCall po; po.apply_filter = 1; po.result = &F[6];
  auto step = [&](bool frames, bool feat, bool deltas, bool gradp, bool p, bool post) {
    StepCall s;
    if (frames) s.frames = fr;
    if (feat) s.feat = ft;
    if (deltas) s.deltas = dl;
    if (gradp) s.gradp = gp;
    if (p) s.p = &F[7];
    if (post) s.post = po;
    return s;
  };
  //                frames feat deltas gradp p post
  CHECK(!step(0, 0, 0, 0, 0, 0).fault(), "psm_solve_grid*");
  CHECK(!step(0, 0, 0, 0, 1, 0).fault(), "psm_solve_pressure*");
  CHECK(!step(0, 0, 0, 0, 0, 1).fault(), "psm_solve_poststeps*");
  CHECK(!step(0, 0, 0, 0, 1, 1).fault(), "psm_time_kernels with both bound");
  CHECK(!step(0, 1, 0, 0, 0, 1).fault(), "psm_poisson_step*");
  CHECK(!step(1, 1, 0, 0, 0, 1).fault(), "psm_poisson_frames*");
  CHECK(!step(1, 0, 1, 0, 0, 0).fault() && !step(1, 0, 1, 0, 0, 1).fault(), "psm_deltas_frames*");
  CHECK(!step(1, 0, 0, 1, 0, 0).fault() && !step(1, 0, 0, 1, 0, 1).fault(), "psm_gradp_frames*");
  CHECK(step(1, 0, 1, 1, 0, 0).fault(), "deltas with gradp");
  CHECK(step(0, 0, 1, 0, 0, 0).fault(), "deltas without frames");
  CHECK(step(0, 0, 0, 1, 0, 0).fault(), "gradp without frames");
  CHECK(step(1, 1, 1, 0, 0, 0).fault(), "feat with deltas");
  CHECK(step(1, 1, 0, 1, 0, 0).fault(), "feat with gradp");
  CHECK(step(1, 0, 0, 1, 1, 0).fault(), "p with gradp");
  CHECK(step(1, 0, 0, 0, 0, 0).fault() && step(1, 0, 0, 0, 0, 1).fault(), "frames alone");

  std::printf("step keys: %zu variants, %d classes, %d failures\n", n, next_cls, g_failures);
  return g_failures ? 1 : 0;
}
