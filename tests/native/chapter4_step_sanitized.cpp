// The Chapter-4 image pack as a stage of the step around a solve (csrc/psm_handle.h: Chapter4Call in StepCall, GraphKey), in a
// stand-alone host program: no HIP call, so it runs without a device.  Built with AddressSanitizer + UBSan.
//
// Every field of Chapter4Call gets one GraphKey that differs from the base in that field alone: the keys must be pairwise
// inequivalent and find their own entries in a map -- a pointer that is in the captured launch but not in the key would make two
// different steps replay one graph.  Then StepCall::fault: the step psm_chapter4_frames* builds is defined, and every combination
// the sequence excludes is refused with a message of its own.
#include "psm_handle.h"

#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double D[32];     // addresses to point at: elements of one array, so that comparing them is defined
static float F[32];

static GraphKey base_key() {
  GraphKey k{5, &F[0], &F[1], StepCall{}};
  StepCall& s = k.step;
  s.frames.cols = &D[0]; s.frames.k = 3; s.frames.fill = 1;
  for (int c = 0; c < 3; ++c) s.frames.out[c] = PsmFramePlane{&D[1 + c], 100, 0};
  s.chapter4 = Chapter4Call{&D[4], &F[2], &D[5]};
  return k;
}

int main() {
  struct Variant { std::string name; GraphKey key; };
  std::vector<Variant> v;
  auto add = [&](const std::string& name, void (*edit)(GraphKey&)) { GraphKey k = base_key(); edit(k); v.push_back({name, k}); };
  add("base", [](GraphKey&) {});
  add("chapter4.planes", [](GraphKey& k) { k.step.chapter4.planes = &D[10]; });
  add("chapter4.grid", [](GraphKey& k) { k.step.chapter4.grid = &F[10]; });
  add("chapter4.truth", [](GraphKey& k) { k.step.chapter4.truth = &D[11]; });
  add("chapter4.truth null", [](GraphKey& k) { k.step.chapter4.truth = nullptr; });
  add("no chapter4", [](GraphKey& k) { k.step.chapter4 = Chapter4Call{}; });
  add("deltas on the same planes", [](GraphKey& k) { k.step.deltas.planes = k.step.chapter4.planes; k.step.deltas.grid = k.step.chapter4.grid;
                                                     k.step.deltas.truth = k.step.chapter4.truth; k.step.chapter4 = Chapter4Call{}; });
  add("gradp on the same planes", [](GraphKey& k) { k.step.gradp.planes = k.step.chapter4.planes; k.step.gradp.grid = k.step.chapter4.grid;
                                                    k.step.gradp.truth = k.step.chapter4.truth; k.step.chapter4 = Chapter4Call{}; });
  const size_t n = v.size();
  for (size_t i = 0; i < n; ++i) {
    CHECK(!(v[i].key < v[i].key), "%s < itself", v[i].name.c_str());
    for (size_t j = 0; j < n; ++j) {
      const bool a = v[i].key < v[j].key, b = v[j].key < v[i].key;
      CHECK(!(a && b), "%s and %s are each below the other", v[i].name.c_str(), v[j].name.c_str());
      CHECK((i == j) == (!a && !b), "%s and %s: equivalent = %d", v[i].name.c_str(), v[j].name.c_str(), (int)(!a && !b));
    }
  }
  std::map<GraphKey, size_t> cache;
  for (size_t i = 0; i < n; ++i) cache.emplace(v[i].key, i);
  CHECK(cache.size() == n, "the map holds %zu keys, expected %zu", cache.size(), n);
  for (size_t i = 0; i < n; ++i) CHECK(cache.count(v[i].key) == 1 && cache.at(v[i].key) == i, "%s finds another step's entry", v[i].name.c_str());
  { GraphKey c = base_key(); CHECK(!(c < v[0].key) && !(v[0].key < c), "a copy of the base is another key"); }

  // ---- the combinations of stages ----
  FrameCall fr; fr.cols = &D[0]; fr.k = 3;
  const Chapter4Call c4{&D[1], &F[0], &D[2]};
  StepCall ok; ok.frames = fr; ok.chapter4 = c4;
  CHECK(!ok.fault(), "psm_chapter4_frames*: %s", ok.fault() ? ok.fault() : "");
  { StepCall s = ok; s.chapter4.truth = nullptr; CHECK(!s.fault(), "psm_chapter4_image_device's pack without the truth plane"); }
  std::set<std::string> messages;
  auto refused = [&](const char* what, StepCall s) {
    const char* m = s.fault();
    CHECK(m != nullptr, "%s is not refused", what);
    if (m) { CHECK(std::string(m).find("Chapter-4") != std::string::npos, "%s: the message does not name the Chapter-4 pack: %s", what, m); messages.insert(m); }
  };
  { StepCall s = ok; s.deltas = DeltasCall{&D[3], &F[1], &F[2], &D[4], &F[3]}; refused("with the deltas pack", s); }
  { StepCall s = ok; s.gradp = GradpCall{&D[5], &F[4], &D[6], &F[5]}; refused("with the gradP pack", s); }
  { StepCall s = ok; s.feat = FeatCall{&D[7], &F[6]}; refused("with the features", s); }
  { StepCall s = ok; s.p = &F[7]; refused("with the bound integration", s); }
  { StepCall s = ok; s.post.apply_filter = 0; s.post.result = &F[8]; refused("with post-steps (no filter)", s); }
  { StepCall s = ok; s.post.apply_filter = 1; s.post.result = &F[8]; refused("with post-steps (filter)", s); }
  { StepCall s; s.chapter4 = c4; refused("without frames", s); }
  CHECK(messages.size() == 6, "%zu distinct messages for six rules", messages.size());

  std::printf("chapter4 step: %zu keys, %zu fault messages, %d failures\n", n, messages.size(), g_failures);
  return g_failures ? 1 : 0;
}
