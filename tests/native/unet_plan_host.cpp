// The conv path's planner (csrc/psm_unet_plan.cpp) on the host, no device: every configuration of tests/golden/unet_plan_matrix.txt is planned
// in float32 and in bf16 through psm_unet_plan_env + psm_unet_plan_layers, and the table of decision records must equal the fixture
// byte for byte (it was recorded from the planner as it stood inside psm_unet_api.cpp before the split).  Then structural invariants
// of every row and the coverage of the matrix.  Usage: unet_plan_host FIXTURE
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "psm_unet_plan.h"

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out; std::string cur; std::istringstream is(s);
  while (std::getline(is, cur, sep)) out.push_back(cur);
  return out;
}
static const char* SWITCHES[] = {"FILL", "KSPLIT_MAX", "KW", "NO_BIG_TILES", "SPLIT_MIN_CHUNKS", "X6", "PAIR_MIN", "NO_PAIR", "F32_ACT", "PAIR32",
                                 "NO_STEM", "NO_SPLIT", "NO_HEAD_FUSION", "FORCE"};
static int failures = 0;
static void check(bool ok, const std::string& what) { if (!ok) { std::printf("FAIL %s\n", what.c_str()); ++failures; } }

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: unet_plan_host FIXTURE\n"); return 2; }
  std::ifstream in(argv[1]);
  std::vector<std::string> want, got;           // the fixture's lines but its comments / the lines this planner writes
  for (std::string line; std::getline(in, line);) if (!line.empty() && line[0] != '#') want.push_back(line);
  std::map<std::string, int> seen;              // coverage: rows per value
  int n_configs = 0;
  for (const std::string& line : want) {
    if (line.rfind("config ", 0) != 0) continue;
    got.push_back(line); ++n_configs;
    const std::vector<std::string> tok = split(line, ' ');
    std::map<std::string, std::string> kv;
    for (size_t i = 2; i < tok.size(); ++i) { const size_t e = tok[i].find('='); kv[tok[i].substr(0, e)] = tok[i].substr(e + 1); }
    std::vector<int> widths; for (auto& w : split(kv["widths"], ',')) widths.push_back(std::atoi(w.c_str()));
    for (const char* s : SWITCHES) unsetenv((std::string("PSM_UNET_") + s).c_str());
    if (kv["env"] != "-") for (auto& a : split(kv["env"], ';')) { const size_t e = a.find('='); setenv(a.substr(0, e).c_str(), a.substr(e + 1).c_str(), 1); }
    const ConvPlanEnv env = psm_unet_plan_env();
    const int c_in = std::atoi(kv["c_in"].c_str()), c_out = std::atoi(kv["c_out"].c_str());
    const int ny = std::atoi(kv["ny"].c_str()), nx = std::atoi(kv["nx"].c_str()), n = std::atoi(kv["n"].c_str());
    for (int bf16 = 0; bf16 < 2; ++bf16) {
      std::vector<ConvLayer> L = psm_unet_layers(c_in, c_out, widths);
      std::vector<int32_t> choices(4 * L.size(), -1);                                       // every choice by rule,
      for (size_t i = 0; i < L.size(); ++i) choices[4 * i + PSM_CHOICE_KSPLIT_CAP] = 8;     // any split
      if (kv["choices"] != "-") { choices.clear(); for (auto& l : split(kv["choices"], ',')) for (auto& v : split(l, ':')) choices.push_back(std::atoi(v.c_str())); }
      std::string why;
      const std::string tag = tok[1] + (bf16 ? " bf16 " : " f32 ");
      if (psm_unet_plan_layers(L, c_in, ny, nx, n, bf16 != 0, choices, env, why)) { check(false, tag + "not planned: " + why); continue; }
      for (size_t i = 0; i < L.size(); ++i) {
        const ConvLayer& c = L[i];
        int32_t d[16];
        psm_unet_layer_detail(c, c.src != 0 ? &L[i - 1] : nullptr, c.src == 3 ? &L[c.skip] : nullptr, bf16 != 0, false, d);
        const long long v[29] = {c.k, c.cin, c.cout, c.level, c.src, c.skip, c.relu, c.arrangement, c.nct, c.n_chunks, c.groups, c.ksplit, c.kw, c.stem, c.fuse_head,
                                 c.in_bf, c.out_bf, c.x6, c.pair, c.pair == 1 ? c.pair_kind : 0, c.padded, c.P, c.case_elems, c.origin, c.slab, d[7], d[8], d[12], d[13]};
        std::string row = "row " + tag + std::to_string(i);
        for (long long x : v) row += ' ' + std::to_string(x);
        got.push_back(row);
        const std::string at = tag + std::to_string(i);
        if (c.k == 3) {
          check(c.groups * c.nct >= (c.cout + 15) / 16, at + ": groups * nct < ceil(cout / 16)");
          check(c.ksplit <= c.n_chunks, at + ": ksplit > n_chunks");
          ++seen["arrangement " + std::to_string(c.arrangement)]; ++seen["nct " + std::to_string(c.nct)];
          ++seen["ksplit " + std::to_string(c.ksplit)]; ++seen["kw " + std::to_string(c.kw)]; ++seen["x6 " + std::to_string(c.x6)];
        }
        if (c.pair == 1) { check(i + 1 < L.size() && L[i + 1].pair == 2, at + ": a pair leader is not followed by pair == 2"); ++seen["pair kind " + std::to_string(c.pair_kind)]; }
        if (c.pair == 2) check(i > 0 && L[i - 1].pair == 1, at + ": pair == 2 without a leader in front");
        ++seen["pair " + std::to_string(c.pair)]; ++seen["stem " + std::to_string(d[8])]; ++seen["in_bf " + std::to_string(c.in_bf)];
        ++seen["out_bf " + std::to_string(c.out_bf)]; ++seen["fuse_head " + std::to_string(c.fuse_head)]; ++seen["source " + std::to_string(d[7])];
      }
    }
  }
  check(got.size() == want.size(), "the planner wrote " + std::to_string(got.size()) + " lines, the fixture holds " + std::to_string(want.size()));
  for (size_t i = 0; i < got.size() && i < want.size(); ++i)
    if (got[i] != want[i]) { check(false, "line differs from the fixture\n  fixture: " + want[i] + "\n  planner: " + got[i]); if (failures > 20) break; }
  // every kernel-selecting value in at least 4 rows (arrangements 3 and 4, each: the forced configurations)
  for (const char* key : {"arrangement 0", "arrangement 1", "arrangement 2", "arrangement 3", "arrangement 4", "nct 1", "nct 2", "nct 4", "ksplit 1", "ksplit 2", "ksplit 4", "ksplit 8",
                          "kw 1", "kw 2", "x6 0", "x6 1", "pair 0", "pair 1", "pair 2", "pair kind 0", "pair kind 1", "pair kind 2", "stem 0", "stem 1", "stem 2",
                          "in_bf 0", "in_bf 1", "out_bf 0", "out_bf 1", "fuse_head 0", "fuse_head 1", "source 0", "source 1", "source 2", "source 3", "source 4"})
    check(seen[key] >= 4, std::string("coverage: '") + key + "' in " + std::to_string(seen[key]) + " rows, 4 wanted");
  std::printf("configurations: %d, rows: %zu, failures: %d\n", n_configs, got.size() - (size_t)n_configs, failures);
  return failures ? 1 : 0;
}
