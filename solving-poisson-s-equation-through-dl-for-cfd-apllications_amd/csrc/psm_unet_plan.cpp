// psm_unet_plan.cpp -- planner of the convolutional path (psm_unet_plan.h): the decisions of psm_unet_plan, one function each, no device.
#include "psm_unet_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

bool psm_pair_kernel_available(int kind, int cm, int c0, int c1, bool head) {
  if (kind == PSM_PAIR_STEM) return cm == 16 && (c0 == 3 || c0 == 4) && !head;
  if (kind == PSM_PAIR_POOL) return cm == 32 && c0 % 16 == 0 && c0 >= 16 && !head;
  if (kind == PSM_PAIR_UPCAT && cm == 16) return c0 == 32 && c1 == 16;          // with or without the fused 1x1 head
  return kind == PSM_PAIR_UPCAT && cm == 32 && c0 % 32 == 0 && c0 >= 32 && c1 % 16 == 0 && c1 >= 16 && !head;
}
static long env_num(const char* name, long unset) { const char* v = getenv(name); return v ? atol(v) : unset; }
ConvPlanEnv psm_unet_plan_env() {
  ConvPlanEnv e;
  e.fill = env_num("PSM_UNET_FILL", 256); e.ksplit_max = (int)env_num("PSM_UNET_KSPLIT_MAX", 8); e.kw = (int)env_num("PSM_UNET_KW", 1);
  e.split_min_chunks = (int)env_num("PSM_UNET_SPLIT_MIN_CHUNKS", 0); e.split_min_set = getenv("PSM_UNET_SPLIT_MIN_CHUNKS") != nullptr;
  e.x6 = env_num("PSM_UNET_X6", 1) != 0; e.pair_min = env_num("PSM_UNET_PAIR_MIN", 96); e.pair32 = env_num("PSM_UNET_PAIR32", 1) != 0;
  e.no_big_tiles = getenv("PSM_UNET_NO_BIG_TILES") != nullptr; e.no_pair = getenv("PSM_UNET_NO_PAIR") != nullptr; e.f32_act = getenv("PSM_UNET_F32_ACT") != nullptr;
  e.no_stem = getenv("PSM_UNET_NO_STEM") != nullptr; e.no_split = getenv("PSM_UNET_NO_SPLIT") != nullptr; e.no_head_fusion = getenv("PSM_UNET_NO_HEAD_FUSION") != nullptr;
  if (const char* f = getenv("PSM_UNET_FORCE")) e.force = f;
  return e;
}
std::vector<ConvLayer> psm_unet_layers(int c_in, int c_out, const std::vector<int>& widths) {
  const int L = (int)widths.size();
  std::vector<ConvLayer> convs;
  auto add = [&](int cin, int cout, int level, int src, int skip = -1) {
    ConvLayer c; c.cin = cin; c.cout = cout; c.level = level; c.src = src; c.skip = skip;
    convs.push_back(c);
  };
  for (int l = 0; l < L; ++l) { add(l == 0 ? c_in : widths[l - 1], widths[l], l, l == 0 ? 0 : 2); add(widths[l], widths[l], l, 1); }
  for (int l = L - 2; l >= 0; --l) { add(widths[l + 1] + widths[l], widths[l], l, 3, 2 * l + 1); add(widths[l], widths[l], l, 1); }   // skip: enc{l}b
  add(widths[0], c_out, 0, 1);                     // the 1x1 head, linear
  convs.back().k = 1; convs.back().relu = 0;
  return convs;
}
void psm_unet_layer_detail(const ConvLayer& c, const ConvLayer* pv, const ConvLayer* sk, bool bf16, bool keep_act, int32_t v[16]) {
  int src = c.src, km = 1;
  if (pv) km = std::max(km, pv->ksplit);
  if (c.src == 3) {
    km = std::max(km, sk->ksplit);
    if (pv->cout % psm_conv_chunk_width(c.x6, bf16) != 0) src = 4;       // the launchers' seam_inside
  }
  const int stem = c.stem ? 1 : (c.k == 3 && c.src == 0 && c.cin % 4 != 0) ? 2 : 0;
  const int32_t d[16] = {c.arrangement, c.nct, c.ksplit, c.kw, c.x6 ? 1 : 0, c.pair, c.pair ? c.pair_kind : 0, src, stem, c.in_bf ? 1 : 0, c.out_bf ? 1 : 0,
                         c.fuse_head ? 1 : 0, km, (c.n_chunks + c.ksplit - 1) / c.ksplit <= 1 ? 1 : 0, keep_act ? 1 : 0, bf16 ? 1 : 0};
  std::copy(d, d + 16, v);
}
namespace {
struct Plan {            // what one plan is made for; H / W: a layer's resolution
  std::vector<ConvLayer>& L;
  int c_in, ny, nx, cases;
  bool bf16;
  const std::vector<int32_t>& choices;
  const ConvPlanEnv& env;
  int H(const ConvLayer& c) const { return ny >> c.level; }
  int W(const ConvLayer& c) const { return nx >> c.level; }
  int choice(size_t i, int what) const { return choices[4 * i + what]; }
};
// The 3x3 loaders address a case's input tensor with 32-bit element offsets (psm_unet.hip: PsmFetchPos::off0 / off1 are int,
// the bf16 loaders add channel and row offsets to them as unsigned): every tensor a loader reads -- the image, and each
// activation at its own resolution, which covers the max-pool source's doubled extent and the upsample / skip sources -- must
// hold fewer than 2^31 elements per case.  Counted on the zero-haloed layout in bf16 mode (act_layout: whether a tensor is
// stored haloed depends on choices a re-plan may change) and on the dense float32 layout otherwise; split-K slabs are
// addressed per slab with 64-bit strides.
bool case_tensors_fit(const Plan& p, std::string& why) {
  int64_t worst = (int64_t)p.ny * p.nx * p.c_in;
  for (size_t i = 0; i + 1 < p.L.size(); ++i) {
    const ConvLayer& c = p.L[i];
    const int64_t H = p.H(c), W = p.W(c);
    worst = std::max(worst, p.bf16 ? (ACT_PADT + H + ACT_PADB) * (ACT_PADL + W + ACT_PADR) * c.cout : H * W * c.cout);
  }
  if (worst >= (int64_t)1 << 31)
    why = "image too large: a case's activation tensor would hold " + std::to_string(worst) +
          " elements, the convolution loaders' 32-bit offsets allow fewer than 2^31 per case";
  return worst < (int64_t)1 << 31;
}
// Tile and split of 3x3 layer ci: workgroup count first (fill 256 CUs; PSM_UNET_FILL: another count, tools/attic/unet_bench.py sweeps),
// then the most reuse per workgroup.  The autotuner's tile choice (an index into the candidate list, -1 = by rule) goes first; the
// split rule below then runs for the tile that was chosen, not for the rule's.
// big_ok (round 6): the layer may take arrangement 2 (16 rows x 64 channels per workgroup, a 64 px x 64 channel register block per
// wave: half the LDS operand reads per MFMA and half the staged bytes per flop) -- bf16 mode, not the stem; whether its inputs
// really are finished bf16 activations is only known after every layer's split is (big_tiles_need_bf16_inputs falls back to the
// 8-row tile otherwise).  Rule from profiles/r06_conv_experiments.txt (2): only where such tiles still fill the chip AND the layer walks six or
// more channel chunks (64 cases of 256 x 256: dec3a 72.4 -> 65.4 us, enc4b 27.6 -> 24.4, dec2a 82.3 -> 78.5; shorter layers and
// every layer at 8 cases per step are slower with it).
void choose_config(Plan& p, size_t ci, bool can_split, bool x6_ok) {
  ConvLayer& c = p.L[ci];
  const ConvPlanEnv& env = p.env;
  const int H = p.H(c), W = p.W(c), ctiles = (c.cout + 15) / 16, forced = p.choice(ci, PSM_CHOICE_TILE);
  int chunk_ch = psm_conv_chunk_width(false, p.bf16);
  const bool big_ok = p.bf16 && !c.stem && c.src != 0;
  // an input arrives as split-K slabs (producers are planned before their consumers)
  const bool in_split = (c.src != 0 && ci > 0 && p.L[ci - 1].ksplit > 1) || (c.src == 3 && p.L[c.skip].ksplit > 1);
  struct Cand { int arr, nct; };
  const Cand cands[4] = {{0, 2}, {0, 1}, {1, 4}, {2, 4}};
  long best_score = -1;
  const bool use_forced = forced >= 0 && forced < (big_ok ? 4 : 3) && cands[forced].nct <= ctiles;
  if (use_forced) { c.arrangement = cands[forced].arr; c.nct = cands[forced].nct; c.groups = (ctiles + c.nct - 1) / c.nct; }
  for (int ki = 0; ki < 3 && !use_forced; ++ki) {
    const Cand& k = cands[ki];
    if (k.nct > ctiles) continue;                       // never compute padded channel tiles
    const int groups = (ctiles + k.nct - 1) / k.nct;
    const long wgs = psm_conv_wgs(H, W, k.arr, groups) * p.cases;
    const long reuse = (long)k.nct * psm_conv_tile_rows(k.arr);
    // equal workgroup count / reuse: the 2-row x 64-channel tile (arrangement 1), except for bf16 layers of four or more 32-channel chunks, where the
    // 8-row x 16-channel tile stages half the bytes per chunk for the same MFMAs and can take the in-workgroup K split (in_workgroup_k_split): enc4b at 8 cases
    // 8.9 us as 2 x 64, 7.7 us as 8 x 16, 6.8 us with the split on top; 512 x 512 x 1: enc3b 5.6 -> 5.0, dec3b 5.4 -> 4.6 us (profiles/r06_conv_experiments.txt (8));
    // PSM_UNET_KW=0: the planner without either change
    // (in_split: an input arrives as float32 partial-sum slabs -- the summing loader, no in-workgroup split: 512 x 512 x 1, enc4b behind a split enc4a, 10.1 us as 2 x 64, 11.2 us as 8 x 16)
    const bool long_bf16 = chunk_ch == 32 && !x6_ok && env.kw != 0 && !in_split && psm_conv_chunks(c.cin, chunk_ch) >= 4;
    const long tie = long_bf16 ? (k.arr == 0 && k.nct == 1 ? 1 : 0) : (k.arr ? 1 : 0);
    const long score = wgs >= env.fill ? 1000000 + reuse * 1000 + tie : wgs * 10 + tie;
    if (score > best_score) { best_score = score; c.arrangement = k.arr; c.nct = k.nct; c.groups = groups; }
  }
  if (!use_forced && big_ok && ctiles >= 4 && ctiles % 4 == 0 && psm_conv_chunks(c.cin, chunk_ch) >= 6 && !env.no_big_tiles &&
      psm_conv_wgs(H, W, 2, ctiles / 4) * p.cases >= env.fill) { c.arrangement = 2; c.nct = 4; c.groups = ctiles / 4; }
  c.x6 = x6_ok && c.arrangement == 0;                 // the x6 form exists for the 8-row tiles (psm_unet.hip)
  if (c.x6) chunk_ch = 32;
  c.n_chunks = psm_conv_chunks(c.cin, chunk_ch);
  // split the input channels over workgroups until the chip is filled (partial-sum slabs, see psm_unet.h); only
  // layers whose output feeds another convolution can be split, at most 8 ways (PSM_UNET_KSPLIT_MAX, the autotuner's cap)
  const long wgs = psm_conv_wgs(H, W, c.arrangement, c.groups) * p.cases;
  c.ksplit = 1;
  // chunks per split, at least: one for layers of four or more chunks, two below.  Measured at batch 1 against "two
  // everywhere": float32 174 -> 167 us, bf16 107 -> 98 us (the 16^2 layer with 4 chunks runs as 128 workgroups instead of
  // 64); one everywhere also splits the 2-chunk layers, whose consumers then read float32 slabs: bf16 105 us.  No change at
  // 8 cases per step.
  const int min_chunks = env.split_min_set ? env.split_min_chunks : (c.n_chunks >= 4 ? 1 : 2);
  // Whether a split pays is not decidable from the workgroup count alone: 512 x 512 batch 1 bf16, enc4b split in two runs in
  // 9.4 us against 9.2 us whole while its consumer dec3a then reads float32 partial-sum slabs through the summing loader
  // instead of finished bf16 activations (25.6 against 13.4 us); 256 x 256 batch 1, dec2a split in two: 9.0 against 14.3 us.
  // psm_unet_autotune measures it per layer (the split cap); this is the starting point.
  // (A bf16 layer that can take the IN-WORKGROUP split -- 8-row tile, four or more chunks, at most one workgroup per CU, inputs that are not slabs themselves -- is
  // not split over workgroups: its consumer keeps reading finished bf16 activations.  512 x 512 x 1: enc4a / enc4b / dec3a / dec3b 5.2 + 7.0 + 16.9 + 5.3 us with the
  // splits over workgroups the rule below starts from (the autotuner got them to 4.3 + 10.1 + 8.5 + 6.5), 6.3 + 6.4 + 8.5 + 5.3 us this way.)
  const bool kw_ok = chunk_ch == 32 && !c.x6 && env.kw != 0 && !in_split && c.arrangement == 0 && c.n_chunks >= 4 && wgs <= 256;
  const int ks_max = std::min(env.ksplit_max, p.choice(ci, PSM_CHOICE_KSPLIT_CAP));
  while (can_split && !kw_ok && wgs * c.ksplit < env.fill && c.ksplit < ks_max && c.n_chunks / (c.ksplit * 2) >= min_chunks) c.ksplit *= 2;
}
// per layer in network order (producers before their consumers): stem, x6 eligibility, tile and split, the forced override, head fusion
void tiles_and_splits(Plan& p) {
  for (size_t ci = 0; ci < p.L.size(); ++ci) {
    ConvLayer& c = p.L[ci];
    const bool feeds_conv3 = ci + 1 < p.L.size() && p.L[ci + 1].k == 3;
    c.stem = psm_conv_is_stem(c) && !p.env.no_stem;
    // x6 pays where the matrix work dominates: measured at 8 cases per step it halves the wide layers (dec3a 66 -> 43 us,
    // enc4b 31 -> 20 us) and loses on the 16-channel 256^2 layers (enc0b 30 -> 67 us: half of every 32-channel chunk is
    // padding and the three-plane tiles leave one workgroup per CU) -- rule: c_in >= 64; psm_unet_autotune measures the rest
    const int x6c = p.choice(ci, PSM_CHOICE_X6);
    const bool x6_ok = !p.bf16 && p.env.x6 && c.k == 3 && !c.stem && c.src != 0 && (x6c == 1 || (x6c < 0 && c.cin >= 64));
    if (c.k == 3) choose_config(p, ci, feeds_conv3 && !p.env.no_split, x6_ok);
    // diagnostic override: PSM_UNET_FORCE="layer:arrangement:nct:ksplit,..." (tools/attic/unet_bench.py experiments)
    for (const char* q = p.env.force.c_str(); q && *q; q = std::strchr(q, ',') ? std::strchr(q, ',') + 1 : nullptr) {
      int li, arr, nct, ks;
      if (std::sscanf(q, "%d:%d:%d:%d", &li, &arr, &nct, &ks) == 4 && li == (int)ci && c.k == 3 && psm_conv_tile_rows(arr) &&
          nct == psm_conv_tile_nct(arr, nct) && nct <= (c.cout + 15) / 16 && ks >= 1 && ks <= 8 && (ks == 1 || feeds_conv3) && ks <= c.n_chunks) {
        c.arrangement = arr; c.nct = nct; c.groups = ((c.cout + 15) / 16 + nct - 1) / nct;
        c.x6 = x6_ok && arr == 0;
        c.n_chunks = psm_conv_chunks(c.cin, psm_conv_chunk_width(c.x6, p.bf16));
        c.ksplit = std::min(ks, c.n_chunks);
      }
    }
    if (c.stem) { c.ksplit = 1; c.nct = 1; c.groups = 1; c.arrangement = 0; c.x6 = false; }
    c.fuse_head = c.k == 3 && ci + 1 < p.L.size() && p.L[ci + 1].k == 1 && c.cout == 16 && !c.stem && !p.env.no_head_fusion;
    if (c.fuse_head) { c.arrangement = 0; c.nct = 1; c.groups = 1; c.ksplit = 1; c.x6 = x6_ok; c.n_chunks = psm_conv_chunks(c.cin, psm_conv_chunk_width(c.x6, p.bf16)); }
  }
}
// the level of convolution i may become a fused pair: the autotuner's choice, else enough 30 x 14 tiles (PSM_UNET_PAIR_MIN)
bool pair_wanted(const Plan& p, size_t i) {
  const int pc = p.choice(i, PSM_CHOICE_PAIR);
  return pc > 0 || (pc < 0 && psm_pair_tiles(p.H(p.L[i]), p.W(p.L[i])) * p.cases >= p.env.pair_min);
}
// level pairs come first: two convolutions that the pair kernels could take (shape and tile count) are not split over K
// -- a pair has no slabs, and a level large enough for a pair fills the chip without them
void pair_candidates_release_splits(Plan& p) {
  for (size_t i = 0; p.bf16 && !p.env.no_pair && i + 1 < p.L.size(); ++i)
    if (psm_pair_shape(p.L[i], p.L[i + 1]) && pair_wanted(p, i)) p.L[i].ksplit = p.L[i + 1].ksplit = 1;
}
// bf16 activation storage (bf16 mode): a finished activation is stored as bf16 when every consumer reads bf16, i.e. is
// a 3x3 layer none of whose inputs arrives as split-K slabs (those loaders sum float32 slabs) and whose concatenation
// seam lies on a chunk boundary; a consumer with one float32 input takes all its inputs in float32.
void bf16_storage(Plan& p) {
  const size_t n = p.L.size();
  std::vector<char> obf(n, 0);
  for (size_t i = 0; i < n; ++i) obf[i] = (p.bf16 && p.L[i].k == 3 && p.L[i].ksplit == 1 && !p.env.f32_act) ? 1 : 0;
  for (bool changed = true; changed;) {
    changed = false;
    for (size_t i = 0; i < n; ++i) {
      ConvLayer& c = p.L[i];
      std::vector<int> ins;
      if (c.src != 0) ins.push_back((int)i - 1);
      if (c.src == 3) ins.push_back(c.skip);
      bool ok = c.k == 3 && !c.stem && c.src != 0;
      for (int j : ins) ok = ok && obf[j] && p.L[j].ksplit == 1;
      if (c.src == 3 && (p.L[i - 1].cout % 32) != 0) ok = false;                 // seam inside a 32-channel chunk
      if (c.k == 1 && i > 0 && p.L[i - 1].fuse_head) continue;                   // fused head reads registers
      c.in_bf = ok;
      if (!ok) for (int j : ins) if (obf[j]) { obf[j] = 0; changed = true; }
    }
  }
  for (size_t i = 0; i < n; ++i) p.L[i].out_bf = obf[i] != 0;
}
// arrangements 2-4 exist for finished bf16 inputs only (psm_unet.hip, launch_variant_abf): back to the 8-row tile otherwise
void big_tiles_need_bf16_inputs(Plan& p) {
  for (ConvLayer& c : p.L)
    if (c.k == 3 && c.arrangement >= 2 && !c.in_bf) { c.arrangement = 0; c.nct = 2; c.groups = ((c.cout + 15) / 16 + 1) / 2; }
}
// bytes of a zero-haloed bf16 tensor for the whole case batch: the pair kernels address it with 32-bit offsets
int64_t padded_bytes(int H, int W, int C, int cases) { return (int64_t)cases * (ACT_PADT + H + ACT_PADB) * (ACT_PADL + W + ACT_PADR) * C * 2; }
// fused level pairs (psm_unet_pair.hip): both 3x3 convolutions of a level in one launch, where the level is wide
// enough to fill the chip with 30 x 14 tiles and the shapes are ones the pair kernels are written for
void place_pairs(Plan& p) {
  for (ConvLayer& c : p.L) c.pair = 0;
  for (size_t i = 0; p.bf16 && !p.env.no_pair && i + 1 < p.L.size(); ++i) {
    ConvLayer& A = p.L[i]; ConvLayer& B = p.L[i + 1];
    if (!psm_pair_shape(A, B) || A.pair || B.pair || A.ksplit != 1 || B.ksplit != 1) continue;
    if (!(B.out_bf || B.fuse_head) || !pair_wanted(p, i)) continue;
    const int cm = A.cout, H = p.H(A), W = p.W(A);
    // the source transform names the kind; whether a kernel exists for these channel counts (and a fused head) is the
    // launcher's own predicate
    int kind = -1, c0 = A.cin, c1 = 0;
    if (A.src == 0) kind = PSM_PAIR_STEM;
    else if (A.src == 2 && A.in_bf) kind = PSM_PAIR_POOL;
    else if (A.src == 3 && A.in_bf) { kind = PSM_PAIR_UPCAT; c0 = p.L[i - 1].cout; c1 = p.L[A.skip].cout; }
    if (kind < 0 || !psm_pair_kernel_available(kind, cm, c0, c1, B.fuse_head)) continue;
    // the tile descriptors hold 32-bit byte offsets into the (zero-haloed) tensors of the whole case batch
    int64_t big = padded_bytes(H, W, cm, p.cases);
    if (kind == PSM_PAIR_POOL) big = std::max(big, padded_bytes(2 * H, 2 * W, c0, p.cases));
    if (kind == PSM_PAIR_UPCAT) big = std::max(big, std::max(padded_bytes(H / 2, W / 2, c0, p.cases), padded_bytes(H, W, c1, p.cases)));
    if (big >= ((int64_t)1 << 31)) continue;
    if (cm == 32 && !p.env.pair32) continue;            // PSM_UNET_PAIR32=0 (diagnostic): 16-channel pairs only
    A.pair = 1; A.pair_kind = kind; B.pair = 2;
  }
}
// in-workgroup K split (psm_conv3x3_kernel<..., KW = 2>): generic launches on finished bf16 inputs, 8-row tiles, two or more chunks, no split over workgroups
// Rule (profiles/r06_conv_experiments.txt (8)): four or more chunks AND at most one workgroup per CU -- an eight-wave workgroup holds 128 KB of LDS, so a
// launch of more than 256 of them runs in two rounds (dec2a at 8 cases, 512 workgroups: 11.6 -> 14.3 us), and a two-chunk layer has nothing to pipeline
// in a half (enc2b 6.0 -> 9.2 us).  PSM_UNET_KW=0 switches it off, PSM_UNET_KW=-n forces it for every eligible layer of n or more chunks (diagnostic).
void in_workgroup_k_split(Plan& p) {
  for (ConvLayer& c : p.L) {
    const bool can = p.bf16 && c.k == 3 && !c.stem && c.pair == 0 && !c.fuse_head && c.arrangement == 0 && c.in_bf && c.ksplit == 1 && c.n_chunks >= 2 && !c.x6;
    const long wgs = psm_conv_wgs(p.H(c), p.W(c), 0, c.groups) * p.cases;
    c.kw = !can || p.env.kw == 0 ? 1 : p.env.kw < 0 ? (c.n_chunks >= -p.env.kw ? 2 : 1) : (c.n_chunks >= 4 && wgs <= 256 ? 2 : 1);
  }
}
// bf16 tensors (finished activations of bf16 mode; a fused pair always writes bf16) get the zero halo
void act_layout(Plan& p) {
  for (ConvLayer& c : p.L) {
    const int H = p.H(c), W = p.W(c);
    c.padded = p.bf16 && c.k == 3 && (c.out_bf || c.pair != 0);
    c.P = c.padded ? ACT_PADL + W + ACT_PADR : W;
    c.case_elems = c.padded ? (int64_t)(ACT_PADT + H + ACT_PADB) * c.P * c.cout : (int64_t)H * W * c.cout;
    c.origin = c.padded ? ((int64_t)ACT_PADT * c.P + ACT_PADL) * c.cout : 0;
    c.slab = (int64_t)p.cases * H * W * c.cout;
  }
}
}  // namespace
int psm_unet_plan_layers(std::vector<ConvLayer>& layers, int c_in, int ny, int nx, int max_cases, bool bf16, const std::vector<int32_t>& choices, const ConvPlanEnv& env, std::string& why) {
  Plan p{layers, c_in, ny, nx, max_cases, bf16, choices, env};
  if (!case_tensors_fit(p, why)) return 1;
  tiles_and_splits(p);
  pair_candidates_release_splits(p);
  bf16_storage(p);
  big_tiles_need_bf16_inputs(p);
  place_pairs(p);
  in_workgroup_k_split(p);
  act_layout(p);
  return 0;
}
