// psm_unet_plan.h -- planner of the convolutional path (psm_unet_plan.cpp): every per-layer decision of psm_unet_plan as a pure
// function of the network, the image size, the case batch, the precision, the autotuner's choices and the PSM_UNET_* switches.
// No HIP: compiles with a plain C++17 compiler (tests/native/unet_plan_host.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// workgroup tile of an arrangement (psm_unet.h): rows, and the channel tiles per workgroup it runs with
inline int psm_conv_tile_rows(int arrangement) { return arrangement == 0 ? 8 : arrangement == 1 ? 2 : arrangement == 2 ? 16 : arrangement == 3 ? 16 : arrangement == 4 ? 8 : 0; }
inline int psm_conv_tile_nct(int arrangement, int nct) { return arrangement == 0 ? (nct == 2 ? 2 : 1) : arrangement == 3 ? 2 : 4; }
#define PSM_PAIR_TX 30          // fused level pairs (psm_unet_pair.hip): output tile of a workgroup (the mid tile is 32 x 16: two MFMA pixel tiles wide)
#define PSM_PAIR_TY 14
enum { PSM_PAIR_STEM = 0, PSM_PAIR_UPCAT = 1, PSM_PAIR_POOL = 2 };
// Which (kind, channel counts, fused head) combinations the pair kernels are instantiated for: the ONE predicate the planner and
// the launcher (psm_launch_conv_pair) share.
bool psm_pair_kernel_available(int kind, int cm, int c0, int c1, bool head);

// Finished bf16 activations (bf16 mode) live in ZERO-HALOED tensors: [case][ACT_PADT + H + ACT_PADB][ACT_PADL + W + ACT_PADR][C],
// the halo written once (memset at plan time) and never again -- every producer masks its stores to the image.  A consumer
// that stages whole tiles (the fused level pairs, psm_unet_pair.hip) then reads its halo -- the 'same' padding, the overhang of
// the last tile, a max-pool's doubled extent -- straight from memory: no clamps, no selects, and the tile can be moved by
// LDS-DMA, which cannot write zeros of its own.  The margins cover: 2 pixels of halo left / top at the tensor's own resolution
// and 4 when it is read through a 2x2 max-pool; right / bottom the last 30 x 14 tile's overhang + halo (32 / 16), doubled
// through a max-pool (64 / 32).  288 GB of HBM: the 20-45 % of extra footprint are never traffic.
constexpr int ACT_PADL = 4, ACT_PADT = 4, ACT_PADR = 64, ACT_PADB = 32;
// One convolution: its place in the network (psm_unet_layers) and everything psm_unet_plan_layers decides about it.
struct ConvLayer {
  int k = 3, cin = 0, cout = 0, level = 0;
  int src = 0;          // 0 input image, 1 previous conv, 2 max-pool of previous conv, 3 upsample(previous) ++ skip
  int skip = -1;        // conv index whose output is concatenated (src == 3)
  int relu = 1;
  int arrangement = 0, nct = 1, n_chunks = 0, groups = 1, ksplit = 1;   // launch configuration
  int kw = 1;                  // 2: in-workgroup K split (PsmConvArgs::kw)
  bool stem = false;            // K = 9*c_in flattened (first layer on the raw image)
  bool fuse_head = false;       // this layer's epilogue also computes the 1x1 head
  bool in_bf = false, out_bf = false;   // bf16 mode: inputs read / output stored as bf16 (finished activations only)
  bool x6 = false;              // float32 mode: this layer runs the x6 form (three bf16 planes per operand, chunks of 32 channels; 8-row tiles only)
  int pair = 0, pair_kind = 0;  // fused level pair (psm_unet_pair.hip): 1 = first convolution of a pair (its launch computes both), 2 = second (no launch)
  // layout of the output tensor (act_layout): finished bf16 activations are zero-haloed, everything else is dense
  bool padded = false;
  int P = 0;                   // row pitch (pixels)
  int64_t case_elems = 0, origin = 0;   // elements per case; element offset of pixel (0, 0) of case 0
  int64_t slab = 0;            // elements of one split-K slab: [max_cases][H][W][cout]
};
// The PSM_UNET_<NAME> planner switches (diagnostic; the rules of psm_unet_plan.cpp that read them say what they do), read from the
// process environment at every plan: tests change them between handles.  *_set / no_*: the variable exists.
struct ConvPlanEnv {
  long fill = 256, pair_min = 96;
  int ksplit_max = 8, kw = 1, split_min_chunks = 0;
  bool split_min_set = false, x6 = true, pair32 = true, no_big_tiles = false, no_pair = false, f32_act = false, no_stem = false, no_split = false, no_head_fusion = false;
  std::string force;
};
ConvPlanEnv psm_unet_plan_env();
// slots of the autotuner's choices, four per convolution (psm_unet_get_choices / psm_unet_set_choices)
enum { PSM_CHOICE_KSPLIT_CAP = 0, PSM_CHOICE_TILE = 1, PSM_CHOICE_PAIR = 2, PSM_CHOICE_X6 = 3 };
// enc0a, enc0b, ... enc{L-1}b, dec{L-2}a, ... dec0b, head (include/psm_unet.h)
std::vector<ConvLayer> psm_unet_layers(int c_in, int c_out, const std::vector<int>& widths);
// Plans every layer for [max_cases][ny][nx] images; choices: [4 * layers.size()].  0, or nonzero with `why` set (image too large).
int psm_unet_plan_layers(std::vector<ConvLayer>& layers, int c_in, int ny, int nx, int max_cases, bool bf16, const std::vector<int32_t>& choices, const ConvPlanEnv& env, std::string& why);
inline bool psm_conv_is_stem(const ConvLayer& c) { return c.k == 3 && c.src == 0 && 9 * c.cin <= 64 && c.cout <= 16; }
// two convolutions of one level that a pair kernel could take by shape
inline bool psm_pair_shape(const ConvLayer& a, const ConvLayer& b) { return a.k == 3 && b.k == 3 && b.src == 1 && a.level == b.level && b.cin == a.cout && b.cout == a.cout && (a.cout == 16 || a.cout == 32); }
inline long psm_pair_tiles(int H, int W) { return (long)((W + PSM_PAIR_TX - 1) / PSM_PAIR_TX) * ((H + PSM_PAIR_TY - 1) / PSM_PAIR_TY); }
inline int psm_conv_chunk_width(bool x6, bool bf16) { return x6 || bf16 ? 32 : 16; }
inline int psm_conv_chunks(int cin, int width) { return (cin + width - 1) / width; }
// workgroups of a generic 3x3 launch per case and split: 16-column tiles of the arrangement's rows, times the channel groups
inline long psm_conv_wgs(int H, int W, int arrangement, int groups) { const int th = psm_conv_tile_rows(arrangement); return (long)((W + 15) / 16) * ((H + th - 1) / th) * groups; }
// info[16] of psm_unet_plan_detail for layer c; pv / sk: the layers behind its inputs (nullptr where it has none)
void psm_unet_layer_detail(const ConvLayer& c, const ConvLayer* pv, const ConvLayer* sk, bool bf16, bool keep_act, int32_t v[16]);
