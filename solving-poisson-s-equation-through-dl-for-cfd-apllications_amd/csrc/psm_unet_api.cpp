// psm_unet_api.cpp -- handle, weight packing, forward pass and C-ABI of the convolutional path
// (include/psm_unet.h; kernels in psm_unet.hip; layer schedule and planner in psm_unet_plan.cpp).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "psm_alloc.h"

#include "../../include/psm.h"
#include "../../include/psm_unet.h"
#include "psm_unet.h"

namespace {
// One convolution: the planner's record (psm_unet_plan.h) with the host weights and what psm_unet_plan put on the device for it.
struct Conv : ConvLayer {
  Conv() = default;
  Conv(const ConvLayer& l) : ConvLayer(l) {}
  uint4* d_wpa = nullptr;       // pair leader: conv A's fragments
  uint4* d_wpb = nullptr;       // pair leader: conv B's fragments
  PsmPairTile* d_tiles = nullptr;   // pair leader: one descriptor per tile of the planned case batch (build_pair_tiles)
  std::vector<float> W, b;     // host copies (HWIO), kept for re-packing at plan time
  bool set = false;
  float4* d_w = nullptr;
  float* d_b = nullptr;
  float* d_w1 = nullptr;       // head: [cin][cout]
  float* d_out = nullptr;      // [ksplit][max_cases][H][W][cout] (ksplit > 1: partial-sum slabs, finished by the consumer's loader), laid out by the planner's act_layout
};
thread_local std::string g_err;
}  // namespace

struct psm_unet {
  int c_in = 0, c_out = 0, L = 0, device = 0;
  std::vector<int> widths;
  std::vector<Conv> convs;
  int ny = 0, nx = 0, max_cases = 0, last_cases = 0, bf16 = 0;
  bool planned = false;
  // per convolution {deepest split-K the planner may choose, tile -1 (planner's) / 0 (8 rows x 2 channel tiles) / 1 (8 x 1) / 2 (2 rows x 4), pair -1 (tile-count
  // rule) / 0 never / 1 whenever a kernel exists, x6 -1 (rule: c_in >= 64) / 0 float32 MFMA / 1 wherever the kernel exists} -- psm_unet_autotune, psm_unet_set_choices
  std::vector<int32_t> choices;
  bool keep_act = false;        // fused pairs also store what they would keep on chip (introspection for the parity tests)
  bool x6 = true;               // float32 mode: 8-row-tile layers run on the bf16 matrix pipe with exactly split operands (PSM_UNET_X6=0: float32 MFMA)
  float *d_in = nullptr, *d_field = nullptr, *h_in = nullptr, *h_out = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
};

namespace {
int fail(psm_unet* u, int code, const std::string& m) { if (u) u->err = m; else g_err = m; return code; }
#define UCHK(u, expr)                                                                                   \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail((u), PSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
void free_dev(void* p) { if (p) (void)psm_dev_free(p); }
// the packed operands of a convolution (upload_conv, build_pair_tiles); its activation tensor d_out is psm_unet_plan's
void free_conv_device(Conv& c) {
  for (void** p : {(void**)&c.d_w, (void**)&c.d_b, (void**)&c.d_w1, (void**)&c.d_wpa, (void**)&c.d_wpb, (void**)&c.d_tiles}) { free_dev(*p); *p = nullptr; }
}
template <class T, class V> int upload(psm_unet* u, T** p, const V& v) {      // a fresh device copy of the host vector v in *p
  free_dev(*p); *p = nullptr;
  UCHK(u, psm_dev_malloc((void**)p, v.size() * sizeof(v[0])));
  UCHK(u, psm_copy_h2d(*p, v.data(), v.size() * sizeof(v[0])));
  return PSM_OK;
}
// pixel (0, 0) of case 0 of a convolution's output, as the kernels' float pointer (bf16 tensors are addressed in 2-byte elements)
float* act_ptr(const Conv& c) {
  return c.padded ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(c.d_out) + c.origin) : c.d_out;
}

// Per-tile descriptors of a fused pair (PsmPairTile, psm_unet.h) for the planned case batch: tile t = (cs * tiles_y + by) * tiles_x + bx.
int build_pair_tiles(psm_unet* u, Conv& A, const Conv& B, const Conv* pv, const Conv* sk, int H, int W, int cases) {
  const int tx = (W + PSM_PAIR_TX - 1) / PSM_PAIR_TX, ty = (H + PSM_PAIR_TY - 1) / PSM_PAIR_TY;
  std::vector<PsmPairTile> t((size_t)cases * tx * ty);
  for (int cs = 0; cs < cases; ++cs)
    for (int by = 0; by < ty; ++by)
      for (int bx = 0; bx < tx; ++bx) {
        PsmPairTile& d = t[((size_t)cs * ty + by) * tx + bx];
        const int y0 = by * PSM_PAIR_TY, x0 = bx * PSM_PAIR_TX;
        d.y0 = y0; d.x0 = x0; d.cs = cs;
        d.pix = (cs * H + y0) * W + x0;
        d.flags = (x0 >= 2 && x0 + 33 <= W && y0 >= 2 && y0 + 16 <= H) ? 1 : 0;
        d.offo = (int)(((int64_t)cs * B.case_elems + ((int64_t)y0 * B.P + x0) * B.cout) * 2);
        d.off0 = d.off1 = 0;
        if (A.pair_kind == PSM_PAIR_UPCAT) {
          d.off0 = (int)(((int64_t)cs * pv->case_elems + ((int64_t)(y0 / 2 - 1) * pv->P + (x0 / 2 - 1)) * pv->cout) * 2);
          d.off1 = (int)(((int64_t)cs * sk->case_elems + ((int64_t)(y0 - 2) * sk->P + (x0 - 2)) * sk->cout) * 2);
        } else if (A.pair_kind == PSM_PAIR_POOL) {
          d.off0 = (int)(((int64_t)cs * pv->case_elems + ((int64_t)(2 * y0 - 4) * pv->P + (2 * x0 - 4)) * pv->cout) * 2);
        }
      }
  return upload(u, &A.d_tiles, t);
}

uint16_t f2bf(float f) {       // round to nearest even, like v_cvt_pk_bf16_f32
  uint32_t u; std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf2f(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f; }
// Operands of the generic 3x3 kernels in MFMA order: wpack[cog][chunk g of 4 J][plane][tap][ct][lane][j < J] =
// plane(W[tap][4 J g + J (lane >> 4) + j][16 (cog nct + ct) + (lane & 15)]), zero beyond c_in / c_out.  split(w, planes) writes a weight's planes:
//   float32: J = 4 (chunks of 16 channels), the float itself;   bf16: J = 8 (chunks of 32), the weight rounded to bf16;
//   x6 (float32 mode on the bf16 matrix pipe): J = 8, every weight split exactly into hi + mid + lo bf16 planes
template <class T, int J, int PLANES, class Split>
std::vector<T> pack_conv3x3(const Conv& c, Split split) {
  const int chunks = c.n_chunks, nct = c.nct, groups = c.groups;
  std::vector<T> p((size_t)groups * chunks * PLANES * 9 * nct * 64 * J, 0);
  for (int cog = 0; cog < groups; ++cog) for (int g = 0; g < chunks; ++g) for (int tap = 0; tap < 9; ++tap)
    for (int ct = 0; ct < nct; ++ct) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < J; ++j) {
      const int ci = 4 * J * g + J * (lane >> 4) + j, co = 16 * (cog * nct + ct) + (lane & 15);
      if (ci >= c.cin || co >= c.cout) continue;
      T pl[PLANES];
      split(c.W[((size_t)tap * c.cin + ci) * c.cout + co], pl);
      for (int q = 0; q < PLANES; ++q) p[((((((size_t)cog * chunks + g) * PLANES + q) * 9 + tap) * nct + ct) * 64 + lane) * J + j] = pl[q];
    }
  return p;
}
void split_x6(float w, uint16_t* pl) {                  // both remainders are exact
  const float r1 = w - bf2f(pl[0] = f2bf(w)), r2 = r1 - bf2f(pl[1] = f2bf(r1));
  pl[2] = f2bf(r2);
}
// stem: wpack[g][lane][j] = W[k = 16g + 4*(lane>>4) + j -> (tap = k / c_in, ci = k % c_in)][co = lane & 15]
std::vector<float> pack_stem(const Conv& c, bool bf16) {
  const int K = 9 * c.cin, kg = (K + 15) / 16;
  std::vector<float> p((size_t)kg * 64 * 4, 0.f);
  for (int g = 0; g < kg; ++g) for (int lane = 0; lane < 64; ++lane) for (int j = 0; j < 4; ++j) {
    const int k = 16 * g + 4 * (lane >> 4) + j, co = lane & 15;
    if (k >= K || co >= c.cout) continue;
    const float w = c.W[((size_t)(k / c.cin) * c.cin + (k % c.cin)) * c.cout + co];
    p[((size_t)g * 64 + lane) * 4 + j] = bf16 ? bf2f(f2bf(w)) : w;
  }
  return p;
}

// Fragments of the fused-pair kernels (psm_unet_pair.hip): 64 lanes x 8 bf16 each, the MFMA's FIRST operand: lane l holds
// W[tap][ci(l >> 4, j)][co = 16*nt + (l & 15)], j < 8.
//   stem (flat):        step s:            k = 32 s + 8 (l >> 4) + j -> (tap = k / c_in, ci = k % c_in), zero beyond 9 c_in
//   32-channel chunk:   [kx][ky][nt]:      ci = base + 8 (l >> 4) + j
//   16-channel chunk:   [pair s][ky][nt]:  kx = 2 s + (l >> 5), ci = base + 8 ((l >> 4) & 1) + j, zero for kx = 3
// Chunks: the channels of in0 then of in1 (c0 + c1 = c.cin), 32 at a time while they last, then one of 16.
std::vector<uint16_t> pack_pair(const Conv& c, bool flat, int c0, int c1) {
  const int NT = c.cout / 16;
  std::vector<uint16_t> p;
  auto frag = [&](auto&& wat) {                       // wat(kq, j, co) -> weight
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) p.push_back(f2bf(wat(lane >> 4, j, lane & 15)));
  };
  auto W = [&](int tap, int ci, int co) { return c.W[((size_t)tap * c.cin + ci) * c.cout + co]; };
  if (flat) {
    const int K = 9 * c.cin;
    for (int s = 0; s < (K + 31) / 32; ++s)
      frag([&](int kq, int j, int co) { const int k = 32 * s + 8 * kq + j; return k < K ? W(k / c.cin, k % c.cin, co) : 0.f; });
    return p;
  }
  for (int part = 0; part < 2; ++part) {
    const int cn = part == 0 ? c0 : c1, base = part == 0 ? 0 : c0;
    for (int cb = 0; cb < cn; cb += 32) {
      if (cn - cb >= 32) {
        for (int kx = 0; kx < 3; ++kx) for (int ky = 0; ky < 3; ++ky) for (int nt = 0; nt < NT; ++nt)
          frag([&](int kq, int j, int co) { return W(ky * 3 + kx, base + cb + 8 * kq + j, 16 * nt + co); });
      } else {
        for (int s = 0; s < 2; ++s) for (int ky = 0; ky < 3; ++ky) for (int nt = 0; nt < NT; ++nt)
          frag([&](int kq, int j, int co) { const int kx = 2 * s + (kq >> 1); return kx < 3 ? W(ky * 3 + kx, base + cb + 8 * (kq & 1) + j, 16 * nt + co) : 0.f; });
      }
    }
  }
  return p;
}

int upload_conv(psm_unet* u, Conv& c) {
  free_conv_device(c);
  std::vector<float> bias((size_t)((c.cout + 15) / 16 + 4) * 16, 0.f);
  std::memcpy(bias.data(), c.b.data(), c.cout * sizeof(float));
  int rc = upload(u, &c.d_b, bias);
  if (rc) return rc;
  if (c.k != 3) rc = upload(u, &c.d_w1, c.W);
  else if (c.stem) rc = upload(u, &c.d_w, pack_stem(c, u->bf16 != 0));
  else if (c.x6) rc = upload(u, &c.d_w, pack_conv3x3<uint16_t, 8, 3>(c, split_x6));
  else if (u->bf16) rc = upload(u, &c.d_w, pack_conv3x3<uint16_t, 8, 1>(c, [](float w, uint16_t* pl) { pl[0] = f2bf(w); }));
  else rc = upload(u, &c.d_w, pack_conv3x3<float, 4, 1>(c, [](float w, float* pl) { pl[0] = w; }));
  if (rc || c.pair != 1) return rc;
  const size_t ci = &c - u->convs.data();
  const Conv& B = u->convs[ci + 1];
  int c0 = c.cin, c1 = 0;
  if (c.pair_kind == PSM_PAIR_UPCAT) { c0 = u->convs[ci - 1].cout; c1 = u->convs[c.skip].cout; }
  if ((rc = upload(u, &c.d_wpa, pack_pair(c, c.pair_kind == PSM_PAIR_STEM, c0, c1)))) return rc;
  return upload(u, &c.d_wpb, pack_pair(B, false, B.cin, 0));
}

int forward(psm_unet* u, const float* d_grid, int n, float* d_field, hipStream_t st, hipEvent_t* ev = nullptr, int n_layers = -1) {
  const size_t n_run = n_layers < 0 ? u->convs.size() : (size_t)n_layers;
  for (size_t i = 0; i < n_run; ++i) {
    if (ev) UCHK(u, hipEventRecord(ev[i], st));
    if (psm_launch_probe) psm_launch_probe->tag = (int)i;
    Conv& c = u->convs[i];
    const int H = u->ny >> c.level, W = u->nx >> c.level;
    float* out = (i + 1 == u->convs.size()) ? d_field : act_ptr(c);
    if (c.pair == 2) continue;                                // computed by the pair's first convolution's launch
    if (c.pair == 1) {
      const Conv& B = u->convs[i + 1];
      PsmPairArgs p{};
      p.wA = c.d_wpa; p.wB = c.d_wpb; p.biasA = c.d_b; p.biasB = B.d_b;
      p.H = H; p.W = W; p.tiles_x = (W + PSM_PAIR_TX - 1) / PSM_PAIR_TX; p.tiles_y = (H + PSM_PAIR_TY - 1) / PSM_PAIR_TY; p.n_cases = n;
      p.out_case = B.case_elems; p.PO = B.P;                // conv A's kept activation (mid_out) has the same layout
      p.tiles = c.d_tiles; p.cm = c.cout;
      p.out = (B.fuse_head && !u->keep_act) ? nullptr : reinterpret_cast<unsigned short*>(act_ptr(B));
      p.mid_out = u->keep_act ? reinterpret_cast<unsigned short*>(act_ptr(c)) : nullptr;
      if (c.pair_kind == PSM_PAIR_STEM) { p.in0 = d_grid; p.c0 = c.cin; p.in0_case = (int64_t)H * W * c.cin; p.P0 = W; }
      else {
        const Conv& pv = u->convs[i - 1];
        p.in0 = act_ptr(pv); p.c0 = pv.cout; p.in0_case = pv.case_elems; p.P0 = pv.P;
        if (c.pair_kind == PSM_PAIR_UPCAT) { const Conv& sk = u->convs[c.skip]; p.in1 = act_ptr(sk); p.c1 = sk.cout; p.in1_case = sk.case_elems; p.P1 = sk.P; }
      }
      if (B.fuse_head) {
        const Conv& hd = u->convs[i + 2];
        p.head_w = hd.d_w1; p.head_b = hd.d_b; p.head_out = d_field; p.head_cout = hd.cout; p.head_case = (int64_t)H * W * hd.cout;
      }
      UCHK(u, psm_launch_conv_pair(p, c.pair_kind, c.cout, n, st));
      continue;
    }
    if (c.k == 1) {
      if (u->convs[i - 1].fuse_head) continue;               // computed in the previous layer's epilogue
      PsmHeadArgs ha{u->convs[i - 1].d_out, c.d_w1, c.d_b, out, (int64_t)n * H * W, c.cin, c.cout};     // its input is float32 (dense) by the planner's rule
      UCHK(u, psm_launch_head1x1(ha, st));
      continue;
    }
    PsmConvArgs a{};
    a.wpack = c.d_w; a.bias = c.d_b; a.out = out; a.n_chunks = c.n_chunks; a.H = H; a.W = W; a.cout = c.cout; a.relu = c.relu;
    a.out_case = (i + 1 == u->convs.size()) ? (int64_t)H * W * c.cout : c.case_elems;
    a.PO = (i + 1 == u->convs.size()) ? W : c.P;
    a.kw = c.kw; a.ksplit = c.ksplit; a.out_slab = c.slab; a.ks0 = 1; a.ks1 = 1; a.bf16 = u->bf16;
    a.in_bf = c.in_bf ? 1 : 0; a.out_bf = c.out_bf ? 1 : 0; a.x6 = c.x6 ? 1 : 0;
    if (c.src == 0) { a.in0 = d_grid; a.c0 = c.cin; a.mode0 = PSM_SRC_SAME; a.H0 = H; a.W0 = W; a.P0 = W; a.in0_case = (int64_t)H * W * c.cin; }
    else {
      const Conv& pv = u->convs[i - 1];
      a.in0 = act_ptr(pv); a.c0 = pv.cout; a.ks0 = pv.ksplit; a.slab0 = pv.slab; a.pbias0 = pv.d_b; a.P0 = pv.P; a.in0_case = pv.case_elems;
      if (c.src == 1) { a.mode0 = PSM_SRC_SAME; a.H0 = H; a.W0 = W; }
      else if (c.src == 2) { a.mode0 = PSM_SRC_MAXPOOL; a.H0 = 2 * H; a.W0 = 2 * W; }
      else { const Conv& sk = u->convs[c.skip];
             a.mode0 = PSM_SRC_UPSAMPLE; a.H0 = H / 2; a.W0 = W / 2; a.in1 = act_ptr(sk); a.c1 = sk.cout;
             a.ks1 = sk.ksplit; a.slab1 = sk.slab; a.pbias1 = sk.d_b; a.in1_case = sk.case_elems; a.P1 = sk.P; }
    }
    if (c.fuse_head) {
      const Conv& hd = u->convs[i + 1];
      a.head_w = hd.d_w1; a.head_b = hd.d_b; a.head_out = d_field; a.head_cout = hd.cout; a.head_case = (int64_t)H * W * hd.cout;
    }
    if (c.stem) UCHK(u, psm_launch_conv_stem(a, n, st));
    else UCHK(u, psm_launch_conv3x3(a, c.arrangement, c.nct, n, st));
  }
  if (ev) UCHK(u, hipEventRecord(ev[u->convs.size()], st));
  u->last_cases = n;
  return PSM_OK;
}
}  // namespace

extern "C" {

const char* psm_unet_last_error(const psm_unet* u) { return u ? u->err.c_str() : g_err.c_str(); }

int psm_unet_create(int32_t c_in, int32_t c_out, int32_t n_levels, const int32_t* widths, int32_t device, psm_unet** out) {
  if (!out || !widths) return fail(nullptr, PSM_ERR_ARG, "null argument");
  *out = nullptr;
  if (c_in < 1 || c_in > 16 || c_out < 1 || c_out > 16) return fail(nullptr, PSM_ERR_ARG, "c_in / c_out must be 1..16");
  if (n_levels < 2 || n_levels > 7) return fail(nullptr, PSM_ERR_ARG, "n_levels must be 2..7");
  for (int l = 0; l < n_levels; ++l)
    if (widths[l] < 16 || widths[l] > 1024 || widths[l] % 16) return fail(nullptr, PSM_ERR_ARG, "widths must be multiples of 16 in [16, 1024]");
  if (widths[0] > 64) return fail(nullptr, PSM_ERR_ARG, "first-level width above 64 is not supported by the 1x1 head");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, PSM_ERR_NO_DEVICE, "no HIP device: the convolutional path has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, PSM_ERR_ARG, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, PSM_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(nullptr, PSM_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  psm_unet* u = new psm_unet();
  u->c_in = c_in; u->c_out = c_out; u->L = n_levels; u->device = device;
  u->widths.assign(widths, widths + n_levels);
  const std::vector<ConvLayer> layers = psm_unet_layers(c_in, c_out, u->widths);
  u->convs.assign(layers.begin(), layers.end());
  u->choices.assign(4 * layers.size(), -1);                                     // by rule, and
  for (size_t i = 0; i < layers.size(); ++i) u->choices[4 * i + PSM_CHOICE_KSPLIT_CAP] = 8;   // any split
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&u->stream, hipStreamNonBlocking) != hipSuccess) {
    delete u;
    return fail(nullptr, PSM_ERR_HIP, "cannot create a stream on the device");
  }
  *out = u;
  return PSM_OK;
}

void psm_unet_destroy(psm_unet* u) {
  if (!u) return;
  (void)hipSetDevice(u->device);
  if (u->stream) (void)hipStreamSynchronize(u->stream);
  for (Conv& c : u->convs) { free_conv_device(c); free_dev(c.d_out); }
  free_dev(u->d_in); free_dev(u->d_field);
  if (u->h_in) (void)hipHostFree(u->h_in);
  if (u->h_out) (void)hipHostFree(u->h_out);
  if (u->stream) (void)hipStreamDestroy(u->stream);
  delete u;
}

int psm_unet_num_convs(const psm_unet* u) { return u ? (int)u->convs.size() : PSM_ERR_ARG; }

int psm_unet_conv_shape(const psm_unet* u, int32_t idx, int32_t* k, int32_t* c_in, int32_t* c_out) {
  if (!u || idx < 0 || idx >= (int)u->convs.size() || !k || !c_in || !c_out) return PSM_ERR_ARG;
  *k = u->convs[idx].k; *c_in = u->convs[idx].cin; *c_out = u->convs[idx].cout;
  return PSM_OK;
}

int psm_unet_set_conv(psm_unet* u, int32_t idx, const float* weight, const float* bias) {
  if (!u) return PSM_ERR_ARG;
  if (idx < 0 || idx >= (int)u->convs.size()) return fail(u, PSM_ERR_ARG, "convolution index out of range");
  if (!weight || !bias) return fail(u, PSM_ERR_ARG, "null weights");
  Conv& c = u->convs[idx];
  c.W.assign(weight, weight + (size_t)c.k * c.k * c.cin * c.cout);
  c.b.assign(bias, bias + c.cout);
  c.set = true;
  if (u->planned) { UCHK(u, hipSetDevice(u->device)); return upload_conv(u, c); }
  return PSM_OK;
}

int psm_unet_set_precision(psm_unet* u, int32_t precision) {
  if (!u) return PSM_ERR_ARG;
  if (precision != PSM_PRECISION_F32 && precision != PSM_PRECISION_BF16) return fail(u, PSM_ERR_ARG, "unknown precision");
  if (u->planned) return fail(u, PSM_ERR_STATE, "set the precision before psm_unet_plan");
  u->bf16 = precision == PSM_PRECISION_BF16 ? 1 : 0;
  return PSM_OK;
}

int psm_unet_keep_activations(psm_unet* u, int32_t on) {
  if (!u) return PSM_ERR_ARG;
  if (u->planned) return fail(u, PSM_ERR_STATE, "call psm_unet_keep_activations before psm_unet_plan");
  u->keep_act = on != 0;
  return PSM_OK;
}

int psm_unet_plan(psm_unet* u, int32_t ny, int32_t nx, int32_t max_cases) {
  if (!u) return PSM_ERR_ARG;
  for (const Conv& c : u->convs) if (!c.set) return fail(u, PSM_ERR_STATE, "model incomplete: call psm_unet_set_conv for every convolution first");
  const int m = 1 << (u->L - 1);
  if (ny < m || nx < m || ny % m || nx % m) return fail(u, PSM_ERR_ARG, "ny and nx must be multiples of 2^(n_levels-1)");
  if (max_cases < 1 || (int64_t)ny * nx * max_cases > ((int64_t)1 << 28)) return fail(u, PSM_ERR_ARG, "bad case batch");
  const ConvPlanEnv env = psm_unet_plan_env();
  std::vector<ConvLayer> plan(u->convs.begin(), u->convs.end());
  std::string why;
  if (psm_unet_plan_layers(plan, u->c_in, ny, nx, max_cases, u->bf16 != 0, u->choices, env, why)) return fail(u, PSM_ERR_ARG, why);
  UCHK(u, hipSetDevice(u->device));
  UCHK(u, hipStreamSynchronize(u->stream));
  u->ny = ny; u->nx = nx; u->max_cases = max_cases; u->x6 = env.x6;
  for (size_t ci = 0; ci < plan.size(); ++ci) static_cast<ConvLayer&>(u->convs[ci]) = plan[ci];
  // realise the plan: packed weights, pair tiles (their offsets need every layer's layout), activation tensors
  for (size_t ci = 0; ci < u->convs.size(); ++ci) {
    Conv& c = u->convs[ci];
    int rc = upload_conv(u, c);
    if (rc) return rc;
    if (c.pair == 1 && (rc = build_pair_tiles(u, c, u->convs[ci + 1], c.src != 0 ? &u->convs[ci - 1] : nullptr, c.src == 3 ? &u->convs[c.skip] : nullptr,
                                              ny >> c.level, nx >> c.level, max_cases))) return rc;
    free_dev(c.d_out); c.d_out = nullptr;
    if (c.padded) {
      const size_t bytes = (size_t)max_cases * c.case_elems * sizeof(uint16_t) + 4096;      // + slack: a tile's last LDS-DMA piece may start past its last row
      UCHK(u, psm_dev_malloc((void**)&c.d_out, bytes));
      UCHK(u, hipMemsetAsync(c.d_out, 0, bytes, u->stream));                                // the zero halo, written once
      UCHK(u, hipStreamSynchronize(u->stream));
    } else UCHK(u, psm_dev_malloc((void**)&c.d_out, (size_t)c.ksplit * c.slab * sizeof(float) + 64));
  }
  free_dev(u->d_in); free_dev(u->d_field);
  if (u->h_in) { (void)hipHostFree(u->h_in); u->h_in = nullptr; }
  if (u->h_out) { (void)hipHostFree(u->h_out); u->h_out = nullptr; }
  const size_t npix = (size_t)ny * nx * max_cases;
  UCHK(u, psm_dev_malloc((void**)&u->d_in, npix * u->c_in * sizeof(float)));
  UCHK(u, psm_dev_malloc((void**)&u->d_field, npix * u->c_out * sizeof(float)));
  UCHK(u, hipHostMalloc((void**)&u->h_in, npix * u->c_in * sizeof(float), hipHostMallocDefault));
  UCHK(u, hipHostMalloc((void**)&u->h_out, npix * u->c_out * sizeof(float), hipHostMallocDefault));
  u->planned = true;
  return PSM_OK;
}

int psm_unet_forward_device(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, void* stream) {
  if (!u) return PSM_ERR_ARG;
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  if (!d_grid || !d_field) return fail(u, PSM_ERR_ARG, "null buffer");
  if (n_cases < 1 || n_cases > u->max_cases) return fail(u, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  UCHK(u, hipSetDevice(u->device));
  return forward(u, d_grid, n_cases, d_field, stream ? (hipStream_t)stream : u->stream);
}

int psm_unet_forward(psm_unet* u, const float* grid, int32_t n_cases, float* field) {
  if (!u) return PSM_ERR_ARG;
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  if (!grid || !field) return fail(u, PSM_ERR_ARG, "null buffer");
  if (n_cases < 1 || n_cases > u->max_cases) return fail(u, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  UCHK(u, hipSetDevice(u->device));
  const size_t npix = (size_t)u->ny * u->nx * n_cases;
  std::memcpy(u->h_in, grid, npix * u->c_in * sizeof(float));
  UCHK(u, hipMemcpyAsync(u->d_in, u->h_in, npix * u->c_in * sizeof(float), hipMemcpyHostToDevice, u->stream));
  int rc = forward(u, u->d_in, n_cases, u->d_field, u->stream);
  if (rc) return rc;
  UCHK(u, hipMemcpyAsync(u->h_out, u->d_field, npix * u->c_out * sizeof(float), hipMemcpyDeviceToHost, u->stream));
  {   // synchronous call of a few hundred us: poll instead of sleeping (see psm_api_solve.cpp, wait_stream); PSM_SYNC_BLOCK=1 blocks
    static const bool block = getenv("PSM_SYNC_BLOCK") != nullptr;
    hipError_t e = hipSuccess;
    if (block) e = hipStreamSynchronize(u->stream);
    else while ((e = hipStreamQuery(u->stream)) == hipErrorNotReady) { }
    UCHK(u, e);
  }
  std::memcpy(field, u->h_out, npix * u->c_out * sizeof(float));
  return PSM_OK;
}

int psm_unet_synchronize(psm_unet* u) {
  if (!u) return PSM_ERR_ARG;
  UCHK(u, hipSetDevice(u->device));
  UCHK(u, hipStreamSynchronize(u->stream));
  return PSM_OK;
}

int psm_unet_read_activation(psm_unet* u, int32_t idx, float* dst, int64_t dst_floats) {
  if (!u || !dst) return PSM_ERR_ARG;
  if (!u->planned || u->last_cases < 1) return fail(u, PSM_ERR_STATE, "no forward pass yet");
  if (idx < 0 || idx + 1 >= (int)u->convs.size()) return fail(u, PSM_ERR_ARG, "activation index out of range (the head's output is the field)");
  const Conv& c = u->convs[idx];
  if (!u->keep_act && (c.pair == 1 || (c.pair == 2 && c.fuse_head)))
    return fail(u, PSM_ERR_STATE, "this activation stays on chip (fused level pair): call psm_unet_keep_activations(u, 1) before psm_unet_plan");
  const int64_t n = (int64_t)u->last_cases * (u->ny >> c.level) * (u->nx >> c.level) * c.cout;
  if (dst_floats < n) return fail(u, PSM_ERR_ARG, "destination too small");
  UCHK(u, hipSetDevice(u->device));
  UCHK(u, hipStreamSynchronize(u->stream));
  if (c.padded) {                 // stored as bf16 in a zero-haloed tensor (act_layout): take the image rows, widen
    const int H = u->ny >> c.level, W = u->nx >> c.level;
    std::vector<uint16_t> hb((size_t)u->last_cases * c.case_elems);
    UCHK(u, psm_copy_d2h(hb.data(), c.d_out, hb.size() * sizeof(uint16_t)));
    for (int cs = 0; cs < u->last_cases; ++cs)
      for (int y = 0; y < H; ++y) {
        const uint16_t* row = hb.data() + (size_t)cs * c.case_elems + c.origin + (size_t)y * c.P * c.cout;
        float* d = dst + ((size_t)cs * H + y) * W * c.cout;
        for (int q = 0; q < W * c.cout; ++q) d[q] = bf2f(row[q]);
      }
    return PSM_OK;
  }
  UCHK(u, psm_copy_d2h(dst, c.d_out, n * sizeof(float)));
  if (c.ksplit > 1) {            // partial-sum slabs: finish like the consumer's loader (slab order, bias, ReLU)
    std::vector<float> tmp(n);
    for (int s = 1; s < c.ksplit; ++s) {
      UCHK(u, psm_copy_d2h(tmp.data(), c.d_out + (int64_t)s * c.slab, n * sizeof(float)));
      for (int64_t q = 0; q < n; ++q) dst[q] += tmp[q];
    }
    for (int64_t q = 0; q < n; ++q) { const float v = dst[q] + c.b[q % c.cout]; dst[q] = v > 0.f ? v : 0.f; }
  }
  return PSM_OK;
}

int psm_unet_profile(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, float* ms, int32_t* wgs) {
  if (!u || !ms) return PSM_ERR_ARG;
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  if (!d_grid || !d_field || n_cases < 1 || n_cases > u->max_cases) return fail(u, PSM_ERR_ARG, "bad arguments");
  UCHK(u, hipSetDevice(u->device));
  std::vector<hipEvent_t> ev(u->convs.size() + 1);
  for (auto& e : ev) UCHK(u, hipEventCreate(&e));
  int rc = forward(u, d_grid, n_cases, d_field, u->stream, ev.data());
  if (rc == PSM_OK) {
    hipError_t e = hipStreamSynchronize(u->stream);
    if (e != hipSuccess) rc = fail(u, PSM_ERR_HIP, hipGetErrorString(e));
  }
  for (size_t i = 0; rc == PSM_OK && i < u->convs.size(); ++i) {
    (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    if (wgs) {
      const Conv& c = u->convs[i];
      const int H = u->ny >> c.level, W = u->nx >> c.level;
      wgs[i] = c.pair == 1 ? (int32_t)psm_pair_tiles(H, W) * n_cases : (c.k != 3 || c.pair == 2) ? 0 : (int32_t)psm_conv_wgs(H, W, c.arrangement, c.groups) * c.ksplit * n_cases;
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

// every dispatch of `steps` forward passes with its own begin / end stamps: per convolution that owns a launch, the samples in ms
static int unet_collect_samples(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, int32_t steps,
                                std::vector<std::vector<float>>& samp, char* names) {
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  if (!d_grid || !d_field || n_cases < 1 || n_cases > u->max_cases) return fail(u, PSM_ERR_ARG, "bad arguments");
  UCHK(u, hipSetDevice(u->device));
  UCHK(u, hipStreamSynchronize(u->stream));
  const size_t nc = u->convs.size();
  samp.assign(nc, {});
  if (names) std::memset(names, 0, nc * 64);
  PsmLaunchProbe probe;
  auto drain = [&]() -> int {
    UCHK(u, hipStreamSynchronize(u->stream));
    for (auto& r : probe.recs) {
      float t = 0.f;
      if (r.tag >= 0 && r.tag < (int)nc && hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) {
        samp[r.tag].push_back(t);
        if (names && !names[(size_t)r.tag * 64]) {
          std::string nm(r.name);
          while (!nm.empty() && (nm[0] == '(' || nm[0] == ' ')) nm.erase(0, 1);
          while (!nm.empty() && (nm.back() == ')' || nm.back() == ' ')) nm.pop_back();
          std::snprintf(names + (size_t)r.tag * 64, 64, "%s", nm.c_str());
        }
      }
      probe.pool.push_back(r.e0); probe.pool.push_back(r.e1);
    }
    probe.recs.clear();
    return PSM_OK;
  };
  int rc = PSM_OK;
  psm_launch_probe = &probe;
  for (int i = 0; i < steps && rc == PSM_OK; ++i) {
    rc = forward(u, d_grid, n_cases, d_field, u->stream);
    if (rc == PSM_OK && (i % 16) == 15) rc = drain();
  }
  psm_launch_probe = nullptr;
  if (rc == PSM_OK) rc = drain(); else (void)hipStreamSynchronize(u->stream);
  for (auto& r : probe.recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto e : probe.pool) (void)hipEventDestroy(e);
  return rc;
}

// per launch the MEAN of its dispatch durations (microseconds), or the MEDIAN and the 10th / 90th percentile
static int unet_time(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, int32_t steps, double* mean_us, double* median_us, double* p10_us,
                     double* p90_us, int32_t* launches, char* names) {
  if (!u || !(mean_us || median_us) || steps < 1) return PSM_ERR_ARG;
  std::vector<std::vector<float>> samp;
  int rc = unet_collect_samples(u, d_grid, n_cases, d_field, steps, samp, names);
  for (size_t i = 0; !rc && i < samp.size(); ++i) {
    std::vector<float>& v = samp[i];
    const size_t n = v.size();
    double tot = 0.0;
    for (float t : v) tot += t;
    std::sort(v.begin(), v.end());
    auto q = [&](double f) { return n ? (double)v[std::min(n - 1, (size_t)(f * (double)(n - 1) + 0.5))] * 1e3 : 0.0; };
    if (mean_us) mean_us[i] = n ? tot / (double)n * 1e3 : 0.0;
    if (median_us) median_us[i] = q(0.5);
    if (p10_us) p10_us[i] = q(0.1);
    if (p90_us) p90_us[i] = q(0.9);
    if (launches) launches[i] = (int32_t)(n / (size_t)steps);
  }
  return rc;
}
int psm_unet_time_kernels(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, int32_t steps, double* us, int32_t* launches, char* names) {
  return unet_time(u, d_grid, n_cases, d_field, steps, us, nullptr, nullptr, nullptr, launches, names);
}
int psm_unet_time_kernels_q(psm_unet* u, const float* d_grid, int32_t n_cases, float* d_field, int32_t steps, double* median_us, double* p10_us, double* p90_us, int32_t* launches, char* names) {
  return unet_time(u, d_grid, n_cases, d_field, steps, nullptr, median_us, p10_us, p90_us, launches, names);
}

// Plan-time autotune of the split-K depth: the planner splits the input channels of a layer that cannot fill the chip over up
// to 8 workgroups, which shortens that layer but makes its consumer sum float32 partial-sum slabs; whether the pair comes
// out ahead depends on both layers' shapes.  Measured, not guessed: for every split layer, in network order, halve the cap
// while the whole forward pass (median of `iters` passes of n_cases zero images) gets faster by more than 1 %.
int psm_unet_autotune(psm_unet* u, int32_t n_cases, int32_t iters, float* us_before, float* us_after) {
  if (!u) return PSM_ERR_ARG;
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  if (n_cases < 1 || n_cases > u->max_cases || iters < 1) return fail(u, PSM_ERR_ARG, "bad arguments");
  UCHK(u, hipSetDevice(u->device));
  const int ny = u->ny, nx = u->nx, mc = u->max_cases;
  auto measure = [&](double* out) -> int {
    UCHK(u, hipMemsetAsync(u->d_in, 0, (size_t)ny * nx * n_cases * u->c_in * sizeof(float), u->stream));
    hipEvent_t e0, e1;
    UCHK(u, hipEventCreate(&e0)); UCHK(u, hipEventCreate(&e1));
    int rc = PSM_OK;
    std::vector<float> t;
    for (int rep = 0; rep < 5 && rc == PSM_OK; ++rep) {           // 5 batches of `iters` passes, median batch
      for (int w = 0; w < 2 && rc == PSM_OK; ++w) rc = forward(u, u->d_in, n_cases, u->d_field, u->stream);
      (void)hipEventRecord(e0, u->stream);
      for (int i = 0; i < iters && rc == PSM_OK; ++i) rc = forward(u, u->d_in, n_cases, u->d_field, u->stream);
      (void)hipEventRecord(e1, u->stream);
      if (hipEventSynchronize(e1) != hipSuccess) rc = fail(u, PSM_ERR_HIP, "autotune: synchronize failed");
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      t.push_back(ms * 1e3f / iters);
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    std::sort(t.begin(), t.end());
    *out = t[t.size() / 2];
    return PSM_OK;
  };
  const size_t nc = u->convs.size();
  double best = 0.0;
  int rc = measure(&best);
  if (rc) return rc;
  if (us_before) *us_before = (float)best;
  auto try_set = [&](int what, size_t i, int value) -> int {       // keep choice `what` of layer i = `value` if the whole pass gets > 1 % faster
    int32_t& choice = u->choices[4 * i + what];
    const int old = choice;
    choice = value;
    int r = psm_unet_plan(u, ny, nx, mc);
    double t = 0.0;
    if (!r) r = measure(&t);
    if (r) return r;
    if (t < best * 0.99) { best = t; return PSM_OK; }
    choice = old;
    return psm_unet_plan(u, ny, nx, mc);
  };
  // 1. fused level pairs (bf16 mode): the other choice than the tile-count rule made, per level that has a pair kernel
  for (size_t i = 0; u->bf16 && i + 1 < nc; ++i)
    if (psm_pair_shape(u->convs[i], u->convs[i + 1]) && (rc = try_set(PSM_CHOICE_PAIR, i, u->convs[i].pair == 1 ? 0 : 1))) return rc;
  // Steps 2 and 3 run twice: a shallower split of a producer changes what its consumer can run (finished bf16 inputs: the
  // in-workgroup K split, the 8-row x 16-channel tile of the long layers), which only a second look at the tiles can pick up.
  for (int sweep = 0; sweep < 2; ++sweep) {
  const double best_at_sweep = best;
  // 2. tile shape of the unfused 3x3 layers: the two candidates the planner did not pick
  for (size_t i = 0; i < nc; ++i) {
    const Conv& c = u->convs[i];
    if (c.k != 3 || c.stem || c.pair != 0 || c.fuse_head) continue;
    const int cur = c.arrangement == 2 ? 3 : c.arrangement == 1 ? 2 : (c.nct == 2 ? 0 : 1);
    for (int cand = 0; cand < 3; ++cand) {
      static const int NCT[3] = {2, 1, 4};
      if (cand == cur || NCT[cand] > (c.cout + 15) / 16) continue;
      if ((rc = try_set(PSM_CHOICE_TILE, i, cand))) return rc;
    }
  }
  // 2b. float32 mode: the other arithmetic (x6 on the bf16 matrix pipe / float32 MFMA) for every layer with an 8-row tile
  for (size_t i = 0; !u->bf16 && u->x6 && i < nc; ++i) {
    const Conv& c = u->convs[i];
    if (c.k != 3 || c.stem || c.src == 0 || c.arrangement != 0) continue;
    if ((rc = try_set(PSM_CHOICE_X6, i, c.x6 ? 0 : 1))) return rc;
  }
  // 3. split-K depth
  for (size_t i = 0; i < u->convs.size(); ++i) {
    while (u->convs[i].ksplit > 1) {
      int32_t& cap = u->choices[4 * i + PSM_CHOICE_KSPLIT_CAP];
      const int old_cap = cap, old_split = u->convs[i].ksplit;
      cap = old_split / 2;
      if ((rc = psm_unet_plan(u, ny, nx, mc))) return rc;
      if (u->convs[i].ksplit >= old_split) {                      // the cap did not bind (a layer pinned by PSM_UNET_FORCE): the plan is the
        cap = old_cap;                                            // one just measured -- re-measuring it would only chase timing noise
        if ((rc = psm_unet_plan(u, ny, nx, mc))) return rc;
        break;
      }
      double t = 0.0;
      if ((rc = measure(&t))) return rc;
      if (t < best * 0.99) { best = t; continue; }                // keep the shallower split, try one more halving
      cap = old_cap;                                               // no gain: back to what it was
      if ((rc = psm_unet_plan(u, ny, nx, mc))) return rc;
      break;
    }
  }
  if (best >= best_at_sweep) break;                                // nothing moved: a second sweep would only chase timing noise
  }
  if (us_after) *us_after = (float)best;
  return PSM_OK;
}

int psm_unet_get_choices(const psm_unet* u, int32_t* choices, int32_t n) {
  if (!u || !choices) return PSM_ERR_ARG;
  if (!u->planned) return PSM_ERR_STATE;
  const size_t nc = u->convs.size();
  if (n < (int32_t)(4 * nc)) return PSM_ERR_ARG;
  std::copy(u->choices.begin(), u->choices.end(), choices);
  return (int)nc;
}

int psm_unet_set_choices(psm_unet* u, const int32_t* choices, int32_t n) {
  if (!u || !choices) return PSM_ERR_ARG;
  if (!u->planned) return fail(u, PSM_ERR_STATE, "psm_unet_plan has not been called");
  const size_t nc = u->convs.size();
  if (n != (int32_t)(4 * nc)) return fail(u, PSM_ERR_ARG, "choices must hold 4 values per convolution");
  for (size_t i = 0; i < nc; ++i) {
    const int32_t* c = choices + 4 * i;
    if (c[0] < 1 || c[0] > 8 || c[1] < -1 || c[1] > 2 || c[2] < -1 || c[2] > 1 || c[3] < -1 || c[3] > 1)
      return fail(u, PSM_ERR_ARG, "choice out of range (split cap 1..8, tile -1..2, pair -1..1, x6 -1..1)");
  }
  u->choices.assign(choices, choices + 4 * nc);
  UCHK(u, hipSetDevice(u->device));
  return psm_unet_plan(u, u->ny, u->nx, u->max_cases);
}

int psm_unet_ksplit(const psm_unet* u, int32_t idx) {
  if (!u || !u->planned || idx < 0 || idx >= (int)u->convs.size()) return PSM_ERR_ARG;
  return u->convs[idx].ksplit;
}

int psm_unet_plan_info(const psm_unet* u, int32_t idx, int32_t* info) {
  if (!u || !info || !u->planned || idx < 0 || idx >= (int)u->convs.size()) return PSM_ERR_ARG;
  const Conv& c = u->convs[idx];
  info[0] = psm_conv_tile_rows(c.arrangement); info[1] = c.nct; info[2] = c.ksplit; info[3] = c.pair | (c.x6 ? 4 : 0) | (c.kw == 2 ? 8 : 0);
  return PSM_OK;
}

int psm_unet_plan_detail(const psm_unet* u, int32_t idx, int32_t* info, int32_t n) {
  if (!u || !info || n < 0 || !u->planned || idx < 0 || idx >= (int)u->convs.size()) return PSM_ERR_ARG;
  const Conv& c = u->convs[idx];
  int32_t v[16];
  psm_unet_layer_detail(c, c.src != 0 ? &u->convs[idx - 1] : nullptr, c.src == 3 ? &u->convs[c.skip] : nullptr, u->bf16 != 0, u->keep_act, v);
  for (int k = 0; k < 16 && k < n; ++k) info[k] = v[k];
  return 16;
}

int psm_unet_debug_run_layer(psm_unet* u, int32_t idx, float* stamps_us) {
  // diagnostic builds: re-run convolution `idx` alone on the activations of the last forward pass and return the
  // workgroup-0 stamps in microseconds after the first one (-1: not reached); stamps are overwritten by every layer, so run up to idx
  if (!u || !stamps_us) return PSM_ERR_ARG;
  if (!u->planned || u->last_cases < 1 || idx < 0 || idx >= (int)u->convs.size()) return fail(u, PSM_ERR_STATE, "run a forward pass first");
  UCHK(u, hipSetDevice(u->device));
  int rc = forward(u, u->d_in, u->last_cases, u->d_field, u->stream, nullptr, idx + 1);
  if (rc) return rc;
  UCHK(u, hipStreamSynchronize(u->stream));
  unsigned long long t[64];
  if (u->convs[idx].pair == 1) UCHK(u, psm_unet_pair_read_stamps(t));       // 3 workgroups x 16 stamps (first, middle, last)
  else UCHK(u, psm_unet_read_stamps(t));
  unsigned long long t0 = ~0ull;
  for (int k = 0; k < 64; ++k) if (t[k] && t[k] < t0) t0 = t[k];
  for (int k = 0; k < 64; ++k) stamps_us[k] = t[k] ? (float)((double)(t[k] - t0) * 0.01) : -1.f;
  return PSM_OK;
}

int64_t psm_unet_flops(const psm_unet* u) {
  if (!u || !u->planned) return 0;
  int64_t t = 0;
  for (const Conv& c : u->convs) t += 2LL * (u->ny >> c.level) * (u->nx >> c.level) * c.k * c.k * c.cin * c.cout;
  return t;
}

}  // extern "C"
