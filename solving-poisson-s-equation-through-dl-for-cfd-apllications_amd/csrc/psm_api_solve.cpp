// psm_api_solve.cpp -- C-ABI of libpsm_hip.so (include/psm.h): one solve: route, argument builders, launch sequence, host-buffer entries (the step around it: psm_api_step.cpp).  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {


// K groups of the M-tiled x6 encode (psm_encode_x6_mt_kernel) for Mpad block rows; 1 = the one-slab-per-slice form (psm_encode_x6_kernel).
// A workgroup = one K group x 64 block rows, two workgroups per CU: the group count decides both the slab bytes and how the
// workgroups fill 512 slots.  Measured on one box, whole step of the deltas case batch in us (g1 = one slab per slice):
//   cases  rows(pad)  row groups   g1      256 groups  128     64      uneven 512 / row groups
//     8      96         2          42.2    41.0
//    12     128         2          47.9    44.6
//    16     160         3          59.8    56.1        56.8    59.1
//    20     192         3          64.6    60.0        59.7    61.5
//    28     256         4          74.5    70.1        65.7    65.9
//    32     288         5          88.9    84.1        85.4    86.3    92.1 (102 groups)
//    40     384         6         102.0    95.7        91.4    92.0
//    48     448         7         113.8   106.3       104.0    99.1   110.6 (73)
//    56     512         8         124.7   116.9       110.6   106.5
//    64     576         9         140.7   132.1       130.4   134.9   123.5 (56)
// Even groups (a power of two) by row-group count from that table; from nine row groups up 512 / row groups (uneven by one slice).
// Below 96 rows (4 cases: 37.6 against 38.0 us) the launch is bound by the basis stream and the one-slab-per-slice form stays.
// PSM_ENCODE_KGROUPS=n forces the group count (1: the old form), PSM_ENCODE_MT_MIN_ROWS the first row count.
static int encode_groups(const psm_handle* h, int Mpad) {
  if (h->cfg.precision == PSM_PRECISION_BF16 || h->NT > 4 || Mpad % 32 != 0 || Mpad < h->sw.at_create.encode_mt_min_rows || ((PSM_PIX_PER_SLICE * h->cfg.c_in) % 32) != 0) return 1;
  if (h->x6_mode >= 0 && !(h->x6_mode & 1)) return 1;
  // psm_encode_x6_mt_kernel addresses the grids of the whole case batch with unsigned 32-bit BYTE offsets from a scalar base
  if ((int64_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_in >= ((int64_t)1 << 30)) return 1;
  const int row_groups = (Mpad + PSM_ENC_MT_ROWS - 1) / PSM_ENC_MT_ROWS;
  static const int by_rg[9] = {0, 256, 256, 256, 128, 256, 128, 64, 64};
  int groups = row_groups <= 8 ? by_rg[row_groups] : std::max(1, 512 / row_groups);
  groups = std::max((h->n_slices + 7) / 8, std::min(h->n_slices, groups));
  if (h->sw.at_create.encode_kgroups > 0) groups = h->sw.at_create.encode_kgroups;
  return (groups > 1 && groups <= h->n_slices && (h->n_slices + groups - 1) / groups <= 8) ? groups : 1;
}
// Slabs the float32 / x6 encode launch (psm_launch_encode, psm_encode.hip) writes for these arguments = what the reduce behind it must sum.
// The launcher's three branches, in its order; psm_encode_pairs is a predicate of the arguments alone, so this is the one place the rule lives.
static int encode_slabs(const PsmEncodeArgs& a) {
  const int n_slices = a.S * a.S / PSM_PIX_PER_SLICE;
  if (a.x6 && a.kgroup > 1) return a.kgroup;              // M-tiled x6 form: one slab per K group
  return psm_encode_pairs(a) ? n_slices / 2 : n_slices;   // two slices per workgroup, or one slab per slice
}
// What that encode needs beyond the plan, built on first use and OUTSIDE any stream capture (it allocates): the basis pre-split
// into three bf16 planes (1.5 x the bytes of the float32 pack), made on the device from the float32 pack.
int ensure_encode_aux(psm_handle* h, int n_cases) {
  const int Mpad = round_up(n_cases * h->B, 32);
  if (h->d_bpack_x6 || encode_groups(h, Mpad) <= 1) return PSM_OK;
  const size_t n16 = (size_t)h->n_slices * h->NT * (PSM_PIX_PER_SLICE * h->cfg.c_in / 16) * 3 * 64;
  int rc = dev_alloc(h, &h->d_bpack_x6, n16);
  if (rc) return rc;
  HIPCHK(h, psm_launch_split_basis(h->d_bpack_in, h->d_bpack_x6, h->n_slices, h->NT, PSM_PIX_PER_SLICE * h->cfg.c_in, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PSM_OK;
}


// ---- the route --------------------------------------------------------------------------------------------------
// The bound geometry applies to a solve of this many cases: THE spelling of "is this solve bound", for the route and for the graph keys.
bool bound_applies(const psm_handle* h, int n_cases) {
  return h->bound && (h->bound_scope == 2 || h->in_mesh_solve) && n_cases == h->bound_cases;
}

// The SDF fold applies to a solve of this many cases (psm_handle.h): a float32 single case of one row tile on a geometry bound with
// psm_bind_geometry (whose guard riders then check the SDF channel's values; not psm_solve's own binding, whose grids nobody checks),
// float32 MFMA arithmetic.  PSM_SDF_FOLD=0 switches it off; read per solve, and part of sequence_key.
bool fold_applies(const psm_handle* h, int n_cases, const PsmSwitches::PerSolve& ps) {
  if (!(bound_applies(h, n_cases) && n_cases == 1 && h->bound_scope == 2 && h->fold_bound && h->d_bpack_fold && h->d_ib_fold && h->d_sdf_bound)) return false;
  if (h->cfg.precision != PSM_PRECISION_F32 || h->NT > 4 || round_up(h->B, 32) != 32 || (h->x6_mode >= 0 && (h->x6_mode & 1))) return false;
  return ps.sdf_fold;
}

static PsmEncodeArgs encode_args(const psm_handle* h, const Workspace& w, const SolveRoute& r, const float* d_grid) {
  PsmEncodeArgs ea{};
  ea.grid = d_grid; ea.mean = h->d_mean_in; ea.bpack = r.fold ? h->d_bpack_fold : h->d_bpack_in; ea.part = w.d_part;
  ea.fold = r.fold ? 1 : 0;
  ea.row_base = h->d_row_base; ea.row_stride = (int64_t)h->Nx * h->cfg.c_in;
  ea.M = r.M; ea.Mpad = r.Mpad; ea.NT = h->NT; ea.ldp = h->ld_in; ea.S = h->S; ea.c_in = h->cfg.c_in;
  ea.aligned = r.aligned; ea.whole = r.whole; ea.x6 = r.x6; ea.kgroup = r.kgroup;
  if (r.kgroup > 1) ea.bpack_x6 = h->d_bpack_x6;
  ea.pairs_ok = (!r.bf16 && h->sw.at_create.encode_pairs) ? 1 : 0;   // PSM_ENCODE_PAIRS=0 keeps one slab per slice.  A single case of four component tiles: two K slices per workgroup, half the slabs (psm_encode_pair_kernel)
  return ea;
}

// Makes no HIP call and writes nothing to the handle.  Runs when launches are enqueued or captured, never on a graph replay.
SolveRoute choose_route(const psm_handle* h, const Workspace& w, const float* d_grid, int n_cases, bool profiled, const PsmSwitches::PerSolve& ps) {
  SolveRoute r;
  const int nl = (int)h->dense.size();
  r.n_cases = n_cases; r.M = n_cases * h->B; r.Mpad = round_up(r.M, 32);
  r.bf16 = (h->cfg.precision == PSM_PRECISION_BF16);
  // geometry-bound fast path: nothing but the encode group being timed / skipped
  r.bound = bound_applies(h, n_cases) && (h->timed_kernel < 0 || h->timed_kernel == PSM_K_ENCODE) && h->debug_skip == 0;
  // case batches (and single cases of more than 64 blocks) on a bound geometry: closed form of the chain where it was built
  r.cf = r.bound && h->bound_cf && w.d_dots2;
  // bound-geometry contract: guard riders in the launch that computes the strip dots (not for psm_solve, whose grid is
  // built from the bound sdfunct itself)
  r.guard = r.bound && h->guard_on && h->bound_scope == 2 && h->d_maskbits && w.d_gflags;
  r.guard_wgs = (h->guard_waves + PSM_GUARD_WG_WAVES - 1) / PSM_GUARD_WG_WAVES;

  r.stamp_encode = h->timed_kernel == PSM_K_ENCODE && !profiled;   // dominant kernel: dispatch-level begin / end stamps (no marker packets around the launch)
  r.aligned = (h->plan_aligned && (reinterpret_cast<uintptr_t>(d_grid) & 15) == 0) ? 1 : 0;
  r.whole = h->sw.at_create.encode_chunked ? 0 : 1;
  // arithmetic of the encode contraction: exact-float32 MFMA for a single row tile (one case: the launch is bound by the basis
  // stream, the matrix phase is short), the x6 form (six bf16 MFMA terms of exactly split operands, float32 accuracy,
  // psm_encode_x6_kernel) from two row tiles up, where the matrix phase is the longest serial phase of the launch
  // (8 cases: 17.6 -> 15.5 us, 64 cases: 75 -> 60 us).  PSM_X6=0 / 1 forces float32 / x6 everywhere.
  r.x6 = h->x6_mode < 0 ? (r.Mpad > 32 ? 1 : 0) : ((h->x6_mode & 1) ? 1 : 0);
  // Negative result, kept as a knob: two workgroups per slice of the x6 form (64 rows each, half the LDS, two per CU so that one's
  // matrix phase covers the other's load latency) -- 17.7 against 15.0 us at 8 cases, 21.8 against 17.6 us at 12: the launch is bound
  // by its streams, and the split reads the basis slice twice.  PSM_ENCODE_ROWSPLIT=1 selects it.
  r.row_wgs = (r.x6 && h->sw.at_create.encode_rowsplit && r.Mpad > 64 && r.Mpad <= 32 * PSM_MT_CHUNK) ? 2 : 1;
  r.fold = r.bound && !r.bf16 && !r.x6 && r.Mpad == 32 && fold_applies(h, n_cases, ps);
  // Large case batches (>= 32 cases of 9 blocks): the M-tiled, wave-specialised x6 form (encode_groups / ensure_encode_aux)
  const int groups = (r.x6 && !r.bf16) ? encode_groups(h, r.Mpad) : 1;
  r.kgroup = (groups > 1 && h->d_bpack_x6) ? groups : 1;
  r.n_slabs = r.bf16 ? h->n_slices : encode_slabs(encode_args(h, w, r, d_grid));   // bf16 handles (psm_launch_encode_bf16): one slab per slice

  // few block rows: slab reduce + first dense layer in one launch (one workgroup per row)
  r.fuse1 = h->fuse_reduce_dense1 && r.Mpad <= 128 && h->ld_in <= 512 && h->dense[0].ldw <= 1024 &&
            h->timed_kernel != PSM_K_REDUCE && h->conv1d.empty();
  // Large case batches (more than 128 block rows): the activation between two plain float32 Dense launches in MFMA operand order
  // (PsmDenseArgs::in_packed / out_packed): the consumer's row loads are then contiguous KiBs -- 64 cases: 10.0 -> 8.4 us per hidden
  // layer, 32 cases: 6.7 -> 5.2 (profiles/r06_case_batch.txt).  Not with a LayerNormalization behind the producer (its kernel and the
  // fused form read rows), not for bf16 handles, not in front of the Conv1D head.  PSM_DENSE_PACKED=0 keeps rows everywhere.
  bool pack = h->sw.at_create.dense_packed && r.Mpad > 128 && !r.bf16;
  for (const DenseLayer& q : h->dense) if (q.ln) pack = false;       // densePCA_attention: its normalisations (and their residuals) read rows
  r.packed.assign(nl, 0);
  for (int l = 0; pack && l < nl - 1; ++l) r.packed[l] = h->dense[l].ldw % 16 == 0 && h->dense[l + 1].Kp <= h->dense[l].ldw;
  // LayerNormalization (+ residual with the layer's own input) behind a hidden layer: densePCA_attention.  Where the consumer
  // is another hidden Dense launch the normalisation is DEFERRED into it (psm_dense_kernel<..., LNIN>: moments of its own input
  // rows in the prologue, the residual of NNs.py:64 in its epilogue) -- no launch; the last one, whose consumers are the head,
  // the strip-dot riders and the introspection entries, finishes its activation with psm_layernorm_kernel.  PSM_LN_FUSE=0
  // launches every normalisation on its own.
  r.ln_fuse = ps.ln_fuse;                                // read per solve (diagnostic; the tests switch it in-process), part of sequence_key
  // Large case batches: the guard workgroups (one per 4096 pixels: 1024 for 64 cases, 50 MB of grid to look at again) are dealt
  // evenly over the hidden-layer launches and the head launch instead of all riding behind the head (64 cases: 14.9 us for a
  // 4.3 us layer).  PSM_GUARD_SPREAD=0 keeps them behind the head.
  r.rider_carriers = nl - 1 - (r.fuse1 ? 1 : 0);       // hidden layers launched through psm_launch_dense
  r.spread = r.guard && h->sw.at_create.guard_spread && r.guard_wgs > 256 && r.rider_carriers > 0;
  r.rider_share = r.spread ? r.guard_wgs / (r.rider_carriers + 1) : 0;

  // decode + paste on a bound geometry: x6 arithmetic by default (single case 8.44 -> 8.16 us, 8 cases 10.2 -> 8.8 us; same
  // accuracy as the float32 MFMA, tools/x6_check.py); PSM_X6 bit 1 = 0 keeps v_mfma_f32_32x32x2_f32
  r.decode_x6 = (r.bound && (h->x6_mode < 0 || (h->x6_mode & 2))) ? 1 : 0;
  r.one_launch_tail = r.bound && n_cases == 1 && h->B <= 64;
  // Case batches (psm_launch_decode_paste_batch): one 32-row tile per chunk, the row tiles spread over up to `decode_wgs / column
  // workgroups` row groups (grid.y): measured against two and three tiles per chunk (fewer passes over the basis slice, but 2-3x the
  // LDS and registers per workgroup) at 8 ... 64 cases and both field counts -- 16 cases: 12.5 against 20.0 us, 64 cases: 30.2
  // against 48.8 us, U_to_gradP 8 cases: 24.1 against 36.8 us, 8 deltas cases: equal (tools/attic/decode_mtc_sweep.py).  With fewer
  // than 256 column workgroups (a single-field basis: 128) that spreads the rows -- 8 cases x 9 blocks of a one-field model ran as
  // 128 workgroups of 3 tiles (14.7 us), as 384 workgroups of one tile they take 10.6 us.  PSM_DECODE_MTC (1..3; the 4-tile form
  // spills: acc + tile + row operands) / PSM_DECODE_WGS: diagnostic.
  r.decode_mtc = h->sw.at_create.decode_mtc; r.decode_wgs = h->sw.at_create.decode_wgs;
  const int64_t fb = (int64_t)n_cases * h->Ny * h->Nx * h->cfg.c_out * (int64_t)sizeof(float);
  r.field_bytes = (r.bound && h->sw.at_create.paste_buffer_stores && fb < ((int64_t)1 << 32)) ? (uint32_t)fb : 0u;
  // few blocks, few cases: every paste workgroup re-runs the chain (one launch less); for case batches one chain workgroup
  // per case + a streaming paste
  r.fused_assemble = !r.bound && h->fused_assemble && n_cases < 4;
  r.pred_stored = !r.bound && !((h->debug_skip >> PSM_K_DECODE) & 1);
  return r;
}


// ---- one builder per kernel-argument block ------------------------------------------------------------------------
PsmDecodeArgs decode_args(const psm_handle* h, const Workspace& w, int n_cases, const float* row_scale, float* pred, int x6) {
  PsmDecodeArgs de{};
  de.res = w.d_res; de.ld_res = h->ld_out; de.bpack = h->d_bpack_out; de.mean = h->d_mean_out;
  de.row_scale = row_scale; de.pred = pred; de.M = n_cases * h->B; de.Mpad = round_up(de.M, 32); de.Gd = h->Gd;
  de.n_coltiles = h->n_coltiles; de.K_out = h->K_out; de.x6 = x6;
  return de;
}

// strip dots of the bound geometry: the pair rows of the closed form (cf), or the strip rows of the chain.  float32 handles contract
// with the last hidden activation (head folded into the tables), bf16 handles with the bf16-rounded res.
PsmDotsArgs dots_args(const psm_handle* h, const Workspace& w, bool cf, int n_cases, const float* row_scale, const PsmGuardArgs& guard) {
  const int CB = h->cfg.c_out * h->B, Kh = h->cfg.precision == PSM_PRECISION_BF16 ? h->ld_out : h->dense.back().Kpad;
  return cf ? PsmDotsArgs{h->d_g2p, h->d_c2p, h->d_cntp, h->d_row_of_p, row_scale, w.d_dots2, n_cases * CB, Kh, guard, h->B, CB}
            : PsmDotsArgs{h->d_g2, h->d_c2, h->d_cnt, h->d_row_of, row_scale, w.d_dots, h->bound_rows * n_cases, Kh, guard};
}

PsmStripArgs strip_args(const psm_handle* h, const Workspace& w, const float* d_grid) {
  PsmStripArgs sa{};
  sa.pred = w.d_pred; sa.grid = d_grid; sa.strips = h->d_strips; sa.blk_y0x0 = h->d_blk; sa.spart = w.d_spart; sa.colpart = w.d_colpart; sa.NS = h->plan.cp.NS; sa.n_bands = h->n_bands;
  sa.B = h->B; sa.S = h->S; sa.c_in = h->cfg.c_in; sa.c_out = h->cfg.c_out;
  sa.sdf_ch = h->cfg.sdf_channel; sa.Ny = h->Ny; sa.Nx = h->Nx;
  return sa;
}

PsmChainArgs chain_args(const psm_handle* h, const Workspace& w) {
  PsmChainArgs ca{};
  ca.cp = h->plan.cp; ca.blocks = h->d_blocks; ca.spart = w.d_spart; ca.colpart = w.d_colpart; ca.n_bands = h->n_bands; ca.pred = w.d_pred; ca.owner = h->d_owner;
  ca.shiftA = h->d_shiftA; ca.shiftB = h->d_shiftB; ca.shiftOwnA = h->d_shiftOwnA; ca.shiftOwnB = h->d_shiftOwnB; ca.shiftW = h->d_shiftW;
  for (int f = 0; f < 2; ++f) ca.shiftL[f] = (int)h->plan.shiftA[f].size();
  ca.Lmax = h->Lmax; ca.offs = w.d_offs; ca.shift = w.d_shift; ca.n_strips = h->n_strips; ca.c_out = h->cfg.c_out; ca.stamps = h->d_stamps;
  return ca;
}

PsmPasteArgs paste_args(const psm_handle* h, const Workspace& w, float* d_fields) {
  return PsmPasteArgs{w.d_pred, h->d_owner, w.d_offs, w.d_shift, d_fields, h->B, h->S, h->cfg.c_out, h->Ny * h->Nx};
}


// ---- the launch sequence: encode, reduce + MLP, then the bound or the general tail ----------------------------------
struct Solve {                        // what the stages of one launch_all share
  psm_handle* h; Workspace& w; const SolveRoute& r;
  const float* grid; float* fields; const float* row_scale;
  hipStream_t st; Timer tm;
};

// guard workgroups of this solve for the launch that carries them: hidden Dense launch `carrier` of a spread guard takes its share,
// carrier == rider_carriers is the head launch (bf16 handles: their own dots launch) with what the hidden launches did not carry
static PsmGuardArgs guard_args(const Solve& s, int carrier) {
  PsmGuardArgs ga{};
  if (!s.r.guard) return ga;
  const psm_handle* h = s.h;
  ga.sdf = s.grid + h->cfg.sdf_channel; ga.bits = h->d_maskbits; ga.flags = s.w.d_gflags;
  ga.host_flag = h->m_guard ? h->m_guard + s.w.gidx : nullptr;
  ga.npix = (long long)s.r.n_cases * h->Ny * h->Nx; ga.c_in = h->cfg.c_in; ga.n_ballots = h->guard_ballots; ga.n_waves = h->guard_waves;
  ga.wg_first = carrier * s.r.rider_share;
  ga.wg_count = carrier < s.r.rider_carriers ? s.r.rider_share : s.r.guard_wgs - ga.wg_first;
  ga.sdf_ref = s.r.fold ? h->d_sdf_bound : nullptr;       // folded encode: the contract is the SDF channel's values
  return ga;
}

static int stage_encode(Solve& s) {
  psm_handle* h = s.h;
  const PsmEncodeArgs ea = encode_args(h, s.w, s.r, s.grid);
  auto launch = [&](hipEvent_t e0, hipEvent_t e1) { return s.r.bf16 ? psm_launch_encode_bf16(ea, s.st, e0, e1) : psm_launch_encode(ea, s.st, e0, e1, s.r.row_wgs); };
  if (s.r.stamp_encode) {
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    h->timed_events.push_back({e0, e1});
    HIPCHK(h, launch(e0, e1));
    return PSM_OK;
  }
  s.tm.before(PSM_K_ENCODE);
  PSM_REPEAT(h, PSM_K_ENCODE) HIPCHK(h, launch(nullptr, nullptr));
  s.tm.after(PSM_K_ENCODE);
  return PSM_OK;
}

static PsmDenseArgs dense_args(const Solve& s, int l, const float* cur, int ld_cur) {
  const psm_handle* h = s.h;
  const int nl = (int)h->dense.size();
  const DenseLayer& d = h->dense[l];
  const bool head = (l == nl - 1);
  PsmDenseArgs da{};
  da.in = cur; da.ld_in = ld_cur; da.W = d.W; da.ld_w = d.ldw; da.bias = d.b; da.Wp = d.Wp; da.Kp = d.Kp;
  da.sa = h->d_sa; da.sb = h->d_sb;
  da.out = head ? s.w.d_res : s.w.d_act[l & 1]; da.ld_out = d.ldw;
  da.Kpad = d.Kpad; da.Mpad = s.r.Mpad; da.relu = (head || d.linear) ? 0 : 1; da.head = head ? 1 : 0;
  da.bf16 = s.r.bf16 ? 1 : 0;
  da.layer = l;
  da.out_packed = s.r.packed[l];                          // hidden activation of a large batch: written in MFMA operand order ...
  da.in_packed = l > 0 ? s.r.packed[l - 1] : 0;           // ... and read as such by the next Dense launch
  // the head's strip-dot riders (and psm_read_stage) read whole rows: the last hidden layer also leaves a row-major copy
  if (da.out_packed && l == nl - 2) da.out_rows = s.w.d_act_rows;
  if (da.in_packed && head) da.in_rows = s.w.d_act_rows;
  // keep mode: output pointers only -- a hidden layer stores into its own buffer (packed chains: its row-major copy there)
  if (&s.w == &h->ws0 && !h->d_keep.empty()) {
    if (!head) { if (da.out_packed) da.out_rows = h->d_keep[l]; else da.out = h->d_keep[l]; }
    if (head && da.in_packed) da.in_rows = h->d_keep[nl - 2];
  }
  return da;
}

// conv1D_PCA head: Conv1D layers over the scaled coefficients, then Flatten; cur / ld_cur: the input of Dense layer 0
static int conv1d_head(Solve& s, const float*& cur, int& ld_cur) {
  psm_handle* h = s.h;
  int64_t stride = ld_cur;
  const int nc = (int)h->conv1d.size();
  for (int q = 0; q < nc; ++q) {
    const Conv1dLayer& c = h->conv1d[q];
    PsmConv1dArgs ca{};
    ca.in = cur; ca.in_stride = stride; ca.W = c.W; ca.bias = c.b; ca.out = s.w.d_c1[q & 1];
    ca.out_stride = q == nc - 1 ? (int64_t)round_up(h->cfg.p_in * c.cout, 32) : (int64_t)h->cfg.p_in * c.cout;
    ca.M = s.r.M; ca.P = h->cfg.p_in; ca.k = c.k; ca.c_in = c.cin; ca.c_out = c.cout; ca.relu = 1;
    HIPCHK(h, psm_launch_conv1d(ca, s.st));
    cur = ca.out; stride = ca.out_stride;
  }
  ld_cur = (int)stride;
  return PSM_OK;
}

static int stage_mlp(Solve& s) {
  psm_handle* h = s.h;
  const SolveRoute& r = s.r;
  const int nl = (int)h->dense.size();
  // folded encode: the SDF channel's share of the coefficients is in the binding's per-row copy of the scaler offset
  const PsmReduceArgs ra{s.w.d_part, s.w.d_xin, h->d_ia, r.fold ? h->d_ib_fold : h->d_ib, r.n_slabs, r.Mpad, h->ld_in, r.fold ? h->ld_in : 0};
  s.tm.before(PSM_K_REDUCE);
  if (!r.fuse1) PSM_REPEAT(h, PSM_K_REDUCE) HIPCHK(h, psm_launch_reduce(ra, s.st));      // fused: Dense 0's launch sums the slabs
  s.tm.after(PSM_K_REDUCE);
  s.tm.before(PSM_K_MLP);
  PSM_REPEAT(h, PSM_K_MLP) {
    const float* cur = s.w.d_xin; int ld_cur = h->ld_in;
    int rc = conv1d_head(s, cur, ld_cur);
    if (rc) return rc;
    int pending = -1;       // >= 0: `cur` is the raw output of that layer, whose LayerNormalization the next launch applies
    int carrier = 0;        // hidden launches through psm_launch_dense so far: the next one's share of the guard workgroups
    for (int l = 0; l < nl; ++l) {
      const DenseLayer& d = h->dense[l];
      PsmDenseArgs da = dense_args(s, l, cur, ld_cur);
      bool residual_done = false;
      if (pending >= 0) {                               // this launch normalises its input (and adds the residual of its own LN)
        const DenseLayer& p = h->dense[pending];
        da.ln_gamma = p.ln_gamma; da.ln_beta = p.ln_beta; da.ln_eps = p.ln_eps; da.ln_n = p.n_out;
        da.ln_residual = (d.ln && d.ln_residual) ? 1 : 0;
        residual_done = da.ln_residual != 0;
        pending = -1;
      }
      if (l == 0 && r.fuse1) {
        HIPCHK(h, psm_launch_reduce_dense1(ra, da, s.st));
      } else if (l < nl - 1) {
        const PsmGuardArgs ga = r.spread ? guard_args(s, carrier++) : PsmGuardArgs{};
        HIPCHK(h, psm_launch_dense(da, s.st, r.spread ? &ga : nullptr));
      } else if (r.bound && !r.bf16) {                  // head layer + strip dots of the bound geometry in one launch
        HIPCHK(h, psm_launch_dense_dots(da, dots_args(h, s.w, r.cf, r.n_cases, s.row_scale, guard_args(s, r.rider_carriers)), s.st));
      } else {
        HIPCHK(h, psm_launch_dense(da, s.st));
      }
      if (d.ln) {                                       // hidden layers only (psm_set_layernorm)
        if (r.ln_fuse && l + 1 <= nl - 2) pending = l;  // the next hidden layer applies it
        else {
          PsmLayerNormArgs la{da.out, d.ldw, (d.ln_residual && !residual_done) ? cur : nullptr, ld_cur, d.ln_gamma, d.ln_beta, r.Mpad, d.n_out, d.ln_eps};
          HIPCHK(h, psm_launch_layernorm(la, s.st));
        }
      }
      cur = da.out; ld_cur = d.ldw;
    }
  }
  s.tm.after(PSM_K_MLP);
  return PSM_OK;
}

// bound geometry: decode, offset chain and paste from the strip dots, in one launch or (case batches) chain launch + decode + paste
static int stage_bound_tail(Solve& s) {
  psm_handle* h = s.h;
  const SolveRoute& r = s.r;
  const PsmDecodeArgs de = decode_args(h, s.w, r.n_cases, s.row_scale, nullptr, r.decode_x6);
  if (h->bound_zero_fill)                               // cells no block covers stay 0 like the reference's np.zeros field
    HIPCHK(h, hipMemsetAsync(s.fields, 0, (size_t)r.n_cases * h->Ny * h->Nx * h->cfg.c_out * sizeof(float), s.st));
  // bf16 handles: dots from the bf16-rounded res (own small launch): pair rows, or the strip rows of the chain
  auto res_dots = [&] { return psm_launch_res_dots(dots_args(h, s.w, r.cf, r.n_cases, s.row_scale, guard_args(s, r.rider_carriers)), s.w.d_res, h->ld_out, s.st); };
  if (r.one_launch_tail) {
    PsmBoundArgs ba{};
    bound_common(ba, h, s.w, r, s.fields);
    s.tm.before(PSM_K_DECODE);
    if (r.bf16) HIPCHK(h, res_dots());
    PSM_REPEAT(h, PSM_K_DECODE) HIPCHK(h, psm_launch_decode_paste(de, ba, h->cfg.c_out, s.st, r.bf16 ? 1 : 0));
    s.tm.after(PSM_K_DECODE);
    s.tm.skip(PSM_K_STRIPS); s.tm.skip(PSM_K_CHAIN); s.tm.skip(PSM_K_PASTE);
    return PSM_OK;
  }
  // case batch: the chains of all cases in one small launch, then decode + paste over all block rows
  PsmBoundBatchArgs bb{};
  bound_common(bb, h, s.w, r, s.fields);
  bb.npix = h->Ny * h->Nx; bb.rows_pc = h->bound_rows; bb.n_cases = r.n_cases;
  s.tm.skip(PSM_K_DECODE); s.tm.skip(PSM_K_STRIPS);
  s.tm.before(PSM_K_CHAIN);
  if (r.bf16) HIPCHK(h, res_dots());
  if (!r.cf) HIPCHK(h, psm_launch_chain_dots(bb, h->cfg.c_out, s.st));     // closed form: no chain launch
  s.tm.after(PSM_K_CHAIN);
  s.tm.before(PSM_K_PASTE);
  HIPCHK(h, psm_launch_decode_paste_batch(de, bb, h->cfg.c_out, s.st, r.decode_mtc, r.decode_wgs, r.bf16 ? 1 : 0));
  s.tm.after(PSM_K_PASTE);
  return PSM_OK;
}

// general path: decode to blocks, strip sums, offset chain, paste
static int stage_general_tail(Solve& s) {
  psm_handle* h = s.h;
  const SolveRoute& r = s.r;
  const PsmDecodeArgs de = decode_args(h, s.w, r.n_cases, s.row_scale, s.w.d_pred);
  s.tm.before(PSM_K_DECODE);
  PSM_REPEAT(h, PSM_K_DECODE) HIPCHK(h, r.bf16 ? psm_launch_decode_bf16(de, s.st) : psm_launch_decode(de, s.st));
  s.tm.after(PSM_K_DECODE);
  s.tm.before(PSM_K_STRIPS);
  PSM_REPEAT(h, PSM_K_STRIPS) HIPCHK(h, psm_launch_strips(strip_args(h, s.w, s.grid), r.n_cases, s.st));
  s.tm.after(PSM_K_STRIPS);
  const PsmChainArgs ca = chain_args(h, s.w);
  const PsmPasteArgs pa = paste_args(h, s.w, s.fields);
  s.tm.before(PSM_K_CHAIN);
  if (!r.fused_assemble) HIPCHK(h, psm_launch_chain(ca, r.n_cases, s.st));      // fused: every paste workgroup re-runs the chain
  s.tm.after(PSM_K_CHAIN);
  s.tm.before(PSM_K_PASTE);
  if (r.fused_assemble) PSM_REPEAT(h, PSM_K_PASTE) HIPCHK(h, psm_launch_assemble(ca, pa, r.n_cases, s.st));
  else HIPCHK(h, psm_launch_paste(pa, r.n_cases, s.st));
  s.tm.after(PSM_K_PASTE);
  return PSM_OK;
}

int launch_all(psm_handle* h, Workspace& w, const float* d_grid, int n_cases, float* d_fields, const float* d_row_scale,
               hipStream_t st, hipEvent_t* prof, const PsmSwitches::PerSolve& ps) {
  const SolveRoute r = choose_route(h, w, d_grid, n_cases, prof != nullptr, ps);
  // the record of what this solve leaves (a ring slot's solve leaves nothing readable: the rest of the record is stale then)
  if (&w == &h->ws0) h->last = Ws0Solve{true, r.pred_stored, r.cf, h->dense.size() > 1 && r.packed[h->dense.size() - 2], d_row_scale, nullptr, d_grid, n_cases};
  else h->last.on_ws0 = false;
  Solve s{h, w, r, d_grid, d_fields, d_row_scale, st, Timer{h, st, 0, prof}};
  int rc;
  if ((rc = stage_encode(s)) || (rc = stage_mlp(s))) return rc;
  return r.bound ? stage_bound_tail(s) : stage_general_tail(s);
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_solve_grid_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale,
                          float* d_fields, void* stream) {
  return solve_device(h, d_grid, n_cases, out_scale, d_fields, (hipStream_t)stream, nullptr);
}

int psm_solve_grid(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, float* fields) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!grid || !fields) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)n_cases * npix * h->cfg.c_in * sizeof(float);
  const size_t gout = (size_t)n_cases * npix * h->cfg.c_out * sizeof(float);
  const bool reg_in = host_registered(h, grid, gin), reg_out = host_registered(h, fields, gout);
  if (!reg_in) memcpy(h->h_grid, grid, gin);
  HIPCHK(h, hipMemcpyAsync(h->d_grid_stage, reg_in ? grid : h->h_grid, gin, hipMemcpyHostToDevice, h->stream));
  const int rc = guarded_host_step(h, h->stream, "psm_solve_grid", [&](int) {
    const int rs = solve_device(h, h->d_grid_stage, n_cases, out_scale, h->d_fields_stage, h->stream, nullptr);
    if (rs) return rs;
    HIPCHK(h, hipMemcpyAsync(reg_out ? fields : h->h_fields, h->d_fields_stage, gout, hipMemcpyDeviceToHost, h->stream));
    return PSM_OK;
  });
  if (rc) return rc;
  if (!reg_out) memcpy(fields, h->h_fields, gout);
  return PSM_OK;
}


int psm_synchronize(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipDeviceSynchronize());
  if (guard_take(h, h->ws0)) {                 // a psm_solve_grid_device call on another geometry: its field is NaN
    int rc = guard_drop(h, "psm_solve_grid_device");
    return rc ? rc : PSM_ERR_GEOMETRY;
  }
  return PSM_OK;
}


int64_t psm_guard_trips(const psm_handle* h) { return h ? h->guard_trips : -1; }

}  // extern "C"
