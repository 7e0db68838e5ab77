// psm_handle.h -- INTERNAL to libpsm_hip.so: the handle behind include/psm.h and the helpers its translation units share.
// The C-ABI is implemented in twenty files along the seams of the path (nothing here is exported: namespace psm_impl is hidden):
//   psm_api_model.cpp       psm_create / psm_destroy, model artefacts (PCA bases, scaler, Dense / Conv1D / attention / LayerNorm), packing
//   psm_api_plan.cpp        psm_plan_grid (block layout, workspaces), psm_bind_geometry* (bound-geometry tables, closed-form chain)
//   psm_api_solve.cpp       one solve: its route (choose_route), launch sequence (launch_all, a function per stage), argument builders, psm_solve_grid*
//   psm_api_step.cpp        the step around a solve (solve_device: StepCall, step_check, row scale, graph capture and key) and the guarded host loop of every host entry
//   psm_api_ring.cpp        the pinned submission ring (psm_ring_*, psm_submit_grid*, psm_wait_grid) and registered host memory (psm_host_*)
//   psm_api_mesh.cpp        the solver boundary (psm_set_geometry / psm_solve*; the case batch psm_set_geometry_cases / psm_solve_cases*; host tables of both in psm_mesh_tables.cpp), psm_mesh_to_grid
//   psm_api_delta.cpp       the delta step at the solver boundary (dU -> dp, U(t-1) on the device): psm_delta_prime* / _reset / _state, psm_solve_delta*, psm_solve_cases_delta*
//   psm_api_eval.cpp        evaluator helpers on the planned grid: psm_reassemble, psm_label_blocks, psm_block_error
//   psm_api_integ.cpp       the gradP integration: tables, host entry and the device-resident U -> p (psm_set_integration ... psm_solve_pressure)
//   psm_api_filter.cpp      the Gaussian post-steps: psm_gaussian_filter (host entry), psm_bind_poststeps and the device-resident / case-batched entries
//   psm_api_features.cpp    the pressureSM_Poisson input features: the host entry psm_poisson_features; on the device psm_bind_features, psm_features_device and the whole step psm_poisson_step*
//   psm_api_frames.cpp      frames of cell columns -> planes on the device: psm_bind_frames, psm_frames_to_grid_device and the evaluator's step psm_poisson_frames*; what the three evaluator bindings below share (EvalSet / EvalKind: eval_free, eval_state, eval_image_call, eval_bind)
//   psm_api_errors.cpp      the per-frame error blocks of assembled fields on the device: psm_field_errors_device and the metrics-only frame step psm_poisson_frames_errors* (host arithmetic: psm_errors.cpp)
//   psm_api_deltas_frames.cpp  the deltas evaluator's frame batch on the device: psm_bind_deltas_frames, the image pack psm_deltas_image_device (kernels of the three packs: psm_pack.hip), the batched block errors psm_block_errors_device and the step psm_deltas_frames*
//   psm_api_gradp_frames.cpp   the U_to_gradP evaluator's frame batch on the device: psm_bind_gradp_frames, the image / label pack psm_gradp_image_device and the step psm_gradp_frames* (columns -> p -> errors)
//   psm_api_chapter4_frames.cpp  the Chapter-4 evaluators' frame batch on the device: psm_bind_chapter4_frames, the image / label pack psm_chapter4_image_device and the step psm_chapter4_frames* (columns -> p -> errors)
//   psm_api_rows.cpp        a frame's dataset rows -> scalars + columns on the device: psm_bind_rows, the stage alone psm_rows_prepare_device and the evaluators' steps behind it, psm_deltas_rows* / psm_poisson_rows* / psm_gradp_rows*
//   psm_api_poisson_solve.cpp  the Poisson-model step at the solver boundary (cells -> p, two-frame state on the device): psm_bind_poisson_solve, psm_poisson_solve_push / _reset / _state, psm_solve_poisson*; for a case set psm_bind_poisson_solve_cases, psm_poisson_solve_push_cases, psm_solve_cases_poisson*
//   psm_api_gradp_solve.cpp  the gradient-model step at the solver boundary (cells -> p through solve, integration and the outlet level, no state): psm_bind_gradp_solve, psm_solve_gradp*; for a case set psm_bind_gradp_solve_cases, psm_solve_cases_gradp*
//   psm_api_trust.cpp       the input-trust score of the last solve (per-block PCA reconstruction residual): psm_bind_trust, psm_trust_last*
//   psm_api_introspect.cpp  psm_read_stage, profiling and kernel timing, host-side reference reassembly
// The PSM_* environment switches of all of them are read in psm_switches.cpp (host only): psm_create and psm_plan_grid fill h->sw, the
// bind entries and a solve read theirs at the entry, the rest is one process-wide table.  No file above reads the environment itself.
// Compiled with hipcc for gfx950 only.  There is no CPU fallback: without a usable device psm_create fails with PSM_ERR_NO_DEVICE.
#pragma once
#include <hip/hip_runtime.h>

#include "psm_alloc.h"

#include <sched.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/psm.h"
#include "psm_kernels.h"
#include "psm_mesh.h"
#include "psm_pack.h"
#include "psm_rows.h"
#include "psm_eval.h"
#include "psm_filter.h"
#include "psm_integ.h"
#include "psm_features.h"
#include "psm_trust.h"
#include "psm_plan.h"
#include "psm_fold.h"
#include "psm_errors.h"
#include "psm_switches.h"

struct PsmMeshCaseTables;   // psm_mesh_tables.h

namespace psm_impl __attribute__((visibility("hidden"))) {
extern thread_local std::string g_create_error;   // message of the last failed psm_create (psm_api_model.cpp)

// The ring keeps PSM_RING_SLOTS tickets in flight on their own streams, each stream with copy and kernel work; with the HIP
// runtime's default number of hardware queues streams share queues and neighbouring tickets end up behind each other
// (measured with 8 slots: 50 us per solve with 8 queues, 40 with 4, 34-35 with 12 / 16 / 32).  The runtime reads
// GPU_MAX_HW_QUEUES once, when it initialises: that is the HOST PROGRAM's choice (bench.py and INTEGRATION.md set 16) --
// the library never touches the environment of the process it is loaded into.

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct DenseLayer {
  int n_in = 0, n_out = 0, Kpad = 0, ldw = 0, Kp = 0;
  float* W = nullptr;      // [Kpad][ldw] (bf16 precision: bf16 elements)
  void* Wp = nullptr;      // MFMA-packed copy, see psm_dense_kernel
  float* b = nullptr;
  bool set = false;
  bool linear = false;     // hidden layer without ReLU (the folded attention block of densePCA_attention)
  // LayerNormalization behind this layer (densePCA_attention, NNs.py:56, 64): act = LN(act [+ this layer's input]) * gamma + beta
  bool ln = false, ln_residual = false;
  float *ln_gamma = nullptr, *ln_beta = nullptr;
  float ln_eps = 1e-3f;
};

struct Conv1dLayer {            // conv1D_PCA head (NNs.py:75-124)
  int k = 0, cin = 0, cout = 0;
  float *W = nullptr, *b = nullptr;
  bool set = false;
};

// What the most recent solve left on ws0 (psm_read_stage and psm_block_error read it), derived from the route by launch_all when the
// launches are enqueued or captured.  A graph replay does not run launch_all: the record stored at capture is put back.
struct Ws0Solve {
  bool on_ws0 = false;                  // the solve ran on the handle's own workspace, not a ring slot's (then the rest is stale)
  // it stored the decoded blocks (general path; the bound path pastes them) / took the closed form (offsets and shift are computed on
  // demand) / left its last hidden activation in MFMA operand order (PsmDenseArgs::out_packed: readers take d_act_rows)
  bool pred_stored = false, used_cf = false, act_packed = false;
  const float* row_scale = nullptr;     // its row scale
  const float* res = nullptr;           // where its network output rows [cases * B][ld_out] are when not in ws0.d_res (psm_deltas_frames*: one solve per frame)
  // the image its encode read and its case count (psm_trust_last* scores exactly that chain: an evaluator's step leaves its last
  // frame's single-case solve).  Null once the buffer that held an image of the library's own is released (image_gone).
  const float* grid = nullptr;
  int n_cases = 0;
};

// Every decision of one solve's launch sequence, made once by choose_route (psm_api_solve.cpp) from the handle, the workspace, the grid
// pointer and the case count; the stage functions and the argument builders branch on nothing else.
struct SolveRoute {
  int n_cases = 0, M = 0, Mpad = 0;     // block rows, padded to the 32-row MFMA tile
  bool bf16 = false;
  bool bound = false;                   // geometry-bound path (6 / 7 launches), else the general path
  bool cf = false;                      // bound: closed form of the offset chain (pair dots, no chain launch)
  bool guard = false;                   // bound: guard riders check the grid's flow-cell pattern (fold: the SDF channel's values)
  bool fold = false;                    // bound single case: the encode contracts the c_in - 1 leading channels, the SDF channel's share of the
                                        // coefficients comes from the binding (PsmEncodeArgs::fold, PsmReduceArgs::ib_stride); PSM_SDF_FOLD=0: off
  int guard_wgs = 0;                    // guard workgroups of the solve (one flag each)
  bool spread = false;                  // they are dealt over the `rider_carriers` hidden Dense launches, `rider_share` each; the head launch
  int rider_share = 0, rider_carriers = 0;   // (bf16 handles: their dots launch) carries the rest.  Not spread: all of them ride there
  bool stamp_encode = false;            // encode timed by dispatch stamps (no event pair around the launch)
  int aligned = 0, whole = 1, x6 = 0, kgroup = 1, n_slabs = 0;   // encode: PsmEncodeArgs fields of the same name; slabs the reduce sums
  int row_wgs = 1;                      // encode, x6 form of two to four row tiles: workgroups per slice (2: PSM_ENCODE_ROWSPLIT)
  bool fuse1 = false;                   // slab reduce + Dense 0 in one launch
  std::vector<char> packed;             // [layers] the output of Dense layer l is written in MFMA operand order
  bool ln_fuse = true;                  // LayerNormalization deferred into the next hidden launch where there is one
  int decode_x6 = 0;                    // bound: x6 arithmetic of decode + paste
  int decode_mtc = 1, decode_wgs = 512; // bound case batch: row tiles per chunk (1..3) and workgroup target of decode + paste
  bool one_launch_tail = false;         // bound: decode + chain + paste in one launch (single case of <= 64 blocks), else chain launch + batch paste
  uint32_t field_bytes = 0;             // bound: the paste stores through a buffer descriptor of this size (PsmBoundArgs::field_bytes)
  bool fused_assemble = false;          // general: chain + paste in one launch
  bool pred_stored = false;             // the decode stores the blocks
};

// What the Gaussian post-steps behind a solve read and write (psm_solve_poststeps*): every pointer is part of the captured launches.
struct PostCall {
  int apply_filter = -1;                // -1: no post-steps
  const float *dU = nullptr, *prev = nullptr;        // dU == nullptr: filter only
  float *result = nullptr, *change = nullptr, *next = nullptr;
  auto tie() const { return std::tie(apply_filter, dU, prev, result, change, next); }
};

// The Poisson input features in front of a solve (psm_poisson_step*): both pointers are part of the captured launches.
struct FeatCall {
  const double* vel = nullptr;          // [n_cases][4][ny*nx] velocity planes; nullptr: no features stage
  float* grid = nullptr;                // the image the two launches write and the solve reads
  auto tie() const { return std::tie(vel, grid); }
};

// The rows -> scalars + columns stage at the head of an evaluator's frame step (psm_*_rows*): everything the two launches hold.  The
// frame's scalars reach the step's kernels through the device arrays those read anyway (the workspace's row scale, the deltas
// binding's U^2, the feature binding's (L, U)): with this stage in the step nothing is uploaded in front of the replay.
struct RowsCall {
  const float* rows = nullptr;          // [n_frames][n_cells][width]; nullptr: no rows stage
  int kind = 0, width = 0;
  double* cols = nullptr;               // [n_frames][n_cells][k] what the mesh -> grid stage reads
  double* scalars = nullptr;            // [n_frames][8]
  int64_t n_cells = 0;
  double base = 1.0, phi = 1.0, ex = 1.0, ey = 1.0;
  bool wired = false;                   // a step: the finish launch also writes the device arrays the step's kernels read
  bool scaled() const { return rows && wired && kind != PSM_ROWS_KIND_GRADP; }   // ... among them the solve's row scale
  auto tie() const { return std::tie(rows, kind, width, cols, scalars, n_cells, base, phi, ex, ey, wired); }
};

// The mesh -> grid stage in front of the features (psm_poisson_frames*): the launch holds the column array and the k plane descriptors.
struct FrameCall {
  const double* cols = nullptr;         // [n_frames][n_cells][k]; nullptr: no frame stage
  int k = 0, fill = 1;
  PsmFramePlane out[PSM_FRAME_MAX_COLS] = {};
  struct Key {                          // (a type of this namespace: what is instantiated over it stays out of the exported symbols)
    std::array<int64_t, 3 + 3 * PSM_FRAME_MAX_COLS> a{};
    bool operator<(const Key& o) const { return a < o.a; }
  };
  Key key() const {                     // everything the captured launch holds, as one comparable value
    Key key;
    auto& a = key.a;
    a[0] = (int64_t)reinterpret_cast<intptr_t>(cols); a[1] = k; a[2] = fill;
    for (int c = 0; c < k && c < PSM_FRAME_MAX_COLS; ++c) {
      a[3 + 3 * c] = (int64_t)reinterpret_cast<intptr_t>(out[c].dst); a[4 + 3 * c] = out[c].frame_stride; a[5 + 3 * c] = out[c].as_f32;
    }
    return key;
  }
};

// The image pack between the mesh -> grid stage and the solve (psm_deltas_frames*): every pointer is part of the captured launch; the
// SDF plane, the scales and the per-frame U^2 array are the binding's (DeltasSet), which drops these graphs when it goes.
struct DeltasCall {
  const double* planes = nullptr;       // [n_frames][3][npix] what the frame stage wrote; nullptr: no pack stage
  float *grid = nullptr, *label = nullptr;
  double* truth = nullptr;
  float* res = nullptr;                 // the binding's copy of every frame's network output rows (the frames are solved one by one)
  auto tie() const { return std::tie(planes, grid, label, truth); }   // not res: the binding's buffer, the same for every call
};

// The image / label pack between the mesh -> grid stage and the solve, and the integration behind the solve (and its filter), of the
// U_to_gradP evaluator's frame batch (psm_gradp_frames*): every pointer is part of the captured launches; the SDF plane, the scales
// and the integration tables are the binding's (GradpSet), which drops these graphs when it goes.
struct GradpCall {
  const double* planes = nullptr;       // [n_frames][5][npix] what the frame stage wrote; nullptr: no pack stage
  float* grid = nullptr;
  double* truth = nullptr;
  float* p = nullptr;                   // [n_frames][npix] where the binding's integration writes p
  auto tie() const { return std::tie(planes, grid, truth, p); }
};

// The image / label pack between the mesh -> grid stage and the solve of the Chapter-4 evaluators' frame batch (psm_chapter4_frames*):
// every pointer is part of the captured launch; the SDF plane and the scales are the binding's (Chapter4Set), which drops these
// graphs when it goes.
struct Chapter4Call {
  const double* planes = nullptr;       // [n_frames][c_in][npix] what the frame stage wrote; nullptr: no pack stage
  float* grid = nullptr;
  double* truth = nullptr;
  auto tie() const { return std::tie(planes, grid, truth); }
};

// The mesh ends of the Poisson-model step at the solver boundary (psm_solve_poisson*): two launches in front of the features (partial
// maxima; mesh -> grid of the six columns gathered from cells + state, the step's scalars into the device arrays the chain reads)
// and one behind the post-steps (grid -> mesh, p(t-1) + dp, the state turned over).  Every member is held by the captured launches;
// the state, the partials and the tables are the binding's (PoissonSolveSet) and the mesh's, which drop these graphs when they go.
struct PoissonSolveCall {
  const double* cells = nullptr;        // [N,5]; nullptr: no such stage
  double* p = nullptr;                  // [N]
  double* scalars = nullptr;            // [8]
  int weighting = 0, prime = 0, frames = 0;   // prime: the push alone is a plain launch, never part of a sequence (always 0 in one); frames held before the call
  int cases = 0;                        // 0: the single mesh; K: the case set's form (psm_solve_cases_poisson*): cells [sum n_i, 5], p [sum n_i], scalars [K][8]
  auto tie() const { return std::tie(cells, p, scalars, weighting, prime, frames, cases); }
};

// The mesh ends of the gradient-model step at the solver boundary (psm_solve_gradp*): psm_solve's two head launches in front of the
// solve and, behind the optional filter, the two integration launches on the binding's own tables and the tail launch (grid -> mesh
// of q = p / U^2 with the outlet level).  Every member is held by the captured launches; the tables, the scalar slots and the planes
// are the binding's (GradpSolveSet) and the mesh's, which drop these graphs when they go.
struct GradpSolveCall {
  const double* cells = nullptr;        // [N,5]; nullptr: no such stage
  double* p = nullptr;                  // [N]
  float* image = nullptr;               // [K][npix][3] the image the head writes and the solve reads
  float* gradp = nullptr;               // [K][npix][2] the gradient behind the filter: what the integration reads
  float* q = nullptr;                   // [K][npix] the integrated plane
  double* scalars = nullptr;            // [K][8]
  int apply_filter = 0;
  int cases = 0;                        // 0: the single mesh; K: the case set's form (psm_solve_cases_gradp*)
  auto tie() const { return std::tie(cells, p, image, gradp, q, scalars, apply_filter, cases); }
};

// What surrounds ONE solve (solve_device, psm_api_step.cpp), in launch order; every stage keeps its own "absent" value.  A new stage
// is one member here and one entry in key(): the graph cache compares nothing else, so a stage in the sequence is in the cache key.
struct StepCall {
  RowsCall rows{};                      // psm_*_rows*: the two launches that make the columns and the frame scalars (rows == nullptr: none)
  FrameCall frames{};                   // psm_poisson_frames*, psm_deltas_frames*, psm_gradp_frames*: the mesh -> grid launch (cols == nullptr: none)
  FeatCall feat{};                      // psm_poisson_step*: the two feature launches write the solve's image (vel == nullptr: none)
  DeltasCall deltas{};                  // psm_deltas_frames*: the image pack, the frames solved one by one (planes == nullptr: none)
  GradpCall gradp{};                    // psm_gradp_frames*: likewise, and BEHIND the post-steps the integration with the binding's own tables
  Chapter4Call chapter4{};              // psm_chapter4_frames*: the image pack, the frames solved one by one; nothing behind the solve
  float* p = nullptr;                   // psm_solve_pressure*: where the bound integration (psm_bind_integration) behind the solve writes p
  PostCall post{};                      // psm_solve_poststeps*: the bound post-steps behind the solve (apply_filter == -1: none)
  PoissonSolveCall psolve{};            // psm_solve_poisson*: the head in front of the features, the tail behind the post-steps (cells == nullptr: none)
  GradpSolveCall gsolve{};              // psm_solve_gradp*: psm_solve's head in front of the solve; behind it (and the filter) the integration and the tail (cells == nullptr: none)
  auto key() const { return std::make_tuple(rows.tie(), frames.key(), feat.tie(), deltas.tie(), gradp.tie(), chapter4.tie(), p, post.tie(), psolve.tie(), gsolve.tie()); }
  const char* fault() const {           // the combinations the sequence does not define (null: defined); no C entry builds one
    const bool fr = frames.cols, ft = feat.vel, dl = deltas.planes, gp = gradp.planes, c4 = chapter4.planes;
    if (psolve.cells && (!ft || post.apply_filter < 0)) return "the Poisson solver step is the features, the solve and the post-steps between its mesh ends: it needs all three";
    if (psolve.cells && (rows.rows || fr || dl || gp || c4 || p)) return "the Poisson solver step writes the feature planes itself: no rows, frames, pack or integration stage beside it";
    if (psolve.cells && psolve.prime) return "a priming step of the Poisson solver step is one plain launch, not a sequence";
    if (gsolve.cells && (!gsolve.p || !gsolve.image || !gsolve.gradp || !gsolve.q || !gsolve.scalars)) return "the gradient solver step needs the gradP handle's image, gradient, plane and scalar slots";
    if (gsolve.cells && (rows.rows || fr || ft || dl || gp || c4 || p || psolve.cells)) return "the gradient solver step writes its image and integrates itself: no rows, frames, features, pack, integration or Poisson stage beside it";
    if (gsolve.cells && (post.apply_filter >= 0) != (gsolve.apply_filter != 0)) return "the gradient solver step has the filter among the post-steps or no post-steps at all";
    if (gsolve.cells && post.dU) return "the gradient solver step has no weighting: filter only";
    if (rows.rows && (!fr || rows.cols != frames.cols)) return "the rows stage writes the columns the mesh -> grid stage reads: it needs frames on its columns";
    if (dl && gp) return "the deltas and the gradP pack exclude each other";
    if (c4 && dl) return "the Chapter-4 and the deltas pack exclude each other";
    if (c4 && gp) return "the Chapter-4 and the gradP pack exclude each other";
    if (c4 && !fr) return "the Chapter-4 pack reads the planes of the mesh -> grid stage: it needs frames";
    if (c4 && ft) return "the features and the Chapter-4 pack both write the solve's image";
    if (c4 && p) return "the Chapter-4 frames solve p itself: no bound integration behind them";
    if (c4 && post.apply_filter >= 0) return "the Chapter-4 frames have no post-steps: the reference cannot process a filtered field";
    if ((dl || gp) && !fr) return "an image pack reads the planes of the mesh -> grid stage: it needs frames";
    if (ft && (dl || gp)) return "the features and an image pack both write the solve's image";
    if (p && gp) return "the gradP frames integrate with their own tables: not the bound integration as well";
    if (fr && !ft && !dl && !gp && !c4) return "frames alone: nothing reads the planes (features or an image pack)";
    return nullptr;
  }
};

struct GraphKey {
  int n; const void* g; void* f;        // n: sequence_key(); the solve's grid and field
  StepCall step{};
  auto key() const { return std::make_tuple(n, g, f, step.key()); }
  bool operator<(const GraphKey& o) const { return key() < o.key(); }
};

// Everything ONE in-flight solve writes.  The handle owns one for the synchronous / device entries (ws0) and one per
// ring slot, so that the solves of neighbouring tickets run on their own streams without sharing scratch.
struct Workspace {
  float *d_part = nullptr, *d_xin = nullptr, *d_act[2] = {nullptr, nullptr}, *d_res = nullptr, *d_pred = nullptr;
  float* d_act_rows = nullptr;          // row-major copy of the last hidden activation when the chain between the Dense launches is packed (large batches)
  float *d_row_scale = nullptr;
  float4* d_spart = nullptr;
  float2* d_colpart = nullptr;
  float *d_offs = nullptr, *d_shift = nullptr;
  float* d_dots = nullptr;            // strip dots of the geometry-bound path (allocated by the bind)
  float* d_dots2 = nullptr;           // pair dots of the closed-form chain (allocated by the bind)
  float* d_c1[2] = {nullptr, nullptr}; // Conv1D activations of the conv1D_PCA head (ping-pong), [Mpad][c1_stride]
  float* d_gflags = nullptr;          // guard flags of the bound-geometry contract (psm_kernels.h PsmGuardArgs; allocated by the bind)
  int gidx = 0;                       // this workspace's word in the handle's mapped guard page (0 = ws0, 1 + i = ring slot i)
};

// Device tables of one integration binding (PsmIntegArgs, psm_integ.h) and the handle's own gradient / pressure buffers.
struct IntegSet {
  bool ready = false;
  int n_cases = 0;
  int2 *d_fix = nullptr, *d_cuts = nullptr, *d_npair = nullptr;
  uint8_t* d_mask = nullptr;
  float4* d_aux = nullptr;
  float *d_gradp = nullptr, *d_p = nullptr;
  PsmIntegArgs args{};
};

// The device tables of a mesh, or of K meshes concatenated in the layout of PsmMeshCasesArgs (host side: PsmMeshCaseTables,
// psm_mesh_tables.h): uploaded by mesh_tables_upload, released by mesh_tables_free (both in psm_api_mesh.cpp).
struct MeshTablesDev {
  int64_t* off = nullptr;               // [K + 1]
  int32_t *vtx_m2g = nullptr, *src_of_cell = nullptr, *vtx_g2m = nullptr, *cell_of_point = nullptr;
  double *wts_m2g = nullptr, *sdf = nullptr, *wts_g2m = nullptr;
  uint8_t* near_wall = nullptr;
};

// What the single mesh and the case set hold alike: the tables and every buffer a step touches, so that a step allocates nothing.
// Allocated by mesh_buffers_alloc (with U(t-1) of the delta step, DeltaState below), released by mesh_buffers_free (psm_api_mesh.cpp).
struct MeshBuffers {
  MeshTablesDev t;
  double *d_cells = nullptr, *d_p = nullptr, *d_umax = nullptr, *d_umax_part = nullptr;   // staged cells, p, U_max (one per case), partial maxima
  double *h_cells = nullptr, *h_p = nullptr;   // pinned staging of the host entries
  std::vector<double> h_sdf;            // [K][npix] the raw sdfunct as given to psm_set_geometry*: psm_bind_gradp_solve* builds its integration tables from it
  bool inflight = false;                // a *_begin is enqueued, its *_end not yet called
  double* copy_out = nullptr;           // where *_end copies p to (null: it was DMA'd / stored into the caller's registered array)
};

// The single mesh of psm_set_geometry.  d_umax is one scalar, d_umax_part holds <= 256 partials.
struct MeshSingle : MeshBuffers {
  const double* pinned_cells = nullptr;   // caller buffers registered with psm_pin_buffers (DMA without staging copies)
  double* pinned_p = nullptr;
  double* pinned_p_dev = nullptr;       // device-side address of the registered output (the last kernel writes p straight into it)
  const double* pinned_cells_dev = nullptr;   // device-side address of the registered input (psm_stage_cells_kernel reads it over PCIe)
  hipGraphExec_t graph = nullptr;       // psm_solve on registered buffers: stage + to_grid + the solve + to_mesh as ONE graph replay
  Ws0Solve graph_left;                  // what `graph` leaves on ws0
};

// The case set of psm_set_geometry_cases: K meshes on the planned grid, their tables in the layout of PsmMeshCasesArgs (d_umax [K],
// d_umax_part [K][n_parts]).  A handle holds this or the single mesh of psm_set_geometry.
struct MeshCaseSet : MeshBuffers {
  bool ready = false;
  int n_cases = 0;
  std::vector<int64_t> off;             // [n_cases + 1] host copy of t.off
  PsmMeshCasesArgs args{};              // everything but cells / p_out, which are the call's
};

// The state of the delta step (psm_solve_delta*, psm_solve_cases_delta*; psm_api_delta.cpp): U(t-1) per cell of the single mesh or of
// the case set, allocated with the geometry and gone with it (delta_drop), so that a step allocates nothing.  Written by the last
// launch of a step (psm_to_mesh_kernel, delta form); the host flags follow once the whole chain is enqueued.
struct DeltaState {
  double* d_u_prev = nullptr;           // [sum n_i][2]
  bool primed = false;                  // d_u_prev holds the velocities of a previous step (or of psm_delta_prime*)
  int64_t steps = 0;                    // delta steps taken since the state was last empty (a priming step does not count)
};

// Binding of the Gaussian post-steps to the planned grid (psm_bind_poststeps): the four tap tables and per-case scratch for
// max_cases cases, so that a step allocates nothing and copies nothing.
struct PostSet {
  bool ready = false;
  int r_field[2] = {0, 0}, r_weight[2] = {0, 0};         // radii per axis (y, x)
  float* d_taps = nullptr;                               // the four tables, 16-byte aligned pieces
  const float *w_field[2] = {nullptr, nullptr}, *w_weight[2] = {nullptr, nullptr};
  float *d_tmp_a = nullptr, *d_tmp_b = nullptr, *d_t = nullptr;     // axis-0 outputs of field / weighting input [max_cases][npix][c_out], t [max_cases][npix]
  float* d_fields = nullptr;                             // the solve's field in front of the post-steps [max_cases][npix][c_out]
  float *d_dU = nullptr, *d_prev = nullptr, *d_out = nullptr;       // staging of the host entry (and of psm_time_kernels): [max_cases][npix], d_out x 3
};

// Binding of the pressureSM_Poisson input features to the planned grid (psm_bind_features): the SDF planes of the case slots, the
// bind-time constants and every buffer a step touches, so that a step allocates nothing.
struct FeatureSet {
  static constexpr int RING = 8;
  bool ready = false;
  int n_cases = 0;
  double k = 0.0, max_abs[4] = {1, 1, 1, 1};
  double *d_sdf = nullptr, *d_term = nullptr, *d_partial = nullptr;   // [n_cases][npix], [n_cases][npix], [n_cases][2 * workgroups]
  double* d_lu = nullptr;                                // [n_cases][2] (L, U) of the step: uploaded in front of every call, outside the graph
  float* d_grid = nullptr;                               // the image of psm_poisson_step* [n_cases][npix][4]
  double* d_vel = nullptr;                               // staging of the host entry (and of psm_time_kernels) [n_cases][4][npix]
  double* h_lu = nullptr;                                // pinned upload ring [RING][n_cases][2]
  hipEvent_t lu_ev[RING] = {};
  int lu_pos = 0;
};

// Binding of the frame batch to the single mesh of psm_set_geometry (psm_bind_frames): what the host entry psm_poisson_frames stages
// through, so that a step allocates nothing.  The device entries hold no table of their own: they read the mesh's.
struct FrameSet {
  bool ready = false;
  int n_frames = 0, k = 0;
  double* d_cols = nullptr;             // [n_frames][n_cells][k]
  double* d_extra = nullptr;            // [n_frames][k][npix]: the float64 planes of the columns between the velocities and the weighting pair
  double *h_cols = nullptr, *h_extra = nullptr;   // pinned copies of the two
  float* h_out = nullptr;               // pinned [n_frames][npix][c_out + 2]: result, change, next
  double *d_raw = nullptr, *h_raw = nullptr;   // psm_poisson_frames_errors: [n_frames][3][8] sums, device and pinned
};

// Binding of the Poisson-model step at the solver boundary (psm_bind_poisson_solve, behind psm_bind_features, psm_bind_poststeps and
// psm_bind_frames on the single mesh; psm_bind_poisson_solve_cases, behind the first two on a case set): the step's constants, the
// two-frame state, the partial maxima and the scalar slots, so that a step allocates nothing.  The state is written by the last launch
// of a step; the host counters follow once the whole step is enqueued.  A case set has ONE frame counter and one step counter; its
// arrays are the single mesh's with N = sum n_i and a row of partials and of scalars per case.
struct PoissonSolveSet {
  bool ready = false;
  int cases = 0;                        // 0: bound on the single mesh; K: bound on a case set of K cases
  double phi = 1.0, max_abs_dp = 1.0;
  int weighting = 0, apply_filter = 0;
  double* d_state = nullptr;            // [5 N]: u_prev [N][2] | du_prev [N][2] | p_prev [N], every piece 16-byte aligned
  double* d_part = nullptr;             // [2][PSM_POISSON_PARTS] ([K] of them for a case set)
  double* d_scalars = nullptr;          // [PSM_POISSON_SCALARS] ([K] of them for a case set)
  int frames = 0;                       // frames held: 0, 1 or 2
  int64_t steps = 0;                    // steps taken since the state was last empty (a priming step does not count)
};

// Binding of the gradient-model step at the solver boundary (psm_bind_gradp_solve on the single mesh, psm_bind_gradp_solve_cases on
// a case set): integration tables of its own from the mesh's raw sdfunct and the caller's cut(s) (integ: K case slots; integ.d_gradp
// and integ.d_p are the step's gradient and q), the image, the field in front of the filter and the scalar slots, so that a step
// allocates nothing.  No state: a step depends on its cells alone.
struct GradpSolveSet {
  bool ready = false;
  int cases = 0;                        // 0: bound on the single mesh; K: bound on a case set of K cases
  int apply_filter = 0, reference = 0;
  double sx = 1.0, sy = 1.0;            // dx * max_abs_dPdx / extent_x, dy * max_abs_dPdy / extent_y
  IntegSet integ;
  float* d_image = nullptr;             // [K][npix][3]
  double* d_scalars = nullptr;          // [K][PSM_GRADP_SCALARS]
};

// Binding of the rows stage (psm_bind_rows, behind psm_bind_frames): staging for the bound frame count x mesh cells x width float32
// rows, the partial maxima and the scalar slots, so that a step allocates nothing.  The columns go to the frame binding's d_cols.
struct RowsSet {
  bool ready = false;
  int n_frames = 0, width = 0;
  float *d_rows = nullptr, *h_rows = nullptr;     // [n_frames][n_cells][width], device and pinned
  float* d_part = nullptr;                         // [n_frames][3][PSM_ROWS_PARTS]
  double *d_scalars = nullptr, *h_scalars = nullptr;   // [n_frames][8], device and pinned
};

// What the three evaluator frame bindings hold alike (psm_bind_deltas_frames, psm_bind_gradp_frames, psm_bind_chapter4_frames, each
// behind psm_bind_frames): the simulation's normalised SDF plane, the scales and the buffers every one of them touches in a step for
// the bound frame count, so that a step allocates nothing.  The columns go through the frame binding's staging (FrameSet::d_cols /
// h_cols).  Allocated by eval_bind, released by eval_free (psm_api_frames.cpp); the sizes that differ are the kind's (EvalKind).
struct EvalSet {
  bool ready = false;
  int n_frames = 0;
  double max_abs[5] = {1, 1, 1, 1, 1};  // the scales the kind checks, in the order of its image and label channels
  double* d_sdn = nullptr;              // [npix] nan0(sdfunct) / max_abs_dist in float64: the SDF channel of the image, and the field errors' mask
  double* d_planes = nullptr;           // [n_frames][cols][npix] float64 planes of the stored columns
  float* d_grid = nullptr;              // image [n][npix][c_in]
  double* d_truth = nullptr;            // [n][truth_planes][npix]
  double *d_raw = nullptr, *h_raw = nullptr;     // [n][raw_rows][8], device and pinned (host entry)
  double* h_truth = nullptr;            // pinned [n][truth_planes][npix]
};

// What differs between the three kinds and is not a buffer, as data: the shared bodies (eval_state, eval_image_call, eval_bind) take one
// of these and never ask which evaluator called.  0 / -1 stand for the value the model's c_in gives.
struct EvalKind {
  const char* bind_name;                // the bind entry, in front of its allocation failures
  int cols;                             // columns stored as planes (0: c_in)
  int scales;                           // max_abs scales checked and kept (0: c_in + 1)
  int dist;                             // index of the distance scale among them (-1: c_in - 1)
  int truth_planes, raw_rows;           // label planes and error blocks per frame
  const char *k_msg, *align_msg, *unbound_msg;
  int n_cols(const psm_config& c) const { return cols ? cols : c.c_in; }
  int n_scales(const psm_config& c) const { return scales ? scales : c.c_in + 1; }
  int dist_at(const psm_config& c) const { return dist >= 0 ? dist : c.c_in - 1; }
};

// The deltas evaluator's frame batch: max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p; planes of columns 0-2; truth [n][npix];
// raw [n][2][8].  On top of the common set the label plane, the field, the block stage's buffers and the U^2 ring.
struct DeltasSet : EvalSet {
  static constexpr int RING = 8;
  float *d_label = nullptr, *d_result = nullptr;   // label plane [n][npix], field [n][npix]
  float* d_res = nullptr;               // [round_up(n * B, 32)][ld_out] network output rows of the step's frames, for the block stage
  double *d_part = nullptr, *d_fraw = nullptr;   // block partials [n][B][8]; the field's sums [n][8] in front of the fold
  float* h_result = nullptr;            // pinned [n][npix]
  double *d_u2 = nullptr, *h_u2 = nullptr;       // U^2 of the step's frames [n]; pinned upload ring [RING][n]
  hipEvent_t u2_ev[RING] = {};
  int u2_pos = 0;
};

// The U_to_gradP evaluator's frame batch: scales of grid channels 0-4 (Ux, Uy, SDF, dPdx label, dPdy label); planes of columns 0-4;
// truth [n][3][npix] (grid channels 3-5); raw [n][4][8].  On top of the common set integration tables OF ITS OWN (the simulation's
// one geometry and cut, replicated per frame slot so that the integration kernels index them by case as ever; h->integ_dev and
// h->integ_host are not touched).
struct GradpSet : EvalSet {
  IntegSet integ;                       // the tables; integ.d_gradp [n][npix][2] and integ.d_p [n][npix] are the step's gradient and p
  float *h_gradp = nullptr, *h_p = nullptr;      // pinned [n][npix][2], [n][npix]
};

// The Chapter-4 evaluators' frame batch: scales [c_in + 1] (the c_in - 1 input channels, dist, p); planes of columns 0 .. c_in - 1;
// truth [n][npix]; raw [n][1][8].  No block stage and no U^2 ring: prediction and label are compared in normalised units.
struct Chapter4Set : EvalSet {
  float* d_result = nullptr;            // field [n][npix]
  float* h_result = nullptr;            // pinned [n][npix]
};
}  // namespace psm_impl
using namespace psm_impl;

namespace psm_impl __attribute__((visibility("hidden"))) {
// Binding of the input-trust score (psm_bind_trust): the Gram matrix of the input basis and every buffer a call touches, so that
// psm_trust_last* allocates nothing.  The mean is the handle's own d_mean_in, which is in natural order.
struct TrustSet {
  bool ready = false;
  int bands = 0;
  double* d_gram = nullptr;             // [p_in][p_in] C C^T of the float32 basis, float64
  double* d_part = nullptr;             // [max_cases][B][bands]
  double *d_out = nullptr, *h_out = nullptr;   // [max_cases][B][2], device and pinned: the host entry's staging
};
}  // namespace psm_impl

struct psm_handle {
  psm_config cfg{};
  std::string err;
  int S = 0, ov = 0, K_in = 0, K_out = 0, ld_in = 0, ld_out = 0, NT = 0, n_slices = 0, Gd = 0, n_coltiles = 0;
  bool have_pca = false, have_scaler = false;
  std::vector<DenseLayer> dense;
  std::vector<Conv1dLayer> conv1d;      // in front of the dense layers when the model is the reference's conv1D_PCA
  int64_t c1_stride = 0;                // floats per block row of the Conv1D activation buffers
  float *d_mean_in = nullptr, *d_mean_out = nullptr;
  float4 *d_bpack_in = nullptr, *d_bpack_out = nullptr;
  uint4* d_bpack_x6 = nullptr;          // encode basis as three bf16 planes in MFMA fragment order (pack_comp_in_x6): the large-batch encode
  float *d_ia = nullptr, *d_ib = nullptr, *d_sa = nullptr, *d_sb = nullptr;
  // plan
  bool planned = false;
  PsmPlan plan;
  int Ny = 0, Nx = 0, B = 0, Mcap = 0, Mpad_cap = 0, n_strips = 0, Lmax = 0, max_width = 0;
  bool plan_aligned = false;            // every block origin and the case stride are multiples of four floats: the encode's 16-byte loads
  Workspace ws0;
  int64_t* d_row_base = nullptr;
  float* d_ones = nullptr;
  int32_t *d_strips = nullptr, *d_blk = nullptr, *d_owner = nullptr, *d_shiftA = nullptr, *d_shiftB = nullptr, *d_shiftOwnA = nullptr, *d_shiftOwnB = nullptr;
  float* d_shiftW = nullptr;
  PsmBlock* d_blocks = nullptr;
  int n_bands = 0;
  unsigned long long* d_stamps = nullptr;
  double* d_err_part = nullptr;         // partials of psm_field_errors_device: [max_cases][PSM_FIELD_ERR_MAX_PAIRS][workgroups][8], sized by the plan
  // mesh-side tables (psm_set_geometry)
  bool have_geometry = false, have_g2m = false;
  int64_t n_cells = 0;
  MeshSingle mesh;
  MeshCaseSet mcs;                      // or a case set (psm_set_geometry_cases): setting one drops the other
  DeltaState delta;                     // U(t-1) of psm_solve_delta* / psm_solve_cases_delta*, allocated with either of the two
  // U_to_gradP integration: the evaluator's single geometry of any size (psm_set_integration, host buffers) and the case
  // batch on the planned grid (psm_bind_integration, device buffers)
  IntegSet integ_host, integ_dev;
  PostSet post;                         // Gaussian post-steps on the planned grid (psm_bind_poststeps)
  FeatureSet feat;                      // Poisson input features on the planned grid (psm_bind_features)
  FrameSet frames;                      // frame batch on the single mesh (psm_bind_frames)
  RowsSet rows;                         // the rows stage's staging behind it (psm_bind_rows)
  PoissonSolveSet psolve;               // the Poisson-model step at the solver boundary behind features, post-steps and frames (psm_bind_poisson_solve) or behind features and post-steps on a case set (psm_bind_poisson_solve_cases)
  GradpSolveSet gsolve;                 // the gradient-model step at the solver boundary on the mesh or the case set (psm_bind_gradp_solve*)
  TrustSet trust;                       // the input-trust score of the last solve (psm_bind_trust)
  DeltasSet deltas;                     // the deltas evaluator's frame batch behind it (psm_bind_deltas_frames)
  GradpSet gradp;                       // the U_to_gradP evaluator's frame batch behind it (psm_bind_gradp_frames)
  Chapter4Set chapter4;                 // the Chapter-4 evaluators' frame batch behind it (psm_bind_chapter4_frames)
  double maxs[4] = {1, 1, 1, 1};
  int normalise_sdf = 0, fill_input = 0;
  double case_maxs[4] = {1, 1, 1, 1}, case_delta = 5e-3, case_wall = 0.05;   // psm_set_case (PM:106-109, 195, 494)
  int case_every = 10;                                                        // PM:94-95
  float *d_grid_stage = nullptr, *d_fields_stage = nullptr;
  float *h_grid = nullptr, *h_fields = nullptr;
  // host-buffer submission ring (psm_submit_grid / psm_wait_grid): pinned in/out + device in/out per slot
  // One ring slot = pinned host buffers + device buffers + its own workspace, stream and graphs: the H2D copy, the
  // kernels and the D2H copy of a ticket run in order on the slot's stream, different slots overlap freely.
  struct Slot {
    float *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr, *h_rs = nullptr;
    float *m_in = nullptr, *m_out = nullptr, *m_rs = nullptr;   // device-side addresses of the pinned buffers (mapped)
    Workspace ws;
    const float* last_src = nullptr;   // what the ticket in flight was launched with (re-run on the general path when
    float* last_dst = nullptr;         // the guard of the bound-geometry contract trips)
    std::vector<float> last_scale;
    hipStream_t st = nullptr;
    hipEvent_t ev_out = nullptr;
    hipGraphExec_t g_full = nullptr, g_kern = nullptr;   // H2D + kernels + D2H on the slot's own buffers / the kernels alone
    int g_full_key = -1, g_kern_key = -1;
    int state = 0;             // 0 free, 1 acquired (the caller is packing), 2 in flight
    int64_t ticket = -1;
    int n_cases = 0;
    float* user_out = nullptr; // where psm_wait_grid copies to when the caller gave the pointer at submission
    bool direct_out = false;   // the D2H went straight into user_out (registered memory)
  };
  static constexpr int SLOTS = PSM_RING_SLOTS;
  Slot slot[SLOTS];
  bool ring_ready = false;
  int ring_slots = SLOTS;      // slots in rotation (PSM_RING_USE=n, n <= PSM_RING_SLOTS: experiments)
  int ring_graph = 1;          // PSM_RING_GRAPH=0: plain launches on the slot streams
  int ring_dma = 1;            // PSM_RING_PULL=1 clears it: the GPU pulls the grid from / stores the field to the mapped pinned
                               // buffers itself instead of hipMemcpyAsync (SDMA) copies around the kernels -- measured slower
  int64_t next_ticket = 0;
  struct HostReg { char* base; size_t bytes; char* dev; };
  std::vector<HostReg> host_regs;                    // psm_host_register
  // row-scale upload ring (pinned)
  static constexpr int RING = 8;
  float* h_scale[RING] = {};
  hipEvent_t scale_ev[RING] = {};
  int scale_pos = 0;
  hipStream_t stream = nullptr;
  struct SolveGraph { hipGraphExec_t exec; Ws0Solve left; };   // left: what the captured solve leaves on ws0
  std::map<GraphKey, SolveGraph> graphs;
  PsmSwitches sw;                       // at_create: psm_create, at_plan: psm_plan_grid (psm_switches.h); the fields below named after a switch are filled from it
  bool use_graph = true;
  bool fused_assemble = false;
  // scratch of the helper entries (gaussian filter, mesh -> grid, Poisson features, gradp integration): one device and one
  // pinned host buffer, grown on demand and reused -- a hipMalloc / hipFree pair per call cost more than the kernels
  void *scr_dev = nullptr, *scr_pin = nullptr;
  size_t scr_dev_cap = 0, scr_pin_cap = 0;
  // geometry-bound fast path (psm_bind_geometry): tables of psm_kernels.h PsmBindArgs
  bool bound = false, bound_zero_fill = false;
  int bound_scope = 0;                  // 2: every single-case solve (psm_bind_geometry); 1: psm_solve only (bound by psm_set_geometry)
  bool in_mesh_solve = false;
  int bound_rows = 0;                   // table rows per case
  int bound_cases = 0;                  // cases bound (solves with exactly this many cases take the bound path)
  float *d_comp_nat = nullptr;          // comp_out in natural layout [ld_out][K_out] (f32 precision only)
  float *d_g2 = nullptr, *d_c2 = nullptr, *d_cnt = nullptr;
  size_t bound_dots = 0;                // floats of Workspace::d_dots
  std::vector<uint8_t> bound_mask;      // [bound_cases][Ny*Nx] flow-cell pattern that was bound (psm_bound_mask)
  int32_t* d_row_of = nullptr;
  uint32_t* d_ownbits = nullptr;
  // closed form of the offset chain for case batches (psm_kernels.h PsmBoundBatchArgs): pair tables
  int x6_mode = -1;                     // PSM_X6 at psm_create: -1 default (see launch_all), bit 0 encode, bit 1 bound decode
  bool bound_cf = false;
  size_t cf_rows_all = 0;               // cases * c_out * B * B
  float *d_g2p = nullptr, *d_c2p = nullptr, *d_cntp = nullptr, *d_cfa0 = nullptr;
  int32_t* d_row_of_p = nullptr;
  std::vector<float> h_shiftW;          // host copy of d_shiftW [c_out][B]
  Ws0Solve last;
  // keep mode (PSM_KEEP_HIDDEN=1 at psm_create): hidden Dense layer l of a ws0 solve writes d_keep[l] ([Mpad_cap][max_width],
  // row-major; where the chain is packed, its row-major copy) instead of a ping-pong buffer, for psm_read_stage(PSM_STAGE_HIDDEN + l)
  bool keep_hidden = false;
  std::vector<float*> d_keep;
  // guard of the bound-geometry contract (psm_kernels.h PsmGuardArgs)
  unsigned long long* d_maskbits = nullptr;   // bound flow-cell pattern, one 64-pixel ballot per word
  int guard_ballots = 0, guard_waves = 0;
  bool guard_on = true;                 // PSM_NO_GUARD=1 switches the riders off (diagnostic)
  int *h_guard = nullptr, *m_guard = nullptr;   // mapped pinned page: one word per workspace, raised by a guard wave on mismatch
  float* d_gzero = nullptr;             // one zero: the flags of solves without a guard
  int64_t guard_trips = 0;
  // SDF fold of the bound single-case encode (PsmEncodeArgs::fold, psm_fold.h): float32 handles whose SDF channel
  // is the last one.  psm_set_pca keeps a float32 host copy of comp_in until the first bind that can use it (bind_sdf_fold, psm_api_plan.cpp),
  // which turns it into the basis packed over the leading channels (d_bpack_fold: as many bytes as (c_in - 1) / c_in of d_bpack_in) and
  // the SDF channel's rows; every bind builds the per-row input-scaler offset and keeps the bound SDF image for the guard riders.
  std::vector<float> h_comp_in;         // [p_in][K_in], released by the first fold bind
  std::vector<float> h_comp_sdf, h_mean_sdf;   // [p_in][S*S], [S*S]
  std::vector<float> h_ia, h_ib;        // host copies of d_ia / d_ib
  float4* d_bpack_fold = nullptr;
  float* d_ib_fold = nullptr;           // [32][ld_in]: ib[p] + ia[p] * c_sdf[m][p] (rows beyond B: ib)
  float* d_sdf_bound = nullptr;         // [Ny*Nx] SDF channel of the bound grid
  bool fold_bound = false;              // the three tables above belong to the current binding
  int debug_skip = 0;                   // PSM_DEBUG_SKIP bit mask of kernel groups NOT launched (timing experiments only)
  bool fuse_reduce_dense1 = true;       // PSM_NO_FUSED_REDUCE=1 disables
  int last_cases = 0;
  // event timing of one kernel group
  int timed_kernel = -1;
  int timed_repeat = 1;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timed_events;
  double timed_total_ms = 0.0;
  int64_t timed_launches = 0;
};

namespace psm_impl __attribute__((visibility("hidden"))) {

// ---- helpers shared by the translation units (defined in the file named in the list above) ----
bool sync_blocks();
hipError_t wait_stream(hipStream_t st);
hipError_t wait_event(hipEvent_t ev);
int fail(psm_handle* h, int code, const std::string& msg);
int scratch_reserve(psm_handle* h, size_t dev_bytes, size_t pin_bytes);
void destroy_graphs(psm_handle* h);
// drops the captured solve graphs whose key `gone` names (graphs that hold the addresses of a binding's tables, when the binding goes)
template <typename P>
void drop_graphs_if(psm_handle* h, P gone) {
  for (auto it = h->graphs.begin(); it != h->graphs.end();)
    if (gone(it->first)) { (void)hipGraphExecDestroy(it->second.exec); it = h->graphs.erase(it); } else ++it;
}
void ws_free(Workspace& w);
int ws_alloc_guard(psm_handle* h, Workspace& w);
int ws_alloc(psm_handle* h, Workspace& w);
void ring_drop_graphs(psm_handle* h);
void free_plan(psm_handle* h);
std::vector<float4> pack_comp_in(const double* comp, int P, int K, int c_in, int S, int NT);
std::vector<float4> pack_comp_out(const double* comp, int P, int K_out, int Gd);
void unpin_buffers(psm_handle* h);
void free_geometry(psm_handle* h);
void mesh_cases_free(psm_handle* h);
int mesh_tables_upload(psm_handle* h, MeshTablesDev& dev, const PsmMeshCaseTables& t);
void mesh_tables_free(MeshTablesDev& dev);
// every device and pinned buffer of `b` for total_cells cells, and U(t-1) of the delta step; the tables are the caller's upload.  A
// failure leaves what was allocated to the caller's free function; a failed pinned allocation is host_alloc_err, "hipHostMalloc(<what>): ..."
int mesh_buffers_alloc(psm_handle* h, MeshBuffers& b, size_t total_cells, size_t n_umax, size_t n_partials, int host_alloc_err, const char* what);
void mesh_buffers_free(MeshBuffers& b);   // tables and buffers; U(t-1) goes with delta_drop
void integ_free(IntegSet& s);
int integ_bind(psm_handle* h, IntegSet& s, int ny, int nx, const double* sdfunct, int n_cases, const int32_t* cy, const int32_t* cx,
               double dx, double dy, bool one_geometry = false);
int integrate_device(psm_handle* h, const float* d_gradp, int n_cases, float* d_p, hipStream_t st);
int integrate_device(psm_handle* h, const IntegSet& s, const float* d_gradp, int n_cases, float* d_p, hipStream_t st);
void post_free(PostSet& s);
int poststeps_device(psm_handle* h, const float* d_fields, int n_cases, const PostCall& pc, hipStream_t st);
int post_check(psm_handle* h, int n_cases, const PostCall& pc);
void feat_free(FeatureSet& s);
void frames_free(psm_handle* h);
void deltas_free(psm_handle* h);
void gradp_free(psm_handle* h);
void chapter4_free(psm_handle* h);
void rows_free(psm_handle* h);
void trust_free(psm_handle* h);           // psm_plan_grid drops the trust binding; the model setters clear its flag (psm_api_trust.cpp)
// a buffer of the library's own that held a solve's image is released: psm_trust_last* has no image to score until the next solve
inline void image_gone(psm_handle* h) { h->last.grid = nullptr; }
void poisson_solve_free(psm_handle* h);   // whatever drops the feature, post-step or frame binding, the mesh or the case set drops this one (psm_api_poisson_solve.cpp)
// the two head launches / the tail launch of a Poisson solver step on `st` (the tail's field: next with the weighting, else result)
int poisson_solve_head(psm_handle* h, const PoissonSolveCall& ps, hipStream_t st);
int poisson_solve_tail(psm_handle* h, const PoissonSolveCall& ps, const PostCall& pc, hipStream_t st);
void gradp_solve_free(psm_handle* h);     // whatever drops the mesh or the case set, the plan, the model or (with apply_filter) the post-steps drops this one (psm_api_gradp_solve.cpp)
// the two head launches / the integration and the tail launch of a gradient solver step on `st`
int gradp_solve_head(psm_handle* h, const GradpSolveCall& gs, hipStream_t st);
int gradp_solve_tail(psm_handle* h, const GradpSolveCall& gs, hipStream_t st);
int rows_device(psm_handle* h, const RowsCall& rc, int n_frames, hipStream_t st);
int frames_state(psm_handle* h);
int frames_count_check(psm_handle* h, int n_frames);
int frames_device(psm_handle* h, const FrameCall& fc, int n_frames, hipStream_t st);
int poisson_frame_call(psm_handle* h, const double* d_cols, int n_frames, int k, int weighting, double* d_extra, FrameCall& fc);
int field_errors_device(psm_handle* h, const PsmFieldErrorArgs& stage, double* d_raw, hipStream_t st);
int poisson_step_device(psm_handle* h, const double* d_vel, int n_cases, const double* LU, const float* out_scale, const PostCall& pc,
                        hipStream_t st, const FrameCall* frames = nullptr, const RowsCall* rows = nullptr, const PoissonSolveCall* psolve = nullptr);
PostCall post_call(int apply_filter, const float* dU, const float* prev, float* result, float* change, float* next);
int features_device(psm_handle* h, const double* d_vel, int n_cases, float* d_grid, hipStream_t st);
std::vector<uint16_t> pack_comp_in_bf16(const double* comp, int P, int K, int c_in, int S, int NT);
std::vector<uint16_t> pack_comp_out_bf16(const double* comp, int P, int K_out, int G);
bool model_complete(const psm_handle* h);
int ensure_encode_aux(psm_handle* h, int n_cases);
// ps: the per-solve switches, read once by the entry that starts the solve (solve_device, ring_launch, mesh_sequence) and handed down
SolveRoute choose_route(const psm_handle* h, const Workspace& w, const float* d_grid, int n_cases, bool profiled, const PsmSwitches::PerSolve& ps);
int launch_all(psm_handle* h, Workspace& w, const float* d_grid, int n_cases, float* d_fields, const float* d_row_scale,
               hipStream_t st, hipEvent_t* prof, const PsmSwitches::PerSolve& ps);
bool bound_applies(const psm_handle* h, int n_cases);
bool fold_applies(const psm_handle* h, int n_cases, const PsmSwitches::PerSolve& ps);
int sequence_key(const psm_handle* h, int n_cases, bool scale, const PsmSwitches::PerSolve& ps, bool ring = false);
int capture_graph(psm_handle* h, hipStream_t st, const char* label, const std::function<int()>& enqueue, hipGraphExec_t* exec);
// one builder per kernel-argument block (psm_api_solve.cpp): the stages of launch_all, psm_read_stage, psm_block_error and psm_reassemble
PsmDecodeArgs decode_args(const psm_handle* h, const Workspace& w, int n_cases, const float* row_scale, float* pred, int x6 = 0);
PsmDotsArgs dots_args(const psm_handle* h, const Workspace& w, bool cf, int n_cases, const float* row_scale, const PsmGuardArgs& guard);
PsmStripArgs strip_args(const psm_handle* h, const Workspace& w, const float* d_grid);
PsmChainArgs chain_args(const psm_handle* h, const Workspace& w);
PsmPasteArgs paste_args(const psm_handle* h, const Workspace& w, float* d_fields);
// the two ends of psm_solve on the single mesh (psm_api_mesh.cpp).  U_max: the device scalar d_umax, else umax_val; to_grid folds
// n_partials > 0 partial maxima itself and leaves the scalar in the mesh's d_umax
PsmToGridArgs to_grid_args(const psm_handle* h, const double* d_umax, double umax_val, int n_partials);
PsmToMeshArgs to_mesh_args(const psm_handle* h, const double* d_umax, double umax_val, double* p_out);
// The step entries of the solver boundary, absolute (psm_solve*, psm_solve_cases*) and delta (psm_api_delta.cpp) alike: the same
// checks, copies and launches; `delta` swaps the two mesh ends for their delta forms, keeps off the one-kernel staging route of
// registered buffers and, on a state that is not primed, enqueues the priming step instead (no U_max, no network).
int mesh_step_begin(psm_handle* h, const double* cells, int64_t n, double* p_out, bool delta);
// the state and argument checks of a step on the single mesh, in the step's order; `prime`: those of psm_delta_prime (no p_out, no solve)
int mesh_step_check(psm_handle* h, const double* cells, int64_t n, const double* p_out, bool prime);
int step_end(psm_handle* h, MeshBuffers& b, int64_t total_cells, const char* begin_name);   // behind psm_solve_end and psm_solve_cases_end
int cases_check(psm_handle* h);
int cases_step_device(psm_handle* h, const double* d_cells, double* d_p, void* stream, bool delta);
int cases_step_begin(psm_handle* h, const double* cells, double* p_out, bool delta);
// The host staging of one cells [n,5] -> p [n] step on a mesh's buffers (psm_api_mesh.cpp): one H2D of the cells and one D2H of p,
// straight from / into ranges registered with psm_host_register, else through the pinned staging.  p_out null: no output (a push).
// The caller keeps its own order around the calls: nothing before copy_in may still use the staging (the stream waited for, or the
// in-flight flag), and p is delivered -- memcpy h_p -> pending() -- once the stream has been waited for.
struct HostStaging {
  MeshBuffers& m;
  const double* cells;
  double* p_out;
  size_t in_bytes, out_bytes;
  bool reg_in, reg_out;
  HostStaging(const psm_handle* h, MeshBuffers& m, const double* cells, double* p_out, size_t n);
  hipError_t copy_in(hipStream_t st) const;
  hipError_t copy_out(hipStream_t st) const;
  double* pending() const { return reg_out ? nullptr : p_out; }   // where p is still to be copied to (null: it was DMA'd, or there is none)
  void deliver() const { if (pending()) memcpy(p_out, m.h_p, out_bytes); }
};
// What the entries of a bound step kind at the solver boundary (Poisson model, gradient model) ask before anything else: bound on the
// form the entry serves (cases: 0 the single mesh, 1 a case set, -1 either), bound at all -- `usable`: the binding is ready and what
// else the kind stands on is there --, no step in flight.  The texts are the kind's.
struct BoundStepTexts { const char *on_cases, *on_single, *unbound_cases, *unbound_single; };
int bound_step_state(psm_handle* h, const BoundStepTexts& t, bool ready, int bound_cases, bool usable, int cases);
// The tail of a psm_bind_*_solve* entry: `zero` (pointer, bytes) cleared on the handle's stream and the stream drained; on a failure
// free_fn and the error under the bind entry's name.
int bind_zero_sync(psm_handle* h, const char* name, std::initializer_list<std::pair<void*, size_t>> zero, void (*free_fn)(psm_handle*));
// every pointer of `ps` (null included) is a multiple of `bytes` (a power of two)
inline bool aligned_to(uintptr_t bytes, std::initializer_list<const void*> ps) {
  uintptr_t u = 0;
  for (const void* p : ps) u |= reinterpret_cast<uintptr_t>(p);
  return (u & (bytes - 1)) == 0;
}
void delta_drop(psm_handle* h);       // the geometry or case set goes: so does U(t-1)
// the stages of `step` and the solve between them on one stream / in one graph replay; the combinations of stages: step_check there
int solve_device(psm_handle* h, const float* d_grid, int n_cases, const float* out_scale, float* d_fields,
                 hipStream_t st, hipEvent_t* prof, const StepCall& step = {});
int deltas_pack_device(psm_handle* h, const DeltasCall& dc, int n_frames, hipStream_t st);
int gradp_pack_device(psm_handle* h, const GradpCall& gc, int n_frames, hipStream_t st);
int chapter4_pack_device(psm_handle* h, const Chapter4Call& cc, int n_frames, hipStream_t st);
// what the three evaluator bindings share (psm_api_frames.cpp); the kind is data, none of these asks which evaluator called
void eval_free(EvalSet& s);           // the common buffers and the flags; the kind's *_free drops its graphs and its own buffers first
int eval_state(psm_handle* h, const EvalSet& s, const EvalKind& kind);   // the mesh, the frame binding and this binding
// state and arguments of a kind's image stage; the frame stage's descriptors: the stored columns into the binding's planes, the rest not stored
int eval_image_call(psm_handle* h, const EvalSet& s, const EvalKind& kind, const double* d_cols, int n_frames, int k, const float* d_grid,
                    const double* d_truth, FrameCall& fc);
// The body of a psm_bind_*_frames entry behind its model-shape check: argument checks, nothing in flight, free_fn, `own` (the kind's own
// tables and buffers for n frames of npix pixels, first: what it refuses binds nothing), the common buffers, the SDF plane, the flags.
// Any failure leaves the set freed and not ready.
int eval_bind(psm_handle* h, EvalSet& s, const EvalKind& kind, const double* sdfunct, const double* max_abs, void (*free_fn)(psm_handle*),
              const std::function<int(size_t n, size_t npix)>& own);
// The deltas and the gradP evaluator's frame step behind a device or a host entry, of the _frames and the _rows form alike
// (psm_api_deltas_frames.cpp, psm_api_gradp_frames.cpp): null destinations become the binding's, then the step's checks and its one
// graph replay, then the error stage when d_raw is given.  With `rows` the rows stage heads the step, d_cols are its columns, and U2 /
// out_scale are not read: the finish launch leaves them on the device.  *_host_check: every check of that step on the binding's own
// buffers and nothing else, for a host entry to run before its first copy.
int deltas_frames_step(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, const float* out_scale, int apply_filter,
                       float* d_result, double* d_truth, double* d_raw, hipStream_t st, const RowsCall* rows = nullptr);
int deltas_host_check(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, int apply_filter, const RowsCall* rows = nullptr);
int gradp_frames_step(psm_handle* h, const double* d_cols, int n_frames, int k, const float* out_scale, int apply_filter, float* d_gradp,
                      float* d_p, double* d_truth, double* d_raw, hipStream_t st, const RowsCall* rows = nullptr);
int gradp_host_check(psm_handle* h, const double* d_cols, int n_frames, int k, int apply_filter);
PsmFieldErrorArgs poisson_error_pairs(const psm_handle* h, int n_frames, int n_extra, const double* d_extra, const float* d_result, const float* d_next);
int poisson_errors_call_check(psm_handle* h, int k, int weighting, const void* d_raw);
bool guard_take(psm_handle* h, Workspace& w);
int guard_drop(psm_handle* h, const char* where);
// A host entry's step: `enqueue` puts the step and its device -> host copies on `st`, this waits; a tripped guard drops the binding
// and the step runs once more (pass 1), on the general path.
int guarded_host_step(psm_handle* h, hipStream_t st, const char* where, const std::function<int(int pass)>& enqueue);
int frames_upload_cols(psm_handle* h, const double* cols, int n_frames, int k);   // a frame host entry's columns, through the frame binding's staging
// nan0(sdfunct) / max_abs_dist in float64 into d_sdn [npix]: the SDF channel of the deltas and the gradP image, once for the simulation
hipError_t upload_sdf_plane(psm_handle* h, const double* sdfunct, double max_abs_dist, double* d_sdn);
int unbind(psm_handle* h, const std::function<void()>& free_fn);   // the body of a psm_unbind_* entry: nothing in flight reads what free_fn releases
inline hipStream_t stream_of(const psm_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }
int bind_geometry_device(psm_handle* h, const float* d_grid, int n_cases = 1);
bool host_registered(const psm_handle* h, const void* p, size_t bytes);

template <typename Query, typename Block>
hipError_t bounded_wait(Query query, Block block) {
  if (sync_blocks()) return block();
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e;
  int n = 0;
  while ((e = query()) == hipErrorNotReady) {
    if ((++n & 63) == 0 && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > psm_switches_process().spin_us)
      return block();
  }
  return e;
}

// carve helpers: 256-byte aligned pieces of the two scratch buffers
struct Carver {
  char* base; size_t off = 0;
  template <typename T> T* take(size_t n) { T* p = reinterpret_cast<T*>(base + off); off += (n * sizeof(T) + 255) & ~(size_t)255; return p; }
};

inline size_t carve_size(std::initializer_list<size_t> bytes) { size_t t = 0; for (size_t b : bytes) t += (b + 255) & ~(size_t)255; return t; }


#define HIPCHK(h, expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail((h), PSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)


template <typename T>
int dev_alloc(psm_handle* h, T** p, size_t n) {
  if (*p) { (void)psm_dev_free(*p); *p = nullptr; }
  if (n == 0) n = 1;
  hipError_t e = psm_dev_malloc((void**)p, n * sizeof(T));
  if (e != hipSuccess) return fail(h, PSM_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return PSM_OK;
}


template <typename T>
int dev_upload(psm_handle* h, T** p, const std::vector<T>& v) {
  int rc = dev_alloc(h, p, v.size());
  if (rc) return rc;
  if (!v.empty()) HIPCHK(h, psm_copy_h2d(*p, v.data(), v.size() * sizeof(T)));
  return PSM_OK;
}


template <typename T>
void dev_free(T*& p) { if (p) { (void)psm_dev_free(p); p = nullptr; } }


// pinned host memory of a binding: n elements; a failure carries the entry's name (`where`) and the entry's code
template <typename T>
int pin_alloc(psm_handle* h, T** p, size_t n, const char* where, int code = PSM_ERR_NOMEM) {
  const hipError_t e = hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault);
  return e == hipSuccess ? PSM_OK : fail(h, code, std::string(where) + ": " + hipGetErrorString(e));
}
template <typename T>
void pin_free(T*& p) { if (p) { (void)hipHostFree(p); p = nullptr; } }


// result / change / next of a post-step call through pinned memory (result | change | next behind `pinned`): what was asked for
struct PostOut {
  float* host[3]; const float* dev[3]; float* pin[3]; size_t bytes[3];
  PostOut(const PostCall& pc, float* result, float* change, float* next, float* pinned, size_t fb, size_t pb)
      : host{result, pc.change ? change : nullptr, pc.next ? next : nullptr}, dev{pc.result, pc.change, pc.next},
        pin{pinned, pinned + fb / 4, pinned + (fb + pb) / 4}, bytes{fb, pb, pb} {}
  int enqueue(psm_handle* h, hipStream_t st) const {
    for (int q = 0; q < 3; ++q) if (host[q]) HIPCHK(h, hipMemcpyAsync(pin[q], dev[q], bytes[q], hipMemcpyDeviceToHost, st));
    return PSM_OK;
  }
  void deliver() const { for (int q = 0; q < 3; ++q) if (host[q]) memcpy(host[q], pin[q], bytes[q]); }
};


// One output of an evaluator's host entry through pinned memory, companion of PostOut: a host entry describes what it returns as a
// stack array of at most five of these (a step allocates nothing) and host_step runs the step, the copies and the delivery.
struct HostOut {
  void* host;                           // the caller's destination (null: not wanted)
  void* pin;                            // the binding's pinned staging
  const void* dev;                      // the device source
  size_t bytes;
  bool pass0_only;                      // does not depend on the route (labels, the rows' scalars): not copied again after a guard trip
};
// what the deltas / gradP host entries return, the same for the _frames and the _rows form (which adds the scalars behind them)
void deltas_host_outs(psm_handle* h, int n_frames, float* result, double* truth, double* raw, HostOut* out);             // 3 outputs
void gradp_host_outs(psm_handle* h, int n_frames, float* gradp, float* p, double* truth, double* raw, HostOut* out);     // 4 outputs

// The tail of an evaluator's host entry: `step` (the step and its error stage) and one device -> host copy per wanted output on `st`
// under guarded_host_step, then one memcpy per wanted output, in the order of `out`.
template <size_t N, typename Step>
int host_step(psm_handle* h, hipStream_t st, const char* where, const HostOut (&out)[N], const Step& step) {
  static_assert(N <= 5, "a host entry returns at most five outputs");
  const int rc = guarded_host_step(h, st, where, [&](int pass) {
    const int rs = step();
    if (rs) return rs;
    for (const HostOut& o : out)
      if (o.host && (pass == 0 || !o.pass0_only)) HIPCHK(h, hipMemcpyAsync(o.pin, o.dev, o.bytes, hipMemcpyDeviceToHost, st));
    return PSM_OK;
  });
  if (rc) return rc;
  for (const HostOut& o : out) if (o.host) memcpy(o.host, o.pin, o.bytes);
  return PSM_OK;
}


inline uint16_t f2bf(double v) {             // round-to-nearest-even float -> bf16 (NaN stays NaN)
  const float f = (float)v;
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}


// the fields PsmBoundArgs and PsmBoundBatchArgs share (two kernel-argument structs, one set of assignments)
template <typename A>
void bound_common(A& a, const psm_handle* h, const Workspace& w, const SolveRoute& r, float* d_fields) {
  a.cp = h->plan.cp; a.blocks = h->d_blocks; a.dots = w.d_dots; a.scnt = h->d_cnt; a.ownbits = h->d_ownbits;
  a.blk_y0x0 = h->d_blk; a.shiftW = h->d_shiftW;
  for (int f = 0; f < 2; ++f) a.shiftL[f] = (int)h->plan.shiftA[f].size();
  a.fields = d_fields; a.offs = w.d_offs; a.shift = w.d_shift; a.Nx = h->Nx; a.n_strips = h->n_strips; a.B = h->B;
  a.field_bytes = r.field_bytes;
  a.gflags = r.guard ? w.d_gflags : h->d_gzero; a.n_gwaves = r.guard ? r.guard_wgs : 1;   // flags the launch sums: one per guard workgroup
  a.cf = r.cf ? 1 : 0; a.cf_dots = w.d_dots2; a.cf_a0 = h->d_cfa0;
}


// ---- the launch sequence -------------------------------------------------------
// launches of a kernel group: once, or `timed_repeat` times back to back between the two timing
// events when that group is being timed (the group is idempotent; amortises the ~2.7 us an event
// pair adds to a single launch)
#define PSM_REPEAT(h, k) for (int rep_ = 0, nrep_ = (((h)->debug_skip >> (k)) & 1) ? 0 : ((h)->timed_kernel == (k) ? (h)->timed_repeat : 1); rep_ < nrep_; ++rep_)


struct Timer {                      // optional event pair around one kernel group
  psm_handle* h; hipStream_t st; int k; hipEvent_t* ev;   // ev: [PSM_K_COUNT+1] profile events or null
  void before(int kernel) {
    if (ev && kernel == 0) (void)hipEventRecord(ev[0], st);
    if (h->timed_kernel == kernel && !(kernel == PSM_K_ENCODE && !ev)) {
      hipEvent_t a, b;
      (void)hipEventCreate(&a); (void)hipEventCreate(&b);
      (void)hipEventRecord(a, st);
      h->timed_events.push_back({a, b});
    }
  }
  void after(int kernel) {
    if (ev) (void)hipEventRecord(ev[kernel + 1], st);
    if (h->timed_kernel == kernel && !(kernel == PSM_K_ENCODE && !ev)) (void)hipEventRecord(h->timed_events.back().second, st);
  }
  void skip(int kernel) { before(kernel); after(kernel); }   // a group this route does not launch: its (empty) event pair, in order
};


}  // namespace psm_impl
