// psm_api_deltas_frames.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the frame batch of the pressureSM_deltas evaluator on the
// device.  psm_bind_deltas_frames stands on psm_bind_frames; psm_deltas_image_device is the image stage alone (the mesh -> grid launch
// of psm_api_frames.cpp, then the pack: the PsmDeltasPackArgs overload of psm_to_grid_kernel, psm_pack.hip); psm_block_errors_device
// is compute_in_block_error for a batch of frames (decode again, then the PsmBlockErrorBatchArgs / PsmBlockErrorFoldArgs overloads of
// psm_block_error_kernel, psm_eval.hip); psm_deltas_frames* put planes -> image -> one solve per frame (-> filter) into one graph replay and the
// two error stages behind it, so that a metrics-only sweep returns 16 doubles per frame.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// captured step graphs (StepCall::deltas) hold the addresses of the binding's planes, SDF plane and U^2 array
static void drop_deltas_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.deltas.planes != nullptr; }); }

// columns 0-2 are stored; four scales, the SDF plane by max_abs_dist (the statements of SM_call.py:439-444 on the SDF channel)
static const EvalKind DELTAS{
    "psm_bind_deltas_frames", 3, 4, 2, 1, 2,
    "k outside [3, 16]: (dUx / U, dUy / U, dp / U^2), further columns are not stored",
    "a destination is misaligned (4 bytes for the image and the label plane, 8 for the truth plane)",
    "psm_bind_deltas_frames has not been called (psm_bind_frames, a new mesh, plan or model drop the binding)"};

void deltas_free(psm_handle* h) {
  DeltasSet& s = h->deltas;
  drop_deltas_graphs(h);
  dev_free(s.d_label); dev_free(s.d_result); dev_free(s.d_res); dev_free(s.d_part); dev_free(s.d_fraw); dev_free(s.d_u2);
  pin_free(s.h_result); pin_free(s.h_u2);
  for (auto& e : s.u2_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  s.u2_pos = 0;
  eval_free(s);
  image_gone(h);
}

// The pack launch on `st`: the binding's SDF plane, scales and U^2 array, the call's planes and destinations.
int deltas_pack_device(psm_handle* h, const DeltasCall& dc, int n_frames, hipStream_t st) {
  const DeltasSet& D = h->deltas;
  PsmDeltasPackArgs a{};
  a.planes = dc.planes; a.sdn = D.d_sdn; a.u2 = D.d_u2;
  a.grid = dc.grid; a.label = dc.label; a.truth = dc.truth;
  a.npix = (int64_t)h->Ny * h->Nx;
  a.max_abs_ux = D.max_abs[0]; a.max_abs_uy = D.max_abs[1]; a.max_abs_p = D.max_abs[3];
  a.n_frames = n_frames;
  HIPCHK(h, psm_launch_deltas_pack(a, st));
  return PSM_OK;
}

// the shared image call, then what only this kind has: the label plane (one misalignment message for the three destinations) and U^2
static int image_call(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, const float* d_grid, const float* d_label,
                      const double* d_truth, FrameCall& fc) {
  int rc = eval_image_call(h, h->deltas, DELTAS, d_cols, n_frames, k, d_grid, d_truth, fc);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_label) & 3) return fail(h, PSM_ERR_ARG, DELTAS.align_msg);
  if (d_truth && !U2) return fail(h, PSM_ERR_ARG, "the truth plane needs U2");
  for (int f = 0; U2 && f < n_frames; ++f)
    if (!std::isfinite(U2[f])) return fail(h, PSM_ERR_ARG, "U2 must be finite for every frame");
  return PSM_OK;
}

// U^2 of this step's frames: a pinned ring slot + hipMemcpyAsync in front of the launches / the replay, outside any captured graph
static int upload_u2(psm_handle* h, const double* U2, int n_frames, hipStream_t st) {
  DeltasSet& D = h->deltas;
  const int slot = D.u2_pos;
  D.u2_pos = (D.u2_pos + 1) % DeltasSet::RING;
  HIPCHK(h, hipEventSynchronize(D.u2_ev[slot]));
  double* p = D.h_u2 + (size_t)slot * D.n_frames;
  memcpy(p, U2, (size_t)n_frames * sizeof(double));
  HIPCHK(h, hipMemcpyAsync(D.d_u2, p, (size_t)n_frames * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipEventRecord(D.u2_ev[slot], st));
  return PSM_OK;
}

// what the block stage needs of the last solve
static int block_state(psm_handle* h, int n_frames) {
  if (h->last_cases < 1) return fail(h, PSM_ERR_STATE, "no solve has run yet");
  if (!h->last.on_ws0)
    return fail(h, PSM_ERR_STATE, "psm_block_errors_device follows a synchronous or device solve; the last solve ran on the ring");
  if (h->last_cases < n_frames) return fail(h, PSM_ERR_STATE, "the last solve had fewer cases than n_frames");
  return PSM_OK;
}

// The block stage on `st`: the decoded blocks of the last solve's n_frames cases into ws0.d_pred (the geometry-bound route never
// stored them), the (block, frame) launch, the fold into d_raw -- [n][8], or with d_field_raw [n][2][8] behind a copy of that row.
static int block_errors_device(psm_handle* h, const float* d_grid, const float* d_label, int n_frames, const double* d_field_raw, double* d_raw,
                               hipStream_t st) {
  const float* scale = h->last.row_scale ? h->last.row_scale : h->d_ones;
  PsmDecodeArgs de = decode_args(h, h->ws0, n_frames, scale, h->ws0.d_pred);
  if (h->last.res) de.res = h->last.res;                  // a deltas step: the rows of its frames, solved one by one
  HIPCHK(h, h->cfg.precision == PSM_PRECISION_BF16 ? psm_launch_decode_bf16(de, st) : psm_launch_decode(de, st));
  if (n_frames == h->last_cases) h->last.pred_stored = true;   // ws0 holds the decoded blocks of every case now: psm_read_stage may return them
  PsmBlockErrorBatchArgs a{};
  a.grid = d_grid; a.label = d_label; a.pred = h->ws0.d_pred; a.row_scale = scale; a.blk_y0x0 = h->d_blk; a.part = h->deltas.d_part;
  a.npix = (int64_t)h->Ny * h->Nx;
  a.S = h->S; a.c_in = h->cfg.c_in; a.sdf_ch = h->cfg.sdf_channel; a.Nx = h->Nx; a.B = h->B; a.n_frames = n_frames;
  HIPCHK(h, psm_launch_block_error_batch(a, st));
  HIPCHK(h, psm_launch_block_error_fold(PsmBlockErrorFoldArgs{h->deltas.d_part, d_field_raw, d_raw, h->B}, n_frames, st));
  return PSM_OK;
}

// The two error stages behind a step: the field's sums (the existing field-error launches, one pair) into the binding's scratch
// row, then the block stage, whose fold leaves both rows in d_raw [n][2][8].
static int deltas_step_errors_device(psm_handle* h, int n_frames, const float* d_result, const double* d_truth, double* d_raw, hipStream_t st) {
  const DeltasSet& D = h->deltas;
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  const PsmErrPlane none{nullptr, 0, 0, 0};
  PsmFieldErrorArgs a{};
  a.mask = PsmErrPlane{D.d_sdn, 0, 1, 0};                 // one plane for every frame
  a.pair[0] = PsmFieldErrorPair{PsmErrPlane{d_result, npix, 1, 1}, PsmErrPlane{d_truth, npix, 1, 0}, none, none, 0};
  a.n_pairs = 1; a.n_frames = n_frames;
  int rc = field_errors_device(h, a, D.d_fraw, st);
  if (rc) return rc;
  return block_errors_device(h, D.d_grid, D.d_label, n_frames, D.d_fraw, d_raw, st);
}

// every check of one step; nothing is enqueued before they pass
static int deltas_step_check(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, int apply_filter, const float* d_result,
                             const double* d_truth, const double* d_raw, const RowsCall* rows, FrameCall& fc) {
  const DeltasSet& D = h->deltas;
  int rc = image_call(h, d_cols, n_frames, k, U2, D.d_grid, D.d_label, rows ? nullptr : d_truth, fc);   // rows: U^2 is made on the device
  if (rc) return rc;
  if (rows && (reinterpret_cast<uintptr_t>(d_truth) & 7)) return fail(h, PSM_ERR_ARG, "a destination is misaligned (8 bytes for the truth plane)");
  if (!rows && !U2) return fail(h, PSM_ERR_ARG, "null argument");
  if (apply_filter && !h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: apply_filter needs it as well as psm_bind_deltas_frames");
  if ((reinterpret_cast<uintptr_t>(d_result) & 3) || (reinterpret_cast<uintptr_t>(d_raw) & 7))
    return fail(h, PSM_ERR_ARG, "a destination is misaligned (4 bytes for d_result, 8 for d_raw)");
  return PSM_OK;
}

int deltas_host_check(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, int apply_filter, const RowsCall* rows) {
  const DeltasSet& D = h->deltas;
  FrameCall fc;
  return deltas_step_check(h, d_cols, n_frames, k, U2, apply_filter, D.d_result, D.d_truth, D.d_raw, rows, fc);
}

// null destinations become the binding's; the checks; the step's scalars and the one graph replay: frames -> planes -> image (label,
// truth) -> solve (-> filter); the two error stages when d_raw is given
int deltas_frames_step(psm_handle* h, const double* d_cols, int n_frames, int k, const double* U2, const float* out_scale, int apply_filter,
                       float* d_result, double* d_truth, double* d_raw, hipStream_t st, const RowsCall* rows) {
  DeltasSet& D = h->deltas;
  if (!d_result) d_result = D.d_result;
  if (!d_truth) d_truth = D.d_truth;
  StepCall step;
  int rc = deltas_step_check(h, d_cols, n_frames, k, U2, apply_filter, d_result, d_truth, d_raw, rows, step.frames);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (rows) step.rows = *rows;
  else if ((rc = upload_u2(h, U2, n_frames, st))) return rc;
  step.deltas = DeltasCall{D.d_planes, D.d_grid, D.d_label, d_truth, D.d_res};
  if (apply_filter) { step.post.apply_filter = 1; step.post.result = d_result; }
  rc = solve_device(h, D.d_grid, n_frames, out_scale, apply_filter ? h->post.d_fields : d_result, st, nullptr, step);
  if (rc || !d_raw) return rc;
  return deltas_step_errors_device(h, n_frames, d_result, d_truth, d_raw, st);
}

void deltas_host_outs(psm_handle* h, int n_frames, float* result, double* truth, double* raw, HostOut* out) {
  const DeltasSet& D = h->deltas;
  const size_t fb = (size_t)n_frames * h->Ny * h->Nx * sizeof(float);
  out[0] = HostOut{result, D.h_result, D.d_result, fb, false};
  out[1] = HostOut{truth, D.h_truth, D.d_truth, 2 * fb, true};            // the labels do not depend on the route
  out[2] = HostOut{raw, D.h_raw, D.d_raw, (size_t)n_frames * 2 * PSM_ERR_RAW * sizeof(double), false};
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_deltas_frames(psm_handle* h, const double* sdfunct, const double* max_abs) {
  if (!h) return PSM_ERR_ARG;
  int rc = frames_state(h);
  if (rc) return rc;
  if (h->cfg.c_in != 3 || h->cfg.sdf_channel != 2 || h->cfg.c_out != 1)
    return fail(h, PSM_ERR_STATE, "the deltas frames are a three-channel image with the SDF last and a one-channel field: c_in == 3, sdf_channel == 2, c_out == 1");
  DeltasSet& s = h->deltas;
  return eval_bind(h, s, DELTAS, sdfunct, max_abs, deltas_free, [&](size_t n, size_t npix) {
    const size_t n_res = (size_t)round_up((int)n * h->B, 32) * h->ld_out;
    int ro;
    if ((ro = dev_alloc(h, &s.d_label, n * npix)) || (ro = dev_alloc(h, &s.d_result, n * npix)) || (ro = dev_alloc(h, &s.d_res, n_res)) ||
        (ro = dev_alloc(h, &s.d_part, n * h->B * PSM_ERR_RAW)) || (ro = dev_alloc(h, &s.d_fraw, n * PSM_ERR_RAW)) || (ro = dev_alloc(h, &s.d_u2, n)) ||
        (ro = pin_alloc(h, &s.h_result, n * npix, DELTAS.bind_name)) || (ro = pin_alloc(h, &s.h_u2, DeltasSet::RING * n, DELTAS.bind_name))) return ro;
    hipError_t e = hipSuccess;
    for (auto& ev : s.u2_ev) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemset(s.d_res, 0, n_res * sizeof(float));   // the rows the decode pads to
    const std::vector<double> ones(n, 1.0);
    if (e == hipSuccess) e = psm_copy_h2d(s.d_u2, ones.data(), n * sizeof(double));
    return e == hipSuccess ? PSM_OK : fail(h, PSM_ERR_NOMEM, std::string(DELTAS.bind_name) + ": " + hipGetErrorString(e));
  });
}


int psm_unbind_deltas_frames(psm_handle* h) {
  return unbind(h, [h] { deltas_free(h); });
}


int psm_deltas_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* U2, float* d_grid,
                            float* d_label, double* d_truth, void* stream) {
  if (!h) return PSM_ERR_ARG;
  FrameCall fc;
  int rc = image_call(h, d_cols, n_frames, k, U2, d_grid, d_label, d_truth, fc);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = stream_of(h, stream);
  if (U2 && (rc = upload_u2(h, U2, n_frames, st))) return rc;
  if ((rc = frames_device(h, fc, n_frames, st))) return rc;
  return deltas_pack_device(h, DeltasCall{h->deltas.d_planes, d_grid, d_label, d_truth, nullptr}, n_frames, st);
}


int psm_block_errors_device(psm_handle* h, const float* d_grid, const float* d_label, int32_t n_frames, double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  int rc = eval_state(h, h->deltas, DELTAS);
  if (rc) return rc;
  if ((rc = frames_count_check(h, n_frames))) return rc;
  if (!d_grid || !d_label || !d_raw) return fail(h, PSM_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_grid) & 3) || (reinterpret_cast<uintptr_t>(d_label) & 3)) return fail(h, PSM_ERR_ARG, "the image and the label plane must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_raw) & 7) return fail(h, PSM_ERR_ARG, "d_raw must be 8-byte aligned");
  if ((rc = block_state(h, n_frames))) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return block_errors_device(h, d_grid, d_label, n_frames, nullptr, d_raw, stream_of(h, stream));
}


int psm_deltas_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* U2, const float* out_scale,
                             int32_t apply_filter, float* d_result, double* d_truth, double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  return deltas_frames_step(h, d_cols, n_frames, k, U2, out_scale, apply_filter, d_result, d_truth, d_raw, stream_of(h, stream));
}


int psm_deltas_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* U2, const float* out_scale,
                      int32_t apply_filter, float* result, double* truth, double* raw) {
  if (!h) return PSM_ERR_ARG;
  if (!cols || !(result || truth || raw)) return fail(h, PSM_ERR_ARG, "null buffer");
  const double* d_cols = h->frames.d_cols;
  hipStream_t st = h->stream;
  // every check of the step before the first copy: the step itself repeats them
  int rc = deltas_host_check(h, d_cols, n_frames, k, U2, apply_filter);
  if (rc || (rc = frames_upload_cols(h, cols, n_frames, k))) return rc;
  HostOut out[3];
  deltas_host_outs(h, n_frames, result, truth, raw, out);
  return host_step(h, st, "psm_deltas_frames", out, [&] {
    return deltas_frames_step(h, d_cols, n_frames, k, U2, out_scale, apply_filter, nullptr, nullptr, raw ? h->deltas.d_raw : nullptr, st);
  });
}

}  // extern "C"
