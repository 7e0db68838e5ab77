// psm_api_frames.cpp -- C-ABI of libpsm_hip.so (include/psm.h): frames of cell columns on the single mesh of psm_set_geometry, on the
// device.  psm_frames_to_grid_device is the mesh -> grid stage alone (interpolate_fill + last-writer scatter of k columns per frame,
// every column into a plane of its own, one launch for the batch); psm_poisson_frames* put it in front of the Poisson time step of
// psm_api_features.cpp, column convention of the pressureSM_Poisson evaluator, as one graph replay:
// d_cols -> planes -> features -> solve -> post-steps.  Kernel: the PsmFrameArgs overload of psm_interp_to_grid_kernel (psm_mesh.hip).
// See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// captured step graphs (StepCall::frames) hold the addresses of the mesh tables and of the column array
static void drop_frame_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.frames.cols != nullptr; }); }

void frames_free(psm_handle* h) {
  FrameSet& s = h->frames;
  deltas_free(h);                       // psm_bind_deltas_frames stands on this binding,
  gradp_free(h);                        // psm_bind_gradp_frames,
  chapter4_free(h);                     // psm_bind_chapter4_frames
  rows_free(h);                         // psm_bind_rows
  poisson_solve_free(h);                // and psm_bind_poisson_solve
  drop_frame_graphs(h);
  dev_free(s.d_cols); dev_free(s.d_extra); dev_free(s.d_raw);
  pin_free(s.h_cols); pin_free(s.h_extra); pin_free(s.h_out); pin_free(s.h_raw);
  s.ready = false; s.n_frames = 0; s.k = 0;
}

// The one launch of the stage on `st`: the mesh's tables, the call's columns and plane descriptors.
int frames_device(psm_handle* h, const FrameCall& fc, int n_frames, hipStream_t st) {
  PsmFrameArgs a{};
  a.cols = fc.cols; a.vtx = h->mesh.t.vtx_m2g; a.wts = h->mesh.t.wts_m2g; a.src_of_cell = h->mesh.t.src_of_cell;
  a.n_grid = (int64_t)h->Ny * h->Nx; a.n_cells = h->n_cells;
  a.k = fc.k; a.fill = fc.fill ? 1 : 0; a.n_frames = n_frames;
  for (int c = 0; c < fc.k; ++c) a.out[c] = fc.out[c];
  HIPCHK(h, psm_launch_frames_to_grid(a, st));
  return PSM_OK;
}

// the mesh and the binding every entry below needs
int frames_state(psm_handle* h) {
  if (h->mcs.ready) return fail(h, PSM_ERR_STATE, "the handle holds a case set (psm_set_geometry_cases): frames take the single mesh of psm_set_geometry");
  if (!h->have_geometry || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (a new plan drops the mesh)");
  if (!h->frames.ready) return fail(h, PSM_ERR_STATE, "psm_bind_frames has not been called (a new mesh, plan or model drops the binding)");
  return PSM_OK;
}

int frames_count_check(psm_handle* h, int n_frames) {
  if (n_frames < 1 || n_frames > h->frames.n_frames) return fail(h, PSM_ERR_ARG, "n_frames outside [1, frames bound with psm_bind_frames]");
  return PSM_OK;
}

int frames_upload_cols(psm_handle* h, const double* cols, int n_frames, int k) {
  FrameSet& F = h->frames;
  if (k > F.k) return fail(h, PSM_ERR_ARG, "more columns than psm_bind_frames reserved staging for");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const size_t cb = (size_t)n_frames * h->n_cells * k * sizeof(double);
  memcpy(F.h_cols, cols, cb);
  HIPCHK(h, hipMemcpyAsync(F.d_cols, F.h_cols, cb, hipMemcpyHostToDevice, h->stream));
  return PSM_OK;
}

hipError_t upload_sdf_plane(psm_handle* h, const double* sdfunct, double max_abs_dist, double* d_sdn) {
  const size_t npix = (size_t)h->Ny * h->Nx;
  std::vector<double> sdn(npix);
  for (size_t i = 0; i < npix; ++i) sdn[i] = (sdfunct[i] != sdfunct[i] ? 0.0 : sdfunct[i]) / max_abs_dist;
  return psm_copy_h2d(d_sdn, sdn.data(), npix * sizeof(double));
}

// ---- what the three evaluator frame bindings share (EvalSet, EvalKind: psm_handle.h) ----
void eval_free(EvalSet& s) {
  dev_free(s.d_sdn); dev_free(s.d_planes); dev_free(s.d_grid); dev_free(s.d_truth); dev_free(s.d_raw);
  pin_free(s.h_raw); pin_free(s.h_truth);
  s.ready = false; s.n_frames = 0;
}

int eval_state(psm_handle* h, const EvalSet& s, const EvalKind& kind) {
  int rc = frames_state(h);
  if (rc) return rc;
  if (!s.ready) return fail(h, PSM_ERR_STATE, kind.unbound_msg);
  return PSM_OK;
}

int eval_image_call(psm_handle* h, const EvalSet& s, const EvalKind& kind, const double* d_cols, int n_frames, int k, const float* d_grid,
                    const double* d_truth, FrameCall& fc) {
  int rc = eval_state(h, s, kind);
  if (rc) return rc;
  const int cols = kind.n_cols(h->cfg);
  if (k < cols || k > PSM_FRAME_MAX_COLS) return fail(h, PSM_ERR_ARG, kind.k_msg);
  if ((rc = frames_count_check(h, n_frames))) return rc;
  if (!d_cols || !d_grid) return fail(h, PSM_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_grid) & 3) || (reinterpret_cast<uintptr_t>(d_truth) & 7)) return fail(h, PSM_ERR_ARG, kind.align_msg);
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  fc = FrameCall{};
  fc.cols = d_cols; fc.k = k; fc.fill = 1;
  for (int c = 0; c < cols; ++c) fc.out[c] = PsmFramePlane{s.d_planes + c * npix, cols * npix, 0};
  return PSM_OK;
}

int eval_bind(psm_handle* h, EvalSet& s, const EvalKind& kind, const double* sdfunct, const double* max_abs, void (*free_fn)(psm_handle*),
              const std::function<int(size_t n, size_t npix)>& own) {
  if (!sdfunct || !max_abs) return fail(h, PSM_ERR_ARG, "null argument");
  const int scales = kind.n_scales(h->cfg);
  for (int q = 0; q < scales; ++q)
    if (!(max_abs[q] != 0.0) || !std::isfinite(max_abs[q])) return fail(h, PSM_ERR_ARG, "max_abs scales must be finite and non-zero");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // a step in flight reads the buffers that are replaced
  free_fn(h);
  const size_t npix = (size_t)h->Ny * h->Nx, n = (size_t)h->frames.n_frames;
  const size_t n_truth = n * kind.truth_planes * npix, n_raw = n * kind.raw_rows * PSM_ERR_RAW;
  int rc = own(n, npix);
  if (!rc && !(rc = dev_alloc(h, &s.d_sdn, npix)) && !(rc = dev_alloc(h, &s.d_planes, n * kind.n_cols(h->cfg) * npix)) &&
      !(rc = dev_alloc(h, &s.d_grid, n * npix * h->cfg.c_in)) && !(rc = dev_alloc(h, &s.d_truth, n_truth)) && !(rc = dev_alloc(h, &s.d_raw, n_raw)) &&
      !(rc = pin_alloc(h, &s.h_raw, n_raw, kind.bind_name)) && !(rc = pin_alloc(h, &s.h_truth, n_truth, kind.bind_name))) {
    const hipError_t e = upload_sdf_plane(h, sdfunct, max_abs[kind.dist_at(h->cfg)], s.d_sdn);   // the reference's statements on the SDF channel
    if (e != hipSuccess) rc = fail(h, PSM_ERR_NOMEM, std::string(kind.bind_name) + ": " + hipGetErrorString(e));
  }
  if (rc) { free_fn(h); return rc; }
  s.n_frames = h->frames.n_frames;
  for (int q = 0; q < scales; ++q) s.max_abs[q] = max_abs[q];
  s.ready = true;
  return PSM_OK;
}

// The evaluator's column convention as plane descriptors: 0-3 -> the feature binding's velocity planes, the last two (weighting) ->
// the post-steps' dU / prev as float32, the columns between -> d_extra (nullptr: not stored).
int poisson_frame_call(psm_handle* h, const double* d_cols, int n_frames, int k, int weighting, double* d_extra, FrameCall& fc) {
  int rc = frames_state(h);
  if (rc) return rc;
  if (!h->feat.ready) return fail(h, PSM_ERR_STATE, "psm_bind_features has not been called: the frames step needs it as well as psm_bind_frames");
  if (!h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: the frames step needs it as well as psm_bind_frames");
  const int k_min = weighting ? 6 : 4;
  if (k < k_min || k > PSM_FRAME_MAX_COLS) return fail(h, PSM_ERR_ARG, "k outside [4 (6 with the weighting), 16]: (Ux, Uy, dUx, dUy), extra columns, (dU-change weight, delta_p_prev)");
  if ((rc = frames_count_check(h, n_frames))) return rc;
  if (!d_cols) return fail(h, PSM_ERR_ARG, "null buffer");
  if (reinterpret_cast<uintptr_t>(d_extra) & 7) return fail(h, PSM_ERR_ARG, "d_extra must be 8-byte aligned");
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  const int n_extra = k - k_min;
  fc = FrameCall{};
  fc.cols = d_cols; fc.k = k; fc.fill = 1;
  for (int c = 0; c < 4; ++c) fc.out[c] = PsmFramePlane{h->feat.d_vel + c * npix, 4 * npix, 0};
  for (int e = 0; e < n_extra; ++e) fc.out[4 + e] = PsmFramePlane{d_extra ? d_extra + e * npix : nullptr, n_extra * npix, 0};
  if (weighting) {
    fc.out[k - 2] = PsmFramePlane{h->post.d_dU, npix, 1};
    fc.out[k - 1] = PsmFramePlane{h->post.d_prev, npix, 1};
  }
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_frames(psm_handle* h, int32_t n_frames, int32_t k) {
  if (!h) return PSM_ERR_ARG;
  if (h->mcs.ready) return fail(h, PSM_ERR_STATE, "the handle holds a case set (psm_set_geometry_cases): frames take the single mesh of psm_set_geometry");
  if (!h->have_geometry || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (a new plan drops the mesh)");
  if (n_frames < 1 || n_frames > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_frames outside [1, max_cases]");
  if (k < 1 || k > PSM_FRAME_MAX_COLS) return fail(h, PSM_ERR_ARG, "1..16 columns");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // a step in flight reads the staging that is replaced
  frames_free(h);
  FrameSet& s = h->frames;
  const size_t npix = (size_t)h->Ny * h->Nx, n = (size_t)n_frames;
  const size_t n_cols = n * (size_t)h->n_cells * k, n_extra = n * (size_t)k * npix, n_out = n * npix * ((size_t)h->cfg.c_out + 2);
  int rc;
  const size_t n_raw = n * 3 * PSM_ERR_RAW;             // psm_poisson_frames_errors: the three error blocks of every frame
  if ((rc = dev_alloc(h, &s.d_cols, n_cols)) || (rc = dev_alloc(h, &s.d_extra, n_extra)) || (rc = dev_alloc(h, &s.d_raw, n_raw))) { frames_free(h); return rc; }
  if ((rc = pin_alloc(h, &s.h_cols, n_cols, "psm_bind_frames")) || (rc = pin_alloc(h, &s.h_extra, n_extra, "psm_bind_frames")) ||
      (rc = pin_alloc(h, &s.h_out, n_out, "psm_bind_frames")) || (rc = pin_alloc(h, &s.h_raw, n_raw, "psm_bind_frames"))) { frames_free(h); return rc; }
  s.n_frames = n_frames; s.k = k;
  s.ready = true;
  return PSM_OK;
}


int psm_unbind_frames(psm_handle* h) {
  return unbind(h, [h] { frames_free(h); });
}


int psm_frames_to_grid_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, int32_t fill, const psm_frame_col* out,
                              void* stream) {
  if (!h) return PSM_ERR_ARG;
  int rc = frames_state(h);
  if (rc) return rc;
  if (k < 1 || k > PSM_FRAME_MAX_COLS) return fail(h, PSM_ERR_ARG, "1..16 columns");
  if ((rc = frames_count_check(h, n_frames))) return rc;
  if (!d_cols || !out) return fail(h, PSM_ERR_ARG, "null argument");
  FrameCall fc;
  fc.cols = d_cols; fc.k = k; fc.fill = fill ? 1 : 0;
  bool any = false;
  for (int c = 0; c < k; ++c) {
    if (!out[c].dst) continue;
    any = true;
    if (reinterpret_cast<uintptr_t>(out[c].dst) & (out[c].as_f32 ? 3 : 7))
      return fail(h, PSM_ERR_ARG, "a destination plane is misaligned (8 bytes for float64, 4 for float32)");
    if (out[c].frame_stride < 0) return fail(h, PSM_ERR_ARG, "frame_stride must not be negative");
    fc.out[c] = PsmFramePlane{out[c].dst, out[c].frame_stride, out[c].as_f32 ? 1 : 0};
  }
  if (!any) return fail(h, PSM_ERR_ARG, "every destination is NULL: nothing to store");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return frames_device(h, fc, n_frames, stream_of(h, stream));
}


int psm_poisson_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* LU, const float* out_scale,
                              int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change, float* d_next,
                              void* stream) {
  if (!h) return PSM_ERR_ARG;
  FrameCall fc;
  int rc = poisson_frame_call(h, d_cols, n_frames, k, weighting, d_extra, fc);
  if (rc) return rc;
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.result = d_result;
  if (weighting) { pc.dU = h->post.d_dU; pc.prev = h->post.d_prev; pc.change = d_change; pc.next = d_next; }
  return poisson_step_device(h, h->feat.d_vel, n_frames, LU, out_scale, pc, (hipStream_t)stream, &fc);
}


int psm_poisson_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* LU, const float* out_scale,
                       int32_t apply_filter, int32_t weighting, double* extra, float* result, float* change, float* next) {
  if (!h) return PSM_ERR_ARG;
  if (!cols || !result) return fail(h, PSM_ERR_ARG, "null buffer");
  FrameSet& F = h->frames;
  FrameCall fc;
  int rc = poisson_frame_call(h, F.d_cols, n_frames, k, weighting, extra ? F.d_extra : nullptr, fc);
  if (rc) return rc;
  PostSet& s = h->post;
  const size_t cap = (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out;
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.result = s.d_out;
  if (weighting) { pc.dU = s.d_dU; pc.prev = s.d_prev; pc.change = change ? s.d_out + cap : nullptr; pc.next = next ? s.d_out + 2 * cap : nullptr; }
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx, n_extra = (size_t)k - (weighting ? 6 : 4);
  const size_t pb = (size_t)n_frames * npix * sizeof(float), fb = pb * h->cfg.c_out;
  const size_t eb = extra ? (size_t)n_frames * n_extra * npix * sizeof(double) : 0;
  const PostOut out(pc, result, change, next, F.h_out, fb, pb);
  if ((rc = frames_upload_cols(h, cols, n_frames, k))) return rc;
  rc = guarded_host_step(h, st, "psm_poisson_frames", [&](int pass) {
    int rs = poisson_step_device(h, h->feat.d_vel, n_frames, LU, out_scale, pc, st, &fc);
    if (rs || (rs = out.enqueue(h, st))) return rs;
    if (eb && pass == 0) HIPCHK(h, hipMemcpyAsync(F.h_extra, F.d_extra, eb, hipMemcpyDeviceToHost, st));   // the planes do not depend on the route
    return PSM_OK;
  });
  if (rc) return rc;
  out.deliver();
  if (eb) memcpy(extra, F.h_extra, eb);
  return PSM_OK;
}

}  // extern "C"
