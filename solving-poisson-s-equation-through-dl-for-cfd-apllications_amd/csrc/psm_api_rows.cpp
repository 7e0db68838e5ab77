// psm_api_rows.cpp -- C-ABI of libpsm_hip.so (include/psm.h): a frame's dataset rows as stored (float32, row-major) -> the per-frame
// scalars and the float64 columns of the evaluators' frame steps, on the device.  psm_bind_rows stands on psm_bind_frames;
// psm_rows_prepare_device is the stage alone (two plain launches, psm_rows.hip); psm_deltas_rows*, psm_poisson_rows*(_errors) and
// psm_gradp_rows* put the two launches at the head of the one graph replay of their _frames counterparts (StepCall::rows), whose
// kernels then read U^2, (L, U) and the row scale from the device arrays the finish launch wrote: nothing is uploaded in front of
// a step but the rows.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

static_assert(PSM_ROWS_DELTAS == PSM_ROWS_KIND_DELTAS && PSM_ROWS_POISSON == PSM_ROWS_KIND_POISSON && PSM_ROWS_GRADP == PSM_ROWS_KIND_GRADP,
              "psm.h and psm_rows.h disagree on the kinds");

// captured step graphs (StepCall::rows) hold the addresses of the binding's partials and scalar slots
static void drop_rows_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.rows.rows != nullptr; }); }

void rows_free(psm_handle* h) {
  RowsSet& s = h->rows;
  drop_rows_graphs(h);
  dev_free(s.d_rows); dev_free(s.d_part); dev_free(s.d_scalars);
  pin_free(s.h_rows); pin_free(s.h_scalars);
  s.ready = false; s.n_frames = 0; s.width = 0;
}

// The two launches of the stage on `st`.  A step (wired): the finish launch also writes what the step's kernels read.
int rows_device(psm_handle* h, const RowsCall& rc, int n_frames, hipStream_t st) {
  PsmRowsArgs a{};
  a.rows = rc.rows; a.part = h->rows.d_part; a.cols = rc.cols; a.scalars = rc.scalars;
  a.n_cells = rc.n_cells; a.width = rc.width; a.kind = rc.kind; a.n_frames = n_frames; a.n_parts = psm_rows_parts(rc.n_cells);
  a.base = rc.base; a.phi = rc.phi; a.ex = (float)rc.ex; a.ey = (float)rc.ey;
  a.B = h->B;
  if (rc.wired) {
    if (rc.scaled()) a.row_scale = h->ws0.d_row_scale;
    if (rc.kind == PSM_ROWS_KIND_DELTAS) a.u2 = h->deltas.d_u2;
    if (rc.kind == PSM_ROWS_KIND_POISSON) a.lu = h->feat.d_lu;
  }
  HIPCHK(h, psm_launch_rows_partial(a, st));
  HIPCHK(h, psm_launch_rows_finish(a, st));
  return PSM_OK;
}

// the mesh, the frame binding and this binding
static int rows_state(psm_handle* h) {
  int rc = frames_state(h);
  if (rc) return rc;
  if (!h->rows.ready) return fail(h, PSM_ERR_STATE, "psm_bind_rows has not been called (psm_bind_frames, a new mesh, plan or model drop the binding)");
  return PSM_OK;
}

// Every check of the stage; nothing is enqueued before they pass.  d_cols == nullptr: the frame binding's column buffer.
static int rows_call(psm_handle* h, int kind, const float* d_rows, int n_frames, int64_t n_cells, int width, double base, double phi, double ex,
                     double ey, double* d_cols, double* d_scalars, bool wired, RowsCall& rc) {
  int r = rows_state(h);
  if (r) return r;
  const int k = psm_rows_cols(kind);
  if (!k) return fail(h, PSM_ERR_ARG, "unknown kind: PSM_ROWS_DELTAS, PSM_ROWS_POISSON or PSM_ROWS_GRADP");
  if (width < 8 || width > 16 || width < psm_rows_min_width(kind))
    return fail(h, PSM_ERR_ARG, "width outside [8, 16] (the deltas and the Poisson recipe read column 10: at least 11)");
  if ((r = frames_count_check(h, n_frames))) return r;
  if (n_cells < 1 || n_cells > h->n_cells) return fail(h, PSM_ERR_ARG, "n_cells outside [1, cells of the mesh]");
  if (!d_rows) return fail(h, PSM_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_rows) & 3) || (reinterpret_cast<uintptr_t>(d_cols) & 7) || (reinterpret_cast<uintptr_t>(d_scalars) & 7))
    return fail(h, PSM_ERR_ARG, "a pointer is misaligned (4 bytes for the rows, 8 for the columns and the scalars)");
  if (kind != PSM_ROWS_KIND_GRADP && (!(base != 0.0) || !std::isfinite(base))) return fail(h, PSM_ERR_ARG, "base must be finite and non-zero");
  if (!std::isfinite(phi) || !std::isfinite(ex) || !std::isfinite(ey)) return fail(h, PSM_ERR_ARG, "phi, ex and ey must be finite");
  if (!d_cols) {
    if (k > h->frames.k) return fail(h, PSM_ERR_ARG, "psm_bind_frames reserved fewer columns than this kind writes");
    d_cols = h->frames.d_cols;
  }
  rc = RowsCall{};
  rc.rows = d_rows; rc.kind = kind; rc.width = width; rc.cols = d_cols; rc.scalars = d_scalars ? d_scalars : h->rows.d_scalars;
  rc.n_cells = n_cells; rc.base = base; rc.phi = phi; rc.ex = ex; rc.ey = ey; rc.wired = wired;
  return PSM_OK;
}

// a step's rows call: the whole mesh, the frame binding's columns
static int step_rows_call(psm_handle* h, int kind, const float* d_rows, int n_frames, int width, double base, double phi, double ex, double ey,
                          double* d_scalars, RowsCall& rc) {
  return rows_call(h, kind, d_rows, n_frames, h->n_cells, width, base, phi, ex, ey, nullptr, d_scalars, true, rc);
}

// a host entry's rows through the binding's staging (after every check of the step)
static int upload_rows(psm_handle* h, const float* rows, int n_frames, int width) {
  RowsSet& R = h->rows;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const size_t rb = (size_t)n_frames * h->n_cells * width * sizeof(float);
  memcpy(R.h_rows, rows, rb);
  HIPCHK(h, hipMemcpyAsync(R.d_rows, R.h_rows, rb, hipMemcpyHostToDevice, h->stream));
  return PSM_OK;
}

static int host_width_check(psm_handle* h, int width) {
  if (h->rows.ready && width > h->rows.width) return fail(h, PSM_ERR_ARG, "wider rows than psm_bind_rows reserved staging for");
  return PSM_OK;
}

// the scalars behind an evaluator's outputs: made by the rows stage, the same on every route
static HostOut scalars_out(psm_handle* h, int n_frames, double* scalars) {
  return HostOut{scalars, h->rows.h_scalars, h->rows.d_scalars, (size_t)n_frames * PSM_ROWS_SCALARS * sizeof(double), true};
}

// the Poisson step's post-step descriptor on caller pointers
static PostCall poisson_post(psm_handle* h, int apply_filter, int weighting, float* d_result, float* d_change, float* d_next) {
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.result = d_result;
  if (weighting) { pc.dU = h->post.d_dU; pc.prev = h->post.d_prev; pc.change = d_change; pc.next = d_next; }
  return pc;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_rows(psm_handle* h, int32_t width) {
  if (!h) return PSM_ERR_ARG;
  int rc = frames_state(h);
  if (rc) return rc;
  if (width < 8 || width > 16) return fail(h, PSM_ERR_ARG, "width outside [8, 16]");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // a step in flight reads the staging that is replaced
  rows_free(h);
  RowsSet& s = h->rows;
  const size_t n = (size_t)h->frames.n_frames, n_rows = n * (size_t)h->n_cells * width;
  if ((rc = dev_alloc(h, &s.d_rows, n_rows)) || (rc = dev_alloc(h, &s.d_part, n * 3 * PSM_ROWS_PARTS)) ||
      (rc = dev_alloc(h, &s.d_scalars, n * PSM_ROWS_SCALARS))) { rows_free(h); return rc; }
  if ((rc = pin_alloc(h, &s.h_rows, n_rows, "psm_bind_rows")) || (rc = pin_alloc(h, &s.h_scalars, n * PSM_ROWS_SCALARS, "psm_bind_rows"))) { rows_free(h); return rc; }
  s.n_frames = h->frames.n_frames; s.width = width;
  s.ready = true;
  return PSM_OK;
}


int psm_unbind_rows(psm_handle* h) {
  return unbind(h, [h] { rows_free(h); });
}


int psm_rows_prepare_device(psm_handle* h, int32_t kind, const float* d_rows, int32_t n_frames, int64_t n_cells, int32_t width,
                            const double* params, double* d_cols, double* d_scalars, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!params) return fail(h, PSM_ERR_ARG, "null argument");
  RowsCall rc;
  int r = rows_call(h, kind, d_rows, n_frames, n_cells, width, params[0], params[1], params[2], params[3], d_cols, d_scalars, false, rc);
  if (r) return r;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return rows_device(h, rc, n_frames, stream_of(h, stream));
}


int psm_deltas_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, int32_t apply_filter,
                           float* d_result, double* d_truth, double* d_raw, double* d_scalars, void* stream) {
  if (!h) return PSM_ERR_ARG;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_DELTAS, d_rows, n_frames, width, base, 1.0, 1.0, 1.0, d_scalars, rc);
  if (r) return r;
  return deltas_frames_step(h, rc.cols, n_frames, 3, nullptr, nullptr, apply_filter, d_result, d_truth, d_raw, stream_of(h, stream), &rc);
}


int psm_deltas_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, int32_t apply_filter, float* result,
                    double* truth, double* raw, double* scalars) {
  if (!h) return PSM_ERR_ARG;
  if (!rows || !(result || truth || raw || scalars)) return fail(h, PSM_ERR_ARG, "null buffer");
  RowsSet& R = h->rows;
  hipStream_t st = h->stream;
  // every check of the step before the first copy: the step itself repeats them
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_DELTAS, R.d_rows, n_frames, width, base, 1.0, 1.0, 1.0, R.d_scalars, rc);
  if (r || (r = host_width_check(h, width)) || (r = deltas_host_check(h, rc.cols, n_frames, 3, nullptr, apply_filter, &rc))) return r;
  if ((r = upload_rows(h, rows, n_frames, width))) return r;
  HostOut out[4];
  deltas_host_outs(h, n_frames, result, truth, raw, out);
  out[3] = scalars_out(h, n_frames, scalars);
  return host_step(h, st, "psm_deltas_rows", out, [&] {
    return deltas_frames_step(h, rc.cols, n_frames, 3, nullptr, nullptr, apply_filter, nullptr, nullptr, raw ? h->deltas.d_raw : nullptr, st, &rc);
  });
}


int psm_poisson_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, double phi,
                            int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change, float* d_next,
                            double* d_scalars, void* stream) {
  if (!h) return PSM_ERR_ARG;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_POISSON, d_rows, n_frames, width, base, phi, 1.0, 1.0, d_scalars, rc);
  if (r) return r;
  FrameCall fc;
  if ((r = poisson_frame_call(h, rc.cols, n_frames, 8, weighting, d_extra, fc))) return r;
  const PostCall pc = poisson_post(h, apply_filter, weighting, d_result, d_change, d_next);
  return poisson_step_device(h, h->feat.d_vel, n_frames, nullptr, nullptr, pc, (hipStream_t)stream, &fc, &rc);
}


int psm_poisson_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, double phi, int32_t apply_filter,
                     int32_t weighting, double* extra, float* result, float* change, float* next, double* scalars) {
  if (!h) return PSM_ERR_ARG;
  if (!rows || !result) return fail(h, PSM_ERR_ARG, "null buffer");
  FrameSet& F = h->frames;
  RowsSet& R = h->rows;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_POISSON, R.d_rows, n_frames, width, base, phi, 1.0, 1.0, R.d_scalars, rc);
  if (r || (r = host_width_check(h, width))) return r;
  FrameCall fc;
  if ((r = poisson_frame_call(h, rc.cols, n_frames, 8, weighting, extra ? F.d_extra : nullptr, fc))) return r;
  PostSet& s = h->post;
  const size_t cap = (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out;
  const PostCall pc = poisson_post(h, apply_filter, weighting, s.d_out, change ? s.d_out + cap : nullptr, next ? s.d_out + 2 * cap : nullptr);
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx, n_extra = weighting ? 2 : 4;
  const size_t pb = (size_t)n_frames * npix * sizeof(float), fb = pb * h->cfg.c_out;
  const size_t eb = extra ? (size_t)n_frames * n_extra * npix * sizeof(double) : 0, sb = (size_t)n_frames * PSM_ROWS_SCALARS * sizeof(double);
  const PostOut out(pc, result, change, next, F.h_out, fb, pb);
  if ((r = upload_rows(h, rows, n_frames, width))) return r;
  r = guarded_host_step(h, st, "psm_poisson_rows", [&](int pass) {
    int rs = poisson_step_device(h, h->feat.d_vel, n_frames, nullptr, nullptr, pc, st, &fc, &rc);
    if (rs || (rs = out.enqueue(h, st))) return rs;
    if (eb && pass == 0) HIPCHK(h, hipMemcpyAsync(F.h_extra, F.d_extra, eb, hipMemcpyDeviceToHost, st));   // the planes do not depend on the route
    if (scalars && pass == 0) HIPCHK(h, hipMemcpyAsync(R.h_scalars, R.d_scalars, sb, hipMemcpyDeviceToHost, st));
    return PSM_OK;
  });
  if (r) return r;
  out.deliver();
  if (eb) memcpy(extra, F.h_extra, eb);
  if (scalars) memcpy(scalars, R.h_scalars, sb);
  return PSM_OK;
}


int psm_poisson_rows_errors_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, double phi,
                                   int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change,
                                   float* d_next, double* d_raw, double* d_scalars, void* stream) {
  if (!h) return PSM_ERR_ARG;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_POISSON, d_rows, n_frames, width, base, phi, 1.0, 1.0, d_scalars, rc);
  if (r) return r;
  FrameCall fc;
  if ((r = poisson_frame_call(h, rc.cols, n_frames, 8, weighting, d_extra, fc))) return r;
  if ((r = poisson_errors_call_check(h, 8, weighting, d_raw))) return r;
  if (!d_extra || !d_result || !d_next) return fail(h, PSM_ERR_ARG, "the error blocks read d_extra, d_result and d_next: none of them may be NULL");
  const PostCall pc = poisson_post(h, apply_filter, 1, d_result, d_change, d_next);
  hipStream_t st = stream_of(h, stream);
  if ((r = poisson_step_device(h, h->feat.d_vel, n_frames, nullptr, nullptr, pc, st, &fc, &rc))) return r;
  return field_errors_device(h, poisson_error_pairs(h, n_frames, 2, d_extra, d_result, d_next), d_raw, st);
}


int psm_poisson_rows_errors(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, double phi,
                            int32_t apply_filter, int32_t weighting, double* raw, double* scalars) {
  if (!h) return PSM_ERR_ARG;
  if (!rows || !raw) return fail(h, PSM_ERR_ARG, "null buffer");
  FrameSet& F = h->frames;
  RowsSet& R = h->rows;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_POISSON, R.d_rows, n_frames, width, base, phi, 1.0, 1.0, R.d_scalars, rc);
  if (r || (r = host_width_check(h, width))) return r;
  FrameCall fc;
  if ((r = poisson_frame_call(h, rc.cols, n_frames, 8, weighting, F.d_extra, fc))) return r;
  if ((r = poisson_errors_call_check(h, 8, weighting, F.d_raw))) return r;
  PostSet& s = h->post;
  const size_t cap = (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out;
  const PostCall pc = poisson_post(h, apply_filter, 1, s.d_out, s.d_out + cap, s.d_out + 2 * cap);
  hipStream_t st = h->stream;
  const size_t eb = (size_t)n_frames * 3 * PSM_ERR_RAW * sizeof(double), sb = (size_t)n_frames * PSM_ROWS_SCALARS * sizeof(double);
  const PsmFieldErrorArgs stage = poisson_error_pairs(h, n_frames, 2, F.d_extra, pc.result, pc.next);
  if ((r = upload_rows(h, rows, n_frames, width))) return r;
  r = guarded_host_step(h, st, "psm_poisson_rows_errors", [&](int pass) {
    int rs = poisson_step_device(h, h->feat.d_vel, n_frames, nullptr, nullptr, pc, st, &fc, &rc);
    if (rs || (rs = field_errors_device(h, stage, F.d_raw, st))) return rs;
    HIPCHK(h, hipMemcpyAsync(F.h_raw, F.d_raw, eb, hipMemcpyDeviceToHost, st));
    if (scalars && pass == 0) HIPCHK(h, hipMemcpyAsync(R.h_scalars, R.d_scalars, sb, hipMemcpyDeviceToHost, st));
    return PSM_OK;
  });
  if (r) return r;
  memcpy(raw, F.h_raw, eb);
  if (scalars) memcpy(scalars, R.h_scalars, sb);
  return PSM_OK;
}


int psm_gradp_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double ex, double ey, int32_t apply_filter,
                          float* d_gradp, float* d_p, double* d_truth, double* d_raw, double* d_scalars, void* stream) {
  if (!h) return PSM_ERR_ARG;
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_GRADP, d_rows, n_frames, width, 1.0, 1.0, ex, ey, d_scalars, rc);
  if (r) return r;
  return gradp_frames_step(h, rc.cols, n_frames, 5, nullptr, apply_filter, d_gradp, d_p, d_truth, d_raw, stream_of(h, stream), &rc);
}


int psm_gradp_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double ex, double ey, int32_t apply_filter,
                   float* gradp, float* p, double* truth, double* raw, double* scalars) {
  if (!h) return PSM_ERR_ARG;
  if (!rows || !(gradp || p || truth || raw || scalars)) return fail(h, PSM_ERR_ARG, "null buffer");
  RowsSet& R = h->rows;
  hipStream_t st = h->stream;
  // every check of the step before the first copy: the step itself repeats them
  RowsCall rc;
  int r = step_rows_call(h, PSM_ROWS_KIND_GRADP, R.d_rows, n_frames, width, 1.0, 1.0, ex, ey, R.d_scalars, rc);
  if (r || (r = host_width_check(h, width)) || (r = gradp_host_check(h, rc.cols, n_frames, 5, apply_filter))) return r;
  if ((r = upload_rows(h, rows, n_frames, width))) return r;
  HostOut out[5];
  gradp_host_outs(h, n_frames, gradp, p, truth, raw, out);
  out[4] = scalars_out(h, n_frames, scalars);
  return host_step(h, st, "psm_gradp_rows", out, [&] {
    return gradp_frames_step(h, rc.cols, n_frames, 5, nullptr, apply_filter, nullptr, nullptr, nullptr, raw ? h->gradp.d_raw : nullptr, st, &rc);
  });
}

}  // extern "C"
