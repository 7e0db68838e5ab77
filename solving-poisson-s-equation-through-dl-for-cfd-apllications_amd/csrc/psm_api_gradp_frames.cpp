// psm_api_gradp_frames.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the frame batch of the U_to_gradP evaluator on the device.
// psm_bind_gradp_frames stands on psm_bind_frames and holds integration tables of its own (integ_bind of psm_api_integ.cpp, the
// simulation's one geometry for every frame slot); psm_gradp_image_device is the image stage alone (the mesh -> grid launch of
// psm_api_frames.cpp, then the pack: the PsmGradpPackArgs overload of psm_to_grid_kernel, psm_pack.hip); psm_gradp_frames* put
// planes -> image, labels -> one solve per frame (-> filter) -> integration into one graph replay (solve_device, psm_api_solve.cpp)
// and the field-error launches of psm_api_errors.cpp with four pairs behind it, so that a metrics-only sweep returns 32 doubles per
// frame.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

constexpr int GRADP_PAIRS = 4;
static_assert(GRADP_PAIRS <= PSM_FIELD_ERR_MAX_PAIRS, "the step's error blocks are one call of the field-error stage");

// captured step graphs (StepCall::gradp) hold the addresses of the binding's planes, SDF plane and integration tables
static void drop_gradp_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.gradp.planes != nullptr; }); }

// columns 0-4 are stored; five scales, the SDF plane by max_abs[2] (the statements of Eval_dual_Dense_onlycil.py:461-465 on the SDF channel)
static const EvalKind GRADP{
    "psm_bind_gradp_frames", 5, 5, 2, 3, GRADP_PAIRS,
    "k outside [5, 16]: (Ux / U, Uy / U, dPdx / U^2, dPdy / U^2, p / U^2), further columns are not stored",
    "a destination is misaligned (4 bytes for the image, 8 for the label planes)",
    "psm_bind_gradp_frames has not been called (psm_bind_frames, a new mesh, plan or model drop the binding)"};

void gradp_free(psm_handle* h) {
  GradpSet& s = h->gradp;
  drop_gradp_graphs(h);
  integ_free(s.integ);
  pin_free(s.h_gradp); pin_free(s.h_p);
  eval_free(s);
  image_gone(h);
}

// The pack launch on `st`: the binding's SDF plane and scales, the call's planes and destinations.
int gradp_pack_device(psm_handle* h, const GradpCall& gc, int n_frames, hipStream_t st) {
  const GradpSet& G = h->gradp;
  PsmGradpPackArgs a{};
  a.planes = gc.planes; a.sdn = G.d_sdn;
  a.grid = gc.grid; a.truth = gc.truth;
  a.npix = (int64_t)h->Ny * h->Nx;
  a.m0 = G.max_abs[0]; a.m1 = G.max_abs[1]; a.m3 = G.max_abs[3]; a.m4 = G.max_abs[4];
  a.n_frames = n_frames;
  HIPCHK(h, psm_launch_gradp_pack(a, st));
  return PSM_OK;
}

// The error blocks behind a step: the two field-error launches, four pairs over the binding's SDF plane.
static int gradp_step_errors_device(psm_handle* h, int n_frames, const float* d_gradp, const float* d_p, const double* d_truth, double* d_raw,
                              hipStream_t st) {
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  const PsmErrPlane none{nullptr, 0, 0, 0};
  const PsmErrPlane p{d_p, npix, 1, 1}, gx{d_gradp, 2 * npix, 2, 1}, gy{d_gradp + 1, 2 * npix, 2, 1};
  const PsmErrPlane t0{d_truth, 3 * npix, 1, 0}, t1{d_truth + npix, 3 * npix, 1, 0}, t2{d_truth + 2 * npix, 3 * npix, 1, 0};
  PsmFieldErrorArgs a{};
  a.mask = PsmErrPlane{h->gradp.d_sdn, 0, 1, 0};          // one plane for every frame
  a.pair[0] = PsmFieldErrorPair{p, t0, none, none, 0};    // the reference's own metric (:667-687)
  a.pair[1] = PsmFieldErrorPair{p, t2, none, none, 0};    // p against the pressure label
  a.pair[2] = PsmFieldErrorPair{gx, t0, none, none, 0};   // the network's own output against its labels
  a.pair[3] = PsmFieldErrorPair{gy, t1, none, none, 0};
  a.n_pairs = GRADP_PAIRS; a.n_frames = n_frames;
  return field_errors_device(h, a, d_raw, st);
}

// every check of one step; nothing is enqueued before they pass
static int gradp_step_check(psm_handle* h, const double* d_cols, int n_frames, int k, int apply_filter, const float* d_gradp, const float* d_p,
                            const double* d_truth, const double* d_raw, FrameCall& fc) {
  int rc = eval_image_call(h, h->gradp, GRADP, d_cols, n_frames, k, h->gradp.d_grid, d_truth, fc);
  if (rc) return rc;
  if (apply_filter && !h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: apply_filter needs it as well as psm_bind_gradp_frames");
  if ((reinterpret_cast<uintptr_t>(d_gradp) & 7) || (reinterpret_cast<uintptr_t>(d_p) & 3) || (reinterpret_cast<uintptr_t>(d_raw) & 7))
    return fail(h, PSM_ERR_ARG, "a destination is misaligned (8 bytes for d_gradp and d_raw, 4 for d_p)");
  return PSM_OK;
}

int gradp_host_check(psm_handle* h, const double* d_cols, int n_frames, int k, int apply_filter) {
  const GradpSet& G = h->gradp;
  FrameCall fc;
  return gradp_step_check(h, d_cols, n_frames, k, apply_filter, G.integ.d_gradp, G.integ.d_p, G.d_truth, G.d_raw, fc);
}

// null destinations become the binding's; the checks; the one graph replay: frames -> planes -> image, labels -> solve (-> filter) ->
// integration; the error blocks when d_raw is given
int gradp_frames_step(psm_handle* h, const double* d_cols, int n_frames, int k, const float* out_scale, int apply_filter, float* d_gradp,
                      float* d_p, double* d_truth, double* d_raw, hipStream_t st, const RowsCall* rows) {
  GradpSet& G = h->gradp;
  if (!d_gradp) d_gradp = G.integ.d_gradp;
  if (!d_p) d_p = G.integ.d_p;
  if (!d_truth) d_truth = G.d_truth;
  StepCall step;
  int rc = gradp_step_check(h, d_cols, n_frames, k, apply_filter, d_gradp, d_p, d_truth, d_raw, step.frames);
  if (rc) return rc;
  if (rows) step.rows = *rows;
  step.gradp = GradpCall{G.d_planes, G.d_grid, d_truth, d_p};
  if (apply_filter) { step.post.apply_filter = 1; step.post.result = d_gradp; }
  rc = solve_device(h, G.d_grid, n_frames, out_scale, apply_filter ? h->post.d_fields : d_gradp, st, nullptr, step);
  if (rc || !d_raw) return rc;
  return gradp_step_errors_device(h, n_frames, d_gradp, d_p, d_truth, d_raw, st);
}

void gradp_host_outs(psm_handle* h, int n_frames, float* gradp, float* p, double* truth, double* raw, HostOut* out) {
  const GradpSet& G = h->gradp;
  const size_t npix = (size_t)h->Ny * h->Nx, pb = (size_t)n_frames * npix * sizeof(float);
  out[0] = HostOut{gradp, G.h_gradp, G.integ.d_gradp, 2 * pb, false};
  out[1] = HostOut{p, G.h_p, G.integ.d_p, pb, false};
  out[2] = HostOut{truth, G.h_truth, G.d_truth, (size_t)n_frames * 3 * npix * sizeof(double), true};   // the labels do not depend on the route
  out[3] = HostOut{raw, G.h_raw, G.d_raw, (size_t)n_frames * GRADP_PAIRS * PSM_ERR_RAW * sizeof(double), false};
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_gradp_frames(psm_handle* h, const double* sdfunct, const double* max_abs, int32_t center_y, int32_t center_x, double dx,
                          double dy) {
  if (!h) return PSM_ERR_ARG;
  int rc = frames_state(h);
  if (rc) return rc;
  if (h->cfg.c_in != 3 || h->cfg.sdf_channel != 2 || h->cfg.c_out != 2)
    return fail(h, PSM_ERR_STATE, "the gradP frames are a three-channel image with the SDF last and a (dp/dx, dp/dy) field: c_in == 3, sdf_channel == 2, c_out == 2");
  GradpSet& s = h->gradp;
  return eval_bind(h, s, GRADP, sdfunct, max_abs, gradp_free, [&](size_t n, size_t npix) {
    // the tables first: a geometry the reference cannot process (PSM_ERR_UNSUPPORTED) or a cut outside the grid (PSM_ERR_ARG) binds nothing
    int ro = integ_bind(h, s.integ, h->Ny, h->Nx, sdfunct, (int)n, &center_y, &center_x, dx, dy, true);
    if (ro || (ro = pin_alloc(h, &s.h_gradp, n * npix * 2, GRADP.bind_name))) return ro;
    return pin_alloc(h, &s.h_p, n * npix, GRADP.bind_name);
  });
}


int psm_unbind_gradp_frames(psm_handle* h) {
  return unbind(h, [h] { gradp_free(h); });
}


int psm_gradp_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_grid, double* d_truth, void* stream) {
  if (!h) return PSM_ERR_ARG;
  FrameCall fc;
  int rc = eval_image_call(h, h->gradp, GRADP, d_cols, n_frames, k, d_grid, d_truth, fc);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = stream_of(h, stream);
  if ((rc = frames_device(h, fc, n_frames, st))) return rc;
  return gradp_pack_device(h, GradpCall{h->gradp.d_planes, d_grid, d_truth, nullptr}, n_frames, st);
}


int psm_gradp_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const float* out_scale,
                            int32_t apply_filter, float* d_gradp, float* d_p, double* d_truth, double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  return gradp_frames_step(h, d_cols, n_frames, k, out_scale, apply_filter, d_gradp, d_p, d_truth, d_raw, stream_of(h, stream));
}


int psm_gradp_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const float* out_scale, int32_t apply_filter,
                     float* gradp, float* p, double* truth, double* raw) {
  if (!h) return PSM_ERR_ARG;
  if (!cols || !(gradp || p || truth || raw)) return fail(h, PSM_ERR_ARG, "null buffer");
  const double* d_cols = h->frames.d_cols;
  hipStream_t st = h->stream;
  // every check of the step before the first copy: the step itself repeats them
  int rc = gradp_host_check(h, d_cols, n_frames, k, apply_filter);
  if (rc || (rc = frames_upload_cols(h, cols, n_frames, k))) return rc;
  HostOut out[4];
  gradp_host_outs(h, n_frames, gradp, p, truth, raw, out);
  return host_step(h, st, "psm_gradp_frames", out, [&] {
    return gradp_frames_step(h, d_cols, n_frames, k, out_scale, apply_filter, nullptr, nullptr, nullptr, raw ? h->gradp.d_raw : nullptr, st);
  });
}

}  // extern "C"
