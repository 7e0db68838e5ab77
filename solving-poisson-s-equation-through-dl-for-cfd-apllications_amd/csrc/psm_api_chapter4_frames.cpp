// psm_api_chapter4_frames.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the frame batch of the two Chapter-4 evaluators
// (Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py: (Ux, Uy, SDF) -> p; Chapter4/MLP/M_fU/Evaluation/Eval.py: (f(U), SDF) -> p)
// on the device.  psm_bind_chapter4_frames stands on psm_bind_frames; psm_chapter4_image_device is the image stage alone (the mesh ->
// grid launch of psm_api_frames.cpp, then the pack: the PsmChapter4PackArgs overload of psm_to_grid_kernel, psm_pack.hip);
// psm_chapter4_frames* put planes -> image, label -> one solve per frame into one graph replay (solve_device, psm_api_step.cpp) and
// the field-error launches of psm_api_errors.cpp with one pair behind it, so that a metrics-only sweep returns 8 doubles per frame.
// No block stage and no dimensional scale: the reference compares prediction and label in normalised units (M_u :457-476).
// See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// captured step graphs (StepCall::chapter4) hold the addresses of the binding's planes and SDF plane
static void drop_chapter4_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.chapter4.planes != nullptr; }); }

// columns 0 .. c_in - 1 are stored; c_in + 1 scales, the SDF plane by max_abs[c_in - 1] (the statements of M_u :215-225 on the SDF channel)
static const EvalKind CHAPTER4{
    "psm_bind_chapter4_frames", 0, 0, -1, 1, 1,
    "k outside [c_in, 16]: the c_in - 1 input channels (Ux / U, Uy / U or f(U) / U^2), then p / U^2; further columns are not stored",
    "a destination is misaligned (4 bytes for the image, 8 for the truth plane)",
    "psm_bind_chapter4_frames has not been called (psm_bind_frames, a new mesh, plan or model drop the binding)"};

void chapter4_free(psm_handle* h) {
  Chapter4Set& s = h->chapter4;
  drop_chapter4_graphs(h);
  dev_free(s.d_result);
  pin_free(s.h_result);
  eval_free(s);
  image_gone(h);
}

// The pack launch on `st`: the binding's SDF plane and scales, the call's planes and destinations.
int chapter4_pack_device(psm_handle* h, const Chapter4Call& cc, int n_frames, hipStream_t st) {
  const Chapter4Set& S = h->chapter4;
  const int c_in = h->cfg.c_in;
  PsmChapter4PackArgs a{};
  a.planes = cc.planes; a.sdn = S.d_sdn;
  a.grid = cc.grid; a.truth = cc.truth;
  a.npix = (int64_t)h->Ny * h->Nx;
  a.m[0] = S.max_abs[0]; a.m[1] = c_in == 3 ? S.max_abs[1] : 1.0; a.m_p = S.max_abs[c_in];
  a.c_in = c_in; a.n_frames = n_frames;
  HIPCHK(h, psm_launch_chapter4_pack(a, st));
  return PSM_OK;
}

// The error block behind a step: the two field-error launches, one pair over the binding's SDF plane.
static int chapter4_step_errors_device(psm_handle* h, int n_frames, const float* d_result, const double* d_truth, double* d_raw, hipStream_t st) {
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  const PsmErrPlane none{nullptr, 0, 0, 0};
  PsmFieldErrorArgs a{};
  a.mask = PsmErrPlane{h->chapter4.d_sdn, 0, 1, 0};       // one plane for every frame
  a.pair[0] = PsmFieldErrorPair{PsmErrPlane{d_result, npix, 1, 1}, PsmErrPlane{d_truth, npix, 1, 0}, none, none, 0};
  a.n_pairs = 1; a.n_frames = n_frames;
  return field_errors_device(h, a, d_raw, st);
}

// a device or a host entry's step: null destinations become the binding's; every check of the step; the one graph replay: frames ->
// planes -> image, label -> one solve per frame; the error block when d_raw is given
static int chapter4_frames_step(psm_handle* h, const double* d_cols, int n_frames, int k, float* d_result, double* d_truth, double* d_raw,
                                hipStream_t st) {
  Chapter4Set& S = h->chapter4;
  if (!d_result) d_result = S.d_result;
  if (!d_truth) d_truth = S.d_truth;
  StepCall step;
  int rc = eval_image_call(h, h->chapter4, CHAPTER4, d_cols, n_frames, k, S.d_grid, d_truth, step.frames);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(d_result) & 3) || (reinterpret_cast<uintptr_t>(d_raw) & 7))
    return fail(h, PSM_ERR_ARG, "a destination is misaligned (4 bytes for d_result, 8 for d_raw)");
  step.chapter4 = Chapter4Call{S.d_planes, S.d_grid, d_truth};
  rc = solve_device(h, S.d_grid, n_frames, nullptr, d_result, st, nullptr, step);
  if (rc || !d_raw) return rc;
  return chapter4_step_errors_device(h, n_frames, d_result, d_truth, d_raw, st);
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_chapter4_frames(psm_handle* h, const double* sdfunct, const double* max_abs) {
  if (!h) return PSM_ERR_ARG;
  int rc = frames_state(h);
  if (rc) return rc;
  const int c_in = h->cfg.c_in;
  if (h->cfg.variant != PSM_VARIANT_CHAPTER5 || h->cfg.c_out != 1 || (c_in != 2 && c_in != 3) || h->cfg.sdf_channel != c_in - 1)
    return fail(h, PSM_ERR_STATE, "the Chapter-4 frames are a two- or three-channel image with the SDF last and a one-channel field on a chapter5-variant handle: variant == PSM_VARIANT_CHAPTER5, c_out == 1, c_in in {2, 3}, sdf_channel == c_in - 1");
  Chapter4Set& s = h->chapter4;
  return eval_bind(h, s, CHAPTER4, sdfunct, max_abs, chapter4_free, [&](size_t n, size_t npix) {
    const int ro = dev_alloc(h, &s.d_result, n * npix);
    return ro ? ro : pin_alloc(h, &s.h_result, n * npix, CHAPTER4.bind_name);
  });
}


int psm_unbind_chapter4_frames(psm_handle* h) {
  return unbind(h, [h] { chapter4_free(h); });
}


int psm_chapter4_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_grid, double* d_truth, void* stream) {
  if (!h) return PSM_ERR_ARG;
  FrameCall fc;
  int rc = eval_image_call(h, h->chapter4, CHAPTER4, d_cols, n_frames, k, d_grid, d_truth, fc);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = stream_of(h, stream);
  if ((rc = frames_device(h, fc, n_frames, st))) return rc;
  return chapter4_pack_device(h, Chapter4Call{h->chapter4.d_planes, d_grid, d_truth}, n_frames, st);
}


int psm_chapter4_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_result, double* d_truth,
                               double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  return chapter4_frames_step(h, d_cols, n_frames, k, d_result, d_truth, d_raw, stream_of(h, stream));
}


int psm_chapter4_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, float* result, double* truth, double* raw) {
  if (!h) return PSM_ERR_ARG;
  if (!cols || !(result || truth || raw)) return fail(h, PSM_ERR_ARG, "null buffer");
  const double* d_cols = h->frames.d_cols;
  Chapter4Set& S = h->chapter4;
  hipStream_t st = h->stream;
  // every check of the step before the first copy: the step itself repeats them
  FrameCall fc;
  int rc = eval_image_call(h, h->chapter4, CHAPTER4, d_cols, n_frames, k, S.d_grid, S.d_truth, fc);
  if (rc || (rc = frames_upload_cols(h, cols, n_frames, k))) return rc;
  const size_t fb = (size_t)n_frames * h->Ny * h->Nx * sizeof(float);
  const HostOut out[3] = {{result, S.h_result, S.d_result, fb, false},
                          {truth, S.h_truth, S.d_truth, 2 * fb, true},            // the labels do not depend on the route
                          {raw, S.h_raw, S.d_raw, (size_t)n_frames * PSM_ERR_RAW * sizeof(double), false}};
  return host_step(h, st, "psm_chapter4_frames", out, [&] { return chapter4_frames_step(h, d_cols, n_frames, k, nullptr, nullptr, raw ? S.d_raw : nullptr, st); });
}

}  // extern "C"
