// psm_api_errors.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the per-frame error blocks of assembled fields on the device.
// psm_field_errors_device is the stage alone -- two plain launches (the PsmFieldErrorArgs / PsmFieldErrorFinalArgs overloads of
// psm_block_error_kernel, psm_eval.hip) that leave raw[n_frames][n_pairs][8] sums for psm_error_metrics_from_sums (psm_errors.cpp);
// psm_poisson_frames_errors* put it behind the Poisson evaluator's frame step of psm_api_frames.cpp with the three pairs the
// reference prints (pressureSM_Poisson/SM_call.py:962-1043), so that a metrics-only sweep returns 24 doubles per frame and no field.
// See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

static_assert(PSM_ERR_MAX_PAIRS == PSM_FIELD_ERR_MAX_PAIRS, "psm.h and psm_eval.h disagree on the pairs of one call");
static_assert(sizeof(psm_err_plane) == 32 && sizeof(psm_err_pair) == 136, "layout of the public descriptors (mirrored by _lib.py)");

static PsmErrPlane plane_of(const psm_err_plane& p) { return PsmErrPlane{p.ptr, p.frame_stride, p.elem_stride, p.as_f32 ? 1 : 0}; }

// a plane the stage reads: present unless `optional`, aligned to its element, strides not negative
static const char* plane_fault(const psm_err_plane& p, bool optional) {
  if (!p.ptr) return optional ? nullptr : "a mask, pred or truth plane is NULL";
  if (reinterpret_cast<uintptr_t>(p.ptr) & (p.as_f32 ? 3 : 7)) return "a plane is misaligned (8 bytes for float64, 4 for float32)";
  if (p.frame_stride < 0 || p.elem_stride < 0) return "strides must not be negative";
  return nullptr;
}

// The two launches on `st`; the partials live in the plan's scratch (max_cases x PSM_ERR_MAX_PAIRS rows).
int field_errors_device(psm_handle* h, const PsmFieldErrorArgs& stage, double* d_raw, hipStream_t st) {
  PsmFieldErrorArgs a = stage;
  a.npix = (int64_t)h->Ny * h->Nx;
  a.n_wg = psm_field_error_workgroups(a.npix);
  a.part = h->d_err_part;
  HIPCHK(h, psm_launch_field_errors(a, st));
  HIPCHK(h, psm_launch_field_errors_final(PsmFieldErrorFinalArgs{h->d_err_part, d_raw, a.n_wg}, a.n_pairs, a.n_frames, st));
  return PSM_OK;
}

// The evaluator's three pairs on what a frame step leaves: delta-p with the weighting (next), without it (result), and p
// (next + p label - delta-p label against the p label); the labels are the first two extra planes, NaN -> 0 (SM_call.py:687-711).
PsmFieldErrorArgs poisson_error_pairs(const psm_handle* h, int n_frames, int n_extra, const double* d_extra, const float* d_result, const float* d_next) {
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  const PsmErrPlane none{nullptr, 0, 0, 0};
  const PsmErrPlane dp{d_extra, n_extra * npix, 1, 0}, p{d_extra + npix, n_extra * npix, 1, 0};
  const PsmErrPlane next{d_next, npix, 1, 1}, result{d_result, npix * h->cfg.c_out, h->cfg.c_out, 1};
  PsmFieldErrorArgs a{};
  a.mask = PsmErrPlane{h->feat.d_sdf, npix, 1, 0};
  a.pair[0] = PsmFieldErrorPair{next, dp, none, none, 1};
  a.pair[1] = PsmFieldErrorPair{result, dp, none, none, 1};
  a.pair[2] = PsmFieldErrorPair{next, p, p, dp, 1};
  a.n_pairs = 3; a.n_frames = n_frames;
  return a;
}

int poisson_errors_call_check(psm_handle* h, int k, int weighting, const void* d_raw) {
  if (!weighting) return fail(h, PSM_ERR_ARG, "the error blocks compare the weighted field: weighting must be on");
  if (k < 8) return fail(h, PSM_ERR_ARG, "the error blocks need the two label columns (delta_p, p) between the velocities and the weighting pair: k >= 8");
  if (!d_raw) return fail(h, PSM_ERR_ARG, "null buffer");
  if (reinterpret_cast<uintptr_t>(d_raw) & 7) return fail(h, PSM_ERR_ARG, "d_raw must be 8-byte aligned");
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_field_errors_device(psm_handle* h, const psm_err_plane* mask, const psm_err_pair* pairs, int32_t n_pairs, int32_t n_frames,
                            double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!mask || !pairs || !d_raw) return fail(h, PSM_ERR_ARG, "null argument");
  if (n_pairs < 1 || n_pairs > PSM_ERR_MAX_PAIRS) return fail(h, PSM_ERR_ARG, "n_pairs outside [1, 4]");
  if (n_frames < 1 || n_frames > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_frames outside [1, max_cases]");
  if (reinterpret_cast<uintptr_t>(d_raw) & 7) return fail(h, PSM_ERR_ARG, "d_raw must be 8-byte aligned");
  const char* bad = plane_fault(*mask, false);
  for (int p = 0; p < n_pairs && !bad; ++p) {
    bad = plane_fault(pairs[p].pred, false);
    if (!bad) bad = plane_fault(pairs[p].truth, false);
    if (!bad) bad = plane_fault(pairs[p].add, true);
    if (!bad) bad = plane_fault(pairs[p].sub, true);
  }
  if (bad) return fail(h, PSM_ERR_ARG, bad);
  PsmFieldErrorArgs a{};
  a.mask = plane_of(*mask);
  for (int p = 0; p < n_pairs; ++p)
    a.pair[p] = PsmFieldErrorPair{plane_of(pairs[p].pred), plane_of(pairs[p].truth), plane_of(pairs[p].add), plane_of(pairs[p].sub),
                                  pairs[p].truth_nan_to_zero ? 1 : 0};
  a.n_pairs = n_pairs; a.n_frames = n_frames;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return field_errors_device(h, a, d_raw, stream_of(h, stream));
}


int psm_poisson_frames_errors_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* LU, const float* out_scale,
                                     int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change, float* d_next,
                                     double* d_raw, void* stream) {
  if (!h) return PSM_ERR_ARG;
  FrameCall fc;
  int rc = poisson_frame_call(h, d_cols, n_frames, k, weighting, d_extra, fc);
  if (rc) return rc;
  if ((rc = poisson_errors_call_check(h, k, weighting, d_raw))) return rc;
  if (!d_extra || !d_result || !d_next) return fail(h, PSM_ERR_ARG, "the error blocks read d_extra, d_result and d_next: none of them may be NULL");
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.result = d_result;
  pc.dU = h->post.d_dU; pc.prev = h->post.d_prev; pc.change = d_change; pc.next = d_next;
  hipStream_t st = stream_of(h, stream);
  if ((rc = poisson_step_device(h, h->feat.d_vel, n_frames, LU, out_scale, pc, st, &fc))) return rc;
  return field_errors_device(h, poisson_error_pairs(h, n_frames, k - 6, d_extra, d_result, d_next), d_raw, st);
}


int psm_poisson_frames_errors(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* LU, const float* out_scale,
                              int32_t apply_filter, int32_t weighting, double* raw) {
  if (!h) return PSM_ERR_ARG;
  if (!cols || !raw) return fail(h, PSM_ERR_ARG, "null buffer");
  FrameSet& F = h->frames;
  FrameCall fc;
  int rc = poisson_frame_call(h, F.d_cols, n_frames, k, weighting, F.d_extra, fc);
  if (rc) return rc;
  if ((rc = poisson_errors_call_check(h, k, weighting, F.d_raw))) return rc;
  PostSet& s = h->post;
  const size_t cap = (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out;
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.result = s.d_out;
  pc.dU = s.d_dU; pc.prev = s.d_prev; pc.change = s.d_out + cap; pc.next = s.d_out + 2 * cap;
  hipStream_t st = h->stream;
  const size_t rb = (size_t)n_frames * 3 * PSM_ERR_RAW * sizeof(double);
  const PsmFieldErrorArgs stage = poisson_error_pairs(h, n_frames, k - 6, F.d_extra, pc.result, pc.next);
  if ((rc = frames_upload_cols(h, cols, n_frames, k))) return rc;
  rc = guarded_host_step(h, st, "psm_poisson_frames_errors", [&](int) {
    int rs = poisson_step_device(h, h->feat.d_vel, n_frames, LU, out_scale, pc, st, &fc);
    if (rs || (rs = field_errors_device(h, stage, F.d_raw, st))) return rs;
    HIPCHK(h, hipMemcpyAsync(F.h_raw, F.d_raw, rb, hipMemcpyDeviceToHost, st));
    return PSM_OK;
  });
  if (rc) return rc;
  memcpy(raw, F.h_raw, rb);
  return PSM_OK;
}

}  // extern "C"
