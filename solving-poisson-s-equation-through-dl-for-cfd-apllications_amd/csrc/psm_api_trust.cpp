// psm_api_trust.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the input-trust score of the last solve -- per block row the squared
// norm n of the centred input block and the residual spe of its PCA round trip, 1 - spe / n being the explained share the model's
// var_in threshold speaks of.  psm_bind_trust builds the Gram matrix of the input basis once; psm_trust_last* are two launches
// (psm_trust.hip) on what the solve left: its image (Ws0Solve::grid, recorded by launch_all and kept through a graph replay) and
// the scaled coefficients in ws0.d_xin.  Nothing here is part of a solve's sequence.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

void trust_free(psm_handle* h) {
  TrustSet& s = h->trust;
  dev_free(s.d_gram); dev_free(s.d_part); dev_free(s.d_out);
  pin_free(s.h_out);
  s.ready = false; s.bands = 0;
}

// What every trust entry asks first, enqueuing nothing: a float32 handle, bound, planned, a solve since the plan, on ws0
static int trust_state(psm_handle* h) {
  if (h->cfg.precision != PSM_PRECISION_F32)
    return fail(h, PSM_ERR_UNSUPPORTED, "the trust score is float32 handles only: a bf16 encode rounds its inputs");
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!h->trust.ready) return fail(h, PSM_ERR_STATE, "psm_bind_trust has not been called (or its binding was dropped by a later psm_set_* / psm_plan_grid)");
  if (h->last_cases < 1 || h->last.n_cases < 1) return fail(h, PSM_ERR_STATE, "no solve has run yet");
  if (!h->last.on_ws0)
    return fail(h, PSM_ERR_STATE, "psm_trust_last follows a synchronous solve (psm_solve_grid / psm_solve_grid_device / psm_solve*); the last solve ran on the ring");
  if (!h->last.grid) return fail(h, PSM_ERR_STATE, "the image of the last solve is gone (its binding or plan was released): solve again");
  return PSM_OK;
}

// The two launches on `st`: band partials of n over the image, then (n, spe) per block row into d_out [n_cases * B][2]
static int trust_device(psm_handle* h, double* d_out, hipStream_t st) {
  const TrustSet& s = h->trust;
  const int n_cases = h->last.n_cases;
  PsmTrustNormArgs na{};
  na.grid = h->last.grid; na.mean = h->d_mean_in; na.blk_y0x0 = h->d_blk; na.part = s.d_part;
  na.S = h->S; na.c_in = h->cfg.c_in; na.Nx = h->Nx; na.B = h->B; na.bands = s.bands; na.n_cases = n_cases;
  na.case_stride = (int64_t)h->Ny * h->Nx * h->cfg.c_in;
  na.aligned = h->plan_aligned && (h->S * h->cfg.c_in) % 4 == 0 && aligned_to(16, {na.grid, na.mean}) ? 1 : 0;
  HIPCHK(h, psm_launch_trust_norm(na, st));
  const PsmTrustFinishArgs fa{s.d_part, h->ws0.d_xin, h->d_ia, h->d_ib, s.d_gram, d_out, n_cases * h->B, s.bands, h->cfg.p_in, h->ld_in};
  HIPCHK(h, psm_launch_trust_finish(fa, st));
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_trust(psm_handle* h, const double* comp_in) {
  if (!h) return PSM_ERR_ARG;
  if (h->cfg.precision != PSM_PRECISION_F32)
    return fail(h, PSM_ERR_UNSUPPORTED, "the trust score is float32 handles only: a bf16 encode rounds its inputs");
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!comp_in) return fail(h, PSM_ERR_ARG, "null comp_in");
  const int P = h->cfg.p_in, K = h->K_in;
  if (P > PSM_TRUST_MAX_P || K > PSM_TRUST_MAX_K) return fail(h, PSM_ERR_UNSUPPORTED, "the trust score holds p_in <= 1024 and block * block * c_in <= 65536");
  if ((int)h->h_ia.size() < P) return fail(h, PSM_ERR_STATE, "psm_set_scaler has not been called");
  for (int p = 0; p < P; ++p)
    if (!std::isfinite(h->h_ia[p]) || h->h_ia[p] == 0.f)
      return fail(h, PSM_ERR_ARG, "the input scaler cannot be undone: a factor of it is zero or not finite in float32");
  for (const PsmBlock& b : h->plan.blocks)                  // what the norm launch reads: S rows of S pixels from every origin
    if (b.y0 < 0 || b.x0 < 0 || b.y0 + h->S > h->Ny || b.x0 + h->S > h->Nx) return fail(h, PSM_ERR_UNSUPPORTED, "a block of the plan reaches beyond the grid");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  trust_free(h);
  TrustSet& s = h->trust;
  s.bands = psm_trust_bands(h->S);
  const size_t rows = (size_t)h->cfg.max_cases * h->B;
  int rc;
  if ((rc = dev_alloc(h, &s.d_gram, (size_t)P * P)) || (rc = dev_alloc(h, &s.d_part, rows * s.bands)) || (rc = dev_alloc(h, &s.d_out, rows * 2)) ||
      (rc = pin_alloc(h, &s.h_out, rows * 2, "psm_bind_trust"))) { trust_free(h); return rc; }
  // the basis as the encode sees it: float32, natural order, for this bind only
  float* d_comp = nullptr;
  {
    std::vector<float> c32((size_t)P * K);
    for (size_t q = 0; q < c32.size(); ++q) c32[q] = (float)comp_in[q];
    if ((rc = dev_upload(h, &d_comp, c32))) { trust_free(h); return rc; }
  }
  hipError_t e = psm_launch_trust_gram(d_comp, s.d_gram, P, K, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  dev_free(d_comp);
  if (e != hipSuccess) { trust_free(h); return fail(h, PSM_ERR_HIP, std::string("psm_bind_trust: ") + hipGetErrorString(e)); }
  s.ready = true;
  return PSM_OK;
}


int psm_unbind_trust(psm_handle* h) {
  return unbind(h, [h] { trust_free(h); });
}


int psm_trust_last_device(psm_handle* h, double* d_out, void* stream) {
  if (!h) return PSM_ERR_ARG;
  int rc = trust_state(h);
  if (rc) return rc;
  if (!d_out) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!aligned_to(8, {d_out})) return fail(h, PSM_ERR_ARG, "d_out must be 8-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return trust_device(h, d_out, stream_of(h, stream));
}


int psm_trust_last(psm_handle* h, int32_t* n_cases, double* out, size_t out_doubles) {
  if (!h) return PSM_ERR_ARG;
  int rc = trust_state(h);
  if (rc) return rc;
  if (!out) return fail(h, PSM_ERR_ARG, "null buffer");
  const size_t n = (size_t)h->last.n_cases * h->B * 2;
  if (out_doubles < n) return fail(h, PSM_ERR_ARG, "destination too small: 2 doubles per block row of the last solve");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipDeviceSynchronize());                        // the solve may have run on the caller's stream
  TrustSet& s = h->trust;
  hipStream_t st = h->stream;
  if ((rc = trust_device(h, s.d_out, st))) return rc;
  HIPCHK(h, hipMemcpyAsync(s.h_out, s.d_out, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(st));
  memcpy(out, s.h_out, n * sizeof(double));
  if (n_cases) *n_cases = h->last.n_cases;
  return PSM_OK;
}

}  // extern "C"
