// psm_api_features.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the pressureSM_Poisson input features on the device, case-batched
// (psm_bind_features, psm_features_device) and the whole Poisson time step behind them as one graph replay (psm_poisson_step*):
// d_vel -> features -> solve -> post-steps.  The host entry psm_poisson_features (one case, host arrays) is the first entry below.  Kernels: psm_features.hip.
// See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

void feat_free(FeatureSet& s) {
  dev_free(s.d_sdf); dev_free(s.d_term); dev_free(s.d_partial); dev_free(s.d_lu); dev_free(s.d_grid); dev_free(s.d_vel);
  pin_free(s.h_lu);
  for (auto& e : s.lu_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  s.ready = false; s.n_cases = 0; s.lu_pos = 0;
}

// captured step graphs (StepCall::feat) hold the addresses of the binding's planes and scratch
static void drop_feature_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.feat.vel != nullptr; }); }

// The two feature launches of d_vel [n][4][npix] into d_grid [n][npix][4] on `st`; (L, U) per case are read from the binding's d_lu.
int features_device(psm_handle* h, const double* d_vel, int n, float* d_grid, hipStream_t st) {
  const FeatureSet& F = h->feat;
  const int64_t npix = (int64_t)h->Ny * h->Nx;
  PsmFeatureArgs fa{};
  fa.ux = d_vel; fa.uy = d_vel + npix; fa.dux = d_vel + 2 * npix; fa.duy = d_vel + 3 * npix; fa.sdf = F.d_sdf;
  fa.vel_stride = 4 * npix; fa.sdf_stride = npix; fa.n_cases = n;
  fa.term = F.d_term; fa.partial = F.d_partial; fa.grid = d_grid; fa.ny = h->Ny; fa.nx = h->Nx;
  fa.lu = F.d_lu; fa.k = F.k;
  for (int q = 0; q < 4; ++q) fa.max_abs[q] = F.max_abs[q];
  HIPCHK(h, psm_launch_poisson_features(fa, st));
  return PSM_OK;
}

// state and argument checks shared by the entries below; nothing is enqueued before they pass
static int feat_check_state(psm_handle* h, int n_cases) {
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!h->feat.ready) return fail(h, PSM_ERR_STATE, "psm_bind_features has not been called (a new plan or model drops the binding)");
  if (n_cases < 1 || n_cases > h->feat.n_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, cases bound with psm_bind_features]");
  return PSM_OK;
}
static int feat_check(psm_handle* h, int n_cases, const double* LU) {
  int rc = feat_check_state(h, n_cases);
  if (rc) return rc;
  if (!LU) return fail(h, PSM_ERR_ARG, "null argument");
  for (int c = 0; c < n_cases; ++c)
    if (!(LU[2 * c + 1] != 0.0) || !std::isfinite(LU[2 * c + 1])) return fail(h, PSM_ERR_ARG, "U must be finite and non-zero for every case");
  return PSM_OK;
}

// (L, U) of this step: a pinned ring slot + hipMemcpyAsync in front of the launches / the replay, outside any captured graph
static int upload_lu(psm_handle* h, const double* LU, int n_cases, hipStream_t st) {
  FeatureSet& F = h->feat;
  const int slot = F.lu_pos;
  F.lu_pos = (F.lu_pos + 1) % FeatureSet::RING;
  HIPCHK(h, hipEventSynchronize(F.lu_ev[slot]));
  double* p = F.h_lu + (size_t)slot * F.n_cases * 2;
  memcpy(p, LU, (size_t)n_cases * 2 * sizeof(double));
  HIPCHK(h, hipMemcpyAsync(F.d_lu, p, (size_t)n_cases * 2 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipEventRecord(F.lu_ev[slot], st));
  return PSM_OK;
}

PostCall post_call(int apply_filter, const float* dU, const float* prev, float* result, float* change, float* next) {
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0; pc.dU = dU; pc.prev = prev; pc.result = result; pc.change = change; pc.next = next;
  return pc;
}

// every check of one whole step, then its scalars and the one graph replay: (frames -> planes,) features into the binding's image, solve,
// post-steps
int poisson_step_device(psm_handle* h, const double* d_vel, int n_cases, const double* LU, const float* out_scale, const PostCall& pc, hipStream_t st,
                        const FrameCall* frames, const RowsCall* rows, const PoissonSolveCall* psolve) {
  const bool device_lu = rows || psolve;                   // (L, U) are made on the device, nothing to check or upload
  int rc = device_lu ? feat_check_state(h, n_cases) : feat_check(h, n_cases, LU);
  if (rc) return rc;
  if (!h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: a Poisson step needs it as well as psm_bind_features");
  if ((rc = post_check(h, n_cases, pc))) return rc;
  if (!d_vel) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (!st) st = h->stream;
  if (!device_lu && (rc = upload_lu(h, LU, n_cases, st))) return rc;
  StepCall step;
  if (psolve) step.psolve = *psolve;
  if (rows) step.rows = *rows;
  if (frames) step.frames = *frames;
  step.feat = FeatCall{d_vel, h->feat.d_grid};
  step.post = pc;
  return solve_device(h, step.feat.grid, n_cases, out_scale, h->post.d_fields, st, nullptr, step);
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_poisson_features(psm_handle* h, const double* ux, const double* uy, const double* dux, const double* duy,
                         const double* sdfunct, int32_t ny, int32_t nx, const double* params, float* grid_out) {
  if (!h) return PSM_ERR_ARG;
  if (!ux || !uy || !dux || !duy || !sdfunct || !params || !grid_out) return fail(h, PSM_ERR_ARG, "null argument");
  if (ny < 2 || nx < 2 || (int64_t)ny * nx > ((int64_t)1 << 26)) return fail(h, PSM_ERR_ARG, "grid must be at least 2x2 (np.gradient)");
  if (!(params[1] != 0.0)) return fail(h, PSM_ERR_ARG, "U must be non-zero");
  for (int q = 3; q < 7; ++q)
    if (!(params[q] != 0.0)) return fail(h, PSM_ERR_ARG, "max_abs scales must be non-zero");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t n = (size_t)ny * nx, nwg = (n + 255) / 256;
  int rc;
  const size_t ib = 5 * n * sizeof(double), gb = 4 * n * sizeof(float);
  if ((rc = scratch_reserve(h, carve_size({ib, n * sizeof(double), 2 * nwg * sizeof(double), gb}), carve_size({ib, gb})))) return rc;
  Carver cd{(char*)h->scr_dev}, cp{(char*)h->scr_pin};
  double* d_in = cd.take<double>(5 * n); double* d_term = cd.take<double>(n); double* d_part = cd.take<double>(2 * nwg);
  float* d_grid = cd.take<float>(4 * n);
  double* p_in = cp.take<double>(5 * n); float* p_grid = cp.take<float>(4 * n);
  const double* src[5] = {ux, uy, dux, duy, sdfunct};
  for (int q = 0; q < 5; ++q) memcpy(p_in + q * n, src[q], n * sizeof(double));
  hipError_t e = hipMemcpyAsync(d_in, p_in, ib, hipMemcpyHostToDevice, st);
  PsmFeatureArgs fa{};
  fa.ux = d_in; fa.uy = d_in + n; fa.dux = d_in + 2 * n; fa.duy = d_in + 3 * n; fa.sdf = d_in + 4 * n;
  fa.term = d_term; fa.partial = d_part; fa.grid = d_grid; fa.ny = ny; fa.nx = nx;
  fa.L = params[0]; fa.U = params[1]; fa.k = params[2];
  for (int q = 0; q < 4; ++q) fa.max_abs[q] = params[3 + q];
  if (e == hipSuccess) e = psm_launch_poisson_features(fa, st);
  if (e == hipSuccess) e = hipMemcpyAsync(p_grid, d_grid, gb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = wait_stream(st);
  if (e == hipSuccess) memcpy(grid_out, p_grid, gb);
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string("poisson features: ") + hipGetErrorString(e));
  return PSM_OK;
}


int psm_bind_features(psm_handle* h, const double* sdfunct, int32_t n_cases, double k, const double* max_abs) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (h->cfg.c_in != 4 || h->cfg.sdf_channel != 3)
    return fail(h, PSM_ERR_STATE, "the Poisson features are a four-channel image with the SDF last: c_in == 4 and sdf_channel == 3");
  if (!sdfunct || !max_abs) return fail(h, PSM_ERR_ARG, "null argument");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  if (!std::isfinite(k)) return fail(h, PSM_ERR_ARG, "k must be finite");
  for (int q = 0; q < 4; ++q)
    if (!(max_abs[q] != 0.0)) return fail(h, PSM_ERR_ARG, "max_abs scales must be non-zero");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // features in flight read the planes that are replaced,
  drop_feature_graphs(h);                               // and the captured step graphs hold their addresses
  poisson_solve_free(h);                                // psm_bind_poisson_solve stands on this binding
  FeatureSet& s = h->feat;
  feat_free(s);
  image_gone(h);
  const size_t npix = (size_t)h->Ny * h->Nx, nwg = (npix + 255) / 256, n = (size_t)n_cases;
  int rc;
  if ((rc = dev_alloc(h, &s.d_sdf, n * npix)) || (rc = dev_alloc(h, &s.d_term, n * npix)) || (rc = dev_alloc(h, &s.d_partial, n * 2 * nwg)) ||
      (rc = dev_alloc(h, &s.d_lu, n * 2)) || (rc = dev_alloc(h, &s.d_grid, n * npix * 4)) || (rc = dev_alloc(h, &s.d_vel, n * 4 * npix))) { feat_free(s); return rc; }
  // the host entry's pinned staging (velocities; dU, prev and the three outputs as psm_solve_poststeps): grown here, not in a step
  const size_t pb = n * npix * sizeof(float);
  if ((rc = scratch_reserve(h, 0, carve_size({n * 4 * npix * sizeof(double), pb, pb, pb * h->cfg.c_out + 2 * pb})))) { feat_free(s); return rc; }
  if ((rc = pin_alloc(h, &s.h_lu, FeatureSet::RING * n * 2, "psm_bind_features", PSM_ERR_HIP))) { feat_free(s); return rc; }
  hipError_t e = hipSuccess;
  for (auto& ev : s.lu_ev) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e == hipSuccess) e = psm_copy_h2d(s.d_sdf, sdfunct, n * npix * sizeof(double));
  // what psm_time_kernels reads as velocities and scalars is defined: zero planes, (L, U) = (1, 1)
  const std::vector<double> ones(n * 2, 1.0);
  if (e == hipSuccess) e = psm_copy_h2d(s.d_lu, ones.data(), ones.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemsetAsync(s.d_vel, 0, n * 4 * npix * sizeof(double), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { feat_free(s); return fail(h, PSM_ERR_HIP, std::string("psm_bind_features: ") + hipGetErrorString(e)); }
  s.n_cases = n_cases; s.k = k;
  for (int q = 0; q < 4; ++q) s.max_abs[q] = max_abs[q];
  s.ready = true;
  return PSM_OK;
}


int psm_unbind_features(psm_handle* h) {
  return unbind(h, [h] { drop_feature_graphs(h); poisson_solve_free(h); feat_free(h->feat); image_gone(h); });
}


int psm_features_device(psm_handle* h, const double* d_vel, int32_t n_cases, const double* LU, float* d_grid, void* stream) {
  if (!h) return PSM_ERR_ARG;
  int rc = feat_check(h, n_cases, LU);
  if (rc) return rc;
  if (!d_vel || !d_grid) return fail(h, PSM_ERR_ARG, "null buffer");
  if (reinterpret_cast<uintptr_t>(d_grid) & 15) return fail(h, PSM_ERR_ARG, "the image must be 16-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = stream_of(h, stream);
  if ((rc = upload_lu(h, LU, n_cases, st))) return rc;
  return features_device(h, d_vel, n_cases, d_grid, st);
}


int psm_poisson_step_device(psm_handle* h, const double* d_vel, int32_t n_cases, const double* LU, const float* out_scale,
                            int32_t apply_filter, const float* d_dU, const float* d_prev, float* d_result, float* d_change,
                            float* d_next, void* stream) {
  if (!h) return PSM_ERR_ARG;
  return poisson_step_device(h, d_vel, n_cases, LU, out_scale, post_call(apply_filter, d_dU, d_prev, d_result, d_change, d_next), (hipStream_t)stream);
}


int psm_poisson_step(psm_handle* h, const double* vel, int32_t n_cases, const double* LU, const float* out_scale, int32_t apply_filter,
                     const float* dU, const float* prev, float* result, float* change, float* next) {
  if (!h) return PSM_ERR_ARG;
  PostSet& s = h->post;
  const size_t cap = h->planned ? (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out : 0;
  const PostCall pc = post_call(apply_filter, dU ? s.d_dU : nullptr, dU ? s.d_prev : nullptr, s.d_out, (dU && change) ? s.d_out + cap : nullptr,
                                (dU && next) ? s.d_out + 2 * cap : nullptr);
  if (!vel || !result || (dU && !prev)) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = feat_check(h, n_cases, LU);
  if (rc) return rc;
  if (!s.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: a Poisson step needs it as well as psm_bind_features");
  if ((rc = post_check(h, n_cases, pc))) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t vb = (size_t)n_cases * 4 * npix * sizeof(double), pb = (size_t)n_cases * npix * sizeof(float), fb = pb * h->cfg.c_out;
  if ((rc = scratch_reserve(h, 0, carve_size({vb, pb, pb, fb + 2 * pb})))) return rc;
  Carver cp{(char*)h->scr_pin};
  double* p_vel = cp.take<double>(vb / 8);
  float* p_dU = cp.take<float>(pb / 4); float* p_prev = cp.take<float>(pb / 4);
  const PostOut out(pc, result, change, next, cp.take<float>((fb + 2 * pb) / 4), fb, pb);
  memcpy(p_vel, vel, vb);
  HIPCHK(h, hipMemcpyAsync(h->feat.d_vel, p_vel, vb, hipMemcpyHostToDevice, st));
  if (dU) {
    memcpy(p_dU, dU, pb); memcpy(p_prev, prev, pb);
    HIPCHK(h, hipMemcpyAsync(s.d_dU, p_dU, pb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(s.d_prev, p_prev, pb, hipMemcpyHostToDevice, st));
  }
  rc = guarded_host_step(h, st, "psm_poisson_step", [&](int) {
    const int rs = poisson_step_device(h, h->feat.d_vel, n_cases, LU, out_scale, pc, st);
    return rs ? rs : out.enqueue(h, st);
  });
  if (rc) return rc;
  out.deliver();
  return PSM_OK;
}

}  // extern "C"
