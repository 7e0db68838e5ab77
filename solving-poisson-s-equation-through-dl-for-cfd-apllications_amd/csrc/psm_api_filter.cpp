// psm_api_filter.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the Gaussian post-steps of assemble_prediction (SM_call.py:352-363,
// UGP:366-367) -- the host entry psm_gaussian_filter and the device-resident, case-batched entries behind psm_bind_poststeps.
// Kernels: psm_filter.hip.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// scipy.ndimage._gaussian_kernel1d, order 0: computed in double, normalised, rounded to float.  Returns the radius.
static int gauss_weights(double sigma, std::vector<float>& w) {
  const int r = (int)(4.0 * sigma + 0.5);
  std::vector<double> p(2 * r + 1);
  double sum = 0.0;
  for (int x = -r; x <= r; ++x) { p[x + r] = std::exp(-0.5 / (sigma * sigma) * (double)x * (double)x); sum += p[x + r]; }
  w.resize(2 * r + 1);
  for (int k = 0; k < 2 * r + 1; ++k) w[k] = (float)(p[k] / sum);
  return r;
}

static bool sigma_ok(double s) { return s > 0.0 && s <= 1e4; }

void post_free(PostSet& s) {
  dev_free(s.d_taps); dev_free(s.d_tmp_a); dev_free(s.d_tmp_b); dev_free(s.d_t); dev_free(s.d_fields); dev_free(s.d_dU); dev_free(s.d_prev); dev_free(s.d_out);
  s.ready = false;
}

// captured solve + post-step graphs (StepCall::post) hold the addresses of the binding's tables and scratch
static void drop_post_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.post.apply_filter >= 0; }); }

// axis 0 then axis 1 of ONE filter over [n][ny][nx][c]: in -> tmp -> out (in and out may alias)
static int filter_pair(psm_handle* h, const float* in, int n, int ny, int nx, int c, float* tmp, float* out, const float* wy, int ry,
                       const float* wx, int rx, hipStream_t st) {
  PsmGaussArgs a{};
  a.ny = ny; a.nx = nx; a.c = c; a.n_cases = n; a.n_jobs = 1;
  a.job[0] = PsmGaussJob{in, wy, ry}; a.out[0] = tmp; a.tap_chunk = psm_gauss_tap_chunk(ry);
  HIPCHK(h, psm_launch_gauss(a, 0, 0, st));
  a.job[0] = PsmGaussJob{tmp, wx, rx}; a.out[0] = out; a.tap_chunk = psm_gauss_tap_chunk(rx);
  HIPCHK(h, psm_launch_gauss(a, 1, 0, st));
  return PSM_OK;
}

// The post-steps of d_fields [n][Ny][Nx][c_out] on `st`: at most 4 launches with the weighting (pc.dU), at most 2 without.
int poststeps_device(psm_handle* h, const float* d_fields, int n, const PostCall& pc, hipStream_t st) {
  const PostSet& P = h->post;
  const int ny = h->Ny, nx = h->Nx, c = h->cfg.c_out;
  if (!pc.dU) {                                       // filter only
    if (pc.apply_filter) return filter_pair(h, d_fields, n, ny, nx, c, P.d_tmp_a, pc.result, P.w_field[0], P.r_field[0], P.w_field[1], P.r_field[1], st);
    if (pc.result != d_fields) HIPCHK(h, hipMemcpyAsync(pc.result, d_fields, (size_t)n * ny * nx * c * sizeof(float), hipMemcpyDeviceToDevice, st));
    return PSM_OK;
  }
  const bool af = pc.apply_filter != 0;
  PsmGaussArgs a{};
  a.ny = ny; a.nx = nx; a.c = 1; a.n_cases = n;
  // 1: axis 0 of the field (sigma_field) and of dU (sigma_weight), one launch
  const PsmGaussJob f0{d_fields, P.w_field[0], P.r_field[0]}, w0{pc.dU, P.w_weight[0], P.r_weight[0]};
  a.n_jobs = af ? 2 : 1;
  a.job[0] = af ? f0 : w0; a.out[0] = af ? P.d_tmp_a : P.d_tmp_b;
  a.job[1] = w0; a.out[1] = P.d_tmp_b;
  a.tap_chunk = psm_gauss_tap_chunk(af ? std::max(P.r_field[0], P.r_weight[0]) : P.r_weight[0]);
  HIPCHK(h, psm_launch_gauss(a, 0, 0, st));
  // 2: axis 1 of both; result and t = (result - prev) * w
  a.n_jobs = 2;
  a.job[0] = PsmGaussJob{af ? P.d_tmp_a : nullptr, P.w_field[1], P.r_field[1]};
  a.job[1] = PsmGaussJob{P.d_tmp_b, P.w_weight[1], P.r_weight[1]};
  a.out[0] = a.out[1] = nullptr;
  a.fields = d_fields; a.prev = pc.prev; a.t = P.d_t;
  a.result = (af || pc.result != d_fields) ? pc.result : nullptr;
  a.tap_chunk = psm_gauss_tap_chunk(af ? std::max(P.r_field[1], P.r_weight[1]) : P.r_weight[1]);
  HIPCHK(h, psm_launch_gauss(a, 1, 1, st));
  if (!pc.change && !pc.next) return PSM_OK;
  // 3, 4: the filter of t; change and next = prev + change
  a.n_jobs = 1;
  a.job[0] = PsmGaussJob{P.d_t, P.w_field[0], P.r_field[0]}; a.out[0] = P.d_tmp_a;
  a.tap_chunk = psm_gauss_tap_chunk(P.r_field[0]);
  HIPCHK(h, psm_launch_gauss(a, 0, 0, st));
  a.job[0] = PsmGaussJob{P.d_tmp_a, P.w_field[1], P.r_field[1]}; a.out[0] = nullptr;
  a.change = pc.change; a.next = pc.next;
  a.tap_chunk = psm_gauss_tap_chunk(P.r_field[1]);
  HIPCHK(h, psm_launch_gauss(a, 1, 2, st));
  return PSM_OK;
}

// state and argument checks shared by the device-resident entries
int post_check(psm_handle* h, int n_cases, const PostCall& pc) {
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called (a new plan or model drops the binding)");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  if (pc.dU && h->cfg.c_out != 1) return fail(h, PSM_ERR_STATE, "the deltaU-change weighting needs a one-channel field: c_out == 1");
  if (!pc.result || (pc.dU && !pc.prev)) return fail(h, PSM_ERR_ARG, "null buffer");
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_gaussian_filter(psm_handle* h, const float* in, int32_t ny, int32_t nx, double sigma_y, double sigma_x, float* out) {
  if (!h) return PSM_ERR_ARG;
  if (!in || !out || ny < 1 || nx < 1 || (int64_t)ny * nx > ((int64_t)1 << 28)) return fail(h, PSM_ERR_ARG, "bad field");
  if (!sigma_ok(sigma_y) || !sigma_ok(sigma_x)) return fail(h, PSM_ERR_ARG, "sigma must be positive");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  psm_gauss_init();
  hipStream_t st = h->stream;
  const size_t n = (size_t)ny * nx;
  std::vector<float> wy, wx;
  const int ry = gauss_weights(sigma_y, wy), rx = gauss_weights(sigma_x, wx);
  std::vector<float> wall(wy);
  wall.insert(wall.end(), wx.begin(), wx.end());
  const size_t nb = n * sizeof(float), wb = wall.size() * sizeof(float);
  int rc;
  if ((rc = scratch_reserve(h, carve_size({nb, nb, wb}), carve_size({nb, wb})))) return rc;
  Carver cd{(char*)h->scr_dev}, cp{(char*)h->scr_pin};
  float* d_a = cd.take<float>(n); float* d_b = cd.take<float>(n); float* d_w = cd.take<float>(wall.size());
  float* p_io = cp.take<float>(n); float* p_w = cp.take<float>(wall.size());
  memcpy(p_io, in, nb); memcpy(p_w, wall.data(), wb);
  HIPCHK(h, hipMemcpyAsync(d_a, p_io, nb, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(d_w, p_w, wb, hipMemcpyHostToDevice, st));
  if ((rc = filter_pair(h, d_a, 1, ny, nx, 1, d_b, d_a, d_w, ry, d_w + wy.size(), rx, st))) { (void)hipStreamSynchronize(st); return rc; }
  HIPCHK(h, hipMemcpyAsync(p_io, d_a, nb, hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(st));
  memcpy(out, p_io, nb);
  return PSM_OK;
}


int psm_bind_poststeps(psm_handle* h, const double* sigma_field, const double* sigma_weight) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!sigma_field || !sigma_weight) return fail(h, PSM_ERR_ARG, "null argument");
  for (int k = 0; k < 2; ++k)
    if (!sigma_ok(sigma_field[k]) || !sigma_ok(sigma_weight[k])) return fail(h, PSM_ERR_ARG, "sigma must be positive");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // post-steps in flight read the tables that are replaced,
  drop_post_graphs(h);                                  // and the captured solve + post-step graphs hold their addresses
  poisson_solve_free(h);                                // psm_bind_poisson_solve stands on this binding
  if (h->gsolve.apply_filter) gradp_solve_free(h);      // and so does psm_bind_gradp_solve* with apply_filter
  psm_gauss_init();
  PostSet& s = h->post;
  post_free(s);
  std::vector<float> all, w;
  size_t at[4];
  for (int k = 0; k < 4; ++k) {                         // field y, field x, weight y, weight x; each piece starts 16-byte aligned
    const int r = gauss_weights(k < 2 ? sigma_field[k] : sigma_weight[k - 2], w);
    (k < 2 ? s.r_field[k] : s.r_weight[k - 2]) = r;
    at[k] = all.size();
    all.insert(all.end(), w.begin(), w.end());
    all.resize((all.size() + 3) & ~(size_t)3, 0.f);
  }
  const size_t plane = (size_t)h->cfg.max_cases * h->Ny * h->Nx, c = (size_t)h->cfg.c_out;
  int rc;
  if ((rc = dev_upload(h, &s.d_taps, all)) || (rc = dev_alloc(h, &s.d_tmp_a, plane * c)) || (rc = dev_alloc(h, &s.d_tmp_b, plane)) ||
      (rc = dev_alloc(h, &s.d_t, plane)) || (rc = dev_alloc(h, &s.d_fields, plane * c)) || (rc = dev_alloc(h, &s.d_dU, plane)) ||
      (rc = dev_alloc(h, &s.d_prev, plane)) || (rc = dev_alloc(h, &s.d_out, plane * 3 * c))) { post_free(s); return rc; }
  // what psm_time_kernels reads as dU / prev is defined
  HIPCHK(h, hipMemsetAsync(s.d_dU, 0, plane * sizeof(float), h->stream));
  HIPCHK(h, hipMemsetAsync(s.d_prev, 0, plane * sizeof(float), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < 2; ++k) { s.w_field[k] = s.d_taps + at[k]; s.w_weight[k] = s.d_taps + at[2 + k]; }
  s.ready = true;
  return PSM_OK;
}


int psm_unbind_poststeps(psm_handle* h) {
  return unbind(h, [h] { drop_post_graphs(h); poisson_solve_free(h); if (h->gsolve.apply_filter) gradp_solve_free(h); post_free(h->post); });
}


int psm_filter_fields_device(psm_handle* h, const float* d_in, int32_t n_cases, float* d_out, void* stream) {
  if (!h) return PSM_ERR_ARG;
  PostCall pc;
  pc.apply_filter = 1; pc.result = d_out;
  int rc = post_check(h, n_cases, pc);
  if (rc) return rc;
  if (!d_in) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return poststeps_device(h, d_in, n_cases, pc, stream_of(h, stream));
}


int psm_poststeps_device(psm_handle* h, const float* d_fields, int32_t n_cases, int32_t apply_filter, const float* d_dU,
                         const float* d_prev, float* d_result, float* d_change, float* d_next, void* stream) {
  if (!h) return PSM_ERR_ARG;
  const PostCall pc = post_call(apply_filter, d_dU, d_prev, d_result, d_change, d_next);
  int rc = post_check(h, n_cases, pc);
  if (rc) return rc;
  if (!d_fields) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return poststeps_device(h, d_fields, n_cases, pc, stream_of(h, stream));
}


int psm_solve_poststeps_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale, int32_t apply_filter,
                               const float* d_dU, const float* d_prev, float* d_result, float* d_change, float* d_next, void* stream) {
  if (!h) return PSM_ERR_ARG;
  const PostCall pc = post_call(apply_filter, d_dU, d_prev, d_result, d_change, d_next);
  int rc = post_check(h, n_cases, pc);
  if (rc) return rc;
  if (!d_grid) return fail(h, PSM_ERR_ARG, "null buffer");
  // one graph replay: the solve's launches into the handle's field buffer + the post-steps' behind them
  StepCall step;
  step.post = pc;
  return solve_device(h, d_grid, n_cases, out_scale, h->post.d_fields, stream_of(h, stream), nullptr, step);
}


int psm_solve_poststeps(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, int32_t apply_filter, const float* dU,
                        const float* prev, float* result, float* change, float* next) {
  if (!h) return PSM_ERR_ARG;
  PostSet& s = h->post;
  const size_t cap = h->planned ? (size_t)h->cfg.max_cases * h->Ny * h->Nx * h->cfg.c_out : 0;
  PostCall pc;
  pc.apply_filter = apply_filter ? 1 : 0;
  pc.dU = dU ? s.d_dU : nullptr; pc.prev = dU ? s.d_prev : nullptr;
  pc.result = s.d_out; pc.change = (dU && change) ? s.d_out + cap : nullptr; pc.next = (dU && next) ? s.d_out + 2 * cap : nullptr;
  if (!grid || !result || (dU && !prev)) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = post_check(h, n_cases, pc);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)n_cases * npix * h->cfg.c_in * sizeof(float), pb = (size_t)n_cases * npix * sizeof(float), fb = pb * h->cfg.c_out;
  if ((rc = scratch_reserve(h, 0, carve_size({pb, pb, fb + 2 * pb})))) return rc;
  Carver cp{(char*)h->scr_pin};
  float* p_dU = cp.take<float>(pb / 4); float* p_prev = cp.take<float>(pb / 4);
  const PostOut out(pc, result, change, next, cp.take<float>((fb + 2 * pb) / 4), fb, pb);
  const bool reg_in = host_registered(h, grid, gin);
  if (!reg_in) memcpy(h->h_grid, grid, gin);
  HIPCHK(h, hipMemcpyAsync(h->d_grid_stage, reg_in ? grid : h->h_grid, gin, hipMemcpyHostToDevice, st));
  if (dU) {
    memcpy(p_dU, dU, pb); memcpy(p_prev, prev, pb);
    HIPCHK(h, hipMemcpyAsync(s.d_dU, p_dU, pb, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(s.d_prev, p_prev, pb, hipMemcpyHostToDevice, st));
  }
  StepCall step;
  step.post = pc;
  rc = guarded_host_step(h, st, "psm_solve_poststeps", [&](int) {
    const int rs = solve_device(h, h->d_grid_stage, n_cases, out_scale, s.d_fields, st, nullptr, step);
    return rs ? rs : out.enqueue(h, st);
  });
  if (rc) return rc;
  out.deliver();
  return PSM_OK;
}

}  // extern "C"
