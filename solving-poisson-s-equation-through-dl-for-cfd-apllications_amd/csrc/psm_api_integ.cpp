// psm_api_integ.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the U_to_gradP integration -- the host-side tables of a geometry,
// the evaluator's host entry (psm_set_integration, psm_integrate_gradp) and the device-resident, case-batched U -> p
// (psm_bind_integration, psm_integrate_gradp_device, psm_solve_pressure*).  Kernels: psm_integ.hip.
// See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// ---- U_to_gradP integration: host-side tables ----------------------------------------------------------------------
void integ_free(IntegSet& s) {
  dev_free(s.d_fix); dev_free(s.d_cuts); dev_free(s.d_npair); dev_free(s.d_mask); dev_free(s.d_aux); dev_free(s.d_gradp); dev_free(s.d_p);
  s.ready = false; s.n_cases = 0;
}

// Tables of ONE geometry: fix [ny][PSM_INTEG_MAX_FIX] (rows beyond the taller half stay unused), mask [ny], npair (top, bottom).
// Returns PSM_OK, or PSM_ERR_ARG / PSM_ERR_UNSUPPORTED with the reason in `why`.
static int integ_tables(int ny, int nx, const double* sdfunct, int cy, int cx, int2* fix, uint8_t* mask, int2* npair, std::string& why) {
  if (cy < 1 || cy >= ny || cx < 1 || cx >= nx) { why = "cut outside the grid"; return PSM_ERR_ARG; }
  const int wl = cx, wr = nx - cx + 1, hmax = std::max(cy, ny - cy);
  // "reset" quirk (Eval_dual_Dense_onlycil.py:394-396): nn = sdfunct[i,:].astype(int) indexes the block row
  for (int a = 0; a < hmax; ++a) {
    std::map<int, int> last;                       // index value -> last position
    std::vector<int> nn(nx);
    for (int k = 0; k < nx; ++k) {
      nn[k] = (int)sdfunct[(int64_t)a * nx + k];   // C truncation == astype(int) for finite values
      if (nn[k] < 0) nn[k] += std::min(wl, wr);    // negative indices wrap in NumPy; not expected for a distance
      last[nn[k]] = k;
    }
    if ((int)last.size() > PSM_INTEG_MAX_FIX) { why = "more distinct int(sdf) values on a row than supported"; return PSM_ERR_UNSUPPORTED; }
    int e = 0;
    for (auto& kv : last) {
      if (kv.first < 0 || kv.first >= std::min(wl, wr)) { why = "int(sdfunct) indexes outside a quadrant row (the reference raises IndexError)"; return PSM_ERR_UNSUPPORTED; }
      fix[(size_t)a * PSM_INTEG_MAX_FIX + e++] = make_int2(kv.first, kv.second > 0 ? nn[kv.second - 1] : -1);
    }
  }
  int np[2];
  for (int q = 0; q < 2; ++q) {
    const int r0 = q ? cy : 0, r1 = q ? ny : cy;
    int nl = 0, nr = 0;
    for (int y = r0; y < r1; ++y) {
      const bool l = sdfunct[(int64_t)y * nx + cx] != 0.0;        // mask2 / mask4 (column cx)
      const bool r = sdfunct[(int64_t)y * nx + cx - 1] != 0.0;    // mask1 / mask3 (column cx-1)
      mask[y] = (uint8_t)((l ? 1 : 0) | (r ? 2 : 0));
      nl += l; nr += r;
    }
    if (nl != nr) { why = "flow-cell counts of the two cut columns differ (the reference raises a broadcast error)"; return PSM_ERR_UNSUPPORTED; }
    np[q] = nl;
  }
  *npair = make_int2(np[0], np[1]);
  return PSM_OK;
}

// Build and upload the tables of n_cases geometries on a ny x nx grid into `s`; all-or-nothing: a geometry the reference cannot
// process leaves `s` as it was (the caller decides whether an earlier binding survives).  one_geometry: sdfunct [ny*nx], cy [1] and
// cx [1] describe ONE geometry, whose tables every case slot gets (psm_bind_gradp_frames: the frames of one simulation).
int integ_bind(psm_handle* h, IntegSet& s, int ny, int nx, const double* sdfunct, int n_cases, const int32_t* cy, const int32_t* cx,
               double dx, double dy, bool one_geometry) {
  const size_t npix = (size_t)ny * nx;
  if (npix * n_cases >= ((size_t)1 << 30)) return fail(h, PSM_ERR_ARG, "integration batch too large");
  std::vector<int2> fix((size_t)n_cases * ny * PSM_INTEG_MAX_FIX, make_int2(-1, -1)), cuts(n_cases), npair(n_cases);
  std::vector<uint8_t> mask((size_t)n_cases * ny, 0);
  for (int c = 0; c < n_cases; ++c) {
    std::string why;
    const int g = one_geometry ? 0 : c;
    const int rc = integ_tables(ny, nx, sdfunct + (size_t)g * npix, cy[g], cx[g], fix.data() + (size_t)c * ny * PSM_INTEG_MAX_FIX,
                                mask.data() + (size_t)c * ny, &npair[c], why);
    if (rc) return fail(h, rc, n_cases > 1 && !one_geometry ? "case " + std::to_string(c) + ": " + why : why);
    cuts[c] = make_int2(cy[g], cx[g]);
  }
  integ_free(s);
  int rc;
  if ((rc = dev_upload(h, &s.d_fix, fix)) || (rc = dev_upload(h, &s.d_cuts, cuts)) || (rc = dev_upload(h, &s.d_npair, npair)) ||
      (rc = dev_upload(h, &s.d_mask, mask)) || (rc = dev_alloc(h, &s.d_aux, (size_t)n_cases * ny)) ||
      (rc = dev_alloc(h, &s.d_gradp, (size_t)n_cases * npix * 2)) || (rc = dev_alloc(h, &s.d_p, (size_t)n_cases * npix))) { integ_free(s); return rc; }
  PsmIntegArgs& a = s.args;
  a.gradp = s.d_gradp; a.p = s.d_p; a.aux = s.d_aux; a.fixups = s.d_fix; a.cuts = s.d_cuts; a.rowmask = s.d_mask; a.npair = s.d_npair;
  a.ny = ny; a.nx = nx; a.n_cases = n_cases; a.dx = (float)dx; a.dy = (float)dy;
  s.n_cases = n_cases; s.ready = true;
  return PSM_OK;
}

// captured solve + integration graphs (StepCall::p) hold the addresses of the binding's tables
static void drop_pressure_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.p != nullptr; }); }

// state checks shared by the device-resident entries
static int integ_check(psm_handle* h, int n_cases) {
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (h->cfg.c_out != 2) return fail(h, PSM_ERR_STATE, "the integration needs a (dp/dx, dp/dy) field: c_out == 2");
  if (!h->integ_dev.ready) return fail(h, PSM_ERR_STATE, "psm_bind_integration has not been called (a new plan or model drops the binding)");
  if (n_cases != h->integ_dev.n_cases) return fail(h, PSM_ERR_STATE, "n_cases differs from the number of integration geometries bound");
  return PSM_OK;
}

// the two launches on `st`, from / into caller memory, with the tables of `s` (its first n_cases case slots)
int integrate_device(psm_handle* h, const IntegSet& s, const float* d_gradp, int n_cases, float* d_p, hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(d_gradp) & 7) || (reinterpret_cast<uintptr_t>(d_p) & 3)) return fail(h, PSM_ERR_ARG, "gradient buffer must be 8-byte aligned");
  PsmIntegArgs a = s.args;
  a.gradp = d_gradp; a.p = d_p; a.n_cases = n_cases;
  HIPCHK(h, psm_launch_integrate(a, st));
  return PSM_OK;
}

int integrate_device(psm_handle* h, const float* d_gradp, int n_cases, float* d_p, hipStream_t st) {
  return integrate_device(h, h->integ_dev, d_gradp, n_cases, d_p, st);
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_set_integration(psm_handle* h, int32_t ny, int32_t nx, const double* sdfunct, int32_t cy, int32_t cx, double dx, double dy) {
  if (!h) return PSM_ERR_ARG;
  if (!sdfunct || ny < 2 || nx < 3) return fail(h, PSM_ERR_ARG, "bad integration geometry");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return integ_bind(h, h->integ_host, ny, nx, sdfunct, 1, &cy, &cx, dx, dy);
}


int psm_integrate_gradp(psm_handle* h, const float* gradp, float* p_out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->integ_host.ready) return fail(h, PSM_ERR_STATE, "psm_set_integration has not been called");
  if (!gradp || !p_out) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const IntegSet& s = h->integ_host;
  const size_t n = (size_t)s.args.ny * s.args.nx;
  int rc;
  if ((rc = scratch_reserve(h, 0, carve_size({n * 2 * sizeof(float), n * sizeof(float)})))) return rc;
  Carver cp{(char*)h->scr_pin};
  float* p_g = cp.take<float>(n * 2); float* p_p = cp.take<float>(n);
  memcpy(p_g, gradp, n * 2 * sizeof(float));
  HIPCHK(h, hipMemcpyAsync(s.d_gradp, p_g, n * 2 * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(h, psm_launch_integrate(s.args, st));
  HIPCHK(h, hipMemcpyAsync(p_p, s.d_p, n * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(st));
  memcpy(p_out, p_p, n * sizeof(float));
  return PSM_OK;
}


int psm_bind_integration(psm_handle* h, const double* sdfunct, int32_t n_cases, const int32_t* center_y, const int32_t* center_x,
                         double dx, double dy) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (h->cfg.c_out != 2) return fail(h, PSM_ERR_STATE, "the integration needs a (dp/dx, dp/dy) field: c_out == 2");
  if (!sdfunct || !center_y || !center_x) return fail(h, PSM_ERR_ARG, "null argument");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // an integration in flight reads the tables that are replaced,
  drop_pressure_graphs(h);                              // and the captured solve + integration graphs hold their addresses
  const int rc = integ_bind(h, h->integ_dev, h->Ny, h->Nx, sdfunct, n_cases, center_y, center_x, dx, dy);
  if (rc) integ_free(h->integ_dev);                     // nothing stays bound
  return rc;
}


int psm_unbind_integration(psm_handle* h) {
  return unbind(h, [h] { drop_pressure_graphs(h); integ_free(h->integ_dev); });
}


int psm_integrate_gradp_device(psm_handle* h, const float* d_gradp, int32_t n_cases, float* d_p, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!d_gradp || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = integ_check(h, n_cases);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return integrate_device(h, d_gradp, n_cases, d_p, stream_of(h, stream));
}


int psm_solve_pressure_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale, float* d_gradp,
                              float* d_p, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!d_grid || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = integ_check(h, n_cases);
  if (rc) return rc;
  float* g = d_gradp ? d_gradp : h->integ_dev.d_gradp;
  if ((reinterpret_cast<uintptr_t>(g) & 7) || (reinterpret_cast<uintptr_t>(d_p) & 3)) return fail(h, PSM_ERR_ARG, "gradient buffer must be 8-byte aligned");
  StepCall step;
  step.p = d_p;
  return solve_device(h, d_grid, n_cases, out_scale, g, stream_of(h, stream), nullptr, step);   // one graph replay: the solve's launches + the two of the integration
}


int psm_solve_pressure(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, float* p) {
  if (!h) return PSM_ERR_ARG;
  if (!grid || !p) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = integ_check(h, n_cases);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)n_cases * npix * h->cfg.c_in * sizeof(float), pout = (size_t)n_cases * npix * sizeof(float);
  const bool reg_in = host_registered(h, grid, gin), reg_out = host_registered(h, p, pout);
  IntegSet& s = h->integ_dev;
  if (!reg_in) memcpy(h->h_grid, grid, gin);
  HIPCHK(h, hipMemcpyAsync(h->d_grid_stage, reg_in ? grid : h->h_grid, gin, hipMemcpyHostToDevice, h->stream));
  StepCall step;
  step.p = s.d_p;
  rc = guarded_host_step(h, h->stream, "psm_solve_pressure", [&](int) {
    const int rs = solve_device(h, h->d_grid_stage, n_cases, out_scale, s.d_gradp, h->stream, nullptr, step);
    if (rs) return rs;
    HIPCHK(h, hipMemcpyAsync(reg_out ? p : h->h_fields, s.d_p, pout, hipMemcpyDeviceToHost, h->stream));
    return PSM_OK;
  });
  if (rc) return rc;
  if (!reg_out) memcpy(p, h->h_fields, pout);
  return PSM_OK;
}

}  // extern "C"
