// psm_api_mesh.cpp -- C-ABI of libpsm_hip.so (include/psm.h): solver boundary (mesh <-> grid) and evaluator helpers.  See psm_handle.h for the map of the files.
#include "psm_handle.h"
#include "psm_mesh_tables.h"

namespace psm_impl {

// psm_solve on registered, mapped caller buffers: every device-side step of the call, in stream order (captured once)
static int mesh_sequence(psm_handle* h, int64_t n, hipStream_t st) {
  int n_partials = 0;
  HIPCHK(h, psm_launch_stage_cells(h->pinned_cells_dev, h->d_cells, n, h->d_umax_part, &n_partials, st));
  PsmToGridArgs ga{};
  ga.cells = h->d_cells; ga.umax = nullptr; ga.umax_val = 0.0;
  ga.umax_partials = h->d_umax_part; ga.n_partials = n_partials; ga.umax_out = h->d_umax;
  ga.vtx = h->d_vtx_m2g; ga.wts = h->d_wts_m2g; ga.src_of_cell = h->d_src_of_cell;
  ga.sdf = h->d_sdf; ga.grid = h->d_grid_stage; ga.n_grid = (int64_t)h->Ny * h->Nx;
  ga.max_abs_ux = h->maxs[0]; ga.max_abs_uy = h->maxs[1]; ga.sdf_scale = h->normalise_sdf ? 1.0 / h->maxs[2] : 1.0;
  ga.c_in = h->cfg.c_in; ga.fill = h->fill_input;
  HIPCHK(h, psm_launch_to_grid(ga, st));
  h->in_mesh_solve = true;
  int rc = launch_all(h, h->ws0, h->d_grid_stage, 1, h->d_fields_stage, h->d_ones, st, nullptr);
  h->in_mesh_solve = false;
  if (rc) return rc;
  PsmToMeshArgs ma{};
  ma.cells = h->d_cells; ma.umax = h->d_umax; ma.umax_val = 0.0; ma.vtx = h->d_vtx_g2m; ma.wts = h->d_wts_g2m; ma.cell_of_point = h->d_cell_of_point;
  ma.field = h->d_fields_stage; ma.near_wall = h->d_near_wall; ma.p_out = h->pinned_p_dev; ma.n_cells = n; ma.max_abs_p = h->maxs[3];
  ma.c_out = h->cfg.c_out;
  HIPCHK(h, psm_launch_to_mesh(ma, st));
  return PSM_OK;
}

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
// process leaves `s` as it was (the caller decides whether an earlier binding survives).
static int integ_bind(psm_handle* h, IntegSet& s, int ny, int nx, const double* sdfunct, int n_cases, const int32_t* cy, const int32_t* cx,
                      double dx, double dy) {
  const size_t npix = (size_t)ny * nx;
  if (npix * n_cases >= ((size_t)1 << 30)) return fail(h, PSM_ERR_ARG, "integration batch too large");
  std::vector<int2> fix((size_t)n_cases * ny * PSM_INTEG_MAX_FIX, make_int2(-1, -1)), cuts(n_cases), npair(n_cases);
  std::vector<uint8_t> mask((size_t)n_cases * ny, 0);
  for (int c = 0; c < n_cases; ++c) {
    std::string why;
    const int rc = integ_tables(ny, nx, sdfunct + (size_t)c * npix, cy[c], cx[c], fix.data() + (size_t)c * ny * PSM_INTEG_MAX_FIX,
                                mask.data() + (size_t)c * ny, &npair[c], why);
    if (rc) return fail(h, rc, n_cases > 1 ? "case " + std::to_string(c) + ": " + why : why);
    cuts[c] = make_int2(cy[c], cx[c]);
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

// captured solve + integration graphs (GraphKey::p) hold the addresses of the binding's tables
static void drop_pressure_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.p != nullptr; }); }

// state checks shared by the device-resident entries
static int integ_check(psm_handle* h, int n_cases) {
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (h->cfg.c_out != 2) return fail(h, PSM_ERR_STATE, "the integration needs a (dp/dx, dp/dy) field: c_out == 2");
  if (!h->integ_dev.ready) return fail(h, PSM_ERR_STATE, "psm_bind_integration has not been called (a new plan or model drops the binding)");
  if (n_cases != h->integ_dev.n_cases) return fail(h, PSM_ERR_STATE, "n_cases differs from the number of integration geometries bound");
  return PSM_OK;
}

// the two launches on `st`, from / into caller memory
int integrate_device(psm_handle* h, const float* d_gradp, int n_cases, float* d_p, hipStream_t st) {
  if ((reinterpret_cast<uintptr_t>(d_gradp) & 7) || (reinterpret_cast<uintptr_t>(d_p) & 3)) return fail(h, PSM_ERR_ARG, "gradient buffer must be 8-byte aligned");
  PsmIntegArgs a = h->integ_dev.args;
  a.gradp = d_gradp; a.p = d_p; a.n_cases = n_cases;
  HIPCHK(h, psm_launch_integrate(a, st));
  return PSM_OK;
}

// ---- the case set of psm_set_geometry_cases -----------------------------------------------------------------------
// state checks shared by the step entries
static int cases_check(psm_handle* h) {
  if (h->have_geometry && !h->mcs.ready)
    return fail(h, PSM_ERR_STATE, "the handle holds the single mesh of psm_set_geometry: psm_solve_cases* needs a case set (psm_set_geometry_cases)");
  if (!h->mcs.ready || !h->planned)
    return fail(h, PSM_ERR_STATE, "psm_set_geometry_cases has not been called (or its case set was dropped by a later psm_set_* / psm_plan_grid)");
  return PSM_OK;
}

// One step of the case set, a linear chain on `st`: U_max partials, to_grid, the batched solve, to_mesh.  Plain launches (like
// psm_solve; the solve inside replays its graph under PSM_GRAPH=1); copies nothing.
static int cases_sequence(psm_handle* h, const double* d_cells, double* d_p, hipStream_t st) {
  PsmMeshCasesArgs a = h->mcs.args;
  a.cells = d_cells; a.p_out = d_p;
  HIPCHK(h, psm_launch_umax_cases(a, st));
  HIPCHK(h, psm_launch_to_grid_cases(a, st));
  h->in_mesh_solve = true;
  const int rc = solve_device(h, h->d_grid_stage, h->mcs.n_cases, nullptr, h->d_fields_stage, st, nullptr);
  h->in_mesh_solve = false;
  if (rc) return rc;
  HIPCHK(h, psm_launch_to_mesh_cases(a, st));
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_reassemble(psm_handle* h, const float* grid, const float* block_pred, float* fields) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!grid || !block_pred || !fields) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx;
  HIPCHK(h, hipStreamSynchronize(st));                    // the staging buffers are free; caller memory goes through the bounce buffer
  HIPCHK(h, psm_copy_h2d(h->d_grid_stage, grid, npix * h->cfg.c_in * sizeof(float)));
  HIPCHK(h, psm_copy_h2d(h->ws0.d_pred, block_pred, (size_t)h->B * h->K_out * sizeof(float)));
  HIPCHK(h, psm_launch_strips(strip_args(h, h->ws0, h->d_grid_stage), 1, st));
  HIPCHK(h, psm_launch_chain(chain_args(h, h->ws0), 1, st));
  HIPCHK(h, psm_launch_paste(paste_args(h, h->ws0, h->d_fields_stage), 1, st));
  HIPCHK(h, wait_stream(st));
  HIPCHK(h, psm_copy_d2h(fields, h->d_fields_stage, npix * h->cfg.c_out * sizeof(float)));
  h->last_cases = 1;
  return PSM_OK;
}


int psm_label_blocks(psm_handle* h, const float* grid, const float* labels, float* blocks_out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!grid || !labels || !blocks_out) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gb = npix * h->cfg.c_in * sizeof(float), lb = npix * h->cfg.c_out * sizeof(float), ob = (size_t)h->B * h->K_out * sizeof(float);
  int rc;
  if ((rc = scratch_reserve(h, carve_size({gb, lb, ob}), carve_size({gb, lb, ob})))) return rc;
  Carver cd{(char*)h->scr_dev}, cp{(char*)h->scr_pin};
  float* d_g = cd.take<float>(npix * h->cfg.c_in); float* d_l = cd.take<float>(npix * h->cfg.c_out); float* d_o = cd.take<float>((size_t)h->B * h->K_out);
  float* p_g = cp.take<float>(npix * h->cfg.c_in); float* p_l = cp.take<float>(npix * h->cfg.c_out); float* p_o = cp.take<float>((size_t)h->B * h->K_out);
  memcpy(p_g, grid, gb); memcpy(p_l, labels, lb);
  hipError_t e = hipMemcpyAsync(d_g, p_g, gb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_l, p_l, lb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = psm_launch_label_blocks(d_g, d_l, h->d_blk, d_o, h->B, h->S, h->cfg.c_in, h->cfg.c_out, h->cfg.sdf_channel, h->Nx, st);
  if (e == hipSuccess) e = hipMemcpyAsync(p_o, d_o, ob, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = wait_stream(st);
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string("label blocks: ") + hipGetErrorString(e));
  memcpy(blocks_out, p_o, ob);
  return PSM_OK;
}


int psm_block_error(psm_handle* h, const float* grid, const float* labels, double* out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned || h->last_cases < 1) return fail(h, PSM_ERR_STATE, "no solve has run yet");
  // The network output it decodes lives in the handle's own workspace.  A solve through the asynchronous ring
  // (psm_submit_grid*, psm_ring_*, psm_bench_host) ran on a ring slot's workspace and left an OLDER solve here.
  if (!h->last.on_ws0)
    return fail(h, PSM_ERR_STATE, "psm_block_error follows a synchronous solve (psm_solve_grid / psm_solve_grid_device / psm_solve); the last solve ran on the ring");
  if (!grid || !labels || !out) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipDeviceSynchronize());                        // the solve may have run on the caller's stream
  hipStream_t st = h->stream;
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gb = npix * h->cfg.c_in * sizeof(float), lb = npix * h->cfg.c_out * sizeof(float), ob = (size_t)h->B * h->K_out * sizeof(float);
  const size_t pb = (size_t)h->B * 8 * sizeof(double);
  int rc;
  if ((rc = scratch_reserve(h, carve_size({gb, lb, ob, pb}), carve_size({gb, lb, pb})))) return rc;
  Carver cd{(char*)h->scr_dev}, cp{(char*)h->scr_pin};
  float* d_g = cd.take<float>(npix * h->cfg.c_in); float* d_l = cd.take<float>(npix * h->cfg.c_out); float* d_o = cd.take<float>((size_t)h->B * h->K_out);
  double* d_p = cd.take<double>((size_t)h->B * 8);
  float* p_g = cp.take<float>(npix * h->cfg.c_in); float* p_l = cp.take<float>(npix * h->cfg.c_out); double* p_p = cp.take<double>((size_t)h->B * 8);
  memcpy(p_g, grid, gb); memcpy(p_l, labels, lb);
  // the decoded blocks of the last solve (case 0): on the geometry-bound path they were never stored -- decode its network output again
  const float* scale = h->last.row_scale ? h->last.row_scale : h->d_ones;
  const PsmDecodeArgs de = decode_args(h, h->ws0, 1, scale, h->ws0.d_pred);
  const bool bf16 = h->cfg.precision == PSM_PRECISION_BF16;
  hipError_t e = bf16 ? psm_launch_decode_bf16(de, st) : psm_launch_decode(de, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_g, p_g, gb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_l, p_l, lb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = psm_launch_label_blocks(d_g, d_l, h->d_blk, d_o, h->B, h->S, h->cfg.c_in, h->cfg.c_out, h->cfg.sdf_channel, h->Nx, st);
  if (e == hipSuccess) e = psm_launch_block_error(d_g, h->ws0.d_pred, d_o, scale, h->d_blk, d_p, h->B, h->S, h->cfg.c_in, h->cfg.c_out, h->cfg.sdf_channel, h->Nx, st);
  if (e == hipSuccess) e = hipMemcpyAsync(p_p, d_p, pb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = wait_stream(st);
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string("block error: ") + hipGetErrorString(e));
  double n = 0, s1 = 0, s2 = 0, tmin = INFINITY, tmax = -INFINITY, pmin = INFINITY, pmax = -INFINITY, tnan = 0;
  for (int b = 0; b < h->B; ++b) {
    const double* q = p_p + (size_t)b * 8;
    n += q[0]; s1 += q[1]; s2 += q[2]; tnan += q[7];
    tmin = std::min(tmin, q[3]); tmax = std::max(tmax, q[4]); pmin = std::min(pmin, q[5]); pmax = std::max(pmax, q[6]);
  }
  const double norm = tnan > 0 ? NAN : tmax - tmin;        // np.max / np.min propagate a NaN label
  out[0] = s1 / n / norm;                                   // pred_minus_true_block (utils.py:241)
  out[1] = s2 / n / (norm * norm);                          // pred_minus_true_squared_block (utils.py:242)
  out[2] = norm; out[3] = pmax - pmin; out[4] = n;
  return PSM_OK;
}


int psm_set_geometry(psm_handle* h, int64_t n_cells, int32_t ny, int32_t nx, const int32_t* vtx_m2g, const double* wts_m2g,
                     const int32_t* indices, const double* sdfunct, const int32_t* vtx_g2m, const double* wts_g2m,
                     const double* maxs, int32_t normalise_sdf, int32_t fill_input, double wall_threshold) {
  if (!h) return PSM_ERR_ARG;
  if (!vtx_m2g || !wts_m2g || !indices || !sdfunct || !maxs) return fail(h, PSM_ERR_ARG, "null geometry table");
  if ((vtx_g2m == nullptr) != (wts_g2m == nullptr)) return fail(h, PSM_ERR_ARG, "vtx_g2m and wts_g2m go together");
  const bool g2m = vtx_g2m != nullptr;
  if (n_cells < 1 || n_cells > (int64_t)1 << 30) return fail(h, PSM_ERR_ARG, "bad cell count");
  const int64_t ng = (int64_t)ny * nx;
  for (int64_t t = 0; t < ng; ++t) {
    for (int j = 0; j < 3; ++j)
      if (vtx_m2g[t * 3 + j] < 0 || vtx_m2g[t * 3 + j] >= n_cells) return fail(h, PSM_ERR_ARG, "mesh->grid vertex index out of range");
    if (indices[t * 2] < 0 || indices[t * 2] >= ny || indices[t * 2 + 1] < 0 || indices[t * 2 + 1] >= nx)
      return fail(h, PSM_ERR_ARG, "indices outside the grid");
  }
  for (int64_t n = 0; g2m && n < n_cells; ++n)
    for (int j = 0; j < 3; ++j)
      if (vtx_g2m[n * 3 + j] < 0 || vtx_g2m[n * 3 + j] >= ng) return fail(h, PSM_ERR_ARG, "grid->mesh vertex index out of range");
  int rc = psm_plan_grid(h, ny, nx);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  free_geometry(h);
  h->n_cells = n_cells;
  for (int k = 0; k < 4; ++k) h->maxs[k] = maxs[k];
  h->normalise_sdf = normalise_sdf; h->fill_input = fill_input;
  // NumPy fancy assignment grid[...][tuple(indices.T)] = values writes in point order: last wins
  std::vector<int32_t> src(ng, -1), cop(ng);
  for (int64_t t = 0; t < ng; ++t) {
    const int64_t cell = (int64_t)indices[t * 2] * nx + indices[t * 2 + 1];
    src[cell] = (int32_t)t;
    cop[t] = (int32_t)cell;
  }
  // sdf_mesh = interpolate_fill(sdfunct.flatten(), vert_NPtoOF, weights_NPtoOF) < threshold  (PM:492-494)
  std::vector<uint8_t> nw(n_cells, 0);
  for (int64_t n = 0; g2m && n < n_cells; ++n) {
    double acc = 0.0; bool neg = false;
    for (int j = 0; j < 3; ++j) { acc += sdfunct[vtx_g2m[n * 3 + j]] * wts_g2m[n * 3 + j]; neg = neg || wts_g2m[n * 3 + j] < 0.0; }
    nw[n] = (!neg && acc < wall_threshold) ? 1 : 0;     // NaN (fill) compares false
  }
  std::vector<int32_t> v1(vtx_m2g, vtx_m2g + ng * 3), v2;
  std::vector<double> w1(wts_m2g, wts_m2g + ng * 3), w2, sd(sdfunct, sdfunct + ng);
  if (g2m) { v2.assign(vtx_g2m, vtx_g2m + n_cells * 3); w2.assign(wts_g2m, wts_g2m + n_cells * 3); }
  else { v2.assign((size_t)n_cells * 3, 0); w2.assign((size_t)n_cells * 3, 0.0); }
  h->have_g2m = g2m;
  if ((rc = dev_upload(h, &h->d_vtx_m2g, v1))) return rc;
  if ((rc = dev_upload(h, &h->d_wts_m2g, w1))) return rc;
  if ((rc = dev_upload(h, &h->d_src_of_cell, src))) return rc;
  if ((rc = dev_upload(h, &h->d_cell_of_point, cop))) return rc;
  if ((rc = dev_upload(h, &h->d_sdf, sd))) return rc;
  if ((rc = dev_upload(h, &h->d_vtx_g2m, v2))) return rc;
  if ((rc = dev_upload(h, &h->d_wts_g2m, w2))) return rc;
  if ((rc = dev_upload(h, &h->d_near_wall, nw))) return rc;
  if ((rc = dev_alloc(h, &h->d_cells, (size_t)n_cells * 5))) return rc;
  if ((rc = dev_alloc(h, &h->d_p, (size_t)n_cells))) return rc;
  if ((rc = dev_alloc(h, &h->d_umax, (size_t)1))) return rc;
  if ((rc = dev_alloc(h, &h->d_umax_part, (size_t)256))) return rc;
  HIPCHK(h, hipHostMalloc((void**)&h->h_cells, (size_t)n_cells * 5 * sizeof(double), hipHostMallocDefault));
  HIPCHK(h, hipHostMalloc((void**)&h->h_p, (size_t)n_cells * sizeof(double), hipHostMallocDefault));
  h->have_geometry = true;
  // The mesh entry builds its grid from THIS sdfunct at every step, so the geometry of psm_solve is fixed from here
  // on: bind it (scope: psm_solve only -- grid-native solves on the same handle stay general until psm_bind_geometry).
  if (h->cfg.c_in == 3 && h->cfg.sdf_channel == 2 && g2m && getenv("PSM_NO_BIND") == nullptr) {
    std::vector<float> g((size_t)ng * 3, 0.f);
    const double sc = normalise_sdf ? 1.0 / maxs[2] : 1.0;
    for (int64_t t = 0; t < ng; ++t) {
      const double sdv = sdfunct[t] * sc;                    // the SDF channel exactly as psm_to_grid_kernel writes it
      g[(size_t)t * 3 + 2] = (sdv != sdv) ? 0.f : (float)sdv;
    }
    HIPCHK(h, psm_copy_h2d(h->d_grid_stage, g.data(), g.size() * sizeof(float)));
    h->bound_scope = 1;                                      // before the bind: this scope builds no SDF-fold tables
    rc = bind_geometry_device(h, h->d_grid_stage);
    if (rc == PSM_OK) h->bound_scope = 1;
    else if (rc == PSM_ERR_UNSUPPORTED) h->err.clear();      // configuration outside the fused path: general path
    else return rc;
  }
  return PSM_OK;
}


int psm_set_case(psm_handle* h, const double* maxs, double delta, int32_t every, double wall_threshold) {
  if (!h) return PSM_ERR_ARG;
  if (!maxs || !(delta > 0.0) || every < 1 || !(wall_threshold >= 0.0)) return fail(h, PSM_ERR_ARG, "bad case constants");
  for (int k = 0; k < 4; ++k) {
    if (!(maxs[k] != 0.0)) return fail(h, PSM_ERR_ARG, "maxs must be non-zero");
    h->case_maxs[k] = maxs[k];
  }
  h->case_delta = delta; h->case_every = every; h->case_wall = wall_threshold;
  return PSM_OK;
}


int psm_init_geometry(psm_handle* h, const double* cells, int64_t n, const double* top, int64_t n_top, const double* obst,
                      int64_t n_obst, int32_t rank) {
  (void)rank;
  if (!h) return PSM_ERR_ARG;
  if (!cells || !top || !obst) return fail(h, PSM_ERR_ARG, "null buffer");
  int32_t ny = 0, nx = 0;
  if (psm_geometry_shape(cells, n, h->case_delta, &ny, &nx, nullptr) != PSM_OK) return fail(h, PSM_ERR_ARG, psm_geometry_last_error());
  const size_t ng = (size_t)ny * nx;
  std::vector<int32_t> v1(ng * 3), idx(ng * 2), v2((size_t)n * 3);
  std::vector<double> w1(ng * 3), sdf(ng), w2((size_t)n * 3);
  int rc = psm_geometry_build(cells, n, top, n_top, obst, n_obst, h->case_delta, h->case_every, v1.data(), w1.data(), idx.data(),
                              sdf.data(), v2.data(), w2.data());
  if (rc) return fail(h, rc, psm_geometry_last_error());
  return psm_set_geometry(h, n, ny, nx, v1.data(), w1.data(), idx.data(), sdf.data(), v2.data(), w2.data(), h->case_maxs, 0, 0, h->case_wall);
}


int psm_solve_begin(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  (void)rank;
  if (!h) return PSM_ERR_ARG;
  if (h->mesh_inflight) return fail(h, PSM_ERR_STATE, "a psm_solve_begin is already in flight on this handle: call psm_solve_end first");
  if (h->mcs.ready) return fail(h, PSM_ERR_STATE, "the handle holds the case set of psm_set_geometry_cases: psm_solve needs the single mesh of psm_set_geometry (use psm_solve_cases*)");
  if (!h->have_geometry || !h->planned)
    return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (or the plan it belonged to was dropped by a later psm_set_* / psm_plan_grid)");
  if (h->cfg.c_in != 3 || h->cfg.c_out != 1) return fail(h, PSM_ERR_UNSUPPORTED, "the mesh entry needs c_in == 3 and c_out == 1 (python_module.py:288-292)");
  if (!h->have_g2m) return fail(h, PSM_ERR_STATE, "psm_set_geometry was called without the grid->mesh tables");
  if (!cells || !p_out) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n != h->n_cells) return fail(h, PSM_ERR_ARG, "cell count differs from the geometry");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  { int rc0 = ensure_encode_aux(h, 1); if (rc0) return rc0; }   // many-block cases (the shipped 104-block shape): the M-tiled encode's split basis, once, outside any capture
  // Both arrays registered (psm_pin_buffers) and mapped: the whole call is ONE hipGraph replay -- psm_stage_cells_kernel reads
  // the cells over PCIe and takes the partial maxima of U_max on the way (no DMA-engine copy, no host pass, U_max never leaves
  // the device: to_grid reduces the partials and hands the scalar to to_mesh through d_umax), to_grid, the kernels of the
  // solve, to_mesh storing p straight into the caller's array.
  // PSM_MESH_GRAPH: 0 = the separate submissions below (DMA copy, host U_max), 1 = one graph replay, 2 = the same sequence as
  // plain launches (measured default)
  static const int mesh_mode = getenv("PSM_MESH_GRAPH") ? atoi(getenv("PSM_MESH_GRAPH")) : 2;
  static const int64_t stage_max = getenv("PSM_MESH_STAGE_MAX") ? atoll(getenv("PSM_MESH_STAGE_MAX")) : PSM_MESH_STAGE_MAX_DEFAULT;
  if (mesh_mode != 0 && h->timed_kernel < 0 && n <= stage_max && cells == h->pinned_cells && h->pinned_cells_dev && p_out == h->pinned_p && h->pinned_p_dev) {
    h->last_cases = 1;
    if (mesh_mode == 2) {
      int rc = mesh_sequence(h, n, st);
      if (rc) return rc;
    } else {
      if (!h->mesh_graph) {
        int rc = capture_graph(h, st, "psm_solve", [&] { return mesh_sequence(h, n, st); }, &h->mesh_graph);
        if (rc) return rc;
        h->mesh_graph_left = h->last;
      } else {
        h->last = h->mesh_graph_left;
      }
      HIPCHK(h, hipGraphLaunch(h->mesh_graph, st));
    }
    h->mesh_copy_out = nullptr;
    h->mesh_inflight = true;
    return PSM_OK;
  }
  if (cells == h->pinned_cells) {            // registered by the caller: DMA straight from its buffer
    HIPCHK(h, hipMemcpyAsync(h->d_cells, cells, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice, st));
  } else {
    memcpy(h->h_cells, cells, (size_t)n * 5 * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(h->d_cells, h->h_cells, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice, st));
  }
  // U_max = max sqrt(Ux^2 + Uy^2) (PM:270) on the host while the copy above is in flight: sqrt is monotonic and
  // correctly rounded on both sides, so sqrt(max(Ux^2 + Uy^2)) is the kernel's value bit for bit (NaN propagates
  // like np.max); one launch less.  PSM_DEVICE_UMAX=1 keeps the device reduction.
  // Large meshes (the host pass would take longer than the copy it hides under): parallel device reduction, whose
  // per-workgroup maxima every psm_to_grid workgroup folds itself.
  static const bool dev_umax_env = getenv("PSM_DEVICE_UMAX") != nullptr;
  const bool big = n > 32768;
  const bool dev_umax = dev_umax_env && !big;
  double umax_val = 0.0;
  int n_partials = 0;
  if (big) {
    HIPCHK(h, psm_launch_umax_partial(h->d_cells, n, h->d_umax_part, &n_partials, st));
  } else if (dev_umax) {
    HIPCHK(h, psm_launch_umax(h->d_cells, n, h->d_umax, st));
  } else {
    double m2 = 0.0; bool nan = false;
    for (int64_t i = 0; i < n; ++i) {
      const double ux = cells[i * 5], uy = cells[i * 5 + 1];
      const double v = ux * ux + uy * uy;
      nan = nan || (v != v);
      m2 = v > m2 ? v : m2;
    }
    umax_val = nan ? std::nan("") : std::sqrt(m2);
  }
  PsmToGridArgs ga{};
  ga.cells = h->d_cells; ga.umax = dev_umax ? h->d_umax : nullptr; ga.umax_val = umax_val;
  if (big) { ga.umax_partials = h->d_umax_part; ga.n_partials = n_partials; ga.umax_out = h->d_umax; } ga.vtx = h->d_vtx_m2g; ga.wts = h->d_wts_m2g; ga.src_of_cell = h->d_src_of_cell;
  ga.sdf = h->d_sdf; ga.grid = h->d_grid_stage; ga.n_grid = (int64_t)h->Ny * h->Nx;
  ga.max_abs_ux = h->maxs[0]; ga.max_abs_uy = h->maxs[1]; ga.sdf_scale = h->normalise_sdf ? 1.0 / h->maxs[2] : 1.0;
  ga.c_in = h->cfg.c_in; ga.fill = h->fill_input;
  HIPCHK(h, psm_launch_to_grid(ga, st));
  h->in_mesh_solve = true;
  int rc = solve_device(h, h->d_grid_stage, 1, nullptr, h->d_fields_stage, st, nullptr);
  h->in_mesh_solve = false;
  if (rc) return rc;
  PsmToMeshArgs ma{};
  ma.cells = h->d_cells; ma.umax = (dev_umax || big) ? h->d_umax : nullptr; ma.umax_val = umax_val; ma.vtx = h->d_vtx_g2m; ma.wts = h->d_wts_g2m; ma.cell_of_point = h->d_cell_of_point;
  ma.field = h->d_fields_stage; ma.near_wall = h->d_near_wall; ma.p_out = h->d_p; ma.n_cells = n; ma.max_abs_p = h->maxs[3];
  ma.c_out = h->cfg.c_out;
  const bool direct = p_out == h->pinned_p && h->pinned_p_dev != nullptr;
  if (direct) ma.p_out = h->pinned_p_dev;                 // 8 bytes per cell over PCIe from the kernel itself: no D2H copy
  HIPCHK(h, psm_launch_to_mesh(ma, st));
  if (p_out == h->pinned_p) {
    if (!direct) HIPCHK(h, hipMemcpyAsync(p_out, h->d_p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    h->mesh_copy_out = nullptr;
  } else {
    HIPCHK(h, hipMemcpyAsync(h->h_p, h->d_p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    h->mesh_copy_out = p_out;
  }
  h->mesh_inflight = true;
  return PSM_OK;
}


int psm_solve_end(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  if (!h->mesh_inflight) return fail(h, PSM_ERR_STATE, "no psm_solve_begin in flight");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  h->mesh_inflight = false;
  HIPCHK(h, wait_stream(h->stream));
  if (h->mesh_copy_out) memcpy(h->mesh_copy_out, h->h_p, (size_t)h->n_cells * sizeof(double));
  return PSM_OK;
}


int psm_solve(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  int rc = psm_solve_begin(h, cells, n, rank, p_out);
  return rc ? rc : psm_solve_end(h);
}


int psm_set_geometry_cases(psm_handle* h, int32_t n_cases, const int64_t* n_cells, int32_t ny, int32_t nx,
                           const int32_t* const* vtx_m2g, const double* const* wts_m2g, const int32_t* const* indices,
                           const double* const* sdfunct, const int32_t* const* vtx_g2m, const double* const* wts_g2m,
                           const double* maxs, int32_t normalise_sdf, int32_t fill_input, double wall_threshold) {
  if (!h) return PSM_ERR_ARG;
  if (!n_cells || !vtx_m2g || !wts_m2g || !indices || !sdfunct || !vtx_g2m || !wts_g2m || !maxs) return fail(h, PSM_ERR_ARG, "null geometry table");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  if (h->cfg.c_in != 3 || h->cfg.c_out != 1) return fail(h, PSM_ERR_UNSUPPORTED, "the mesh entry needs c_in == 3 and c_out == 1 (python_module.py:288-292)");
  if (ny < 1 || nx < 1) return fail(h, PSM_ERR_ARG, "bad grid shape");
  // everything that needs no device first: a bad table leaves the handle as it was
  std::vector<PsmMeshCaseInput> in(n_cases);
  for (int k = 0; k < n_cases; ++k) in[k] = PsmMeshCaseInput{n_cells[k], vtx_m2g[k], wts_m2g[k], indices[k], sdfunct[k], vtx_g2m[k], wts_g2m[k]};
  PsmMeshCaseTables t;
  std::string why;
  if (psm_build_mesh_case_tables(n_cases, in.data(), ny, nx, normalise_sdf ? 1.0 / maxs[2] : 1.0, wall_threshold, t, why)) return fail(h, PSM_ERR_ARG, why);
  int rc = psm_plan_grid(h, ny, nx);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  free_geometry(h);                                         // the single mesh goes, and an earlier case set
  MeshCaseSet& m = h->mcs;
  for (int k = 0; k < 4; ++k) h->maxs[k] = maxs[k];
  h->normalise_sdf = normalise_sdf; h->fill_input = fill_input;
  const int n_parts = (int)std::min<int64_t>(PSM_MESH_CASE_PARTS, (t.max_cells + 4095) / 4096);
  const size_t total = (size_t)t.total;
  hipError_t e = hipSuccess;
  if ((rc = dev_upload(h, &m.d_off, t.cell_off)) || (rc = dev_upload(h, &m.d_vtx_m2g, t.vtx_m2g)) || (rc = dev_upload(h, &m.d_wts_m2g, t.wts_m2g)) ||
      (rc = dev_upload(h, &m.d_src_of_cell, t.src_of_cell)) || (rc = dev_upload(h, &m.d_cell_of_point, t.cell_of_point)) ||
      (rc = dev_upload(h, &m.d_sdf, t.sdf)) || (rc = dev_upload(h, &m.d_vtx_g2m, t.vtx_g2m)) || (rc = dev_upload(h, &m.d_wts_g2m, t.wts_g2m)) ||
      (rc = dev_upload(h, &m.d_near_wall, t.near_wall)) || (rc = dev_alloc(h, &m.d_cells, total * 5)) || (rc = dev_alloc(h, &m.d_p, total)) ||
      (rc = dev_alloc(h, &m.d_umax, (size_t)n_cases)) || (rc = dev_alloc(h, &m.d_umax_part, (size_t)n_cases * n_parts))) { mesh_cases_free(h); return rc; }
  if ((e = hipHostMalloc((void**)&m.h_cells, total * 5 * sizeof(double), hipHostMallocDefault)) != hipSuccess ||
      (e = hipHostMalloc((void**)&m.h_p, total * sizeof(double), hipHostMallocDefault)) != hipSuccess) {
    mesh_cases_free(h);
    return fail(h, PSM_ERR_NOMEM, std::string("hipHostMalloc(case set staging): ") + hipGetErrorString(e));
  }
  PsmMeshCasesArgs& a = m.args;
  a = PsmMeshCasesArgs{};
  a.cell_off = m.d_off; a.umax_part = m.d_umax_part; a.umax = m.d_umax; a.n_parts = n_parts; a.n_cases = n_cases;
  a.vtx_m2g = m.d_vtx_m2g; a.wts_m2g = m.d_wts_m2g; a.src_of_cell = m.d_src_of_cell; a.sdf = m.d_sdf; a.grid = h->d_grid_stage;
  a.n_grid = t.n_grid; a.max_abs_ux = maxs[0]; a.max_abs_uy = maxs[1]; a.sdf_scale = normalise_sdf ? 1.0 / maxs[2] : 1.0;
  a.c_in = h->cfg.c_in; a.fill = fill_input;
  a.vtx_g2m = m.d_vtx_g2m; a.wts_g2m = m.d_wts_g2m; a.cell_of_point = m.d_cell_of_point; a.field = h->d_fields_stage;
  a.near_wall = m.d_near_wall; a.max_cells = t.max_cells; a.max_abs_p = maxs[3]; a.c_out = h->cfg.c_out;
  m.off = t.cell_off; m.n_cases = n_cases;
  // The entry builds its K images from THESE sdfuncts at every step: bind the K geometries for psm_solve_cases* only (scope 1,
  // like psm_set_geometry binds its one; a single case takes the single-case binding and with it the route of psm_solve).
  if (h->cfg.sdf_channel == 2 && getenv("PSM_NO_BIND") == nullptr) {
    HIPCHK(h, psm_copy_h2d(h->d_grid_stage, t.sdf_image.data(), t.sdf_image.size() * sizeof(float)));
    h->bound_scope = 1;
    rc = bind_geometry_device(h, h->d_grid_stage, n_cases);
    if (rc == PSM_ERR_UNSUPPORTED) h->err.clear();           // configuration outside the fused path: general path
    else if (rc) { mesh_cases_free(h); return rc; }
  }
  if ((rc = ensure_encode_aux(h, n_cases))) { mesh_cases_free(h); return rc; }   // once, outside any capture (psm_solve_begin does the same)
  m.ready = true;
  return PSM_OK;
}


int psm_init_geometry_cases(psm_handle* h, int32_t n_cases, const double* const* cells, const int64_t* n, const double* const* top,
                            const int64_t* n_top, const double* const* obst, const int64_t* n_obst) {
  if (!h) return PSM_ERR_ARG;
  if (!cells || !n || !top || !n_top || !obst || !n_obst) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  int32_t ny = 0, nx = 0;
  for (int k = 0; k < n_cases; ++k) {
    if (!cells[k] || !top[k] || !obst[k]) return fail(h, PSM_ERR_ARG, "case " + std::to_string(k) + ": null buffer");
    int32_t nyk = 0, nxk = 0;
    if (psm_geometry_shape(cells[k], n[k], h->case_delta, &nyk, &nxk, nullptr) != PSM_OK)
      return fail(h, PSM_ERR_ARG, "case " + std::to_string(k) + ": " + psm_geometry_last_error());
    if (k == 0) { ny = nyk; nx = nxk; }
    else if (nyk != ny || nxk != nx)
      return fail(h, PSM_ERR_ARG, "case " + std::to_string(k) + ": grid shape " + std::to_string(nyk) + " x " + std::to_string(nxk) + " differs from case 0's " +
                                      std::to_string(ny) + " x " + std::to_string(nx));
  }
  const size_t ng = (size_t)ny * nx;
  std::vector<std::vector<int32_t>> v1(n_cases), idx(n_cases), v2(n_cases);
  std::vector<std::vector<double>> w1(n_cases), sdf(n_cases), w2(n_cases);
  std::vector<const int32_t*> pv1(n_cases), pidx(n_cases), pv2(n_cases);
  std::vector<const double*> pw1(n_cases), psdf(n_cases), pw2(n_cases);
  for (int k = 0; k < n_cases; ++k) {
    v1[k].resize(ng * 3); w1[k].resize(ng * 3); idx[k].resize(ng * 2); sdf[k].resize(ng); v2[k].resize((size_t)n[k] * 3); w2[k].resize((size_t)n[k] * 3);
    const int rc = psm_geometry_build(cells[k], n[k], top[k], n_top[k], obst[k], n_obst[k], h->case_delta, h->case_every, v1[k].data(), w1[k].data(),
                                      idx[k].data(), sdf[k].data(), v2[k].data(), w2[k].data());
    if (rc) return fail(h, rc, "case " + std::to_string(k) + ": " + psm_geometry_last_error());
    pv1[k] = v1[k].data(); pw1[k] = w1[k].data(); pidx[k] = idx[k].data(); psdf[k] = sdf[k].data(); pv2[k] = v2[k].data(); pw2[k] = w2[k].data();
  }
  return psm_set_geometry_cases(h, n_cases, n, ny, nx, pv1.data(), pw1.data(), pidx.data(), psdf.data(), pv2.data(), pw2.data(), h->case_maxs, 0, 0,
                                h->case_wall);
}


int psm_mesh_cases(const psm_handle* h, int32_t* n_cases, int64_t* cell_off) {
  if (!h) return PSM_ERR_ARG;
  if (!h->mcs.ready || !h->planned) return PSM_ERR_STATE;
  if (n_cases) *n_cases = h->mcs.n_cases;
  if (cell_off) std::copy(h->mcs.off.begin(), h->mcs.off.end(), cell_off);
  return PSM_OK;
}


int psm_solve_cases_device(psm_handle* h, const double* d_cells, double* d_p, void* stream) {
  if (!h) return PSM_ERR_ARG;
  int rc = cases_check(h);
  if (rc) return rc;
  if (h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a psm_solve_cases_begin is in flight on this handle: call psm_solve_cases_end first");
  if (!d_cells || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_cells) | reinterpret_cast<uintptr_t>(d_p)) & 7) return fail(h, PSM_ERR_ARG, "device buffers must be 8-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return cases_sequence(h, d_cells, d_p, stream ? (hipStream_t)stream : h->stream);
}


int psm_solve_cases_begin(psm_handle* h, const double* cells, double* p_out) {
  if (!h) return PSM_ERR_ARG;
  if (h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a psm_solve_cases_begin is already in flight on this handle: call psm_solve_cases_end first");
  int rc = cases_check(h);
  if (rc) return rc;
  if (!cells || !p_out) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  MeshCaseSet& m = h->mcs;
  hipStream_t st = h->stream;
  const size_t total = (size_t)m.off[m.n_cases], in_bytes = total * 5 * sizeof(double), out_bytes = total * sizeof(double);
  // one H2D of the concatenated cells, one D2H of p: straight from / into arrays registered with psm_host_register, else through the pinned staging
  const bool reg_in = host_registered(h, cells, in_bytes), reg_out = host_registered(h, p_out, out_bytes);
  if (!reg_in) memcpy(m.h_cells, cells, in_bytes);
  HIPCHK(h, hipMemcpyAsync(m.d_cells, reg_in ? cells : m.h_cells, in_bytes, hipMemcpyHostToDevice, st));
  if ((rc = cases_sequence(h, m.d_cells, m.d_p, st))) return rc;
  HIPCHK(h, hipMemcpyAsync(reg_out ? p_out : m.h_p, m.d_p, out_bytes, hipMemcpyDeviceToHost, st));
  m.copy_out = reg_out ? nullptr : p_out;
  m.inflight = true;
  return PSM_OK;
}


int psm_solve_cases_end(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  if (!h->mcs.inflight) return fail(h, PSM_ERR_STATE, "no psm_solve_cases_begin in flight");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  h->mcs.inflight = false;
  HIPCHK(h, wait_stream(h->stream));
  if (h->mcs.copy_out) memcpy(h->mcs.copy_out, h->mcs.h_p, (size_t)h->mcs.off[h->mcs.n_cases] * sizeof(double));
  return PSM_OK;
}


int psm_solve_cases(psm_handle* h, const double* cells, double* p_out) {
  int rc = psm_solve_cases_begin(h, cells, p_out);
  return rc ? rc : psm_solve_cases_end(h);
}



int psm_pin_buffers(psm_handle* h, const double* cells, double* p_out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->have_geometry) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unpin_buffers(h);
  if (cells) {
    hipError_t e = hipHostRegister((void*)cells, (size_t)h->n_cells * 5 * sizeof(double), hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, PSM_ERR_HIP, std::string("hipHostRegister(cells): ") + hipGetErrorString(e)); }
    h->pinned_cells = cells;
    void* dc = nullptr;                                   // mapped address: lets psm_stage_cells_kernel read the cells from the host array
    if (hipHostGetDevicePointer(&dc, (void*)cells, 0) == hipSuccess && getenv("PSM_NO_DIRECT_IN") == nullptr) h->pinned_cells_dev = (const double*)dc;
    else (void)hipGetLastError();
  }
  if (p_out) {
    hipError_t e = hipHostRegister((void*)p_out, (size_t)h->n_cells * sizeof(double), hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); unpin_buffers(h); return fail(h, PSM_ERR_HIP, std::string("hipHostRegister(p_out): ") + hipGetErrorString(e)); }
    h->pinned_p = p_out;
    void* dp = nullptr;                                   // mapped address: lets psm_to_mesh_kernel store p into the host array
    if (hipHostGetDevicePointer(&dp, (void*)p_out, 0) == hipSuccess && getenv("PSM_NO_DIRECT_OUT") == nullptr) h->pinned_p_dev = (double*)dp;
    else (void)hipGetLastError();
  }
  return PSM_OK;
}


int psm_unpin_buffers(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unpin_buffers(h);
  return PSM_OK;
}


int psm_mesh_to_grid(psm_handle* h, const double* values, int64_t n, int32_t k, int32_t fill, double* grid_out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->have_geometry) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called");
  if (!values || !grid_out) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n != h->n_cells) return fail(h, PSM_ERR_ARG, "cell count differs from the geometry");
  if (k < 1 || k > 16) return fail(h, PSM_ERR_ARG, "1..16 columns");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t st = h->stream;
  const size_t ng = (size_t)h->Ny * h->Nx;
  int rc;
  const size_t vb = (size_t)n * k * sizeof(double), ob = ng * k * sizeof(double);
  if ((rc = scratch_reserve(h, carve_size({vb, ob}), carve_size({vb, ob})))) return rc;
  Carver cd{(char*)h->scr_dev}, cp{(char*)h->scr_pin};
  double* d_v = cd.take<double>((size_t)n * k); double* d_o = cd.take<double>(ng * k);
  double* p_v = cp.take<double>((size_t)n * k); double* p_o = cp.take<double>(ng * k);
  memcpy(p_v, values, vb);
  hipError_t e = hipMemcpyAsync(d_v, p_v, vb, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = psm_launch_interp_to_grid(d_v, k, h->d_vtx_m2g, h->d_wts_m2g, h->d_src_of_cell, fill, d_o, (int64_t)ng, st);
  if (e == hipSuccess) e = hipMemcpyAsync(p_o, d_o, ob, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = wait_stream(st);
  if (e == hipSuccess) memcpy(grid_out, p_o, ob);
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string("mesh_to_grid: ") + hipGetErrorString(e));
  return PSM_OK;
}


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
  if (!h) return PSM_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_pressure_graphs(h);
  integ_free(h->integ_dev);
  return PSM_OK;
}


int psm_integrate_gradp_device(psm_handle* h, const float* d_gradp, int32_t n_cases, float* d_p, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!d_gradp || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = integ_check(h, n_cases);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return integrate_device(h, d_gradp, n_cases, d_p, stream ? (hipStream_t)stream : h->stream);
}


int psm_solve_pressure_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale, float* d_gradp,
                              float* d_p, void* stream) {
  if (!h) return PSM_ERR_ARG;
  if (!d_grid || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  int rc = integ_check(h, n_cases);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  float* g = d_gradp ? d_gradp : h->integ_dev.d_gradp;
  if ((reinterpret_cast<uintptr_t>(g) & 7) || (reinterpret_cast<uintptr_t>(d_p) & 3)) return fail(h, PSM_ERR_ARG, "gradient buffer must be 8-byte aligned");
  return solve_device(h, d_grid, n_cases, out_scale, g, st, nullptr, d_p);       // one graph replay: the solve's launches + the two of the integration
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
  for (int pass = 0; pass < 2; ++pass) {
    if ((rc = solve_device(h, h->d_grid_stage, n_cases, out_scale, s.d_gradp, h->stream, nullptr, s.d_p))) return rc;
    HIPCHK(h, hipMemcpyAsync(reg_out ? p : h->h_fields, s.d_p, pout, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h->stream));
    if (pass == 1 || !guard_take(h, h->ws0)) break;     // not the bound geometry: the gradient is NaN -- drop the binding, solve again on the general path
    if ((rc = guard_drop(h, "psm_solve_pressure"))) return rc;
    h->err += " (solved on the general path)";
  }
  if (!reg_out) memcpy(p, h->h_fields, pout);
  return PSM_OK;
}

}  // extern "C"
