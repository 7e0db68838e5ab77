// psm_api_mesh.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the solver boundary (mesh <-> grid): the single mesh and the case batch.  See psm_handle.h for the map of the files.
#include "psm_handle.h"
#include "psm_mesh_tables.h"

namespace psm_impl {

// One builder per end of psm_solve, for the plain launches of psm_solve_begin and for mesh_sequence alike
PsmToGridArgs to_grid_args(const psm_handle* h, const double* d_umax, double umax_val, int n_partials) {
  const MeshSingle& m = h->mesh;
  PsmToGridArgs ga{};
  ga.cells = m.d_cells; ga.umax = d_umax; ga.umax_val = umax_val;
  if (n_partials > 0) { ga.umax_partials = m.d_umax_part; ga.n_partials = n_partials; ga.umax_out = m.d_umax; }
  ga.vtx = m.t.vtx_m2g; ga.wts = m.t.wts_m2g; ga.src_of_cell = m.t.src_of_cell;
  ga.sdf = m.t.sdf; ga.grid = h->d_grid_stage; ga.n_grid = (int64_t)h->Ny * h->Nx;
  ga.max_abs_ux = h->maxs[0]; ga.max_abs_uy = h->maxs[1]; ga.sdf_scale = h->normalise_sdf ? 1.0 / h->maxs[2] : 1.0;
  ga.c_in = h->cfg.c_in; ga.fill = h->fill_input;
  return ga;
}

PsmToMeshArgs to_mesh_args(const psm_handle* h, const double* d_umax, double umax_val, double* p_out) {
  const MeshSingle& m = h->mesh;
  PsmToMeshArgs ma{};
  ma.cells = m.d_cells; ma.umax = d_umax; ma.umax_val = umax_val; ma.vtx = m.t.vtx_g2m; ma.wts = m.t.wts_g2m; ma.cell_of_point = m.t.cell_of_point;
  ma.field = h->d_fields_stage; ma.near_wall = m.t.near_wall; ma.p_out = p_out; ma.n_cells = h->n_cells; ma.max_abs_p = h->maxs[3];
  ma.c_out = h->cfg.c_out;
  return ma;
}

// The tables of one mesh or of a case set, validated and derived by psm_build_mesh_case_tables, to the device.  A failure leaves
// what was uploaded so far to the caller's free function.
int mesh_tables_upload(psm_handle* h, MeshTablesDev& d, const PsmMeshCaseTables& t) {
  int rc;
  if ((rc = dev_upload(h, &d.off, t.cell_off)) || (rc = dev_upload(h, &d.vtx_m2g, t.vtx_m2g)) || (rc = dev_upload(h, &d.wts_m2g, t.wts_m2g)) ||
      (rc = dev_upload(h, &d.src_of_cell, t.src_of_cell)) || (rc = dev_upload(h, &d.cell_of_point, t.cell_of_point)) ||
      (rc = dev_upload(h, &d.sdf, t.sdf)) || (rc = dev_upload(h, &d.vtx_g2m, t.vtx_g2m)) || (rc = dev_upload(h, &d.wts_g2m, t.wts_g2m)) ||
      (rc = dev_upload(h, &d.near_wall, t.near_wall))) return rc;
  return PSM_OK;
}

void mesh_tables_free(MeshTablesDev& t) {
  dev_free(t.off); dev_free(t.vtx_m2g); dev_free(t.src_of_cell); dev_free(t.vtx_g2m); dev_free(t.cell_of_point);
  dev_free(t.wts_m2g); dev_free(t.sdf); dev_free(t.wts_g2m); dev_free(t.near_wall);
}

int mesh_buffers_alloc(psm_handle* h, MeshBuffers& b, size_t total_cells, size_t n_umax, size_t n_partials, int host_alloc_err, const char* what) {
  int rc;
  if ((rc = dev_alloc(h, &b.d_cells, total_cells * 5)) || (rc = dev_alloc(h, &b.d_p, total_cells)) || (rc = dev_alloc(h, &b.d_umax, n_umax)) ||
      (rc = dev_alloc(h, &b.d_umax_part, n_partials)) || (rc = dev_alloc(h, &h->delta.d_u_prev, total_cells * 2))) return rc;
  hipError_t e = hipSuccess;
  if ((e = hipHostMalloc((void**)&b.h_cells, total_cells * 5 * sizeof(double), hipHostMallocDefault)) != hipSuccess ||
      (e = hipHostMalloc((void**)&b.h_p, total_cells * sizeof(double), hipHostMallocDefault)) != hipSuccess)
    return fail(h, host_alloc_err, std::string("hipHostMalloc(") + what + "): " + hipGetErrorString(e));
  return PSM_OK;
}

void mesh_buffers_free(MeshBuffers& b) {
  mesh_tables_free(b.t);
  dev_free(b.d_cells); dev_free(b.d_p); dev_free(b.d_umax); dev_free(b.d_umax_part);
  b.h_sdf.clear();
  if (b.h_cells) { (void)hipHostFree(b.h_cells); b.h_cells = nullptr; }
  if (b.h_p) { (void)hipHostFree(b.h_p); b.h_p = nullptr; }
}

// psm_solve on registered, mapped caller buffers: every device-side step of the call, in stream order (captured once)
static int mesh_sequence(psm_handle* h, int64_t n, hipStream_t st) {
  MeshSingle& m = h->mesh;
  int n_partials = 0;
  HIPCHK(h, psm_launch_stage_cells(m.pinned_cells_dev, m.d_cells, n, m.d_umax_part, &n_partials, st));
  HIPCHK(h, psm_launch_to_grid(to_grid_args(h, nullptr, 0.0, n_partials), st));
  h->in_mesh_solve = true;
  int rc = launch_all(h, h->ws0, h->d_grid_stage, 1, h->d_fields_stage, h->d_ones, st, nullptr, psm_switches_per_solve());
  h->in_mesh_solve = false;
  if (rc) return rc;
  HIPCHK(h, psm_launch_to_mesh(to_mesh_args(h, m.d_umax, 0.0, m.pinned_p_dev), st));
  return PSM_OK;
}

// ---- the case set of psm_set_geometry_cases -----------------------------------------------------------------------
// state checks shared by the step entries
int cases_check(psm_handle* h) {
  if (h->have_geometry && !h->mcs.ready)
    return fail(h, PSM_ERR_STATE, "the handle holds the single mesh of psm_set_geometry: psm_solve_cases* needs a case set (psm_set_geometry_cases)");
  if (!h->mcs.ready || !h->planned)
    return fail(h, PSM_ERR_STATE, "psm_set_geometry_cases has not been called (or its case set was dropped by a later psm_set_* / psm_plan_grid)");
  // a case set under the four-channel model serves psm_solve_cases_poisson* alone, one under the gradP model psm_solve_cases_gradp*
  if (h->cfg.c_in != 3 || h->cfg.c_out != 1) return fail(h, PSM_ERR_UNSUPPORTED, "the mesh entry needs c_in == 3 and c_out == 1 (python_module.py:288-292)");
  return PSM_OK;
}

// the whole chain of a delta step is enqueued: the state has advanced (a priming step does not count)
static void delta_advance(psm_handle* h) { h->delta.steps += h->delta.primed; h->delta.primed = true; }

// One step of the case set, a linear chain on `st`: U_max partials, to_grid, the batched solve, to_mesh.  Plain launches (like
// psm_solve; the solve inside replays its graph under PSM_GRAPH=1); copies nothing.  `delta`: the two ends in their delta form on
// U(t-1); a state that is not primed gets the priming step, the last launch alone.  The state's host flags move once all is enqueued.
static int cases_sequence(psm_handle* h, const double* d_cells, double* d_p, hipStream_t st, bool delta) {
  PsmDeltaCasesArgs d{h->mcs.args, h->delta.d_u_prev, delta && !h->delta.primed};
  PsmMeshCasesArgs& a = d.c;
  a.cells = d_cells; a.p_out = d_p;
  if (!d.prime) {
    HIPCHK(h, psm_launch_umax_cases(a, st));
    HIPCHK(h, delta ? psm_launch_to_grid_cases_delta(d, st) : psm_launch_to_grid_cases(a, st));
    h->in_mesh_solve = true;
    const int rc = solve_device(h, h->d_grid_stage, h->mcs.n_cases, nullptr, h->d_fields_stage, st, nullptr);
    h->in_mesh_solve = false;
    if (rc) return rc;
  }
  HIPCHK(h, delta ? psm_launch_to_mesh_cases_delta(d, st) : psm_launch_to_mesh_cases(a, st));
  if (delta) delta_advance(h);
  return PSM_OK;
}

// The six tables of psm_set_geometry for one case on its ny x nx grid (psm_geometry_build), behind psm_init_geometry (the K = 1
// use, no prefix to its messages) and psm_init_geometry_cases ("case k: ")
struct GeometryTables {
  std::vector<int32_t> v1, idx, v2;
  std::vector<double> w1, sdf, w2;
};
static int geometry_tables_build(psm_handle* h, const std::string& prefix, const double* cells, int64_t n, const double* top, int64_t n_top,
                                 const double* obst, int64_t n_obst, int32_t ny, int32_t nx, GeometryTables& t) {
  const size_t ng = (size_t)ny * nx;
  t.v1.resize(ng * 3); t.w1.resize(ng * 3); t.idx.resize(ng * 2); t.sdf.resize(ng); t.v2.resize((size_t)n * 3); t.w2.resize((size_t)n * 3);
  const int rc = psm_geometry_build(cells, n, top, n_top, obst, n_obst, h->case_delta, h->case_every, t.v1.data(), t.w1.data(), t.idx.data(),
                                    t.sdf.data(), t.v2.data(), t.w2.data());
  return rc ? fail(h, rc, prefix + psm_geometry_last_error()) : PSM_OK;
}

void delta_drop(psm_handle* h) {
  dev_free(h->delta.d_u_prev);
  h->delta.primed = false; h->delta.steps = 0;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_set_geometry(psm_handle* h, int64_t n_cells, int32_t ny, int32_t nx, const int32_t* vtx_m2g, const double* wts_m2g,
                     const int32_t* indices, const double* sdfunct, const int32_t* vtx_g2m, const double* wts_g2m,
                     const double* maxs, int32_t normalise_sdf, int32_t fill_input, double wall_threshold) {
  if (!h) return PSM_ERR_ARG;
  if (!vtx_m2g || !wts_m2g || !indices || !sdfunct || !maxs) return fail(h, PSM_ERR_ARG, "null geometry table");
  if ((vtx_g2m == nullptr) != (wts_g2m == nullptr)) return fail(h, PSM_ERR_ARG, "vtx_g2m and wts_g2m go together");
  if (n_cells < 1 || n_cells > (int64_t)1 << 30) return fail(h, PSM_ERR_ARG, "bad cell count");
  if (ny < 1 || nx < 1) { const int rc = psm_plan_grid(h, ny, nx); return rc ? rc : fail(h, PSM_ERR_ARG, "bad grid shape"); }   // no grid has that shape: psm_plan_grid says so
  // everything that needs no device first: a bad table leaves the handle as it was
  const PsmMeshCaseInput in{n_cells, vtx_m2g, wts_m2g, indices, sdfunct, vtx_g2m, wts_g2m};
  PsmMeshCaseTables t;
  std::string why;
  if (psm_build_mesh_case_tables(1, &in, ny, nx, normalise_sdf ? 1.0 / maxs[2] : 1.0, wall_threshold, t, why, true)) return fail(h, PSM_ERR_ARG, why);
  int rc = psm_plan_grid(h, ny, nx);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  free_geometry(h);
  MeshSingle& m = h->mesh;
  // all-or-nothing from here on: a failure leaves no geometry
  if ((rc = mesh_tables_upload(h, m.t, t)) || (rc = mesh_buffers_alloc(h, m, (size_t)n_cells, 1, 256, PSM_ERR_HIP, "mesh staging"))) { free_geometry(h); return rc; }
  h->n_cells = n_cells;
  m.h_sdf = t.sdf;                                         // the raw sdfunct, for psm_bind_gradp_solve
  for (int k = 0; k < 4; ++k) h->maxs[k] = maxs[k];
  h->normalise_sdf = normalise_sdf; h->fill_input = fill_input;
  h->have_g2m = t.have_g2m;
  h->have_geometry = true;
  // The mesh entry builds its grid from THIS sdfunct at every step, so the geometry of psm_solve is fixed from here
  // on: bind it (scope: psm_solve only -- grid-native solves on the same handle stay general until psm_bind_geometry).
  if (h->cfg.c_in == 3 && h->cfg.sdf_channel == 2 && t.have_g2m && !psm_switches_at_bind().no_bind) {
    hipError_t ec = psm_copy_h2d(h->d_grid_stage, t.sdf_image.data(), t.sdf_image.size() * sizeof(float));   // the SDF channel exactly as psm_to_grid_kernel writes it
    if (ec != hipSuccess) { free_geometry(h); return fail(h, PSM_ERR_HIP, std::string("psm_copy_h2d(sdf image): ") + hipGetErrorString(ec)); }
    h->bound_scope = 1;                                      // before the bind: this scope builds no SDF-fold tables
    rc = bind_geometry_device(h, h->d_grid_stage);
    if (rc == PSM_OK) h->bound_scope = 1;
    else if (rc == PSM_ERR_UNSUPPORTED) h->err.clear();      // configuration outside the fused path: general path
    else { free_geometry(h); return rc; }
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
  GeometryTables t;
  const int rc = geometry_tables_build(h, "", cells, n, top, n_top, obst, n_obst, ny, nx, t);
  return rc ? rc : psm_set_geometry(h, n, ny, nx, t.v1.data(), t.w1.data(), t.idx.data(), t.sdf.data(), t.v2.data(), t.w2.data(), h->case_maxs, 0, 0, h->case_wall);
}


int psm_solve_begin(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  (void)rank;
  return h ? mesh_step_begin(h, cells, n, p_out, false) : PSM_ERR_ARG;
}

}  // extern "C"

namespace psm_impl {

int mesh_step_check(psm_handle* h, const double* cells, int64_t n, const double* p_out, bool prime) {
  if (h->mesh.inflight)
    return fail(h, PSM_ERR_STATE, prime ? "a step is in flight on this handle: call psm_solve_end first"
                                        : "a psm_solve_begin is already in flight on this handle: call psm_solve_end first");
  if (h->mcs.ready)
    return fail(h, PSM_ERR_STATE, prime ? "the handle holds the case set of psm_set_geometry_cases: use psm_delta_prime_cases"
                                        : "the handle holds the case set of psm_set_geometry_cases: psm_solve needs the single mesh of psm_set_geometry (use psm_solve_cases*)");
  if (!h->have_geometry || !h->planned)
    return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (or the plan it belonged to was dropped by a later psm_set_* / psm_plan_grid)");
  if (!prime) {
    if (h->cfg.c_in != 3 || h->cfg.c_out != 1) return fail(h, PSM_ERR_UNSUPPORTED, "the mesh entry needs c_in == 3 and c_out == 1 (python_module.py:288-292)");
    if (!h->have_g2m) return fail(h, PSM_ERR_STATE, "psm_set_geometry was called without the grid->mesh tables");
  }
  if (!cells || (!prime && !p_out)) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n != h->n_cells) return fail(h, PSM_ERR_ARG, "cell count differs from the geometry");
  return PSM_OK;
}

int step_end(psm_handle* h, MeshBuffers& b, int64_t total_cells, const char* begin_name) {
  if (!b.inflight) return fail(h, PSM_ERR_STATE, std::string("no ") + begin_name + " in flight");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  b.inflight = false;
  HIPCHK(h, wait_stream(h->stream));
  if (b.copy_out) memcpy(b.copy_out, b.h_p, (size_t)total_cells * sizeof(double));
  return PSM_OK;
}

// ---- the route of a step on the single mesh, chosen once (like choose_route of a solve, psm_api_solve.cpp) --------------------------
// Its switches, from the handle's table (psm_create): PSM_MESH_GRAPH (registered + mapped buffers: 0 = the staged route, 1 = one
// graph replay, 2 = the same sequence as plain launches, the measured default), PSM_MESH_STAGE_MAX (largest
// mesh psm_stage_cells_kernel reads over PCIe), PSM_DEVICE_UMAX (set: small meshes reduce U_max by psm_umax_kernel, not on the
// host).  At every psm_pin_buffers: PSM_NO_DIRECT_IN / _OUT (set: no mapped address, DMA only).

// mapped_*: both arrays registered (psm_pin_buffers) and mapped -- psm_stage_cells_kernel reads the cells over PCIe and takes the
// partial maxima of U_max on the way (no DMA-engine copy, no host pass, U_max never leaves the device: to_grid reduces the partials
// and hands the scalar to to_mesh through d_umax), to_grid, the kernels of the solve, to_mesh storing p straight into the caller's
// array; as ONE hipGraph replay or as plain launches.  A delta step stays off it.
// staged: a DMA copy in; U_max on the host while that copy is in flight (one launch less), by psm_umax_kernel, or for large meshes
// (the host pass would take longer than the copy it hides under) by the parallel reduction whose partials every to_grid workgroup
// folds itself; none for the priming step of a delta state, which is the last launch alone, p = cells[:,4].
enum class MeshRouteKind { mapped_graph, mapped_plain, staged };
enum class UmaxFrom { none, host, device_scalar, partials };
struct MeshRoute { MeshRouteKind kind; UmaxFrom umax; bool direct_p; };   // direct_p: to_mesh stores p over PCIe into the registered output, no D2H copy
static MeshRoute choose_mesh_route(const psm_handle* h, const double* cells, int64_t n, const double* p_out, bool delta) {
  const PsmSwitches::AtCreate& env = h->sw.at_create;
  const MeshSingle& m = h->mesh;
  if (!delta && env.mesh_graph != 0 && h->timed_kernel < 0 && n <= env.mesh_stage_max && cells == m.pinned_cells && m.pinned_cells_dev && p_out == m.pinned_p && m.pinned_p_dev)
    return MeshRoute{env.mesh_graph == 2 ? MeshRouteKind::mapped_plain : MeshRouteKind::mapped_graph, UmaxFrom::partials, true};
  const UmaxFrom umax = delta && !h->delta.primed ? UmaxFrom::none : n > 32768 ? UmaxFrom::partials : env.device_umax ? UmaxFrom::device_scalar : UmaxFrom::host;
  return MeshRoute{MeshRouteKind::staged, umax, p_out == m.pinned_p && m.pinned_p_dev != nullptr};
}

// U_max = max sqrt(Ux^2 + Uy^2) (PM:270) on the host: sqrt is monotonic and correctly rounded on both sides, so
// sqrt(max(Ux^2 + Uy^2)) is the kernel's value bit for bit (NaN propagates like np.max).
static double host_umax(const double* cells, int64_t n) {
  double m2 = 0.0; bool nan = false;
  for (int64_t i = 0; i < n; ++i) {
    const double ux = cells[i * 5], uy = cells[i * 5 + 1];
    const double v = ux * ux + uy * uy;
    nan = nan || (v != v);
    m2 = v > m2 ? v : m2;
  }
  return nan ? std::nan("") : std::sqrt(m2);
}

static int mesh_step_mapped(psm_handle* h, int64_t n, bool graph) {
  MeshSingle& m = h->mesh;
  hipStream_t st = h->stream;
  h->last_cases = 1;
  m.copy_out = nullptr;
  if (!graph) return mesh_sequence(h, n, st);
  if (!m.graph) {
    int rc = capture_graph(h, st, "psm_solve", [&] { return mesh_sequence(h, n, st); }, &m.graph);
    if (rc) return rc;
    m.graph_left = h->last;
  } else {
    h->last = m.graph_left;
  }
  HIPCHK(h, hipGraphLaunch(m.graph, st));
  return PSM_OK;
}

static int mesh_step_staged(psm_handle* h, const double* cells, int64_t n, double* p_out, bool delta, const MeshRoute& r) {
  MeshSingle& m = h->mesh;
  hipStream_t st = h->stream;
  const bool reg_in = cells == m.pinned_cells, reg_out = p_out == m.pinned_p;   // registered by the caller: DMA straight from / into its buffer
  if (!reg_in) memcpy(m.h_cells, cells, (size_t)n * 5 * sizeof(double));
  HIPCHK(h, hipMemcpyAsync(m.d_cells, reg_in ? cells : m.h_cells, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice, st));
  const bool prime = r.umax == UmaxFrom::none;
  double umax_val = 0.0;
  int n_partials = 0;
  if (r.umax == UmaxFrom::partials) HIPCHK(h, psm_launch_umax_partial(m.d_cells, n, m.d_umax_part, &n_partials, st));
  else if (r.umax == UmaxFrom::device_scalar) HIPCHK(h, psm_launch_umax(m.d_cells, n, m.d_umax, st));
  else if (r.umax == UmaxFrom::host) umax_val = host_umax(cells, n);   // while the copy above is in flight
  if (!prime) {
    // to_grid must not take the scalar with partials: it folds them itself and only then leaves U_max in d_umax, for to_mesh
    const PsmToGridArgs ga = to_grid_args(h, r.umax == UmaxFrom::device_scalar ? m.d_umax : nullptr, umax_val, n_partials);
    HIPCHK(h, delta ? psm_launch_to_grid_delta(PsmDeltaGridArgs{ga, h->delta.d_u_prev}, st) : psm_launch_to_grid(ga, st));
    h->in_mesh_solve = true;
    int rc = solve_device(h, h->d_grid_stage, 1, nullptr, h->d_fields_stage, st, nullptr);
    h->in_mesh_solve = false;
    if (rc) return rc;
  }
  const double* d_umax = (r.umax == UmaxFrom::device_scalar || r.umax == UmaxFrom::partials) ? m.d_umax : nullptr;
  const PsmToMeshArgs ma = to_mesh_args(h, d_umax, umax_val, r.direct_p ? m.pinned_p_dev : m.d_p);
  HIPCHK(h, delta ? psm_launch_to_mesh_delta(PsmDeltaMeshArgs{ma, h->delta.d_u_prev, prime}, st) : psm_launch_to_mesh(ma, st));
  if (delta) delta_advance(h);
  if (!r.direct_p) HIPCHK(h, hipMemcpyAsync(reg_out ? p_out : m.h_p, m.d_p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  m.copy_out = reg_out ? nullptr : p_out;
  return PSM_OK;
}

int mesh_step_begin(psm_handle* h, const double* cells, int64_t n, double* p_out, bool delta) {
  int rc = mesh_step_check(h, cells, n, p_out, false);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if ((rc = ensure_encode_aux(h, 1))) return rc;   // many-block cases (the shipped 104-block shape): the M-tiled encode's split basis, once, outside any capture
  const MeshRoute r = choose_mesh_route(h, cells, n, p_out, delta);
  rc = r.kind == MeshRouteKind::staged ? mesh_step_staged(h, cells, n, p_out, delta, r) : mesh_step_mapped(h, n, r.kind == MeshRouteKind::mapped_graph);
  if (rc) return rc;
  h->mesh.inflight = true;
  return PSM_OK;
}

}  // namespace psm_impl

extern "C" {

int psm_solve_end(psm_handle* h) { return h ? step_end(h, h->mesh, h->n_cells, "psm_solve_begin") : PSM_ERR_ARG; }


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
  // the three-channel models of psm_solve_cases*, or the four-channel Poisson model, whose set serves psm_solve_cases_poisson* alone
  // (maxs: max_abs_dUx, max_abs_dUy, max_abs_dist, max_abs_dp, as the single mesh reads them for that model), or the gradP model
  // (c_in == 3, c_out == 2; maxs: max_abs_Ux, max_abs_Uy, max_abs_dist, unused), whose set serves psm_solve_cases_gradp* alone
  const bool poisson_model = h->cfg.c_in == 4 && h->cfg.c_out == 1 && h->cfg.sdf_channel == 3;
  const bool gradp_model = h->cfg.c_in == 3 && h->cfg.c_out == 2;
  if (!poisson_model && !gradp_model && (h->cfg.c_in != 3 || h->cfg.c_out != 1))
    return fail(h, PSM_ERR_UNSUPPORTED, "the mesh entry needs c_in == 3 and c_out == 1 (python_module.py:288-292), the Poisson model's c_in == 4, c_out == 1, sdf_channel == 3, or the gradP model's c_in == 3, c_out == 2");
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
  if ((rc = mesh_tables_upload(h, m.t, t)) ||
      (rc = mesh_buffers_alloc(h, m, (size_t)t.total, (size_t)n_cases, (size_t)n_cases * n_parts, PSM_ERR_NOMEM, "case set staging"))) { mesh_cases_free(h); return rc; }
  PsmMeshCasesArgs& a = m.args;
  a = PsmMeshCasesArgs{};
  a.cell_off = m.t.off; a.umax_part = m.d_umax_part; a.umax = m.d_umax; a.n_parts = n_parts; a.n_cases = n_cases;
  a.vtx_m2g = m.t.vtx_m2g; a.wts_m2g = m.t.wts_m2g; a.src_of_cell = m.t.src_of_cell; a.sdf = m.t.sdf; a.grid = h->d_grid_stage;
  a.n_grid = t.n_grid; a.max_abs_ux = maxs[0]; a.max_abs_uy = maxs[1]; a.sdf_scale = normalise_sdf ? 1.0 / maxs[2] : 1.0;
  a.c_in = h->cfg.c_in; a.fill = fill_input;
  a.vtx_g2m = m.t.vtx_g2m; a.wts_g2m = m.t.wts_g2m; a.cell_of_point = m.t.cell_of_point; a.field = h->d_fields_stage;
  a.near_wall = m.t.near_wall; a.max_cells = t.max_cells; a.max_abs_p = maxs[3]; a.c_out = h->cfg.c_out;
  m.off = t.cell_off; m.n_cases = n_cases;
  m.h_sdf = t.sdf;                                          // the K raw sdfuncts, for psm_bind_gradp_solve_cases
  // The entry builds its K images from THESE sdfuncts at every step: bind the K geometries for psm_solve_cases* only (scope 1,
  // like psm_set_geometry binds its one; a single case takes the single-case binding and with it the route of psm_solve).
  if (h->cfg.sdf_channel == 2 && !psm_switches_at_bind().no_bind) {
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
  std::vector<GeometryTables> t(n_cases);
  std::vector<const int32_t*> pv1(n_cases), pidx(n_cases), pv2(n_cases);
  std::vector<const double*> pw1(n_cases), psdf(n_cases), pw2(n_cases);
  for (int k = 0; k < n_cases; ++k) {
    const int rc = geometry_tables_build(h, "case " + std::to_string(k) + ": ", cells[k], n[k], top[k], n_top[k], obst[k], n_obst[k], ny, nx, t[k]);
    if (rc) return rc;
    pv1[k] = t[k].v1.data(); pw1[k] = t[k].w1.data(); pidx[k] = t[k].idx.data(); psdf[k] = t[k].sdf.data(); pv2[k] = t[k].v2.data(); pw2[k] = t[k].w2.data();
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
  return h ? cases_step_device(h, d_cells, d_p, stream, false) : PSM_ERR_ARG;
}

int psm_solve_cases_begin(psm_handle* h, const double* cells, double* p_out) {
  return h ? cases_step_begin(h, cells, p_out, false) : PSM_ERR_ARG;
}

}  // extern "C"

int psm_impl::cases_step_device(psm_handle* h, const double* d_cells, double* d_p, void* stream, bool delta) {
  int rc = cases_check(h);
  if (rc) return rc;
  if (h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a psm_solve_cases_begin is in flight on this handle: call psm_solve_cases_end first");
  if (!d_cells || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!aligned_to(8, {d_cells, d_p})) return fail(h, PSM_ERR_ARG, "device buffers must be 8-byte aligned");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  return cases_sequence(h, d_cells, d_p, stream ? (hipStream_t)stream : h->stream, delta);
}


int psm_impl::cases_step_begin(psm_handle* h, const double* cells, double* p_out, bool delta) {
  if (h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a psm_solve_cases_begin is already in flight on this handle: call psm_solve_cases_end first");
  int rc = cases_check(h);
  if (rc) return rc;
  if (!cells || !p_out) return fail(h, PSM_ERR_ARG, "null buffer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  MeshCaseSet& m = h->mcs;
  hipStream_t st = h->stream;
  const HostStaging s(h, m, cells, p_out, (size_t)m.off[m.n_cases]);   // the in-flight flag (above) keeps the staging this step's
  HIPCHK(h, s.copy_in(st));
  if ((rc = cases_sequence(h, m.d_cells, m.d_p, st, delta))) return rc;
  HIPCHK(h, s.copy_out(st));
  m.copy_out = s.pending();
  m.inflight = true;
  return PSM_OK;
}

psm_impl::HostStaging::HostStaging(const psm_handle* h, MeshBuffers& m, const double* cells, double* p_out, size_t n)
    : m(m), cells(cells), p_out(p_out), in_bytes(n * 5 * sizeof(double)), out_bytes(n * sizeof(double)),
      reg_in(host_registered(h, cells, in_bytes)), reg_out(p_out && host_registered(h, p_out, out_bytes)) {}

hipError_t psm_impl::HostStaging::copy_in(hipStream_t st) const {
  if (!reg_in) memcpy(m.h_cells, cells, in_bytes);
  return hipMemcpyAsync(m.d_cells, reg_in ? cells : m.h_cells, in_bytes, hipMemcpyHostToDevice, st);
}

hipError_t psm_impl::HostStaging::copy_out(hipStream_t st) const {
  return p_out ? hipMemcpyAsync(reg_out ? p_out : m.h_p, m.d_p, out_bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
}

int psm_impl::bound_step_state(psm_handle* h, const BoundStepTexts& t, bool ready, int bound_cases, bool usable, int cases) {
  if (ready && cases == 0 && bound_cases) return fail(h, PSM_ERR_STATE, t.on_cases);
  if (ready && cases == 1 && !bound_cases) return fail(h, PSM_ERR_STATE, t.on_single);
  if (!usable) return fail(h, PSM_ERR_STATE, cases == 1 ? t.unbound_cases : t.unbound_single);
  if (h->mesh.inflight || h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a step is in flight on this handle: call psm_solve_end first");
  return PSM_OK;
}

int psm_impl::bind_zero_sync(psm_handle* h, const char* name, std::initializer_list<std::pair<void*, size_t>> zero, void (*free_fn)(psm_handle*)) {
  hipError_t e = hipSuccess;
  for (const auto& z : zero)
    if (e == hipSuccess) e = hipMemsetAsync(z.first, 0, z.second, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess) return PSM_OK;
  free_fn(h);
  return fail(h, PSM_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e));
}

extern "C" {


int psm_solve_cases_end(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  return step_end(h, h->mcs, h->mcs.inflight ? h->mcs.off[h->mcs.n_cases] : 0, "psm_solve_cases_begin");
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
  const PsmSwitches::AtBind sw = psm_switches_at_bind();
  if (cells) {
    hipError_t e = hipHostRegister((void*)cells, (size_t)h->n_cells * 5 * sizeof(double), hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, PSM_ERR_HIP, std::string("hipHostRegister(cells): ") + hipGetErrorString(e)); }
    h->mesh.pinned_cells = cells;
    void* dc = nullptr;                                   // mapped address: lets psm_stage_cells_kernel read the cells from the host array
    if (hipHostGetDevicePointer(&dc, (void*)cells, 0) == hipSuccess && !sw.no_direct_in) h->mesh.pinned_cells_dev = (const double*)dc;
    else (void)hipGetLastError();
  }
  if (p_out) {
    hipError_t e = hipHostRegister((void*)p_out, (size_t)h->n_cells * sizeof(double), hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); unpin_buffers(h); return fail(h, PSM_ERR_HIP, std::string("hipHostRegister(p_out): ") + hipGetErrorString(e)); }
    h->mesh.pinned_p = p_out;
    void* dp = nullptr;                                   // mapped address: lets psm_to_mesh_kernel store p into the host array
    if (hipHostGetDevicePointer(&dp, (void*)p_out, 0) == hipSuccess && !sw.no_direct_out) h->mesh.pinned_p_dev = (double*)dp;
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
  if (e == hipSuccess) e = psm_launch_interp_to_grid(d_v, k, h->mesh.t.vtx_m2g, h->mesh.t.wts_m2g, h->mesh.t.src_of_cell, fill, d_o, (int64_t)ng, st);
  if (e == hipSuccess) e = hipMemcpyAsync(p_o, d_o, ob, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = wait_stream(st);
  if (e == hipSuccess) memcpy(grid_out, p_o, ob);
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string("mesh_to_grid: ") + hipGetErrorString(e));
  return PSM_OK;
}

}  // extern "C"
