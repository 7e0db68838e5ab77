// psm_api_gradp_solve.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the gradient-model step at the solver boundary, cells [N,5] -> p [N]
// (U_to_gradP; the dimensionalisation of Eval_dual_Dense_onlycil.py:537-538, inverse of :441-442 and :467-468), on the single mesh
// (psm_solve_gradp*) and on a case set of K meshes (psm_solve_cases_gradp*).  See psm_handle.h for the map of the files.
//
// A step is psm_solve's two head launches (partial maxima, mesh -> grid), the handle's solve with the gradient left in the network's
// units, optionally the sigma_field filter of both components, the two integration launches of psm_integ.hip on tables of the
// binding's own with the spacings (sx, sy) = (dx max_abs_dPdx / extent_x, dy max_abs_dPdy / extent_y) -- the integration is linear in
// (SdPx dx, SdPy dy), so the plane it leaves is q = p / U^2 -- and one tail launch (psm_mesh.hip, PsmGradpMeshArgs / PsmGradpCasesArgs):
// the outlet level, grid -> mesh, p = acc U^2.  All of it is one graph replay (StepCall::gsolve).  No state: a step depends on its
// cells alone.  The two forms share every function below: a case set is the single mesh with N = sum n_i and K case slots.
#include "psm_handle.h"

namespace psm_impl {

// captured step graphs (StepCall::gsolve) hold the addresses of the mesh tables, the integration tables, the planes and the scalar slots
static void drop_gradp_solve_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.gsolve.cells != nullptr; }); }

void gradp_solve_free(psm_handle* h) {
  GradpSolveSet& s = h->gsolve;
  drop_gradp_solve_graphs(h);
  integ_free(s.integ);
  dev_free(s.d_image); dev_free(s.d_scalars);
  image_gone(h);
  s.ready = false; s.cases = 0; s.apply_filter = 0;
}

// psm_solve's two head launches on the call's cells, into the call's image; U_max stays in the mesh's device scalar(s) for the tail
int gradp_solve_head(psm_handle* h, const GradpSolveCall& gs, hipStream_t st) {
  if (gs.cases) {
    PsmMeshCasesArgs a = h->mcs.args;
    a.cells = gs.cells; a.grid = gs.image;
    HIPCHK(h, psm_launch_umax_cases(a, st));
    HIPCHK(h, psm_launch_to_grid_cases(a, st));
    return PSM_OK;
  }
  int n_partials = 0;
  HIPCHK(h, psm_launch_umax_partial(gs.cells, h->n_cells, h->mesh.d_umax_part, &n_partials, st));
  PsmToGridArgs ga = to_grid_args(h, nullptr, 0.0, n_partials);
  ga.cells = gs.cells; ga.grid = gs.image;
  HIPCHK(h, psm_launch_to_grid(ga, st));
  return PSM_OK;
}

// the two integration launches on the binding's tables, then the tail launch of either form
int gradp_solve_tail(psm_handle* h, const GradpSolveCall& gs, hipStream_t st) {
  const GradpSolveSet& S = h->gsolve;
  const int K = gs.cases ? gs.cases : 1;
  int rc = integrate_device(h, S.integ, gs.gradp, K, gs.q, st);
  if (rc) return rc;
  if (gs.cases) {
    const MeshCaseSet& m = h->mcs;
    PsmGradpCasesArgs a{};
    a.cells = gs.cells; a.cell_off = m.t.off; a.umax = m.d_umax; a.n_cases = m.n_cases; a.max_cells = m.args.max_cells;
    a.vtx_g2m = m.t.vtx_g2m; a.wts_g2m = m.t.wts_g2m; a.cell_of_point = m.t.cell_of_point; a.q = gs.q; a.near_wall = m.t.near_wall;
    a.p_out = gs.p; a.ny = h->Ny; a.nx = h->Nx; a.reference = S.reference; a.scalars = gs.scalars; a.sx = S.sx; a.sy = S.sy;
    HIPCHK(h, psm_launch_gradp_to_mesh_cases(a, st));
    return PSM_OK;
  }
  const MeshSingle& m = h->mesh;
  PsmGradpMeshArgs a{};
  a.cells = gs.cells; a.umax = m.d_umax; a.vtx = m.t.vtx_g2m; a.wts = m.t.wts_g2m; a.cell_of_point = m.t.cell_of_point; a.q = gs.q;
  a.near_wall = m.t.near_wall; a.p_out = gs.p; a.n_cells = h->n_cells; a.ny = h->Ny; a.nx = h->Nx; a.reference = S.reference;
  a.scalars = gs.scalars; a.sx = S.sx; a.sy = S.sy;
  HIPCHK(h, psm_launch_gradp_to_mesh(a, st));
  return PSM_OK;
}

// the binding and the form the entry serves (cases: 0 the single mesh, 1 a case set); one step in flight per handle, across all step kinds
static const BoundStepTexts kGradpTexts = {
    "the step is bound on a case set (psm_bind_gradp_solve_cases): use psm_solve_cases_gradp*",
    "the step is bound on the single mesh (psm_bind_gradp_solve): use psm_solve_gradp*",
    "psm_bind_gradp_solve_cases has not been called (a new case set, plan or model and, with apply_filter, psm_bind_poststeps drop the binding)",
    "psm_bind_gradp_solve has not been called (a new mesh, plan or model and, with apply_filter, psm_bind_poststeps drop the binding)"};

static int gradp_solve_state(psm_handle* h, int cases) {   // this kind also asks for the plan and the mesh of the form
  const bool usable = h->gsolve.ready && h->planned && (cases ? h->mcs.ready : h->have_geometry);
  return bound_step_state(h, kGradpTexts, h->gsolve.ready, h->gsolve.cases, usable, cases);
}

// One call on device buffers: the step's one graph replay.  Every check is made before anything is enqueued.  A case set: d_cells
// [sum n_i, 5], d_p [sum n_i], d_image [K][npix][3], d_gradp [K][npix][2], d_pgrid [K][npix], d_scalars [K][8].
static int gradp_solve_device(psm_handle* h, int cases, const double* d_cells, double* d_p, float* d_image, float* d_gradp, float* d_pgrid,
                              double* d_scalars, hipStream_t st) {
  int rc = gradp_solve_state(h, cases);
  if (rc) return rc;
  GradpSolveSet& S = h->gsolve;
  if (!d_cells || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!aligned_to(8, {d_cells, d_p, d_scalars, d_gradp}) || !aligned_to(4, {d_image, d_pgrid}))
    return fail(h, PSM_ERR_ARG, "a pointer is misaligned (8 bytes for the cells, p, the gradient and the scalars, 4 for the image and the plane)");
  if (S.apply_filter && !h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: apply_filter needs it as well as psm_bind_gradp_solve");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const int K = S.cases ? S.cases : 1;
  StepCall step;
  GradpSolveCall& gs = step.gsolve;
  gs.cells = d_cells; gs.p = d_p; gs.image = d_image ? d_image : S.d_image; gs.gradp = d_gradp ? d_gradp : S.integ.d_gradp;
  gs.q = d_pgrid ? d_pgrid : S.integ.d_p; gs.scalars = d_scalars ? d_scalars : S.d_scalars; gs.apply_filter = S.apply_filter; gs.cases = S.cases;
  if (S.apply_filter) step.post = post_call(1, nullptr, nullptr, gs.gradp, nullptr, nullptr);
  h->in_mesh_solve = true;                                 // the route psm_set_geometry* bound for psm_solve
  rc = solve_device(h, gs.image, K, nullptr, S.apply_filter ? h->post.d_fields : gs.gradp, st, nullptr, step);
  h->in_mesh_solve = false;
  return rc;
}

// A host call: one H2D copy of cells, the device call, one D2H copy of p, straight from / into ranges registered with
// psm_host_register, else through the pinned staging of the mesh or of the case set; synchronous.  `cases`: n is the set's sum n_i.
static int gradp_solve_host(psm_handle* h, int cases, const double* cells, int64_t n, double* p_out) {
  int rc = gradp_solve_state(h, cases);
  if (rc) return rc;
  if (!cells || !p_out) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!cases && n != h->n_cells) return fail(h, PSM_ERR_ARG, "cell count differs from the geometry");
  if (cases) n = h->mcs.off[h->mcs.n_cases];
  HIPCHK(h, hipSetDevice(h->cfg.device));
  MeshBuffers& m = cases ? static_cast<MeshBuffers&>(h->mcs) : static_cast<MeshBuffers&>(h->mesh);
  hipStream_t st = h->stream;
  const HostStaging s(h, m, cells, p_out, (size_t)n);
  HIPCHK(h, wait_stream(st));                                // the staging buffers are a step's too
  HIPCHK(h, s.copy_in(st));
  // no state turns over: a tripped guard (a geometry bound with psm_bind_geometry that is not the mesh's) runs the step again on the general path
  rc = guarded_host_step(h, st, cases ? "psm_solve_cases_gradp" : "psm_solve_gradp", [&](int) {
    const int rs = gradp_solve_device(h, cases, m.d_cells, m.d_p, nullptr, nullptr, nullptr, nullptr, st);
    if (rs) return rs;
    HIPCHK(h, s.copy_out(st));
    return PSM_OK;
  });
  if (rc) { (void)wait_stream(st); return rc; }
  s.deliver();
  return PSM_OK;
}

static bool scale_ok(double v) { return std::isfinite(v) && v != 0.0; }

// What the two bind entries do behind their own mesh checks, in the order of the header's error list; all-or-nothing.  `cases`: 0 the
// single mesh (one cut), K a case set (K cuts); sdfunct is the mesh's own host copy [K][npix].
static int gradp_solve_bind(psm_handle* h, const char* name, int cases, const std::vector<double>& sdfunct, const int32_t* cy, const int32_t* cx, double dx,
                            double dy, double extent_x, double extent_y, const double* max_abs_grad, int32_t apply_filter, int32_t reference) {
  if (apply_filter && !h->post.ready)
    return fail(h, PSM_ERR_STATE, std::string("psm_bind_poststeps has not been called: ") + name + " with apply_filter needs it");
  if (!cy || !cx || !max_abs_grad) return fail(h, PSM_ERR_ARG, "null argument");
  if (!scale_ok(dx) || !scale_ok(dy) || !scale_ok(extent_x) || !scale_ok(extent_y) || !scale_ok(max_abs_grad[0]) || !scale_ok(max_abs_grad[1]))
    return fail(h, PSM_ERR_ARG, "the spacings, the extents and max_abs_grad must be finite and non-zero");
  if (reference != PSM_GRADP_REF_NONE && reference != PSM_GRADP_REF_OUTLET) return fail(h, PSM_ERR_ARG, "reference must be PSM_GRADP_REF_NONE or PSM_GRADP_REF_OUTLET");
  const double sx = dx * max_abs_grad[0] / extent_x, sy = dy * max_abs_grad[1] / extent_y;
  if (!scale_ok(sx) || !scale_ok(sy) || !scale_ok((double)(float)sx) || !scale_ok((double)(float)sy))
    return fail(h, PSM_ERR_ARG, "the spacings, the extents and max_abs_grad must be finite and non-zero (so must dx max_abs_dPdx / extent_x and dy max_abs_dPdy / extent_y in float32)");
  if (h->mesh.inflight || h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a step is in flight on this handle: call psm_solve_end first");
  const int K = cases ? cases : 1;
  const size_t npix = (size_t)h->Ny * h->Nx;
  if (sdfunct.size() != (size_t)K * npix) return fail(h, PSM_ERR_STATE, "the mesh holds no copy of its sdfunct");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // a step in flight reads the tables that are replaced
  gradp_solve_free(h);
  GradpSolveSet& s = h->gsolve;
  // the tables first: a cut the reference cannot process (PSM_ERR_UNSUPPORTED) or outside the grid (PSM_ERR_ARG) binds nothing
  int rc = integ_bind(h, s.integ, h->Ny, h->Nx, sdfunct.data(), K, cy, cx, sx, sy);
  if (!rc) rc = dev_alloc(h, &s.d_image, (size_t)K * npix * 3);
  if (!rc) rc = dev_alloc(h, &s.d_scalars, (size_t)K * PSM_GRADP_SCALARS);
  if (rc) { gradp_solve_free(h); return rc; }
  if ((rc = bind_zero_sync(h, name, {{s.d_scalars, (size_t)K * PSM_GRADP_SCALARS * sizeof(double)}}, gradp_solve_free))) return rc;
  s.sx = sx; s.sy = sy; s.apply_filter = apply_filter ? 1 : 0; s.reference = reference; s.cases = cases;
  s.ready = true;
  return PSM_OK;
}

static int gradp_model_check(psm_handle* h) {
  if (h->cfg.variant != PSM_VARIANT_GRADP || h->cfg.c_in != 3 || h->cfg.c_out != 2 || h->cfg.sdf_channel != 2)
    return fail(h, PSM_ERR_UNSUPPORTED, "the gradient solver step needs the gradP model: PSM_VARIANT_GRADP with c_in == 3, c_out == 2, sdf_channel == 2");
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_gradp_solve(psm_handle* h, int32_t center_y, int32_t center_x, double dx, double dy, double extent_x, double extent_y,
                         const double* max_abs_grad, int32_t apply_filter, int32_t reference) {
  if (!h) return PSM_ERR_ARG;
  int rc = gradp_model_check(h);
  if (rc) return rc;
  if (h->mcs.ready) return fail(h, PSM_ERR_STATE, "the handle holds a case set (psm_set_geometry_cases): use psm_bind_gradp_solve_cases (psm_bind_gradp_solve takes the single mesh of psm_set_geometry)");
  if (!h->have_geometry || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (a new plan drops the mesh); a case set takes psm_bind_gradp_solve_cases");
  if (!h->have_g2m) return fail(h, PSM_ERR_ARG, "psm_set_geometry was called without the grid->mesh tables");
  return gradp_solve_bind(h, "psm_bind_gradp_solve", 0, h->mesh.h_sdf, &center_y, &center_x, dx, dy, extent_x, extent_y, max_abs_grad, apply_filter, reference);
}


int psm_bind_gradp_solve_cases(psm_handle* h, const int32_t* center_y, const int32_t* center_x, double dx, double dy, double extent_x, double extent_y,
                               const double* max_abs_grad, int32_t apply_filter, int32_t reference) {
  if (!h) return PSM_ERR_ARG;
  int rc = gradp_model_check(h);
  if (rc) return rc;
  if (h->have_geometry && !h->mcs.ready)
    return fail(h, PSM_ERR_STATE, "the handle holds the single mesh of psm_set_geometry: use psm_bind_gradp_solve (psm_bind_gradp_solve_cases needs a case set, psm_set_geometry_cases)");
  if (!h->mcs.ready || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry_cases has not been called (a new plan drops the case set); the single mesh takes psm_bind_gradp_solve");
  return gradp_solve_bind(h, "psm_bind_gradp_solve_cases", h->mcs.n_cases, h->mcs.h_sdf, center_y, center_x, dx, dy, extent_x, extent_y, max_abs_grad, apply_filter,
                          reference);
}


int psm_unbind_gradp_solve(psm_handle* h) {
  return unbind(h, [h] { gradp_solve_free(h); });
}


int psm_solve_gradp(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  (void)rank;
  return h ? gradp_solve_host(h, 0, cells, n, p_out) : PSM_ERR_ARG;
}


int psm_solve_gradp_device(psm_handle* h, const double* d_cells, double* d_p, float* d_image, float* d_gradp, float* d_pgrid, double* d_scalars,
                           void* stream) {
  return h ? gradp_solve_device(h, 0, d_cells, d_p, d_image, d_gradp, d_pgrid, d_scalars, stream_of(h, stream)) : PSM_ERR_ARG;
}


int psm_solve_cases_gradp(psm_handle* h, const double* cells, double* p_out) {
  return h ? gradp_solve_host(h, 1, cells, -1, p_out) : PSM_ERR_ARG;
}


int psm_solve_cases_gradp_device(psm_handle* h, const double* d_cells, double* d_p, float* d_image, float* d_gradp, float* d_pgrid, double* d_scalars,
                                 void* stream) {
  return h ? gradp_solve_device(h, 1, d_cells, d_p, d_image, d_gradp, d_pgrid, d_scalars, stream_of(h, stream)) : PSM_ERR_ARG;
}

}  // extern "C"
