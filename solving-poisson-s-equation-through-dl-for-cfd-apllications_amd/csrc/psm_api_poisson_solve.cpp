// psm_api_poisson_solve.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the Poisson-model step at the solver boundary, cells [N,5] -> p [N]
// (pressureSM_Poisson/SM_call.py:549-556, 815-818, 842-847), with U(t-1), dU(t-1) and p(t-2) kept on the device; on the single mesh
// (psm_solve_poisson*) and on a case set of K meshes (psm_solve_cases_poisson*).  See psm_handle.h for the map of the files.
//
// A step IS the chain of psm_poisson_step_device (psm_api_features.cpp: features x2, the 4-channel deltas solve, the post-steps) between
// two mesh ends of its own (psm_mesh.hip, PsmPoissonCellsArgs / PsmPoissonMeshArgs; PsmPoissonCasesArgs for a case set), in the same
// graph replay (StepCall::psolve): the head makes the six planes and the step's scalars from cells + state, the tail gathers dp back to
// the mesh and turns the state over.  A step with fewer than 1 + weighting held frames is a priming step: the tail alone as one plain
// launch, p = cells[:,4].  What lives here is the two bindings, the state's host counters and the argument blocks of the three
// launches.  The two forms share every function below: a case set is the single mesh with N = sum n_i, the chain run on K cases and
// the three launches in their case-batched form (PoissonSolveCall::cases).
#include "psm_handle.h"

namespace psm_impl {

// captured step graphs (StepCall::psolve) hold the addresses of the state, the partials and the scalar slots
static void drop_poisson_solve_graphs(psm_handle* h) { drop_graphs_if(h, [](const GraphKey& k) { return k.step.psolve.cells != nullptr; }); }

void poisson_solve_free(psm_handle* h) {
  PoissonSolveSet& s = h->psolve;
  drop_poisson_solve_graphs(h);
  dev_free(s.d_state); dev_free(s.d_part); dev_free(s.d_scalars);
  s.ready = false; s.cases = 0; s.frames = 0; s.steps = 0;
}

// The argument block of the three case-batched launches: the set's tables, the state and the planes of the feature and post-step
// bindings at their per-case strides.  `field`: what the tail gathers (null for the head and for a priming step).
static PsmPoissonCasesArgs cases_args(const psm_handle* h, const PoissonSolveCall& ps, const float* field) {
  const PoissonSolveSet& S = h->psolve;
  const MeshCaseSet& m = h->mcs;
  const int64_t total = m.off[m.n_cases];
  PsmPoissonCasesArgs a{};
  a.cells = ps.cells; a.cell_off = m.t.off; a.n_cases = m.n_cases; a.max_cells = m.args.max_cells; a.n_parts = psm_poisson_parts(m.args.max_cells);
  a.u_prev = S.d_state; a.du_prev = S.d_state + 2 * total; a.p_prev = S.d_state + 4 * total;
  a.partials = S.d_part;
  a.vtx_m2g = m.t.vtx_m2g; a.wts_m2g = m.t.wts_m2g; a.src_of_cell = m.t.src_of_cell; a.n_grid = (int64_t)h->Ny * h->Nx;
  a.vel = h->feat.d_vel;
  if (ps.weighting) { a.w_plane = h->post.d_dU; a.prev_plane = h->post.d_prev; }
  a.scalars = ps.scalars; a.lu = h->feat.d_lu; a.row_scale = h->ws0.d_row_scale; a.B = h->B;
  a.phi = S.phi; a.max_abs_dp = S.max_abs_dp; a.weighting = ps.weighting; a.frames = ps.frames; a.prime = ps.prime;
  a.vtx_g2m = m.t.vtx_g2m; a.wts_g2m = m.t.wts_g2m; a.cell_of_point = m.t.cell_of_point; a.field = field; a.near_wall = m.t.near_wall;
  a.p_out = ps.p;
  return a;
}

int poisson_solve_head(psm_handle* h, const PoissonSolveCall& ps, hipStream_t st) {
  if (ps.cases) {
    const PsmPoissonCasesArgs c = cases_args(h, ps, nullptr);
    HIPCHK(h, psm_launch_poisson_partial_cases(c, st));
    HIPCHK(h, psm_launch_poisson_to_grid_cases(c, st));
    return PSM_OK;
  }
  const PoissonSolveSet& S = h->psolve;
  const MeshTablesDev& t = h->mesh.t;
  const int64_t n = h->n_cells;
  PsmPoissonCellsArgs a{};
  a.cells = ps.cells; a.u_prev = S.d_state; a.du_prev = S.d_state + 2 * n; a.p_prev = S.d_state + 4 * n; a.n_cells = n;
  a.partials = S.d_part; a.n_partials = psm_poisson_parts(n);
  a.vtx = t.vtx_m2g; a.wts = t.wts_m2g; a.src_of_cell = t.src_of_cell; a.n_grid = (int64_t)h->Ny * h->Nx;
  a.vel = h->feat.d_vel;
  if (ps.weighting) { a.w_plane = h->post.d_dU; a.prev_plane = h->post.d_prev; }
  a.scalars = ps.scalars; a.lu = h->feat.d_lu; a.row_scale = h->ws0.d_row_scale; a.B = h->B;
  a.phi = S.phi; a.max_abs_dp = S.max_abs_dp; a.weighting = ps.weighting; a.frames = ps.frames;
  HIPCHK(h, psm_launch_poisson_partial(a, st));
  HIPCHK(h, psm_launch_poisson_to_grid(a, st));
  return PSM_OK;
}

static PsmPoissonMeshArgs tail_args(const psm_handle* h, const PoissonSolveCall& ps, const float* field) {
  const PoissonSolveSet& S = h->psolve;
  const MeshTablesDev& t = h->mesh.t;
  const int64_t n = h->n_cells;
  PsmPoissonMeshArgs a{};
  a.cells = ps.cells; a.vtx = t.vtx_g2m; a.wts = t.wts_g2m; a.cell_of_point = t.cell_of_point; a.field = field; a.near_wall = t.near_wall;
  a.p_out = ps.p; a.n_cells = n;
  a.u_prev = S.d_state; a.du_prev = S.d_state + 2 * n; a.p_prev = S.d_state + 4 * n;
  a.scalars = ps.scalars; a.prime = ps.prime; a.frames = ps.frames;
  return a;
}

// the tail launch of either form on `field` (null: the priming step)
static int tail_launch(psm_handle* h, const PoissonSolveCall& ps, const float* field, hipStream_t st) {
  if (ps.cases) HIPCHK(h, psm_launch_poisson_to_mesh_cases(cases_args(h, ps, field), st));
  else HIPCHK(h, psm_launch_poisson_to_mesh(tail_args(h, ps, field), st));
  return PSM_OK;
}

int poisson_solve_tail(psm_handle* h, const PoissonSolveCall& ps, const PostCall& pc, hipStream_t st) {
  return tail_launch(h, ps, ps.weighting ? pc.next : pc.result, st);   // SMP:842-847
}

// the mesh or the case set, the bindings under this one and this one; `cases`: the form the entry serves (-1: either)
static const BoundStepTexts kPoissonTexts = {
    "the step is bound on a case set (psm_bind_poisson_solve_cases): use psm_poisson_solve_push_cases / psm_solve_cases_poisson*",
    "the step is bound on the single mesh (psm_bind_poisson_solve): use psm_poisson_solve_push / psm_solve_poisson*",
    "psm_bind_poisson_solve_cases has not been called (a new case set, plan or model, psm_bind_features and psm_bind_poststeps drop the binding)",
    "psm_bind_poisson_solve has not been called (a new mesh, plan or model, psm_bind_features, psm_bind_poststeps and psm_bind_frames drop the binding)"};

static int poisson_solve_state(psm_handle* h, int cases) {
  return bound_step_state(h, kPoissonTexts, h->psolve.ready, h->psolve.cases, h->psolve.ready, cases);
}

// the whole frame is on the device: the counters move
static void frame_pushed(PoissonSolveSet& S) { S.frames = std::min(S.frames + 1, 2); }

// One call on device buffers: the priming launch, or the step's one graph replay.  Every check is made before anything is enqueued.
// A case set: d_cells [sum n_i, 5], d_p [sum n_i], d_fields [3][K][ny*nx], d_scalars [K][8]; one frame counter for all cases.
static int poisson_solve_device(psm_handle* h, int cases, const double* d_cells, double* d_p, float* d_fields, double* d_scalars, hipStream_t st, bool push_only) {
  int rc = poisson_solve_state(h, cases);
  if (rc) return rc;
  PoissonSolveSet& S = h->psolve;
  if (!d_cells || !d_p) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!aligned_to(8, {d_cells, d_p, d_scalars}) || !aligned_to(4, {d_fields}))
    return fail(h, PSM_ERR_ARG, "a pointer is misaligned (8 bytes for the cells, p and the scalars, 4 for the fields)");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const int K = S.cases ? S.cases : 1;
  PoissonSolveCall ps;
  ps.cells = d_cells; ps.p = d_p; ps.scalars = d_scalars ? d_scalars : S.d_scalars; ps.weighting = S.weighting; ps.frames = S.frames; ps.cases = S.cases;
  if (push_only || S.frames < 1 + S.weighting) {
    ps.prime = 1;
    if ((rc = tail_launch(h, ps, nullptr, st))) return rc;
    frame_pushed(S);
    return PSM_OK;
  }
  const size_t npix = (size_t)h->Ny * h->Nx, cap = (size_t)h->cfg.max_cases * npix * h->cfg.c_out;
  const PostSet& P = h->post;
  float* res = d_fields ? d_fields : P.d_out;
  const size_t stride = d_fields ? (size_t)K * npix : cap;
  const PostCall pc = S.weighting ? post_call(S.apply_filter, P.d_dU, P.d_prev, res, res + stride, res + 2 * stride)
                                  : post_call(S.apply_filter, nullptr, nullptr, res, nullptr, nullptr);
  if ((rc = poisson_step_device(h, h->feat.d_vel, K, nullptr, nullptr, pc, st, nullptr, nullptr, &ps))) return rc;
  frame_pushed(S);
  ++S.steps;
  return PSM_OK;
}

// A host call: one H2D copy of cells, the device call, one D2H copy of p (not for a push), straight from / into ranges registered with
// psm_host_register, else through the pinned staging of the mesh or of the case set; synchronous.  `cases`: n is the set's sum n_i.
static int poisson_solve_host(psm_handle* h, int cases, const double* cells, int64_t n, double* p_out, bool push_only) {
  int rc = poisson_solve_state(h, cases);
  if (rc) return rc;
  if (!cells || (!push_only && !p_out)) return fail(h, PSM_ERR_ARG, "null buffer");
  if (!cases && n != h->n_cells) return fail(h, PSM_ERR_ARG, "cell count differs from the geometry");
  if (cases) n = h->mcs.off[h->mcs.n_cases];
  HIPCHK(h, hipSetDevice(h->cfg.device));
  MeshBuffers& m = cases ? static_cast<MeshBuffers&>(h->mcs) : static_cast<MeshBuffers&>(h->mesh);
  hipStream_t st = h->stream;
  const HostStaging s(h, m, cells, push_only ? nullptr : p_out, (size_t)n);
  HIPCHK(h, wait_stream(st));                                // the staging buffers are a step's too
  HIPCHK(h, s.copy_in(st));
  if ((rc = poisson_solve_device(h, cases, m.d_cells, m.d_p, nullptr, nullptr, st, push_only))) { (void)wait_stream(st); return rc; }
  HIPCHK(h, s.copy_out(st));
  HIPCHK(h, wait_stream(st));
  if (guard_take(h, h->ws0)) {
    // The state has turned over with the step: it cannot run again on the general path as a grid-native solve does.
    if ((rc = guard_drop(h, cases ? "psm_solve_cases_poisson" : "psm_solve_poisson"))) return rc;
    return fail(h, PSM_ERR_STATE, h->err + "; the step's p is not valid and its frame was pushed: psm_poisson_solve_reset and prime again");
  }
  s.deliver();
  return PSM_OK;
}

// What the two bind entries do behind their own checks: the scalars' checks, nothing in flight, then the state (zeroed), the partials
// and the scalar slots for `total` cells and K rows (cases == 0: one row, the single mesh).
static int poisson_solve_bind(psm_handle* h, const char* name, int cases, size_t total, double phi, double max_abs_delta_p, int32_t weighting, int32_t apply_filter) {
  if (!(phi != 0.0) || !std::isfinite(phi) || !(max_abs_delta_p != 0.0) || !std::isfinite(max_abs_delta_p))
    return fail(h, PSM_ERR_ARG, "phi and max_abs_delta_p must be finite and non-zero");
  if (h->mesh.inflight || h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a step is in flight on this handle: call psm_solve_end first");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));           // a step in flight reads the state that is replaced
  poisson_solve_free(h);
  PoissonSolveSet& s = h->psolve;
  const size_t n = total, rows = cases ? (size_t)cases : 1;
  int rc;
  if ((rc = dev_alloc(h, &s.d_state, 5 * n)) || (rc = dev_alloc(h, &s.d_part, rows * 2 * PSM_POISSON_PARTS)) ||
      (rc = dev_alloc(h, &s.d_scalars, rows * PSM_POISSON_SCALARS))) { poisson_solve_free(h); return rc; }
  // the state is defined before the first push reads u_prev (and discards what it makes of it)
  if ((rc = bind_zero_sync(h, name, {{s.d_state, 5 * n * sizeof(double)}, {s.d_part, rows * 2 * PSM_POISSON_PARTS * sizeof(double)},
                                     {s.d_scalars, rows * PSM_POISSON_SCALARS * sizeof(double)}}, poisson_solve_free))) return rc;
  s.phi = phi; s.max_abs_dp = max_abs_delta_p; s.weighting = weighting ? 1 : 0; s.apply_filter = apply_filter ? 1 : 0;
  s.cases = cases;
  s.ready = true;
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_bind_poisson_solve(psm_handle* h, double phi, double max_abs_delta_p, int32_t weighting, int32_t apply_filter) {
  if (!h) return PSM_ERR_ARG;
  if (h->mcs.ready) return fail(h, PSM_ERR_STATE, "the handle holds a case set (psm_set_geometry_cases): the Poisson solver step takes the single mesh of psm_set_geometry");
  if (!h->have_geometry || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry has not been called (a new plan drops the mesh)");
  if (h->cfg.c_in != 4 || h->cfg.c_out != 1 || h->cfg.sdf_channel != 3)
    return fail(h, PSM_ERR_UNSUPPORTED, "the Poisson solver step needs the four-channel image with the SDF last and a one-channel field: c_in == 4, c_out == 1, sdf_channel == 3");
  if (!h->have_g2m) return fail(h, PSM_ERR_ARG, "psm_set_geometry was called without the grid->mesh tables");
  if (!h->feat.ready) return fail(h, PSM_ERR_STATE, "psm_bind_features has not been called: the Poisson solver step needs it as well as psm_bind_poststeps and psm_bind_frames");
  if (!h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: the Poisson solver step needs it as well as psm_bind_features and psm_bind_frames");
  if (!h->frames.ready || h->frames.k < 6)
    return fail(h, PSM_ERR_STATE, "psm_bind_frames has not been called with at least 6 columns: the Poisson solver step needs it as well as psm_bind_features and psm_bind_poststeps");
  return poisson_solve_bind(h, "psm_bind_poisson_solve", 0, (size_t)h->n_cells, phi, max_abs_delta_p, weighting, apply_filter);
}


int psm_bind_poisson_solve_cases(psm_handle* h, double phi, double max_abs_delta_p, int32_t weighting, int32_t apply_filter) {
  if (!h) return PSM_ERR_ARG;
  if (h->have_geometry && !h->mcs.ready)
    return fail(h, PSM_ERR_STATE, "the handle holds the single mesh of psm_set_geometry: use psm_bind_poisson_solve (psm_bind_poisson_solve_cases needs a case set, psm_set_geometry_cases)");
  if (!h->mcs.ready || !h->planned) return fail(h, PSM_ERR_STATE, "psm_set_geometry_cases has not been called (a new plan drops the case set)");
  if (h->cfg.c_in != 4 || h->cfg.c_out != 1 || h->cfg.sdf_channel != 3)
    return fail(h, PSM_ERR_UNSUPPORTED, "the Poisson solver step needs the four-channel image with the SDF last and a one-channel field: c_in == 4, c_out == 1, sdf_channel == 3");
  if (!h->feat.ready) return fail(h, PSM_ERR_STATE, "psm_bind_features has not been called: the Poisson solver step of a case set needs it as well as psm_bind_poststeps");
  if (h->feat.n_cases < h->mcs.n_cases)
    return fail(h, PSM_ERR_STATE, "psm_bind_features is bound for fewer cases (" + std::to_string(h->feat.n_cases) + ") than the case set holds (" + std::to_string(h->mcs.n_cases) + ")");
  if (!h->post.ready) return fail(h, PSM_ERR_STATE, "psm_bind_poststeps has not been called: the Poisson solver step of a case set needs it as well as psm_bind_features");
  return poisson_solve_bind(h, "psm_bind_poisson_solve_cases", h->mcs.n_cases, (size_t)h->mcs.off[h->mcs.n_cases], phi, max_abs_delta_p, weighting, apply_filter);
}


int psm_unbind_poisson_solve(psm_handle* h) {
  return unbind(h, [h] { poisson_solve_free(h); });
}


int psm_poisson_solve_push(psm_handle* h, const double* cells, int64_t n) {
  return h ? poisson_solve_host(h, 0, cells, n, nullptr, true) : PSM_ERR_ARG;
}


int psm_poisson_solve_push_cases(psm_handle* h, const double* cells) {
  return h ? poisson_solve_host(h, 1, cells, -1, nullptr, true) : PSM_ERR_ARG;
}


int psm_poisson_solve_reset(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  const int rc = poisson_solve_state(h, -1);
  if (rc) return rc;
  h->psolve.frames = 0; h->psolve.steps = 0;            // the arrays stay: the next push writes all of them before anything reads them
  return PSM_OK;
}


int psm_poisson_solve_state(const psm_handle* h, int32_t* frames, int64_t* steps) {
  if (!h) return PSM_ERR_ARG;
  if (frames) *frames = h->psolve.frames;
  if (steps) *steps = h->psolve.steps;
  return PSM_OK;
}


int psm_solve_poisson(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  (void)rank;
  return h ? poisson_solve_host(h, 0, cells, n, p_out, false) : PSM_ERR_ARG;
}


int psm_solve_poisson_device(psm_handle* h, const double* d_cells, double* d_p, float* d_fields, double* d_scalars, void* stream) {
  return h ? poisson_solve_device(h, 0, d_cells, d_p, d_fields, d_scalars, stream_of(h, stream), false) : PSM_ERR_ARG;
}


int psm_solve_cases_poisson(psm_handle* h, const double* cells, double* p_out) {
  return h ? poisson_solve_host(h, 1, cells, -1, p_out, false) : PSM_ERR_ARG;
}


int psm_solve_cases_poisson_device(psm_handle* h, const double* d_cells, double* d_p, float* d_fields, double* d_scalars, void* stream) {
  return h ? poisson_solve_device(h, 1, d_cells, d_p, d_fields, d_scalars, stream_of(h, stream), false) : PSM_ERR_ARG;
}

}  // extern "C"
