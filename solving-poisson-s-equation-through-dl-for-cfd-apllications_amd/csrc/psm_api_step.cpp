// psm_api_step.cpp -- libpsm_hip.so: the step around one solve -- solve_device puts the stages of a StepCall and the solve between them
// on one stream or into one cached graph; guarded_host_step is the loop every host entry runs it in.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

static int prepare_scale(psm_handle* h, Workspace& w, const float* out_scale, int n_cases, hipStream_t st, const float** d_scale) {
  if (!out_scale) { *d_scale = h->d_ones; return PSM_OK; }
  const int M = n_cases * h->B;
  const int slot = h->scale_pos;
  h->scale_pos = (h->scale_pos + 1) % psm_handle::RING;
  HIPCHK(h, hipEventSynchronize(h->scale_ev[slot]));
  for (int c = 0; c < n_cases; ++c)
    for (int b = 0; b < h->B; ++b) h->h_scale[slot][c * h->B + b] = out_scale[c];
  HIPCHK(h, hipMemcpyAsync(w.d_row_scale, h->h_scale[slot], (size_t)M * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipEventRecord(h->scale_ev[slot], st));
  *d_scale = w.d_row_scale;
  return PSM_OK;
}


// ---- captured sequences ---------------------------------------------------------------------------------------------
// The integer part of a captured sequence's cache key (GraphKey::n of solve_device, the key of a ring slot's graphs): the case
// count, whether a row scale is uploaded, whether the bound geometry applies and, for the ring, the DMA / pull form.  Everything
// else the route depends on is fixed while cached graphs live, because what changes it drops them: psm_plan_grid (free_plan), the
// model setters, psm_bind_geometry* / psm_unbind_geometry and a guard trip (destroy_graphs, which calls ring_drop_graphs), the
// integration, post-step and feature bind / unbind entries (the graphs that hold their tables); timed and profiled solves are never captured.
// Both per-solve switches, PSM_SDF_FOLD (fold_applies) and PSM_LN_FUSE, ARE part of the key, from the same read (`ps`) the route gets: a
// sequence captured under one value of either is never replayed under the other.
int sequence_key(const psm_handle* h, int n_cases, bool scale, const PsmSwitches::PerSolve& ps, bool ring) {
  const int k = (((n_cases * 2 + (scale ? 1 : 0)) * 2 + (bound_applies(h, n_cases) ? 1 : 0)) * 2 + (fold_applies(h, n_cases, ps) ? 1 : 0)) * 2 + (ps.ln_fuse ? 1 : 0);
  return ring ? k * 2 + (h->ring_dma ? 1 : 0) : k;
}

// Captures what `enqueue` puts on `st` into an executable graph.  The callable's own error comes first; the graph is destroyed on
// every arm.
int capture_graph(psm_handle* h, hipStream_t st, const char* label, const std::function<int()>& enqueue, hipGraphExec_t* exec) {
  hipGraph_t graph = nullptr;
  HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  const int rc = enqueue();
  hipError_t e = hipStreamEndCapture(st, &graph);
  hipGraphExec_t made = nullptr;
  if (!rc && e == hipSuccess) e = hipGraphInstantiate(&made, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (rc) return rc;
  if (e != hipSuccess) return fail(h, PSM_ERR_HIP, std::string(label) + " capture: " + hipGetErrorString(e));
  *exec = made;
  return PSM_OK;
}


// The combinations of stages the sequence below defines, as StepCall::fault spells them.
static int step_check(psm_handle* h, const StepCall& step) {
  const char* bad = step.fault();
  return bad ? fail(h, PSM_ERR_ARG, std::string("solve_device: ") + bad) : PSM_OK;
}

int solve_device(psm_handle* h, const float* d_grid, int n_cases, const float* out_scale, float* d_fields,
                 hipStream_t st, hipEvent_t* prof, const StepCall& step) {
  if (!h) return PSM_ERR_ARG;
  int rc = step_check(h, step);
  if (rc) return rc;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!d_grid || !d_fields) return fail(h, PSM_ERR_ARG, "null buffer");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (!st) st = h->stream;
  const PsmSwitches::PerSolve ps = psm_switches_per_solve();      // this solve's one read: the key and the route see the same values
  const float* d_scale = nullptr;
  if ((rc = ensure_encode_aux(h, n_cases))) return rc;
  const bool rows = step.rows.rows, psolve = step.psolve.cells, gsolve = step.gsolve.cells;
  if (step.rows.scaled() || psolve) d_scale = h->ws0.d_row_scale;   // the finish launch of the rows stage / the mesh -> grid launch of the Poisson solver step writes it, inside the sequence
  else if ((rc = prepare_scale(h, h->ws0, out_scale, n_cases, st, &d_scale))) return rc;
  const bool frames = step.frames.cols, feat = step.feat.vel, deltas = step.deltas.planes, gradp = step.gradp.planes, chapter4 = step.chapter4.planes, post = step.post.apply_filter >= 0;
  h->last_cases = gradp || chapter4 ? 1 : n_cases;  // gradp, chapter4: ws0 holds the last frame's single-case solve
  // psolve: the two head launches of the Poisson solver step in front of the features and its tail launch behind the post-steps;
  // gsolve: psm_solve's two head launches in front of the solve; behind the filter (if any) the two integration launches and the tail launch;
  // the two rows launches (rows), the mesh -> grid launch (frames), the two feature launches (feat) or the image pack (deltas, gradp, chapter4), the solve, then the two integration launches (p) or the
  // post-steps' (at most four); gradp: the filter among the post-steps and BEHIND it the integration with the gradp binding's tables: one linear chain
  auto sequence = [&](hipStream_t on, hipEvent_t* ev) {
    int rs = rows ? rows_device(h, step.rows, n_cases, on) : PSM_OK;
    if (!rs && frames) rs = frames_device(h, step.frames, n_cases, on);
    if (!rs && psolve) rs = poisson_solve_head(h, step.psolve, on);
    if (!rs && gsolve) rs = gradp_solve_head(h, step.gsolve, on);
    if (!rs && feat) rs = features_device(h, step.feat.vel, n_cases, step.feat.grid, on);
    if (!rs && deltas) rs = deltas_pack_device(h, step.deltas, n_cases, on);
    if (!rs && gradp) rs = gradp_pack_device(h, step.gradp, n_cases, on);
    if (!rs && chapter4) rs = chapter4_pack_device(h, step.chapter4, n_cases, on);
    if (!rs && (deltas || gradp || chapter4)) {
      // An evaluator's frames are solved ONE BY ONE, each as the single case Evaluation.timeStep / EvaluationGradP.timeStep / EvaluationChapter4.timeStep solves on
      // its image (with a geometry bound for one case: the 6-launch route with the folded encode), so that a frame's field holds the
      // bits of that call whatever the batch.  deltas: the network output rows of every frame are kept for the block stage, which
      // decodes them again.
      const size_t npix = (size_t)h->Ny * h->Nx, rows = (size_t)h->B * h->ld_out;
      for (int f = 0; f < n_cases && !rs; ++f) {
        rs = launch_all(h, h->ws0, d_grid + f * npix * h->cfg.c_in, 1, d_fields + f * npix * h->cfg.c_out, d_scale + (d_scale == h->d_ones ? 0 : f * h->B), on, ev, ps);
        if (!rs && deltas && hipMemcpyAsync(step.deltas.res + f * rows, h->ws0.d_res, rows * sizeof(float), hipMemcpyDeviceToDevice, on) != hipSuccess)
          rs = fail(h, PSM_ERR_HIP, "psm_deltas_frames: copy of the network output");
      }
      if (deltas) {
        h->last.pred_stored = false;      // ws0.d_pred holds the last frame's blocks at most
        h->last.row_scale = d_scale;
        h->last.res = step.deltas.res;
      }
    } else if (!rs) rs = launch_all(h, h->ws0, d_grid, n_cases, d_fields, d_scale, on, ev, ps);
    if (!rs && step.p) rs = integrate_device(h, d_fields, n_cases, step.p, on);
    if (!rs && post) rs = poststeps_device(h, d_fields, n_cases, step.post, on);
    if (!rs && gradp) rs = integrate_device(h, h->gradp.integ, post ? step.post.result : d_fields, n_cases, step.gradp.p, on);
    if (!rs && psolve) rs = poisson_solve_tail(h, step.psolve, step.post, on);
    if (!rs && gsolve) rs = gradp_solve_tail(h, step.gsolve, on);
    return rs;
  };
  if (prof || h->timed_kernel >= 0 || !h->use_graph) return sequence(st, prof);
  const GraphKey key{sequence_key(h, n_cases, d_scale != h->d_ones, ps), d_grid, d_fields, step};
  auto it = h->graphs.find(key);
  if (it == h->graphs.end()) {
    if (h->graphs.size() > 64) destroy_graphs(h);
    hipGraphExec_t exec = nullptr;
    if ((rc = capture_graph(h, h->stream, "solve", [&] { return sequence(h->stream, nullptr); }, &exec))) return rc;
    it = h->graphs.emplace(key, psm_handle::SolveGraph{exec, h->last}).first;   // launch_all ran for the capture
  } else {
    h->last = it->second.left;                    // a replay runs no host code of launch_all
  }
  HIPCHK(h, hipGraphLaunch(it->second.exec, st));
  return PSM_OK;
}


// ---- guard of the bound-geometry contract, host side -------------------------------------------------------------
// true once per trip: a guard wave of a solve on workspace `w` found a grid whose flow-cell pattern is not the bound one
bool guard_take(psm_handle* h, Workspace& w) {
  if (!h->h_guard) return false;
  volatile int* f = h->h_guard + w.gidx;
  if (!*f) return false;
  *f = 0;
  return true;
}

// drop the binding: the following solves (and the re-run of the one that tripped) take the general path
int guard_drop(psm_handle* h, const char* where) {
  ++h->guard_trips;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  destroy_graphs(h);
  h->bound = false;
  h->fold_bound = false;
  h->err = std::string(where) + ": the grid's flow-cell pattern (SDF channel != 0; with the SDF fold, the SDF channel's values) is not the one bound with psm_bind_geometry; the binding was dropped";
  return PSM_OK;
}

int guarded_host_step(psm_handle* h, hipStream_t st, const char* where, const std::function<int(int pass)>& enqueue) {
  for (int pass = 0; pass < 2; ++pass) {
    int rc = enqueue(pass);
    if (rc) return rc;
    HIPCHK(h, wait_stream(st));
    if (pass == 1 || !guard_take(h, h->ws0)) break;     // not the bound geometry: the field is NaN -- drop the binding, solve again on the general path
    if ((rc = guard_drop(h, where))) return rc;
    h->err += " (solved on the general path)";
  }
  return PSM_OK;
}

int unbind(psm_handle* h, const std::function<void()>& free_fn) {
  if (!h) return PSM_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_fn();
  return PSM_OK;
}

}  // namespace psm_impl
