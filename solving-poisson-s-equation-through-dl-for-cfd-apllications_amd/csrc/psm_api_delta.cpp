// psm_api_delta.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the delta step at the solver boundary, [U(t) - U(t-1)], SDF -> p(t) - p(t-1)
// (pressureSM_deltas/SM_call.py:389-391), with U(t-1) kept on the device.  See psm_handle.h for the map of the files.
//
// A delta step IS the step of psm_solve / psm_solve_cases (psm_api_mesh.cpp: mesh_step_begin, cases_step_*) with the two mesh ends in
// their delta form (psm_mesh.hip): the same checks, copies and launches, no launch of its own.  What lives here is the state: who
// may set it, forget it and ask for it.  The state's array is allocated with the geometry and goes with it (delta_drop).
#include "psm_handle.h"

namespace {

// U(t-1) := cells[:,0:2] for `total` cells: the two columns packed through pinned staging (`stage` holds [total][5]), nothing else
// of `cells` is read.  Nothing of this handle may be in flight: the copy is ordered behind the handle's stream and waited for.
int prime_from_host(psm_handle* h, const double* cells, int64_t total, double* stage) {
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, wait_stream(h->stream));                       // the staging buffer is a step's too
  for (int64_t i = 0; i < total; ++i) { stage[2 * i] = cells[5 * i]; stage[2 * i + 1] = cells[5 * i + 1]; }
  HIPCHK(h, hipMemcpyAsync(h->delta.d_u_prev, stage, (size_t)total * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, wait_stream(h->stream));
  h->delta.primed = true;
  return PSM_OK;
}

}  // namespace

extern "C" {

int psm_delta_prime(psm_handle* h, const double* cells, int64_t n) {
  if (!h) return PSM_ERR_ARG;
  const int rc = mesh_step_check(h, cells, n, nullptr, true);
  return rc ? rc : prime_from_host(h, cells, n, h->mesh.h_cells);
}


int psm_delta_prime_cases(psm_handle* h, const double* cells) {
  if (!h) return PSM_ERR_ARG;
  if (h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a step is in flight on this handle: call psm_solve_cases_end first");
  const int rc = cases_check(h);
  if (rc) return rc;
  if (!cells) return fail(h, PSM_ERR_ARG, "null buffer");
  return prime_from_host(h, cells, h->mcs.off[h->mcs.n_cases], h->mcs.h_cells);
}


int psm_delta_reset(psm_handle* h) {
  if (!h) return PSM_ERR_ARG;
  if (h->mesh.inflight || h->mcs.inflight) return fail(h, PSM_ERR_STATE, "a step is in flight on this handle: end it first");
  h->delta.primed = false; h->delta.steps = 0;             // the array stays: the next step writes all of it before anything reads it
  return PSM_OK;
}


int psm_delta_state(const psm_handle* h, int32_t* primed, int64_t* steps) {
  if (!h) return PSM_ERR_ARG;
  if (primed) *primed = h->delta.primed ? 1 : 0;
  if (steps) *steps = h->delta.steps;
  return PSM_OK;
}


int psm_solve_delta_begin(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  (void)rank;
  return h ? mesh_step_begin(h, cells, n, p_out, true) : PSM_ERR_ARG;
}

int psm_solve_delta_end(psm_handle* h) { return psm_solve_end(h); }   // one step in flight per handle, either kind: either end completes it

int psm_solve_delta(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out) {
  const int rc = psm_solve_delta_begin(h, cells, n, rank, p_out);
  return rc ? rc : psm_solve_end(h);
}


int psm_solve_cases_delta_device(psm_handle* h, const double* d_cells, double* d_p, void* stream) {
  return h ? cases_step_device(h, d_cells, d_p, stream, true) : PSM_ERR_ARG;
}

int psm_solve_cases_delta_begin(psm_handle* h, const double* cells, double* p_out) {
  return h ? cases_step_begin(h, cells, p_out, true) : PSM_ERR_ARG;
}

int psm_solve_cases_delta_end(psm_handle* h) { return psm_solve_cases_end(h); }

int psm_solve_cases_delta(psm_handle* h, const double* cells, double* p_out) {
  const int rc = psm_solve_cases_delta_begin(h, cells, p_out);
  return rc ? rc : psm_solve_cases_end(h);
}

}  // extern "C"
