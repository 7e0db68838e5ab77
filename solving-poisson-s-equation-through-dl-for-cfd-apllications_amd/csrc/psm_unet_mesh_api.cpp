// psm_unet_mesh_api.cpp -- the convolutional path at the solver boundary (include/psm_unet.h, psm_unet_mesh_*, psm_unet_solve*): a
// mesh binding ON TOP of a planned psm_unet.  It reaches the network through the public entries of psm_unet.h alone
// (psm_unet_num_convs, psm_unet_conv_shape, psm_unet_flops, psm_unet_forward_device), so psm_unet_api.cpp and the conv kernels are
// what they were; the tables come from psm_build_mesh_case_tables (psm_mesh_tables.cpp, pure host), the first launch of a step is
// psm_launch_umax_cases (psm_mesh.hip) and the two ends around the network are psm_unet_mesh.hip's.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "psm_alloc.h"

#include "../../include/psm.h"
#include "../../include/psm_unet.h"
#include "psm_mesh.h"
#include "psm_mesh_tables.h"
#include "psm_switches.h"
#include "psm_unet_mesh.h"

namespace {
// What psm_unet_mesh_set_geometry puts on the device and reserves for the steps: replaced as a whole, so a refused or failed call
// leaves the binding as it was.
struct Geometry {
  int n_cases = 0, ny = 0, nx = 0;
  int64_t total = 0;
  std::vector<int64_t> off;
  int64_t* d_off = nullptr;
  int32_t *d_vtx_m2g = nullptr, *d_src_of_cell = nullptr, *d_pixel_of_point = nullptr, *d_vtx_g2m = nullptr;
  double *d_wts_m2g = nullptr, *d_sdf = nullptr, *d_wts_g2m = nullptr;
  uint8_t* d_near_wall = nullptr;
  double *d_umax_part = nullptr, *d_umax = nullptr, *d_u_prev = nullptr;
  double *d_cells = nullptr, *d_p = nullptr, *h_cells = nullptr, *h_p = nullptr;   // staging of the host entries
  PsmUnetMeshArgs args{};
};
thread_local std::string g_err;
}  // namespace

struct psm_unet_mesh {
  psm_unet* u = nullptr;
  int device = 0, ny_c = 0, nx_c = 0, max_cases = 0, step = 0;
  float *d_canvas = nullptr, *d_field = nullptr;   // [max_cases][ny_c][nx_c][3] | [max_cases][ny_c][nx_c]
  Geometry g;
  bool ready = false, ran = false;                 // a geometry is set | a step has run the network on it
  bool primed = false;
  int64_t steps = 0;
  hipStream_t stream = nullptr;
  std::string err;
};

namespace {
int fail(psm_unet_mesh* m, int code, const std::string& msg) { if (m) m->err = msg; else g_err = msg; return code; }
#define MCHK(m, expr)                                                                                   \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail((m), PSM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

void free_geometry(Geometry& g) {
  for (void* p : {(void*)g.d_off, (void*)g.d_vtx_m2g, (void*)g.d_src_of_cell, (void*)g.d_pixel_of_point, (void*)g.d_vtx_g2m, (void*)g.d_wts_m2g, (void*)g.d_sdf,
                  (void*)g.d_wts_g2m, (void*)g.d_near_wall, (void*)g.d_umax_part, (void*)g.d_umax, (void*)g.d_u_prev, (void*)g.d_cells, (void*)g.d_p})
    if (p) (void)psm_dev_free(p);
  if (g.h_cells) (void)hipHostFree(g.h_cells);
  if (g.h_p) (void)hipHostFree(g.h_p);
  g = Geometry{};
}
template <class T, class V> hipError_t upload(T** p, const V& v) {
  hipError_t e = psm_dev_malloc((void**)p, v.size() * sizeof(v[0]));
  return e != hipSuccess ? e : psm_copy_h2d(*p, v.data(), v.size() * sizeof(v[0]));
}
int round_up(int v, int m) { return (v + m - 1) / m * m; }

// resolution level of convolution idx of an L-level network (the order of psm_unet.h: enc0a .. enc{L-1}b, dec{L-2}a .. dec0b, head)
int conv_level(int idx, int L, int n_convs) { return idx < 2 * L ? idx / 2 : idx == n_convs - 1 ? 0 : L - 2 - (idx - 2 * L) / 2; }

// synchronous entries of a few hundred us: poll instead of sleeping (psm_unet_forward does the same); PSM_SYNC_BLOCK=1 blocks
hipError_t wait_stream(hipStream_t st) {
  if (psm_switches_process().sync_block == 1) return hipStreamSynchronize(st);
  hipError_t e;
  while ((e = hipStreamQuery(st)) == hipErrorNotReady) { }
  return e;
}

// One step, a linear chain on `st`: partial maxima, mesh -> canvas, the network, canvas -> mesh; a delta step on a state that is not
// primed is the last launch alone.  Copies nothing and waits for nothing; the state's host flags move once all is enqueued.
int sequence(psm_unet_mesh* m, const double* d_cells, double* d_p, hipStream_t st) {
  const bool delta = m->step == PSM_UNET_STEP_DELTA;
  PsmUnetMeshArgs a = m->g.args;
  a.cells = d_cells; a.p_out = d_p; a.prime = delta && !m->primed;
  if (!a.prime) {
    PsmMeshCasesArgs c{};
    c.cells = d_cells; c.cell_off = a.cell_off; c.umax_part = a.umax_part; c.n_parts = a.n_parts; c.n_cases = a.n_cases;
    MCHK(m, psm_launch_umax_cases(c, st));
    MCHK(m, psm_launch_unet_to_canvas(a, delta, st));
    const int rc = psm_unet_forward_device(m->u, m->d_canvas, a.n_cases, m->d_field, st);
    if (rc) return fail(m, rc, std::string("psm_unet_forward_device: ") + psm_unet_last_error(m->u));
    m->ran = true;
  }
  MCHK(m, psm_launch_unet_to_mesh(a, delta, st));
  if (delta) { m->steps += m->primed; m->primed = true; }
  return PSM_OK;
}

int need_geometry(psm_unet_mesh* m) {
  return m->ready ? PSM_OK : fail(m, PSM_ERR_STATE, "psm_unet_mesh_set_geometry has not been called");
}
}  // namespace

extern "C" {

const char* psm_unet_mesh_last_error(const psm_unet_mesh* m) { return m ? m->err.c_str() : g_err.c_str(); }

int psm_unet_canvas_shape(int32_t n_levels, int32_t ny, int32_t nx, int32_t* ny_c, int32_t* nx_c) {
  if (n_levels < 2 || n_levels > 7 || ny < 1 || nx < 1 || ny > (1 << 24) || nx > (1 << 24) || !ny_c || !nx_c) return PSM_ERR_ARG;
  const int mult = 1 << (n_levels - 1);
  *ny_c = round_up(ny, mult); *nx_c = round_up(nx, mult);
  return PSM_OK;
}

int psm_unet_mesh_create(psm_unet* u, int32_t device, int32_t ny_c, int32_t nx_c, int32_t max_cases, int32_t step, psm_unet_mesh** out) {
  if (!out) return fail(nullptr, PSM_ERR_ARG, "null argument");
  *out = nullptr;
  if (!u) return fail(nullptr, PSM_ERR_ARG, "null network handle");
  if (step != PSM_UNET_STEP_ABSOLUTE && step != PSM_UNET_STEP_DELTA) return fail(nullptr, PSM_ERR_ARG, "step must be PSM_UNET_STEP_ABSOLUTE or PSM_UNET_STEP_DELTA");
  const int64_t flops = psm_unet_flops(u);
  if (flops <= 0) return fail(nullptr, PSM_ERR_STATE, "the network is not planned: call psm_unet_plan for the canvas first");
  const int n = psm_unet_num_convs(u), L = (n + 1) / 4;
  int32_t k = 0, ci = 0, co = 0, head_out = 0;
  if (n < 7 || psm_unet_conv_shape(u, n - 1, &k, &ci, &head_out) || psm_unet_conv_shape(u, 0, &k, &ci, &co)) return fail(nullptr, PSM_ERR_ARG, "cannot read the network's layers");
  if (ci != 3 || head_out != 1)
    return fail(nullptr, PSM_ERR_UNSUPPORTED, "the mesh entry needs a stem with c_in == 3 and a head with c_out == 1 (python_module.py:288-292)");
  const int mult = 1 << (L - 1);
  if (ny_c < mult || nx_c < mult || ny_c % mult || nx_c % mult) return fail(nullptr, PSM_ERR_ARG, "ny_c and nx_c must be multiples of 2^(n_levels-1): see psm_unet_canvas_shape");
  if (max_cases < 1 || (int64_t)ny_c * nx_c * max_cases > ((int64_t)1 << 28)) return fail(nullptr, PSM_ERR_ARG, "bad case batch");
  int64_t want = 0;
  for (int i = 0; i < n; ++i) {
    if (psm_unet_conv_shape(u, i, &k, &ci, &co)) return fail(nullptr, PSM_ERR_ARG, "cannot read the network's layers");
    const int lv = conv_level(i, L, n);
    want += 2LL * (ny_c >> lv) * (nx_c >> lv) * k * k * ci * co;
  }
  if (want != flops) return fail(nullptr, PSM_ERR_ARG, "the network is planned for another image size than the canvas ny_c x nx_c");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(nullptr, PSM_ERR_ARG, "device ordinal out of range");
  psm_unet_mesh* m = new psm_unet_mesh();
  m->u = u; m->device = device; m->ny_c = ny_c; m->nx_c = nx_c; m->max_cases = max_cases; m->step = step;
  const size_t npix = (size_t)ny_c * nx_c * max_cases;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = psm_dev_malloc((void**)&m->d_canvas, npix * 3 * sizeof(float));
  if (e == hipSuccess) e = psm_dev_malloc((void**)&m->d_field, npix * sizeof(float));
  if (e != hipSuccess) {
    const std::string why = std::string("canvas buffers: ") + hipGetErrorString(e);
    psm_unet_mesh_destroy(m);
    return fail(nullptr, PSM_ERR_HIP, why);
  }
  *out = m;
  return PSM_OK;
}

void psm_unet_mesh_destroy(psm_unet_mesh* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  free_geometry(m->g);
  if (m->d_canvas) (void)psm_dev_free(m->d_canvas);
  if (m->d_field) (void)psm_dev_free(m->d_field);
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;
}

int psm_unet_mesh_set_geometry(psm_unet_mesh* m, int32_t n_cases, const int64_t* n_cells, int32_t ny, int32_t nx,
                               const int32_t* const* vtx_m2g, const double* const* wts_m2g, const int32_t* const* indices,
                               const double* const* sdfunct, const int32_t* const* vtx_g2m, const double* const* wts_g2m,
                               const double* maxs, int32_t normalise_sdf, int32_t fill_input, double wall_threshold) {
  if (!m) return PSM_ERR_ARG;
  if (!n_cells || !vtx_m2g || !wts_m2g || !indices || !sdfunct || !vtx_g2m || !wts_g2m || !maxs) return fail(m, PSM_ERR_ARG, "null geometry table");
  if (n_cases < 1 || n_cases > m->max_cases) return fail(m, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  if (ny < 1 || nx < 1) return fail(m, PSM_ERR_ARG, "bad grid shape");
  const int mult = 1 << ((psm_unet_num_convs(m->u) + 1) / 4 - 1);
  if (round_up(ny, mult) != m->ny_c || round_up(nx, mult) != m->nx_c)
    return fail(m, PSM_ERR_ARG, "the canvas of a " + std::to_string(ny) + " x " + std::to_string(nx) + " grid is " + std::to_string(round_up(ny, mult)) + " x " +
                                    std::to_string(round_up(nx, mult)) + ", the binding was created for " + std::to_string(m->ny_c) + " x " + std::to_string(m->nx_c));
  for (int k = 0; k < 4; ++k) if (!(maxs[k] != 0.0)) return fail(m, PSM_ERR_ARG, "maxs must be non-zero");
  // everything that needs no device first: a bad table leaves the binding as it was
  std::vector<PsmMeshCaseInput> in(n_cases);
  for (int k = 0; k < n_cases; ++k) in[k] = PsmMeshCaseInput{n_cells[k], vtx_m2g[k], wts_m2g[k], indices[k], sdfunct[k], vtx_g2m[k], wts_g2m[k]};
  PsmMeshCaseTables t;
  std::string why;
  const double sdf_scale = normalise_sdf ? 1.0 / maxs[2] : 1.0;
  if (psm_build_mesh_case_tables(n_cases, in.data(), ny, nx, sdf_scale, wall_threshold, t, why)) return fail(m, PSM_ERR_ARG, why);
  // cell_of_point is ii * nx + jj: the tail reads the field at canvas pitch
  std::vector<int32_t> pixel(t.cell_of_point.size());
  for (size_t q = 0; q < pixel.size(); ++q) pixel[q] = (t.cell_of_point[q] / nx) * m->nx_c + t.cell_of_point[q] % nx;
  MCHK(m, hipSetDevice(m->device));
  MCHK(m, hipStreamSynchronize(m->stream));
  Geometry g;
  g.n_cases = n_cases; g.ny = ny; g.nx = nx; g.total = t.total; g.off = t.cell_off;
  const int n_parts = (int)std::min<int64_t>(PSM_MESH_CASE_PARTS, (t.max_cells + 4095) / 4096);
  const size_t N = (size_t)t.total;
  hipError_t e = upload(&g.d_off, t.cell_off);
  if (e == hipSuccess) e = upload(&g.d_vtx_m2g, t.vtx_m2g);
  if (e == hipSuccess) e = upload(&g.d_wts_m2g, t.wts_m2g);
  if (e == hipSuccess) e = upload(&g.d_src_of_cell, t.src_of_cell);
  if (e == hipSuccess) e = upload(&g.d_sdf, t.sdf);
  if (e == hipSuccess) e = upload(&g.d_pixel_of_point, pixel);
  if (e == hipSuccess) e = upload(&g.d_vtx_g2m, t.vtx_g2m);
  if (e == hipSuccess) e = upload(&g.d_wts_g2m, t.wts_g2m);
  if (e == hipSuccess) e = upload(&g.d_near_wall, t.near_wall);
  if (e == hipSuccess) e = psm_dev_malloc((void**)&g.d_umax_part, (size_t)n_cases * n_parts * sizeof(double));
  if (e == hipSuccess) e = psm_dev_malloc((void**)&g.d_umax, (size_t)n_cases * sizeof(double));
  if (e == hipSuccess && m->step == PSM_UNET_STEP_DELTA) e = psm_dev_malloc((void**)&g.d_u_prev, N * 2 * sizeof(double));
  if (e == hipSuccess) e = psm_dev_malloc((void**)&g.d_cells, N * 5 * sizeof(double));
  if (e == hipSuccess) e = psm_dev_malloc((void**)&g.d_p, N * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&g.h_cells, N * 5 * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&g.h_p, N * sizeof(double), hipHostMallocDefault);
  // the padding: every canvas pixel is +0.0 from here on, the steps write the image region alone
  if (e == hipSuccess) e = hipMemsetAsync(m->d_canvas, 0, (size_t)m->max_cases * m->ny_c * m->nx_c * 3 * sizeof(float), m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  if (e != hipSuccess) { free_geometry(g); return fail(m, PSM_ERR_HIP, std::string("geometry tables: ") + hipGetErrorString(e)); }
  PsmUnetMeshArgs& a = g.args;
  a.cell_off = g.d_off; a.umax_part = g.d_umax_part; a.umax = g.d_umax; a.n_parts = n_parts; a.n_cases = n_cases;
  a.vtx_m2g = g.d_vtx_m2g; a.wts_m2g = g.d_wts_m2g; a.src_of_cell = g.d_src_of_cell; a.sdf = g.d_sdf; a.canvas = m->d_canvas;
  a.ny = ny; a.nx = nx; a.ny_c = m->ny_c; a.nx_c = m->nx_c;
  a.max_abs_ux = maxs[0]; a.max_abs_uy = maxs[1]; a.sdf_scale = sdf_scale; a.fill = fill_input;
  a.vtx_g2m = g.d_vtx_g2m; a.wts_g2m = g.d_wts_g2m; a.pixel_of_point = g.d_pixel_of_point; a.field = m->d_field; a.near_wall = g.d_near_wall;
  a.max_cells = t.max_cells; a.max_abs_p = maxs[3]; a.u_prev = g.d_u_prev;
  free_geometry(m->g);
  m->g = std::move(g);
  m->ready = true; m->ran = false; m->primed = false; m->steps = 0;
  return PSM_OK;
}

int psm_unet_solve_device(psm_unet_mesh* m, const double* d_cells, double* d_p, void* stream) {
  if (!m) return PSM_ERR_ARG;
  int rc = need_geometry(m);
  if (rc) return rc;
  if (!d_cells || !d_p) return fail(m, PSM_ERR_ARG, "null buffer");
  if ((reinterpret_cast<uintptr_t>(d_cells) | reinterpret_cast<uintptr_t>(d_p)) & 7) return fail(m, PSM_ERR_ARG, "device buffers must be 8-byte aligned");
  MCHK(m, hipSetDevice(m->device));
  return sequence(m, d_cells, d_p, stream ? (hipStream_t)stream : m->stream);
}

int psm_unet_solve(psm_unet_mesh* m, const double* cells, double* p_out) {
  if (!m) return PSM_ERR_ARG;
  int rc = need_geometry(m);
  if (rc) return rc;
  if (!cells || !p_out) return fail(m, PSM_ERR_ARG, "null buffer");
  Geometry& g = m->g;
  const size_t N = (size_t)g.total;
  MCHK(m, hipSetDevice(m->device));
  std::memcpy(g.h_cells, cells, N * 5 * sizeof(double));
  MCHK(m, hipMemcpyAsync(g.d_cells, g.h_cells, N * 5 * sizeof(double), hipMemcpyHostToDevice, m->stream));
  if ((rc = sequence(m, g.d_cells, g.d_p, m->stream))) return rc;
  MCHK(m, hipMemcpyAsync(g.h_p, g.d_p, N * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  MCHK(m, wait_stream(m->stream));
  std::memcpy(p_out, g.h_p, N * sizeof(double));
  return PSM_OK;
}

int psm_unet_mesh_prime(psm_unet_mesh* m, const double* cells) {
  if (!m) return PSM_ERR_ARG;
  if (m->step != PSM_UNET_STEP_DELTA) return fail(m, PSM_ERR_STATE, "the binding was created with PSM_UNET_STEP_ABSOLUTE: the state belongs to the delta step");
  const int rc = need_geometry(m);
  if (rc) return rc;
  if (!cells) return fail(m, PSM_ERR_ARG, "null buffer");
  Geometry& g = m->g;
  MCHK(m, hipSetDevice(m->device));
  MCHK(m, wait_stream(m->stream));                         // the staging buffer is a step's too
  for (int64_t i = 0; i < g.total; ++i) { g.h_cells[2 * i] = cells[5 * i]; g.h_cells[2 * i + 1] = cells[5 * i + 1]; }
  MCHK(m, hipMemcpyAsync(g.d_u_prev, g.h_cells, (size_t)g.total * 2 * sizeof(double), hipMemcpyHostToDevice, m->stream));
  MCHK(m, wait_stream(m->stream));
  m->primed = true;
  return PSM_OK;
}

int psm_unet_mesh_reset(psm_unet_mesh* m) {
  if (!m) return PSM_ERR_ARG;
  if (m->step != PSM_UNET_STEP_DELTA) return fail(m, PSM_ERR_STATE, "the binding was created with PSM_UNET_STEP_ABSOLUTE: the state belongs to the delta step");
  m->primed = false; m->steps = 0;                         // the array stays: the next step writes all of it before anything reads it
  return PSM_OK;
}

int psm_unet_mesh_state(const psm_unet_mesh* m, int32_t* primed, int64_t* steps) {
  if (!m) return PSM_ERR_ARG;
  if (primed) *primed = m->primed ? 1 : 0;
  if (steps) *steps = m->steps;
  return PSM_OK;
}

int psm_unet_mesh_read(psm_unet_mesh* m, int32_t what, void* dst, int64_t cap) {
  if (!m) return PSM_ERR_ARG;
  if (!dst) return fail(m, PSM_ERR_ARG, "null buffer");
  if (!m->ready || !m->ran) return fail(m, PSM_ERR_STATE, "no step has run the network on this geometry yet");
  const int64_t npix = (int64_t)m->g.n_cases * m->ny_c * m->nx_c;
  const void* src = nullptr;
  int64_t bytes = 0;
  switch (what) {
    case PSM_UNET_READ_CANVAS: src = m->d_canvas; bytes = npix * 3 * (int64_t)sizeof(float); break;
    case PSM_UNET_READ_FIELD: src = m->d_field; bytes = npix * (int64_t)sizeof(float); break;
    case PSM_UNET_READ_UMAX: src = m->g.d_umax; bytes = m->g.n_cases * (int64_t)sizeof(double); break;
    default: return fail(m, PSM_ERR_ARG, "unknown quantity");
  }
  if (cap < bytes) return fail(m, PSM_ERR_ARG, "destination too small");
  MCHK(m, hipSetDevice(m->device));
  MCHK(m, hipStreamSynchronize(m->stream));
  MCHK(m, psm_copy_d2h(dst, src, (size_t)bytes));
  return PSM_OK;
}

}  // extern "C"
