// psm_api_ring.cpp -- C-ABI of libpsm_hip.so (include/psm.h): the pinned submission ring and registered host memory.  See psm_handle.h for the map of the files.
#include "psm_handle.h"

namespace psm_impl {

// ---- host-buffer ring ------------------------------------------------------------------------------------------
// Every slot owns pinned host buffers, device buffers, a workspace and a stream; the H2D copy, the kernels and the D2H
// copy of one ticket are ONE hipGraph replay on that stream (one host call per solve), and the slots overlap freely:
// the copies of ticket k+1 / k-1 run on the DMA engines while the kernels of ticket k compute.
bool host_registered(const psm_handle* h, const void* p, size_t bytes) {
  const char* c = (const char*)p;
  for (auto& r : h->host_regs) if (c >= r.base && c + bytes <= r.base + r.bytes) return true;
  return false;
}

// device-side address of a host pointer inside a registered range (nullptr: not registered / not mapped)
static float* host_mapped(const psm_handle* h, const void* p, size_t bytes) {
  const char* c = (const char*)p;
  for (auto& r : h->host_regs)
    if (c >= r.base && c + bytes <= r.base + r.bytes) return r.dev ? (float*)(r.dev + (c - r.base)) : nullptr;
  return nullptr;
}


static int ring_init(psm_handle* h) {
  if (h->ring_ready) return PSM_OK;
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)h->cfg.max_cases * npix * h->cfg.c_in, gout = (size_t)h->cfg.max_cases * npix * h->cfg.c_out;
  h->ring_dma = h->sw.at_create.ring_pull ? 0 : 1;
  for (auto& s : h->slot) {
    HIPCHK(h, hipHostMalloc((void**)&s.h_in, gin * sizeof(float), hipHostMallocMapped));
    HIPCHK(h, hipHostMalloc((void**)&s.h_out, gout * sizeof(float), hipHostMallocMapped));
    HIPCHK(h, hipHostMalloc((void**)&s.h_rs, (size_t)h->Mpad_cap * sizeof(float), hipHostMallocMapped));
    if (hipHostGetDevicePointer((void**)&s.m_in, s.h_in, 0) != hipSuccess || hipHostGetDevicePointer((void**)&s.m_out, s.h_out, 0) != hipSuccess ||
        hipHostGetDevicePointer((void**)&s.m_rs, s.h_rs, 0) != hipSuccess) {
      (void)hipGetLastError();
      s.m_in = s.m_out = s.m_rs = nullptr;
      h->ring_dma = 1;                                   // no mapped view of pinned memory: DMA copies
    }
    int rc;
    if ((rc = dev_alloc(h, &s.d_in, gin))) return rc;
    if ((rc = dev_alloc(h, &s.d_out, gout))) return rc;
    if ((rc = ws_alloc(h, s.ws))) return rc;
    HIPCHK(h, hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
    s.state = 0; s.ticket = -1;
  }
  HIPCHK(h, hipDeviceSynchronize());
  h->ring_ready = true;
  return PSM_OK;
}


// The launch sequence of one ticket on the slot's stream.
//  pull form (src_dev / dst_dev = device-side addresses of pinned or registered host memory): a stage-in kernel pulls the
//    grid over PCIe into s.d_in (and expands the out_scale), the solve's last kernel stores the field straight into
//    dst_dev -- kernels only;
//  DMA form (src_dev == nullptr): hipMemcpyAsync H2D from src, kernels, hipMemcpyAsync D2H into dst (copies optional:
//    with_copies = false enqueues the kernels alone).
static int ring_sequence(psm_handle* h, psm_handle::Slot& s, int n_cases, bool scale, const PsmSwitches::PerSolve& ps, const float* src_dev, float* dst_dev,
                         const float* src, float* dst, bool with_copies) {
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t nin = (size_t)n_cases * npix * h->cfg.c_in, nout = (size_t)n_cases * npix * h->cfg.c_out;
  const int M = n_cases * h->B;
  if (src_dev) {
    const int dbg = h->sw.at_create.ring_debug;   // timing experiments only: 1 no stage-in, 2 field stays on the device
    if (!(dbg & 1)) HIPCHK(h, psm_launch_stage_in(src_dev, s.d_in, nin, scale ? s.m_rs : nullptr, s.ws.d_row_scale, M, h->B, s.st));
    return launch_all(h, s.ws, s.d_in, n_cases, (dbg & 2) ? s.d_out : dst_dev, scale ? s.ws.d_row_scale : h->d_ones, s.st, nullptr, ps);
  }
  if (with_copies) HIPCHK(h, hipMemcpyAsync(s.d_in, src, nin * sizeof(float), hipMemcpyHostToDevice, s.st));
  if (scale) HIPCHK(h, hipMemcpyAsync(s.ws.d_row_scale, s.h_rs, (size_t)M * sizeof(float), hipMemcpyHostToDevice, s.st));
  int rc = launch_all(h, s.ws, s.d_in, n_cases, s.d_out, scale ? s.ws.d_row_scale : h->d_ones, s.st, nullptr, ps);
  if (rc) return rc;
  if (with_copies) HIPCHK(h, hipMemcpyAsync(dst, s.d_out, nout * sizeof(float), hipMemcpyDeviceToHost, s.st));
  return PSM_OK;
}


// Enqueue one ticket.  src / dst: where the grid is read from / the field is written to (the slot's pinned buffers or
// registered caller memory).
static int ring_launch(psm_handle* h, psm_handle::Slot& s, int n_cases, const float* out_scale, const float* src, float* dst) {
  { int rc0 = ensure_encode_aux(h, n_cases); if (rc0) return rc0; }
  h->last.on_ws0 = false;                               // captured or replayed, the ticket runs on the slot's workspace
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)n_cases * npix * h->cfg.c_in * sizeof(float), gout = (size_t)n_cases * npix * h->cfg.c_out * sizeof(float);
  const bool scale = out_scale != nullptr;
  const bool own = (src == s.h_in && dst == s.h_out);
  if (h->h_guard) h->h_guard[s.ws.gidx] = 0;            // the slot is free: nothing of an earlier ticket can still raise it
  s.last_src = src; s.last_dst = dst;
  if (scale) { if (out_scale != s.last_scale.data()) s.last_scale.assign(out_scale, out_scale + n_cases); } else s.last_scale.clear();
  const float* src_dev = nullptr;
  float* dst_dev = nullptr;
  if (!h->ring_dma) {                                    // pull form needs device-side views of both host buffers
    src_dev = src == s.h_in ? s.m_in : host_mapped(h, src, gin);
    dst_dev = dst == s.h_out ? s.m_out : host_mapped(h, dst, gout);
    if (!src_dev || !dst_dev) src_dev = nullptr, dst_dev = nullptr;
  }
  if (scale) {
    if (src_dev) for (int c = 0; c < n_cases; ++c) s.h_rs[c] = out_scale[c];
    else
      for (int c = 0; c < n_cases; ++c)
        for (int b = 0; b < h->B; ++b) s.h_rs[c * h->B + b] = out_scale[c];
  }
  const PsmSwitches::PerSolve ps = psm_switches_per_solve();     // this ticket's one read: the key and the route see the same values
  const int key = sequence_key(h, n_cases, scale, ps, true);
  const bool graphs = h->ring_graph && h->timed_kernel < 0;
  auto capture = [&](const float* from_dev, float* to_dev, bool with_copies, hipGraphExec_t* out) {   // on the slot's own buffers
    return capture_graph(h, s.st, "ring", [&] { return ring_sequence(h, s, n_cases, scale, ps, from_dev, to_dev, s.h_in, s.h_out, with_copies); }, out);
  };
  int rc;
  if (src_dev && graphs && own) {                        // pull form on the slot's own buffers: the whole ticket is one replay
    if (!s.g_full || s.g_full_key != key) {
      if (s.g_full) { (void)hipGraphExecDestroy(s.g_full); s.g_full = nullptr; }
      if ((rc = capture(src_dev, dst_dev, true, &s.g_full))) return rc;
      s.g_full_key = key;
    }
    HIPCHK(h, hipGraphLaunch(s.g_full, s.st));
  } else if (src_dev || !graphs) {                       // pull form on caller memory (pointers differ per ticket) / plain launches
    if ((rc = ring_sequence(h, s, n_cases, scale, ps, src_dev, dst_dev, src, dst, true))) return rc;
  } else {
    // Default: the two copies are hipMemcpyAsync calls on the slot's stream (DMA engines; inside a graph they would
    // become blit kernels, which read host memory at ~20 GB/s), the kernels in between are one graph replay.
    const int dbg = h->sw.at_create.ring_debug;   // timing experiments only: 1 no H2D, 2 no D2H
    if (!(dbg & 1)) HIPCHK(h, hipMemcpyAsync(s.d_in, src, gin, hipMemcpyHostToDevice, s.st));
    if (!s.g_kern || s.g_kern_key != key) {
      if (s.g_kern) { (void)hipGraphExecDestroy(s.g_kern); s.g_kern = nullptr; }
      if ((rc = capture(nullptr, nullptr, false, &s.g_kern))) return rc;
      s.g_kern_key = key;
    }
    HIPCHK(h, hipGraphLaunch(s.g_kern, s.st));
    if (!(dbg & 2)) HIPCHK(h, hipMemcpyAsync(dst, s.d_out, gout, hipMemcpyDeviceToHost, s.st));
  }
  HIPCHK(h, hipEventRecord(s.ev_out, s.st));
  return PSM_OK;
}


static int ring_check(psm_handle* h, int32_t n_cases) {
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (n_cases < 1 || n_cases > h->cfg.max_cases) return fail(h, PSM_ERR_ARG, "n_cases outside [1, max_cases]");
  return PSM_OK;
}


// A ticket whose grid was not the bound geometry (its field is NaN): drop the binding and run the ticket again on the
// general path, from the same source into the same destination.
static int ring_guard_rerun(psm_handle* h, psm_handle::Slot& s, const char* where) {
  if (!guard_take(h, s.ws)) return PSM_OK;
  int rc = guard_drop(h, where);
  if (rc) return rc;
  const std::string note = h->err;
  std::vector<float> sc = s.last_scale;
  if ((rc = ring_launch(h, s, s.n_cases, sc.empty() ? nullptr : sc.data(), s.last_src, s.last_dst))) return rc;
  HIPCHK(h, wait_event(s.ev_out));
  h->err = note + " (ticket solved again on the general path)";
  return PSM_OK;
}


static int slot_of(psm_handle* h, int64_t ticket, int state, psm_handle::Slot** out) {
  if (ticket < 0 || !h->ring_ready) return fail(h, PSM_ERR_ARG, "unknown ticket");
  psm_handle::Slot& s = h->slot[ticket % h->ring_slots];
  if (s.ticket != ticket || s.state != state)
    return fail(h, PSM_ERR_ARG, state == 1 ? "unknown ticket (not acquired, or already submitted)" : "unknown ticket (never submitted or already waited for)");
  *out = &s;
  return PSM_OK;
}

}  // namespace psm_impl

// ============================================================================
extern "C" {


int psm_ring_acquire(psm_handle* h, int64_t* ticket, float** grid_in, float** fields_out) {
  if (!h) return PSM_ERR_ARG;
  if (!h->planned) return fail(h, PSM_ERR_STATE, "psm_plan_grid has not been called");
  if (!ticket || !grid_in || !fields_out) return fail(h, PSM_ERR_ARG, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  int rc = ring_init(h);
  if (rc) return rc;
  psm_handle::Slot& s = h->slot[h->next_ticket % h->ring_slots];
  if (s.state != 0)
    return fail(h, PSM_ERR_STATE, "submission ring full: wait for the oldest ticket first (PSM_RING_SLOTS in flight)");
  s.state = 1; s.ticket = h->next_ticket; s.user_out = nullptr; s.direct_out = false;
  *ticket = h->next_ticket++;
  *grid_in = s.h_in; *fields_out = s.h_out;
  return PSM_OK;
}

int psm_ring_release(psm_handle* h, int64_t ticket) {
  if (!h) return PSM_ERR_ARG;
  psm_handle::Slot* s = nullptr;
  int rc = slot_of(h, ticket, 1, &s);                  // acquired, not submitted
  if (rc) return rc;
  s->state = 0;
  // the slot comes round again PSM_RING_SLOTS tickets later; the ticket counter does not go back (tickets stay unique)
  return PSM_OK;
}


int psm_ring_submit(psm_handle* h, int64_t ticket, int32_t n_cases, const float* out_scale) {
  if (!h) return PSM_ERR_ARG;
  int rc = ring_check(h, n_cases);
  if (rc) return rc;
  psm_handle::Slot* s = nullptr;
  if ((rc = slot_of(h, ticket, 1, &s))) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if ((rc = ring_launch(h, *s, n_cases, out_scale, s->h_in, s->h_out))) return rc;
  s->state = 2; s->n_cases = n_cases;
  return PSM_OK;
}


int psm_ring_wait(psm_handle* h, int64_t ticket) {
  if (!h) return PSM_ERR_ARG;
  psm_handle::Slot* s = nullptr;
  int rc = slot_of(h, ticket, 2, &s);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, wait_event(s->ev_out));
  if ((rc = ring_guard_rerun(h, *s, "psm_ring_wait"))) return rc;
  s->state = 0;
  return PSM_OK;
}


int psm_submit_grid_io(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, float* fields, int64_t* ticket) {
  if (!h) return PSM_ERR_ARG;
  int rc = ring_check(h, n_cases);
  if (rc) return rc;
  if (!grid || !ticket) return fail(h, PSM_ERR_ARG, "null argument");
  int64_t t; float *gi, *fo;
  if ((rc = psm_ring_acquire(h, &t, &gi, &fo))) return rc;
  psm_handle::Slot& s = h->slot[t % h->ring_slots];
  const size_t npix = (size_t)h->Ny * h->Nx;
  const size_t gin = (size_t)n_cases * npix * h->cfg.c_in * sizeof(float), gout = (size_t)n_cases * npix * h->cfg.c_out * sizeof(float);
  const float* src = s.h_in;
  float* dst = s.h_out;
  if (host_registered(h, grid, gin)) src = grid;                       // DMA straight from the caller's memory
  else memcpy(s.h_in, grid, gin);                                      // caller's buffer is free on return
  if (fields && host_registered(h, fields, gout)) { dst = fields; s.direct_out = true; }
  s.user_out = fields;
  if ((rc = ring_launch(h, s, n_cases, out_scale, src, dst))) { s.state = 0; return rc; }
  s.state = 2; s.n_cases = n_cases;
  *ticket = t;
  return PSM_OK;
}


int psm_submit_grid(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, int64_t* ticket) {
  return psm_submit_grid_io(h, grid, n_cases, out_scale, nullptr, ticket);
}


int psm_wait_grid(psm_handle* h, int64_t ticket, float* fields) {
  if (!h) return PSM_ERR_ARG;
  psm_handle::Slot* s = nullptr;
  int rc = slot_of(h, ticket, 2, &s);
  if (rc) return rc;
  if (!fields) fields = s->user_out;
  if (!fields) return fail(h, PSM_ERR_ARG, "null buffer (no destination was given at submission either)");
  if (s->direct_out && fields != s->user_out) return fail(h, PSM_ERR_ARG, "this ticket's field was DMA'd into the buffer given at submission");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, wait_event(s->ev_out));
  if ((rc = ring_guard_rerun(h, *s, "psm_wait_grid"))) return rc;
  if (!s->direct_out) memcpy(fields, s->h_out, (size_t)s->n_cases * h->Ny * h->Nx * h->cfg.c_out * sizeof(float));
  s->state = 0;
  return PSM_OK;
}


int psm_host_register(psm_handle* h, void* ptr, size_t bytes) {
  if (!h) return PSM_ERR_ARG;
  if (!ptr || bytes == 0) return fail(h, PSM_ERR_ARG, "null range");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  for (auto& r : h->host_regs) if (r.base == (char*)ptr) return fail(h, PSM_ERR_STATE, "range already registered");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, PSM_ERR_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess) { (void)hipGetLastError(); dev = nullptr; }   // DMA copies only
  h->host_regs.push_back({(char*)ptr, bytes, (char*)dev});
  return PSM_OK;
}


int psm_host_unregister(psm_handle* h, void* ptr) {
  if (!h) return PSM_ERR_ARG;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  for (size_t i = 0; i < h->host_regs.size(); ++i)
    if (h->host_regs[i].base == (char*)ptr) {
      HIPCHK(h, hipDeviceSynchronize());                  // no DMA of this handle may still touch the range
      (void)hipHostUnregister(ptr);
      h->host_regs.erase(h->host_regs.begin() + i);
      return PSM_OK;
    }
  return fail(h, PSM_ERR_ARG, "range was not registered with this handle");
}

}  // extern "C"
