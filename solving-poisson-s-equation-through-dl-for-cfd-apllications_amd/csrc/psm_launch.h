// psm_launch.h -- PSM_LAUNCH: kernel launches that can be stamped dispatch by dispatch (psm_time_kernels, psm_unet_time_kernels).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <vector>

// Dispatch-level timing of every kernel launch of the solve path (psm_time_kernels): while a probe is installed on the
// calling thread, PSM_LAUNCH stamps each dispatch's own begin / end into an event pair (hipExtLaunchKernelGGL -- the
// source rocprofv3 reads, not marker packets around the launch) and records the kernel's name.
struct PsmLaunchProbe {
  struct Rec { const char* name; hipEvent_t e0, e1; int tag; };
  int tag = -1;                          // set by the caller around a launch (psm_unet_time_kernels: the convolution index)
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;          // recycled events
  hipEvent_t get() { if (pool.empty()) { hipEvent_t e; (void)hipEventCreate(&e); return e; } hipEvent_t e = pool.back(); pool.pop_back(); return e; }
};
extern thread_local PsmLaunchProbe* psm_launch_probe;
#define PSM_LAUNCH(kern, grid, block, lds, st, ...)                                                                   \
  do {                                                                                                                \
    if (psm_launch_probe) {                                                                                           \
      PsmLaunchProbe::Rec r_{#kern, psm_launch_probe->get(), psm_launch_probe->get(), psm_launch_probe->tag};                                \
      psm_launch_probe->recs.push_back(r_);                                                                           \
      hipExtLaunchKernelGGL(kern, grid, block, (std::uint32_t)(lds), st, r_.e0, r_.e1, 0, __VA_ARGS__);               \
    } else {                                                                                                          \
      hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);                                                    \
    }                                                                                                                 \
  } while (0)


// The encode kernel families are templates on <c_in, aligned>: the one ladder over both for all of them (psm_launch_encode,
// psm_launch_encode_bf16).  With events, hipExtLaunchKernelGGL stamps them with the dispatch's own begin / end times (the
// source rocprofv3 reads), not with separate marker packets around the launch; without, PSM_LAUNCH.  A macro, not a function
// template: PSM_LAUNCH records the kernel's name by stringising `(family<C, AL>)` after C and AL were substituted, and tools key
// on those names.  Returns hipErrorInvalidValue from the calling function for a c_in outside 1..4.
#define PSM_ENCODE_LAUNCH_(family, C, AL, grid, lds, st, ev0, ev1, a)                                                              \
  if (ev0) hipExtLaunchKernelGGL((family<C, AL>), grid, dim3(256), (std::uint32_t)(lds), st, ev0, ev1, 0, a);                      \
  else PSM_LAUNCH((family<C, AL>), grid, dim3(256), lds, st, a)
#define PSM_ENCODE_CASE_(family, C, grid, lds, st, ev0, ev1, a)                                                                    \
  case C:                                                                                                                         \
    if ((a).aligned) { PSM_ENCODE_LAUNCH_(family, C, true, grid, lds, st, ev0, ev1, a); }                                         \
    else { PSM_ENCODE_LAUNCH_(family, C, false, grid, lds, st, ev0, ev1, a); }                                                    \
    break;
#define PSM_LAUNCH_ENCODE_FAMILY(family, grid, lds, st, ev0, ev1, a)                                                               \
  switch ((a).c_in) {                                                                                                             \
    PSM_ENCODE_CASE_(family, 1, grid, lds, st, ev0, ev1, a)                                                                       \
    PSM_ENCODE_CASE_(family, 2, grid, lds, st, ev0, ev1, a)                                                                       \
    PSM_ENCODE_CASE_(family, 3, grid, lds, st, ev0, ev1, a)                                                                       \
    PSM_ENCODE_CASE_(family, 4, grid, lds, st, ev0, ev1, a)                                                                       \
    default: return hipErrorInvalidValue;                                                                                         \
  }
