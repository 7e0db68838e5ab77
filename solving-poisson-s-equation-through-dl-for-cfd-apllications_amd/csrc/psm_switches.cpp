// psm_switches.cpp -- see psm_switches.h.  Host only: no HIP header, no handle.
#include "psm_switches.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

#include "../../include/psm.h"

// ---- the parse rules: a reader below names one per switch -----------------------------------------------------------
static bool is_set(const char* name) { return getenv(name) != nullptr; }                                           // set at all, "" and "0" included
static bool starts_with(const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; }          // first character
static int number(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }         // atoi; text that is no number: 0
static bool on_unless_zero(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }         // unset: on; "", "0", "x": off

PsmSwitches::AtCreate psm_switches_at_create() {
  PsmSwitches::AtCreate s;
  s.graph = starts_with("PSM_GRAPH", '1');
  s.guard = !starts_with("PSM_NO_GUARD", '1');
  s.keep_hidden = number("PSM_KEEP_HIDDEN", 0) != 0;
  s.x6 = number("PSM_X6", -1);
  s.encode_mt_min_rows = number("PSM_ENCODE_MT_MIN_ROWS", 96);
  s.encode_kgroups = number("PSM_ENCODE_KGROUPS", 0);
  s.encode_chunked = is_set("PSM_ENCODE_CHUNKED");
  s.encode_rowsplit = is_set("PSM_ENCODE_ROWSPLIT");
  s.encode_pairs = on_unless_zero("PSM_ENCODE_PAIRS");
  s.dense_packed = on_unless_zero("PSM_DENSE_PACKED");
  s.guard_spread = on_unless_zero("PSM_GUARD_SPREAD");
  s.paste_buffer_stores = on_unless_zero("PSM_PASTE_BUFFER_STORES");
  const int mtc = number("PSM_DECODE_MTC", 0);
  s.decode_mtc = mtc ? std::min(std::max(mtc, 1), 3) : 1;
  s.decode_wgs = number("PSM_DECODE_WGS", 512);
  s.mesh_graph = number("PSM_MESH_GRAPH", 2);
  { const char* e = getenv("PSM_MESH_STAGE_MAX"); s.mesh_stage_max = e ? atoll(e) : PSM_MESH_STAGE_MAX_DEFAULT; }
  s.device_umax = is_set("PSM_DEVICE_UMAX");
  s.ring_graph = !starts_with("PSM_RING_GRAPH", '0');
  s.ring_pull = starts_with("PSM_RING_PULL", '1');
  const int use = number("PSM_RING_USE", 0);
  s.ring_use = (use >= 1 && use <= PSM_RING_SLOTS) ? use : PSM_RING_SLOTS;
  s.ring_debug = number("PSM_RING_DEBUG", 0);
  return s;
}

PsmSwitches::AtPlan psm_switches_at_plan() {
  PsmSwitches::AtPlan s;
  s.debug_skip = number("PSM_DEBUG_SKIP", 0);
  s.no_fused_reduce = starts_with("PSM_NO_FUSED_REDUCE", '1');
  s.no_fused_assemble = starts_with("PSM_NO_FUSED_ASSEMBLE", '1');
  s.no_closed_form = is_set("PSM_NO_CLOSED_FORM");
  return s;
}

PsmSwitches::AtBind psm_switches_at_bind() {
  return PsmSwitches::AtBind{is_set("PSM_NO_BIND"), is_set("PSM_NO_DIRECT_IN"), is_set("PSM_NO_DIRECT_OUT")};
}

PsmSwitches::PerSolve psm_switches_per_solve() {
  return PsmSwitches::PerSolve{on_unless_zero("PSM_SDF_FOLD"), on_unless_zero("PSM_LN_FUSE")};
}

PsmSwitches::Process psm_switches_read_process() {
  PsmSwitches::Process s;
  { const char* e = getenv("PSM_SPIN_US"); s.spin_us = e ? atof(e) : 300.0; }
  s.sync_block = is_set("PSM_SYNC_BLOCK") ? (starts_with("PSM_SYNC_BLOCK", '0') ? 0 : 1) : -1;
  s.local_ranks = 1;
  for (const char* k : {"OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS", "PMI_LOCAL_SIZE", "SLURM_NTASKS_PER_NODE", "LOCAL_WORLD_SIZE"})
    if (number(k, 0) > 0) { s.local_ranks = number(k, 0); break; }
  s.bench_verbose = is_set("PSM_BENCH_VERBOSE");
  s.guard_pages = starts_with("PSM_GUARD_PAGES", '1') ? 1 : starts_with("PSM_GUARD_PAGES", '2') ? 2 : 0;
  s.guard_fill = is_set("PSM_GUARD_FILL") ? (number("PSM_GUARD_FILL", 0) & 255) : -1;
  s.guard_log = is_set("PSM_GUARD_LOG");
  return s;
}

const PsmSwitches::Process& psm_switches_process() {
  static const PsmSwitches::Process table = psm_switches_read_process();
  return table;
}
