// The PCA path's switch table (csrc/psm_switches.cpp) on the host, no device: every switch under unset, "", "0", "1", "2", "x", "-1"
// (and "9", past every clamp) through the reader of its read moment, against the value the parse rule of the site it was moved from
// gives.  The expectations were worked out by hand from that site (file:line of the commit before the table existed, in each row),
// not from the readers.  Usage: switches_host
#include <cstdio>
#include <cstdlib>

#include "psm_switches.h"

static const char* VALUES[] = {nullptr, "", "0", "1", "2", "x", "-1", "9"};
constexpr int NV = sizeof(VALUES) / sizeof(VALUES[0]);

struct Row {
  const char* name;
  const char* site;                     // where the rule was read from
  double (*get)();
  double want[NV];                      // in the order of VALUES
};

#define CREATE(f) [] { return (double)psm_switches_at_create().f; }
#define PLAN(f) [] { return (double)psm_switches_at_plan().f; }
#define BIND(f) [] { return (double)psm_switches_at_bind().f; }
#define SOLVE(f) [] { return (double)psm_switches_per_solve().f; }
#define PROC(f) [] { return (double)psm_switches_read_process().f; }

static const Row ROWS[] = {
    // ---- at_create
    {"PSM_GRAPH", "psm_api_model.cpp:301-302  ug && ug[0] == '1'", CREATE(graph), {0, 0, 0, 1, 0, 0, 0, 0}},
    {"PSM_NO_GUARD", "psm_api_model.cpp:311-312  guard_on = !(ng && ng[0] == '1')", CREATE(guard), {1, 1, 1, 0, 1, 1, 1, 1}},
    {"PSM_X6", "psm_api_model.cpp:313  set ? atoi : -1", CREATE(x6), {-1, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_KEEP_HIDDEN", "psm_api_model.cpp:314  set && atoi != 0", CREATE(keep_hidden), {0, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_ENCODE_MT_MIN_ROWS", "psm_api_solve.cpp:25  set ? atoi : 96", CREATE(encode_mt_min_rows), {96, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_ENCODE_KGROUPS", "psm_api_solve.cpp:30  set ? atoi : 0", CREATE(encode_kgroups), {0, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_ENCODE_CHUNKED", "psm_api_solve.cpp:104  != nullptr", CREATE(encode_chunked), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_ENCODE_ROWSPLIT", "psm_encode.hip:838  != nullptr", CREATE(encode_rowsplit), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_ENCODE_PAIRS", "psm_encode.hip:848  !(set && atoi == 0)", CREATE(encode_pairs), {1, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_DENSE_PACKED", "psm_api_solve.cpp:123  !(set && atoi == 0)", CREATE(dense_packed), {1, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_GUARD_SPREAD", "psm_api_solve.cpp:138  !(set && atoi == 0)", CREATE(guard_spread), {1, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_PASTE_BUFFER_STORES", "psm_api_solve.cpp:147  !(set && atoi == 0)", CREATE(paste_buffer_stores), {1, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_DECODE_MTC", "psm_bound.hip:644,646  atoi != 0 ? clamp(atoi, 1, 3) : 1", CREATE(decode_mtc), {1, 1, 1, 1, 2, 1, 1, 3}},
    {"PSM_DECODE_WGS", "psm_bound.hip:645  set ? atoi : 512", CREATE(decode_wgs), {512, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_MESH_GRAPH", "psm_api_mesh.cpp:248  set ? atoi : 2", CREATE(mesh_graph), {2, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_MESH_STAGE_MAX", "psm_api_mesh.cpp:249  set ? atoll : 50000 (psm_handle.h:977)", CREATE(mesh_stage_max), {50000, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_DEVICE_UMAX", "psm_api_mesh.cpp:249  != nullptr", CREATE(device_umax), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_RING_GRAPH", "psm_api_ring.cpp:29-30  (rg && rg[0] == '0') ? 0 : 1", CREATE(ring_graph), {1, 1, 0, 1, 1, 1, 1, 1}},
    {"PSM_RING_USE", "psm_api_ring.cpp:31-32  1 <= atoi <= 8 (PSM_RING_SLOTS) ? atoi : 8", CREATE(ring_use), {8, 8, 8, 1, 2, 8, 8, 8}},
    {"PSM_RING_PULL", "psm_api_ring.cpp:33-34  ring_dma = (rp && rp[0] == '1') ? 0 : 1", CREATE(ring_pull), {0, 0, 0, 1, 0, 0, 0, 0}},
    {"PSM_RING_DEBUG", "psm_api_ring.cpp:71,127  set ? atoi : 0", CREATE(ring_debug), {0, 0, 0, 1, 2, 0, -1, 9}},
    // ---- at_plan
    {"PSM_DEBUG_SKIP", "psm_api_plan.cpp:371-372  set ? atoi : 0", PLAN(debug_skip), {0, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_NO_FUSED_REDUCE", "psm_api_plan.cpp:375-376  nr && nr[0] == '1'", PLAN(no_fused_reduce), {0, 0, 0, 1, 0, 0, 0, 0}},
    // the documented rule of :379-380 at both sites; :188 was "set at all" (= 0 refused a bind): the one rule changed on purpose
    {"PSM_NO_FUSED_ASSEMBLE", "psm_api_plan.cpp:379-380  nf && nf[0] == '1'", PLAN(no_fused_assemble), {0, 0, 0, 1, 0, 0, 0, 0}},
    {"PSM_NO_CLOSED_FORM", "psm_api_plan.cpp:254  != nullptr", PLAN(no_closed_form), {0, 1, 1, 1, 1, 1, 1, 1}},
    // ---- at_bind
    {"PSM_NO_BIND", "psm_api_mesh.cpp:167,401  != nullptr", BIND(no_bind), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_NO_DIRECT_IN", "psm_api_mesh.cpp:252  != nullptr", BIND(no_direct_in), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_NO_DIRECT_OUT", "psm_api_mesh.cpp:252  != nullptr", BIND(no_direct_out), {0, 1, 1, 1, 1, 1, 1, 1}},
    // ---- per_solve
    {"PSM_SDF_FOLD", "psm_api_solve.cpp:71-72  !(e && atoi(e) == 0)", SOLVE(sdf_fold), {1, 0, 0, 1, 1, 0, 1, 1}},
    {"PSM_LN_FUSE", "psm_api_solve.cpp:133-134  !(ln_env && atoi(ln_env) == 0)", SOLVE(ln_fuse), {1, 0, 0, 1, 1, 0, 1, 1}},
    // ---- process
    {"PSM_SPIN_US", "psm_handle.h:814  e ? atof(e) : 300.0", PROC(spin_us), {300, 0, 0, 1, 2, 0, -1, 9}},
    {"PSM_SYNC_BLOCK", "psm_api_model.cpp:24-25  e ? e[0] != '0' : by the core count (-1 here)", PROC(sync_block), {-1, 1, 0, 1, 1, 1, 1, 1}},
    {"PSM_BENCH_VERBOSE", "psm_hostbench.cpp:32  != nullptr", PROC(bench_verbose), {0, 1, 1, 1, 1, 1, 1, 1}},
    {"PSM_GUARD_PAGES", "psm_alloc.cpp:16  (e[0] == '1' || e[0] == '2') ? e[0] - '0' : 0", PROC(guard_pages), {0, 0, 0, 1, 2, 0, 0, 0}},
    {"PSM_GUARD_FILL", "psm_alloc.cpp:54-55  set ? atoi & 255 : no fill (-1 here)", PROC(guard_fill), {-1, 0, 0, 1, 2, 0, 255, 9}},
    {"PSM_GUARD_LOG", "psm_alloc.cpp:61,81  != nullptr", PROC(guard_log), {0, 1, 1, 1, 1, 1, 1, 1}},
    // the launchers' rank counts of psm_api_model.cpp:14-20 (v && atoi(v) > 0 ? atoi(v) : the next name; none: 1)
    {"OMPI_COMM_WORLD_LOCAL_SIZE", "psm_api_model.cpp:15-17", PROC(local_ranks), {1, 1, 1, 1, 2, 1, 1, 9}},
    {"MPI_LOCALNRANKS", "psm_api_model.cpp:15-17", PROC(local_ranks), {1, 1, 1, 1, 2, 1, 1, 9}},
    {"PMI_LOCAL_SIZE", "psm_api_model.cpp:15-17", PROC(local_ranks), {1, 1, 1, 1, 2, 1, 1, 9}},
    {"SLURM_NTASKS_PER_NODE", "psm_api_model.cpp:15-17", PROC(local_ranks), {1, 1, 1, 1, 2, 1, 1, 9}},
    {"LOCAL_WORLD_SIZE", "psm_api_model.cpp:15-17", PROC(local_ranks), {1, 1, 1, 1, 2, 1, 1, 9}},
};

static int failures = 0;
static void check(bool ok, const char* name, const char* value, double got, double want, const char* site) {
  if (ok) return;
  std::printf("FAIL %s=%s: got %g, want %g (%s)\n", name, value ? (value[0] ? value : "\"\"") : "<unset>", got, want, site);
  ++failures;
}

int main() {
  for (const Row& r : ROWS) unsetenv(r.name);
  int checks = 0;
  for (const Row& r : ROWS) {
    for (int v = 0; v < NV; ++v) {
      if (VALUES[v]) setenv(r.name, VALUES[v], 1); else unsetenv(r.name);
      const double got = r.get();
      check(got == r.want[v], r.name, VALUES[v], got, r.want[v], r.site);
      ++checks;
    }
    unsetenv(r.name);
  }
  // a 64-bit cell count (atoll, not atoi), the order of the launchers' names, and the cached table: read once, at the first use
  setenv("PSM_MESH_STAGE_MAX", "5000000000", 1);
  check(psm_switches_at_create().mesh_stage_max == 5000000000LL, "PSM_MESH_STAGE_MAX", "5000000000", (double)psm_switches_at_create().mesh_stage_max, 5e9, "psm_api_mesh.cpp:249");
  unsetenv("PSM_MESH_STAGE_MAX");
  setenv("LOCAL_WORLD_SIZE", "4", 1); setenv("OMPI_COMM_WORLD_LOCAL_SIZE", "0", 1); setenv("PMI_LOCAL_SIZE", "6", 1);
  check(psm_switches_read_process().local_ranks == 6, "PMI_LOCAL_SIZE before LOCAL_WORLD_SIZE", "6", psm_switches_read_process().local_ranks, 6, "psm_api_model.cpp:15-17");
  setenv("PSM_SPIN_US", "12.5", 1);
  const double first = psm_switches_process().spin_us;
  setenv("PSM_SPIN_US", "40", 1);
  check(first == 12.5 && psm_switches_process().spin_us == 12.5 && psm_switches_read_process().spin_us == 40.0, "PSM_SPIN_US (process table)", "12.5 then 40",
        psm_switches_process().spin_us, 12.5, "psm_handle.h:814");
  checks += 3;
  std::printf("switches: %d, checks: %d, failures: %d\n", (int)(sizeof(ROWS) / sizeof(ROWS[0])), checks, failures);
  return failures ? 1 : 0;
}
