// psm_switches.h -- every PSM_* environment switch of the PCA solve path (the conv path keeps its own table, psm_unet_plan.h): one nested
// struct per moment at which the environment is read, one field per switch, one reader per struct (psm_switches.cpp, host only).
// No other file of the path reads the environment; what a switch does is described where its field is used, INTEGRATION.md section 3d lists them all.
#pragma once
#include <cstdint>

#ifndef PSM_MESH_STAGE_MAX_DEFAULT

// cells up to which psm_solve reads registered input with the stage kernel; above, the DMA engine's higher large-copy rate (49 against
// 40 GB/s over this PCIe link) wins: measured crossover between 44 k (stage 107 / DMA 110 us) and 69 k cells (147 / 142 us),
// profiles/archive/r04_psm_solve.txt
#define PSM_MESH_STAGE_MAX_DEFAULT 50000

#endif

struct PsmSwitches {
  struct AtCreate {                     // psm_create, kept as h->sw.at_create for the life of the handle
    bool graph, guard, keep_hidden;     // PSM_GRAPH=1; PSM_NO_GUARD=1 clears guard; PSM_KEEP_HIDDEN
    int x6;                             // PSM_X6: -1 unset, bit 0 encode, bit 1 bound decode
    int encode_mt_min_rows, encode_kgroups;                    // PSM_ENCODE_MT_MIN_ROWS (96), PSM_ENCODE_KGROUPS (0: by the table)
    bool encode_chunked, encode_rowsplit, encode_pairs;        // PSM_ENCODE_CHUNKED, PSM_ENCODE_ROWSPLIT (set at all); PSM_ENCODE_PAIRS=0 clears
    bool dense_packed, guard_spread, paste_buffer_stores;      // PSM_DENSE_PACKED, PSM_GUARD_SPREAD, PSM_PASTE_BUFFER_STORES: =0 clears
    int decode_mtc, decode_wgs;                                // PSM_DECODE_MTC clamped to 1..3 (1), PSM_DECODE_WGS (512)
    int mesh_graph; int64_t mesh_stage_max; bool device_umax;  // PSM_MESH_GRAPH (2), PSM_MESH_STAGE_MAX, PSM_DEVICE_UMAX (set at all)
    bool ring_graph, ring_pull; int ring_use, ring_debug;      // PSM_RING_GRAPH=0 clears, PSM_RING_PULL=1, PSM_RING_USE: slots in rotation, 1..PSM_RING_SLOTS (all), PSM_RING_DEBUG
  } at_create;
  struct AtPlan {                       // psm_plan_grid, kept as h->sw.at_plan until the next plan
    int debug_skip;                     // PSM_DEBUG_SKIP
    bool no_fused_reduce, no_fused_assemble, no_closed_form;   // PSM_NO_FUSED_REDUCE=1, PSM_NO_FUSED_ASSEMBLE=1; PSM_NO_CLOSED_FORM (set at all)
  } at_plan;
  struct AtBind {                       // psm_set_geometry, psm_set_geometry_cases, psm_pin_buffers: read at the entry, not kept
    bool no_bind, no_direct_in, no_direct_out;                 // PSM_NO_BIND, PSM_NO_DIRECT_IN, PSM_NO_DIRECT_OUT (set at all)
  };
  struct PerSolve {                     // once per solve; both are bits of sequence_key (psm_api_step.cpp)
    bool sdf_fold, ln_fuse;             // PSM_SDF_FOLD=0, PSM_LN_FUSE=0 clear
  };
  struct Process {                      // no handle in reach: read once, at the first use
    double spin_us;                     // PSM_SPIN_US (300)
    int sync_block;                     // PSM_SYNC_BLOCK: -1 unset, 0 spin, 1 block
    int local_ranks;                    // ranks on this node as the MPI / torchrun launcher announces them (1); not a PSM_* switch
    bool bench_verbose;                 // PSM_BENCH_VERBOSE (set at all)
    int guard_pages, guard_fill;        // PSM_GUARD_PAGES: 0 off, 1, 2; PSM_GUARD_FILL: the byte, -1 unset
    bool guard_log;                     // PSM_GUARD_LOG (set at all)
  };
};

PsmSwitches::AtCreate psm_switches_at_create();
PsmSwitches::AtPlan psm_switches_at_plan();
PsmSwitches::AtBind psm_switches_at_bind();
PsmSwitches::PerSolve psm_switches_per_solve();
PsmSwitches::Process psm_switches_read_process();       // the reader behind the table below (the host test calls it per value)
const PsmSwitches::Process& psm_switches_process();    // the one process-wide table
