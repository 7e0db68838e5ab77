"""One smallest shape per route of the PCA solve path: for every configuration one solve by plain launches, then a capture and
two graph replays (PSM_GRAPH=1 handle), and a SHA-256 of the output of the plain solve and of each graph solve.  Two builds of
the library that take the same routes print the same table, and under `rocprofv3 --kernel-trace` dispatch the same kernels in
the same order (--dispatches prints a trace as one line per dispatch, to be compared with diff):

    python tools/route_matrix.py [--lib SO] [--only NAME,...] [--mesh-graph 0|1|2] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_matrix.py --lib tools/_bin/libpsm_base.so
    python tools/route_matrix.py --dispatches DIR/.../*_kernel_trace.csv     (no GPU needed)
    python tools/route_matrix.py --table LIST_A LIST_B      two such lists as one numbered table of the distinct lines + each list as numbers

The `boundary` configurations (--only boundary, or one of BOUNDARY by name) hash the mesh ends of the library at the smallest shapes
that can go wrong: every one runs in a child process of its own with its switches in the environment (as a host program sets
them) and prints one SHA-256 line per output.

The `steps` configurations (--only steps, or one of STEPS by name) hash the entries that put stages around a solve (solve_device,
csrc/psm_api_step.cpp), each in a child process of its own: per variant (with / without out_scale, apply_filter 0 / 1) one call on a
handle that launches plainly, then a capture and two replays on a PSM_GRAPH=1 handle, one SHA-256 per output; the `_host`
configurations go through the host entry on a bound geometry and then, with one frame, on a geometry that is not the frames' (one
guard trip, the re-run on the general path).  The `_rows` entries take the frames as float32 dataset rows (width 11, gradP 8): no
out_scale (the rows stage makes it on the device), and the per-frame scalars are one more hashed output.

The `conv` configurations (--only conv, or one of CONV by name) run the convolutional path, each in a child process with its planner
switches in the environment: per precision one forward pass under the planner's own plan, one line with the SHA-256 of the field and the
plan (psm_unet_plan_info per layer).

The `refusals` configuration (--only refusals) is a fixed list of calls that the three evaluators' image, device, host and rows
entries refuse from their argument checks, before anything is enqueued: one line per call with the return code and the text of
psm_last_error, to be compared with diff between two builds.

--lib: the library to load (default: the tree's libpsm_hip.so), e.g. the parent commit's build.  The `mesh` configuration runs in the one
mode --mesh-graph sets (default 2), so the three modes take three runs: a parent build given with --lib may still read PSM_MESH_GRAPH
once per process (this tree reads it at psm_create).
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name: (variant, c_in, (ny, nx), p_in, p_out, n_cases, precision, env, bind) -- the first thirteen are _CONFIGS of tests/test_pca_stage_oracle.py
GRID_CONFIGS = {
    "deltas_c3_p32_one": ("deltas", 3, (256, 256), 32, 32, 1, "f32", {}, False),
    "gradp_c2_p128_pair": ("gradp", 2, (256, 256), 128, 128, 1, "f32", {}, False),
    "chapter5_c4_odd_nx": ("chapter5", 4, (300, 257), 100, 96, 1, "f32", {}, False),
    "deltas_c1_n8_x6": ("deltas", 1, (256, 256), 40, 64, 8, "f32", {}, False),
    "gradp_c3_p160_n5_packed": ("gradp", 3, (256, 256), 160, 160, 5, "f32", {}, False),
    "deltas_c3_n48_x6_mt": ("deltas", 3, (256, 256), 64, 128, 48, "f32", {}, False),
    "deltas_c3_n8_f32": ("deltas", 3, (256, 256), 48, 96, 8, "f32", {"PSM_X6": "0"}, False),
    "chapter5_c3_one_x6": ("chapter5", 3, (256, 300), 33, 64, 1, "f32", {"PSM_X6": "1"}, False),
    "deltas_bf16_one": ("deltas", 3, (256, 256), 64, 128, 1, "bf16", {}, False),
    "gradp_bf16_n5": ("gradp", 3, (256, 256), 48, 64, 5, "bf16", {}, False),
    "deltas_bound_one": ("deltas", 3, (256, 256), 32, 32, 1, "f32", {}, True),
    "gradp_bound_n4": ("gradp", 3, (256, 256), 64, 96, 4, "f32", {}, True),
    "deltas_bound_bf16": ("deltas", 3, (256, 256), 64, 128, 1, "bf16", {}, True),
    # bound path: one case (the headline shape), batches with the chain launch (gradp) and with the closed form (deltas)
    "gradp_bound_one": ("gradp", 3, (256, 256), 128, 128, 1, "f32", {}, True),
    "gradp_bound_n8": ("gradp", 3, (256, 256), 128, 128, 8, "f32", {}, True),
    "deltas_bound_n8_cf": ("deltas", 3, (256, 256), 64, 64, 8, "f32", {}, True),
    "deltas_bound_100_blocks": ("deltas", 3, (900, 900), 32, 32, 1, "f32", {}, True),        # more than 64 blocks: chain launch + batch paste for one case
    "gradp_bound_bf16_n5": ("gradp", 3, (256, 256), 48, 64, 5, "bf16", {}, True),
    "deltas_bound_n17_spread": ("deltas", 3, (256, 256), 32, 32, 17, "f32", {}, True),       # 272 guard workgroups: dealt over the Dense launches
}
# name: environment of the child process.  psm_solve on the 138 x 300 mesh case unless the name says otherwise.
BOUNDARY = {
    "solve_host_umax": {},                                   # unregistered arrays: U_max on the host
    "solve_device_umax": {"PSM_DEVICE_UMAX": "1"},           # unregistered, psm_umax_kernel
    "solve_partials": {},                                    # 32769 + 37 cells on synthetic tables: psm_umax_partial_kernel, folded by to_grid
    "solve_registered_graph1": {"PSM_MESH_GRAPH": "1"},      # registered arrays: stage kernel + partials, one graph replay
    "solve_registered_graph2": {"PSM_MESH_GRAPH": "2"},      # the same as plain launches
    "solve_nan": {},                                         # one NaN velocity: U_max and with it every pressure
    "cases_k1": {}, "cases_k3": {},                          # psm_solve_cases: 16021 / 16165 / 15838 cells, none a multiple of 256
    "delta_host_umax": {},                                   # psm_solve_delta from an unprimed state: the priming step, then two delta steps
    "delta_partials": {},                                    # the same three steps on the 32769 + 37 cells of solve_partials
    "cases_delta_k3": {},                                    # psm_solve_cases_delta on the three meshes of cases_k3, three steps from unprimed
    "poisson_solve": {}, "poisson_solve_noweight": {},       # psm_solve_poisson behind SolverModule(step='poisson'): the priming step(s), then three steps
    "poisson_cases_k3": {},                                  # psm_solve_cases_poisson on the three meshes of cases_k3
    "gradp_solve": {}, "gradp_solve_noref": {},              # psm_solve_gradp behind SolverModule(step='gradp'), reference 'outlet' / 'none', filter on
    "gradp_cases_k3": {},                                    # psm_solve_cases_gradp on the three meshes of cases_k3
    "mesh_to_grid": {},                                      # psm_mesh_to_grid k = 1 and 3, fill 0 / 1, on hand-made tables (130 x 131)
    "frames_to_grid": {},                                    # psm_frames_to_grid_device: 2 frames, a float64 plane, a float32 plane, a skipped column
    "block_error": {},                                       # psm_block_error behind a solve: label blocks + the per-block sums
    "field_errors": {},                                      # psm_field_errors_device: 17030 pixels (no multiple of 4), dense aligned / odd-offset / strided planes
}
# name: (entry, frames per call; 0: the host entry, bound and tripping).  Frame entries on hand-made tables of 200 cells: 138 x 300, the
# evaluator's grid (161 workgroups + 184 pixels); the gradP frames on 320 x 300.  k: 7 = the velocities, one extra plane, the
# weighting pair (the error blocks need the two label planes: 8); 4 / 6 = one column more than the deltas / gradP pack stores.
# chapter4_frames_<inputs>: both image widths (M_u 3, M_fU 2), c_in + 1 columns; the entry takes no scale and no filter.
STEPS = {"pressure": None, "poststeps": None, "poisson_step": ("poisson_step", 2)}
for _e in ("poisson_frames", "poisson_frames_errors", "deltas_frames", "gradp_frames", "chapter4_frames_M_u", "chapter4_frames_M_fU",
           "deltas_rows", "gradp_rows", "poisson_rows"):
    STEPS.update({f"{_e}_n1": (_e, 1), f"{_e}_n3": (_e, 3), f"{_e}_host": (_e, 0)})
REFUSALS = {"refusals": {}}
# conv path, name: (widths, (ny, nx), n, c_in, environment of the child process): one forward pass per precision under the planner's own plan
_M4 = ((16, 32, 64, 128), (56, 88), 2, 3)
CONV = {
    "conv_m4": _M4 + ({},),                                                              # stem, split-K slabs, x6, fused head
    "conv_m4_pairs": _M4 + ({"PSM_UNET_PAIR_MIN": "1"},),                                # stem / pool / upsample pairs
    "conv_m4_kw": _M4 + ({"PSM_UNET_KW": "-2", "PSM_UNET_NO_PAIR": "1"},),               # in-workgroup K split wherever eligible
    "conv_pairs_44x52": ((16, 32, 64), (44, 52), 3, 4, {"PSM_UNET_PAIR_MIN": "1"}),      # every pair kernel, tiles that overhang on both axes
    "conv_unet_s_256_n8": ((16, 32, 64, 128, 256), (256, 256), 8, 3, {}),                # the bench shape
}
OTHER = ["attention_ln_deferred", "attention_ln_launched", "conv1d_head", "mesh", "ring", "pressure", "poststeps"]
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def report(name, note, run):
    """run(k): called once with PSM_GRAPH=0 (plain launches, one solve) and once with PSM_GRAPH=1 (three solves: the capture and
    two replays); returns the output arrays of its k solves.  note(): text for the end of the line, called after the runs."""
    plain = with_env({"PSM_GRAPH": "0"}, lambda: run(1))
    graph = with_env({"PSM_GRAPH": "1"}, lambda: run(3))
    say(f"{name:28s} plain={sha(plain[0])} capture={sha(graph[0])} replay1={sha(graph[1])} replay2={sha(graph[2])}  {note()}")


def grid_config(name):
    import numpy as np
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate
    from test_pca_stage_oracle import _grids, _model
    variant, c_in, (ny, nx), p_in, p_out, n, precision, env, bind = GRID_CONFIGS[name]
    model = _model(variant, c_in, p_in, p_out, widths=(512, 512, 512), seed=11)
    grids = _grids(n, ny, nx, c_in, seed=7)
    note = []

    def run(solves):
        with GridSurrogate(model, ny, nx, max_cases=n, precision=precision) as sur:
            if bind:
                note[:] = ["bound" if sur.bind_geometry(grids) else "NOT bound"]
            d_in, d_out = DeviceArray(grids), DeviceArray(shape=(n, ny, nx, model.c_out))
            out = []
            for _ in range(solves):
                sur.solve_device(d_in.ptr, n, d_out.ptr)
                out.append(d_out.numpy())
            assert sur.guard_trips == 0
            d_in.free(), d_out.free()
        return out
    report(name, lambda: f"{variant} {ny}x{nx} c_in={c_in} p={p_in}/{p_out} cases={n} {precision} {env or ''} " + " ".join(note), lambda k: with_env(env, lambda: run(k)))


def other_config(name):
    import numpy as np
    import cases
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate, SolverModule, synthetic
    ny = nx = 256

    def device_solves(model, grids, solves, setup=None, step=None):
        n = grids.shape[0]
        with GridSurrogate(model, ny, nx, max_cases=n) as sur:
            d_in, d_out = DeviceArray(grids), DeviceArray(shape=(n, ny, nx, model.c_out))
            extra = setup(sur, d_in) if setup else None
            out = []
            for _ in range(solves):
                out.append(step(sur, d_in, d_out, extra) if step else (sur.solve_device(d_in.ptr, n, d_out.ptr), d_out.numpy())[1])
            d_in.free(), d_out.free()
        return out

    if name.startswith("attention"):
        model = synthetic.make_model("deltas", p_in=48, p_out=48, arch="MLP_attention")
        grids = np.stack([synthetic.channel_grid(ny, nx, seed=4 + k) for k in range(2)]).astype(np.float32)
        env = {"PSM_LN_FUSE": "0"} if name.endswith("launched") else {}
        os.environ.pop("PSM_LN_FUSE", None)
        report(name, lambda: f"densePCA_attention, 2 cases, {env or 'PSM_LN_FUSE unset'}", lambda k: with_env(env, lambda: device_solves(model, grids, k)))
    elif name == "conv1d_head":
        model = synthetic.make_model("deltas", p_in=24, p_out=24)
        model.conv1d, model.weights = synthetic.he_conv1d_head(24, [8, 4, 8], 24, seed=5)
        grids = synthetic.channel_grid(ny, nx, seed=6)[None].astype(np.float32)
        report(name, lambda: "conv1D_PCA head, 1 case", lambda k: device_solves(model, grids, k))
    elif name == "ring":
        model = synthetic.make_model("deltas", p_in=32, p_out=32)
        grid = synthetic.channel_grid(ny, nx, seed=8).astype(np.float32)

        def run(solves):                      # the ring has its own switch (PSM_RING_GRAPH), and every slot captures its own graph:
            tickets = 1 if solves == 1 else 10    # tickets 9 and 10 replay the graphs of slots 0 and 1
            with GridSurrogate(model, ny, nx) as sur:
                got = [sur.wait(sur.submit(grid)).copy() for _ in range(tickets)]
            return got if solves == 1 else [got[0], got[-2], got[-1]]
        report(name, lambda: "psm_submit_grid / psm_wait_grid, one ticket in flight",
               lambda k: with_env({"PSM_RING_GRAPH": "0" if k == 1 else "1"}, lambda: run(k)))
    elif name == "pressure":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from pressure_step import cut_of
        model = synthetic.make_model("gradp", p_in=64, p_out=64)
        grids = synthetic.channel_grid(ny, nx, seed=1)[None].astype(np.float32)
        cy, cx = cut_of(grids[0, ..., 2])

        def setup(sur, d_in):
            assert sur.bind_geometry(d_in.ptr, on_device=True, n_cases=1)
            assert sur.bind_integration(grids[..., 2], [cy], [cx], 1.0 / nx, 1.0 / ny)
            return DeviceArray(shape=(1, ny, nx))

        def step(sur, d_in, d_out, d_p):
            sur.solve_pressure_device(d_in.ptr, 1, d_p.ptr)
            return d_p.numpy()
        report(name, lambda: "psm_solve_pressure_device, bound, 1 case", lambda k: device_solves(model, grids, k, setup, step))
    elif name == "poststeps":
        model = synthetic.make_model("deltas", p_in=32, p_out=32)
        grids = synthetic.channel_grid(ny, nx, seed=2)[None].astype(np.float32)
        rng = np.random.default_rng(3)
        dU, prev = (rng.standard_normal((1, ny, nx)).astype(np.float32) for _ in range(2))

        def setup(sur, d_in):
            assert sur.bind_geometry(d_in.ptr, on_device=True, n_cases=1)
            sur.bind_poststeps()
            return [DeviceArray(dU), DeviceArray(prev)] + [DeviceArray(shape=(1, ny, nx)) for _ in range(3)]

        def step(sur, d_in, d_out, b):
            sur.solve_poststeps_device(d_in.ptr, 1, b[2].ptr, True, b[0].ptr, b[1].ptr, b[3].ptr, b[4].ptr)
            return np.stack([b[2].numpy(), b[3].numpy(), b[4].numpy()])
        report(name, lambda: "psm_solve_poststeps_device (filter + weighting), bound, 1 case", lambda k: device_solves(model, grids, k, setup, step))
    elif name == "mesh":
        array, top, obst, model, maxs = cases.build_mesh_case()
        sm = SolverModule(model, maxs)
        sm.init_func(array, top, obst)
        cells, out = np.ascontiguousarray(array, np.float64).copy(), np.empty(array.shape[0], np.float64)
        sm.pin(cells, out)                    # registered buffers: the graph modes of psm_solve need them
        h = [sha(sm.py_func(cells, out=out).copy()) for _ in range(3)]
        sm.unpin()
        say(f"{'mesh':28s} solve1={h[0]} solve2={h[1]} solve3={h[2]}  psm_solve on the 140x300 mesh case, PSM_MESH_GRAPH={os.environ['PSM_MESH_GRAPH']}")


def hand_mesh(sur, ny, nx, n_cells, seed=1301):
    """Mesh -> grid tables made by hand on `sur` (psm_set_geometry without the grid -> mesh side): random simplices, a quarter of the
    grid points with a negative weight, 15 % of the points redirected to another cell (several writers there, possibly none at home)."""
    import numpy as np
    ng, rng = ny * nx, np.random.default_rng(seed)
    vtx = rng.integers(0, n_cells, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    wts = np.c_[w, 1.0 - w.sum(axis=1)]
    neg = rng.random(ng) < 0.25
    wts[neg, 0] = -wts[neg, 0]
    wts[neg, 2] = 1.0 - wts[neg, 0] - wts[neg, 1]
    cell = np.arange(ng)
    moved = rng.random(ng) < 0.15
    cell[moved] = rng.integers(0, ng, int(moved.sum()))
    sur.set_mesh(vtx, np.ascontiguousarray(wts), np.c_[cell // nx, cell % nx].astype(np.int32), np.ones((ny, nx)), n_cells)


def boundary_config(name):
    """Runs in the child process: one line per output."""
    import numpy as np
    import cases
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, synthetic
    from psm_amd.surrogate import _p
    line = lambda what, a: say(f"{name:28s} {what:18s} {sha(a)}")
    HY, HX, HN = 130, 131, 200                               # the hand-made mesh: 17030 pixels, 200 cells
    if name.startswith("solve_") and name != "solve_partials":
        array, top, obst, model, maxs = cases.build_mesh_case()
        sm = SolverModule(model, maxs)
        sm.init_func(array, top, obst)
        cells, out = np.ascontiguousarray(array, np.float64).copy(), np.empty(array.shape[0], np.float64)
        if name == "solve_nan":
            cells[array.shape[0] // 3, 1] = np.nan
        if "registered" in name:
            sm.pin(cells, out)
        for k in range(2):
            line(f"p solve{k + 1}", sm.py_func(cells, out=out).copy())
        if "registered" in name:
            sm.unpin()
    elif name in ("solve_partials", "delta_partials"):
        _, _, _, model, maxs = cases.build_mesh_case()
        ny, nx, n = 138, 300, 32769 + 37
        ng, rng = ny * nx, np.random.default_rng(1501)

        def simplices(rows, hi):                             # random simplices, a tenth with a negative weight
            v = rng.integers(0, hi, (rows, 3)).astype(np.int32)
            w = rng.random((rows, 2)) * 0.5
            w = np.c_[w, 1.0 - w.sum(axis=1)]
            neg = rng.random(rows) < 0.1
            w[neg, 0] = -w[neg, 0]
            w[neg, 2] = 1.0 - w[neg, 0] - w[neg, 1]
            return v, np.ascontiguousarray(w)
        v1, w1 = simplices(ng, n)
        v2, w2 = simplices(n, ng)
        cell = np.arange(ng)
        moved = rng.random(ng) < 0.15
        cell[moved] = rng.integers(0, ng, int(moved.sum()))
        idx = np.ascontiguousarray(np.c_[cell // nx, cell % nx], np.int32)
        sdf = np.ascontiguousarray(np.abs(rng.standard_normal((ny, nx))) * (rng.random((ny, nx)) > 0.1))
        mx = np.ascontiguousarray(maxs, np.float64)
        cells = np.ascontiguousarray(rng.standard_normal((n, 5)))
        out = np.empty(n, np.float64)
        with GridSurrogate(model, ny, nx, 1) as sur:
            smd = int(name == "delta_partials")                # the deltas model's convention: normalise_sdf = fill_input = 1
            sur._chk(sur.lib.psm_set_geometry(sur.h, n, ny, nx, _p(v1, C.c_int32), _p(w1, C.c_double), _p(idx, C.c_int32), _p(sdf, C.c_double),
                                              _p(v2, C.c_int32), _p(w2, C.c_double), _p(mx, C.c_double), smd, smd, 0.05))
            for k in range(3 if smd else 2):
                solve = sur.lib.psm_solve_delta if smd else sur.lib.psm_solve
                sur._chk(solve(sur.h, _p(cells, C.c_double), n, 0, _p(out, C.c_double)))
                line(f"p solve{k + 1}", out.copy())
                if smd:                                      # the next time step: other velocities, the pressure just returned
                    cells[:, :2] += 0.1 * rng.standard_normal((n, 2))
                    cells[:, 4] = out
    elif name == "delta_host_umax":
        _, _, _, model, maxs = cases.build_mesh_case()
        sm = SolverModule(model, maxs, geometry="native", step="delta")
        sm.init_func(*synthetic.channel_mesh())
        sm.reset_state()                                     # init_func primes: forget it, the first step below is the priming step
        for step in range(3):
            line(f"p step{step + 1}", sm.py_func(synthetic.channel_mesh(step=step)[0]))
        sm._sur.close()
    elif name.startswith("cases_"):
        _, _, _, model, maxs = cases.build_mesh_case()
        delta = name.startswith("cases_delta")
        obstacles = (dict(), dict(cx=0.55, cy=0.05, R=0.06), dict(cx=0.9, cy=-0.08, R=0.1, step=2))[:int(name[-1])]
        mesh = [synthetic.channel_mesh(**kw) for kw in obstacles]
        se = SolverEnsemble(model, maxs, 4, geometry="native", step="delta" if delta else "absolute")
        se.init_func(*zip(*mesh))
        if delta:
            se.reset_state()                                 # as in delta_host_umax
        for step in range(3 if delta else 2):                # delta: the fields move from step to step
            arrays = [synthetic.channel_mesh(**dict(kw, step=kw.get("step", 0) + step))[0] if delta else m[0] for kw, m in zip(obstacles, mesh)]
            for k, p in enumerate(se.py_func(arrays)):
                line(f"p step{step + 1} case{k}", p)
        se._sur.close()
    elif name.startswith(("poisson_", "gradp_")):            # the two bound step kinds, through the classes that bind them
        OBSTACLES = (dict(), dict(cx=0.55, cy=0.05, R=0.06), dict(cx=0.9, cy=-0.08, R=0.1, step=2))
        if name.startswith("poisson_"):
            model = synthetic.make_model("deltas", p_in=48, p_out=40, c_in=4, seed_pca=777, seed_w=5)
            model.sdf_ch = 3
            kw = dict(maxs=(2.7, 0.004, 0.004, 0.35, 0.005), step="poisson", phi=0.16, k=0.5, weighting="noweight" not in name, apply_filter=True)
        else:
            model = synthetic.make_model("gradp", p_in=8, p_out=8)
            kw = dict(maxs=(2.5, 0.6, 0.35, 40.0, 25.0), step="gradp", apply_filter=True, sigma_field=(2.0, 3.0), sigma_weight=(2.0, 2.0),
                      reference="none" if "noref" in name else "outlet")
            OBSTACLES = (dict(), dict(step=2), dict(step=5))   # one obstacle (a cut the integration takes), three time levels of the fields
        if name.endswith("_k3"):
            mesh = [synthetic.channel_mesh(**o) for o in OBSTACLES]
            se = SolverEnsemble(model, max_cases=4, geometry="native", **kw)
            se.init_func(*zip(*mesh))                        # step='poisson': pushes the first frame
            for step in range(1, 5):                         # the fields move from step to step, p is the one just returned
                arrays = [synthetic.channel_mesh(**dict(o, step=o.get("step", 0) + step))[0] for o in OBSTACLES]
                if step > 1:
                    for a, p in zip(arrays, ps):
                        a[:, 4] = p
                ps = se.py_func(arrays)
                for k, p in enumerate(ps):
                    line(f"p step{step} case{k}", p)
            se._sur.close()
        else:
            sm = SolverModule(model, geometry="native", **kw)
            sm.init_func(*synthetic.channel_mesh())
            p = None
            for step in range(1, 5):                         # with the weighting the first call is a priming step too
                a = synthetic.channel_mesh(step=step)[0]
                if p is not None:
                    a[:, 4] = p
                p = sm.py_func(a)
                line(f"p step{step}", p)
            sm._sur.close()
    elif name == "mesh_to_grid":
        rng = np.random.default_rng(5)
        with GridSurrogate(synthetic.make_model("deltas", p_in=32, p_out=32), HY, HX, 1) as sur:
            hand_mesh(sur, HY, HX, HN)
            for k in (1, 3):
                values = np.ascontiguousarray(rng.standard_normal((HN, k)))
                values[7, 0] = np.nan
                for fill in (0, 1):
                    out = np.empty((HY, HX, k), np.float64)
                    sur._chk(sur.lib.psm_mesh_to_grid(sur.h, _p(values, C.c_double), HN, k, fill, _p(out, C.c_double)))
                    line(f"k={k} fill={fill}", out)
    elif name == "frames_to_grid":
        rng = np.random.default_rng(6)
        nf, k, npix = 2, 3, HY * HX
        cols = np.ascontiguousarray(rng.standard_normal((nf, HN, k)))
        cols[1, 3, 0] = cols[1, HN // 2, 1] = np.nan
        with GridSurrogate(synthetic.make_model("deltas", p_in=32, p_out=32), HY, HX, nf) as sur:
            hand_mesh(sur, HY, HX, HN)
            sur.bind_frames(nf, k)
            d_cols = DeviceArray(cols)
            d64, d32 = DeviceArray(np.full((nf, npix), -7.5, np.float64)), DeviceArray(np.full((nf, npix + 1), -7.5, np.float32))
            # column 0 -> a float64 plane, column 1 -> a float32 plane that starts 4- but not 8-byte aligned, column 2 is not stored
            sur.frames_to_grid_device(d_cols.ptr, nf, k, [(d64.ptr, npix, False), (d32.ptr + 4, npix + 1, True), (0, 0, 0)], fill=True)
            sur.synchronize()
            line("float64 planes", d64.numpy())
            line("float32 planes", d32.numpy())
            d_cols.free(), d64.free(), d32.free()
    elif name == "block_error":
        model = synthetic.make_model("deltas", p_in=32, p_out=32)
        grid = synthetic.channel_grid(256, 256, seed=9).astype(np.float32)
        labels = np.random.default_rng(10).standard_normal((256, 256, model.c_out)).astype(np.float32)
        with GridSurrogate(model, 256, 256, 1) as sur:
            sur.solve(grid[None])
            out = (C.c_double * 5)()
            sur._chk(sur.lib.psm_block_error(sur.h, _p(grid, C.c_float), _p(labels, C.c_float), out))
            line("5 doubles", np.array(list(out)))
            line("label blocks", sur.label_blocks(grid, labels))
    elif name == "field_errors":
        rng = np.random.default_rng(12)
        nf, npix = 2, HY * HX                                # 17030 = 4 * 4257 + 2: a ragged tail of the 4-pixel rounds
        f64 = lambda: rng.standard_normal((nf, npix))
        mask = f64() * (rng.random((nf, npix)) > 0.2)
        mask[0, 5] = np.nan                                  # a NaN SDF is no flow cell
        truth, add = f64(), f64()
        truth[1, 11] = truth[0, npix - 1] = np.nan
        add[0, 17] = np.nan
        sub = np.zeros((nf, npix + 1))                       # its planes start at element 1: dense, 8- but not 16-byte aligned
        sub[:, 1:] = f64()
        pred = rng.standard_normal((nf, npix)).astype(np.float32)
        pred[1, 23] = np.nan
        field = rng.standard_normal((nf, npix, 2)).astype(np.float32)      # a strided plane: channel 1 of an [npix][2] field
        with GridSurrogate(synthetic.make_model("deltas", p_in=32, p_out=32), HY, HX, nf) as sur:
            d = {k: DeviceArray(np.ascontiguousarray(v)) for k, v in dict(mask=mask, truth=truth, add=add, sub=sub, pred=pred, field=field).items()}
            d_raw = DeviceArray(np.zeros((nf, 2, 8)))
            dense = lambda a, f32=False: (d[a].ptr, npix, 1, f32)
            pairs = [(dense("pred", True), dense("truth"), None, None, False),
                     ((d["field"].ptr + 4, 2 * npix, 2, True), dense("truth"), dense("add"), (d["sub"].ptr + 8, npix + 1, 1, False), True)]
            sur.field_errors_device(dense("mask"), pairs, nf, d_raw.ptr)
            sur.synchronize()
            line("raw sums", d_raw.numpy())
            for a in list(d.values()) + [d_raw]:
                a.free()


def steps_config(name):
    """Runs in the child process: one line per output."""
    if STEPS[name] is None:                                  # pressure, poststeps: the configurations of OTHER, in a process of their own
        return other_config(name)
    import numpy as np
    import cases
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate, synthetic
    from test_poisson_step_device import K, MAX_ABS, P_SCALE, S_FIELD, S_WEIGHT, model4
    entry, n = STEPS[name]
    poisson, NF, CELLS = entry.startswith("poisson"), 3, 200
    fam, by_rows = entry.split("_")[0], entry.endswith("_rows")             # poisson / deltas / gradp / chapter4; frames as dataset rows
    chapter4 = entry.startswith("chapter4_frames")
    c4_in = 3 if entry.endswith("M_u") else 2
    c4_maxs = cases.DATASET_MAXS if c4_in == 3 else (cases.DATASET_MAXS[0],) + tuple(cases.DATASET_MAXS[2:])
    ny, nx = (320, 300) if fam == "gradp" else (138, 300)
    k = c4_in + 1 if chapter4 else {"poisson_step": 0, "poisson_frames": 7, "poisson_frames_errors": 8, "deltas_frames": 4, "gradp_frames": 6,
                                    "deltas_rows": 3, "gradp_rows": 5, "poisson_rows": 8}[entry]    # rows: the columns the stage writes
    npix, rng = ny * nx, np.random.default_rng(1901)
    vtx = rng.integers(0, CELLS, (npix, 3)).astype(np.int32)                    # the tables of tests/test_field_errors.py:flow_tables on this grid
    w = rng.random((npix, 2)) * 0.5
    wts = np.ascontiguousarray(np.c_[w, 1.0 - w.sum(axis=1)])
    idx = np.c_[np.arange(npix) // nx, np.arange(npix) % nx].astype(np.int32)
    sdf = 0.05 + 0.2 * rng.random((ny, nx))
    sdf[40:75, 30:70] = 0.0                                                     # no flow; rolled by 11 columns: the geometry that trips the guard
    cols = rng.standard_normal((NF, CELLS, max(k, 1))) * (1.0 + 0.3 * np.arange(NF))[:, None, None]
    if poisson and k:
        cols[..., 2:4] *= 0.05
        cols[..., k - 2] = np.abs(cols[..., k - 2]) / np.abs(cols[..., k - 2]).max(axis=1, keepdims=True)
        cols[..., k - 1] *= 0.1
        cols[0, 3:6, 4] = np.nan                                                # a label plane with NaN cells
    cols = np.ascontiguousarray(cols)
    width = 8 if fam == "gradp" else 11                                         # dataset rows: the least width of the kind
    rows = rng.standard_normal((NF, CELLS, width)).astype(np.float32) * (1.0 + 0.3 * np.arange(NF, dtype=np.float32))[:, None, None]
    rows[..., 5:7] *= np.float32(0.05)
    rows[..., 8:10] *= np.float32(0.05)
    base, phi, ex, ey = (cases.POISSON_MAXS[4] if poisson else cases.DATASET_MAXS[3]), 0.16, 1.45, 0.63
    U = [float(np.sqrt(cols[f, :, 0] ** 2 + cols[f, :, 1] ** 2).max()) for f in range(NF)] if k else [1.3, 1.7, 2.1]
    lu, u2 = np.array([[0.16, u] for u in U]), [u * u for u in U]
    scale = [P_SCALE * u * u for u in U]
    vel = np.ascontiguousarray(rng.standard_normal((NF, 4, ny, nx)) * (sdf != 0))
    dU, prev = np.abs(rng.standard_normal((NF, ny, nx))).astype(np.float32), (0.1 * rng.standard_normal((NF, ny, nx))).astype(np.float32)
    if poisson:
        model, c_in, sdf_scale = model4(), 4, MAX_ABS[3]
    elif fam == "deltas":
        model, c_in, sdf_scale = synthetic.make_model("deltas", p_in=48, p_out=40, c_in=3, seed_pca=778, seed_w=6), 3, cases.DATASET_MAXS[2]
    elif chapter4:
        model, c_in, sdf_scale = synthetic.make_model("chapter5", p_in=32, p_out=32, c_in=c4_in), c4_in, c4_maxs[-2]
        model.ov = 96
    else:
        model, c_in, sdf_scale = synthetic.make_model("gradp", p_in=32, p_out=32), 3, cases.GRADP_MAXS[2]
    model.sdf_ch = c_in - 1

    def handle(graph):
        os.environ["PSM_GRAPH"] = "1" if graph else "0"                          # read by psm_create
        sur = GridSurrogate(model, ny, nx, max_cases=NF)
        sur.set_mesh(vtx, wts, idx, sdf, CELLS)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        if poisson:
            sur.bind_features(np.repeat(sdf[None], NF, axis=0), K, MAX_ABS)
        if k:
            sur.bind_frames(NF, k)
        if fam == "deltas":
            sur.bind_deltas_frames(sdf, cases.DATASET_MAXS)
        if fam == "gradp":
            assert sur.bind_gradp_frames(sdf, cases.GRADP_MAXS, 57, 50, 1.0 / nx, 1.0 / ny)
        if by_rows:
            sur.bind_rows(width)
        if chapter4:
            sur.bind_chapter4_frames(sdf, c4_maxs)
        return sur

    def bind(sur, frames, other):                            # the frames' own geometry, or one whose flow-cell pattern is another
        one = not poisson                                    # the deltas and gradP frames are solved one by one: a single case is bound
        g = np.zeros((1 if one else frames, ny, nx, c_in), np.float32)
        g[..., c_in - 1] = ((np.roll(sdf, 11, axis=1) if other else sdf) / sdf_scale).astype(np.float32)[None]
        assert sur.bind_geometry(g[0] if one else g) and sur.geometry_bound

    def host_call(sur, frames, sc, af):
        c, s = cols[:frames], (scale[:frames] if sc else None)
        if entry == "deltas_rows":
            return dict(zip(("result", "truth", "raw", "scalars"), sur.deltas_rows(rows[:frames], base, apply_filter=af)))
        if entry == "gradp_rows":
            return dict(zip(("gradp", "p", "truth", "raw", "scalars"), sur.gradp_rows(rows[:frames], ex, ey, apply_filter=af)))
        if entry == "poisson_rows":
            return dict(zip(("result", "change", "next", "extra", "scalars"), sur.poisson_rows(rows[:frames], base, phi, apply_filter=af)))
        if entry == "poisson_frames":
            return dict(zip(("result", "change", "next", "extra"), sur.poisson_frames(c, lu[:frames], out_scale=s, apply_filter=af)))
        if entry == "poisson_frames_errors":
            return {"raw": sur.poisson_frames_errors(c, lu[:frames], out_scale=s, apply_filter=af)}
        if entry == "deltas_frames":
            return dict(zip(("result", "truth", "raw"), sur.deltas_frames(c, u2[:frames], out_scale=s, apply_filter=af)))
        if chapter4:
            return dict(zip(("result", "truth", "raw"), sur.chapter4_frames(c)))
        return dict(zip(("gradp", "p", "truth", "raw"), sur.gradp_frames(c, out_scale=s, apply_filter=af)))

    def device_call(sur, b, sc, af):
        s = scale[:n] if sc else None
        ptr = lambda key: C.c_void_p(b[key].ptr)
        if entry == "deltas_rows":                           # the rows' device entries have no Python mirror: the C entries
            sur._chk(sur.lib.psm_deltas_rows_device(sur.h, ptr("rows"), n, width, base, int(af), ptr("result"), ptr("truth"), ptr("raw"), ptr("scalars"), None))
        elif entry == "gradp_rows":
            sur._chk(sur.lib.psm_gradp_rows_device(sur.h, ptr("rows"), n, width, ex, ey, int(af), ptr("gradp"), ptr("p"), ptr("truth"), ptr("raw"),
                                                   ptr("scalars"), None))
        elif entry == "poisson_rows":
            sur._chk(sur.lib.psm_poisson_rows_device(sur.h, ptr("rows"), n, width, base, phi, int(af), 1, ptr("extra"), ptr("result"), ptr("change"),
                                                     ptr("next"), ptr("scalars"), None))
        elif entry == "poisson_step":
            sur.poisson_step_device(b["vel"].ptr, n, lu[:n], b["result"].ptr, af, b["dU"].ptr, b["prev"].ptr, b["change"].ptr, b["next"].ptr, out_scale=s)
        elif entry == "poisson_frames":
            sur.poisson_frames_device(b["cols"].ptr, n, k, lu[:n], b["result"].ptr, af, True, b["extra"].ptr, b["change"].ptr, b["next"].ptr, out_scale=s)
        elif entry == "poisson_frames_errors":
            sur.poisson_frames_errors_device(b["cols"].ptr, n, k, lu[:n], b["extra"].ptr, b["result"].ptr, b["next"].ptr, b["raw"].ptr, af, b["change"].ptr, out_scale=s)
        elif entry == "deltas_frames":
            sur.deltas_frames_device(b["cols"].ptr, n, k, u2[:n], b["result"].ptr, b["truth"].ptr, b["raw"].ptr, af, out_scale=s)
        elif chapter4:
            sur.chapter4_frames_device(b["cols"].ptr, n, k, b["result"].ptr, b["truth"].ptr, b["raw"].ptr)
        else:
            sur.gradp_frames_device(b["cols"].ptr, n, k, b["gradp"].ptr, b["p"].ptr, b["truth"].ptr, b["raw"].ptr, af, out_scale=s)
        sur.synchronize()
        return {key: b[key].numpy() for key in outputs}

    f32, f64 = np.float32, np.float64
    outputs = {"poisson_step": ("result", "change", "next"), "poisson_frames": ("result", "change", "next", "extra"),
               "poisson_frames_errors": ("result", "change", "next", "extra", "raw"), "deltas_frames": ("result", "truth", "raw"),
               "gradp_frames": ("gradp", "p", "truth", "raw"), "deltas_rows": ("result", "truth", "raw", "scalars"),
               "gradp_rows": ("gradp", "p", "truth", "raw", "scalars"),
               "poisson_rows": ("result", "change", "next", "extra", "scalars")}.get(entry, ("result", "truth", "raw"))
    shapes = {"result": ((NF, npix), f32), "change": ((NF, npix), f32), "next": ((NF, npix), f32), "extra": ((NF, max(k - 6, 1), npix), f64),
              "raw": ((NF, 4, 8), f64), "truth": ((NF, 3, npix), f64), "gradp": ((NF, npix, 2), f32), "p": ((NF, npix), f32), "scalars": ((NF, 8), f64)}
    line = lambda what, outs: [say(f"{name:28s} {what:34s} {key:7s} {sha(a)}") for key, a in outs.items() if a is not None]
    for graph in (False, True):
        with handle(graph) as sur:
            mode = "graph" if graph else "plain"
            if n == 0:                                       # host entry: bound (3 frames), then one frame on another geometry
                bind(sur, NF, other=False)
                line(f"{mode} host bound scale={int(not by_rows)} af=1", host_call(sur, NF, not by_rows, True))
                assert sur.guard_trips == 0 and sur.geometry_bound, "the frames' own geometry tripped the guard"
                bind(sur, 1, other=True)
                line(f"{mode} host trip scale=0 af=0", host_call(sur, 1, False, False))
                say(f"{name:28s} {mode} host trip: guard trips {sur.guard_trips}, still bound {sur.geometry_bound}")
                continue
            b = {key: DeviceArray(np.zeros(*shapes[key])) for key in outputs}
            b.update(vel=DeviceArray(vel), dU=DeviceArray(dU), prev=DeviceArray(prev), cols=DeviceArray(cols), rows=DeviceArray(rows))
            for sc in (False,) if chapter4 or by_rows else (False, True):      # the Chapter-4 entry takes neither, a rows entry no scale
                for af in (False,) if chapter4 else (False, True):
                    for rep in range(3 if graph else 1):     # graph: the capture and two replays
                        what = ("plain" if not graph else ("capture", "replay1", "replay2")[rep]) + f" scale={int(sc)} af={int(af)}"
                        line(what, device_call(sur, b, sc, af))
            for d in b.values():
                d.free()


def conv_config(name):
    """Runs in the child process: per precision the plan and the SHA-256 of the field of one forward pass."""
    import numpy as np
    from psm_amd import UNetSurrogate, synthetic
    widths, (ny, nx), n, c_in, _ = CONV[name]
    weights = synthetic.unet_he_weights(c_in, widths, 1, seed=23)
    grids = np.random.default_rng(5).standard_normal((n, ny, nx, c_in)).astype(np.float32)
    for precision in ("f32", "bf16"):
        with UNetSurrogate(weights, ny, nx, c_in=c_in, widths=widths, max_cases=n, precision=precision) as net:
            plan = " ".join("".join(str(v) for v in net.plan_info(i)) for i in range(len(weights)))
            say(f"{name:28s} {precision:4s} field={sha(net.forward(grids))}  plan={plan}")


def refusals_config():
    """Runs in the child process: one line per refused call, `<evaluator> <call> rc=<code> <psm_last_error>`.  The tables, frames and
    SDF plane of tests/test_field_errors.py (130 x 131, 200 cells, 3 frames); no post-steps are bound, so apply_filter is refused too.
    Every pointer that is not the one under test is a real buffer of the full size: a call that were NOT refused would stay in bounds."""
    import numpy as np
    import cases
    from hipmem import DeviceArray
    from psm_amd import GridSurrogate, _lib, synthetic
    from test_field_errors import NF, flow_tables
    os.environ["PSM_GRAPH"] = "0"
    t = flow_tables()
    npix, sdf = t.ny * t.nx, np.ascontiguousarray(t.sdfunct)
    f64p, f32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    chapter4 = synthetic.make_model("chapter5", p_in=32, p_out=32, c_in=3)
    chapter4.ov, chapter4.sdf_ch = 96, 2
    # evaluator: (model, scales, stored columns, rows width or 0, bind arguments behind the scales, float32 outputs per pixel)
    kinds = {"deltas": (synthetic.make_model("deltas", p_in=32, p_out=32), cases.DATASET_MAXS, 3, 11, ()),
             "gradp": (synthetic.make_model("gradp", p_in=32, p_out=32), cases.GRADP_MAXS, 5, 8, (57, 50, 1.0 / t.nx, 1.0 / t.ny)),
             "chapter4": (chapter4, cases.DATASET_MAXS, 3, 0, ())}
    for ev, (model, maxs, k0, width, bind_tail) in kinds.items():
        with GridSurrogate(model, t.ny, t.nx, max_cases=NF) as sur:
            lib, h = sur.lib, sur.h
            sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
            cols, rows = np.zeros((NF + 1, t.n_cells, 16)), np.zeros((NF + 1, t.n_cells, 16), np.float32)
            u2, mx = np.ones(NF + 1), np.array(maxs, np.float64)
            d = {key: DeviceArray(np.zeros((NF + 1) * 3 * npix + 2, dt)) for key, dt in
                 dict(cols=np.float64, rows=np.float32, grid=np.float32, label=np.float32, a=np.float32, b=np.float32, truth=np.float64,
                      raw=np.float64, scalars=np.float64).items()}
            host = {key: np.zeros((NF + 1) * 3 * npix, dt) for key, dt in dict(a=np.float32, b=np.float32, truth=np.float64, raw=np.float64, scalars=np.float64).items()}

            def call(what, n=NF, k=k0, af=0, off={}, null=()):
                """One call of entry `what` with n frames, k columns; off: byte offsets added to device pointers; null: pointers passed as NULL."""
                P = lambda key: None if key in null else C.c_void_p(d[key].ptr + off.get(key, 0))
                H = lambda key: None if key in null else (f32p if host[key].dtype == np.float32 else f64p)(host[key])
                U2 = None if "U2" in null else f64p(u2)
                c_cols, c_rows = (None if "cols" in null else f64p(cols)), (None if "rows" in null else f32p(rows))
                if what == "image":
                    lead = (h, P("cols"), n, k) + ((U2, P("grid"), P("label")) if ev == "deltas" else (P("grid"),))
                    return getattr(lib, f"psm_{ev}_image_device")(*lead, P("truth"), None)
                if what == "device":
                    args = {"deltas": (U2, None, af, P("a"), P("truth"), P("raw")), "gradp": (None, af, P("a"), P("b"), P("truth"), P("raw")),
                            "chapter4": (P("a"), P("truth"), P("raw"))}[ev]
                    return getattr(lib, f"psm_{ev}_frames_device")(h, P("cols"), n, k, *args, None)
                if what == "host":
                    args = {"deltas": (U2, None, af, H("a"), H("truth"), H("raw")), "gradp": (None, af, H("a"), H("b"), H("truth"), H("raw")),
                            "chapter4": (H("a"), H("truth"), H("raw"))}[ev]
                    return getattr(lib, f"psm_{ev}_frames")(h, c_cols, n, k, *args)
                lead = (h, P("rows") if what == "rows_device" else c_rows, n, width) + ((1.0, af) if ev == "deltas" else (1.45, 0.63, af))
                outs = (P if what == "rows_device" else H)
                tail = (outs("a"), outs("truth"), outs("raw"), outs("scalars")) if ev == "deltas" else (outs("a"), outs("b"), outs("truth"), outs("raw"), outs("scalars"))
                return getattr(lib, f"psm_{ev}_{what}")(*lead, *tail, *((None,) if what == "rows_device" else ()))

            def bind(m=mx, tail=bind_tail):
                return getattr(lib, f"psm_bind_{ev}_frames")(h, f64p(sdf), f64p(np.ascontiguousarray(m, np.float64)), *tail)

            def note(label, rc):
                msg = _lib.last_error(h) if rc else ""
                say(f"{ev:9s} {label:44s} rc={rc} {msg}")
            entries = ["image", "device", "host"] + (["rows_device", "rows"] if width else [])
            note("bind, frames unbound", bind())
            for e in entries:
                note(f"{e}, frames unbound", call(e))
            sur.bind_frames(NF, k0)
            if width:
                sur.bind_rows(width)
            for e in entries:
                note(f"{e}, evaluator binding unbound", call(e))
            for q, bad in ((2, 0.0), (0, np.inf), (len(mx) - 1, np.nan)):
                m = mx.copy()
                m[q] = bad
                note(f"bind, scale {q} = {bad}", bind(m))
            if ev == "gradp":
                note("bind, the cut the reference raises on", bind(tail=(57, 30) + bind_tail[2:]))
                note("bind, a cut outside the grid", bind(tail=(t.ny, 50) + bind_tail[2:]))
            for e in entries:
                note(f"{e}, after the refused binds", call(e))
            note("bind", bind())
            for e in entries[:3]:                            # the rows entries take no k
                for k in (k0 - 1, 17):
                    note(f"{e}, k = {k}", call(e, k=k))
            for e in entries:
                for n in (0, NF + 1):
                    note(f"{e}, n_frames = {n}", call(e, n=n))
                note(f"{e}, input NULL", call(e, null=("rows" if e.startswith("rows") else "cols",)))
            note("image, d_grid NULL", call("image", null=("grid",)))
            note("image, d_grid 2 bytes off", call("image", off={"grid": 2}))
            note("image, d_truth 4 bytes off", call("image", off={"truth": 4}))
            if ev == "deltas":
                note("image, d_label 2 bytes off", call("image", off={"label": 2}))
                note("image, d_truth without U2", call("image", null=("U2",)))
                note("device, U2 NULL", call("device", null=("U2",)))
                note("host, U2 NULL", call("host", null=("U2",)))
            for e in ("device", "rows_device")[:2 if width else 1]:
                for key, half in (("a", 4 if ev == "gradp" else 2), ("b", 2), ("truth", 4), ("raw", 4), ("scalars", 4)):
                    if (key == "b" and ev != "gradp") or (key == "scalars" and e == "device"):
                        continue
                    note(f"{e}, {key} {half} bytes off", call(e, off={key: half}))
            if ev != "chapter4":
                for e in entries[1:]:
                    note(f"{e}, apply_filter without post-steps", call(e, af=1))
            note("host, nothing wanted", call("host", null=("a", "b", "truth", "raw")))
            sur.synchronize()
            for a in d.values():
                a.free()


def children(names, lib, flag, envs):
    """One child process per configuration, its switches in its environment; the children's lines are repeated here."""
    import subprocess
    for name in names:
        env = dict(os.environ, **envs.get(name, {}))
        for k in ("PSM_DEVICE_UMAX", "PSM_MESH_GRAPH"):
            if k not in envs.get(name, {}):
                env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), flag, name] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        for ln in r.stdout.splitlines():
            say(ln)
        if r.returncode:
            say(f"{name:28s} FAILED exit {r.returncode}: {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ''}")
            return r.returncode                              # nothing more on the GPU after a child that died
    return 0


def boundary(names, lib):
    return children(names, lib, "--boundary-child", BOUNDARY)


def dispatches(paths):
    """The dispatches of rocprofv3 kernel traces in the order they started: kernel name, grid, workgroup, LDS and scratch bytes."""
    import csv
    for p in paths:
        rows = sorted(csv.DictReader(open(p)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            dims = lambda k: "x".join(r[f"{k}_Size_{a}"] for a in "XYZ")
            lds = next(v for k, v in r.items() if k.startswith("LDS"))
            scr = next(v for k, v in r.items() if k.startswith("Scratch"))
            print(f"{r['Kernel_Name']} grid={dims('Grid')} wg={dims('Workgroup')} lds={lds} scratch={scr}")


def table(paths):
    """Lists of --dispatches in compact form, nothing lost: every distinct line once, numbered in order of first appearance over all
    lists, then each list as the numbers of its lines, 40 to a row."""
    lists = [open(p).read().splitlines() for p in paths]
    ids = {}
    for line in (l for ls in lists for l in ls):
        ids.setdefault(line, len(ids))
    for line, k in ids.items():
        print(f"{k:4d} {line}")
    for p, ls in zip(paths, lists):
        print(f"== {os.path.basename(p)}: {len(ls)} dispatches, sha256 of the list {hashlib.sha256(chr(10).join(ls).encode()).hexdigest()[:16]}")
        for i in range(0, len(ls), 40):
            print(" ".join(str(ids[l]) for l in ls[i:i + 40]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", nargs="+", metavar="LIST")
    ap.add_argument("--dispatches", nargs="+", metavar="CSV")
    ap.add_argument("--lib")
    ap.add_argument("--only")
    ap.add_argument("--mesh-graph", default="2", choices=["0", "1", "2"])
    ap.add_argument("--out")
    ap.add_argument("--boundary-child", help=argparse.SUPPRESS)
    ap.add_argument("--steps-child", help=argparse.SUPPRESS)
    ap.add_argument("--refusals-child", help=argparse.SUPPRESS)
    ap.add_argument("--conv-child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.dispatches:
        return dispatches(args.dispatches)
    if args.table:
        return table(args.table)
    if args.lib:
        os.environ["PSM_LIB"] = os.path.abspath(args.lib)
    if args.boundary_child:
        return boundary_config(args.boundary_child)
    if args.steps_child:
        return steps_config(args.steps_child)
    if args.refusals_child:
        return refusals_config()
    if args.conv_child:
        return conv_config(args.conv_child)
    only = args.only.split(",") if args.only else []
    group = next((g for g, names in (("boundary", BOUNDARY), ("steps", STEPS), ("refusals", REFUSALS), ("conv", CONV)) if only and all(n == g or n in names for n in only)), None)
    if group:                                                            # the parent process never opens the GPU
        if group == "boundary":
            say(f"# tools/route_matrix.py boundary lib={args.lib or 'libpsm_hip.so of the tree'}")
            rc = boundary([b for n in only for b in (BOUNDARY if n == "boundary" else [n])], args.lib)
        elif group == "refusals":
            say("# tools/route_matrix.py refusals")
            rc = children(["refusals"], args.lib, "--refusals-child", {})
        elif group == "conv":
            say("# tools/route_matrix.py conv")
            rc = children([b for n in only for b in (CONV if n == "conv" else [n])], args.lib, "--conv-child", {k: v[4] for k, v in CONV.items()})
        else:                                                            # no library path in the output: two libraries' runs are compared with cmp
            say("# tools/route_matrix.py steps")
            rc = children([b for n in only for b in (STEPS if n == "steps" else [n])], args.lib, "--steps-child", {})
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(_lines) + "\n")
        return rc
    os.environ["PSM_MESH_GRAPH"] = args.mesh_graph
    for k in ("PSM_X6", "PSM_LN_FUSE", "PSM_KEEP_HIDDEN", "PSM_NO_BIND", "PSM_RING_GRAPH"):
        os.environ.pop(k, None)
    from psm_amd import _lib
    _lib.load()
    names = args.only.split(",") if args.only else list(GRID_CONFIGS) + OTHER
    say(f"# tools/route_matrix.py lib={os.path.relpath(_lib.LIB_PATH, ROOT)} mesh_graph={args.mesh_graph}")
    for name in names:
        grid_config(name) if name in GRID_CONFIGS else other_config(name)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
