"""One smallest shape per route of the PCA solve path: for every configuration one solve by plain launches, then a capture and
two graph replays (PSM_GRAPH=1 handle), and a SHA-256 of the output of the plain solve and of each graph solve.  Two builds of
the library that take the same routes print the same table, and under `rocprofv3 --kernel-trace` dispatch the same kernels in
the same order (--dispatches prints a trace as one line per dispatch, to be compared with diff):

    python tools/route_matrix.py [--lib SO] [--only NAME,...] [--mesh-graph 0|1|2] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_matrix.py --lib tools/_bin/libpsm_base.so
    python tools/route_matrix.py --dispatches DIR/.../*_kernel_trace.csv     (no GPU needed)
    python tools/route_matrix.py --table LIST_A LIST_B      two such lists as one numbered table of the distinct lines + each list as numbers

--lib: the library to load (default: the tree's libpsm_hip.so), e.g. the parent commit's build.  PSM_MESH_GRAPH is read once per
process: the `mesh` configuration runs in the mode --mesh-graph sets (default 2), so the three modes take three runs.
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
    args = ap.parse_args()
    if args.dispatches:
        return dispatches(args.dispatches)
    if args.table:
        return table(args.table)
    if args.lib:
        os.environ["PSM_LIB"] = os.path.abspath(args.lib)
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
    main()
