"""What the gradient-model step at the solver boundary costs: psm_solve_gradp (cells [N,5] -> p [N], one graph replay) and
psm_solve_cases_gradp (K meshes, one replay) against the loop a user has to write with the entries that existed before --
psm_mesh_to_grid of (Ux, Uy) / U, the NumPy image, psm_solve_pressure, the NumPy outlet shift, gather, fallback and U^2 -- on ANOTHER
build of the library when one is given (--parent-lib: the parent commit's), else on this one; for K cases that loop runs on K
single-mesh handles in turn.  The 16 021-cell channel mesh on its 138 x 300 grid behind the gradP model (p_in = p_out = 128), tables
from the native builder, no filter, reference = outlet, plain host arrays.

The legs alternate in one process, round by round; every call ends in a device synchronise and is timed on its own.  Per leg: the
median and the p10 .. p90 range over all calls.  Both legs are checked to agree on p before anything is timed.

    python tools/gradp_solve_step.py [--parent-lib PATH] [--cases 1,4,8] [--steps 300] [--rounds 6] [--out FILE]
    python tools/gradp_solve_step.py --trace-leg solve|cases --steps N    the new entry alone (cases: K = 4), for a kernel trace
    python tools/gradp_solve_step.py --kernels STATS.csv                  the tail launch's rows of a trace's kernel stats
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from psm_amd import GridSurrogate, _lib, solver, synthetic  # noqa: E402
from delta_step import alternate, native_tables, other_build, quantiles  # noqa: E402

MAXS4 = (2.5, 0.6, 0.35, 1.0)            # max_abs_Ux, max_abs_Uy, max_abs_dist, unused
MAX_GRAD = (40.0, 25.0)                  # max_abs_dPdx, max_abs_dPdy
NEW_KERNELS = ("psm_to_mesh_kernel(PsmGradpMeshArgs)", "psm_to_mesh_kernel(PsmGradpCasesArgs)")
TOL = 2e-4
_dp, _ip, _fp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)


def on_build(lib, make):
    keep, _lib._lib = _lib._lib, lib or _lib.load()         # GridSurrogate binds whatever _lib.load() returns
    try:
        return make()
    finally:
        _lib._lib = keep


def single_handle(model, tables, n_cells, lib=None):
    """A handle on the single mesh with the gradP model's flags (normalise_sdf = fill_input = 1), on `lib` or the loaded build."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    sur = on_build(lib, lambda: GridSurrogate(model, ny, nx, 1))
    mx = np.asarray(MAXS4, np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, n_cells, ny, nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                  sdf.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    if rc:
        raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
    sur.mesh_cells = n_cells
    return sur


def case_handle(model, tables, n_cells, n_cases, geo):
    """One handle on a case set of `n_cases` meshes with these tables and the step bound."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    sur = GridSurrogate(model, ny, nx, n_cases)
    ptrs = lambda a: (C.c_void_p * n_cases)(*[a.ctypes.data] * n_cases)
    mx = np.asarray(MAXS4, np.float64)
    rc = sur.lib.psm_set_geometry_cases(sur.h, n_cases, (C.c_int64 * n_cases)(*[n_cells] * n_cases), ny, nx, ptrs(v1), ptrs(w1), ptrs(idx), ptrs(sdf),
                                        ptrs(v2), ptrs(w2), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    if rc:
        raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
    cut, dx, dy, extents = geo
    sur.bind_gradp_solve_cases([cut] * n_cases, dx, dy, extents, MAX_GRAD, False, "outlet")
    return sur


def new_leg(sur, frames):
    """-> f(i): one psm_solve_gradp (one case) or psm_solve_cases_gradp on the cases' frames i % len, concatenated once."""
    cells = [np.ascontiguousarray(np.concatenate([f[s] for f in frames])) for s in range(len(frames[0]))]
    out = np.empty(len(cells[0]))
    ptrs, po, h, n, single = [c.ctypes.data_as(_dp) for c in cells], out.ctypes.data_as(_dp), sur.h, len(cells[0]), len(frames) == 1
    fn = sur.lib.psm_solve_gradp if single else sur.lib.psm_solve_cases_gradp

    def call(i):
        if fn(h, ptrs[i % len(ptrs)], n, 0, po) if single else fn(h, ptrs[i % len(ptrs)], po):
            raise RuntimeError(sur.lib.psm_last_error(h).decode())
    call.out = out
    return call


def user_leg(surs, frames, tables, geo):
    """-> f(i): the same step written with what existed before, on every handle in turn: psm_mesh_to_grid of (Ux, Uy) / U, the image
    in NumPy (scales, SDF channel, NaN -> 0, float32), psm_solve_pressure with the integration bound on (sx, sy), then the outlet
    shift, grid -> mesh, the fallback rule and U^2 in NumPy."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    n, ng = len(frames[0][0]), ny * nx
    cut, dx, dy, extents = geo
    sx, sy = dx * MAX_GRAD[0] / extents[0], dy * MAX_GRAD[1] / extents[1]
    for sur in surs:
        if not sur.bind_integration(sdf.reshape(ny, nx), cut[0], cut[1], sx, sy):
            raise RuntimeError("the cut cannot be integrated")
    pix = idx[:, 0].astype(np.int64) * nx + idx[:, 1]
    sdf_mesh = np.einsum("nj,nj->n", sdf.reshape(-1)[v2], w2)
    fallback = (sdf_mesh < 0.05) | (w2 < 0).any(axis=1)
    cell_of_vertex = pix[v2]                                 # [N,3] pixel of every vertex: the gather's table, made once
    sdn = np.nan_to_num(sdf / MAXS4[2]).astype(np.float32)
    vals, planes = np.empty((n, 2)), np.empty((ng, 2))
    image, q = np.empty((ny, nx, 3), np.float32), np.empty((ny, nx), np.float32)
    image[..., 2] = sdn.reshape(ny, nx)
    out = np.empty(len(surs) * n)

    def call(i):
        for k, sur in enumerate(surs):
            a = frames[k][i % len(frames[k])]
            lib, h = sur.lib, sur.h
            U = np.sqrt(np.max(np.square(a[:, 0]) + np.square(a[:, 1])))
            np.divide(a[:, 0:2], U, out=vals)
            if lib.psm_mesh_to_grid(h, vals.ctypes.data_as(_dp), n, 2, 1, planes.ctypes.data_as(_dp)):
                raise RuntimeError(lib.psm_last_error(h).decode())
            image[..., 0] = np.nan_to_num(planes[:, 0] / MAXS4[0]).reshape(ny, nx)
            image[..., 1] = np.nan_to_num(planes[:, 1] / MAXS4[1]).reshape(ny, nx)
            if lib.psm_solve_pressure(h, image.ctypes.data_as(_fp), 1, None, q.ctypes.data_as(_fp)):
                raise RuntimeError(lib.psm_last_error(h).decode())
            q64 = q.astype(np.float64)
            s = np.mean(3.0 * q64[:, -1] - q64[:, -2]) / 3.0
            acc = np.einsum("nj,nj->n", q64.reshape(-1)[cell_of_vertex] - s, w2)
            o = out[k * n:(k + 1) * n]
            np.multiply(acc, U * U, out=o)
            fb = fallback | np.isnan(acc)
            o[fb] = a[fb, 4]
    call.out = out
    return call


def kernels(path):
    """The tail launch's rows of a `rocprofv3 --kernel-trace --stats` kernel-stats CSV, then every kernel of the trace."""
    with open(path) as f:
        rows = list(csv.DictReader(f))
    new = [r for r in rows if any(k.split("(")[0] in r["Name"] and k.split("(")[1].rstrip(")") in r["Name"] for k in NEW_KERNELS)]
    for r in new:
        print(f"  {r['Name'][:70]:70s} {int(r['Calls']):6d} calls  {float(r['AverageNs']) / 1e3:7.2f} us mean  ({float(r['MinNs']) / 1e3:.2f} .. {float(r['MaxNs']) / 1e3:.2f})")
    print("All kernels of that trace, mean per launch:")
    for r in rows:
        print(f"  {r['Name'][:100]:100s} {int(r['Calls']):6d} calls  {float(r['AverageNs']) / 1e3:7.2f} us  {float(r['Percentage']):6.2f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cases", default="1,4,8")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-leg", default=None, choices=("solve", "cases"))
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    model = synthetic.make_model("gradp")
    a0, top, obst = synthetic.channel_mesh()
    a0 = np.ascontiguousarray(a0)
    n = len(a0)
    tables = native_tables(a0, top, obst)
    ny, nx, sdf = tables[0], tables[1], tables[5]
    dx, dy, extents, _ = solver.gradp_grid_metrics(a0, ny, nx)
    geo = (solver.gradp_default_cut(sdf.reshape(ny, nx), a0, 5e-3), dx, dy, extents)
    frames_of = lambda k: [np.ascontiguousarray(synthetic.channel_mesh(step=k + s)[0]) for s in (3, 5, 6)]

    def new_handle(nc):
        if nc > 1:
            return case_handle(model, tables, n, nc, geo)
        sur = single_handle(model, tables, n)
        sur.bind_gradp_solve(geo[0], dx, dy, extents, MAX_GRAD, False, "outlet")
        return sur

    if args.trace_leg:
        nc = 4 if args.trace_leg == "cases" else 1
        sur = new_handle(nc)
        call = new_leg(sur, [frames_of(k) for k in range(nc)])
        for i in range(args.steps):
            call(i)
        print(f"{'psm_solve_cases_gradp, K = 4' if nc > 1 else 'psm_solve_gradp'}: {args.steps} calls")
        return sur.close()
    parent = other_build(args.parent_lib) if args.parent_lib else None
    where = "the parent build" if args.parent_lib else "this build"
    lines, records = [f"cut {geo[0]}, dx {dx:.6f}, dy {dy:.6f}, extents {extents}, max_abs_grad {MAX_GRAD}, reference outlet, no filter"], []
    for nc in [int(v) for v in args.cases.split(",")]:
        frames = [frames_of(k) for k in range(nc)]
        sur = new_handle(nc)
        olds = [single_handle(model, tables, n, parent) for _ in range(nc)]
        a, b = new_leg(sur, frames), user_leg(olds, frames, tables, geo)
        # both legs make the same steps: the same frames in the same order, p compared per case on the cells neither falls back on
        worst = 0.0
        for i in range(3):
            a(i); b(i)
            for k in range(nc):
                prev, pa, pb = frames[k][i][:, 4], a.out[k * n:(k + 1) * n], b.out[k * n:(k + 1) * n]
                moved = pa != prev
                assert np.array_equal(moved, pb != prev), "the legs fall back on different cells"
                worst = max(worst, float(np.abs(pa[moved] - pb[moved]).max() / np.abs(pb[moved]).max()))
        assert worst <= TOL, worst
        entry = "psm_solve_gradp" if nc == 1 else "psm_solve_cases_gradp"
        samples = alternate({"new": a, "user loop": b}, args.steps, args.rounds, args.warmup)
        q = {name: quantiles(us) for name, us in samples.items()}
        lines.append(f"K = {nc} ({n} cells per case, {ny} x {nx} grid, {args.rounds} rounds of {args.steps} steps per leg; both legs on the same three "
                     f"steps: the same fallback cells, max|p_new - p_user| / max|p_user| = {worst:.2e})")
        for name, what in (("new", f"1 handle, {entry}"),
                           ("user loop", f"{nc} handle(s) of {where}: psm_mesh_to_grid + NumPy image + psm_solve_pressure + NumPy tail")):
            r = q[name]
            lines.append(f"  {what:100s} {r['median_us']:8.2f} us per step (p10 .. p90: {r['p10_us']:.2f} .. {r['p90_us']:.2f}) = "
                         f"{r['median_us'] / nc:7.2f} us per case ({r['calls']} calls)")
        lines.append(f"  user loop / {entry} = {q['user loop']['median_us'] / q['new']['median_us']:.2f}")
        records.append({"cases": nc, "cells_per_case": n, "parent_lib": bool(args.parent_lib), "legs": q})
        sur.close()
        for s in olds:
            s.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
