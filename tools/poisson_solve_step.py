"""What the Poisson-model step at the solver boundary costs: psm_solve_poisson (cells [N,5] -> p [N], the state on the device, one
graph replay) against the loop a user had to write with the entries that existed before -- keep U(t-1), U(t-2) and p(t-2), NumPy
columns and scalars, psm_poisson_frames, `next` back, the NumPy grid -> mesh + fallback + p(t-1) + dp -- on ANOTHER build of the
library when one is given (--parent-lib: the parent commit's), else on this one.  The 16 021-cell channel mesh on its 138 x 300
grid behind the four-channel model (p_in = 48, p_out = 40), weighting and filter on, tables from the native builder, plain host arrays.

The legs alternate in one process, round by round; every call ends in a device synchronise and is timed on its own.  Per leg: the
median and the p10 .. p90 range over all calls.  Both legs are checked to agree on dp before anything is timed.

    python tools/poisson_solve_step.py [--parent-lib PATH] [--steps 300] [--rounds 6] [--out FILE]
    python tools/poisson_solve_step.py --trace-leg solve --steps N    the new entry alone, for a kernel trace
    python tools/poisson_solve_step.py --kernels STATS.csv            the three new launches' rows of a trace's kernel stats
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
from psm_amd import GridSurrogate, _lib, synthetic  # noqa: E402
from delta_step import alternate, native_tables, other_build, quantiles  # noqa: E402

PHI, K = 0.16, 0.5
MAXS5 = (2.7, 0.004, 0.004, 0.35, 0.005)
S_FIELD, S_WEIGHT = (10, 10), (50, 50)
NEW_KERNELS = ("psm_umax_partial_kernel(PsmPoissonCellsArgs)", "psm_interp_to_grid_kernel(PsmPoissonCellsArgs)", "psm_to_mesh_kernel(PsmPoissonMeshArgs)")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def model4():
    m = synthetic.make_model("deltas", p_in=48, p_out=40, c_in=4, seed_pca=777, seed_w=5)
    m.sdf_ch = 3
    return m


def bound_handle(model, tables, n_cells, lib=None, solve=True):
    """A handle on the single mesh with features, post-steps and frames (1, 6) bound, and the step itself with `solve`."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    keep, _lib._lib = _lib._lib, lib or _lib.load()         # GridSurrogate binds whatever _lib.load() returns
    try:
        sur = GridSurrogate(model, ny, nx, 1)
    finally:
        _lib._lib = keep
    mx = np.asarray(MAXS5[1:], np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, n_cells, ny, nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                  sdf.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    if rc:
        raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
    sur.mesh_cells = n_cells
    sur.bind_features(sdf.reshape(ny, nx), K, MAXS5[:4])
    sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_frames(1, 6)
    if solve:
        sur.bind_poisson_solve(PHI, MAXS5[4], True, True)
    return sur


def new_leg(sur, arrays):
    """-> f(i): one psm_solve_poisson on arrays[i % len]; the state rotates with the calls as in a solver."""
    out = np.empty(len(arrays[0]))
    ptrs, po, n, h, fn = [a.ctypes.data_as(_dp) for a in arrays], out.ctypes.data_as(_dp), len(arrays[0]), sur.h, sur.lib.psm_solve_poisson

    def call(i):
        if fn(h, ptrs[i % len(ptrs)], n, 0, po):
            raise RuntimeError(sur.lib.psm_last_error(h).decode())
    call.out = out
    return call


def user_leg(sur, arrays, tables):
    """-> f(i): the same step written with what existed before: the caller keeps two frames, makes the six columns and the scalars in
    NumPy, calls psm_poisson_frames, takes `next` back and does grid -> mesh, the fallback rule and p(t-1) + dp itself."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    n = len(arrays[0])
    pix = idx[:, 0].astype(np.int64) * nx + idx[:, 1]
    sdf_mesh = np.einsum("nj,nj->n", sdf.reshape(-1)[v2], w2)
    fallback = (sdf_mesh < 0.05) | (w2 < 0).any(axis=1)
    cell_of_vertex = pix[v2]                                 # [N,3] pixel of every vertex: the gather's table, made once
    state = {"a1": arrays[-1], "a0": arrays[-2]}
    cols = np.empty((1, n, 6))
    result, change, nxt = (np.empty((1, ny, nx, 1), np.float32), np.empty((1, ny, nx), np.float32), np.empty((1, ny, nx), np.float32))
    lu, sc = np.empty((1, 2)), np.empty(1, np.float32)
    out = np.empty(n)
    lib, h = sur.lib, sur.h
    fp = C.POINTER(C.c_float)

    def call(i):
        a2, a1, a0 = arrays[i % len(arrays)], state["a1"], state["a0"]
        U = np.sqrt(np.max(np.square(a2[:, 0]) + np.square(a2[:, 1])))
        dU = a2[:, 0:2] - a1[:, 0:2]
        cc = np.abs(dU - (a1[:, 0:2] - a0[:, 0:2])).sum(axis=-1)
        c = cc.max()
        cols[0, :, 0:2] = a2[:, 0:2]; cols[0, :, 2:4] = dU
        cols[0, :, 4] = cc / c if c != 0 else 0.0
        cols[0, :, 5] = a2[:, 4] - a1[:, 4]
        lu[0] = (PHI, U); sc[0] = MAXS5[4] * U * U
        if lib.psm_poisson_frames(h, cols.ctypes.data_as(_dp), 1, 6, lu.ctypes.data_as(_dp), sc.ctypes.data_as(fp), 1, 1, None,
                                  result.ctypes.data_as(fp), change.ctypes.data_as(fp), nxt.ctypes.data_as(fp)):
            raise RuntimeError(lib.psm_last_error(h).decode())
        dp = np.einsum("nj,nj->n", nxt.reshape(-1)[cell_of_vertex].astype(np.float64), w2)
        np.add(a2[:, 4], dp, out=out)
        fb = fallback | np.isnan(dp)
        out[fb] = a2[fb, 4]
        state["a0"], state["a1"] = a1, a2
    call.out = out
    return call


def kernels(path):
    """The three new launches' rows of a `rocprofv3 --kernel-trace --stats` kernel-stats CSV."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if any(k.split("(")[0] in r["Name"] and k.split("(")[1].rstrip(")") in r["Name"] for k in NEW_KERNELS)]
    for r in rows:
        print(f"  {r['Name'][:70]:70s} {int(r['Calls']):6d} calls  {float(r['AverageNs']) / 1e3:7.2f} us mean  ({float(r['MinNs']) / 1e3:.2f} .. {float(r['MaxNs']) / 1e3:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-leg", default=None, choices=("solve",))
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    model = model4()
    a0, top, obst = synthetic.channel_mesh()
    a0 = np.ascontiguousarray(a0)
    arrays = [np.ascontiguousarray(synthetic.channel_mesh(step=k)[0]) for k in (3, 5, 6)]
    tables = native_tables(a0, top, obst)
    # A solver's tables carry lattice points outside the mesh hull (a negative weight: interpolate_fill makes them NaN, and they all
    # land in pixel (0,0)).  psm_solve_poisson zeroes that NaN in the two weighting planes; psm_poisson_frames, made for the evaluator's
    # tables, keeps it, and the sigma = 50 filter would spread it over the user loop's whole field.  So that the loop can be written at
    # all, such points take their first vertex's value here, for both legs.
    outside = (tables[3] < 0).any(axis=1)
    tables[3][outside] = (1.0, 0.0, 0.0)
    sur = bound_handle(model, tables, len(a0))
    sur.poisson_solve_push(arrays[-2]); sur.poisson_solve_push(arrays[-1])       # the state both legs start from
    new = new_leg(sur, arrays)
    if args.trace_leg:
        for i in range(args.steps):
            new(i)
        print(f"psm_solve_poisson: {args.steps} calls")
        return sur.close()
    old = bound_handle(model, tables, len(a0), other_build(args.parent_lib) if args.parent_lib else None, solve=False)
    user = user_leg(old, arrays, tables)
    lines, records = [], []
    # both legs make the same step: the same frames in the same order, dp compared on the cells neither falls back on
    worst = 0.0
    for i in range(3):
        new(i); user(i)
        moved = new.out != arrays[i][:, 4]
        assert np.array_equal(moved, user.out != arrays[i][:, 4]), "the legs fall back on different cells"
        dp_new, dp_user = new.out[moved] - arrays[i][moved, 4], user.out[moved] - arrays[i][moved, 4]
        worst = max(worst, float(np.abs(dp_new - dp_user).max() / np.abs(dp_user).max()))
    assert worst < 1e-6, worst
    lines.append(f"both legs on the same three steps: the same fallback cells, max|dp_new - dp_user| / max|dp_user| = {worst:.2e}")
    samples = alternate({"psm_solve_poisson": new, "user loop": user}, args.steps, args.rounds, args.warmup)
    q = {name: quantiles(us) for name, us in samples.items()}
    where = "the parent build" if args.parent_lib else "this build"
    lines.append(f"single mesh, {len(a0)} cells, {tables[0]} x {tables[1]} grid, weighting and filter on, {args.rounds} rounds of {args.steps} calls per leg")
    for name, r in q.items():
        label = name if name != "user loop" else f"user loop (NumPy columns + psm_poisson_frames of {where} + NumPy grid -> mesh)"
        lines.append(f"  {label:90s} {r['median_us']:8.2f} us per step (p10 .. p90: {r['p10_us']:.2f} .. {r['p90_us']:.2f}; {r['calls']} calls)")
    lines.append(f"  user loop / psm_solve_poisson = {q['user loop']['median_us'] / q['psm_solve_poisson']['median_us']:.2f}")
    records.append({"cells": len(a0), "parent_lib": bool(args.parent_lib), "legs": q})
    sur.close(); old.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
