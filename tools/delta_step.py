"""What the delta step costs over the absolute one at the solver boundary: psm_solve_delta against psm_solve on the SAME handle
(the cost floor: same launches, absolute semantics) and against psm_solve of ANOTHER build of the library (--parent-lib: the check
that the existing route did not move), on the 16 k-cell channel mesh behind make_model("deltas", p_in=32, p_out=32), geometry
bound, tables from the native builder installed with the deltas model's flags.  Then K cases on one handle: psm_solve_cases_delta
against psm_solve_cases.  Plain host arrays in every leg (the staging DMA-copy form both kinds share).

The legs alternate in one process, round by round; every call ends in a device synchronise and is timed on its own.  Per leg: the
median and the p10 .. p90 range over all calls, and the difference of the medians next to both ranges.

    python tools/delta_step.py [--parent-lib PATH] [--cases 4,8] [--steps 500] [--rounds 6] [--out FILE]
    python tools/delta_step.py --trace-leg delta|absolute|cases_delta|cases_absolute --steps N    one leg alone, for a kernel trace
    python tools/delta_step.py --launches SMALL.csv LARGE.csv N_SMALL N_LARGE    launches per step from two traces' kernel stats
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from psm_amd import GridSurrogate, SolverEnsemble, _lib, synthetic  # noqa: E402

MAXS = (0.01, 0.01, 0.35, 0.5)
OBSTACLES = (dict(), dict(cx=0.55, cy=0.05, R=0.06), dict(cx=0.9, cy=-0.08, R=0.1), dict(cx=0.3, cy=0.1, R=0.05))
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def other_build(path):
    """Another build of the library beside the one _lib loads: its own symbols first (RTLD_DEEPBIND), nothing exported to the
    process, the prototypes of _lib.SIGNATURES for what it exports."""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def single_handle(model, tables, n_cells, lib=None):
    """A handle on the single mesh with the deltas model's flags (normalise_sdf = fill_input = 1), on `lib` or the loaded build."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    keep, _lib._lib = _lib._lib, lib or _lib.load()         # GridSurrogate binds whatever _lib.load() returns
    try:
        sur = GridSurrogate(model, ny, nx, 1)
    finally:
        _lib._lib = keep
    mx = np.asarray(MAXS, np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, n_cells, ny, nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                  sdf.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    if rc:
        raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
    return sur


def native_tables(array, top, obst, delta=5e-3):
    lib = _lib.load()
    a, t, o = (np.ascontiguousarray(x, np.float64) for x in (array, top, obst))
    ny, nx = C.c_int32(), C.c_int32()
    if lib.psm_geometry_shape(a.ctypes.data_as(_dp), len(a), delta, C.byref(ny), C.byref(nx), None):
        raise RuntimeError(lib.psm_geometry_last_error().decode())
    ng, n = ny.value * nx.value, len(a)
    v1, w1, idx, sdf = np.empty((ng, 3), np.int32), np.empty((ng, 3)), np.empty((ng, 2), np.int32), np.empty(ng)
    v2, w2 = np.empty((n, 3), np.int32), np.empty((n, 3))
    if lib.psm_geometry_build(a.ctypes.data_as(_dp), n, t.ctypes.data_as(_dp), len(t), o.ctypes.data_as(_dp), len(o), delta, 10,
                              v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip), sdf.ctypes.data_as(_dp),
                              v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp)):
        raise RuntimeError(lib.psm_geometry_last_error().decode())
    return ny.value, nx.value, v1, w1, idx, sdf, v2, w2


def caller(sur, entry, arrays, single):
    """-> f(i): one synchronous call of `entry` on arrays[i % len(arrays)]; the output array is the leg's own."""
    fn = getattr(sur.lib, entry)
    out = np.empty(len(arrays[0]))
    ptrs = [a.ctypes.data_as(_dp) for a in arrays]
    po, n, h = out.ctypes.data_as(_dp), len(arrays[0]), sur.h

    def call(i):
        rc = fn(h, ptrs[i % len(ptrs)], n, 0, po) if single else fn(h, ptrs[i % len(ptrs)], po)
        if rc:
            raise RuntimeError(f"{entry}: {sur.lib.psm_last_error(h).decode()}")
    call.out = out
    return call


def alternate(legs, steps, rounds, warmup):
    """legs {name: call} -> {name: per-call microseconds}, the legs taking turns round by round."""
    for call in legs.values():
        for i in range(warmup):
            call(i)
    samples = {name: [] for name in legs}
    for _ in range(rounds):
        for name, call in legs.items():
            for i in range(steps):
                t0 = time.perf_counter()
                call(i)
                samples[name].append((time.perf_counter() - t0) * 1e6)
    return samples


def quantiles(us):
    p10, med, p90 = np.percentile(us, [10, 50, 90])
    return {"median_us": round(float(med), 2), "p10_us": round(float(p10), 2), "p90_us": round(float(p90), 2), "calls": len(us)}


def report(title, samples, base, lines, records, extra):
    q = {name: quantiles(us) for name, us in samples.items()}
    lines.append(title)
    for name, r in q.items():
        lines.append(f"  {name:28s} {r['median_us']:8.2f} us per call (p10 .. p90: {r['p10_us']:.2f} .. {r['p90_us']:.2f}; {r['calls']} calls)")
    for name, r in q.items():
        if name != base:
            d = r["median_us"] - q[base]["median_us"]
            spread = max(r["p90_us"] - r["p10_us"], q[base]["p90_us"] - q[base]["p10_us"])
            lines.append(f"  {name} - {base} = {d:+.2f} us (the larger p10 .. p90 range of the two legs: {spread:.2f} us)")
    records.append(dict(extra, legs=q))


def trace_leg(args, model):
    """One leg alone, N calls and nothing else around them but the set-up: the subject of a kernel trace."""
    K = 4 if args.trace_leg.startswith("cases") else 1
    if K == 1:
        a0, top, obst = synthetic.channel_mesh()
        arrays = [np.ascontiguousarray(synthetic.channel_mesh(step=k)[0]) for k in (3, 5)]
        sur = single_handle(model, native_tables(a0, top, obst), len(a0))
        call = caller(sur, "psm_solve_delta" if args.trace_leg == "delta" else "psm_solve", arrays, True)
    else:
        se, arrays = ensemble(model, K)
        sur = se._sur
        call = caller(sur, "psm_solve_cases_delta" if args.trace_leg == "cases_delta" else "psm_solve_cases", arrays, False)
    for i in range(args.steps):
        call(i)
    print(f"{args.trace_leg}: {args.steps} calls")
    sur.close()


def ensemble(model, K):
    meshes = [synthetic.channel_mesh(**OBSTACLES[k % len(OBSTACLES)]) for k in range(K)]
    se = SolverEnsemble(model, MAXS, K, geometry="native", step="delta")
    se.init_func([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes])      # primes with the start fields
    arrays = [np.ascontiguousarray(np.concatenate([synthetic.channel_mesh(**dict(OBSTACLES[k % len(OBSTACLES)], step=s))[0] for k in range(K)]))
              for s in (3, 5)]
    return se, arrays


def launches(small, large, n_small, n_large):
    def calls(path):
        with open(path) as f:
            return sum(int(row["Calls"]) for row in csv.DictReader(f))
    print(f"{(calls(large) - calls(small)) / (int(n_large) - int(n_small)):.2f} kernel launches per step "
          f"({calls(small)} in {n_small} steps, {calls(large)} in {n_large} steps; set-up launches cancel)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--cases", default="4,8")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--trace-leg", default=None, choices=("delta", "absolute", "cases_delta", "cases_absolute"))
    ap.add_argument("--launches", nargs=4, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.launches:
        return launches(*args.launches)
    model = synthetic.make_model("deltas", p_in=32, p_out=32)
    if args.trace_leg:
        return trace_leg(args, model)
    lines, records = [], []
    # ---- the single mesh
    a0, top, obst = synthetic.channel_mesh()
    arrays = [np.ascontiguousarray(synthetic.channel_mesh(step=k)[0]) for k in (3, 5)]
    tables = native_tables(a0, top, obst)
    sur = single_handle(model, tables, len(a0))
    assert sur.lib.psm_delta_prime(sur.h, np.ascontiguousarray(a0).ctypes.data_as(_dp), len(a0)) == 0
    legs = {"psm_solve_delta": caller(sur, "psm_solve_delta", arrays, True), "psm_solve": caller(sur, "psm_solve", arrays, True)}
    old = None
    if args.parent_lib:
        old = single_handle(model, tables, len(a0), other_build(args.parent_lib))
        legs["psm_solve (parent build)"] = caller(old, "psm_solve", arrays, True)
    samples = alternate(legs, args.steps, args.rounds, args.warmup)
    if old is not None:                                      # the existing route computes what it computed: same call, same bits
        legs["psm_solve"](0); legs["psm_solve (parent build)"](0)
        assert np.array_equal(legs["psm_solve"].out, legs["psm_solve (parent build)"].out), "psm_solve differs from the parent build's"
        lines.append("psm_solve of this build and of the parent build: identical bits on the same cells")
    report(f"single mesh, {len(a0)} cells, {tables[0]} x {tables[1]} grid, bound = {bool(sur.geometry_bound)}, {args.rounds} rounds of {args.steps} calls per leg",
           samples, "psm_solve", lines, records, {"cases": 1, "cells": len(a0), "bound": bool(sur.geometry_bound)})
    sur.close()
    if old is not None:
        old.close()
    # ---- K cases on one handle
    for K in [int(v) for v in args.cases.split(",") if v]:
        se, arrays = ensemble(model, K)
        legs = {"psm_solve_cases_delta": caller(se._sur, "psm_solve_cases_delta", arrays, False),
                "psm_solve_cases": caller(se._sur, "psm_solve_cases", arrays, False)}
        samples = alternate(legs, args.steps, args.rounds, args.warmup)
        report(f"K = {K} cases on one handle, {len(arrays[0])} cells in all, bound = {bool(se._sur.geometry_bound)}", samples, "psm_solve_cases",
               lines, records, {"cases": K, "cells": len(arrays[0]), "bound": bool(se._sur.geometry_bound)})
        se._sur.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
