"""What the Poisson-model step of a case set costs: ONE psm_solve_cases_poisson call for K meshes (one handle, the chain run on K
cases between the case-batched mesh ends, one graph replay) against what an ensemble user had before -- K single-mesh handles
advanced in turn by psm_solve_poisson -- on ANOTHER build of the library when one is given (--parent-lib: the parent commit's),
else on this one.  K cases of the 16 021-cell channel mesh on its 138 x 300 grid (the same tables, every case with fields of its own:
the time steps k + 3, k + 5, k + 6 of case k) behind the four-channel model (p_in = 48, p_out = 40), weighting and filter on, tables
from the native builder, plain host arrays.

The legs alternate in one process, round by round; every call ends in a device synchronise and is timed on its own.  Per leg and K:
the median and the p10 .. p90 range over all calls, per step and per case.  Both legs are checked to agree on dp before anything is
timed: the same fallback cells, and max|dp_A - dp_B| <= 2e-4 * max|dp_B| per case (the tolerance of tests/test_poisson_cases.py).

    python tools/poisson_cases_step.py [--parent-lib PATH] [--cases 1,4,8] [--steps 300] [--rounds 6] [--out FILE]
    python tools/poisson_cases_step.py --trace-leg cases --steps N    the batched entry alone at K = 4, for a kernel trace
    python tools/poisson_cases_step.py --kernels STATS.csv            the three new launches' rows of a trace's kernel stats
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
from psm_amd import GridSurrogate, synthetic  # noqa: E402
from delta_step import alternate, native_tables, other_build, quantiles  # noqa: E402
from poisson_solve_step import K as K_FEAT, MAXS5, PHI, S_FIELD, S_WEIGHT, bound_handle, model4  # noqa: E402

NEW_KERNELS = ("psm_umax_partial_kernel(PsmPoissonCasesArgs)", "psm_interp_to_grid_kernel(PsmPoissonCasesArgs)", "psm_to_mesh_kernel(PsmPoissonCasesArgs)")
TOL = 2e-4
_dp = C.POINTER(C.c_double)


def case_handle(model, tables, n_cells, n_cases):
    """One handle on a case set of `n_cases` meshes with these tables, features, post-steps and the step bound."""
    ny, nx, v1, w1, idx, sdf, v2, w2 = tables
    sur = GridSurrogate(model, ny, nx, n_cases)
    ptrs = lambda a: (C.c_void_p * n_cases)(*[a.ctypes.data] * n_cases)
    mx = np.asarray(MAXS5[1:], np.float64)
    rc = sur.lib.psm_set_geometry_cases(sur.h, n_cases, (C.c_int64 * n_cases)(*[n_cells] * n_cases), ny, nx, ptrs(v1), ptrs(w1), ptrs(idx), ptrs(sdf),
                                        ptrs(v2), ptrs(w2), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    if rc:
        raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
    sur.bind_features(np.stack([sdf.reshape(ny, nx)] * n_cases), K_FEAT, MAXS5[:4])
    sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_poisson_solve_cases(PHI, MAXS5[4], True, True)
    return sur


def batched_leg(sur, frames):
    """-> f(i): one psm_solve_cases_poisson on the cases' frames i % len, concatenated once; the state rotates with the calls."""
    cells = [np.ascontiguousarray(np.concatenate([f[s] for f in frames])) for s in range(len(frames[0]))]
    out = np.empty(len(cells[0]))
    ptrs, po, h, fn = [c.ctypes.data_as(_dp) for c in cells], out.ctypes.data_as(_dp), sur.h, sur.lib.psm_solve_cases_poisson

    def call(i):
        if fn(h, ptrs[i % len(ptrs)], po):
            raise RuntimeError(sur.lib.psm_last_error(h).decode())
    call.out = out
    return call


def handles_leg(surs, frames):
    """-> f(i): psm_solve_poisson on every handle in turn, each call synchronous, as K solver modules are advanced."""
    n = len(frames[0][0])
    out = np.empty(len(surs) * n)
    po = [out[k * n:(k + 1) * n].ctypes.data_as(_dp) for k in range(len(surs))]
    ptrs = [[a.ctypes.data_as(_dp) for a in f] for f in frames]

    def call(i):
        for k, sur in enumerate(surs):
            if sur.lib.psm_solve_poisson(sur.h, ptrs[k][i % len(ptrs[k])], n, 0, po[k]):
                raise RuntimeError(sur.lib.psm_last_error(sur.h).decode())
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
    ap.add_argument("--cases", default="1,4,8")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-leg", default=None, choices=("cases",))
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernels:
        return kernels(args.kernels)
    model = model4()
    a0, top, obst = synthetic.channel_mesh()
    n = len(a0)
    tables = native_tables(a0, top, obst)
    frames_of = lambda k: [np.ascontiguousarray(synthetic.channel_mesh(step=k + s)[0]) for s in (3, 5, 6)]
    if args.trace_leg:
        frames = [frames_of(k) for k in range(4)]
        sur = case_handle(model, tables, n, 4)
        sur.poisson_solve_push_cases(np.concatenate([f[-2] for f in frames])); sur.poisson_solve_push_cases(np.concatenate([f[-1] for f in frames]))
        call = batched_leg(sur, frames)
        for i in range(args.steps):
            call(i)
        print(f"psm_solve_cases_poisson, K = 4: {args.steps} calls")
        return sur.close()
    parent = other_build(args.parent_lib) if args.parent_lib else None
    where = "the parent build" if args.parent_lib else "this build"
    lines, records = [], []
    for nc in [int(v) for v in args.cases.split(",")]:
        frames = [frames_of(k) for k in range(nc)]
        sur = case_handle(model, tables, n, nc)
        singles = [bound_handle(model, tables, n, parent) for _ in range(nc)]
        # the state both legs start from
        sur.poisson_solve_push_cases(np.concatenate([f[-2] for f in frames])); sur.poisson_solve_push_cases(np.concatenate([f[-1] for f in frames]))
        for s, f in zip(singles, frames):
            s.poisson_solve_push(f[-2]); s.poisson_solve_push(f[-1])
        a, b = batched_leg(sur, frames), handles_leg(singles, frames)
        # both legs make the same steps: the same frames in the same order, dp compared per case on the cells neither falls back on
        worst = 0.0
        for i in range(3):
            a(i); b(i)
            for k in range(nc):
                prev, pa, pb = frames[k][i][:, 4], a.out[k * n:(k + 1) * n], b.out[k * n:(k + 1) * n]
                moved = pa != prev
                assert np.array_equal(moved, pb != prev), "the legs fall back on different cells"
                worst = max(worst, float(np.abs((pa[moved] - prev[moved]) - (pb[moved] - prev[moved])).max() / np.abs(pb[moved] - prev[moved]).max()))
        assert worst <= TOL, worst
        samples = alternate({"batched": a, "handles": b}, args.steps, args.rounds, args.warmup)
        q = {name: quantiles(us) for name, us in samples.items()}
        lines.append(f"K = {nc} ({n} cells per case, 138 x 300 grid, weighting and filter on, {args.rounds} rounds of {args.steps} steps per leg; "
                     f"both legs on the same three steps: the same fallback cells, max|dp_A - dp_B| / max|dp_B| = {worst:.2e})")
        for name, what in (("batched", "A: 1 handle, psm_solve_cases_poisson"), ("handles", f"B: {nc} handles of {where}, psm_solve_poisson in turn")):
            r = q[name]
            lines.append(f"  {what:62s} {r['median_us']:8.2f} us per step (p10 .. p90: {r['p10_us']:.2f} .. {r['p90_us']:.2f}) = "
                         f"{r['median_us'] / nc:7.2f} us per case ({r['p10_us'] / nc:.2f} .. {r['p90_us'] / nc:.2f}; {r['calls']} calls)")
        lines.append(f"  A / B = {q['batched']['median_us'] / q['handles']['median_us']:.3f}")
        records.append({"cases": nc, "cells_per_case": n, "parent_lib": bool(args.parent_lib), "legs": q})
        sur.close()
        for s in singles:
            s.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
