"""Solver boundary with K cases on one GPU, one host thread: the batched entry (ONE handle, psm_solve_cases: one launch chain
for all cases) against the yardstick it replaces (K handles, psm_solve_begin on all, then psm_solve_end on all: one chain
per case on its own stream).  Workload of tools/attic/mesh_ensemble_bench.py: the 16 k-cell channel mesh, tables from the
native builder, host buffers registered with the library in both forms.  The two forms are timed in alternating rounds in one
process; per form and K the median over the rounds and the spread (min .. max) are reported, per step and per solve.

    python tools/mesh_cases_step.py [--cases 1,4,8] [--steps 1000] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from psm_amd import SolverEnsemble, SolverModule  # noqa: E402

_dp = C.POINTER(C.c_double)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,8")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, top, obst, model, maxs = cases.build_mesh_case()
    lines, records = [], []
    for K in [int(v) for v in args.cases.split(",")]:
        arrays = [np.ascontiguousarray(cases.build_mesh_case(step=k)[0], np.float64) for k in range(K)]
        # yardstick: one handle per case, registered buffers, begin on all / end on all
        mods, outs = [], []
        for a in arrays:
            sm = SolverModule(model, maxs, geometry="native")
            sm.init_func(a, top, obst)
            o = np.empty(a.shape[0])
            sm.pin(a, o)
            mods.append(sm); outs.append(o)
        # batched: one handle, the cases' cells side by side in one registered buffer
        se = SolverEnsemble(model, maxs, K, geometry="native")
        se.init_func(arrays, [top] * K, [obst] * K)
        cells, p = np.ascontiguousarray(np.concatenate(arrays)), np.empty(se.cell_off[-1])
        sur = se._sur
        sur.host_register(cells); sur.host_register(p)

        def yardstick(n):
            for _ in range(n):
                for sm, a, o in zip(mods, arrays, outs):
                    sm.py_func_begin(a, out=o)
                for sm in mods:
                    sm.py_func_end()

        def batched(n):
            for _ in range(n):
                sur._chk(sur.lib.psm_solve_cases(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp)))

        yardstick(args.warmup); batched(args.warmup)
        for k in range(K):                                   # same pressures (bound path of K cases against single cases: float32 summation order)
            d = np.abs(p[se.cell_off[k]:se.cell_off[k + 1]] - outs[k]).max() / np.abs(outs[k]).max()
            assert d <= 2e-5, (k, d)
        t = {"yardstick": [], "batched": []}
        for _ in range(args.rounds):                         # alternating rounds; each ends in a device synchronise (the end call)
            for name, fn in (("yardstick", yardstick), ("batched", batched)):
                t0 = time.perf_counter()
                fn(args.steps)
                t[name].append((time.perf_counter() - t0) / args.steps * 1e6)
        rec = {"cases": K, "cells_per_case": int(arrays[0].shape[0]), "steps": args.steps, "rounds": args.rounds, "bound": bool(sur.geometry_bound)}
        for name in t:
            med = statistics.median(t[name])
            rec[name] = {"us_per_step": round(med, 2), "us_per_solve": round(med / K, 2), "min_us_per_step": round(min(t[name]), 2),
                         "max_us_per_step": round(max(t[name]), 2)}
        rec["batched_over_yardstick"] = round(rec["batched"]["us_per_step"] / rec["yardstick"]["us_per_step"], 3)
        records.append(rec)
        lines.append(f"K = {K} ({rec['cells_per_case']} cells per case, {args.rounds} rounds of {args.steps} steps, registered host buffers)")
        for name, what in (("yardstick", f"{K} handles, psm_solve_begin on all / psm_solve_end on all"), ("batched", "1 handle, psm_solve_cases")):
            r = rec[name]
            lines.append(f"  {name:9s} {r['us_per_step']:8.1f} us per step ({r['min_us_per_step']:.1f} .. {r['max_us_per_step']:.1f}) = "
                         f"{r['us_per_solve']:6.1f} us per solve   [{what}]")
        lines.append(f"  batched / yardstick = {rec['batched_over_yardstick']:.3f}")
        sur.host_unregister(cells); sur.host_unregister(p)
        sur.close()
        for sm in mods:
            sm.unpin()
            sm._sur.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
