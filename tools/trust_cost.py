"""What the input-trust score costs (psm_bind_trust / psm_trust_last, include/psm.h), in one process, alternating rounds:

* a step at the solver boundary alone against the step followed by psm_trust_last, on the 16 k-cell channel mesh (138 x 300) at
  K = 1, 4, 8 (psm_solve_cases, registered host buffers), and psm_solve_grid alone / followed by psm_trust_last on the 256 x 256 grid;
* the two per-call launches alone: `reps` calls of psm_trust_last_device back to back on a stream between one pair of HIP events;
* the loop a caller had to write without the entries: psm_mesh_to_grid, NumPy block extraction, x - mu - C^T (C (x - mu)) per block;
* the step with the binding held but never called against the same step on a handle without it (no launch sequence differs).

Per figure the median over the rounds and the spread (min .. max).

    python tools/trust_cost.py [--cases 1,4,8] [--steps 500] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, surrogate, synthetic  # noqa: E402

_dp = C.POINTER(C.c_double)


def timed(fns, steps, rounds, warmup=20):
    """{name: (median, min, max)} microseconds per call of every fn, alternating rounds; every fn ends synchronised."""
    for fn in fns.values():
        fn(warmup)
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn(steps)
            t[name].append((time.perf_counter() - t0) / steps * 1e6)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def show(r):
    return f"{r[0]:8.1f} us ({r[1]:.1f} .. {r[2]:.1f})"


def launches_alone(sur, n_rows, reps, rounds):
    """GPU time per psm_trust_last_device call: `reps` calls on one stream between two events."""
    hip = C.CDLL("libamdhip64.so")
    st, e0, e1, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    assert hip.hipMalloc(C.byref(d), C.c_size_t(n_rows * 16)) == 0
    out = []
    for r in range(rounds + 1):
        hip.hipEventRecord(e0, st)
        for _ in range(reps):
            sur.trust_last_device(d.value, st.value)
        hip.hipEventRecord(e1, st)
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        if r:
            out.append(ms.value * 1e3 / reps)
    hip.hipFree(d); hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipStreamDestroy(st)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,8")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, top, obst, model, maxs = cases.build_mesh_case()
    lines = []
    for K in [int(v) for v in args.cases.split(",")]:
        arrays = [np.ascontiguousarray(cases.build_mesh_case(step=k)[0], np.float64) for k in range(K)]
        ens = {}
        for name, trust in (("unbound", False), ("bound", True), ("control", False)):     # control: a second handle without the binding
            se = SolverEnsemble(model, maxs, K, geometry="native", trust=trust)
            se.init_func(arrays, [top] * K, [obst] * K)
            cells, p = np.ascontiguousarray(np.concatenate(arrays)), np.empty(se.cell_off[-1])
            se._sur.host_register(cells); se._sur.host_register(p)
            ens[name] = (se, cells, p)

        def step(name, score):
            se, cells, p = ens[name]
            sur = se._sur
            out, n = np.empty((K, sur.B, 2)), C.c_int32()

            def run(count):
                for _ in range(count):
                    sur._chk(sur.lib.psm_solve_cases(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp)))
                    if score:
                        sur._chk(sur.lib.psm_trust_last(sur.h, C.byref(n), out.ctypes.data_as(_dp), out.size))
            return run

        r = timed({"unbound": step("unbound", False), "bound": step("bound", False), "control": step("control", False),
                   "scored": step("bound", True)}, args.steps, args.rounds)
        sur = ens["bound"][0]._sur
        alone = launches_alone(sur, K * sur.B, 200, args.rounds)
        t = ens["bound"][0].trust()
        lines.append(f"mesh 138 x 300, K = {K} ({arrays[0].shape[0]} cells per case, B = {sur.B}, p_in = {model.p_in}, {args.rounds} rounds of {args.steps} steps)")
        lines.append(f"  psm_solve_cases, no trust binding         {show(r['unbound'])}")
        lines.append(f"  psm_solve_cases, trust bound, not called  {show(r['bound'])}   bound - unbound = {r['bound'][0] - r['unbound'][0]:+.1f} us")
        lines.append(f"  psm_solve_cases, a second unbound handle  {show(r['control'])}   control - unbound = {r['control'][0] - r['unbound'][0]:+.1f} us")
        lines.append(f"  psm_solve_cases + psm_trust_last          {show(r['scored'])}   psm_trust_last = {r['scored'][0] - r['bound'][0]:.1f} us")
        lines.append(f"  the two launches alone (events, 200 calls back to back)  {show(alone)}")
        lines.append(f"  explained_total of case 0: {t[0]['explained_total']:.6f}")
        if K == 1:                                            # the caller's loop without the entries: mesh -> grid on the library, the rest NumPy
            sm = SolverModule(model, maxs, geometry="native")
            sm.init_func(arrays[0], top, obst)
            s1 = sm._sur
            orig = [(int(b[0]), int(b[1])) for b in surrogate.layout(model.variant, s1.ny, s1.nx, model.S)[0]]
            Cm, mu, S = np.asarray(model.comp_in), np.asarray(model.mean_in), model.S
            a = arrays[0]
            grid = np.empty((s1.ny * s1.nx, 2))
            sdf = np.zeros((s1.ny, s1.nx))

            def host_loop(count):
                for _ in range(count):
                    U = np.max(np.sqrt(np.square(a[:, 0]) + np.square(a[:, 1])))
                    vals = np.ascontiguousarray(a[:, 0:2] / U / np.asarray(maxs[:2]))
                    s1._chk(s1.lib.psm_mesh_to_grid(s1.h, vals.ctypes.data_as(_dp), a.shape[0], 2, 0, grid.ctypes.data_as(_dp)))
                    img = np.concatenate([grid.reshape(s1.ny, s1.nx, 2), sdf[..., None]], axis=-1)
                    x = np.stack([img[y0:y0 + S, x0:x0 + S].reshape(-1) for y0, x0 in orig]) - mu
                    rho = x - (x @ Cm.T) @ Cm
                    (rho * rho).sum(axis=1), (x * x).sum(axis=1)
            h = timed({"host": host_loop}, max(args.steps // 25, 4), args.rounds, warmup=2)
            lines.append(f"  the caller's own loop (psm_mesh_to_grid + NumPy blocks + x - mu - C^T C (x - mu), float64)  {show(h['host'])}")
            s1.close()
        for se, cells, p in ens.values():
            se._sur.host_unregister(cells); se._sur.host_unregister(p)
            se._sur.close()
    # the headline grid
    m = synthetic.make_model("gradp", p_in=128, p_out=128)
    g = np.ascontiguousarray(synthetic.channel_grid(256, 256, seed=1), np.float32)[None]
    sur = {name: GridSurrogate(m, 256, 256) for name in (False, True, "control")}
    sur[True].bind_trust()
    for s in sur.values():
        assert s.bind_geometry(g[0])
        s.host_register(g)

    def solve(trust, score):
        s = sur[trust]
        def run(count):
            for _ in range(count):
                s.solve(g)
                if score:
                    s.trust_last()
        return run
    r = timed({"unbound": solve(False, False), "bound": solve(True, False), "control": solve("control", False), "scored": solve(True, True)},
              args.steps, args.rounds)
    alone = launches_alone(sur[True], sur[True].B, 200, args.rounds)
    lines.append(f"grid 256 x 256, gradp, p_in = 128, B = {sur[True].B}, geometry bound ({args.rounds} rounds of {args.steps} solves)")
    lines.append(f"  psm_solve_grid, no trust binding          {show(r['unbound'])}")
    lines.append(f"  psm_solve_grid, trust bound, not called   {show(r['bound'])}   bound - unbound = {r['bound'][0] - r['unbound'][0]:+.1f} us")
    lines.append(f"  psm_solve_grid, a second unbound handle   {show(r['control'])}   control - unbound = {r['control'][0] - r['unbound'][0]:+.1f} us")
    lines.append(f"  psm_solve_grid + trust_last               {show(r['scored'])}   trust_last = {r['scored'][0] - r['bound'][0]:.1f} us")
    lines.append(f"  the two launches alone (events, 200 calls back to back)  {show(alone)}")
    t0 = time.perf_counter()
    sur[True].bind_trust()
    lines.append(f"  psm_bind_trust (25 MB basis to float32, upload, Gram matrix): {(time.perf_counter() - t0) * 1e3:.1f} ms")
    for s in sur.values():
        s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
