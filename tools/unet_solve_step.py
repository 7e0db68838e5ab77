"""The convolutional path at the solver boundary, K cases on one GPU, one host thread: what a step of psm_unet_solve* costs, what of
it the three launches around the network cost, and the loop it replaces.  Workload: the 16 k-cell channel mesh (138 x 300 grid,
tables from the native builder, K time steps of it as the K cases) behind UNet-S (widths 16, 32, 64, 128, 256: canvas 144 x 304)
with seeded He-normal weights.  Per K and precision, in one process, in alternating rounds, every step timed on its own by a host
clock around work that ends in a device synchronise; the median over all steps and the 10th .. 90th percentile are reported:

  1  device   psm_unet_solve_device, the cells resident on the device
  2  network  psm_unet_forward_device alone on the same canvases; (1 - 2) is the cost of the three launches of the mesh ends
  3  host     psm_unet_solve from host buffers (pinned staging, one H2D and one D2H copy)
  4  today    the loop a user writes without the entry: NumPy mesh -> grid on the same tables, np.pad, UNetSurrogate.forward, crop,
              NumPy grid -> mesh

    python tools/unet_solve_step.py [--cases 1,4,8] [--precisions f32,bf16] [--steps 200] [--rounds 2] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hipmem  # noqa: E402
from psm_amd import UNetSolverEnsemble, synthetic  # noqa: E402
from psm_amd.unet import WIDTHS_S  # noqa: E402

MAXS = (1.0, 0.536133, 0.999023, 0.510742)
_dp = C.POINTER(C.c_double)


def he_weights(c_in, widths, c_out, seed=7):
    """Seeded He-normal kernels [k,k,c_in,c_out] and small biases in the order of include/psm_unet.h."""
    rng = np.random.default_rng(seed)
    L = len(widths)
    shapes = []
    for l in range(L):
        shapes += [(3, c_in if l == 0 else widths[l - 1], widths[l]), (3, widths[l], widths[l])]
    for l in range(L - 2, -1, -1):
        shapes += [(3, widths[l + 1] + widths[l], widths[l]), (3, widths[l], widths[l])]
    shapes.append((1, widths[0], c_out))
    return [((rng.standard_normal((k, k, ci, co)) * np.sqrt(2.0 / (k * k * ci))).astype(np.float32), (rng.standard_normal(co) * 0.05).astype(np.float32))
            for k, ci, co in shapes]


def numpy_to_grid(array, g):
    """python_module.py:267-297 on the tables g."""
    U = np.max(np.sqrt(np.square(array[:, 0]) + np.square(array[:, 1])))
    grid = np.zeros((g.ny, g.nx, 3))
    idx = tuple(g.indices.T)
    for c in (0, 1):
        grid[:, :, c][idx] = np.einsum("nj,nj->n", np.take(array[:, c] / U, g.vtx_m2g), g.wts_m2g) / MAXS[c]
    grid[:, :, 2] = g.sdfunct
    grid[np.isnan(grid)] = 0
    return grid.astype(np.float32), U


def numpy_to_mesh(field, array, g, near, U):
    """python_module.py:481-496 on the tables g (near: the near-wall cells, constant per geometry)."""
    p = np.einsum("nj,nj->n", np.take(field[tuple(g.indices.T)].astype(np.float64), g.vtx_g2m), g.wts_g2m)
    bad = np.any(g.wts_g2m < 0, axis=1) | near | np.isnan(p)
    return np.where(bad, array[:, 4], p * MAXS[3] * U ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1,4,8")
    ap.add_argument("--precisions", default="f32,bf16")
    ap.add_argument("--steps", type=int, default=200, help="timed steps per round and form")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sync = hipmem.hip().hipDeviceSynchronize
    W = he_weights(3, WIDTHS_S, 1)
    lines, records = [], []
    for precision in args.precisions.split(","):
        for K in [int(v) for v in args.cases.split(",")]:
            meshes = [synthetic.channel_mesh(step=k) for k in range(K)]
            arrays = [np.ascontiguousarray(m[0], np.float64) for m in meshes]
            se = UNetSolverEnsemble(W, MAXS, WIDTHS_S, precision=precision, geometry="native", max_cases=K)
            se.init_func(arrays, [m[1] for m in meshes], [m[2] for m in meshes])
            lib, h, net, off = se.lib, se.h, se.net, se.cell_off
            cells, p = np.ascontiguousarray(np.concatenate(arrays)), np.empty(off[-1])
            d_cells, d_p = hipmem.DeviceArray(cells), hipmem.DeviceArray(shape=(off[-1],), dtype=np.float64)
            near = []
            for g in se.tables:
                sd = np.einsum("nj,nj->n", np.take(g.sdfunct.reshape(-1), g.vtx_g2m), g.wts_g2m)
                near.append(~np.any(g.wts_g2m < 0, axis=1) & (sd < 0.05))
            pad = ((0, 0), (0, se.ny_c - se.ny), (0, se.nx_c - se.nx), (0, 0))
            p_today = np.empty(off[-1])

            def device():
                se._chk(lib.psm_unet_solve_device(h, d_cells.ptr, d_p.ptr, None))
                sync()

            def host():
                se._chk(lib.psm_unet_solve(h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp)))

            def today():
                made = [numpy_to_grid(a, g) for a, g in zip(arrays, se.tables)]
                field = net.forward(np.pad(np.stack([m[0] for m in made]), pad))[:, :se.ny, :se.nx, 0]
                for k, (a, g) in enumerate(zip(arrays, se.tables)):
                    p_today[off[k]:off[k + 1]] = numpy_to_mesh(field[k], a, g, near[k], made[k][1])

            host()
            d_canvas = hipmem.DeviceArray(se.read("canvas"))
            d_field = hipmem.DeviceArray(shape=(K, se.ny_c, se.nx_c), dtype=np.float32)

            def network():
                net.forward_device(d_canvas.ptr, K, d_field.ptr)
                sync()

            forms = (("device", device), ("network", network), ("host", host), ("today", today))
            for _, fn in forms:
                for _ in range(args.warmup):
                    fn()
            # the same pressures from every form (float32 image and field in both; the forward pass is the same handle's)
            scale = np.abs(p_today).max()
            assert np.abs(p - p_today).max() <= 2e-4 * scale and np.abs(d_p.numpy() - p).max() == 0.0
            t = {name: [] for name, _ in forms}
            for _ in range(args.rounds):
                for name, fn in forms:
                    for _ in range(args.steps):
                        t0 = time.perf_counter()
                        fn()
                        t[name].append((time.perf_counter() - t0) * 1e6)
            rec = {"precision": precision, "cases": K, "cells": off[-1], "grid": [se.ny, se.nx], "canvas": [se.ny_c, se.nx_c], "steps": len(t["host"])}
            for name in t:
                q = np.percentile(t[name], [50, 10, 90])
                rec[name] = {"median_us": round(float(q[0]), 1), "p10_us": round(float(q[1]), 1), "p90_us": round(float(q[2]), 1)}
            rec["mesh_ends_us"] = round(rec["device"]["median_us"] - rec["network"]["median_us"], 1)
            rec["host_over_today"] = round(rec["host"]["median_us"] / rec["today"]["median_us"], 3)
            records.append(rec)
            lines.append(f"{precision}, K = {K} ({off[-1]} cells, grid {se.ny} x {se.nx}, canvas {se.ny_c} x {se.nx_c}; medians of {rec['steps']} steps, p10 .. p90)")
            for i, (name, what) in enumerate((("device", "psm_unet_solve_device, cells resident"), ("network", "psm_unet_forward_device alone"),
                                              ("host", "psm_unet_solve, host buffers"), ("today", "NumPy ends around UNetSurrogate.forward"))):
                r = rec[name]
                lines.append(f"  {i + 1} {name:8s} {r['median_us']:9.1f} us per step ({r['p10_us']:.1f} .. {r['p90_us']:.1f})   [{what}]")
            lines.append(f"  1 - 2 = {rec['mesh_ends_us']:.1f} us for the three launches of the mesh ends;  3 / 4 = {rec['host_over_today']:.3f}")
            for d in (d_cells, d_p, d_canvas, d_field):
                d.free()
            se.close()
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in records) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
