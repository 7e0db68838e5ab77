"""What the frame-batched mesh -> grid stage buys the pressureSM_Poisson evaluator (138 x 300 evaluator grid of the dataset fixture,
its 24-component four-channel deltas model, geometry bound for the batch), by the protocol of tools/poststeps_step.py (DESIGN
section 5): >= 200 untimed steps, then 200 event-separated samples of 50 steps for p50 / p10 / p90; all legs in ONE process on one
box, alternated rather than each run once, profiler off.  A step is one batch of K frames.

  i    the host chain EvaluationPoisson.timeStep runs, per frame: psm_mesh_to_grid (8 columns), NumPy slices, psm_poisson_features,
       psm_solve_poststeps -- on the library given with --parent-lib (the parent commit's build), else on this one
  ii   psm_mesh_to_grid per frame, then ONE psm_poisson_step for the batch -- same library as i
  iiih psm_poisson_frames: host columns in, host fields and label planes out, one call for the batch
  iiid psm_poisson_frames_device: columns and fields resident, one graph replay
  iv   psm_poisson_step_device alone on resident planes, on this library; iv0: the same on the --parent-lib library
  g    psm_frames_to_grid_device alone, the evaluator's eight destinations: back-to-back launches, so the p50 is the launch's
       dispatch-to-dispatch time
After the legs: the statements read off the lines above.

    python tools/poisson_frames.py [--parent-lib PATH] [--frames 1,8] [--steps 2000] [--rounds 2] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # as bench.py: the host program's choice, read once by the runtime

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import psm_amd                                   # noqa: E402
from psm_amd import _lib, geometry               # noqa: E402
from hipmem import DeviceArray                   # noqa: E402
import cases                                     # noqa: E402
import poststeps_step as ps                      # noqa: E402  (measure, second_library, surrogate_on, hip_api)

K_ARCSINH, PHI = 0.5, 0.16
say = ps.say
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


def workload(n_frames):
    """Tables of the dataset fixture's simulation and n_frames frames of the evaluator's eight columns (the three frames of the
    file, cycled with another velocity scale per round)."""
    with tempfile.TemporaryDirectory() as d:
        c = cases.build_dataset_case(d, poisson=True)
    n = c["N"]
    cells = np.asarray(c["sim"][0, 0, :n], np.float64)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    t = geometry.build_geometry_evaluator(cells[:, 3:5], cells[:, 2], f32(c["top"]), f32(c["obst"]), 5e-3, idw_fallback=True)
    cols, Us = [], []
    for i in range(n_frames):
        d = c["sim"][0, i % 3, :n] * np.float32(1.0 + 0.1 * (i // 3))
        dU, dUp = d[:, 5:7], d[:, 8:10]
        changed = np.abs(dU - dUp).sum(axis=-1)
        cols.append(np.concatenate([d[:, 0:2], dU, d[:, 7:8], d[:, 2:3], (changed / changed.max())[:, None], d[:, 10:11]], axis=1))
        Us.append(float(np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))))
    return c["model"], t, n, np.ascontiguousarray(np.stack(cols), np.float64), Us


def prepare(sur, t, n_cells, n_frames, frames):
    """Mesh, bindings and the batch's bound geometry on one handle (frames: this tree's library only)."""
    sur.set_mesh(t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct, n_cells)
    sur.bind_features(np.repeat(np.asarray(t.sdfunct, np.float64)[None], n_frames, axis=0), K_ARCSINH, cases.POISSON_MAXS[:4])
    sur.bind_poststeps((10, 10), (50, 50))
    if frames:
        sur.bind_frames(n_frames, 8)
    g = np.zeros((n_frames, t.ny, t.nx, 4), np.float32)
    g[..., 3] = (np.nan_to_num(t.sdfunct) / cases.POISSON_MAXS[3]).astype(np.float32)[None]
    assert sur.bind_geometry(g)


def mesh_to_grid(sur, v, out):
    sur._chk(sur.lib.psm_mesh_to_grid(sur.h, v.ctypes.data_as(_dp), v.shape[0], v.shape[1], 1, out.ctypes.data_as(_dp)))


def run(n_frames, args, h, stream, parent):
    model, t, n_cells, cols, Us = workload(n_frames)
    ny, nx = t.ny, t.nx
    lu = np.array([[PHI, U] for U in Us])
    sc = [cases.POISSON_MAXS[4] * U ** 2 for U in Us]
    sur = psm_amd.GridSurrogate(model, ny, nx, max_cases=n_frames)
    prepare(sur, t, n_cells, n_frames, True)
    old = sur
    if parent is not None:
        old = ps.surrogate_on(parent, model, ny, nx, max_cases=n_frames)
        prepare(old, t, n_cells, n_frames, False)
    sdf = np.ascontiguousarray(t.sdfunct, np.float64)
    g = np.empty((ny, nx, 8))
    planes = np.empty((n_frames, 8, ny, nx))
    for i in range(n_frames):
        mesh_to_grid(old, cols[i], g)
        planes[i] = np.moveaxis(g, 2, 0)
    d_cols, d_vel = DeviceArray(cols), DeviceArray(np.ascontiguousarray(planes[:, :4]))
    d_u, d_p = (DeviceArray(np.ascontiguousarray(planes[:, q], np.float32)) for q in (6, 7))
    d_x = DeviceArray(shape=(n_frames, 2, ny, nx), dtype=np.float64)
    d_r, d_c, d_n = (DeviceArray(shape=(n_frames, ny, nx)) for _ in range(3))
    npix = ny * nx

    def leg_i(_):
        for i in range(n_frames):
            mesh_to_grid(old, cols[i], g)
            img = old.poisson_features(g[..., 0], g[..., 1], g[..., 2], g[..., 3], sdf, PHI, Us[i], K_ARCSINH, cases.POISSON_MAXS[:4])
            old.solve_poststeps(img, False, g[..., 6], g[..., 7], out_scale=[sc[i]])

    def leg_ii(_):
        for i in range(n_frames):
            mesh_to_grid(old, cols[i], g)
            planes[i] = np.moveaxis(g, 2, 0)
        old.poisson_step(planes[:, :4], lu, out_scale=sc, dU=planes[:, 6], prev=planes[:, 7])

    step_dev = lambda s_: s_.poisson_step_device(d_vel.ptr, n_frames, lu, d_r.ptr, False, d_u.ptr, d_p.ptr, d_c.ptr, d_n.ptr, stream=stream.value,
                                                  out_scale=sc)
    outs = [(d_vel.ptr + q * npix * 8, 4 * npix, 0) for q in range(4)]
    outs += [(d_x.ptr + q * npix * 8, 2 * npix, 0) for q in range(2)] + [(d_u.ptr, npix, 1), (d_p.ptr, npix, 1)]
    legs = {"i": leg_i, "ii": leg_ii,
            "iiih": lambda _: sur.poisson_frames(cols, lu, out_scale=sc),
            "iiid": lambda _: sur.poisson_frames_device(d_cols.ptr, n_frames, 8, lu, d_r.ptr, False, True, d_x.ptr, d_c.ptr, d_n.ptr,
                                                        stream=stream.value, out_scale=sc),
            "iv": lambda _: step_dev(sur),
            "g": lambda _: sur.frames_to_grid_device(d_cols.ptr, n_frames, 8, outs, stream=stream.value)}
    if parent is not None:
        legs["iv0"] = lambda _: step_dev(old)
    # iiid gives what iv gives on the planes of psm_mesh_to_grid, bit for bit
    step_dev(sur)
    sur.synchronize()
    want = [d.numpy() for d in (d_r, d_c, d_n)]
    legs["iiid"](0)
    sur.synchronize()
    same = all(np.array_equal(d.numpy().view(np.uint32), w.view(np.uint32)) for d, w in zip((d_r, d_c, d_n), want))
    say(f"frames={n_frames} check iiid == psm_mesh_to_grid -> iv: {same} guard_trips={sur.guard_trips}")
    slow = ("i", "ii", "iiih")
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = ps.measure(h, stream, step, max(200, args.steps // 10) if name in slow else args.steps)
            res_[name].append(r)
            say(f"frames={n_frames} round={rnd} leg={name:4s} mean_us={r[0]:9.2f} p50_us={r[1]:9.2f} p10_us={r[2]:9.2f} p90_us={r[3]:9.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    spread = {k: float(np.median([r[3] - r[2] for r in v])) for k, v in res_.items()}
    say(f"frames={n_frames} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + "  p10-p90 spread_us " +
        " ".join(f"{k}={v:.2f}" for k, v in spread.items()))
    lib_name = "the parent" if parent is not None else "THIS"
    for new in ("iiih", "iiid"):
        for ref in ("i", "ii"):
            gain, worst = med[ref] - med[new], max(spread[ref], spread[new])
            say(f"frames={n_frames} statement ({ref} on {lib_name} library against {new}): {ref} - {new} = {gain:.2f} us, larger p10-p90 spread of the "
                f"two legs {worst:.2f} us: {'faster' if gain > worst else 'NOT faster beyond the spread'}")
    say(f"frames={n_frames} statement (the stage's share): iiid - iv = {med['iiid'] - med['iv']:.2f} us; the launch alone, back to back: "
        f"p50 {med['g']:.2f} us (p10-p90 spread {spread['g']:.2f} us)")
    if "iv0" in med:
        moved, lim = abs(med["iv"] - med["iv0"]), max(spread["iv"], spread["iv0"])
        say(f"frames={n_frames} statement (the step itself did not move): |iv - iv0| = {moved:.2f} us, larger p10-p90 spread of the two legs "
            f"{lim:.2f} us: {'holds' if moved <= lim else 'DOES NOT HOLD'}")
    sur.close()
    if old is not sur:
        old.close()
    for d in (d_cols, d_vel, d_u, d_p, d_x, d_r, d_c, d_n):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    h = ps.hip_api()
    _lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    parent = ps.second_library(args.parent_lib) if args.parent_lib else None
    say(f"# tools/poisson_frames.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for n in (int(c) for c in args.frames.split(",")):
        run(n, args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
