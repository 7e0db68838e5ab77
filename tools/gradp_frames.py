"""What the device-side frame batch buys a metrics-only sweep of the U_to_gradP evaluator (the 320 x 300 evaluator grid of
cases.build_gradp_dataset_case -- 138 x 300 has no row 200, which the reference's cut hard-wires --, its 24-component two-channel
gradp model, the simulation's geometry bound), by the protocol of
tools/frame_errors.py: >= 200 untimed steps, then 200 event-separated samples of 50 steps for p50 / p10 / p90;
all legs in ONE process on one box, alternated rather than each run once, profiler off.  The dataset's frames are read once and
served from memory to every leg, so that no leg times the HDF5 reader.

  A    the per-frame loop of main_gradP as it was: EvaluationGradP.timeStep -- psm_mesh_to_grid and five planes back, the NumPy
       image, the solve, psm_set_integration (tables rebuilt and uploaded), psm_integrate_gradp, two NumPy error_metrics passes --
       on the library given with --parent-lib (the parent commit's build), else on this one.  A step is one frame.
  B    EvaluationGradP.timeSteps(..., fields=False) with max_frames = K: one psm_gradp_frames per K frames, 32 doubles per frame
       come back, psm_error_metrics_from_sums per row.  A step is one batch of K frames.
  d    psm_gradp_frames_device with d_raw, K frames, columns resident: the graph replay and the error launches behind it
After the legs: the statements read off the lines above.

    python tools/gradp_frames.py [--parent-lib PATH] [--frames 1,8] [--steps 2000] [--rounds 2] [--out FILE]
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
from psm_amd import _lib, formats                # noqa: E402
from psm_amd.surrogate import EvaluationGradP    # noqa: E402
from hipmem import DeviceArray                   # noqa: E402
import cases                                     # noqa: E402
import poststeps_step as ps                      # noqa: E402  (measure, second_library, surrogate_on, hip_api)

say = ps.say
NY, NX = 320, 300
KEYS = ("normVal", "biasNorm", "stdeNorm", "rmseNorm", "mean_err", "mean_sq_err")


def serve_frames_from_memory():
    """formats.read_dataset with a cache in front: every (path, sim, time) is read from the file once."""
    inner, cache = formats.read_dataset, {}

    def cached(path, sim, time):
        key = (path, int(sim), int(time))
        if key not in cache:
            cache[key] = inner(path, sim, time)
        return cache[key]
    formats.read_dataset = cached


def evaluator(c, lib=None, **kw):
    ev = EvaluationGradP(5e-3, 128, 96, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, artifact_dir=c["dir"], **kw)
    if lib is not None:                           # the handle lives in the second library; computeOnlyOnce finds the surrogate made
        ev._sur = ps.surrogate_on(lib, ev.artifacts, NY, NX, ev.max_frames, ev.device)
        ev._sur.check_bound = True
    assert ev.computeOnlyOnce(0) == 0 and (ev.grid_shape_y, ev.grid_shape_x) == (NY, NX)
    return ev


def frame_columns(ev, times):
    """The cell columns timeSteps sends for `times`, for the device leg."""
    cols = []
    for t in times:
        d = formats.read_dataset(ev.hdf5_path, 0, t)[0][0, 0, :ev.indice]
        U = np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))
        cols.append(np.concatenate([d[:, 0:1] / U, d[:, 1:2] / U, d[:, 6:7] * (ev.max_x - ev.min_x) / pow(U, 2.0),
                                    d[:, 7:8] * (ev.max_y - ev.min_y) / pow(U, 2.0), d[:, 2:3] / pow(U, 2.0)], axis=1).astype(np.float64))
    return np.stack(cols)


def run(n_frames, args, h, stream, parent, c):
    times = [i % 2 for i in range(n_frames)]
    old = evaluator(c, parent)
    new = evaluator(c, max_frames=n_frames)
    dev = evaluator(c, max_frames=n_frames)
    sur = dev._surrogate(NY, NX)
    dev._bind_frames(sur, False)
    d_cols = DeviceArray(frame_columns(dev, times))
    d_raw = DeviceArray(shape=(n_frames, 4, 8), dtype=np.float64)

    def leg_A(i):
        old.timeStep(0, i % 2)
        return dict(old.last_metrics)

    legs = {"A": leg_A, "B": lambda _: new.timeSteps(0, times, fields=False),
            "d": lambda _: sur.gradp_frames_device(d_cols.ptr, n_frames, 5, d_raw=d_raw.ptr, stream=stream.value)}
    # B gives what A gives: every metric of A's two blocks of every frame, relative to the frame's rmseNorm / 100 (normVal, stdeNorm: relative)
    b = new.timeSteps(0, times, fields=False)
    worst = 0.0
    for j, t in enumerate(times):
        a = leg_A(t)
        for blk in ("reference", "p"):
            ma, mb = a[blk], b[j][blk]
            for key in KEYS:
                scale = abs(ma[key]) if key in ("normVal", "stdeNorm") else ma["rmseNorm"] / 100 * (100 if key.endswith("Norm") else 1)
                worst = max(worst, abs(ma[key] - mb[key]) / scale)
    say(f"frames={n_frames} check B == A: worst difference of any metric {worst:.2e} of its scale, guard_trips={new._sur.guard_trips}, "
        f"bound={new._sur.geometry_bound}")
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = ps.measure(h, stream, step, args.steps if name == "d" else max(200, args.steps // 10))
            res_[name].append(r)
            say(f"frames={n_frames} round={rnd} leg={name:4s} mean_us={r[0]:9.2f} p50_us={r[1]:9.2f} p10_us={r[2]:9.2f} p90_us={r[3]:9.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    spread = {k: float(np.median([r[3] - r[2] for r in v])) for k, v in res_.items()}
    say(f"frames={n_frames} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + "  p10-p90 spread_us " +
        " ".join(f"{k}={v:.2f}" for k, v in spread.items()))
    lib_name = "the parent" if parent is not None else "THIS"
    per_a, per_b = med["A"], med["B"] / n_frames
    lim = max(spread["A"], spread["B"] / n_frames)
    say(f"frames={n_frames} statement (per frame, A on {lib_name} library against B): A {per_a:.2f} us, B {per_b:.2f} us, A - B = {per_a - per_b:.2f} us, "
        f"larger p10-p90 spread of the two legs {lim:.2f} us: {'faster' if per_a - per_b > lim else 'NOT faster beyond the spread'}")
    say(f"frames={n_frames} statement (the device entry): d {med['d']:.2f} us per batch, {med['d'] / n_frames:.2f} us per frame; B - d = "
        f"{med['B'] - med['d']:.2f} us per batch is the host side of timeSteps (scalars, columns, H2D, metrics)")
    for ev in (old, new, dev):
        ev._sur.close()
    d_cols.free(); d_raw.free()


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
    serve_frames_from_memory()
    say(f"# tools/gradp_frames.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    with tempfile.TemporaryDirectory() as d:
        c = cases.build_gradp_dataset_case(d)
        c["dir"] = d
        for n in (int(v) for v in args.frames.split(",")):
            run(n, args, h, stream, parent, c)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
