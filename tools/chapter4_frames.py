"""Microseconds per frame of the Chapter-4 evaluators' frame batch (138 x 300 evaluator grid of tests/chapter4_case.py, its
24-component chapter5-variant models for both `inputs`, the simulation's geometry bound), by the protocol of tools/frame_errors.py
(DESIGN section 5): >= 200 untimed steps, then 200 event-separated samples of 50 steps for p50 / p10 / p90; all legs in ONE process
on one box, alternated rather than each run once, profiler off.  The dataset's frames are read once and served from memory to every
leg, so that no leg times the HDF5 reader.  There is no earlier Chapter-4 evaluator to compare with, so the comparison leg is the
loop a user had to write:

  A    one frame per step with entries that existed before the frame batch: the float32 frame preparation, psm_mesh_to_grid and the
       c_in planes back, the NumPy image, GridSurrogate.solve, the NumPy error_metrics pass.
  F    EvaluationChapter4.timeSteps(..., fields=True) with max_frames = K: one psm_chapter4_frames per K frames, field and truth
       come back, error_metrics on the host.  A step is one batch of K frames.
  S    EvaluationChapter4.timeSteps(..., fields=False): 8 doubles per frame come back, psm_error_metrics_from_sums per row.
After the legs: the statements read off the lines above.

    python tools/chapter4_frames.py [--inputs M_u,M_fU] [--frames 1,8] [--steps 2000] [--rounds 2] [--out FILE]
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
import psm_amd                                                     # noqa: E402
from psm_amd import EvaluationChapter4, _lib, error_metrics       # noqa: E402
import chapter4_case as c4                                         # noqa: E402
import poststeps_step as ps                                        # noqa: E402  (measure, hip_api)
from deltas_frames import serve_frames_from_memory                 # noqa: E402

say = ps.say
_f64, _p = psm_amd.surrogate._f64, psm_amd.surrogate._p
KEYS = ("normVal", "biasNorm", "stdeNorm", "rmseNorm", "mean_err", "mean_sq_err")


def evaluator(c, **kw):
    ev = EvaluationChapter4(c4.DELTA, c4.SHAPE, c4.AVANCE, 0.95, 0.95, c["dataset_path"], c["model_path"], inputs=c["inputs"],
                            artifact_dir=c["dir"], **kw)
    assert ev.computeOnlyOnce(0) == 0 and (ev.grid_shape_y, ev.grid_shape_x) == (138, 300)
    return ev


def users_loop(ev):
    """Leg A: one frame with the host entries, spelled out (what EvaluationChapter4.timeStep does, without the class)."""
    sur, c, mx = ev._sur, ev.c_in_expected, ev._max_abs()
    ny, nx, sdf = ev.grid_shape_y, ev.grid_shape_x, ev.sdfunct[..., 0]

    def step(i):
        d = psm_amd.formats.read_dataset(ev.hdf5_path, 0, i % c4.FRAMES)[0][0, 0, :ev.indice]
        U = np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))
        if c == 3:
            cols = np.concatenate([d[:, 0:1] / U, d[:, 1:2] / U, d[:, 2:3] / pow(U, 2.0)], axis=1)
        else:
            cols = np.concatenate([d[:, 5:6] / pow(U, 2.0), d[:, 2:3] / pow(U, 2.0)], axis=1)
        v = _f64(cols)
        g = np.empty((ny, nx, c), np.float64)
        sur._chk(sur.lib.psm_mesh_to_grid(sur.h, _p(v, C.c_double), v.shape[0], c, 1, _p(g, C.c_double)))
        grid = np.zeros((ny, nx, c + 1))
        grid[..., :c - 1] = g[..., :c - 1]
        grid[..., c - 1] = sdf
        grid[..., c] = g[..., c - 1]
        grid[np.isnan(grid)] = 0
        for ch in range(c + 1):
            grid[..., ch] /= mx[ch]
        res = sur.solve(grid[..., :c])[0, :, :, 0]
        return error_metrics(res, grid[..., c], grid[..., c - 1] == 0)
    return step


def run(n_frames, args, h, stream, c):
    times = [i % c4.FRAMES for i in range(n_frames)]
    old = evaluator(c)
    new = evaluator(c, max_frames=n_frames)
    leg_A = users_loop(old)
    legs = {"A": leg_A, "F": lambda _: new.timeSteps(0, times, fields=True), "S": lambda _: new.timeSteps(0, times, fields=False)}
    # S gives what A gives: every metric of every frame, relative to the frame's rmseNorm / 100 (normVal, stdeNorm: relative)
    b = new.timeSteps(0, times, fields=False)
    worst = 0.0
    for j, t in enumerate(times):
        ma, mb = leg_A(t), b[j]["p"]
        for key in KEYS:
            scale = abs(ma[key]) if key in ("normVal", "stdeNorm") else ma["rmseNorm"] / 100 * (100 if key.endswith("Norm") else 1)
            worst = max(worst, abs(ma[key] - mb[key]) / scale)
    tag = f"inputs={c['inputs']} frames={n_frames}"
    say(f"{tag} check S == A: worst difference of any metric {worst:.2e} of its scale, guard_trips={new._sur.guard_trips}, bound={new._sur.geometry_bound}")
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = ps.measure(h, stream, step, max(200, args.steps // 10))
            res_[name].append(r)
            say(f"{tag} round={rnd} leg={name:4s} mean_us={r[0]:9.2f} p50_us={r[1]:9.2f} p10_us={r[2]:9.2f} p90_us={r[3]:9.2f}")
            new.pred_minus_true, new.pred_minus_true_squared = [], []       # the lists grow by one entry per frame
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    spread = {k: float(np.median([r[3] - r[2] for r in v])) for k, v in res_.items()}
    say(f"{tag} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + "  p10-p90 spread_us " +
        " ".join(f"{k}={v:.2f}" for k, v in spread.items()))
    for name, what in (("F", "fields=True"), ("S", "fields=False")):
        per, lim = med[name] / n_frames, max(spread["A"], spread[name] / n_frames)
        say(f"{tag} statement (per frame, the user's loop A against timeSteps {what}): A {med['A']:.2f} us, {name} {per:.2f} us, A - {name} = "
            f"{med['A'] - per:.2f} us, larger p10-p90 spread of the two legs {lim:.2f} us: {'faster' if med['A'] - per > lim else 'NOT faster beyond the spread'}")
    for ev in (old, new):
        ev._sur.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="M_u,M_fU")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    h = ps.hip_api()
    _lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    serve_frames_from_memory()
    say(f"# tools/chapter4_frames.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
    for inputs in args.inputs.split(","):
        with tempfile.TemporaryDirectory() as d:
            c = c4.build_chapter4_dataset_case(d, inputs)
            c.update(dir=d, inputs=inputs)
            for n in (int(v) for v in args.frames.split(",")):
                run(n, args, h, stream, c)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
