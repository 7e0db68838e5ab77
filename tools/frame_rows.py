"""What device-side frame preparation (timeSteps(device_prep=True): the dataset rows go up as float32, the device derives the
per-frame scalars and the columns) buys a metrics-only sweep of the three dataset evaluators, by the protocol of
tools/frame_errors.py: >= 200 untimed steps, then 200 event-separated samples of 50 steps for p50 / p10 / p90;
all legs in ONE process on one box, alternated rather than each run once, profiler off.  The dataset's frames are read once and
served from memory to every leg, so that no leg times the HDF5 reader.  Evaluators: the 138 x 300 deltas and Poisson grids of
cases.build_dataset_case (16 021 cells, 11 columns), the 320 x 300 gradP grid of cases.build_gradp_dataset_case (8 columns), each
with the simulation's geometry bound as the evaluator binds it.

  P    timeSteps(sim, K frames, fields=False) on the library given with --parent-lib (the parent commit's build): the host prepares
       scalars and float64 columns.  A step is one call of K frames.  Without --parent-lib the leg is left out.
  A    the same call on this library, device_prep=False
  B    the same call on this library, device_prep=True
  r    psm_rows_prepare_device alone, K frames resident on the device: the two launches
After the legs: the statements read off the lines above (per frame; B against P, and against A).

    python tools/frame_rows.py [--parent-lib PATH] [--frames 1,8] [--steps 2000] [--rounds 2] [--only deltas,poisson,gradp] [--out FILE]
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
import psm_amd                                   # noqa: E402,F401
from psm_amd import Evaluation, EvaluationPoisson, _lib, formats    # noqa: E402
from psm_amd.surrogate import EvaluationGradP    # noqa: E402
from hipmem import DeviceArray                   # noqa: E402
import cases                                     # noqa: E402
import poststeps_step as ps                      # noqa: E402  (measure, second_library, surrogate_on, hip_api)
from gradp_frames import serve_frames_from_memory    # noqa: E402

say = ps.say
K_ARCSINH, PHI = 0.5, 0.16
SHAPES = {"deltas": (138, 300), "poisson": (138, 300), "gradp": (320, 300)}
N_TIMES = {"deltas": 3, "poisson": 3, "gradp": 2}


def evaluator(kind, c, lib=None, **kw):
    if kind == "deltas":
        ev = Evaluation(5e-3, 128, 32, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, "std", artifact_dir=c["dir"], **kw)
    elif kind == "poisson":
        ev = EvaluationPoisson(5e-3, 128, 32, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, "std", K_ARCSINH, None, artifact_dir=c["dir"], **kw)
    else:
        ev = EvaluationGradP(5e-3, 128, 96, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, artifact_dir=c["dir"], **kw)
    if lib is not None:                           # the handle lives in the second library; computeOnlyOnce finds the surrogate made
        ev._sur = ps.surrogate_on(lib, ev.artifacts, *SHAPES[kind], ev.max_frames, ev.device)
        ev._sur.check_bound = True
    assert ev.computeOnlyOnce(0) == 0 and (ev.grid_shape_y, ev.grid_shape_x) == SHAPES[kind]
    return ev


def sweep(kind, ev, times, device_prep=None):
    kw = {} if device_prep is None else {"device_prep": device_prep}       # the parent's timeSteps has no such keyword
    if kind == "poisson":
        return ev.timeSteps(0, times, False, PHI, fields=False, **kw)
    return ev.timeSteps(0, times, fields=False, **kw)


def flat(m):
    """Every number of one frame's metrics, in a fixed order."""
    if isinstance(m, dict):
        return [x for k in sorted(m) for x in flat(m[k])]
    return [float(m)]


def run(kind, n_frames, args, h, stream, parent, c):
    times = [i % N_TIMES[kind] for i in range(n_frames)]
    old = evaluator(kind, c, parent, max_frames=n_frames) if parent is not None else None
    new = evaluator(kind, c, max_frames=n_frames)
    a = sweep(kind, new, times, False)
    trips_a = new._sur.guard_trips
    b = sweep(kind, new, times, True)
    same = all(np.array_equal(np.array(flat(x)), np.array(flat(y)), equal_nan=True) for x, y in zip(a, b))
    say(f"{kind} frames={n_frames} check B == A: every metric of every frame equal = {same}, guard_trips after A / after B = {trips_a} / {new._sur.guard_trips}, "
        f"bound={new._sur.geometry_bound}")
    sur = new._sur
    rows = np.stack([formats.read_dataset(new.hdf5_path if kind == "gradp" else new.dataset_path, 0, t)[0][0, 0, :new.indice] for t in times])
    d_rows = DeviceArray(np.ascontiguousarray(rows, np.float32))
    ex, ey = (float(new.max_x - new.min_x), float(new.max_y - new.min_y)) if kind == "gradp" else (1.0, 1.0)
    legs = {}
    if old is not None:
        legs["P"] = lambda _: sweep(kind, old, times)
    legs["A"] = lambda _: sweep(kind, new, times, False)
    legs["B"] = lambda _: sweep(kind, new, times, True)
    legs["r"] = lambda _: sur.rows_prepare_device(kind, d_rows.ptr, n_frames, rows.shape[1], rows.shape[2], base=0.047, ex=ex, ey=ey, stream=stream.value)
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = ps.measure(h, stream, step, args.steps if name == "r" else max(200, args.steps // 10))
            res_[name].append(r)
            say(f"{kind} frames={n_frames} round={rnd} leg={name:4s} mean_us={r[0]:9.2f} p50_us={r[1]:9.2f} p10_us={r[2]:9.2f} p90_us={r[3]:9.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    spread = {k: float(np.median([r[3] - r[2] for r in v])) for k, v in res_.items()}
    say(f"{kind} frames={n_frames} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + "  p10-p90 spread_us " +
        " ".join(f"{k}={v:.2f}" for k, v in spread.items()))
    for ref, what in (("P", "the parent library"), ("A", "this library, device_prep off")):
        if ref not in med:
            continue
        per_ref, per_b = med[ref] / n_frames, med["B"] / n_frames
        lim = max(spread[ref], spread["B"]) / n_frames
        verdict = "faster" if per_ref - per_b > lim else "slower" if per_b - per_ref > lim else "NOT different beyond the spread"
        say(f"{kind} frames={n_frames} statement (per frame, {ref} = {what}, against B = device_prep on): {ref} {per_ref:.2f} us, B {per_b:.2f} us, "
            f"{ref} - B = {per_ref - per_b:.2f} us, larger p10-p90 spread of the two legs {lim:.2f} us per frame: B is {verdict}")
    cells, width, k = rows.shape[1], rows.shape[2], sur.ROWS_KINDS[kind][1]
    say(f"{kind} frames={n_frames} statement (the two launches alone): r {med['r']:.2f} us per call for {n_frames} x {cells} cells x ({width * 4} B in + {8 * k} B out) = "
        f"{n_frames * cells * (width * 4 + 8 * k) / 1e6:.2f} MB, {med['r'] / 2:.2f} us per launch")
    for ev in (old, new):
        if ev is not None:
            ev._sur.close()
    d_rows.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", default="deltas,poisson,gradp")
    ap.add_argument("--out")
    args = ap.parse_args()
    h = ps.hip_api()
    _lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    parent = ps.second_library(args.parent_lib) if args.parent_lib else None
    serve_frames_from_memory()
    say(f"# tools/frame_rows.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for kind in args.only.split(","):
        with tempfile.TemporaryDirectory() as d:
            c = cases.build_gradp_dataset_case(d) if kind == "gradp" else cases.build_dataset_case(d, poisson=(kind == "poisson"))
            c["dir"] = d
            for n in (int(v) for v in args.frames.split(",")):
                run(kind, n, args, h, stream, parent, c)
            if args.out:                          # after every evaluator: a run cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
