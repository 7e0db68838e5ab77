"""What the device-side error blocks buy a metrics-only sweep of the pressureSM_Poisson evaluator (138 x 300 evaluator grid of the
dataset fixture, its 24-component four-channel deltas model, geometry bound for the batch), by the protocol of
tools/poisson_frames.py: >= 200 untimed steps, then 200 event-separated samples of 50 steps for p50 / p10 / p90;
all legs in ONE process on one box, alternated rather than each run once, profiler off.  A step is one batch of K frames.

  A    what EvaluationPoisson.timeSteps does per batch without the stage: psm_poisson_frames with the label planes (fields and
       planes copied back), then per frame the truth chain and the three error_metrics passes in NumPy -- on the library given with
       --parent-lib (the parent commit's build), else on this one
  A0   the psm_poisson_frames call of leg A alone: A - A0 is the host metric passes
  B    psm_poisson_frames_errors + psm_error_metrics_from_sums per row: 24 doubles per frame come back
  d    psm_poisson_frames_device: the step alone, columns and fields resident
  e    psm_poisson_frames_errors_device: the step with the stage behind it
  s    psm_field_errors_device alone on resident planes, the evaluator's three pairs: back-to-back calls, so the p50 is the two
       launches' dispatch-to-dispatch time
After the legs: the statements read off the lines above.

    python tools/frame_errors.py [--parent-lib PATH] [--frames 1,8] [--steps 2000] [--rounds 2] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # as bench.py: the host program's choice, read once by the runtime

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import psm_amd                                   # noqa: E402
from psm_amd import _lib, error_metrics          # noqa: E402
from hipmem import DeviceArray                   # noqa: E402
import cases                                     # noqa: E402
import poststeps_step as ps                      # noqa: E402  (measure, second_library, surrogate_on, hip_api)
import poisson_frames as pf                      # noqa: E402  (workload, prepare)

PHI = pf.PHI
say = ps.say


def host_metrics(res, nxt, extra, Us, no_flow, max_abs_delta_p):
    """The three error blocks of every frame as timeSteps takes them from the fields (EvaluationPoisson._record_fields, evaluators.py)."""
    out = []
    for j, U in enumerate(Us):
        field = nxt[j]
        cfd = np.nan_to_num(extra[j, 0] / pow(U, 2.0), nan=0.0) / max_abs_delta_p * max_abs_delta_p * pow(U, 2.0)
        p_grid = np.nan_to_num(extra[j, 1], nan=0.0)
        out.append((error_metrics(field, cfd, no_flow), error_metrics(res[j, :, :, 0], cfd, no_flow),
                    error_metrics((p_grid - cfd) + field, p_grid, no_flow)))
    return out


def run(n_frames, args, h, stream, parent):
    model, t, n_cells, cols, Us = pf.workload(n_frames)
    ny, nx = t.ny, t.nx
    npix = ny * nx
    lu = np.array([[PHI, U] for U in Us])
    mx = cases.POISSON_MAXS
    sc = [mx[4] * U ** 2 for U in Us]
    sur = psm_amd.GridSurrogate(model, ny, nx, max_cases=n_frames)
    pf.prepare(sur, t, n_cells, n_frames, True)
    old = sur
    if parent is not None:
        old = ps.surrogate_on(parent, model, ny, nx, max_cases=n_frames)
        pf.prepare(old, t, n_cells, n_frames, True)
    no_flow = np.nan_to_num(np.asarray(t.sdfunct, np.float64), nan=0.0) / mx[3] == 0
    d_cols = DeviceArray(cols)
    d_sdf = DeviceArray(np.repeat(np.asarray(t.sdfunct, np.float64)[None], n_frames, axis=0))
    d_x = DeviceArray(shape=(n_frames, 2, ny, nx), dtype=np.float64)
    d_r, d_c, d_n = (DeviceArray(shape=(n_frames, ny, nx)) for _ in range(3))
    d_raw = DeviceArray(shape=(n_frames, 3, 8), dtype=np.float64)
    dp, p = (d_x.ptr, 2 * npix, 1, 0), (d_x.ptr + 8 * npix, 2 * npix, 1, 0)
    nxt, res = (d_n.ptr, npix, 1, 1), (d_r.ptr, npix, 1, 1)
    pairs = [(nxt, dp, None, None, True), (res, dp, None, None, True), (nxt, p, p, dp, True)]

    def leg_A(_):
        r, _c, n, x = old.poisson_frames(cols, lu, out_scale=sc)
        return host_metrics(r, n, x, Us, no_flow, mx[4])

    def leg_B(_):
        raw = sur.poisson_frames_errors(cols, lu, out_scale=sc)
        return [tuple(sur.metrics_from_sums(raw[j, q]) for q in range(3)) for j in range(n_frames)]

    legs = {"A": leg_A, "A0": lambda _: old.poisson_frames(cols, lu, out_scale=sc), "B": leg_B,
            "d": lambda _: sur.poisson_frames_device(d_cols.ptr, n_frames, 8, lu, d_r.ptr, False, True, d_x.ptr, d_c.ptr, d_n.ptr, stream=stream.value,
                                                     out_scale=sc),
            "e": lambda _: sur.poisson_frames_errors_device(d_cols.ptr, n_frames, 8, lu, d_x.ptr, d_r.ptr, d_n.ptr, d_raw.ptr, False, d_c.ptr,
                                                            stream=stream.value, out_scale=sc),
            "s": lambda _: sur.field_errors_device((d_sdf.ptr, npix, 1, 0), pairs, n_frames, d_raw.ptr, stream=stream.value)}
    # B gives what A gives: every metric of every block of every frame, relative to the frame's rmseNorm / 100 (normVal, stdeNorm: relative)
    a, b = leg_A(0), leg_B(0)
    worst = 0.0
    for fa, fb in zip(a, b):
        for ma, mb in zip(fa, fb):
            for key in ma:
                scale = abs(ma[key]) if key in ("normVal", "stdeNorm") else ma["rmseNorm"] / 100 * (100 if key.endswith("Norm") else 1)
                worst = max(worst, abs(ma[key] - mb[key]) / scale)
    say(f"frames={n_frames} check B == A: worst difference of any metric {worst:.2e} of its scale, guard_trips={sur.guard_trips}")
    slow = ("A", "A0", "B")
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
    gain, lim = med["A"] - med["B"], max(spread["A"], spread["B"])
    say(f"frames={n_frames} statement (A on {lib_name} library against B): A - B = {gain:.2f} us, larger p10-p90 spread of the two legs {lim:.2f} us: "
        f"{'faster' if gain > lim else 'NOT faster beyond the spread'}; per frame A {med['A'] / n_frames:.2f} us, B {med['B'] / n_frames:.2f} us")
    say(f"frames={n_frames} statement (the host metric passes): A - A0 = {med['A'] - med['A0']:.2f} us, {(med['A'] - med['A0']) / n_frames:.2f} us per frame")
    say(f"frames={n_frames} statement (the stage's share): e - d = {med['e'] - med['d']:.2f} us, larger p10-p90 spread of the two legs "
        f"{max(spread['e'], spread['d']):.2f} us; the two launches alone, back to back: p50 {med['s']:.2f} us (p10-p90 spread {spread['s']:.2f} us)")
    sur.close()
    if old is not sur:
        old.close()
    for d in (d_cols, d_sdf, d_x, d_r, d_c, d_n, d_raw):
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
    say(f"# tools/frame_errors.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for n in (int(c) for c in args.frames.split(",")):
        run(n, args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
