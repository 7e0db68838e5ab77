"""A/B of the SDF fold of the bound single-case encode against a second library (the parent commit's build) in ONE process on one
box: BASELINE configs[1] (256 x 256 U_to_gradP) and configs[2] (deltaU_to_deltaP with a row scale), geometry bound, device-pointer
entry.  Legs, alternated `--rounds` times: parent library, this library with the fold, this library with PSM_SDF_FOLD=0 (the
switch is read per solve and is part of the graph key).  Per leg 200 event-separated samples of 50 solves: p50 / p10 / p90 in us.
Then the dispatch medians of every launch (psm_time_kernels_q) for the three.

    python tools/sdf_fold_ab.py --parent-lib PATH [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import pressure_step as ps                      # noqa: E402  (its helpers: second library, event-timed samples, dispatch medians)
from pressure_step import psm_amd, synthetic, DeviceArray, say   # noqa: E402


def run(tag, variant, out_scale, args, h, stream, parent):
    ny = nx = 256
    model = synthetic.make_model(variant)
    grid = synthetic.channel_grid(ny, nx, seed=1)[None].astype(np.float32)
    d_in, d_out = DeviceArray(grid), DeviceArray(shape=(1, ny, nx, model.c_out))
    if args.new_first:                          # which handle allocates first: its buffers' placement is the only difference between identical kernels
        new = psm_amd.GridSurrogate(model, ny, nx)
        old = ps.surrogate_on(parent, model, ny, nx)
    else:
        old = ps.surrogate_on(parent, model, ny, nx)
        new = psm_amd.GridSurrogate(model, ny, nx)
    t0 = time.perf_counter()
    assert old.lib.psm_bind_geometry_cases(old.h, C.c_void_p(d_in.ptr), 1, 1) == 0
    t1 = time.perf_counter()
    assert new.bind_geometry(d_in.ptr, on_device=True)          # the first bind also packs the folded basis
    t2 = time.perf_counter()
    assert new.bind_geometry(d_in.ptr, on_device=True)
    t3 = time.perf_counter()
    say(f"{tag} bind_ms parent={1e3 * (t1 - t0):.1f} new_first={1e3 * (t2 - t1):.1f} new_again={1e3 * (t3 - t2):.1f}")

    def leg(sur, fold):
        def step(i):
            sur.solve_device(d_in.ptr, 1, d_out.ptr, stream.value, out_scale=out_scale)
        def go():
            os.environ["PSM_SDF_FOLD"] = fold
            return ps.measure(h, stream, step, args.steps)
        return go
    legs = {"parent": leg(old, "1"), "fold": leg(new, "1"), "fold_off": leg(new, "0")}
    res = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, go in legs.items():
            r = go()
            res[name].append(r)
            say(f"{tag} round={rnd} leg={name:8s} mean_us={r[0]:8.2f} p50_us={r[1]:8.2f} p10_us={r[2]:8.2f} p90_us={r[3]:8.2f}")
    for k, v in res.items():
        say(f"{tag} summary leg={k:8s} p50_us={np.median([r[1] for r in v]):.2f} min_p10_us={min(r[2] for r in v):.2f} max_p90_us={max(r[3] for r in v):.2f}")
    for name, sur, fold in (("parent", old, "1"), ("fold", new, "1"), ("fold_off", new, "0")):
        os.environ["PSM_SDF_FOLD"] = fold
        sur.synchronize()
        for nm, m, lo, hi, n in ps.kernel_medians(sur, d_in.ptr, 1, d_out.ptr, 500):
            say(f"{tag} kernel lib={name:8s} {nm:56s} median_us={m:7.2f} p10_us={lo:7.2f} p90_us={hi:7.2f} launches={n}")
    os.environ["PSM_SDF_FOLD"] = "1"
    new.close(); old.close()
    d_in.free(); d_out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new-first", action="store_true", help="create this library's handle before the parent's")
    ap.add_argument("--out")
    args = ap.parse_args()
    h = ps.hip_api()
    ps._lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    parent = ps.second_library(args.parent_lib)
    say(f"# tools/sdf_fold_ab.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} rounds={args.rounds} new_first={int(args.new_first)} "
        f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')}")
    run("configs[1]", "gradp", None, args, h, stream, parent)
    run("configs[2]", "deltas", [0.75], args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
