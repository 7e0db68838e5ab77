"""What the device-resident Poisson input features cost on the pressureSM_Poisson workload (256 x 256 deltas handle with c_in = 4,
geometry bound, velocities in and fields out in HBM), by the protocol of tools/poststeps_step.py: >= 200 untimed
steps, K = 2000 timed steps between two synchronisations, then 200 event-separated samples of 50 steps for p50 / p10 / p90; all
legs in ONE process on one box, alternated rather than each run once, profiler off.

  a   psm_solve_poststeps_device alone on a resident image (weighting and apply_filter): result, change and next in HBM
  b   psm_poisson_step_device: the two feature launches in front of a, one graph replay, (L, U) uploaded per step
  c   what b replaces: host psm_poisson_features per case (5 planes H2D, image D2H, synchronous), the image into pinned memory and
      H2D again, then a -- single case only; on the library given with --parent-lib (the parent commit's build), else on this one
      (K / 10 steps: the leg is an order of magnitude slower)
  a0  leg a on the --parent-lib library: did the solve itself move?
After the legs: per-kernel dispatch medians of the b step (psm_time_kernels_q), and the three statements read off the lines above.

    python tools/poisson_step.py [--parent-lib PATH] [--cases 1,8] [--steps 2000] [--rounds 2] [--out FILE]
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
from psm_amd import _lib, synthetic              # noqa: E402
from hipmem import DeviceArray                   # noqa: E402
import poststeps_step as ps                      # noqa: E402  (measure, kernel_medians, second_library, surrogate_on, hip_api)

K, MAX_ABS, P_SCALE = 0.5, (2.7, 0.031, 0.027, 0.29), 0.51
say = ps.say


def poisson_case(ny, nx, s):
    """cases.build_poisson_case() at ny x nx with seeds moved by the case index."""
    g = synthetic.channel_grid(ny, nx, seed=51 + 2 * s, obstacle="circle")
    d = synthetic.delta_grid(ny, nx, seed=52 + 2 * s, step=3 + s)
    sdf = g[..., 2] * 0.3
    c = dict(ux=1.3 * g[..., 0], uy=1.3 * g[..., 1], dux=0.05 * d[..., 0], duy=0.05 * d[..., 1])
    for a in c.values():
        a[sdf == 0] = 0.0
    c.update(sdfunct=sdf, L=0.25 + 0.01 * s, U=float(np.sqrt(c["ux"] ** 2 + c["uy"] ** 2).max()))
    return c


def run(n_cases, args, h, stream, parent):
    ny = nx = 256
    npix = ny * nx
    model = synthetic.make_model("deltas", c_in=4, seed_pca=777, seed_w=5)    # 128 components in and out, mask = channel 3
    model.sdf_ch = 3
    cs = [poisson_case(ny, nx, s) for s in range(n_cases)]
    vel = np.ascontiguousarray(np.stack([np.stack([c["ux"], c["uy"], c["dux"], c["duy"]]) for c in cs]), dtype=np.float64)
    lu = np.array([[c["L"], c["U"]] for c in cs], np.float64)
    sc = [P_SCALE * c["U"] ** 2 for c in cs]
    rng = np.random.default_rng(9)
    dU = np.abs(rng.standard_normal((n_cases, ny, nx))).astype(np.float32)
    dU /= dU.max()
    prev = (0.1 * rng.standard_normal((n_cases, ny, nx))).astype(np.float32)
    d_vel, d_img = DeviceArray(vel), DeviceArray(shape=(n_cases, ny, nx, 4))
    d_u, d_p = DeviceArray(dU), DeviceArray(prev)
    d_r, d_c, d_n = (DeviceArray(shape=(n_cases, ny, nx)) for _ in range(3))
    sur = psm_amd.GridSurrogate(model, ny, nx, max_cases=n_cases)
    sur.bind_poststeps((10, 10), (50, 50))
    sur.bind_features(np.stack([c["sdfunct"] for c in cs]), K, MAX_ABS)
    sur.features_device(d_vel.ptr, n_cases, lu, d_img.ptr)
    sur.synchronize()
    assert sur.bind_geometry(d_img.ptr, on_device=True, n_cases=n_cases)
    post = lambda s_, img: s_.solve_poststeps_device(img, n_cases, d_r.ptr, True, d_u.ptr, d_p.ptr, d_c.ptr, d_n.ptr, stream=stream.value,
                                                     out_scale=sc)
    # b gives what features_device -> a gives, bit for bit
    post(sur, d_img.ptr)
    sur.synchronize()
    want = [d.numpy() for d in (d_r, d_c, d_n)]
    step_b = lambda i: sur.poisson_step_device(d_vel.ptr, n_cases, lu, d_r.ptr, True, d_u.ptr, d_p.ptr, d_c.ptr, d_n.ptr, stream=stream.value,
                                               out_scale=sc)
    step_b(0)
    sur.synchronize()
    say(f"cases={n_cases} check b == features_device -> a: {all(np.array_equal(d.numpy(), w) for d, w in zip((d_r, d_c, d_n), want))} "
        f"guard_trips={sur.guard_trips}")
    legs = {"a": lambda i: post(sur, d_img.ptr), "b": step_b}
    sur0 = None
    if parent is not None:
        sur0 = ps.surrogate_on(parent, model, ny, nx, max_cases=n_cases)
        sur0.bind_poststeps((10, 10), (50, 50))
        assert sur0.lib.psm_bind_geometry_cases(sur0.h, C.c_void_p(d_img.ptr), n_cases, 1) == 0
        legs["a0"] = lambda i: post(sur0, d_img.ptr)
    if n_cases == 1:
        old = sur0 if sur0 is not None else sur
        pin = C.c_void_p()
        assert h.hipHostMalloc(C.byref(pin), npix * 16, 0) == 0
        img_pin = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_float)), shape=(ny, nx, 4))
        d_img_c = DeviceArray(shape=(1, ny, nx, 4))
        c0 = cs[0]

        def leg_c(i):
            img_pin[...] = old.poisson_features(c0["ux"], c0["uy"], c0["dux"], c0["duy"], c0["sdfunct"], c0["L"], c0["U"], K, MAX_ABS)
            h.hipMemcpyAsync(d_img_c.ptr, pin, npix * 16, 1, stream)
            post(old, d_img_c.ptr)
        legs["c"] = leg_c
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = ps.measure(h, stream, step, args.steps if name != "c" else max(200, args.steps // 10))
            res_[name].append(r)
            say(f"cases={n_cases} round={rnd} leg={name:2s} mean_us={r[0]:8.2f} p50_us={r[1]:8.2f} p10_us={r[2]:8.2f} p90_us={r[3]:8.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    spread = {k: float(np.median([r[3] - r[2] for r in v])) for k, v in res_.items()}
    say(f"cases={n_cases} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + "  p10-p90 spread_us " +
        " ".join(f"{k}={v:.2f}" for k, v in spread.items()))
    sur.synchronize()
    sur.poisson_step(vel, lu, out_scale=sc, apply_filter=True, dU=dU, prev=prev)     # leaves these velocities and scalars in the staging planes
    feat = 0.0
    for nm, m, lo, hi, n in ps.kernel_medians(sur, d_img.ptr, n_cases, d_r.ptr, 500):
        say(f"cases={n_cases} kernel {nm:56s} median_us={m:7.2f} p10_us={lo:7.2f} p90_us={hi:7.2f} launches={n}")
        feat += m if nm.startswith("psm_poisson_") else 0.0
    say(f"cases={n_cases} statement 1 (the features add launch cost only): b - a = {med['b'] - med['a']:.2f} us; "
        f"the two feature dispatch medians sum to {feat:.2f} us")
    if "c" in med:
        gain, worst = med["c"] - med["b"], max(spread["b"], spread["c"])
        say(f"cases={n_cases} statement 2 (the round trip is gone): c - b = {gain:.2f} us on {'the parent' if sur0 else 'THIS'} library, larger "
            f"p10-p90 spread of the two legs {worst:.2f} us: {'holds' if gain > worst else 'DOES NOT HOLD'}")
    if "a0" in med:
        moved, lim = abs(med["a"] - med["a0"]), max(spread["a"], spread["a0"])
        say(f"cases={n_cases} statement 3 (the solve itself did not move): |a - a0| = {moved:.2f} us, larger p10-p90 spread of the two legs "
            f"{lim:.2f} us: {'holds' if moved <= lim else 'DOES NOT HOLD'}")
    sur.close()
    if sur0 is not None:
        sur0.close()
    for d in (d_vel, d_img, d_u, d_p, d_r, d_c, d_n):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--cases", default="1,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    h = ps.hip_api()
    _lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    parent = ps.second_library(args.parent_lib) if args.parent_lib else None
    say(f"# tools/poisson_step.py steps={args.steps} warmup={ps.WARMUP} samples={ps.Q_SAMPLES}x{ps.Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for n in (int(c) for c in args.cases.split(",")):
        run(n, args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(ps._lines) + "\n")


if __name__ == "__main__":
    main()
