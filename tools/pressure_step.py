"""What the device-resident U -> p step costs on the headline workload (256 x 256 gradP, geometry and integration bound,
input and output in HBM), by bench.py's protocol: >= 200 untimed steps, K = 2000 timed steps between two
synchronisations, then 200 event-separated samples of 50 steps for p50 / p10 / p90; all legs in ONE process on one box,
alternated (a, b, c, a0, a, b, c, a0) rather than each run once, profiler off.

  a   psm_solve_grid_device alone: the step ends with (dp/dx, dp/dy) in HBM
  b   psm_solve_pressure_device: the step ends with p in HBM (one graph replay: the solve's launches + the two of the integration)
  c   the way to p without it: a + synchronise + D2H of the gradient + psm_integrate_gradp (host entry) -- single case only
  a0  leg a on a second library (--parent-lib, e.g. the parent commit's build): did the solve itself move?

    python tools/pressure_step.py [--parent-lib PATH] [--cases 1,8] [--steps 2000] [--rounds 2] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")          # as bench.py: the host program's choice, read once by the runtime

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import psm_amd                                   # noqa: E402
from psm_amd import _lib, synthetic              # noqa: E402
from hipmem import DeviceArray, hip              # noqa: E402

Q_SAMPLES, Q_CHUNK, WARMUP = 200, 50, 200
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def cut_of(sdf):
    """(cy, cx): middle row of the obstacle's rows (rounded up), middle column of the obstacle on that row."""
    solid = sdf == 0
    rows = np.where(solid.any(1))[0]
    cy = int((rows.min() + rows.max() + 1) // 2)
    cols = np.where(solid[cy])[0]
    return cy, int((cols.min() + cols.max()) // 2)


def hip_api():
    h = hip()
    h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    h.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return h


def second_library(path):
    """A second libpsm_hip.so in this process, bound with the signatures it has.  RTLD_DEEPBIND: _lib.load() puts the first
    library's symbols into the global scope, and without it the second library's calls to its own exported functions and
    kernel stubs bind to the FIRST library's (another handle layout: heap corruption)."""
    lib = C.CDLL(path, mode=C.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    assert lib.psm_abi_version() == _lib.PSM_ABI_VERSION
    return lib


def surrogate_on(lib, *a, **kw):
    """GridSurrogate whose handle lives in `lib` (the constructor takes the library from _lib.load())."""
    mine = _lib.load()
    _lib._lib = lib
    try:
        return psm_amd.GridSurrogate(*a, **kw)
    finally:
        _lib._lib = mine


def measure(h, stream, step, steps):
    """(mean us per step over `steps`, p50, p10, p90 of Q_SAMPLES event-separated chunks of Q_CHUNK steps)."""
    for i in range(WARMUP):
        step(i)
    assert h.hipStreamSynchronize(stream) == 0
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    assert h.hipStreamSynchronize(stream) == 0
    mean_us = (time.perf_counter() - t0) / steps * 1e6
    evs = []
    for _ in range(Q_SAMPLES + 1):
        e = C.c_void_p()
        assert h.hipEventCreate(C.byref(e)) == 0
        evs.append(e)
    for j in range(Q_CHUNK):                      # a filled pipeline in front of the first event
        step(j)
    h.hipEventRecord(evs[0], stream)
    for i in range(Q_SAMPLES):
        for j in range(Q_CHUNK):
            step(j)
        h.hipEventRecord(evs[i + 1], stream)
    assert h.hipStreamSynchronize(stream) == 0
    per = []
    for i in range(Q_SAMPLES):
        ms = C.c_float()
        assert h.hipEventElapsedTime(C.byref(ms), evs[i], evs[i + 1]) == 0
        per.append(ms.value / Q_CHUNK * 1e3)
    per.sort()
    return mean_us, per[Q_SAMPLES // 2], per[Q_SAMPLES // 10], per[Q_SAMPLES * 9 // 10]


def kernel_medians(sur, d_grid, n_cases, d_fields, steps):
    cap = 32
    names = C.create_string_buffer(cap * 64)
    med, p10, p90 = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    cnt = (C.c_int64 * cap)()
    nk = C.c_int32()
    sur._chk(sur.lib.psm_time_kernels_q(sur.h, C.c_void_p(d_grid), n_cases, C.c_void_p(d_fields), steps, names, med, p10, p90, cnt, cap, C.byref(nk)))
    return [(names.raw[k * 64:(k + 1) * 64].split(b"\0", 1)[0].decode(), med[k], p10[k], p90[k], cnt[k]) for k in range(min(nk.value, cap))]


def run(n_cases, args, h, stream, parent):
    ny = nx = 256
    model = synthetic.make_model("gradp")                      # BASELINE configs[1]: 128 components in and out
    grids = (synthetic.channel_grid(ny, nx, seed=1)[None] if n_cases == 1 else synthetic.random_obstacle_cases(n_cases, ny, nx, seed=3)).astype(np.float32)
    cuts = np.array([cut_of(g[..., 2]) for g in grids], np.int32)
    d_in, d_grad = DeviceArray(grids), DeviceArray(shape=(n_cases, ny, nx, 2))
    d_p = DeviceArray(shape=(n_cases, ny, nx))
    sur = psm_amd.GridSurrogate(model, ny, nx, max_cases=n_cases)
    assert sur.bind_geometry(d_in.ptr, on_device=True, n_cases=n_cases)
    assert sur.bind_integration(grids[..., 2], cuts[:, 0], cuts[:, 1], 1.0 / nx, 1.0 / ny)
    legs = {"a": lambda i: sur.solve_device(d_in.ptr, n_cases, d_grad.ptr, stream.value),
            "b": lambda i: sur.solve_pressure_device(d_in.ptr, n_cases, d_p.ptr, stream=stream.value)}
    if n_cases == 1:
        sur.set_integration(grids[0, ..., 2], cuts[0, 0], cuts[0, 1], 1.0 / nx, 1.0 / ny)
        pin_g, pin_p = C.c_void_p(), C.c_void_p()
        assert h.hipHostMalloc(C.byref(pin_g), ny * nx * 2 * 4, 0) == 0 and h.hipHostMalloc(C.byref(pin_p), ny * nx * 4, 0) == 0
        f32p = C.POINTER(C.c_float)

        def leg_c(i):
            sur.solve_device(d_in.ptr, 1, d_grad.ptr, stream.value)
            h.hipMemcpyAsync(pin_g, d_grad.ptr, ny * nx * 2 * 4, 2, stream)
            h.hipStreamSynchronize(stream)
            sur.lib.psm_integrate_gradp(sur.h, C.cast(pin_g, f32p), C.cast(pin_p, f32p))
        legs["c"] = leg_c
    if parent is not None:
        sur0 = surrogate_on(parent, model, ny, nx, max_cases=n_cases)
        assert sur0.lib.psm_bind_geometry_cases(sur0.h, C.c_void_p(d_in.ptr), n_cases, 1) == 0
        legs["a0"] = lambda i: sur0.solve_device(d_in.ptr, n_cases, d_grad.ptr, stream.value)
    res = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = measure(h, stream, step, args.steps)
            res[name].append(r)
            say(f"cases={n_cases} round={rnd} leg={name:2s} mean_us={r[0]:8.2f} p50_us={r[1]:8.2f} p10_us={r[2]:8.2f} p90_us={r[3]:8.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res.items()}
    say(f"cases={n_cases} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) + f"  b-a={med['b'] - med['a']:.2f}")
    sur.synchronize()
    for nm, m, lo, hi, n in kernel_medians(sur, d_in.ptr, n_cases, d_grad.ptr, 500):
        say(f"cases={n_cases} kernel {nm:56s} median_us={m:7.2f} p10_us={lo:7.2f} p90_us={hi:7.2f} launches={n}")
    sur.close()
    if parent is not None:
        sur0.close()
    for d in (d_in, d_grad, d_p):
        d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--cases", default="1,8")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    h = hip_api()
    _lib.load()
    stream = C.c_void_p()
    assert h.hipStreamCreate(C.byref(stream)) == 0
    parent = second_library(args.parent_lib) if args.parent_lib else None
    say(f"# tools/pressure_step.py steps={args.steps} warmup={WARMUP} samples={Q_SAMPLES}x{Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for n in (int(c) for c in args.cases.split(",")):
        run(n, args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
