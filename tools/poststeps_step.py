"""What the device-resident Gaussian post-steps cost on the deltas workload (256 x 256, BASELINE configs[2], geometry bound, input
and output in HBM), by bench.py's protocol: >= 200 untimed steps, K = 2000 timed steps between two
synchronisations, then 200 event-separated samples of 50 steps for p50 / p10 / p90; all legs in ONE process on one box,
alternated rather than each run once, profiler off.

  a   psm_solve_grid_device alone: the step ends with the assembled delta-p in HBM
  b1  psm_solve_poststeps_device with the deltaU-change weighting and apply_filter: result, change and next in HBM (one graph
      replay: the solve's launches + four of psm_gauss1d_kernel)
  b0  the same without apply_filter
  c1  what b1 replaces: a + synchronise + D2H of the field + three psm_gaussian_filter host calls (two for c0) with the NumPy
      arithmetic between them -- single case only; on the library given with --parent-lib (the parent commit's build, i.e. the
      old one-thread-per-pixel kernel), else on this one (K / 10 steps: the leg is an order of magnitude slower)
  a0  leg a on the --parent-lib library: did the solve itself move?
After the legs: per-kernel dispatch medians of the b1 step (psm_time_kernels_q).

    python tools/poststeps_step.py [--parent-lib PATH] [--cases 1,8] [--steps 2000] [--rounds 2] [--out FILE]
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
    npix = ny * nx
    model = synthetic.make_model("deltas")                     # BASELINE configs[2]: 128 components in and out
    grids = np.stack([synthetic.delta_grid(ny, nx, seed=2, step=s) for s in range(n_cases)]).astype(np.float32)
    rng = np.random.default_rng(9)
    dU = np.abs(rng.standard_normal((n_cases, ny, nx))).astype(np.float32)
    dU /= dU.max()
    prev = (0.1 * rng.standard_normal((n_cases, ny, nx))).astype(np.float32)
    d_in, d_f = DeviceArray(grids), DeviceArray(shape=(n_cases, ny, nx, 1))
    d_u, d_p = DeviceArray(dU), DeviceArray(prev)
    d_r, d_c, d_n = (DeviceArray(shape=(n_cases, ny, nx)) for _ in range(3))
    sur = psm_amd.GridSurrogate(model, ny, nx, max_cases=n_cases)
    assert sur.bind_geometry(d_in.ptr, on_device=True, n_cases=n_cases)
    legs = {"a": lambda i: sur.solve_device(d_in.ptr, n_cases, d_f.ptr, stream.value)}
    sur0 = None
    if parent is not None:
        sur0 = surrogate_on(parent, model, ny, nx, max_cases=n_cases)
        assert sur0.lib.psm_bind_geometry_cases(sur0.h, C.c_void_p(d_in.ptr), n_cases, 1) == 0
        legs["a0"] = lambda i: sur0.solve_device(d_in.ptr, n_cases, d_f.ptr, stream.value)
    if n_cases == 1:
        # what b replaces: the solve, a synchronise, the field to the host, one psm_gaussian_filter round trip per filter
        old = sur0 if sur0 is not None else sur
        pin = C.c_void_p()
        assert h.hipHostMalloc(C.byref(pin), npix * 4, 0) == 0
        res = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_float)), shape=(ny, nx))

        def leg_c(apply_filter):
            def step(i):
                old.solve_device(d_in.ptr, 1, d_f.ptr, stream.value)
                h.hipMemcpyAsync(pin, d_f.ptr, npix * 4, 2, stream)
                h.hipStreamSynchronize(stream)
                r = old.gaussian_filter(res, (10, 10)) if apply_filter else res
                w = old.gaussian_filter(dU[0], (50, 50))
                return prev[0] + old.gaussian_filter((r - prev[0]) * w, (10, 10))
            return step
        legs["c1"], legs["c0"] = leg_c(True), leg_c(False)
    sur.bind_poststeps((10, 10), (50, 50))                     # after leg a's graph exists: the binding leaves it alone
    for name, af in (("b1", True), ("b0", False)):
        legs[name] = (lambda af: lambda i: sur.solve_poststeps_device(d_in.ptr, n_cases, d_r.ptr, af, d_u.ptr, d_p.ptr, d_c.ptr, d_n.ptr,
                                                                     stream=stream.value))(af)
    res_ = {k: [] for k in legs}
    for rnd in range(args.rounds):
        for name, step in legs.items():
            r = measure(h, stream, step, args.steps if name[0] != "c" else max(200, args.steps // 10))
            res_[name].append(r)
            say(f"cases={n_cases} round={rnd} leg={name:2s} mean_us={r[0]:8.2f} p50_us={r[1]:8.2f} p10_us={r[2]:8.2f} p90_us={r[3]:8.2f}")
    med = {k: float(np.median([r[1] for r in v])) for k, v in res_.items()}
    say(f"cases={n_cases} summary p50_us " + " ".join(f"{k}={v:.2f}" for k, v in med.items()) +
        f"  b1-a={med['b1'] - med['a']:.2f} b0-a={med['b0'] - med['a']:.2f}")
    sur.synchronize()
    for nm, m, lo, hi, n in kernel_medians(sur, d_in.ptr, n_cases, d_f.ptr, 500):
        say(f"cases={n_cases} kernel {nm:56s} median_us={m:7.2f} p10_us={lo:7.2f} p90_us={hi:7.2f} launches={n}")
    sur.close()
    if sur0 is not None:
        sur0.close()
    for d in (d_in, d_f, d_u, d_p, d_r, d_c, d_n):
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
    say(f"# tools/poststeps_step.py steps={args.steps} warmup={WARMUP} samples={Q_SAMPLES}x{Q_CHUNK} GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} "
        f"parent_lib={'yes' if parent else 'no'}")
    for n in (int(c) for c in args.cases.split(",")):
        run(n, args, h, stream, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
