"""Per-frame error blocks on the device (psm_field_errors_device, psm_poisson_frames_errors_device / psm_poisson_frames_errors,
psm_error_metrics_from_sums) and the metrics-only sweep of the Poisson evaluator on top of them (EvaluationPoisson.timeSteps(...,
fields=False), call_SM_main_Poisson(..., fields=False)): the three error blocks of pressureSM_Poisson/SM_call.py:962-1043 as eight
float64 sums per (frame, pair), reduced where the fields are.

Kernel tests run on 130 x 131 = 17 030 pixels (8 workgroups of 2048 pixels + 646: the last one is partly idle and its last vector of
four is cut) with max_cases = 3; plane pitches are odd, so that of the three frames of a plane some start 16-byte aligned (vector
loads) and some do not (one load per pixel).  The step behind the stage needs a mesh: 200 cells with random simplices and positive
weights on the same 130 x 131 grid, an obstacle of SDF zeros, NaNs in the two label columns.

References: NumPy on the same arrays -- counts and extrema bit for bit, the two sums against math.fsum (exact) within
1e-11 * sum|d| resp. 1e-11 * s2: any summation order of 17 030 terms is within n * u = 17 030 * 1.1e-16 = 1.9e-12 --; the stage
applied by hand to the planes psm_poisson_frames_device leaves (bit for bit); surrogate.error_metrics (the host path of timeSteps).
Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
from hipmem import DeviceArray
from psm_amd import EvaluationPoisson, GridSurrogate, _lib, call_SM_main_Poisson, error_metrics
from test_poisson_frames import PHI, Tables, bind_step, evaluator, same_bits, surrogate_on
from test_poisson_step_device import MAX_ABS, P_SCALE, error, free, model4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc")
NEW_ENTRIES = ("psm_field_errors_device", "psm_poisson_frames_errors_device", "psm_poisson_frames_errors", "psm_error_metrics_from_sums")
NEW_METHODS = ("field_errors_device", "poisson_frames_errors_device", "poisson_frames_errors", "metrics_from_sums")
NY, NX, NF = 130, 131, 3
NPIX = NY * NX
PAD, CANARY = 5, -7.5
SUM_TOL = 1e-11
KEYS = ("normVal", "biasNorm", "stdeNorm", "rmseNorm", "mean_err", "mean_sq_err")
N_, S1, S2, TMIN, TMAX, PMIN, PMAX, TNAN = range(8)
EXACT = (N_, TMIN, TMAX, PMIN, PMAX, TNAN)
_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------------------------- the NumPy statement
def nan0(a):
    return np.where(np.isnan(a), 0.0, a)


def flow_of(mask):
    m = np.asarray(mask, np.float64)
    return (m != 0) & ~np.isnan(m)


def differences(pred, truth, flow, add=None, sub=None, truth_nan_to_zero=False):
    """(truth, effective prediction, non-NaN differences) over the flow cells, float64, in the device's order of operations."""
    t = np.asarray(truth, np.float64)
    t = nan0(t) if truth_nan_to_zero else t
    pe = np.asarray(pred, np.float64)
    if add is not None or sub is not None:
        pe = (nan0(np.asarray(add, np.float64)) - nan0(np.asarray(sub, np.float64))) + pe
    else:
        pe = (0.0 - 0.0) + pe
    t, pe = t[flow], pe[flow]
    d = pe - t
    return t, pe, d[~np.isnan(d)]


def np_raw(pred, truth, flow, **kw):
    """One raw row as the library defines it, with np.sum for the two sums."""
    t, pe, d = differences(pred, truth, flow, **kw)
    tn, pn = t[~np.isnan(t)], pe[~np.isnan(pe)]
    return np.array([d.size, np.sum(d), np.sum(d ** 2), tn.min() if tn.size else np.inf, tn.max() if tn.size else -np.inf,
                     pn.min() if pn.size else np.inf, pn.max() if pn.size else -np.inf, np.isnan(t).sum()], np.float64)


def c_metrics(raw):
    out = np.empty(6)
    r = np.ascontiguousarray(raw, np.float64)
    assert _lib.load().psm_error_metrics_from_sums(r.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
    return dict(zip(KEYS, out))


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_entries_are_declared_bound_and_exported():
    """Every new name is in psm.h, in _lib.SIGNATURES and exported by the built library; the descriptors have the layout the
    library asserts; the mirrors exist and timeSteps / call_SM_main_Poisson take ``fields``."""
    import inspect
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "psm_err_plane" in txt and "psm_err_pair" in txt and re.search(r"#define\s+PSM_ERR_MAX_PAIRS\s+4\b", txt)
    assert re.search(r"#define\s+PSM_ABI_VERSION\s+4\b", txt) and _lib.PSM_ABI_VERSION == 4
    assert C.sizeof(_lib.psm_err_plane) == 32 and C.sizeof(_lib.psm_err_pair) == 136 and _lib.PSM_ERR_MAX_PAIRS == 4
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert inspect.signature(EvaluationPoisson.timeSteps).parameters["fields"].default is True
    assert inspect.signature(call_SM_main_Poisson).parameters["fields"].default is True


def test_metrics_from_sums_is_error_metrics():
    """psm_error_metrics_from_sums on raw rows taken in NumPy from random fields against error_metrics on the fields: normVal bit
    for bit, the rest within 1e-12 relative; a NaN truth on a flow cell -> all NaN on both sides; no finite difference -> all NaN
    from the C entry, ValueError from the mirror; a variance that rounds below zero -> NaN stde, everything else finite."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for trial in range(40):
        shape = (int(rng.integers(3, 90)), int(rng.integers(3, 90)))
        truth = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4)
        pred = (truth + (0.3 * rng.standard_normal(shape) + 0.2 * (trial % 4)) * np.abs(truth).max()).astype(np.float32)
        pred[rng.random(shape) < 0.02] = np.nan
        flow = rng.random(shape) < 0.8
        want = error_metrics(pred, truth, ~flow)
        raw = np_raw(pred, truth, flow)
        got, mirror = c_metrics(raw), GridSurrogate.metrics_from_sums(raw)
        assert got["normVal"] == want["normVal"] and mirror == {k: float(v) for k, v in got.items()}
        for k in KEYS[1:]:
            worst = max(worst, rel(got[k], want[k]))
    print(f"40 random fields: worst relative difference to error_metrics {worst:.2e} (bound 1e-12), normVal identical")
    assert worst <= 1e-12
    # a NaN truth on a flow cell
    truth, pred, flow = rng.standard_normal((20, 30)), rng.standard_normal((20, 30)), np.ones((20, 30), bool)
    truth[3, 4] = np.nan
    raw = np_raw(pred, truth, flow)
    with np.errstate(invalid="ignore"):
        want = error_metrics(pred, truth, ~flow)
    assert raw[TNAN] == 1 and all(math.isnan(v) for v in want.values()) and all(math.isnan(v) for v in c_metrics(raw).values())
    assert all(math.isnan(v) for v in GridSurrogate.metrics_from_sums(raw).values())
    # no finite difference: an empty mask, and flow cells whose every prediction is NaN
    for raw in (np_raw(pred, nan0(truth), np.zeros((20, 30), bool)), np_raw(np.full((20, 30), np.nan), nan0(truth), flow)):
        assert raw[N_] == 0 and all(math.isnan(v) for v in c_metrics(raw).values())
        with pytest.raises(ValueError, match="n == 0"):
            GridSurrogate.metrics_from_sums(raw)
    with pytest.raises(ValueError):
        error_metrics(pred, nan0(truth), np.ones((20, 30), bool))            # what NumPy does with the empty selection
    # rmse^2 < bias^2 after rounding: a constant difference, whose variance is rounding noise of either sign
    hits = 0
    for trial in range(400):
        truth = rng.standard_normal(997)
        pred = truth + rng.standard_normal() * 3.0
        flow = np.ones(997, bool)
        raw = np_raw(pred, truth, flow)
        got = c_metrics(raw)
        if not math.isnan(got["stdeNorm"]):
            continue
        hits += 1
        with np.errstate(invalid="ignore"):
            want = error_metrics(pred, truth, ~flow)
        assert got["normVal"] == want["normVal"] and all(rel(got[k], want[k]) <= 1e-12 for k in ("biasNorm", "rmseNorm", "mean_err", "mean_sq_err"))
        assert math.isnan(want["stdeNorm"]) or want["stdeNorm"] <= 1e-6 * want["rmseNorm"]
    print(f"constant differences: {hits} of 400 rows with rmse^2 < bias^2 after rounding, all with NaN stde and finite bias / rmse")
    assert hits >= 1


def test_python_argument_checks_come_before_any_library_call():
    """The new mirrors refuse bad arguments on a surrogate whose library and handle do not exist: any call into the library would
    raise AttributeError instead."""
    sur = GridSurrogate.__new__(GridSurrogate)
    sur.lib = sur.h = None
    sur.ny, sur.nx, sur.model, sur.mesh_cells, sur.max_cases = 6, 7, model4(), 11, 3
    p64, p32 = (4096, 42, 1, 0), (4100, 42, 1, 1)
    pair = (p32, p64, None, None, True)
    with pytest.raises(ValueError, match="1..4 pairs"):
        sur.field_errors_device(p64, [], 2, 4096)
    with pytest.raises(ValueError, match="1..4 pairs"):
        sur.field_errors_device(p64, [pair] * 5, 2, 4096)
    for n in (0, 4):
        with pytest.raises(ValueError, match="n_frames"):
            sur.field_errors_device(p64, [pair], n, 4096)
    for raw in (0, 4100):
        with pytest.raises(ValueError, match="d_raw"):
            sur.field_errors_device(p64, [pair], 2, raw)
    with pytest.raises(ValueError, match="mask"):
        sur.field_errors_device(None, [pair], 2, 4096)
    with pytest.raises(ValueError, match="pair 0 truth"):
        sur.field_errors_device(p64, [(p32, None, None, None, True)], 2, 4096)
    with pytest.raises(ValueError, match="negative"):
        sur.field_errors_device(p64, [((4096, -1, 1, 1), p64, None, None, True)], 2, 4096)
    with pytest.raises(ValueError, match="negative"):
        sur.field_errors_device(p64, [(p32, p64, (4096, 1, -2, 0), None, True)], 2, 4096)
    with pytest.raises(ValueError, match="not aligned"):
        sur.field_errors_device((4100, 42, 1, 0), [pair], 2, 4096)
    with pytest.raises(ValueError, match="not aligned"):
        sur.field_errors_device(p64, [((4098, 42, 1, 1), p64, None, None, True)], 2, 4096)
    with pytest.raises(ValueError, match="pred, truth, add, sub"):
        sur.field_errors_device(p64, [(p32, p64, True)], 2, 4096)
    lu = [[0.2, 1.0], [0.2, 1.1]]
    dev = lambda **kw: sur.poisson_frames_errors_device(**{**dict(d_cols=4096, n_frames=2, k=8, LU=lu, d_extra=4096, d_result=4096, d_next=4096,
                                                                 d_raw=4096), **kw})
    with pytest.raises(ValueError, match="at least 8 columns"):
        dev(k=7)
    with pytest.raises(ValueError, match="at most 16"):
        dev(k=17)
    for name in ("d_extra", "d_result", "d_next"):
        with pytest.raises(ValueError, match="none of them"):
            dev(**{name: 0})
    for raw in (0, 4100):
        with pytest.raises(ValueError, match="d_raw"):
            dev(d_raw=raw)
    with pytest.raises(ValueError, match="LU"):
        dev(LU=lu[:1])
    ok = np.zeros((2, 11, 8))
    with pytest.raises(ValueError, match="at least 8 columns"):
        sur.poisson_frames_errors(ok[..., :7], lu)
    with pytest.raises(ValueError, match=r"\[n,n_cells,k\]"):
        sur.poisson_frames_errors(np.zeros((2, 3, 11, 8)), lu)
    with pytest.raises(ValueError, match="11 cells"):
        sur.poisson_frames_errors(np.zeros((2, 12, 8)), lu)
    with pytest.raises(ValueError, match="LU"):
        sur.poisson_frames_errors(ok, lu[:1])
    with pytest.raises(ValueError, match="out_scale"):
        sur.poisson_frames_errors(ok, lu, out_scale=[1.0, 2.0, 3.0])
    sur.mesh_cells = None
    with pytest.raises(RuntimeError, match="no mesh"):
        sur.poisson_frames_errors(ok, lu)
    with pytest.raises(ValueError, match="8 sums"):
        GridSurrogate.metrics_from_sums(np.zeros(7))
    ev = EvaluationPoisson(5e-3, 128, 32, 0.95, 0.95, "no.hdf5", "no.h5", 128, "std", 0.5, None, model=model4(), max_frames=3)
    with pytest.raises(RuntimeError, match="computeOnlyOnce"):
        ev.timeSteps(0, [0, 1], fields=False)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_arithmetic_is_clean_under_asan_ubsan(tmp_path):
    """csrc/psm_errors.cpp in a stand-alone program (tests/native/field_errors_sanitized.cpp) under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "field_errors_sanitized")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "field_errors_sanitized.cpp"), os.path.join(CSRC, "psm_errors.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "rows checked:" in r.stdout


# ------------------------------------------------------------------------------------------------------- GPU, the stage alone
class Planes:
    """A host array [NF][pitch (* channels)] of one plane with an odd pitch, its device copy and its descriptor."""

    def __init__(self, values, dtype, channels=1, lead=0):
        self.pitch = NPIX + 1 + 2 * lead                       # odd: frame f starts (f * pitch + lead) elements into the buffer
        host = np.full((NF, self.pitch, channels), CANARY, dtype)
        host[:, lead:lead + NPIX, 0] = values
        self.values = host[:, lead:lead + NPIX, 0].copy()      # what the device reads, in the plane's own type
        self.dev = DeviceArray(host)
        size = np.dtype(dtype).itemsize
        self.desc = (self.dev.ptr + lead * channels * size, self.pitch * channels, channels, dtype == np.float32)


@functools.lru_cache(maxsize=None)
def stage_inputs():
    """Host values of the stage-alone test: mask [NF][NPIX] and four pairs, with the planted cases of the module docstring."""
    rng = np.random.default_rng(131)
    mask = rng.standard_normal((NF, NPIX)) * (rng.random((NF, NPIX)) < 0.8)
    mask[1] = 0.0                                              # frame 1: no flow cell at all
    mask[0, 17] = mask[2, NPIX - 1] = np.nan                   # a NaN mask value is no flow
    flow = flow_of(mask)
    on, off = [np.flatnonzero(f) for f in flow], [np.flatnonzero(~f) for f in flow]
    field = lambda s=1.0: rng.standard_normal((NF, NPIX)) * s
    pairs = []
    # 0: float32 pred, float64 truth as it is -- a NaN truth off the flow (does not count), one on a flow cell of frame 2
    p, t = field().astype(np.float32), field(3.0)
    p[0, on[0][:7]] = np.nan
    t[0, off[0][5]] = t[2, off[2][9]] = np.nan
    t[2, on[2][123]] = np.nan
    pairs.append(dict(pred=p, truth=t, add=None, sub=None, t0=False, dtypes=(np.float32, np.float64), channels=1))
    # 1: float32 pred with element stride 2, float32 truth with NaN -> 0, add and sub (with NaNs of their own)
    p, t, a, s = field().astype(np.float32), field(0.5).astype(np.float32), field(2.0), field(2.0)
    t[0, on[0][40:60]] = np.nan
    a[0, on[0][50:70]] = np.nan
    s[2, on[2][:30]] = np.nan
    pairs.append(dict(pred=p, truth=t, add=a, sub=s, t0=True, dtypes=(np.float32, np.float32), channels=2))
    # 2: float64 pred with NaNs on flow cells, float64 truth, add and sub, truth as it is (no NaN on a flow cell)
    p, t, a, s = field(), field(), field(0.1), field(0.1)
    p[2, on[2][1000:1100]] = np.nan
    t[0, off[0][77]] = np.nan
    pairs.append(dict(pred=p, truth=t, add=a, sub=s, t0=False, dtypes=(np.float64, np.float64), channels=1))
    # 3: float32 pred and truth behind a lead of 3 elements (no frame starts 16-byte aligned), NaN -> 0
    p, t = field().astype(np.float32), field().astype(np.float32)
    t[2, on[2][5]] = np.nan
    pairs.append(dict(pred=p, truth=t, add=None, sub=None, t0=True, dtypes=(np.float32, np.float32), channels=1, lead=3))
    return mask, pairs


def expected_rows(mask, pairs):
    """[NF][pairs][8] from NumPy plus, per row, (fsum(d), sum|d|, fsum(d^2)) for the two bounds."""
    raw, sums = np.empty((NF, len(pairs), 8)), {}
    for f in range(NF):
        flow = flow_of(mask[f])
        for q, pr in enumerate(pairs):
            kw = dict(truth_nan_to_zero=pr["t0"])
            if pr["add"] is not None:
                kw.update(add=pr["add"][f], sub=pr["sub"][f])
            raw[f, q] = np_raw(pr["pred"][f], pr["truth"][f], flow, **kw)
            d = differences(pr["pred"][f], pr["truth"][f], flow, **kw)[2]
            sums[f, q] = (math.fsum(d), math.fsum(np.abs(d)), math.fsum(d * d))
    return raw, sums


def check_rows(got, want, sums, label):
    """Counts and extrema bit for bit, the two sums within SUM_TOL of the exact ones; -> worst relative errors."""
    worst1 = worst2 = 0.0
    for (f, q), (s1, sabs, s2) in sums.items():
        g, w = got[f, q], want[f, q]
        assert same_bits(np.ascontiguousarray(g[list(EXACT)]), np.ascontiguousarray(w[list(EXACT)])), (label, f, q, g, w)
        e1, e2 = abs(g[S1] - s1), abs(g[S2] - s2)
        worst1, worst2 = max(worst1, e1 / sabs if sabs else e1), max(worst2, e2 / g[S2] if g[S2] else e2)
        assert e1 <= SUM_TOL * sabs and e2 <= SUM_TOL * g[S2], (label, f, q, e1, sabs, e2, g[S2])
    return worst1, worst2


def raw_buffer(n_pairs):
    return DeviceArray(np.full(PAD + NF * n_pairs * 8 + PAD, CANARY, np.float64))


def read_raw(d_raw, n_pairs, n_frames=NF):
    a = d_raw.numpy()
    body = NF * n_pairs * 8
    assert (a[:PAD] == CANARY).all() and (a[PAD + n_frames * n_pairs * 8:] == CANARY).all(), "canary round d_raw"
    return a[PAD:PAD + body].reshape(NF, n_pairs, 8)[:n_frames].copy()


@pytest.mark.gpu
def test_gpu_stage_alone_is_numpy_on_the_same_arrays():
    """Three frames x four pairs in one psm_field_errors_device, with a float64 and with a float32 mask: n, tmin, tmax, pmin, pmax
    and tnan are NumPy's bit for bit, s1 and s2 within 1e-11 of math.fsum; frame 1 (no flow cell) is n = 0 with tmin = +inf and
    tmax = -inf, frame 2 pair 0 has tnan = 1; the canaries round d_raw stay; a second call gives the same bits; a call with fewer
    pairs and frames gives the same rows."""
    mask, pairs = stage_inputs()
    want, sums = expected_rows(mask, pairs)
    assert want[2, 0, TNAN] == 1 and want[0, 0, TNAN] == 0 and (want[1, :, N_] == 0).all() and (want[0, :, N_] > 10000).all()
    assert (want[1, :, TMIN] == np.inf).all() and (want[1, :, TMAX] == -np.inf).all() and want[0, 0, N_] < flow_of(mask[0]).sum()
    with GridSurrogate(model4(), NY, NX, max_cases=NF) as sur:
        held, desc = [], []
        for pr in pairs:
            lead = pr.get("lead", 0)
            pl = {"pred": Planes(pr["pred"], pr["dtypes"][0], pr["channels"], lead), "truth": Planes(pr["truth"], pr["dtypes"][1], 1, lead)}
            for name in ("add", "sub"):
                pl[name] = Planes(pr[name], np.float64) if pr[name] is not None else None
            held += [p for p in pl.values() if p is not None]
            desc.append((pl["pred"].desc, pl["truth"].desc, pl["add"].desc if pl["add"] else None, pl["sub"].desc if pl["sub"] else None, pr["t0"]))
        aligned = sorted({(p.desc[0] + f * p.desc[1] * (4 if p.desc[3] else 8)) % 16 == 0 for p in held for f in range(NF)})
        assert aligned == [False, True], "the planes must start both 16-byte aligned and not"
        d_raw = raw_buffer(4)
        raw_ptr = d_raw.ptr + PAD * 8
        results = {}
        for name, dtype in (("float64 mask", np.float64), ("float32 mask", np.float32)):
            m = Planes(mask, dtype)
            assert np.array_equal(flow_of(m.values), flow_of(mask))
            sur.field_errors_device(m.desc, desc, NF, raw_ptr)
            sur.synchronize()
            got = read_raw(d_raw, 4)
            w1, w2 = check_rows(got, want, sums, name)
            sur.field_errors_device(m.desc, desc, NF, raw_ptr)
            sur.synchronize()
            again = read_raw(d_raw, 4)
            print(f"{name}: 12 rows, counts and extrema identical to NumPy, |s1 - fsum| / sum|d| <= {w1:.2e}, |s2 - fsum| / s2 <= {w2:.2e} "
                  f"(bound {SUM_TOL}); second call identical {same_bits(got, again)}; n per row {got[..., N_].astype(int).tolist()}")
            assert same_bits(got, again)
            results[name] = got
            held.append(m)
        assert same_bits(results["float64 mask"], results["float32 mask"])
        # two frames, pairs 2 and 1 only: the same rows in the caller's order, nothing written behind them
        d_two = raw_buffer(2)
        sur.field_errors_device(held[-1].desc, [desc[2], desc[1]], 2, d_two.ptr + PAD * 8)
        sur.synchronize()
        two = read_raw(d_two, 2, n_frames=2)
        assert same_bits(two, np.ascontiguousarray(results["float32 mask"][:2][:, [2, 1]]))
        free(d_raw, d_two, *[p.dev for p in held])


# ------------------------------------------------------------------------------------------------------- GPU, behind the step
@functools.lru_cache(maxsize=None)
def flow_tables():
    """130 x 131, 200 mesh cells: random simplices with positive weights (every plane is finite where its column is), every
    grid point in its own cell, an SDF with a rectangle of zeros (no flow) in it."""
    ng, n_cells = NPIX, 200
    rng = np.random.default_rng(1303)
    vtx = rng.integers(0, n_cells, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    wts = np.ascontiguousarray(np.c_[w, 1.0 - w.sum(axis=1)])
    cell = np.arange(ng)
    sdf = 0.05 + 0.2 * rng.random((NY, NX))
    sdf[40:75, 30:70] = 0.0
    return Tables(NY, NX, n_cells, vtx, wts, np.c_[cell // NX, cell % NX].astype(np.int32), sdf)


@functools.lru_cache(maxsize=None)
def frame_inputs():
    """(cols [NF][200][8], LU, out_scale): the evaluator's eight columns with other values per frame; NaNs in both label columns."""
    t = flow_tables()
    rng = np.random.default_rng(77)
    cols = rng.standard_normal((NF, t.n_cells, 8)) * (1.0 + 0.3 * np.arange(NF))[:, None, None]
    cols[..., 2:4] *= 0.05
    cols[..., 6] = np.abs(cols[..., 6]) / np.abs(cols[..., 6]).max(axis=1, keepdims=True)
    cols[..., 7] *= 0.1
    cols[0, 3:6, 4] = cols[1, 10:12, 5] = cols[2, 50, 4] = cols[2, 50, 5] = np.nan
    U = [float(np.sqrt(cols[f, :, 0] ** 2 + cols[f, :, 1] ** 2).max()) for f in range(NF)]
    return np.ascontiguousarray(cols), np.array([[PHI, u] for u in U]), [P_SCALE * u ** 2 for u in U]


class StepBuffers:
    def __init__(self, t, n=NF):
        self.extra = DeviceArray(np.full((n, 2, t.ny, t.nx), CANARY, np.float64))
        self.res, self.chg, self.nxt = (DeviceArray(np.full((n, t.ny, t.nx), CANARY, np.float32)) for _ in range(3))
        self.raw = raw_buffer(3)

    def fields(self):
        return tuple(d.numpy() for d in (self.res, self.chg, self.nxt, self.extra))

    def free(self):
        free(self.extra, self.res, self.chg, self.nxt, self.raw)


def evaluator_pairs(b, npix):
    """The three pairs of psm_poisson_frames_errors_device on the buffers of one step, as the caller of the stage states them."""
    dp, p = (b.extra.ptr, 2 * npix, 1, 0), (b.extra.ptr + 8 * npix, 2 * npix, 1, 0)
    nxt, res = (b.nxt.ptr, npix, 1, 1), (b.res.ptr, npix, 1, 1)
    return [(nxt, dp, None, None, True), (res, dp, None, None, True), (nxt, p, p, dp, True)]


def numpy_rows(fields, sdf):
    """The same three pairs in NumPy on the downloaded planes -> [n][3][8]."""
    res, _, nxt, extra = fields
    flow = flow_of(sdf).reshape(-1)
    out = np.empty((res.shape[0], 3, 8))
    for f in range(res.shape[0]):
        dp, p, r, x = extra[f, 0].reshape(-1), extra[f, 1].reshape(-1), res[f].reshape(-1), nxt[f].reshape(-1)
        out[f, 0] = np_raw(x, dp, flow, truth_nan_to_zero=True)
        out[f, 1] = np_raw(r, dp, flow, truth_nan_to_zero=True)
        out[f, 2] = np_raw(x, p, flow, add=p, sub=dp, truth_nan_to_zero=True)
    return out


def bind_other_geometry(sur, t):
    """A geometry whose flow-cell pattern is not the frames': the next bound solve trips the guard."""
    g = np.zeros((NF, t.ny, t.nx, 4), np.float32)
    g[..., 3] = (np.roll(t.sdfunct, 11, axis=1) / MAX_ABS[3]).astype(np.float32)[None]
    assert sur.bind_geometry(g) and sur.geometry_bound


def bind_own_geometry(sur, t):
    g = np.zeros((NF, t.ny, t.nx, 4), np.float32)
    g[..., 3] = (t.sdfunct / MAX_ABS[3]).astype(np.float32)[None]
    assert sur.bind_geometry(g) and sur.geometry_bound


@pytest.mark.gpu
def test_gpu_stage_behind_the_step_is_the_stage_on_the_steps_planes():
    """psm_poisson_frames_errors_device against psm_poisson_frames_device followed by psm_field_errors_device on the planes it left,
    general and bound route, with and without the filter: raw bit for bit; result / change / next / label planes are the same bits
    with and without the stage behind the step; counts and extrema are NumPy's on the downloaded planes."""
    t = flow_tables()
    cols, lu, sc = frame_inputs()
    npix = t.ny * t.nx
    with surrogate_on(t) as sur:
        bind_step(sur, t)
        d_cols, d_sdf = DeviceArray(cols), DeviceArray(np.repeat(t.sdfunct[None], NF, axis=0))
        for route in ("general", "bound"):
            if route == "bound":
                bind_own_geometry(sur, t)
            for af in (False, True):
                a, b = StepBuffers(t), StepBuffers(t)
                sur.poisson_frames_device(d_cols.ptr, NF, 8, lu, a.res.ptr, af, True, a.extra.ptr, a.chg.ptr, a.nxt.ptr, out_scale=sc)
                sur.field_errors_device((d_sdf.ptr, npix, 1, 0), evaluator_pairs(a, npix), NF, a.raw.ptr + PAD * 8)
                sur.poisson_frames_errors_device(d_cols.ptr, NF, 8, lu, b.extra.ptr, b.res.ptr, b.nxt.ptr, b.raw.ptr + PAD * 8, af, b.chg.ptr,
                                                 out_scale=sc)
                sur.synchronize()
                fa, fb = a.fields(), b.fields()
                ra, rb = read_raw(a.raw, 3), read_raw(b.raw, 3)
                same_fields = [same_bits(x, y) for x, y in zip(fa, fb)]
                ref = numpy_rows(fb, t.sdfunct)
                exact = same_bits(np.ascontiguousarray(rb[..., list(EXACT)]), np.ascontiguousarray(ref[..., list(EXACT)]))
                nan_labels = int(np.isnan(fb[3]).sum())
                print(f"{route} apply_filter={af}: raw identical to the stage by hand {same_bits(ra, rb)}, fields identical with and without the "
                      f"stage {same_fields}, counts / extrema identical to NumPy {exact}, n per row {rb[..., N_].astype(int).tolist()}, "
                      f"{nan_labels} NaN label cells")
                assert same_bits(ra, rb) and all(same_fields) and exact
                assert (rb[..., N_] == flow_of(t.sdfunct).sum()).all() and nan_labels > 100 and (rb[..., TNAN] == 0).all()
                a.free(); b.free()
        assert sur.guard_trips == 0 and sur.geometry_bound
        free(d_cols, d_sdf)


@pytest.mark.gpu
def test_gpu_host_entry_is_the_device_entry_and_survives_a_guard_trip():
    """psm_poisson_frames_errors returns the device entry's 72 doubles bit for bit (general and bound route); bound to another
    geometry it takes the guard_trips route of psm_poisson_frames -- one trip, the binding dropped -- and returns the general
    path's rows; the handle then gives the same rows again and metrics_from_sums accepts every row."""
    t = flow_tables()
    cols, lu, sc = frame_inputs()
    with surrogate_on(t) as sur:
        bind_step(sur, t)
        d_cols = DeviceArray(cols)
        rows = {}
        for route in ("general", "bound"):
            if route == "bound":
                bind_own_geometry(sur, t)
            for af in (False, True):
                b = StepBuffers(t)
                sur.poisson_frames_errors_device(d_cols.ptr, NF, 8, lu, b.extra.ptr, b.res.ptr, b.nxt.ptr, b.raw.ptr + PAD * 8, af, out_scale=sc)
                sur.synchronize()
                dev = read_raw(b.raw, 3)
                host = sur.poisson_frames_errors(cols, lu, out_scale=sc, apply_filter=af)
                print(f"{route} apply_filter={af}: host entry identical to the device entry {same_bits(host, dev)}")
                assert host.shape == (NF, 3, 8) and same_bits(host, dev)
                rows[route, af] = host
                b.free()
        one = sur.poisson_frames_errors(cols[1], lu[1:2], out_scale=sc[1:2])                      # one frame on three bound slots
        assert one.shape == (1, 3, 8) and np.array_equal(one[0, :, N_], rows["general", False][1, :, N_])
        assert sur.guard_trips == 0
        bind_other_geometry(sur, t)
        got = sur.poisson_frames_errors(cols, lu, out_scale=sc, apply_filter=True)
        print(f"bound to another geometry: guard trips {sur.guard_trips}, still bound {sur.geometry_bound}, rows identical to the general "
              f"path {same_bits(got, rows['general', True])}")
        assert sur.guard_trips == 1 and not sur.geometry_bound and "not the one bound" in _lib.last_error(sur.h)
        assert same_bits(got, rows["general", True])
        assert same_bits(sur.poisson_frames_errors(cols, lu, out_scale=sc, apply_filter=True), got) and sur.guard_trips == 1
        for row in got.reshape(-1, 8):
            m = sur.metrics_from_sums(row)
            assert all(math.isfinite(m[k]) for k in KEYS if k != "stdeNorm")
        free(d_cols)


# ------------------------------------------------------------------------------------------------------- GPU, errors
@pytest.mark.gpu
def test_gpu_error_returns_enqueue_nothing_and_leave_the_handle_usable():
    """Not planned; frames, features or post-steps unbound; weighting == 0; k < 8; misaligned d_raw; n_frames > max_cases -- and the
    stage's own argument errors: each returns its code, nothing is enqueued (outputs and d_raw keep their sentinel), and the handle
    then runs a correct call."""
    t = flow_tables()
    cols, lu, sc = frame_inputs()
    npix = t.ny * t.nx
    lib = _lib.load()
    # a handle without a plan
    cfg = _lib.psm_config(abi_version=_lib.PSM_ABI_VERSION, variant=1, block=128, c_in=4, c_out=1, p_in=8, p_out=8, n_dense=2, sdf_channel=3,
                          max_cases=NF)
    h = C.c_void_p()
    assert lib.psm_create(C.byref(cfg), C.byref(h)) == 0
    plane = _lib.psm_err_plane(4096, npix, 1, 0)
    pair = (_lib.psm_err_pair * 1)()
    pair[0].pred = pair[0].truth = plane
    raw_host = np.empty((NF, 3, 8))
    assert lib.psm_field_errors_device(h, C.byref(plane), pair, 1, 1, 4096, None) == -2 and "psm_plan_grid" in _lib.last_error(h)
    assert lib.psm_poisson_frames_errors_device(h, 4096, 1, 8, lu.ctypes.data_as(_dp), None, 0, 1, 4096, 4096, None, 4096, 4096, None) == -2
    assert lib.psm_poisson_frames_errors(h, cols.ctypes.data_as(_dp), 1, 8, lu.ctypes.data_as(_dp), None, 0, 1, raw_host.ctypes.data_as(_dp)) == -2
    lib.psm_destroy(h)
    with GridSurrogate(model4(), t.ny, t.nx, max_cases=NF) as sur:
        d_cols, d_sdf = DeviceArray(cols), DeviceArray(np.repeat(t.sdfunct[None], NF, axis=0))
        b = StepBuffers(t)
        raw_ptr = b.raw.ptr + PAD * 8
        step = lambda n=NF, k=8, raw=raw_ptr, **kw: sur.poisson_frames_errors_device(d_cols.ptr, n, k, lu[:n], b.extra.ptr, b.res.ptr, b.nxt.ptr, raw,
                                                                                False, b.chg.ptr, out_scale=sc[:n], **kw)
        host = lambda n=NF: sur.poisson_frames_errors(cols[:n], lu[:n], out_scale=sc[:n])
        c_step = lambda n, k, w, raw=raw_ptr, extra=b.extra.ptr: sur.lib.psm_poisson_frames_errors_device(
            sur.h, d_cols.ptr, n, k, lu.ctypes.data_as(_dp), None, 0, w, extra, b.res.ptr, b.chg.ptr, b.nxt.ptr, raw, None)
        c_host = lambda n, k, w: sur.lib.psm_poisson_frames_errors(sur.h, cols.ctypes.data_as(_dp), n, k, lu.ctypes.data_as(_dp), None, 0, w,
                                                                   raw_host.ctypes.data_as(_dp))
        sur.mesh_cells = t.n_cells                                                               # the mirror's own check; the library has no mesh yet
        assert "psm_set_geometry" in error(-2, step)
        assert "psm_set_geometry" in error(-2, host)
        sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        assert "psm_bind_frames" in error(-2, step)
        assert "psm_bind_frames" in error(-2, host)
        sur.bind_frames(2, 8)
        assert "psm_bind_features" in error(-2, lambda: step(2))
        sur.bind_features(np.repeat(t.sdfunct[None], NF, axis=0), 0.5, MAX_ABS)
        assert "psm_bind_poststeps" in error(-2, lambda: step(2))
        assert "psm_bind_poststeps" in error(-2, lambda: host(2))
        sur.bind_poststeps((10, 10), (50, 50))
        error(-1, step)                                                                          # three frames, two bound
        error(-1, host)
        sur.bind_frames(NF, 8)
        assert c_step(NF + 1, 8, 1) == -1 and c_host(NF + 1, 8, 1) == -1 and c_step(0, 8, 1) == -1   # n_frames outside [1, max_cases]
        assert c_step(NF, 8, 0) == -1 and "weighting" in _lib.last_error(sur.h) and c_host(NF, 8, 0) == -1
        assert c_step(NF, 7, 1) == -1 and "k >= 8" in _lib.last_error(sur.h) and c_host(NF, 7, 1) == -1 and c_step(NF, 6, 1) == -1
        assert c_step(NF, 8, 1, raw=raw_ptr + 4) == -1 and "8-byte" in _lib.last_error(sur.h)
        assert c_step(NF, 8, 1, raw=None) == -1 and c_step(NF, 8, 1, extra=None) == -1
        # the stage alone
        ok = _lib.psm_err_plane(d_sdf.ptr, npix, 1, 0)
        pred = _lib.psm_err_plane(b.nxt.ptr, npix, 1, 1)
        def c_stage(mask=ok, pred=pred, truth=ok, add=None, n_pairs=1, n_frames=NF, raw=raw_ptr):
            pr = (_lib.psm_err_pair * 4)()
            for q in range(4):
                pr[q].pred, pr[q].truth = pred, truth
                if add is not None:
                    pr[q].add = add
            return sur.lib.psm_field_errors_device(sur.h, C.byref(mask) if mask is not None else None, pr, n_pairs, n_frames, raw, None)
        bad = lambda ptr=d_sdf.ptr, fs=npix, es=1, f32=0: _lib.psm_err_plane(ptr, fs, es, f32)
        assert c_stage(mask=None) == -1 and c_stage(mask=bad(ptr=None)) == -1 and c_stage(pred=bad(ptr=None)) == -1 and c_stage(truth=bad(ptr=None)) == -1
        assert c_stage(mask=bad(ptr=d_sdf.ptr + 4)) == -1 and c_stage(pred=bad(ptr=b.nxt.ptr + 2, f32=1)) == -1 and c_stage(add=bad(ptr=d_sdf.ptr + 4)) == -1
        assert c_stage(n_pairs=0) == -1 and c_stage(n_pairs=5) == -1 and c_stage(n_frames=0) == -1 and c_stage(n_frames=NF + 1) == -1
        assert c_stage(truth=bad(fs=-1)) == -1 and c_stage(pred=bad(ptr=b.nxt.ptr, es=-1, f32=1)) == -1
        assert c_stage(raw=raw_ptr + 4) == -1 and c_stage(raw=None) == -1
        sur.synchronize()
        assert all((a == CANARY).all() for a in b.fields()) and (b.raw.numpy() == CANARY).all()   # nothing was enqueued
        # the handle still works: the step with the stage against the step and the stage by hand
        step()
        sur.synchronize()
        got, fields = read_raw(b.raw, 3), b.fields()
        a = StepBuffers(t)
        sur.poisson_frames_device(d_cols.ptr, NF, 8, lu, a.res.ptr, False, True, a.extra.ptr, a.chg.ptr, a.nxt.ptr, out_scale=sc)
        sur.field_errors_device((d_sdf.ptr, npix, 1, 0), evaluator_pairs(a, npix), NF, a.raw.ptr + PAD * 8)
        sur.synchronize()
        same = [same_bits(x, y) for x, y in zip(fields, a.fields())] + [same_bits(got, read_raw(a.raw, 3)), same_bits(host(), got)]
        print(f"after the refused calls: fields, raw and the host entry identical to the composition by hand {same}")
        assert all(same) and (got[..., N_] > 0).all()
        a.free(); b.free()
        free(d_cols, d_sdf)


# ------------------------------------------------------------------------------------------------------- GPU, the evaluator
@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("field_errors"))
    c = cases.build_dataset_case(d, poisson=True)
    c["dir"] = d
    return c


BLOCKS = (("", "delta_p"), ("_deltap_crude", "deltap_crude"), ("_p", "p"))


def compare_metrics(got, want, label):
    """One block's metrics, device sums against the host path: normVal 1e-12 relative, stdeNorm 1e-8 relative, the rest within
    1e-9 * rmseNorm / 100 absolute (percent entries: 1e-9 * rmseNorm)."""
    rmse = want["rmseNorm"]
    errs = dict(normVal=rel(got["normVal"], want["normVal"]), stdeNorm=rel(got["stdeNorm"], want["stdeNorm"]),
                biasNorm=abs(got["biasNorm"] - want["biasNorm"]) / rmse, rmseNorm=abs(got["rmseNorm"] - want["rmseNorm"]) / rmse,
                mean_err=abs(got["mean_err"] - want["mean_err"]) / (rmse / 100), mean_sq_err=abs(got["mean_sq_err"] - want["mean_sq_err"]) / (rmse / 100))
    print(f"{label}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + " (bounds 1e-12, 1e-8, then 1e-9 of rmseNorm / 100)")
    assert errs["normVal"] <= 1e-12 and errs["stdeNorm"] <= 1e-8
    assert all(errs[k] <= 1e-9 for k in ("biasNorm", "rmseNorm", "mean_err", "mean_sq_err"))


@pytest.mark.gpu
def test_gpu_evaluator_metrics_only_sweep(ds):
    """timeSteps(..., fields=False) against timeSteps(...) on the dataset's three frames: the six lists agree entry by entry within
    1e-9 * rmseNorm / 100 (the reordered sums and the 4-ulp truth chain), normVal within 1e-12, stdeNorm within 1e-8 relative --
    on frames whose host-path |bias| < 0.5 * rmse in all three blocks, checked first; the return is one {suffix: metrics} dict per
    frame, the field attributes are None; an irrelevant frame returns 0; call_SM_main_Poisson(frames_per_call=3, fields=False)
    gives the summaries of the default call within the same bounds."""
    host, dev = evaluator(ds, max_frames=NF), evaluator(ds, max_frames=NF)
    assert host.computeOnlyOnce(0) == 0 and dev.computeOnlyOnce(0) == 0
    seen, inner = [], host._record_metrics                    # every block's full metrics of the host path, in frame order
    host._record_metrics = lambda m, suffix="", title=None: (seen.append((suffix, dict(m))), inner(m, suffix, title))[1]
    fields = host.timeSteps(0, [0, 1, 2], False, PHI)
    assert len(fields) == 3 and [sfx for sfx, _ in seen] == [sfx for sfx, _ in BLOCKS] * 3
    per_frame = [{key: seen[3 * i + q][1] for q, (_, key) in enumerate(BLOCKS)} for i in range(3)]
    for i in range(3):
        for key, m in per_frame[i].items():
            print(f"host path frame {i} {key}: |bias| / rmse = {abs(m['biasNorm']) / m['rmseNorm']:.3f}")
            assert abs(m["biasNorm"]) < 0.5 * m["rmseNorm"], "the comparison needs a well conditioned stde"
    out = dev.timeSteps(0, [0, 1, 2], False, PHI, fields=False)
    assert len(out) == 3 and all(isinstance(o, dict) and set(o) == {"", "_deltap_crude", "_p"} for o in out)
    assert dev.deltap_res is None and dev.cfd_results is None and dev.p_pred is None and dev.label_planes is None
    assert dev._sur.geometry_bound and dev._sur.guard_trips == 0
    for i in range(3):
        for sfx, key in BLOCKS:
            compare_metrics(out[i][sfx], per_frame[i][key], f"frame {i} block '{key}'")
    for sfx, key in BLOCKS:
        for name in ("pred_minus_true" + sfx, "pred_minus_true_squared" + sfx):
            a, b = getattr(dev, name), getattr(host, name)
            assert len(a) == len(b) == 3
            for i in range(3):
                assert abs(a[i] - b[i]) <= 1e-9 * per_frame[i][key]["rmseNorm"] / 100, (name, i, a[i], b[i])
    assert dev.last_metrics.keys() == host.last_metrics.keys() and dev.last_metrics["p"] == out[2]["_p"] and dev.U_max_norm == host.U_max_norm
    # a middle frame whose velocity hardly changed
    import h5write
    from psm_amd import formats
    sim2 = ds["sim"].copy()
    sim2[0, 1, :ds["N"], 5:7] *= 1e-7
    p2 = os.path.join(ds["dir"], "still.hdf5")
    tb, ob = formats.read_dataset(ds["dataset_path"], 0, 0)[1:]
    h5write.write_h5(p2, {"sim_data": sim2, "top_bound": np.repeat(tb, 3, axis=1), "obst_bound": np.repeat(ob, 3, axis=1)})
    dev.dataset_path = p2
    again = dev.timeSteps(0, [0, 1, 2], False, PHI, fields=False)
    assert isinstance(again[1], int) and again[1] == 0 and len(dev.pred_minus_true) == 5 and set(again[0]) == set(again[2]) == {"", "_deltap_crude", "_p"}
    # the main
    phis = os.path.join(ds["dir"], "phis.txt")
    np.savetxt(phis, np.array([PHI, 0.2]))
    args = (5e-3, ds["model_path"], 128, 0.25, 0.95, 0.95, 128, ds["dataset_path"], False, "std", 0.5, False, False, False, False, 1, 3, phis)
    kw = dict(artifact_dir=ds["dir"], sim_offset=0, time_offset=0)
    want = call_SM_main_Poisson(*args, frames_per_call=3, **kw)
    got = call_SM_main_Poisson(*args, frames_per_call=3, fields=False, **kw)
    assert set(got) == set(want) and set(got["overall"]) == set(want["overall"]) and got["sims"][0]["sim"] == 0 and got["sims"][0]["phi"] == PHI
    worst = 0.0
    for blk in ("delta_p", "delta_p_no_weighting", "p"):
        for where_g, where_w in ((got["overall"], want["overall"]), (got["sims"][0], want["sims"][0])):
            if blk not in where_w:
                continue
            g, w = where_g[blk], where_w[blk]
            worst = max(worst, abs(g["BIAS"] - w["BIAS"]) / w["RMSE"], abs(g["RMSE"] - w["RMSE"]) / w["RMSE"], rel(g["STDE"], w["STDE"]) / 10)
    print(f"call_SM_main_Poisson(frames_per_call=3, fields=False) against fields=True: worst BIAS / RMSE difference {worst:.2e} of RMSE "
          f"(bound 1e-9; STDE 1e-8 relative)\n  got  {got['overall']}\n  want {want['overall']}")
    assert worst <= 1e-9
