"""The frame batch of the pressureSM_deltas evaluator on the device (psm_bind_deltas_frames, psm_deltas_image_device,
psm_block_errors_device, psm_deltas_frames_device / psm_deltas_frames) and Evaluation.timeSteps / call_SM_main(frames_per_call,
fields) on top of them.

Stage tests run on the 130 x 131 grid of tests/test_field_errors.py (17 030 pixels: 16 pack workgroups of 1024 pixels + 646, the last
vector of four cut to two; four 128 x 128 blocks that overlap in both directions) with its 200-cell mesh, its rectangle of SDF zeros
and the NaN label cells of its frame columns; max_cases = 3.  An image frame is 204 360 bytes and a label frame 68 120, both
8 (mod 16): of three frames behind a lead of 4 elements frames 0 and 2 start 16-byte aligned and frame 1 does not, behind a lead of 5
none does; the truth frames (136 240 bytes) are all aligned behind a lead of 4 and none behind 5.

References: the NumPy statements of Evaluation.timeStep on the planes psm_frames_to_grid_device wrote (bit for bit); NumPy on the
decoded blocks psm_read_stage returns and the label blocks psm_label_blocks returns -- counts and extrema bit for bit, the two sums
against math.fsum within test_field_errors.SUM_TOL --; psm_block_error, psm_field_errors_device and three timeStep calls.
Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
from hipmem import DeviceArray
from psm_amd import Evaluation, GridSurrogate, _lib, call_SM_main, synthetic
from psm_amd.surrogate import layout
from test_field_errors import (CANARY, EXACT, KEYS, N_, NF, NPIX, NX, NY, PAD, PMAX, PMIN, S1, S2, SUM_TOL, TMAX, TMIN, TNAN, compare_metrics,
                               differences, flow_tables, frame_inputs, np_raw)
from test_poisson_frames import same_bits
from test_poisson_step_device import error, free, model4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc")
NEW_ENTRIES = ("psm_bind_deltas_frames", "psm_unbind_deltas_frames", "psm_deltas_image_device", "psm_block_errors_device",
               "psm_deltas_frames_device", "psm_deltas_frames")
NEW_METHODS = ("bind_deltas_frames", "unbind_deltas_frames", "deltas_image_device", "block_errors_device", "deltas_frames_device", "deltas_frames")
MAXS = cases.DATASET_MAXS                      # max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


@functools.lru_cache(maxsize=None)
def model3():
    m = synthetic.make_model("deltas", p_in=48, p_out=40, c_in=3, seed_pca=778, seed_w=6)
    m.sdf_ch = 2
    return m


@functools.lru_cache(maxsize=None)
def stage_inputs():
    """(cols [NF][200][3], raw SDF plane with NaNs, U2 [NF], out_scale [NF]): columns (dUx, dUy, delta_p) of test_field_errors'
    frames, so the label column carries its NaN cells; the SDF keeps the rectangle of zeros and gets a NaN strip of its own."""
    cols8, lu, _ = frame_inputs()
    cols = np.ascontiguousarray(cols8[..., 2:5])
    assert np.isnan(cols[..., 2]).sum() == 4 and not np.isnan(cols[..., :2]).any()
    sdf = flow_tables().sdfunct.copy()
    sdf[3, 5:60] = np.nan
    u2 = [float(pow(np.float32(u), 2.0)) for u in lu[:, 1]]
    return cols, sdf, u2, [MAXS[3] * np.float32(u) ** 2 for u in lu[:, 1]]


def surrogate3(bind=True, post=False):
    t = flow_tables()
    sur = GridSurrogate(model3(), t.ny, t.nx, max_cases=NF)
    sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
    if bind:
        sur.bind_frames(NF, 3)
        sur.bind_deltas_frames(stage_inputs()[1], MAXS)
    if post:
        sur.bind_poststeps((10, 10), (50, 50))
    return sur


def host_statements(planes, sdf, u2):
    """What Evaluation.timeStep does with the planes of one frame [3][NY][NX]: (image float32 [NY,NX,3], label float32, truth)."""
    grid = np.zeros((NY, NX, 5))
    grid[..., 0:2] = np.moveaxis(planes[0:2], 0, 2)
    grid[..., 2] = sdf
    grid[..., 3] = planes[2]
    grid[np.isnan(grid)] = 0                                                        # SM_call.py:439
    grid[..., 0] /= MAXS[0]; grid[..., 1] /= MAXS[1]                                # :442-445
    grid[..., 2] /= MAXS[2]; grid[..., 3] /= MAXS[3]
    return (np.ascontiguousarray(grid[..., :3], np.float32), np.ascontiguousarray(grid[..., 3], np.float32),
            grid[..., 3] * MAXS[3] * u2)                                              # GridSurrogate.solve's cast; :580


def device_planes(sur, d_cols):
    d_pl = DeviceArray(np.full((NF, 3, NPIX), CANARY, np.float64))
    sur.frames_to_grid_device(d_cols.ptr, NF, 3, [(d_pl.ptr + c * NPIX * 8, 3 * NPIX, False) for c in range(3)])
    sur.synchronize()
    planes = d_pl.numpy().reshape(NF, 3, NY, NX)
    d_pl.free()
    return planes


def device_image(sur, d_cols, u2):
    """The stage's three outputs in dense buffers -> (d_grid, d_label, image, label, truth)."""
    d_grid, d_label = DeviceArray(shape=(NF, NY, NX, 3)), DeviceArray(shape=(NF, NPIX))
    d_truth = DeviceArray(shape=(NF, NPIX), dtype=np.float64)
    sur.deltas_image_device(d_cols.ptr, NF, 3, u2, d_grid.ptr, d_label.ptr, d_truth.ptr)
    sur.synchronize()
    out = d_grid, d_label, d_grid.numpy(), d_label.numpy().reshape(NF, NY, NX), d_truth.numpy().reshape(NF, NY, NX)
    d_truth.free()
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_entries_are_declared_bound_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+PSM_ABI_VERSION\s+4\b", txt) and _lib.PSM_ABI_VERSION == 4
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert inspect.signature(Evaluation.__init__).parameters["max_frames"].default is None and Evaluation.max_frames == 1
    assert inspect.signature(Evaluation.timeSteps).parameters["fields"].default is True
    sig = inspect.signature(call_SM_main).parameters
    assert sig["frames_per_call"].default == 1 and sig["fields"].default is True


def test_python_argument_checks_come_before_any_library_call():
    """The new mirrors refuse bad arguments on a surrogate whose library and handle do not exist: any call into the library would
    raise AttributeError instead."""
    sur = GridSurrogate.__new__(GridSurrogate)
    sur.lib = sur.h = None
    sur.ny, sur.nx, sur.model, sur.mesh_cells, sur.max_cases = 6, 7, model3(), 11, 3
    sdf = np.ones((6, 7))
    with pytest.raises(RuntimeError, match="bind_frames"):
        sur.bind_deltas_frames(sdf, MAXS)
    sur._frames_bound = True
    with pytest.raises(ValueError, match=r"\[6,7\]"):
        sur.bind_deltas_frames(np.ones((6, 8)), MAXS)
    for bad in ((1.0, 1.0, 0.0, 1.0), (1.0, np.inf, 1.0, 1.0), (np.nan, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="four finite non-zero"):
            sur.bind_deltas_frames(sdf, bad)
    four = GridSurrogate.__new__(GridSurrogate)
    four.lib = four.h = None
    four.ny, four.nx, four.model, four._frames_bound = 6, 7, model4(), True
    with pytest.raises(ValueError, match="3 input channels"):
        four.bind_deltas_frames(sdf, MAXS)
    u2 = [1.0, 2.0]
    with pytest.raises(RuntimeError, match="bind_deltas_frames"):
        sur.deltas_frames_device(4096, 2, 3, u2)
    with pytest.raises(RuntimeError, match="bind_deltas_frames"):
        sur.block_errors_device(4096, 4096, 2, 4096)
    sur._deltas_bound = True
    step = lambda **kw: sur.deltas_frames_device(**{**dict(d_cols=4096, n_frames=2, k=3, U2=u2, d_result=4096, d_truth=4096, d_raw=4096), **kw})
    image = lambda **kw: sur.deltas_image_device(**{**dict(d_cols=4096, n_frames=2, k=3, U2=u2, d_grid=4096, d_label=4096, d_truth=4096), **kw})
    for call in (step, image):
        for k in (2, 17):
            with pytest.raises(ValueError, match="3..16 columns"):
                call(k=k)
        for n in (0, 4):
            with pytest.raises(ValueError, match="n_frames"):
                call(n_frames=n)
        with pytest.raises(ValueError, match="U2"):
            call(U2=[1.0])
        with pytest.raises(ValueError, match="U2"):
            call(U2=[1.0, np.nan])
        with pytest.raises(ValueError, match="d_cols"):
            call(d_cols=0)
        with pytest.raises(ValueError, match="d_truth"):
            call(d_truth=4100)
    with pytest.raises(ValueError, match="U2"):
        step(U2=None)
    with pytest.raises(ValueError, match="U2"):
        image(U2=None)                                       # a truth plane needs it
    with pytest.raises(ValueError, match="d_raw"):
        step(d_raw=4100)
    with pytest.raises(ValueError, match="d_result"):
        step(d_result=4098)
    with pytest.raises(ValueError, match="out_scale"):
        step(out_scale=[1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="bind_poststeps"):
        step(apply_filter=True)
    with pytest.raises(ValueError, match="d_grid"):
        image(d_grid=0)
    with pytest.raises(ValueError, match="d_label"):
        image(d_label=4098)
    for n in (0, 4):
        with pytest.raises(ValueError, match="n_frames"):
            sur.block_errors_device(4096, 4096, n, 4096)
    for name, bad in (("d_grid", 0), ("d_label", 4098), ("d_raw", 4100), ("d_raw", 0)):
        with pytest.raises(ValueError, match=name):
            sur.block_errors_device(**{**dict(d_grid=4096, d_label=4096, n_frames=2, d_raw=4096), name: bad})
    ok = np.zeros((2, 11, 3))
    with pytest.raises(ValueError, match="3..16 columns"):
        sur.deltas_frames(ok[..., :2], u2)
    with pytest.raises(ValueError, match=r"\[n,n_cells,k\]"):
        sur.deltas_frames(np.zeros((2, 3, 11, 3)), u2)
    with pytest.raises(ValueError, match="11 cells"):
        sur.deltas_frames(np.zeros((2, 12, 3)), u2)
    with pytest.raises(ValueError, match="U2"):
        sur.deltas_frames(ok, u2[:1])
    with pytest.raises(ValueError, match="out_scale"):
        sur.deltas_frames(ok, u2, out_scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="nothing to return"):
        sur.deltas_frames(ok, u2, want_result=False, want_truth=False, want_raw=False)
    with pytest.raises(RuntimeError, match="bind_poststeps"):
        sur.deltas_frames(ok, u2, apply_filter=True)
    sur.mesh_cells = None
    with pytest.raises(RuntimeError, match="no mesh"):
        sur.deltas_frames(ok, u2)
    with pytest.raises(ValueError, match="max_frames"):
        Evaluation(5e-3, 128, 32, 0.95, 0.95, "no.hdf5", "no.h5", 128, "std", model=model3(), max_frames=0)
    ev = Evaluation(5e-3, 128, 32, 0.95, 0.95, "no.hdf5", "no.h5", 128, "std", model=model3(), max_frames=2)
    assert ev.max_frames == 2 and Evaluation.max_frames == 1
    with pytest.raises(RuntimeError, match="computeOnlyOnce"):
        ev.timeSteps(0, [0, 1], fields=False)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_arithmetic_is_clean_under_asan_ubsan(tmp_path):
    """csrc/psm_errors.cpp -- the host-only piece behind every raw row the new entries return -- in a stand-alone program
    (tests/native/deltas_frames_sanitized.cpp) under AddressSanitizer + UBSan: block rows with n == 0, a NaN truth and a variance
    that rounds below zero."""
    exe = str(tmp_path / "deltas_frames_sanitized")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "deltas_frames_sanitized.cpp"), os.path.join(CSRC, "psm_errors.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "rows checked:" in r.stdout


# ------------------------------------------------------------------------------------------------------- GPU, the pack
@pytest.mark.gpu
def test_gpu_pack_is_the_host_statements_bit_for_bit():
    """Image, label and truth of psm_deltas_image_device against timeStep's NumPy statements on the planes
    psm_frames_to_grid_device wrote: bit for bit, for 1 and 3 frames, behind leads of 4 and 5 elements (frames that start 16-byte
    aligned and frames that do not), with canaries in front of, behind and -- for one frame -- instead of the other frames."""
    cols, sdf, u2, _ = stage_inputs()
    with surrogate3() as sur:
        d_cols = DeviceArray(cols)
        planes = device_planes(sur, d_cols)
        assert np.isnan(planes[:, 2]).sum() > 100 and not np.isnan(planes[:, :2]).any()
        want = [host_statements(planes[f], sdf, u2[f]) for f in range(NF)]
        assert (want[0][0][..., 2] == 0).sum() >= 35 * 40 + 55 and all(np.isfinite(w[2]).all() for w in want)
        sizes, dtypes = (NPIX * 3, NPIX, NPIX), (np.float32, np.float32, np.float64)
        starts = set()
        for lead in (4, 5):
            for n in (1, NF):
                bufs = [DeviceArray(np.full(lead + NF * s + PAD, CANARY, dt)) for s, dt in zip(sizes, dtypes)]
                ptrs = [b.ptr + lead * np.dtype(dt).itemsize for b, dt in zip(bufs, dtypes)]
                starts |= {(p + f * s * np.dtype(dt).itemsize) % 16 == 0 for p, s, dt in zip(ptrs, sizes, dtypes) for f in range(n)}
                sur.deltas_image_device(d_cols.ptr, n, 3, u2[:n], *ptrs)
                sur.synchronize()
                same = []
                for q, (b, s) in enumerate(zip(bufs, sizes)):
                    a = b.numpy()
                    assert (a[:lead] == CANARY).all() and (a[lead + n * s:] == CANARY).all(), ("canary", lead, n, q)
                    got = a[lead:lead + n * s].reshape((n,) + want[0][q].shape)
                    same.append(all(same_bits(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f][q])) for f in range(n)))
                print(f"lead {lead}, {n} frame(s): image / label / truth identical to the host statements {same}")
                assert all(same)
                free(*bufs)
        assert starts == {False, True}, "the frames must start both 16-byte aligned and not"
        # the label and truth planes are optional
        d_g = DeviceArray(np.full((NF, NY, NX, 3), CANARY, np.float32))
        sur.deltas_image_device(d_cols.ptr, NF, 3, None, d_g.ptr)
        sur.synchronize()
        assert all(same_bits(d_g.numpy()[f], want[f][0]) for f in range(NF))
        free(d_cols, d_g)


# ------------------------------------------------------------------------------------------------------- GPU, the block stage
def block_rows(sur, image, label, sc, pred, n):
    """compute_in_block_error's eight sums per frame in NumPy: the decoded blocks `pred` [n * B][S][S] against psm_label_blocks of
    the frame times the float32 row scale, over the flow cells of the image's blocks -> (raw [n][8], {f: (fsum d, sum |d|, fsum d^2)})."""
    S = sur.model.S
    blocks = layout("deltas", NY, NX, S, sur.model.ov or 0)[0]
    assert [tuple(b[:2]) for b in blocks] == [(0, 3), (0, 0), (2, 3), (2, 0)]
    B = len(blocks)
    raw, sums = np.empty((n, 8)), {}
    for f in range(n):
        lb = sur.label_blocks(image[f], label[f])[..., 0].astype(np.float64) * np.float64(np.float32(sc[f]))
        flow = np.stack([image[f, y0:y0 + S, x0:x0 + S, 2] != 0 for y0, x0 in blocks[:, :2]])
        pr = pred[f * B:(f + 1) * B].reshape(B, S, S)
        raw[f] = np_raw(pr, lb, flow)
        d = differences(pr, lb, flow)[2]
        sums[f] = (math.fsum(d), math.fsum(np.abs(d)), math.fsum(d * d))
    return raw, sums


def check_block_rows(got, want, sums, label):
    worst1 = worst2 = 0.0
    for f, (s1, sabs, s2) in sums.items():
        g, w = got[f], want[f]
        assert same_bits(np.ascontiguousarray(g[list(EXACT)]), np.ascontiguousarray(w[list(EXACT)])), (label, f, g, w)
        e1, e2 = abs(g[S1] - s1), abs(g[S2] - s2)
        worst1, worst2 = max(worst1, e1 / sabs), max(worst2, e2 / g[S2])
        assert e1 <= SUM_TOL * sabs and e2 <= SUM_TOL * g[S2], (label, f, e1, sabs, e2, g[S2])
    return worst1, worst2


def raw_buffer(rows):
    return DeviceArray(np.full(PAD + NF * rows * 8 + PAD, CANARY, np.float64))


def read_raw(d_raw, rows, n=NF):
    a = d_raw.numpy()
    assert (a[:PAD] == CANARY).all() and (a[PAD + n * rows * 8:] == CANARY).all(), "canary round d_raw"
    return a[PAD:PAD + n * rows * 8].reshape(n, rows, 8).copy()


@pytest.mark.gpu
def test_gpu_block_stage_alone():
    """psm_block_errors_device after a device solve of three frames, general and bound route, against NumPy on the decoded blocks
    and psm_label_blocks * row scale: n, tnan and the four extrema bit for bit, s1 and s2 within SUM_TOL of math.fsum; a second call
    gives the same bits; on the general route one frame's metrics_from_sums are psm_block_error's out[0], out[1], out[2], out[4]."""
    cols, sdf, u2, sc = stage_inputs()
    with surrogate3() as sur:
        d_cols = DeviceArray(cols)
        d_grid, d_label, image, label, _ = device_image(sur, d_cols, u2)
        d_fields = DeviceArray(shape=(NF, NY, NX, 1))
        nan_labels = int(np.isnan(device_planes(sur, d_cols)[:, 2]).sum())
        for route in ("general", "bound"):
            if route == "bound":
                assert sur.bind_geometry(image) and sur.geometry_bound
            d_raw = raw_buffer(1)
            sur.solve_device(d_grid.ptr, NF, d_fields.ptr, out_scale=sc)
            sur.block_errors_device(d_grid.ptr, d_label.ptr, NF, d_raw.ptr + PAD * 8)
            sur.synchronize()
            got = read_raw(d_raw, 1)[:, 0]
            pred = sur.stage("block_pred", NF)
            want, sums = block_rows(sur, image, label, sc, pred, NF)
            w1, w2 = check_block_rows(got, want, sums, route)
            sur.block_errors_device(d_grid.ptr, d_label.ptr, NF, d_raw.ptr + PAD * 8)
            sur.synchronize()
            again = read_raw(d_raw, 1)[:, 0]
            print(f"{route}: 3 rows, counts and extrema identical to NumPy, |s1 - fsum| / sum|d| <= {w1:.2e}, |s2 - fsum| / s2 <= {w2:.2e} "
                  f"(bound {SUM_TOL}); second call identical {same_bits(got, again)}; n per frame {got[:, N_].astype(int).tolist()}, "
                  f"{nan_labels} NaN label cells went in as 0")
            assert same_bits(got, again) and (got[:, TNAN] == 0).all() and (got[:, N_] > 30000).all()
            assert sur.guard_trips == 0 and (route == "general" or sur.geometry_bound)
            if route == "general":
                # two frames of the three-case solve: the first two rows, nothing behind them
                d_two = raw_buffer(1)
                sur.block_errors_device(d_grid.ptr, d_label.ptr, 2, d_two.ptr + PAD * 8)
                sur.synchronize()
                assert same_bits(read_raw(d_two, 1, 2)[:, 0], got[:2])
                # one frame through the host entries: psm_block_error's host sums against the fold launch
                for f in (0, 2):
                    sur.solve(image[f], out_scale=[sc[f]])
                    m = sur.block_error(image[f], label[f])
                    d_one = raw_buffer(1)
                    sur.block_errors_device(d_grid.ptr + f * NPIX * 12, d_label.ptr + f * NPIX * 4, 1, d_one.ptr + PAD * 8)
                    sur.synchronize()
                    one = read_raw(d_one, 1, 1)[0, 0]
                    d_one.free()
                    mm = sur.metrics_from_sums(one)
                    same = [mm["mean_err"] == m["mean_err"], mm["mean_sq_err"] == m["mean_sq_err"], mm["normVal"] == m["normVal"], int(one[N_]) == m["n"],
                            one[PMAX] - one[PMIN] == m["norm_pred"]]
                    print(f"frame {f} alone: mean_err, mean_sq_err, normVal, n, norm_pred identical to psm_block_error {same}; the row is the "
                          f"batch's row {same_bits(one, got[f])}")
                    assert all(same)
                d_two.free()
            d_raw.free()
        free(d_cols, d_grid, d_label, d_fields)


# ------------------------------------------------------------------------------------------------------- GPU, the whole step
class StepOut:
    def __init__(self):
        self.res = DeviceArray(np.full(PAD + NF * NPIX + PAD, CANARY, np.float32))
        self.truth = DeviceArray(np.full(PAD + 1 + NF * NPIX + PAD, CANARY, np.float64))
        self.raw = raw_buffer(2)
        self.p_res, self.p_truth, self.p_raw = self.res.ptr + PAD * 4, self.truth.ptr + (PAD + 1) * 8, self.raw.ptr + PAD * 8

    def read(self, n=NF):
        r, t = self.res.numpy(), self.truth.numpy()
        assert (r[:PAD] == CANARY).all() and (r[PAD + n * NPIX:] == CANARY).all() and (t[:PAD + 1] == CANARY).all() and (t[PAD + 1 + n * NPIX:] == CANARY).all()
        return r[PAD:PAD + n * NPIX].reshape(n, NY, NX).copy(), t[PAD + 1:PAD + 1 + n * NPIX].reshape(n, NY, NX).copy(), read_raw(self.raw, 2, n)

    def untouched(self):
        return all((d.numpy() == CANARY).all() for d in (self.res, self.truth, self.raw))

    def free(self):
        free(self.res, self.truth, self.raw)


def bind_other_geometry(sur, sdf):
    g = np.zeros((NY, NX, 3), np.float32)                                          # the step solves its frames one by one: one case
    sd = np.roll(np.nan_to_num(sdf, nan=0.0), 11, axis=1) / MAXS[2]
    g[..., 2] = sd.astype(np.float32)
    assert sur.bind_geometry(g) and sur.geometry_bound


@pytest.mark.gpu
def test_gpu_whole_step():
    """psm_deltas_frames_device, general and bound route, with and without the filter: row 0 is psm_field_errors_device on the
    step's own result and truth planes, row 1 is psm_block_errors_device alone, the truth plane is the pack's, the host entry returns
    the device entry's bits; apply_filter changes the result and row 0 and not row 1; bound to another geometry the host entry takes
    one guard trip and returns the unbound run."""
    cols, sdf, u2, sc = stage_inputs()
    with surrogate3(post=True) as sur:
        d_cols = DeviceArray(cols)
        d_grid, d_label, image, label, truth = device_image(sur, d_cols, u2)
        d_sdn = DeviceArray(np.nan_to_num(sdf, nan=0.0) / MAXS[2])
        flow = int(((np.nan_to_num(sdf, nan=0.0) / MAXS[2]) != 0).sum())
        kept = {}
        for route in ("general", "bound"):
            if route == "bound":
                assert sur.bind_geometry(image[0]) and sur.geometry_bound               # every frame carries the simulation's SDF channel
            for af in (False, True):
                o = StepOut()
                sur.deltas_frames_device(d_cols.ptr, NF, 3, u2, o.p_res, o.p_truth, o.p_raw, af, out_scale=sc)
                d_f, d_b = raw_buffer(1), raw_buffer(1)
                sur.field_errors_device((d_sdn.ptr, 0, 1, 0), [((o.p_res, NPIX, 1, 1), (o.p_truth, NPIX, 1, 0), None, None, False)], NF, d_f.ptr + PAD * 8)
                sur.block_errors_device(d_grid.ptr, d_label.ptr, NF, d_b.ptr + PAD * 8)
                sur.synchronize()
                res, tr, raw = o.read()
                rf, rb = read_raw(d_f, 1)[:, 0], read_raw(d_b, 1)[:, 0]
                h_res, h_tr, h_raw = sur.deltas_frames(cols, u2, out_scale=sc, apply_filter=af)
                same = dict(row0=same_bits(np.ascontiguousarray(raw[:, 0]), rf), row1=same_bits(np.ascontiguousarray(raw[:, 1]), rb),
                            truth=same_bits(tr, truth), host_result=same_bits(h_res, res), host_truth=same_bits(h_tr, tr), host_raw=same_bits(h_raw, raw))
                print(f"{route} apply_filter={af}: {same}; n per row {raw[..., N_].astype(int).tolist()}, flow cells {flow}")
                assert all(same.values()) and np.isfinite(res).all()
                assert (raw[:, 0, N_] == flow).all() and (raw[..., TNAN] == 0).all()
                only = sur.deltas_frames(cols, u2, out_scale=sc, apply_filter=af, want_result=False, want_truth=False)
                assert only[0] is None and only[1] is None and same_bits(only[2], raw)
                kept[route, af] = (res, raw)
                free(d_f, d_b)
                o.free()
            (r0, w0), (r1, w1) = kept[route, False], kept[route, True]
            assert not np.array_equal(r0, r1) and not np.array_equal(w0[:, 0], w1[:, 0]) and same_bits(np.ascontiguousarray(w0[:, 1]), np.ascontiguousarray(w1[:, 1]))
        one = sur.deltas_frames(cols[1], u2[1:2], out_scale=sc[1:2])                                   # one frame alone
        assert one[0].shape == (1, NY, NX) and np.array_equal(one[2][0, :, N_], kept["general", False][1][1, :, N_])
        assert sur.guard_trips == 0 and sur.geometry_bound
        bind_other_geometry(sur, sdf)
        got = sur.deltas_frames(cols, u2, out_scale=sc, apply_filter=True)
        print(f"bound to another geometry: guard trips {sur.guard_trips}, still bound {sur.geometry_bound}, result and rows identical to the "
              f"general path {same_bits(got[0], kept['general', True][0])} {same_bits(got[2], kept['general', True][1])}")
        assert sur.guard_trips == 1 and not sur.geometry_bound and "not the one bound" in _lib.last_error(sur.h)
        assert same_bits(got[0], kept["general", True][0]) and same_bits(got[2], kept["general", True][1])
        for row in got[2].reshape(-1, 8):
            m = sur.metrics_from_sums(row)
            assert all(math.isfinite(m[k]) for k in KEYS if k != "stdeNorm")
        free(d_cols, d_grid, d_label, d_sdn)


# ------------------------------------------------------------------------------------------------------- GPU, errors
@pytest.mark.gpu
def test_gpu_error_returns_enqueue_nothing_and_leave_the_handle_usable():
    """Frames, deltas frames or post-steps unbound; a four-channel model; bad scales; k = 2; n_frames 0 and 4; a misaligned d_raw; a
    ring solve in front of the block stage: each returns its code, the outputs keep their sentinels, and the handle then runs a
    correct call."""
    cols, sdf, u2, sc = stage_inputs()
    t = flow_tables()
    u2a, sca, mx = np.array(u2), np.array(sc, np.float32), np.array(MAXS, np.float64)
    sdf_c = np.ascontiguousarray(sdf)
    with GridSurrogate(model4(), NY, NX, max_cases=NF) as four:
        four.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        four.bind_frames(NF, 3)
        assert four.lib.psm_bind_deltas_frames(four.h, sdf_c.ctypes.data_as(_dp), mx.ctypes.data_as(_dp)) == -2 and "c_in == 3" in _lib.last_error(four.h)
    with surrogate3(bind=False) as sur:
        d_cols = DeviceArray(cols)
        o = StepOut()
        d_grid, d_label = DeviceArray(np.full((NF, NY, NX, 3), CANARY, np.float32)), DeviceArray(np.full((NF, NPIX), CANARY, np.float32))
        lib, h = sur.lib, sur.h
        c_bind = lambda m=mx, s=sdf_c: lib.psm_bind_deltas_frames(h, s.ctypes.data_as(_dp) if s is not None else None, m.ctypes.data_as(_dp))
        c_step = lambda n=NF, k=3, af=0, raw=o.p_raw, u=u2a: lib.psm_deltas_frames_device(h, d_cols.ptr, n, k, u.ctypes.data_as(_dp) if u is not None else None,
                                                                                    sca.ctypes.data_as(_fp), af, o.p_res, o.p_truth, raw, None)
        c_image = lambda n=NF, k=3, grid=d_grid.ptr: lib.psm_deltas_image_device(h, d_cols.ptr, n, k, u2a.ctypes.data_as(_dp), grid, d_label.ptr, o.p_truth, None)
        c_block = lambda n=NF, raw=o.p_raw: lib.psm_block_errors_device(h, d_grid.ptr, d_label.ptr, n, raw, None)
        host_raw = np.full((NF, 2, 8), CANARY)
        c_host = lambda n=NF, k=3, af=0: lib.psm_deltas_frames(h, cols.ctypes.data_as(_dp), n, k, u2a.ctypes.data_as(_dp), sca.ctypes.data_as(_fp), af, None, None,
                                                               host_raw.ctypes.data_as(_dp))
        last = lambda: _lib.last_error(h)
        assert c_bind() == -2 and "psm_bind_frames" in last()
        assert c_step() == -2 and "psm_bind_frames" in last() and c_image() == -2 and c_block() == -2 and c_host() == -2
        sur.bind_frames(NF, 3)
        assert c_step() == -2 and "psm_bind_deltas_frames" in last() and c_image() == -2 and c_host() == -2
        assert c_block() == -2 and "psm_bind_deltas_frames" in last()
        for bad in ((1.0, 1.0, 0.0, 1.0), (np.inf, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, np.nan)):
            assert c_bind(m=np.array(bad)) == -1 and "finite and non-zero" in last()
        assert c_bind(s=None) == -1 and c_step() == -2
        assert c_bind() == 0
        sur._deltas_bound = True                                                  # bound through the C entry: tell the mirror
        assert c_block() == -2 and "no solve" in last()
        assert c_step(af=1) == -2 and "psm_bind_poststeps" in last() and c_host(af=1) == -2 and "psm_bind_poststeps" in last()
        assert c_step(k=2) == -1 and "[3, 16]" in last() and c_image(k=2) == -1 and c_host(k=2) == -1 and c_step(k=17) == -1
        for n in (0, NF + 1):
            assert c_step(n=n) == -1 and "n_frames" in last() and c_image(n=n) == -1 and c_host(n=n) == -1 and c_block(n=n) == -1
        assert c_step(raw=o.p_raw + 4) == -1 and "d_raw" in last() and c_block(raw=o.p_raw + 4) == -1 and "8-byte" in last()
        assert c_step(u=None) == -1 and c_image(grid=None) == -1 and c_image(grid=d_grid.ptr + 2) == -1 and c_block(raw=None) == -1
        assert c_host(k=4) == -1 and "reserved staging" in last()
        sur.synchronize()
        assert o.untouched() and (d_grid.numpy() == CANARY).all() and (d_label.numpy() == CANARY).all() and (host_raw == CANARY).all()
        # a ring solve in front of the block stage
        assert c_image() == 0
        d_fields = DeviceArray(shape=(NF, NY, NX, 1))
        sur.solve_device(d_grid.ptr, NF, d_fields.ptr, out_scale=sc)
        sur.synchronize()
        image = d_grid.numpy()
        sur.wait(sur.submit(image[0], out_scale=[sc[0]]))
        assert c_block() == -2 and "ring" in last()
        sur.solve_device(d_grid.ptr, 2, d_fields.ptr, out_scale=sc[:2])
        assert c_block() == -2 and "fewer cases" in last() and c_block(n=2) == 0
        sur.synchronize()
        assert (read_raw(o.raw, 2, 1)[0, :, N_] > 0).all()                      # [2][8] of the stage alone fill the first frame's two rows
        # the handle still works: device entry against the host entry
        assert c_step() == 0
        sur.synchronize()
        res, tr, raw = o.read()
        h_res, h_tr, h_raw = sur.deltas_frames(cols, u2, out_scale=sc)
        same = [same_bits(h_res, res), same_bits(h_tr, tr), same_bits(h_raw, raw)]
        print(f"after the refused calls: result, truth and raw of the device and the host entry identical {same}")
        assert all(same) and (raw[..., N_] > 0).all()
        sur.unbind_deltas_frames()
        assert c_step() == -2 and "psm_bind_deltas_frames" in last()
        sur.bind_deltas_frames(sdf, MAXS)
        sur.bind_frames(NF, 3)                                                   # a new frame binding drops it again
        assert c_step() == -2 and "psm_bind_deltas_frames" in last()
        o.free()
        free(d_cols, d_grid, d_label, d_fields)


# ------------------------------------------------------------------------------------------------------- GPU, the evaluator
@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("deltas_frames"))
    c = cases.build_dataset_case(d)
    c["dir"] = d
    return c


def evaluator(c, **kw):
    return Evaluation(5e-3, 128, 32, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, "std", artifact_dir=c["dir"], **kw)


LISTS = ("pred_minus_true", "pred_minus_true_squared", "pred_minus_true_block", "pred_minus_true_squared_block")


def sweep(ds, general):
    """timeSteps(0, [0, 1, 2]) with max_frames = 2 (chunks of 2 + 1), with and without fields, against three timeStep calls of a
    second evaluator: fields within 1e-4 of the field's maximum (the bound of test_evaluation_from_files_end_to_end), truth planes
    bit for bit, the metrics of both blocks of every frame and the four lists within test_field_errors.compare_metrics' bounds.
    ``general``: both evaluators drop their geometry binding first, so that every frame is solved on the general route by both."""
    ref = evaluator(ds)
    assert ref.computeOnlyOnce(0) == 0
    if general:
        ref._sur.unbind_geometry()
    want_fields, want_truth, want_m = [], [], []
    for time in range(3):
        want_fields.append(ref.timeStep(0, time))
        want_truth.append(ref.cfd_results.copy())
        want_m.append({k: dict(v) for k, v in ref.last_metrics.items()})
    assert (ref.grid_shape_y, ref.grid_shape_x) == (138, 300) and ref._sur.B == 6
    for mode in (True, False):
        ev = evaluator(ds, max_frames=2)
        assert ev.computeOnlyOnce(0) == 0
        if general:
            ev._sur.unbind_geometry()
        out = ev.timeSteps(0, [0, 1, 2], fields=mode)
        assert len(out) == 3 and ev._sur.max_cases == 2 and ev._sur.guard_trips == 0 and ev._sur.geometry_bound == (not general)
        for i in range(3):
            if mode:
                err = np.abs(out[i] - want_fields[i]).max() / np.abs(want_fields[i]).max()
                print(f"fields=True frame {i}: max |field - timeStep's| / max |field| = {err:.2e} (bound 1e-4)")
                assert out[i].shape == (138, 300) and err <= 1e-4
            else:
                assert set(out[i]) == {"delta_p", "blocks"}
                compare_metrics(out[i]["delta_p"], want_m[i]["delta_p"], f"fields=False frame {i} delta_p (returned)")
                compare_metrics(out[i]["blocks"], want_m[i]["blocks"], f"fields=False frame {i} blocks (returned)")
        if mode:
            assert same_bits(np.ascontiguousarray(ev.cfd_results), want_truth[2]) and np.array_equal(ev.no_flow_bool, ref.no_flow_bool)
        else:
            assert ev.cfd_results is None
        assert ev.U_max_norm == ref.U_max_norm
        for key in ("delta_p", "blocks"):
            compare_metrics(ev.last_metrics[key], want_m[2][key], f"fields={mode} last_metrics['{key}']")
        for name in LISTS:
            a, b = getattr(ev, name), getattr(ref, name)
            assert len(a) == len(b) == 3, name
            for i in range(3):
                rmse = want_m[i]["blocks" if name.endswith("_block") else "delta_p"]["rmseNorm"]
                print(f"fields={mode} {name}[{i}]: |difference| / (rmseNorm / 100) = {abs(a[i] - b[i]) / (rmse / 100):.2e} (bound 1e-9)")
                assert abs(a[i] - b[i]) <= 1e-9 * rmse / 100, (name, i, a[i], b[i])
    return ev


@pytest.mark.gpu
def test_gpu_evaluator_time_steps(ds):
    """The sweep with both evaluators on the general route: every frame is solved by the same kernels on both sides, so the
    comparison is the device sums against the host passes, at compare_metrics' bounds.  Then: a still frame yields 0 in its slot,
    and call_SM_main(frames_per_call=2, fields=False) returns the default call's keys."""
    ev = sweep(ds, general=True)
    # a middle frame whose velocity hardly changed (the variant of test_evaluation_from_files_end_to_end)
    import h5write
    from psm_amd import formats
    sim2 = ds["sim"].copy()
    sim2[0, 1, :ds["N"], 5:7] *= 1e-7
    p2 = os.path.join(ds["dir"], "still.hdf5")
    tb, ob = formats.read_dataset(ds["dataset_path"], 0, 0)[1:]
    h5write.write_h5(p2, {"sim_data": sim2, "top_bound": np.repeat(tb, 3, axis=1), "obst_bound": np.repeat(ob, 3, axis=1)})
    ev.dataset_path = p2
    again = ev.timeSteps(0, [0, 1, 2], fields=False)
    assert isinstance(again[1], int) and again[1] == 0 and len(ev.pred_minus_true) == 5 and len(ev.pred_minus_true_block) == 5
    assert set(again[0]) == set(again[2]) == {"delta_p", "blocks"}
    args = (5e-3, ds["model_path"], 128, 0.25, 0.95, 0.95, 128, ds["dataset_path"], False, "std", False, False, False, False, 1, 3)
    want = call_SM_main(*args, artifact_dir=ds["dir"])
    got = call_SM_main(*args, artifact_dir=ds["dir"], frames_per_call=2, fields=False)
    assert set(got) == set(want) and set(got["overall"]) == set(want["overall"]) and set(got["sims"][0]) == set(want["sims"][0])
    for key in want["overall"]:
        print(f"call_SM_main {key}: default {want['overall'][key]:.9g}, frames_per_call=2 fields=False {got['overall'][key]:.9g}")
        assert abs(got["overall"][key] - want["overall"][key]) <= 1e-4 * abs(want["overall"]["RMSE" if "block" not in key else "RSME_block"])


@pytest.mark.gpu
def test_gpu_evaluator_time_steps_on_the_bound_routes(ds):
    """The sweep and the main as the evaluators come, geometry bound for one case: timeSteps solves the frames of a chunk one by one
    inside its call, each on the single-case bound route timeStep takes, so fields and metrics are compared at compare_metrics'
    bounds although two chunk sizes and two evaluators are involved."""
    sweep(ds, general=False)
    # the main
    args = (5e-3, ds["model_path"], 128, 0.25, 0.95, 0.95, 128, ds["dataset_path"], False, "std", False, False, False, False, 1, 3)
    want = call_SM_main(*args, artifact_dir=ds["dir"])
    got = call_SM_main(*args, artifact_dir=ds["dir"], frames_per_call=2, fields=False)
    assert set(got) == set(want) and set(got["overall"]) == set(want["overall"]) and set(got["sims"][0]) == set(want["sims"][0])
    worst = 0.0
    for g, w in ((got["overall"], want["overall"]), (got["sims"][0], want["sims"][0])):
        for b, r, s in (("BIAS", "RMSE", "STDE"), ("BIAS_block", "RSME_block", "STDE_block")):
            worst = max(worst, abs(g[b] - w[b]) / w[r], abs(g[r] - w[r]) / w[r], abs(g[s] - w[s]) / abs(w[s]) / 10)
    print(f"call_SM_main(frames_per_call=2, fields=False) against the default call: worst BIAS / RMSE difference {worst:.2e} of RMSE "
          f"(bound 1e-9; STDE 1e-8 relative)\n  got  {got['overall']}\n  want {want['overall']}")
    assert worst <= 1e-9
