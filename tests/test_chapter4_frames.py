"""The frame batch of the two Chapter-4 evaluators on the device (psm_bind_chapter4_frames, psm_chapter4_image_device,
psm_chapter4_frames_device / psm_chapter4_frames), stage by stage, for both image widths (M_u: c_in = 3, M_fU: c_in = 2).

The stages run on the 130 x 131 grid of tests/test_field_errors.py (17 030 pixels: 16 pack workgroups of 1024 pixels + 646, the last
vector of four cut to two; four 128 x 128 blocks of the chapter5 layout at overlap 96 that overlap in both directions) with its
200-cell mesh, its rectangle of SDF zeros and the NaN label cells of its frame columns; max_cases = 3.  A c_in = 3 frame image is
204 360 bytes = 8 (mod 16): behind a lead of 4 elements frames 0 and 2 start 16-byte aligned and frame 1 does not, behind a lead of
5 none does.  A c_in = 2 frame image is 136 240 bytes = 0 (mod 16): lead 0 is aligned, lead 2 is not.  A truth frame is 136 240
bytes: aligned behind an even lead, not behind an odd one.

References: the NumPy statements of EvaluationChapter4.timeStep on the planes psm_frames_to_grid_device wrote (bit for bit);
GridSurrogate.solve on the same image (bit for bit); psm_field_errors_device alone (bit for bit) and NumPy on the step's planes --
counts and extrema bit for bit, the two sums against math.fsum within test_field_errors.SUM_TOL.
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
from oracle import psm_oracle as orc
from psm_amd import EvaluationChapter4, GridSurrogate, _lib, main_chapter4, synthetic
from test_field_errors import CANARY, EXACT, N_, NF, NPIX, NX, NY, PAD, S1, S2, SUM_TOL, TNAN, differences, flow_tables, frame_inputs, np_raw
from test_poisson_frames import same_bits
from test_poisson_step_device import free, model4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "solving-poisson-s-equation-through-dl-for-cfd-apllications_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW_ENTRIES = ("psm_bind_chapter4_frames", "psm_unbind_chapter4_frames", "psm_chapter4_image_device", "psm_chapter4_frames_device",
               "psm_chapter4_frames")
NEW_METHODS = ("bind_chapter4_frames", "unbind_chapter4_frames", "chapter4_image_device", "chapter4_frames_device", "chapter4_frames")
WIDTHS = (3, 2)
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


def maxs(c_in):
    """[c_in + 1]: the c_in - 1 input channels, dist, p."""
    m = cases.DATASET_MAXS
    return m if c_in == 3 else (m[0], m[2], m[3])


@functools.lru_cache(maxsize=None)
def model(c_in):
    m = synthetic.make_model("chapter5", p_in=32, p_out=32, c_in=c_in)
    m.ov, m.sdf_ch = 96, c_in - 1
    return m


@functools.lru_cache(maxsize=None)
def stage_inputs(c_in):
    """(cols [NF][200][c_in], raw SDF plane with NaNs): the last c_in of the columns (dUx, dUy, delta_p) of test_field_errors' frames,
    so the label column carries its NaN cells; the SDF keeps the rectangle of zeros and gets a NaN strip of its own."""
    cols8 = frame_inputs()[0]
    cols = np.ascontiguousarray(cols8[..., 5 - c_in:5])
    assert np.isnan(cols[..., -1]).sum() == 4 and not np.isnan(cols[..., :-1]).any()
    sdf = flow_tables().sdfunct.copy()
    sdf[3, 5:60] = np.nan
    return cols, sdf


def surrogate(c_in, bind=True, m=None):
    t = flow_tables()
    sur = GridSurrogate(m or model(c_in), t.ny, t.nx, max_cases=NF)
    sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
    if bind:
        sur.bind_frames(NF, c_in)
        sur.bind_chapter4_frames(stage_inputs(c_in)[1], maxs(c_in))
    return sur


def host_statements(planes, sdf, c_in):
    """What EvaluationChapter4.timeStep does with the planes of one frame [c_in][NY][NX]: (image float32 [NY,NX,c_in], truth float64)."""
    mx = maxs(c_in)
    grid = np.zeros((NY, NX, c_in + 1))
    grid[..., :c_in - 1] = np.moveaxis(planes[:c_in - 1], 0, 2)
    grid[..., c_in - 1] = sdf
    grid[..., c_in] = planes[c_in - 1]
    grid[np.isnan(grid)] = 0                                                        # M_u :220
    for ch in range(c_in + 1):
        grid[..., ch] /= mx[ch]                                                     # :222-225
    return np.ascontiguousarray(grid[..., :c_in], np.float32), grid[..., c_in].copy()


def device_planes(sur, d_cols, c_in):
    d_pl = DeviceArray(np.full((NF, c_in, NPIX), CANARY, np.float64))
    sur.frames_to_grid_device(d_cols.ptr, NF, c_in, [(d_pl.ptr + c * NPIX * 8, c_in * NPIX, False) for c in range(c_in)])
    sur.synchronize()
    planes = d_pl.numpy().reshape(NF, c_in, NY, NX)
    d_pl.free()
    return planes


def device_image(sur, d_cols, c_in):
    d_grid, d_truth = DeviceArray(shape=(NF, NY, NX, c_in)), DeviceArray(shape=(NF, NPIX), dtype=np.float64)
    sur.chapter4_image_device(d_cols.ptr, NF, c_in, d_grid.ptr, d_truth.ptr)
    sur.synchronize()
    out = d_grid.numpy(), d_truth.numpy().reshape(NF, NY, NX)
    free(d_grid, d_truth)
    return out


def upload(d, host):
    host = np.ascontiguousarray(host, d.dtype)
    assert host.nbytes == d.nbytes and _lib.load().psm_debug_copy_to_device(d.ptr, host.ctypes.data, d.nbytes) == 0


def raw_buffer():
    return DeviceArray(np.full(PAD + NF * 8 + PAD, CANARY, np.float64))


def read_raw(d_raw, n=NF):
    a = d_raw.numpy()
    assert (a[:PAD] == CANARY).all() and (a[PAD + n * 8:] == CANARY).all(), "canary round d_raw"
    return a[PAD:PAD + n * 8].reshape(n, 1, 8).copy()


class StepOut:
    def __init__(self):
        self.res = DeviceArray(np.full(PAD + NF * NPIX + PAD, CANARY, np.float32))
        self.truth = DeviceArray(np.full(PAD + 1 + NF * NPIX + PAD, CANARY, np.float64))
        self.raw = raw_buffer()
        self.p_res, self.p_truth, self.p_raw = self.res.ptr + PAD * 4, self.truth.ptr + (PAD + 1) * 8, self.raw.ptr + PAD * 8

    def read(self, n=NF):
        r, t = self.res.numpy(), self.truth.numpy()
        assert (r[:PAD] == CANARY).all() and (r[PAD + n * NPIX:] == CANARY).all() and (t[:PAD + 1] == CANARY).all() and (t[PAD + 1 + n * NPIX:] == CANARY).all()
        return r[PAD:PAD + n * NPIX].reshape(n, NY, NX).copy(), t[PAD + 1:PAD + 1 + n * NPIX].reshape(n, NY, NX).copy(), read_raw(self.raw, n)

    def untouched(self):
        return all((d.numpy() == CANARY).all() for d in (self.res, self.truth, self.raw))

    def free(self):
        free(self.res, self.truth, self.raw)


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
    sig = inspect.signature(EvaluationChapter4.__init__).parameters
    assert sig["inputs"].default == "M_u" and sig["max_frames"].default is None
    assert inspect.signature(EvaluationChapter4.timeSteps).parameters["fields"].default is True
    sig = inspect.signature(main_chapter4).parameters
    assert sig["frames_per_call"].default == 1 and sig["fields"].default is True and sig["sims"].default == (0, 3, 6, 8) and sig["n_ts"].default == 10
    import psm_amd
    for name in ("EvaluationChapter4", "main_chapter4"):                    # re-exported from surrogate and from the package
        assert callable(getattr(psm_amd.surrogate, name, None)) and callable(getattr(psm_amd, name, None)) and name in psm_amd.__all__, name


def test_the_stage_grid_has_four_blocks_that_overlap_both_ways():
    lay = orc.block_layout("chapter5", NY, NX, ov=96)
    assert [tuple(int(v) for v in b) for b in lay.origins] == [(0, 3), (0, 0), (2, 3), (2, 0)]
    assert NPIX == 16 * 1024 + 646 and (NPIX * 12) % 16 == 8 and (NPIX * 8) % 16 == 0


def test_python_argument_checks_come_before_any_library_call():
    """The new mirrors refuse bad arguments on a surrogate whose library and handle do not exist: any call into the library would
    raise AttributeError instead."""
    for c_in in WIDTHS:
        sur = GridSurrogate.__new__(GridSurrogate)
        sur.lib = sur.h = None
        sur.ny, sur.nx, sur.model, sur.mesh_cells, sur.max_cases = 6, 7, model(c_in), 11, 3
        sdf, mx = np.ones((6, 7)), maxs(c_in)
        with pytest.raises(RuntimeError, match="bind_frames"):
            sur.bind_chapter4_frames(sdf, mx)
        sur._frames_bound = True
        with pytest.raises(ValueError, match=r"\[6,7\]"):
            sur.bind_chapter4_frames(np.ones((6, 8)), mx)
        for bad in (mx[:-1] + (0.0,), (np.inf,) + mx[1:], mx[:-1] + (np.nan,), mx[:-1], mx + (1.0,)):
            with pytest.raises(ValueError, match=r"c_in \+ 1 finite non-zero"):
                sur.bind_chapter4_frames(sdf, bad)
        with pytest.raises(RuntimeError, match="bind_chapter4_frames"):
            sur.chapter4_frames_device(4096, 2, c_in)
        sur._chapter4_bound = True
        step = lambda **kw: sur.chapter4_frames_device(**{**dict(d_cols=4096, n_frames=2, k=c_in, d_result=4096, d_truth=4096, d_raw=4096), **kw})
        image = lambda **kw: sur.chapter4_image_device(**{**dict(d_cols=4096, n_frames=2, k=c_in, d_grid=4096, d_truth=4096), **kw})
        for call in (step, image):
            for k in (c_in - 1, 17):
                with pytest.raises(ValueError, match=r"c_in\.\.16 columns"):
                    call(k=k)
            for n in (0, 4):
                with pytest.raises(ValueError, match="n_frames"):
                    call(n_frames=n)
            with pytest.raises(ValueError, match="d_cols"):
                call(d_cols=0)
            with pytest.raises(ValueError, match="d_truth"):
                call(d_truth=4100)
        with pytest.raises(ValueError, match="d_raw"):
            step(d_raw=4100)
        with pytest.raises(ValueError, match="d_result"):
            step(d_result=4098)
        with pytest.raises(ValueError, match="d_grid"):
            image(d_grid=0)
        ok = np.zeros((2, 11, c_in))
        with pytest.raises(ValueError, match=r"c_in\.\.16 columns"):
            sur.chapter4_frames(ok[..., :c_in - 1])
        with pytest.raises(ValueError, match="11 cells"):
            sur.chapter4_frames(np.zeros((2, 12, c_in)))
        with pytest.raises(ValueError, match="nothing to return"):
            sur.chapter4_frames(ok, want_result=False, want_truth=False, want_raw=False)
        sur.mesh_cells = None
        with pytest.raises(RuntimeError, match="no mesh"):
            sur.chapter4_frames(ok)
    for m in (model4(), synthetic.make_model("deltas", p_in=8, p_out=8, c_in=3), synthetic.make_model("chapter5", p_in=8, p_out=8, c_in=3, c_out=2)):
        bad = GridSurrogate.__new__(GridSurrogate)
        bad.lib = bad.h = None
        bad.ny, bad.nx, bad.model, bad._frames_bound = 6, 7, m, True
        with pytest.raises(ValueError, match="chapter5-variant model"):
            bad.bind_chapter4_frames(np.ones((6, 7)), (1.0,) * (m.c_in + 1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc (psm_handle.h includes the HIP headers)")
def test_chapter4_call_is_keyed_and_its_combinations_are_refused(tmp_path):
    """tests/native/chapter4_step_sanitized.cpp, a stand-alone host program under AddressSanitizer + UBSan: Chapter4Call is in
    StepCall::key() with distinct keys for distinct planes / grid / truth, and StepCall::fault names every excluded combination."""
    exe = str(tmp_path / "chapter4_step_sanitized")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "chapter4_step_sanitized.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "chapter4 step:" in r.stdout and " 0 failures" in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------------------------------------------- GPU, the pack
@pytest.mark.gpu
@pytest.mark.parametrize("c_in", WIDTHS)
def test_gpu_pack_is_the_host_statements_bit_for_bit(c_in):
    """Image and truth of psm_chapter4_image_device against timeStep's NumPy statements on the planes psm_frames_to_grid_device
    wrote: bit for bit, for 1 and 3 frames, behind leads after which the frames start 16-byte aligned and leads after which they do
    not, with canaries in front of and behind the outputs; the NaN label cells become 0; d_truth is optional."""
    cols, sdf = stage_inputs(c_in)
    leads = ((4, 4), (5, 5)) if c_in == 3 else ((0, 0), (2, 1))        # (image, truth) lead in elements
    with surrogate(c_in) as sur:
        d_cols = DeviceArray(cols)
        planes = device_planes(sur, d_cols, c_in)
        assert np.isnan(planes[:, c_in - 1]).sum() > 100 and not np.isnan(planes[:, :c_in - 1]).any()
        want = [host_statements(planes[f], sdf, c_in) for f in range(NF)]
        assert (want[0][0][..., c_in - 1] == 0).sum() >= 35 * 40 + 55 and all(np.isfinite(w[1]).all() for w in want)
        assert all((w[1][np.isnan(planes[f, c_in - 1])] == 0).all() for f, w in enumerate(want))
        sizes, dtypes = (NPIX * c_in, NPIX), (np.float32, np.float64)
        starts = [set(), set()]
        for lead in leads:
            for n in (1, NF):
                bufs = [DeviceArray(np.full(ld + NF * s + PAD, CANARY, dt)) for ld, s, dt in zip(lead, sizes, dtypes)]
                ptrs = [b.ptr + ld * np.dtype(dt).itemsize for b, ld, dt in zip(bufs, lead, dtypes)]
                for q, (p, s, dt) in enumerate(zip(ptrs, sizes, dtypes)):
                    starts[q] |= {(p + f * s * np.dtype(dt).itemsize) % 16 == 0 for f in range(n)}
                sur.chapter4_image_device(d_cols.ptr, n, c_in, *ptrs)
                sur.synchronize()
                same = []
                for q, (b, ld, s) in enumerate(zip(bufs, lead, sizes)):
                    a = b.numpy()
                    assert (a[:ld] == CANARY).all() and (a[ld + n * s:] == CANARY).all(), ("canary", lead, n, q)
                    got = a[ld:ld + n * s].reshape((n,) + want[0][q].shape)
                    same.append(all(same_bits(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f][q])) for f in range(n)))
                print(f"c_in {c_in}, leads {lead}, {n} frame(s): image / truth identical to the host statements {same}")
                assert all(same)
                free(*bufs)
        assert starts == [{False, True}, {False, True}], "the frames must start both 16-byte aligned and not"
        d_g = DeviceArray(np.full((NF, NY, NX, c_in), CANARY, np.float32))
        sur.chapter4_image_device(d_cols.ptr, NF, c_in, d_g.ptr)                   # the truth plane is optional
        sur.synchronize()
        assert all(same_bits(d_g.numpy()[f], want[f][0]) for f in range(NF))
        free(d_cols, d_g)


# ------------------------------------------------------------------------------------------------------- GPU, the whole step
def bind_other_geometry(sur, sdf, c_in):
    g = np.zeros((NY, NX, c_in), np.float32)                                       # the step solves its frames one by one: one case
    sd = np.roll(np.nan_to_num(sdf, nan=0.0), 11, axis=1) / maxs(c_in)[-2]
    g[..., c_in - 1] = sd.astype(np.float32)
    assert sur.bind_geometry(g) and sur.geometry_bound


@pytest.mark.gpu
@pytest.mark.parametrize("c_in", WIDTHS)
def test_gpu_whole_step(c_in):
    """psm_chapter4_frames_device on the general and the bound route: every frame's result is GridSurrogate.solve on its image, the
    same frame sent alone gives the same bits, the truth plane is the pack's, raw is psm_field_errors_device alone on the step's
    planes and NumPy on them (counts and extrema exact, the sums within SUM_TOL of math.fsum), the host entry returns the device
    entry's bits, also for two of three bound frames; a second call on the same buffers with other columns returns those frames;
    bound to another geometry the host entry takes one guard trip and returns the general path's bits."""
    cols, sdf = stage_inputs(c_in)
    sdn = np.nan_to_num(sdf, nan=0.0) / maxs(c_in)[-2]
    flow = sdn != 0
    with surrogate(c_in) as sur:
        d_cols = DeviceArray(cols)
        image, truth = device_image(sur, d_cols, c_in)
        d_sdn = DeviceArray(sdn)
        kept = {}
        for route in ("general", "bound"):
            if route == "bound":
                assert sur.bind_geometry(image[0]) and sur.geometry_bound              # every frame carries the simulation's SDF channel
            o = StepOut()
            sur.chapter4_frames_device(d_cols.ptr, NF, c_in, o.p_res, o.p_truth, o.p_raw)
            d_f = raw_buffer()
            sur.field_errors_device((d_sdn.ptr, 0, 1, 0), [((o.p_res, NPIX, 1, 1), (o.p_truth, NPIX, 1, 0), None, None, False)], NF, d_f.ptr + PAD * 8)
            sur.synchronize()
            res, tr, raw = o.read()
            rf = read_raw(d_f)
            solved = np.stack([sur.solve(image[f])[0, :, :, 0] for f in range(NF)])
            h_res, h_tr, h_raw = sur.chapter4_frames(cols)
            alone = [sur.chapter4_frames(cols[f]) for f in range(NF)]
            two = sur.chapter4_frames(cols[:2])
            same = dict(solve=same_bits(res, solved), truth=same_bits(tr, truth), raw_alone=same_bits(raw, rf), host_result=same_bits(h_res, res),
                        host_truth=same_bits(h_tr, tr), host_raw=same_bits(h_raw, raw),
                        frame_alone=all(same_bits(a[0][0], res[f]) and same_bits(a[2][0], raw[f]) for f, a in enumerate(alone)),
                        two_of_three=same_bits(two[0], res[:2]) and same_bits(two[1], tr[:2]) and same_bits(two[2], raw[:2]))
            worst1 = worst2 = 0.0
            for f in range(NF):
                w = np_raw(res[f], tr[f], flow)
                d = differences(res[f], tr[f], flow)[2]
                s1, sabs, s2 = math.fsum(d), math.fsum(np.abs(d)), math.fsum(d * d)
                g = raw[f, 0]
                assert same_bits(np.ascontiguousarray(g[list(EXACT)]), np.ascontiguousarray(w[list(EXACT)])), (route, f, g, w)
                worst1, worst2 = max(worst1, abs(g[S1] - s1) / sabs), max(worst2, abs(g[S2] - s2) / s2)
            print(f"c_in {c_in} {route}: {same}; counts and extrema identical to NumPy, |s1 - fsum| / sum|d| <= {worst1:.2e}, "
                  f"|s2 - fsum| / s2 <= {worst2:.2e} (bound {SUM_TOL}); n per frame {raw[:, 0, N_].astype(int).tolist()}, flow cells {int(flow.sum())}")
            assert all(same.values()) and np.isfinite(res).all()
            assert worst1 <= SUM_TOL and worst2 <= SUM_TOL
            assert (raw[:, 0, N_] == flow.sum()).all() and (raw[..., TNAN] == 0).all()
            only = sur.chapter4_frames(cols, want_result=False, want_truth=False)
            assert only[0] is None and only[1] is None and same_bits(only[2], raw)
            # replay: the same buffers, the frames in another order
            kept[route] = (res, raw)
            upload(d_cols, cols[::-1])
            sur.chapter4_frames_device(d_cols.ptr, NF, c_in, o.p_res, o.p_truth, o.p_raw)
            sur.synchronize()
            r2, t2, w2 = o.read()
            rep = same_bits(r2, np.ascontiguousarray(res[::-1])) and same_bits(t2, np.ascontiguousarray(tr[::-1])) and same_bits(w2, np.ascontiguousarray(raw[::-1]))
            upload(d_cols, cols)
            print(f"c_in {c_in} {route}: a replay on the same buffers with the frames reversed returns the reversed results {rep}")
            assert rep
            d_f.free()
            o.free()
        assert sur.guard_trips == 0 and sur.geometry_bound
        d1 = np.abs(kept["bound"][0] - kept["general"][0]).max() / np.abs(kept["general"][0]).max()
        print(f"c_in {c_in}: bound against general route, max |difference| / max |field| = {d1:.2e}")
        assert d1 <= 2e-5
        bind_other_geometry(sur, sdf, c_in)
        got = sur.chapter4_frames(cols)
        print(f"c_in {c_in} bound to another geometry: guard trips {sur.guard_trips}, still bound {sur.geometry_bound}, result and rows identical "
              f"to the general path {same_bits(got[0], kept['general'][0])} {same_bits(got[2], kept['general'][1])}")
        assert sur.guard_trips == 1 and not sur.geometry_bound and "not the one bound" in _lib.last_error(sur.h)
        assert same_bits(got[0], kept["general"][0]) and same_bits(got[2], kept["general"][1]) and same_bits(got[1], truth)
        free(d_cols, d_sdn)


# ------------------------------------------------------------------------------------------------------- GPU, errors and drops
@pytest.mark.gpu
def test_gpu_error_returns_enqueue_nothing_and_leave_the_handle_usable():
    """Every PSM_ERR_STATE / PSM_ERR_ARG arm: a deltas handle, c_in = 4, an SDF channel that is not the last (psm_create
    itself refuses a chapter5 handle with c_out = 2); frames or
    the Chapter-4 binding unbound; bad scales; k outside its range or beyond the staging; n_frames 0 and 4; null and misaligned
    pointers.  Each returns its code, the outputs keep their sentinels, and the handle then runs a correct call.  Then every event
    that drops the binding makes the next call PSM_ERR_STATE."""
    c_in = 3
    cols, sdf = stage_inputs(c_in)
    t = flow_tables()
    mx = np.array(maxs(c_in), np.float64)
    sdf_c = np.ascontiguousarray(sdf)
    not_last = synthetic.make_model("chapter5", p_in=8, p_out=8, c_in=3)
    not_last.ov, not_last.sdf_ch = 96, 1
    four = synthetic.make_model("chapter5", p_in=8, p_out=8, c_in=4)
    four.ov, four.sdf_ch = 96, 3
    deltas = synthetic.make_model("deltas", p_in=8, p_out=8, c_in=3)
    for m, rule in ((deltas, "PSM_VARIANT_CHAPTER5"), (four, "c_in in {2, 3}"), (not_last, "sdf_channel == c_in - 1")):
        with GridSurrogate(m, NY, NX, max_cases=NF) as bad:
            bad.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
            bad.bind_frames(NF, 3)
            rc = bad.lib.psm_bind_chapter4_frames(bad.h, sdf_c.ctypes.data_as(_dp), np.ones(5).ctypes.data_as(_dp))
            print(f"{m.variant} c_in {m.c_in} c_out {m.c_out} sdf_ch {m.sdf_ch}: rc {rc}, {_lib.last_error(bad.h)!r}")
            assert rc == -2 and rule in _lib.last_error(bad.h)
    with surrogate(c_in, bind=False) as sur:
        d_cols = DeviceArray(cols)
        o = StepOut()
        d_grid = DeviceArray(np.full((NF, NY, NX, c_in), CANARY, np.float32))
        lib, h = sur.lib, sur.h
        c_bind = lambda m=mx, s=sdf_c: lib.psm_bind_chapter4_frames(h, s.ctypes.data_as(_dp) if s is not None else None,
                                                                    m.ctypes.data_as(_dp) if m is not None else None)
        c_step = lambda n=NF, k=c_in, cols=d_cols.ptr, res=o.p_res, truth=o.p_truth, raw=o.p_raw: lib.psm_chapter4_frames_device(h, cols, n, k, res, truth, raw, None)
        c_image = lambda n=NF, k=c_in, cols=d_cols.ptr, grid=d_grid.ptr, truth=o.p_truth: lib.psm_chapter4_image_device(h, cols, n, k, grid, truth, None)
        host_raw = np.full((NF, 1, 8), CANARY)
        c_host = lambda n=NF, k=c_in, c=cols, raw=host_raw: lib.psm_chapter4_frames(h, c.ctypes.data_as(_dp) if c is not None else None, n, k, None, None,
                                                                                    raw.ctypes.data_as(_dp) if raw is not None else None)
        last = lambda: _lib.last_error(h)
        assert c_bind() == -2 and "psm_bind_frames" in last()
        assert c_step() == -2 and "psm_bind_frames" in last() and c_image() == -2 and c_host() == -2
        sur.bind_frames(NF, c_in)
        assert c_step() == -2 and "psm_bind_chapter4_frames" in last() and c_image() == -2 and c_host() == -2
        for bad in ((1.0, 1.0, 0.0, 1.0), (np.inf, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, np.nan), (1.0, -np.inf, 1.0, 1.0)):
            assert c_bind(m=np.array(bad)) == -1 and "finite and non-zero" in last()
        assert c_bind(s=None) == -1 and c_bind(m=None) == -1 and c_step() == -2
        assert c_bind() == 0
        sur._chapter4_bound = True                                                # bound through the C entry: tell the mirror
        assert c_step(k=c_in - 1) == -1 and "[c_in, 16]" in last() and c_image(k=c_in - 1) == -1 and c_host(k=c_in - 1) == -1
        assert c_step(k=17) == -1 and c_image(k=17) == -1 and c_host(k=17) == -1
        for n in (0, NF + 1):
            assert c_step(n=n) == -1 and "n_frames" in last() and c_image(n=n) == -1 and c_host(n=n) == -1
        assert c_step(raw=o.p_raw + 4) == -1 and "d_raw" in last() and c_step(res=o.p_res + 2) == -1 and "d_result" in last()
        assert c_step(truth=o.p_truth + 4) == -1 and "truth" in last() and c_image(truth=o.p_truth + 4) == -1
        assert c_step(cols=None) == -1 and c_image(cols=None) == -1 and c_image(grid=None) == -1 and c_image(grid=d_grid.ptr + 2) == -1
        assert c_host(c=None) == -1 and c_host(raw=None) == -1
        assert c_host(k=c_in + 1) == -1 and "reserved staging" in last()
        sur.synchronize()
        assert o.untouched() and (d_grid.numpy() == CANARY).all() and (host_raw == CANARY).all()
        # the handle still works: device entry against the host entry
        assert c_step() == 0
        sur.synchronize()
        res, tr, raw = o.read()
        h_res, h_tr, h_raw = sur.chapter4_frames(cols)
        same = [same_bits(h_res, res), same_bits(h_tr, tr), same_bits(h_raw, raw)]
        print(f"after the refused calls: result, truth and raw of the device and the host entry identical {same}")
        assert all(same) and (raw[..., N_] > 0).all()
        # what drops the binding
        mesh = lambda: sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        m = sur.model
        sc = [np.ascontiguousarray(np.broadcast_to(v, (n,)), np.float64) for v, n in ((m.in_a, m.p_in), (m.in_b, m.p_in), (m.out_a, m.p_out), (m.out_b, m.p_out))]
        drops = {"psm_unbind_chapter4_frames": sur.unbind_chapter4_frames,
                 "psm_bind_frames": lambda: sur.bind_frames(NF, c_in),
                 "psm_unbind_frames": sur.unbind_frames,
                 "a new mesh": mesh,
                 "psm_plan_grid": lambda: sur._chk(lib.psm_plan_grid(h, NY, NX)),
                 "psm_set_scaler": lambda: sur._chk(lib.psm_set_scaler(h, *[v.ctypes.data_as(_dp) for v in sc]))}
        for what, event in drops.items():
            mesh()                                                                # whatever the last event left: plan, mesh, both bindings anew
            sur.bind_frames(NF, c_in)
            sur.bind_chapter4_frames(sdf, maxs(c_in))
            assert c_step() == 0
            sur.synchronize()
            event()
            rc = c_step()
            print(f"after {what}: rc {rc}, {last()!r}")
            assert rc == -2, what
        o.free()
        free(d_cols, d_grid)

