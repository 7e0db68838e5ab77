"""The frame batch of the U_to_gradP evaluator on the device (psm_bind_gradp_frames, psm_gradp_image_device,
psm_gradp_frames_device / psm_gradp_frames) and EvaluationGradP.timeSteps / main_gradP(frames_per_call, fields) on top of them.

Stage tests run on the 130 x 131 grid of tests/test_field_errors.py (17 030 pixels: 16 pack workgroups of 1024 pixels + 646, the last
vector of four cut to two; four 128 x 128 blocks that overlap in both directions) with its 200-cell mesh and its rectangle of SDF
zeros, the NaN label cells of its frame columns in all three label columns, the two-channel model
synthetic.make_model("gradp", p_in=32, p_out=32) and max_cases = 3.  An image frame is 204 360 bytes, 8 (mod 16): of three frames
behind a lead of 4 elements frames 0 and 2 start 16-byte aligned and frame 1 does not, behind a lead of 5 none does; the label frames
(408 720 bytes) are all aligned behind a lead of 4 and none behind 5.  The raw SDF has no NaN (the integration casts its rows to an
index list); the cuts (57, 50), (40, 50) and (20, 50) are accepted by oracle.integrate_gradp on it, (57, 30) makes it raise (40
flow cells against 57 on the two cut columns).

References: the NumPy statements of EvaluationGradP.timeStep on the planes psm_frames_to_grid_device wrote (bit for bit); solve /
solve_poststeps and set_integration + integrate_gradp per frame (bit for bit); psm_field_errors_device alone (bit for bit) and NumPy
(counts and extrema bit for bit, the two sums within test_field_errors.SUM_TOL of math.fsum); the float64 oracle chain within
test_gradp_pressure.CHAIN_TOL; five timeStep calls of a second evaluator.  Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools
import inspect
import math
import re

import numpy as np
import pytest

import cases
from hipmem import DeviceArray
from psm_amd import GridSurrogate, _lib, synthetic
from psm_amd.surrogate import EvaluationGradP, main_gradP
from test_field_errors import (CANARY, EXACT, N_, NF, NPIX, NX, NY, PAD, S1, S2, SUM_TOL, TNAN, compare_metrics, differences, flow_tables,
                               frame_inputs, np_raw)
from test_gradp_pressure import CHAIN_TOL, oracle_gradp, ratio
from test_poisson_frames import same_bits
from test_poisson_step_device import free

NEW_ENTRIES = ("psm_bind_gradp_frames", "psm_unbind_gradp_frames", "psm_gradp_image_device", "psm_gradp_frames_device", "psm_gradp_frames")
NEW_METHODS = ("bind_gradp_frames", "unbind_gradp_frames", "gradp_image_device", "gradp_frames_device", "gradp_frames")
MAXS = cases.GRADP_MAXS                        # the scales of grid channels 0-4
CUT, DX, DY = (57, 50), 1.0 / NX, 1.0 / NY
ROWS = 4
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


@functools.lru_cache(maxsize=None)
def model2():
    m = synthetic.make_model("gradp", p_in=32, p_out=32)
    assert (m.c_in, m.sdf_ch, m.c_out) == (3, 2, 2)
    return m


@functools.lru_cache(maxsize=None)
def stage_inputs():
    """(cols [NF][200][5], raw SDF plane): velocities and three label columns from test_field_errors' frames; its NaN cells sit in
    columns 4 and 5, which become label columns 0 and 1, and label column 2 mixes the two, so it carries the NaN cells of both."""
    c8 = frame_inputs()[0]
    cols = np.ascontiguousarray(np.stack([c8[..., 0], c8[..., 1], c8[..., 4], c8[..., 5], 0.5 * c8[..., 4] + c8[..., 5]], axis=-1))
    nans = np.isnan(cols).sum(axis=(0, 1))
    assert nans.tolist() == [0, 0, 4, 3, 6], nans
    sdf = np.ascontiguousarray(flow_tables().sdfunct)
    assert not np.isnan(sdf).any()
    return cols, sdf


def surrogate2(bind=True, post=False, cut=CUT):
    t = flow_tables()
    sur = GridSurrogate(model2(), t.ny, t.nx, max_cases=NF)
    sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
    if bind:
        sur.bind_frames(NF, 5)
        assert sur.bind_gradp_frames(stage_inputs()[1], MAXS, cut[0], cut[1], DX, DY)
    if post:
        sur.bind_poststeps((10, 10), (50, 50))
    return sur


def host_statements(planes, sdf):
    """What EvaluationGradP.timeStep does with the planes of one frame [5][NY][NX]: (image float32 [NY,NX,3], labels [3][NY][NX])."""
    grid = np.zeros((NY, NX, 6))
    grid[..., 0:2] = np.moveaxis(planes[0:2], 0, 2)
    grid[..., 2] = sdf
    grid[..., 3:6] = np.moveaxis(planes[2:5], 0, 2)
    grid[np.isnan(grid)] = 0                                                        # Eval_dual_Dense_onlycil.py:461
    for ch in range(5):
        grid[..., ch] /= MAXS[ch]                                                   # :463-467
    return np.ascontiguousarray(grid[..., :3], np.float32), np.ascontiguousarray(np.moveaxis(grid[..., 3:6], 2, 0))


def device_planes(sur, d_cols):
    d_pl = DeviceArray(np.full((NF, 5, NPIX), CANARY, np.float64))
    sur.frames_to_grid_device(d_cols.ptr, NF, 5, [(d_pl.ptr + c * NPIX * 8, 5 * NPIX, False) for c in range(5)])
    sur.synchronize()
    planes = d_pl.numpy().reshape(NF, 5, NY, NX)
    d_pl.free()
    return planes


def device_image(sur, d_cols):
    d_grid, d_truth = DeviceArray(shape=(NF, NY, NX, 3)), DeviceArray(shape=(NF, 3, NPIX), dtype=np.float64)
    sur.gradp_image_device(d_cols.ptr, NF, 5, d_grid.ptr, d_truth.ptr)
    sur.synchronize()
    out = d_grid.numpy(), d_truth.numpy().reshape(NF, 3, NY, NX)
    free(d_grid, d_truth)
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
    assert re.search(r"#define\s+PSM_ABI_VERSION\s+4\b", txt) and _lib.PSM_ABI_VERSION == 4 and lib.psm_abi_version() == 4
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert GridSurrogate._gradp_bound is False
    assert inspect.signature(EvaluationGradP.__init__).parameters["max_frames"].default is None and EvaluationGradP.max_frames == 1
    assert EvaluationGradP.timeSteps is not EvaluationGradP.__mro__[1].timeSteps and EvaluationGradP._bind_frames is not EvaluationGradP.__mro__[1]._bind_frames
    sig = inspect.signature(EvaluationGradP.timeSteps).parameters
    assert sig["fields"].default is True and sig["apply_filter"].default is False
    sig = inspect.signature(main_gradP).parameters
    assert sig["frames_per_call"].default == 1 and sig["fields"].default is True
    sig = inspect.signature(GridSurrogate.gradp_frames).parameters
    assert [sig[k].default for k in ("out_scale", "apply_filter", "want_gradp", "want_p", "want_truth")] == [None, False, True, True, True]


def test_python_argument_checks_come_before_any_library_call():
    """The new mirrors refuse bad arguments on a surrogate whose library and handle do not exist: any call into the library would
    raise AttributeError instead."""
    sur = GridSurrogate.__new__(GridSurrogate)
    sur.lib = sur.h = None
    sur.ny, sur.nx, sur.model, sur.mesh_cells, sur.max_cases = 6, 7, model2(), 11, 3
    sdf = np.ones((6, 7))
    bind = lambda **kw: sur.bind_gradp_frames(**{**dict(sdfunct=sdf, max_abs=MAXS, center_y=3, center_x=3, dx=0.1, dy=0.1), **kw})
    with pytest.raises(RuntimeError, match="bind_frames"):
        bind()
    sur._frames_bound = True
    with pytest.raises(ValueError, match=r"\[6,7\]"):
        bind(sdfunct=np.ones((6, 8)))
    for bad in ((1.0, 1.0, 0.0, 1.0, 1.0), (1.0, np.inf, 1.0, 1.0, 1.0), (np.nan, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="five finite non-zero"):
            bind(max_abs=bad)
    for cy, cx in ((0, 3), (6, 3), (3, 0), (3, 7)):
        with pytest.raises(ValueError, match="outside the grid"):
            bind(center_y=cy, center_x=cx)
    one = GridSurrogate.__new__(GridSurrogate)
    one.lib = one.h = None
    one.ny, one.nx, one.model, one._frames_bound = 6, 7, synthetic.make_model("deltas", p_in=8, p_out=8), True
    with pytest.raises(ValueError, match="2 output channels"):
        one.bind_gradp_frames(sdf, MAXS, 3, 3, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="bind_gradp_frames"):
        sur.gradp_frames_device(4096, 2, 5)
    with pytest.raises(RuntimeError, match="bind_gradp_frames"):
        sur.gradp_image_device(4096, 2, 5, 4096)
    with pytest.raises(RuntimeError, match="bind_gradp_frames"):
        sur.gradp_frames(np.zeros((2, 11, 5)))
    sur._gradp_bound = True
    step = lambda **kw: sur.gradp_frames_device(**{**dict(d_cols=4096, n_frames=2, k=5, d_gradp=4096, d_p=4096, d_truth=4096, d_raw=4096), **kw})
    image = lambda **kw: sur.gradp_image_device(**{**dict(d_cols=4096, n_frames=2, k=5, d_grid=4096, d_truth=4096), **kw})
    for call in (step, image):
        for k in (4, 17):
            with pytest.raises(ValueError, match="5..16 columns"):
                call(k=k)
        for n in (0, 4):
            with pytest.raises(ValueError, match="n_frames"):
                call(n_frames=n)
        with pytest.raises(ValueError, match="d_cols"):
            call(d_cols=0)
        with pytest.raises(ValueError, match="d_truth"):
            call(d_truth=4100)
    for name, bad in (("d_raw", 4100), ("d_gradp", 4100), ("d_p", 4098)):
        with pytest.raises(ValueError, match=name):
            step(**{name: bad})
    with pytest.raises(ValueError, match="out_scale"):
        step(out_scale=[1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="bind_poststeps"):
        step(apply_filter=True)
    with pytest.raises(ValueError, match="d_grid"):
        image(d_grid=0)
    with pytest.raises(ValueError, match="d_grid"):
        image(d_grid=4098)
    ok = np.zeros((2, 11, 5))
    with pytest.raises(ValueError, match="5..16 columns"):
        sur.gradp_frames(ok[..., :4])
    with pytest.raises(ValueError, match=r"\[n,n_cells,k\]"):
        sur.gradp_frames(np.zeros((2, 3, 11, 5)))
    with pytest.raises(ValueError, match="11 cells"):
        sur.gradp_frames(np.zeros((2, 12, 5)))
    with pytest.raises(ValueError, match="n_frames"):
        sur.gradp_frames(np.zeros((4, 11, 5)))
    with pytest.raises(ValueError, match="out_scale"):
        sur.gradp_frames(ok, out_scale=[1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="bind_poststeps"):
        sur.gradp_frames(ok, apply_filter=True)
    sur.mesh_cells = None
    with pytest.raises(RuntimeError, match="no mesh"):
        sur.gradp_frames(ok)
    with pytest.raises(ValueError, match="max_frames"):
        EvaluationGradP(5e-3, 128, 96, 0.95, 0.95, "no.hdf5", "no.h5", 128, model=model2(), max_frames=0)
    ev = EvaluationGradP(5e-3, 128, 96, 0.95, 0.95, "no.hdf5", "no.h5", 128, model=model2(), max_frames=2)
    assert ev.max_frames == 2 and EvaluationGradP.max_frames == 1
    with pytest.raises(RuntimeError, match="computeOnlyOnce"):
        ev.timeSteps(0, [0, 1], fields=False)


# ------------------------------------------------------------------------------------------------------- GPU, the pack
@pytest.mark.gpu
def test_gpu_pack_is_the_host_statements_bit_for_bit():
    """Image and labels of psm_gradp_image_device against timeStep's NumPy statements on the planes psm_frames_to_grid_device wrote:
    bit for bit, for 1, 2 and 3 frames, behind leads of 4 and 5 elements (frames that start 16-byte aligned and frames that do not),
    with canaries in front of, behind and instead of the frames not asked for; without the labels the image is the same."""
    cols, sdf = stage_inputs()
    with surrogate2() as sur:
        d_cols = DeviceArray(cols)
        planes = device_planes(sur, d_cols)
        assert all(np.isnan(planes[:, c]).sum() > 100 for c in (2, 3, 4)) and not np.isnan(planes[:, :2]).any()
        want = [host_statements(planes[f], sdf) for f in range(NF)]
        assert (want[0][0][..., 2] == 0).sum() == 35 * 40 and all(np.isfinite(w[1]).all() for w in want)
        assert all(not np.array_equal(want[0][1][2], want[0][1][c] * MAXS[3 + c]) for c in (0, 1))     # label 2 is a plane of its own, undivided
        sizes, dtypes = (NPIX * 3, NPIX * 3), (np.float32, np.float64)
        starts = set()
        for lead in (4, 5):
            for n in (1, 2, NF):
                bufs = [DeviceArray(np.full(lead + NF * s + PAD, CANARY, dt)) for s, dt in zip(sizes, dtypes)]
                ptrs = [b.ptr + lead * np.dtype(dt).itemsize for b, dt in zip(bufs, dtypes)]
                starts |= {(dt.__name__, (p + f * s * np.dtype(dt).itemsize) % 16 == 0) for p, s, dt in zip(ptrs, sizes, dtypes) for f in range(n)}
                sur.gradp_image_device(d_cols.ptr, n, 5, *ptrs)
                sur.synchronize()
                same = []
                for q, (b, s) in enumerate(zip(bufs, sizes)):
                    a = b.numpy()
                    assert (a[:lead] == CANARY).all() and (a[lead + n * s:] == CANARY).all(), ("canary", lead, n, q)
                    got = a[lead:lead + n * s].reshape((n,) + want[0][q].shape)
                    same.append(all(same_bits(np.ascontiguousarray(got[f]), want[f][q]) for f in range(n)))
                print(f"lead {lead}, {n} frame(s): image / labels identical to the host statements {same}")
                assert all(same)
                free(*bufs)
        assert starts == {("float32", False), ("float32", True), ("float64", False), ("float64", True)}, starts
        d_g = DeviceArray(np.full((NF, NY, NX, 3), CANARY, np.float32))                  # the label planes are optional
        sur.gradp_image_device(d_cols.ptr, NF, 5, d_g.ptr)
        sur.synchronize()
        assert all(same_bits(d_g.numpy()[f], want[f][0]) for f in range(NF))
        free(d_cols, d_g)


# ------------------------------------------------------------------------------------------------------- GPU, the whole step
def raw_buffer():
    return DeviceArray(np.full(PAD + NF * ROWS * 8 + PAD, CANARY, np.float64))


def read_raw(d_raw, n=NF):
    a = d_raw.numpy()
    assert (a[:PAD] == CANARY).all() and (a[PAD + n * ROWS * 8:] == CANARY).all(), "canary round d_raw"
    return a[PAD:PAD + n * ROWS * 8].reshape(n, ROWS, 8).copy()


class StepOut:
    """Canary-framed destinations of one step; the gradient behind a lead of 2 * PAD floats (8-byte aligned), p behind PAD floats."""
    def __init__(self):
        self.g = DeviceArray(np.full(2 * PAD + NF * NPIX * 2 + PAD, CANARY, np.float32))
        self.p = DeviceArray(np.full(PAD + NF * NPIX + PAD, CANARY, np.float32))
        self.t = DeviceArray(np.full(PAD + NF * 3 * NPIX + PAD, CANARY, np.float64))
        self.raw = raw_buffer()
        self.p_g, self.p_p, self.p_t, self.p_raw = self.g.ptr + 2 * PAD * 4, self.p.ptr + PAD * 4, self.t.ptr + PAD * 8, self.raw.ptr + PAD * 8

    def read(self, n=NF):
        g, p, t = self.g.numpy(), self.p.numpy(), self.t.numpy()
        for a, lead, size in ((g, 2 * PAD, 2 * NPIX), (p, PAD, NPIX), (t, PAD, 3 * NPIX)):
            assert (a[:lead] == CANARY).all() and (a[lead + n * size:] == CANARY).all(), "canary round an output"
        return (g[2 * PAD:2 * PAD + n * NPIX * 2].reshape(n, NY, NX, 2).copy(), p[PAD:PAD + n * NPIX].reshape(n, NY, NX).copy(),
                t[PAD:PAD + n * 3 * NPIX].reshape(n, 3, NY, NX).copy(), read_raw(self.raw, n))

    def untouched(self):
        return all((d.numpy() == CANARY).all() for d in (self.g, self.p, self.t, self.raw))

    def free(self):
        free(self.g, self.p, self.t, self.raw)


def four_pairs(o):
    """The step's four pairs on its own outputs, as a caller of psm_field_errors_device states them."""
    p = (o.p_p, NPIX, 1, 1)
    gx, gy = (o.p_g, 2 * NPIX, 2, 1), (o.p_g + 4, 2 * NPIX, 2, 1)
    t0, t1, t2 = ((o.p_t + c * NPIX * 8, 3 * NPIX, 1, 0) for c in range(3))
    return [(p, t0, None, None, False), (p, t2, None, None, False), (gx, t0, None, None, False), (gy, t1, None, None, False)]


def numpy_rows(gradp, p, truth, flow):
    """The four rows in NumPy on the downloaded outputs -> (raw [n][4][8], {(f, q): (fsum d, sum |d|, fsum d^2)})."""
    n = p.shape[0]
    raw, sums = np.empty((n, ROWS, 8)), {}
    for f in range(n):
        for q, (pr, tr) in enumerate(((p[f], truth[f, 0]), (p[f], truth[f, 2]), (gradp[f, ..., 0], truth[f, 0]), (gradp[f, ..., 1], truth[f, 1]))):
            raw[f, q] = np_raw(pr, tr, flow)
            d = differences(pr, tr, flow)[2]
            sums[f, q] = (math.fsum(d), math.fsum(np.abs(d)), math.fsum(d * d))
    return raw, sums


def check_rows(got, want, sums, label):
    worst1 = worst2 = 0.0
    for (f, q), (s1, sabs, s2) in sums.items():
        g, w = got[f, q], want[f, q]
        assert same_bits(np.ascontiguousarray(g[list(EXACT)]), np.ascontiguousarray(w[list(EXACT)])), (label, f, q, g, w)
        e1, e2 = abs(g[S1] - s1), abs(g[S2] - s2)
        worst1, worst2 = max(worst1, e1 / sabs), max(worst2, e2 / g[S2])
        assert e1 <= SUM_TOL * sabs and e2 <= SUM_TOL * g[S2], (label, f, q, e1, sabs, e2, g[S2])
    return worst1, worst2


def bind_other_geometry(sur, sdf):
    g = np.zeros((NY, NX, 3), np.float32)                                          # the step solves its frames one by one: one case
    g[..., 2] = (np.roll(sdf, 11, axis=1) / MAXS[2]).astype(np.float32)
    assert sur.bind_geometry(g) and sur.geometry_bound


def oracle_chain(image, sdf):
    from oracle import psm_oracle as orc
    return orc.integrate_gradp(oracle_gradp(image, model2()), sdf, DX, DY, CUT[0], CUT[1])


@pytest.mark.gpu
def test_gpu_whole_step():
    """psm_gradp_frames_device, general and bound route, with and without the filter: a frame's gradient is solve (solve_poststeps)
    on its image, its p is integrate_gradp of that gradient after set_integration with the same cut, the label planes are the
    pack's, the four rows are psm_field_errors_device alone on the step's own outputs and NumPy's, the host entry returns the device
    entry's bits; one and two frames on the binding for three; the filter changes gradient, p and every row; the unfiltered p is
    within CHAIN_TOL of the float64 oracle chain; bound to another geometry the host entry takes one guard trip and returns the
    general route's bits."""
    cols, sdf = stage_inputs()
    sdn = sdf / MAXS[2]
    flow = sdn != 0
    with surrogate2(post=True) as sur:
        d_cols = DeviceArray(cols)
        image, truth = device_image(sur, d_cols)
        d_sdn = DeviceArray(sdn)
        chain = [oracle_chain(image[f], sdf) for f in range(NF)]
        sur.set_integration(sdf, CUT[0], CUT[1], DX, DY)
        kept = {}
        for route in ("general", "bound"):
            if route == "bound":
                assert sur.bind_geometry(image[0]) and sur.geometry_bound               # every frame carries the simulation's SDF channel
            for af in (False, True):
                o = StepOut()
                sur.gradp_frames_device(d_cols.ptr, NF, 5, o.p_g, o.p_p, o.p_t, o.p_raw, af)
                d_alone = raw_buffer()
                sur.field_errors_device((d_sdn.ptr, 0, 1, 0), four_pairs(o), NF, d_alone.ptr + PAD * 8)
                sur.synchronize()
                g, p, tr, raw = o.read()
                alone = read_raw(d_alone)
                h_g, h_p, h_tr, h_raw = sur.gradp_frames(cols, apply_filter=af)
                want_g = [sur.solve_poststeps(image[f], apply_filter=True)[0][0] if af else sur.solve(image[f])[0] for f in range(NF)]
                want_p = [sur.integrate_gradp(want_g[f]) for f in range(NF)]
                same = dict(gradient=all(same_bits(g[f], np.ascontiguousarray(want_g[f])) for f in range(NF)),
                            p=all(same_bits(p[f], want_p[f]) for f in range(NF)), truth=same_bits(tr, truth), raw_alone=same_bits(raw, alone),
                            host_gradient=same_bits(h_g, g), host_p=same_bits(h_p, p), host_truth=same_bits(h_tr, tr), host_raw=same_bits(h_raw, raw))
                want_raw, sums = numpy_rows(g, p, tr, flow)
                w1, w2 = check_rows(raw, want_raw, sums, (route, af))
                print(f"{route} apply_filter={af}: {same}; rows against NumPy: counts and extrema identical, |s1 - fsum| / sum|d| <= {w1:.2e}, "
                      f"|s2 - fsum| / s2 <= {w2:.2e} (bound {SUM_TOL}); n per row {raw[..., N_].astype(int).tolist()}, flow cells {int(flow.sum())}")
                assert all(same.values()) and np.isfinite(g).all() and np.isfinite(p).all()
                assert (raw[..., N_] == flow.sum()).all() and (raw[..., TNAN] == 0).all()
                if not af:
                    r = [ratio(p[f], chain[f]) for f in range(NF)]
                    print(f"{route}: max |p - oracle chain| / max |p| per frame {['%.2e' % v for v in r]} (bound {CHAIN_TOL})")
                    assert max(r) <= CHAIN_TOL
                only = sur.gradp_frames(cols, apply_filter=af, want_gradp=False, want_p=False, want_truth=False)
                assert only[0] is None and only[1] is None and only[2] is None and same_bits(only[3], raw)
                for n in (1, 2):                                                        # fewer frames on the binding for three
                    o2 = StepOut()
                    sur.gradp_frames_device(d_cols.ptr, n, 5, o2.p_g, o2.p_p, o2.p_t, o2.p_raw, af)
                    sur.synchronize()
                    part = o2.read(n)
                    ok = [same_bits(a, np.ascontiguousarray(b[:n])) for a, b in zip(part, (g, p, tr, raw))]
                    print(f"{route} apply_filter={af}: {n} frame(s) alone identical to the batch's first {n} {ok}")
                    assert all(ok)
                    o2.free()
                kept[route, af] = (g, p, raw)
                free(d_alone)
                o.free()
            (g0, p0, w0), (g1, p1, w1_) = kept[route, False], kept[route, True]
            assert not np.array_equal(g0, g1) and not np.array_equal(p0, p1)
            assert all(not np.array_equal(w0[:, q], w1_[:, q]) for q in range(ROWS))
        one = sur.gradp_frames(cols[1])                                               # one frame through the host entry
        assert one[1].shape == (1, NY, NX) and same_bits(one[1][0], kept["bound", False][1][1]) and same_bits(one[3][0], kept["bound", False][2][1])
        assert sur.guard_trips == 0 and sur.geometry_bound
        bind_other_geometry(sur, sdf)
        got = sur.gradp_frames(cols, apply_filter=True)
        ref_g, ref_p, ref_raw = kept["general", True]
        same = [same_bits(got[0], ref_g), same_bits(got[1], ref_p), same_bits(got[3], ref_raw)]
        print(f"bound to another geometry: guard trips {sur.guard_trips}, still bound {sur.geometry_bound}, gradient, p and rows identical "
              f"to the general route {same}")
        assert sur.guard_trips == 1 and not sur.geometry_bound and "not the one bound" in _lib.last_error(sur.h)
        assert all(same)
        free(d_cols, d_sdn)


# ------------------------------------------------------------------------------------------------------- GPU, the tables
@pytest.mark.gpu
def test_gpu_integration_tables_are_the_bindings_own():
    """After bind_gradp_frames psm_integrate_gradp_device still has no binding; a bind_integration and a set_integration with
    another cut, done afterwards, leave the step's p unchanged, and the step leaves theirs alone."""
    cols, sdf = stage_inputs()
    with surrogate2() as sur:
        d_cols = DeviceArray(cols)
        o = StepOut()
        rc = sur.lib.psm_integrate_gradp_device(sur.h, o.p_g, NF, o.p_p, None)
        print(f"psm_integrate_gradp_device after bind_gradp_frames alone: {rc}, '{_lib.last_error(sur.h)}'")
        assert rc == -2 and "psm_bind_integration has not been called" in _lib.last_error(sur.h)
        sur.synchronize()
        assert o.untouched()
        before = sur.gradp_frames(cols)
        assert sur.bind_integration(np.stack([sdf] * NF), [40] * NF, [50] * NF, DX, DY)
        after_bind = sur.gradp_frames(cols)
        sur.set_integration(sdf, 20, 50, DX, DY)
        after_set = sur.gradp_frames(cols)
        same = [all(same_bits(a, b) for a, b in zip(before, x)) for x in (after_bind, after_set)]
        print(f"the step's outputs after bind_integration(cut (40, 50)) / set_integration(cut (20, 50)) identical to before {same}")
        assert all(same)
        # the other two bindings still integrate at their own cuts: not the step's p
        d_g = DeviceArray(before[0])
        sur.integrate_device(d_g.ptr, NF, o.p_p)
        sur.synchronize()
        p40 = o.p.numpy()[PAD:PAD + NF * NPIX].reshape(NF, NY, NX)
        p20 = sur.integrate_gradp(before[0][0])
        differ = [not np.array_equal(p40, before[1]), not np.array_equal(p20, before[1][0])]
        print(f"bind_integration's and set_integration's own p differ from the step's {differ}")
        assert all(differ)
        d_g.free()
        o.free()
        free(d_cols)


# ------------------------------------------------------------------------------------------------------- GPU, errors
@pytest.mark.gpu
def test_gpu_error_returns_enqueue_nothing_and_leave_the_handle_usable():
    """Frames, gradP frames or post-steps unbound; a one-channel-field model; bad scales; a cut the reference raises on; k = 4 and
    17; n_frames 0 and 4; a NULL d_cols; misaligned destinations: each returns its code, the outputs keep their sentinels, and the
    handle then runs a step bit-identical to the one before.  bind_frames and unbind_gradp_frames drop the binding."""
    cols, sdf = stage_inputs()
    t = flow_tables()
    mx = np.array(MAXS, np.float64)
    with GridSurrogate(synthetic.make_model("deltas", p_in=32, p_out=32), NY, NX, max_cases=NF) as one:
        one.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        one.bind_frames(NF, 5)
        rc = one.lib.psm_bind_gradp_frames(one.h, sdf.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), CUT[0], CUT[1], DX, DY)
        assert rc == -2 and "c_out == 2" in _lib.last_error(one.h)
    with surrogate2(bind=False) as sur:
        d_cols = DeviceArray(cols)
        o = StepOut()
        d_grid = DeviceArray(np.full((NF, NY, NX, 3), CANARY, np.float32))
        lib, h = sur.lib, sur.h
        c_bind = lambda m=mx, s=sdf, cut=CUT: lib.psm_bind_gradp_frames(h, s.ctypes.data_as(_dp) if s is not None else None, m.ctypes.data_as(_dp),
                                                                         cut[0], cut[1], DX, DY)
        c_step = lambda n=NF, k=5, af=0, cols_=d_cols.ptr, g=o.p_g, p=o.p_p, tr=o.p_t, raw=o.p_raw: lib.psm_gradp_frames_device(
            h, cols_, n, k, None, af, g, p, tr, raw, None)
        c_image = lambda n=NF, k=5, cols_=d_cols.ptr, grid=d_grid.ptr, tr=o.p_t: lib.psm_gradp_image_device(h, cols_, n, k, grid, tr, None)
        host_raw = np.full((NF, ROWS, 8), CANARY)
        c_host = lambda n=NF, k=5, af=0, raw=host_raw: lib.psm_gradp_frames(h, cols.ctypes.data_as(_dp), n, k, None, af, None, None, None,
                                                                             raw.ctypes.data_as(_dp) if raw is not None else None)
        last = lambda: _lib.last_error(h)
        assert c_bind() == -2 and "psm_bind_frames" in last()
        assert c_step() == -2 and "psm_bind_frames" in last() and c_image() == -2 and c_host() == -2
        sur.bind_frames(NF, 5)
        assert c_step() == -2 and "psm_bind_gradp_frames" in last() and c_image() == -2 and c_host() == -2
        for bad in ((1.0, 1.0, 0.0, 1.0, 1.0), (np.inf, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0, np.nan)):
            assert c_bind(m=np.array(bad)) == -1 and "finite and non-zero" in last()
        assert c_bind(s=None) == -1 and c_step() == -2
        assert c_bind(cut=(57, 30)) == -5 and "flow-cell counts" in last()            # the reference raises: nothing is bound
        assert c_step() == -2 and "psm_bind_gradp_frames" in last()
        assert c_bind(cut=(NY, 50)) == -1 and c_step() == -2
        assert c_bind() == 0
        sur._gradp_bound = True                                                   # bound through the C entry: tell the mirror
        first = sur.gradp_frames(cols)
        assert c_bind(cut=(57, 30)) == -5 and c_step() == -2                        # a refused bind leaves nothing bound either
        assert c_bind() == 0
        assert c_step(af=1) == -2 and "psm_bind_poststeps" in last() and c_host(af=1) == -2 and "psm_bind_poststeps" in last()
        for k in (4, 17):
            assert c_step(k=k) == -1 and "[5, 16]" in last() and c_image(k=k) == -1 and c_host(k=k) == -1
        for n in (0, NF + 1):
            assert c_step(n=n) == -1 and "n_frames" in last() and c_image(n=n) == -1 and c_host(n=n) == -1
        assert c_step(cols_=None) == -1 and c_image(cols_=None) == -1 and c_image(grid=None) == -1 and c_image(grid=d_grid.ptr + 2) == -1
        assert c_step(g=o.p_g + 4) == -1 and "misaligned" in last() and c_step(p=o.p_p + 2) == -1 and c_step(tr=o.p_t + 4) == -1
        assert c_step(raw=o.p_raw + 4) == -1 and c_image(tr=o.p_t + 4) == -1
        assert c_host(raw=None) == -1 and c_host(k=6) == -1 and "reserved staging" in last()
        sur.synchronize()
        assert o.untouched() and (d_grid.numpy() == CANARY).all() and (host_raw == CANARY).all()
        # the handle still works: the device entry and the host entry give the first step's bits
        assert c_step() == 0
        sur.synchronize()
        g, p, tr, raw = o.read()
        again = sur.gradp_frames(cols)
        same = [all(same_bits(a, b) for a, b in zip(again, first)), all(same_bits(a, b) for a, b in zip((g, p, tr, raw), first))]
        print(f"after the refused calls: the host entry and the device entry identical to the step before them {same}")
        assert all(same) and (raw[..., N_] > 0).all()
        sur.unbind_gradp_frames()
        assert c_step() == -2 and "psm_bind_gradp_frames" in last()
        assert sur.bind_gradp_frames(sdf, MAXS, CUT[0], CUT[1], DX, DY)
        assert sur.bind_gradp_frames(sdf, MAXS, 57, 30, DX, DY) is False and not sur._gradp_bound
        assert sur.bind_gradp_frames(sdf, MAXS, CUT[0], CUT[1], DX, DY)
        sur.bind_frames(NF, 5)                                                   # a new frame binding drops it again
        assert not sur._gradp_bound and c_step() == -2 and "psm_bind_gradp_frames" in last()
        o.free()
        free(d_cols, d_grid)


# ------------------------------------------------------------------------------------------------------- GPU, the evaluator
@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gradp_frames"))
    c = cases.build_gradp_dataset_case(d)
    c["dir"] = d
    return c


def evaluator(c, **kw):
    return EvaluationGradP(5e-3, 128, 96, 0.95, 0.95, c["dataset_path"], c["model_path"], 128, artifact_dir=c["dir"], **kw)


TIMES = [0, 1, 1, 0, 1]
LISTS = ("pred_minus_true", "pred_minus_true_squared")


def reference_sweep(ds, general, apply_filter=False):
    ref = evaluator(ds)
    assert ref.computeOnlyOnce(0) == 0 and (ref.grid_shape_y, ref.grid_shape_x) == (320, 300)
    if general:
        ref._sur.unbind_geometry()
    fields, metrics = [], []
    for time in TIMES:
        fields.append(ref.timeStep(0, time, apply_filter=apply_filter))
        metrics.append({k: dict(v) for k, v in ref.last_metrics.items()})
    return ref, fields, metrics


def sweep(ds, general, apply_filter=False, modes=(True, False)):
    """timeSteps(0, TIMES) with max_frames = 2 (chunks of 2, 2 and 1), with and without fields, against five timeStep calls of a
    second evaluator: p images bit for bit, accumulators and the 'reference' and 'p' metrics equal with fields, within
    compare_metrics' bounds from the device sums."""
    ref, want_fields, want_m = reference_sweep(ds, general, apply_filter)
    for mode in modes:
        ev = evaluator(ds, max_frames=2)
        assert ev.computeOnlyOnce(0) == 0
        if general:
            ev._sur.unbind_geometry()
        out = ev.timeSteps(0, TIMES, apply_filter=apply_filter, fields=mode)
        assert len(out) == 5 and len(ev.frame_metrics) == 5 and ev._sur.max_cases == 2 and ev._sur.guard_trips == 0
        assert ev._sur.geometry_bound == (not general) and ref._sur.geometry_bound == (not general)
        assert set(ev.last_metrics) == {"reference", "p", "dp_dx", "dp_dy"}
        for name in LISTS:
            assert len(getattr(ev, name)) == len(getattr(ref, name)) == 5, name
        if mode:
            same = [same_bits(out[i], want_fields[i]) for i in range(5)]
            lists = [getattr(ev, name) == getattr(ref, name) for name in LISTS]
            last = [ev.last_metrics[k] == want_m[4][k] for k in ("reference", "p")]
            kept = [same_bits(np.ascontiguousarray(ev.gradP), np.ascontiguousarray(ref.gradP)), np.array_equal(ev.no_flow_bool, ref.no_flow_bool),
                    ev.U_max_norm == ref.U_max_norm, (ev.center_p_y, ev.center_p_x) == (ref.center_p_y, ref.center_p_x)]
            print(f"general={general} apply_filter={apply_filter} fields=True: p images identical to timeStep's {same}, accumulators equal {lists}, "
                  f"last_metrics reference / p equal {last}, gradP / no_flow_bool / U_max_norm / cut as timeStep leaves them {kept}")
            assert all(same) and all(lists) and all(last) and all(kept)
            for i in range(5):
                assert ev.frame_metrics[i]["reference"] == want_m[i]["reference"] and ev.frame_metrics[i]["p"] == want_m[i]["p"]
        else:
            for i in range(5):
                assert set(out[i]) == {"reference", "p", "dp_dx", "dp_dy"}
                for key in ("reference", "p"):
                    compare_metrics(out[i][key], want_m[i][key], f"general={general} apply_filter={apply_filter} fields=False frame {i} {key}")
            for name in LISTS:
                a, b = getattr(ev, name), getattr(ref, name)
                for i in range(5):
                    rmse = want_m[i]["reference"]["rmseNorm"]
                    print(f"fields=False {name}[{i}]: |difference| / (rmseNorm / 100) = {abs(a[i] - b[i]) / (rmse / 100):.2e} (bound 1e-9)")
                    assert abs(a[i] - b[i]) <= 1e-9 * rmse / 100, (name, i, a[i], b[i])
        # the two additional rows: the assembled gradient against its labels, finite and the same whichever way the frame was batched
        for i in range(5):
            for key in ("dp_dx", "dp_dy"):
                assert all(math.isfinite(ev.frame_metrics[i][key][k]) for k in ("normVal", "biasNorm", "rmseNorm", "mean_err", "mean_sq_err"))
            assert ev.frame_metrics[i]["dp_dx"] == ev.frame_metrics[TIMES.index(TIMES[i])]["dp_dx"]
    return ref


@pytest.mark.gpu
def test_gpu_evaluator_time_steps_bound(ds):
    """The sweep as the evaluators come, geometry bound for one case, then once with the filter; main_gradP(frames_per_call=2,
    fields=False, n_ts=2) gives the "for the sim" summary of main_gradP(n_ts=2)."""
    sweep(ds, general=False)
    sweep(ds, general=False, apply_filter=True)
    kw = dict(delta=5e-3, model_directory=ds["model_path"], shape=128, var_p=0.95, var_in=0.95, max_number_PC=128, hdf5_path=ds["dataset_path"],
              artifact_dir=ds["dir"], n_ts=2)
    want = main_gradP(**kw)
    got = main_gradP(**kw, frames_per_call=2, fields=False)
    assert len(got["sims"]) == len(want["sims"]) == 1 and len(got["frames"]) == len(want["frames"]) == 2
    assert [(f["sim"], f["time"]) for f in got["frames"]] == [(0, 0), (0, 1)] and set(got["frames"][0]) >= {"reference", "p", "dp_dx", "dp_dy"}
    g, w = got["sims"][0], want["sims"][0]
    worst = max(abs(g["BIAS"] - w["BIAS"]) / w["RMSE"], abs(g["RMSE"] - w["RMSE"]) / w["RMSE"])
    stde = abs(g["STDE"] - w["STDE"]) / abs(w["STDE"])
    print(f"main_gradP(frames_per_call=2, fields=False) against the default call: worst BIAS / RMSE difference {worst:.2e} of RMSE (bound 1e-9), "
          f"STDE {stde:.2e} relative (bound 1e-8)\n  got  {g}\n  want {w}")
    assert worst <= 1e-9 and stde <= 1e-8
    for i in range(2):
        for key in ("reference", "p"):
            compare_metrics(got["frames"][i][key], want["frames"][i][key], f"main_gradP frame {i} {key}")


@pytest.mark.gpu
def test_gpu_evaluator_time_steps_general(ds):
    """The sweep with both evaluators on the general route (unbind_geometry after computeOnlyOnce)."""
    sweep(ds, general=True)
