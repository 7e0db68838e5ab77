"""A frame's dataset rows in, per-frame scalars and columns on the device (csrc/psm_rows.hip, csrc/psm_api_rows.cpp).

The stage alone is held to the host statements of the three evaluators' ``_frame_prepare`` (evaluators.py: what ``timeStep`` and
``timeSteps`` both run on a frame's rows) and of their ``_host_call`` (U^2, the out-scale), quoted below and executed on the same float32 rows: columns and scalars bit for bit (uint64 views, NaN positions included).  Shapes are the smallest that
can go wrong.  The partial launch gives every workgroup 256 cells per pass and at most 256 workgroups per frame; the finish
launch writes 256 cells per workgroup and folds the frame's partials with 256 threads (4 waves):
    1      one cell: 255 idle threads, one partial
    255    one workgroup with its last thread idle
    256    exactly one workgroup
    257    a second workgroup (second partial) with one cell
    513    three partials, the last with one cell
    4097   17 partials: more than a quarter of a wave in the finish fold, one cell in the last workgroup
    65793  = 256 * 257 + 1: the cap of 256 partials (all four waves of the finish fold) and a second pass of the partial
           launch's stride with one cell
Frames: 1 and 3 per call; the maximum sits in the last cell of the last chunk in frame 0 and in cell 0 in frame 1; frame 2 has
a NaN in Ux (U = NaN: relevant, NaN columns).  Rows 11 (not 8-byte aligned) and 12 floats wide, and a rows pointer 4 bytes off.
U^2: the kernels take U * U in float32 where the host writes pow(U, 2.0); test_square_is_the_float32_product asserts on the CPU
that the two agree for every U of this file (libm's powf is within 1 ulp, not correctly rounded: on 300 000 random float32 values
it differed from the product 192 times).

The whole steps: ``timeSteps(device_prep=True)`` against ``device_prep=False`` on the same evaluator, handle and library -- only
the source of the columns and scalars differs, so returned fields / metrics, raw sums, U_max_norm and the recorded lists must be
bit for bit equal; an irrelevant middle frame; frame independence; error returns that enqueue nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import test_deltas_frames as tdf
import test_gradp_frames as tgf
import test_poisson_frames as tpf
from hipmem import DeviceArray
from psm_amd import GridSurrogate, formats
from test_poisson_frames import same_bits

CELLS = (1, 255, 256, 257, 513, 4097, 65793)
MESH_CELLS = max(CELLS)
KINDS = {"deltas": (0, 3), "poisson": (1, 8), "gradp": (2, 5)}
BASE = {"deltas": cases.DATASET_MAXS[3], "poisson": cases.POISSON_MAXS[4], "gradp": 1.0}
EX, EY = np.float32(1.4500001), np.float32(0.62999994)          # max_x - min_x, max_y - min_y as EvaluationGradP holds them
PHI = 0.16
CANARY = -7.25e300
_dp, _fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


# ------------------------------------------------------------------------------------------- the host statements (the specification)
def host_deltas(d, base):
    """Evaluation._frame_prepare(d, full=False) and the scalars of _host_call: -> (cols [n,3] float64, scalars [8])."""
    Ux, Uy = d[:, 0:1], d[:, 1:2]
    delta_U, delta_p = d[:, 5:7], d[:, 7:8]
    U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
    deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
    if (deltaU_max_norm / U_max_norm) < 1e-4:
        return np.zeros((d.shape[0], 3)), [1.0, float(deltaU_max_norm), 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    cols = np.concatenate([delta_U / U_max_norm, delta_p / pow(U_max_norm, 2.0)], axis=1).astype(np.float64)
    U2, scale = float(pow(U_max_norm, 2.0)), base * U_max_norm ** 2
    assert isinstance(scale, np.float32)                       # NumPy 2: a Python float times a float32 scalar stays float32
    return cols, [float(U_max_norm), float(deltaU_max_norm), 0.0, 1.0, U2, float(scale), 0.0, 0.0]


def host_poisson(d, base):
    """EvaluationPoisson._frame_prepare and the scalars of _host_call: -> (cols [n,8] float64, scalars [8])."""
    Ux, Uy, p = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    delta_U, delta_p = d[:, 5:7], d[:, 7:8]
    delta_U_prev, delta_p_prev = d[:, 8:10], d[:, 10:11]
    deltaU_changed = np.abs(delta_U - delta_U_prev).sum(axis=-1)
    c = deltaU_changed.max()
    deltaU_changed = deltaU_changed / deltaU_changed.max()
    U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
    deltaU_max_norm = np.max(np.sqrt(np.square(delta_U[:, 0:1]) + np.square(delta_U[:, 1:2])))
    if (deltaU_max_norm / U_max_norm) < 1e-4 or deltaU_max_norm < 1e-6 or U_max_norm < 1e-6:
        return np.zeros((d.shape[0], 8)), [1.0, float(deltaU_max_norm), float(c), 0.0, 1.0, 0.0, 0.0, 0.0]
    cols = np.concatenate([Ux, Uy, delta_U, delta_p, p, deltaU_changed[:, None], delta_p_prev], axis=1).astype(np.float64)
    U = float(U_max_norm)
    return cols, [U, float(deltaU_max_norm), float(c), 1.0, float(pow(U_max_norm, 2.0)), base * U ** 2, 0.0, 0.0]


def host_gradp(d, ex, ey):
    """EvaluationGradP._frame_prepare, with max_x - min_x = ex and max_y - min_y = ey as float32 scalars."""
    assert isinstance(ex, np.float32) and isinstance(ey, np.float32)
    Ux, Uy, p, dPdx, dPdy = d[:, 0:1], d[:, 1:2], d[:, 2:3], d[:, 6:7], d[:, 7:8]
    U_max_norm = np.max(np.sqrt(np.square(Ux) + np.square(Uy)))
    cols = np.concatenate([Ux / U_max_norm, Uy / U_max_norm, dPdx * ex / pow(U_max_norm, 2.0), dPdy * ey / pow(U_max_norm, 2.0),
                           p / pow(U_max_norm, 2.0)], axis=1)
    assert cols.dtype == np.float32                            # every statement stays in float32; the cast is the last step
    return cols.astype(np.float64), [float(U_max_norm), 0.0, 0.0, 1.0, float(pow(U_max_norm, 2.0)), 1.0, 0.0, 0.0]


def host_frames(kind, rows):
    with np.errstate(all="ignore"):
        out = [host_deltas(d, BASE[kind]) if kind == "deltas" else host_poisson(d, BASE[kind]) if kind == "poisson" else host_gradp(d, EX, EY)
               for d in rows]
    return np.stack([c for c, _ in out]), np.array([s for _, s in out], np.float64)


def make_rows(kind, n_frames, n_cells, width, seed=0):
    """[n_frames][n_cells][width] float32 with the planted cases of the module docstring."""
    rng = np.random.default_rng(1000 * n_cells + 10 * width + n_frames + seed)
    r = rng.standard_normal((n_frames, n_cells, width)).astype(np.float32)
    r[..., 5:7] *= np.float32(0.05)
    r[..., 8:10] *= np.float32(0.05)
    r[0, n_cells - 1, 0:2] = (np.float32(7.1234565), np.float32(-3.3))          # the last cell of the last chunk
    r[0, n_cells - 1, 5:7] = (np.float32(0.71), np.float32(0.69))
    r[0, n_cells - 1, 8:10] = (np.float32(-0.5), np.float32(-0.4))
    if n_frames > 1:
        r[1, 0, 0:2] = (np.float32(-6.7), np.float32(5.4321))                    # cell 0
        r[1, 0, 5:7] = (np.float32(-0.9), np.float32(0.31))
        r[1, 0, 8:10] = (np.float32(0.6), np.float32(-0.7))
    if n_frames > 2:
        r[2, n_cells // 2, 0] = np.nan
    return r


def every_test_frame():
    for kind in KINDS:
        for n_cells in CELLS:
            for width in (11, 12):
                for n_frames in (1, 3):
                    yield kind, make_rows(kind, n_frames, n_cells, width)
    for kind, rows, _ in threshold_frames():
        yield kind, rows


def threshold_frames():
    """(kind, rows [n][300][11], expected relevant flags): the skip rule at its edges.  U = 1 exactly, so dU / U = dU."""
    def frame(U, dU):
        d = np.zeros((300, 11), np.float32)
        d[:, 0] = np.float32(U) * np.linspace(0.5, 1.0, 300).astype(np.float32)
        d[:, 5] = np.float32(dU) * np.linspace(0.25, 1.0, 300).astype(np.float32)
        d[:, 7] = np.linspace(-1, 1, 300).astype(np.float32)
        d[:, 8] = np.float32(0.5 * dU)
        d[:, 2] = d[:, 10] = 0.125
        return d
    below, above = frame(1.0, 9.9e-5), frame(1.0, 1.01e-4)
    yield "deltas", np.stack([below, above, frame(1.0, 0.5)]), [0, 1, 1]
    yield "poisson", np.stack([below, above, frame(5e-7, 2e-6)]), [0, 1, 0]      # the last one: U < 1e-6 alone decides
    yield "poisson", np.stack([frame(1e-3, 5e-7), frame(1.0, 0.5)]), [0, 1]      # dU < 1e-6 alone decides


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_square_is_the_float32_product():
    """Before relying on U * U for pow(U, 2.0) and U ** 2: the two agree in float32 for every U this file uses (the dataset frames of
    the whole-step tests are checked there).  Where they did not, the host statement would win."""
    n = 0
    for kind, rows in every_test_frame():
        for d in rows:
            with np.errstate(all="ignore"):
                U = np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))
            if np.isnan(U):
                continue
            assert isinstance(U, np.float32) and pow(U, 2.0) == U * U and U ** 2 == U * U, (kind, U)
            n += 1
    assert n > 100


def test_threshold_frames_fall_on_one_side_in_both_precisions():
    """The frames just below and just above dU / U = 1e-4: the float32 quotient against float32(1e-4) and the float64 quotient
    against 1e-4 decide alike, so the test does not hang on which of the two the comparison is made in."""
    at_the_edge = 0
    for kind, rows, want in threshold_frames():
        got = host_frames(kind, rows)[1][:, 3]
        assert list(got) == want, (kind, got)
        for d, rel in zip(rows, want):
            U = np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))
            dU = np.max(np.sqrt(np.square(d[:, 5:6]) + np.square(d[:, 6:7])))
            q32, q64 = dU / U, float(dU) / float(U)
            assert isinstance(q32, np.float32)
            if abs(q64 - 1e-4) < 2e-6:                           # the two frames of a set that sit at the edge of the rule
                assert (q32 < np.float32(1e-4)) == (q64 < 1e-4) == (not rel), (q32, q64)
                at_the_edge += 1
    assert at_the_edge == 4


# ------------------------------------------------------------------------------------------------------- GPU, the stage alone
@pytest.fixture(scope="module")
def stage():
    """A handle with a mesh of MESH_CELLS cells (random tables: the stage reads none of them), 3 frame slots of 8 columns and
    rows staging."""
    ny, nx = 130, 131
    ng = ny * nx
    rng = np.random.default_rng(77)
    vtx = rng.integers(0, MESH_CELLS, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    wts = np.ascontiguousarray(np.c_[w, 1.0 - w.sum(axis=1)])
    cell = np.arange(ng)
    indices = np.c_[cell // nx, cell % nx].astype(np.int32)
    sur = GridSurrogate(tdf.model3(), ny, nx, max_cases=3)
    sur.set_mesh(vtx, wts, indices, np.ones((ny, nx)), MESH_CELLS)
    sur.bind_frames(3, 8)
    sur.bind_rows(12)
    yield sur
    sur.close()


def run_stage(sur, kind, rows, offset=False):
    """The stage on `rows` -> (cols, scalars); the buffers carry a canary behind their ends.  offset: the rows start 4 bytes into
    their buffer."""
    n, n_cells, width = rows.shape
    k = KINDS[kind][1]
    flat = np.concatenate([np.full(1 if offset else 0, 3.5e30, np.float32), rows.reshape(-1)])
    d_rows = DeviceArray(flat)
    d_cols = DeviceArray(np.full(n * n_cells * k + 4, CANARY, np.float64))
    d_sc = DeviceArray(np.full(n * 8 + 4, CANARY, np.float64))
    try:
        sur.rows_prepare_device(kind, d_rows.ptr + (4 if offset else 0), n, n_cells, width, d_cols.ptr, d_sc.ptr, base=BASE[kind], phi=PHI,
                                ex=float(EX), ey=float(EY))
        sur.synchronize()
        cols, sc = d_cols.numpy(), d_sc.numpy()
    finally:
        for a in (d_rows, d_cols, d_sc):
            a.free()
    assert np.all(cols[-4:] == CANARY) and np.all(sc[-4:] == CANARY), "the stage wrote behind the end of a buffer"
    return cols[:-4].reshape(n, n_cells, k), sc[:-4].reshape(n, 8)


def differing(got, want):
    """Elements whose bits differ: array_equal on the uint64 views, a NaN matching a NaN in the same position whatever its payload."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    both_nan = np.isnan(got) & np.isnan(want)
    return int(((got.view(np.uint64) != want.view(np.uint64)) & ~both_nan).sum())


def check_stage(sur, kind, rows, label, offset=False):
    want_cols, want_sc = host_frames(kind, rows)
    cols, sc = run_stage(sur, kind, rows, offset)
    bad_c, bad_s = differing(cols, want_cols), differing(sc, want_sc)
    print(f"{label}: {bad_c} of {cols.size} column values and {bad_s} of {sc.size} scalars differ in their bits; scalars {sc.tolist()}")
    if bad_s:
        print("  host scalars", want_sc.tolist())
    assert bad_s == 0 and bad_c == 0, label
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", CELLS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_stage_alone_is_the_host_statements_bit_for_bit(stage, kind, n_cells):
    for width in (11, 12):
        for n_frames in (1, 3):
            rows = make_rows(kind, n_frames, n_cells, width)
            # the planted maxima are where the docstring says (frame 2 holds a NaN: no argmax)
            speed = np.hypot(rows[..., 0].astype(np.float64), rows[..., 1])
            assert int(np.argmax(speed[0])) == n_cells - 1 and (n_frames == 1 or int(np.argmax(speed[1])) == 0)
            sc = check_stage(stage, kind, rows, f"{kind} {n_frames} x {n_cells} x {width}")
            assert list(sc[:, 3]) == [1.0] * n_frames
            if n_frames == 3:
                assert np.isnan(sc[2, 0]) and sc[2, 3] == 1.0          # a NaN maximum: every comparison false, relevant
        check_stage(stage, kind, make_rows(kind, 3, n_cells, width), f"{kind} 3 x {n_cells} x {width}, rows 4 bytes off", offset=True)


@pytest.mark.gpu
def test_gpu_stage_skip_rule_at_its_edges(stage):
    for kind, rows, want in threshold_frames():
        sc = check_stage(stage, kind, rows, f"{kind} thresholds")
        assert list(sc[:, 3]) == want
        for f, rel in enumerate(want):
            if not rel:
                assert sc[f, 0] == 1.0 and sc[f, 4] == 1.0 and sc[f, 5] == 0.0


@pytest.mark.gpu
def test_gpu_stage_into_the_bindings_buffers_and_on_fewer_cells(stage):
    """d_cols = d_scalars = 0: the frame binding's column buffer and the binding's slots; the stage is deterministic: twice the
    same bits."""
    rows = make_rows("poisson", 2, 513, 11)
    d_rows = DeviceArray(rows)
    try:
        stage.rows_prepare_device("poisson", d_rows.ptr, 2, 513, 11, base=BASE["poisson"])
        stage.synchronize()
    finally:
        d_rows.free()
    a, b = run_stage(stage, "poisson", rows), run_stage(stage, "poisson", rows)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])           # run to run: the very same bits


ARG, STATE = -1, -2


@pytest.mark.gpu
def test_gpu_error_returns_enqueue_nothing_and_leave_the_handle_usable(stage):
    sur, lib = stage, stage.lib
    rows = make_rows("deltas", 2, 257, 11)
    want_cols, want_sc = host_frames("deltas", rows)
    d_rows = DeviceArray(np.concatenate([rows.reshape(-1), np.zeros(8, np.float32)]))
    d_cols = DeviceArray(np.full(2 * 257 * 8 + 2, CANARY, np.float64))
    d_sc = DeviceArray(np.full(2 * 8 + 2, CANARY, np.float64))
    params = np.array([BASE["deltas"], PHI, 1.0, 1.0])
    pp = lambda a: a.ctypes.data_as(_dp)

    def call(kind=0, rows_ptr=None, n=2, n_cells=257, width=11, par=params, cols_ptr=None, sc_ptr=None):
        return lib.psm_rows_prepare_device(sur.h, kind, C.c_void_p(d_rows.ptr if rows_ptr is None else rows_ptr), n, n_cells, width, pp(par),
                                           C.c_void_p(d_cols.ptr if cols_ptr is None else cols_ptr),
                                           C.c_void_p(d_sc.ptr if sc_ptr is None else sc_ptr), None)

    def untouched(label):
        sur.synchronize()
        assert np.all(d_cols.numpy() == CANARY) and np.all(d_sc.numpy() == CANARY), f"{label}: something was enqueued"

    def valid(label):
        assert call() == 0, sur.lib.psm_last_error(sur.h)
        sur.synchronize()
        cols, sc = d_cols.numpy()[:2 * 257 * 3].reshape(2, 257, 3), d_sc.numpy()[:16].reshape(2, 8)
        assert differing(cols, want_cols) == 0 and differing(sc, want_sc) == 0, label
        for a in (d_cols, d_sc):                                   # the canaries again
            assert lib.psm_debug_copy_to_device(a.ptr, np.full(a.shape, CANARY, np.float64).ctypes.data, a.nbytes) == 0

    try:
        bad = {"width 7": dict(width=7), "width 17": dict(width=17), "deltas rows 10 wide": dict(width=10), "Poisson rows 8 wide": dict(kind=1, width=8),
               "kind 3": dict(kind=3), "kind -1": dict(kind=-1), "no frame": dict(n=0), "more frames than bound": dict(n=4),
               "no cell": dict(n_cells=0), "more cells than the mesh": dict(n_cells=MESH_CELLS + 1), "rows NULL": dict(rows_ptr=0),
               "rows 2 bytes off": dict(rows_ptr=d_rows.ptr + 2), "columns 4 bytes off": dict(cols_ptr=d_cols.ptr + 4),
               "scalars 4 bytes off": dict(sc_ptr=d_sc.ptr + 4), "base 0": dict(par=np.array([0.0, PHI, 1, 1])),
               "base NaN": dict(par=np.array([np.nan, PHI, 1, 1])), "base inf": dict(par=np.array([np.inf, PHI, 1, 1])),
               "ex NaN": dict(kind=2, par=np.array([1.0, PHI, np.nan, 1]))}
        for label, kw in bad.items():
            assert call(**kw) == ARG, label
            assert sur.lib.psm_last_error(sur.h), label
        assert lib.psm_rows_prepare_device(sur.h, 0, C.c_void_p(d_rows.ptr), 2, 257, 11, None, C.c_void_p(d_cols.ptr), C.c_void_p(d_sc.ptr), None) == ARG
        assert lib.psm_bind_rows(sur.h, 7) == ARG and lib.psm_bind_rows(sur.h, 17) == ARG
        untouched("argument errors")
        valid("after the argument errors")
        # the whole steps name the binding that is missing; wider rows than the staging are refused by the host forms
        raw, scal = np.zeros((2, 2, 8)), np.zeros((2, 8))
        assert lib.psm_deltas_rows_device(sur.h, C.c_void_p(d_rows.ptr), 2, 11, BASE["deltas"], 0, None, None, None, None, None) == STATE
        assert b"psm_bind_deltas_frames" in sur.lib.psm_last_error(sur.h)
        assert lib.psm_gradp_rows_device(sur.h, C.c_void_p(d_rows.ptr), 2, 11, 1.0, 1.0, 0, None, None, None, None, None, None) == STATE
        assert b"psm_bind_gradp_frames" in sur.lib.psm_last_error(sur.h)
        assert lib.psm_poisson_rows_errors_device(sur.h, C.c_void_p(d_rows.ptr), 2, 11, 1.0, PHI, 0, 1, None, None, None, None, pp(raw), None, None) == STATE
        assert b"psm_bind_features" in sur.lib.psm_last_error(sur.h)
        host_rows = np.zeros((2, MESH_CELLS, 13), np.float32)
        assert lib.psm_deltas_rows(sur.h, host_rows.ctypes.data_as(_fp), 2, 13, BASE["deltas"], 0, None, None, pp(raw), pp(scal)) == ARG
        assert lib.psm_deltas_rows(sur.h, host_rows.ctypes.data_as(_fp), 2, 11, 0.0, 0, None, None, pp(raw), pp(scal)) == ARG
        assert lib.psm_deltas_rows(sur.h, host_rows.ctypes.data_as(_fp), 2, 11, BASE["deltas"], 0, None, None, pp(raw), pp(scal)) == STATE
        untouched("state errors of the steps")
        # without the rows binding, and without the frame binding under it
        sur.unbind_rows()
        assert call() == STATE and b"psm_bind_rows" in sur.lib.psm_last_error(sur.h)
        sur.bind_rows(12)
        valid("after unbind_rows / bind_rows")
        sur.unbind_frames()                                        # drops the rows binding with it
        assert call() == STATE and b"psm_bind_frames" in sur.lib.psm_last_error(sur.h)
        assert lib.psm_bind_rows(sur.h, 12) == STATE
        sur.bind_frames(3, 8)
        assert call() == STATE and b"psm_bind_rows" in sur.lib.psm_last_error(sur.h)
        untouched("state errors")
        sur.bind_rows(12)
        valid("after the bindings were made again")
        # the frame binding's own column buffer is too narrow for the kind: refused
        sur.bind_frames(3, 3)
        sur.bind_rows(12)
        assert call(kind=1, cols_ptr=0) == ARG and call(kind=0, cols_ptr=0) == 0
        sur.synchronize()
    finally:
        sur.bind_frames(3, 8)
        sur.bind_rows(12)
        for a in (d_rows, d_cols, d_sc):
            a.free()


# ------------------------------------------------------------------------------------------------------- GPU, the evaluators
def equal(a, b):
    """Bit-level equality of what timeSteps returns and records: arrays by their bits, floats with NaN == NaN, containers deep."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    return type(a) is type(b) and a == b


def tap(sur, name, index, store):
    """Records element `index` of what sur.<name> returns (the raw sums; with the rows entries their relevant rows only)."""
    inner = getattr(sur, name)

    def wrapped(*a, **kw):
        out = inner(*a, **kw)
        raw = out if index is None else out[index]
        if name.endswith("_rows") or name.endswith("_rows_errors"):
            raw = raw[out[-1][:, 3] != 0]
        store.append(np.array(raw, copy=True))
        return out
    setattr(sur, name, wrapped)
    return lambda: delattr(sur, name)


LISTS = ("pred_minus_true", "pred_minus_true_squared", "pred_minus_true_block", "pred_minus_true_squared_block", "pred_minus_true_deltap_crude",
         "pred_minus_true_squared_deltap_crude", "pred_minus_true_p", "pred_minus_true_squared_p")
RAW_OF = {"deltas": (("deltas_frames", 2), ("deltas_rows", 2)), "gradp": (("gradp_frames", 3), ("gradp_rows", 3)),
          "poisson": (("poisson_frames_errors", None), ("poisson_rows_errors", 0))}


def run(kind, ev, times, fields, device_prep, **kw):
    """One timeSteps call -> everything it returns and records, copied."""
    sur = ev._sur
    raws = []
    undo = [tap(sur, name, index, raws) for name, index in RAW_OF[kind]]
    n0 = {name: len(getattr(ev, name, None) or []) for name in LISTS}
    try:
        out = ev.timeSteps(0, times, fields=fields, device_prep=device_prep, **kw)
    finally:
        for u in undo:
            u()
    lists = {name: list(getattr(ev, name))[n0[name]:] for name in LISTS if getattr(ev, name, None) is not None}
    keep = lambda v: np.array(v, copy=True) if isinstance(v, np.ndarray) else v
    return dict(out=[keep(o) for o in out], lists=lists, U=ev.U_max_norm, raw=np.concatenate(raws) if raws else None,
                last={k: dict(v) for k, v in ev.last_metrics.items()}, trips=sur.guard_trips,
                labels=[keep(p) for p in ev.label_planes] if getattr(ev, "label_planes", None) is not None else None)


def compare(a, b, label, frames=None):
    """device_prep on (b) against off (a): the returned frames (all, or `frames` of b against all of a), raw sums, U_max_norm, lists,
    last_metrics."""
    out_b = b["out"] if frames is None else [b["out"][i] for i in frames]
    same = dict(out=equal(a["out"], out_b), raw=equal(a["raw"], b["raw"]), U=equal(float(a["U"]), float(b["U"])), lists=equal(a["lists"], b["lists"]),
                last=equal(a["last"], b["last"]))
    print(f"{label}: bit for bit equal -> {same}; U_max_norm {a['U']!r} / {b['U']!r}; guard trips {b['trips']}")
    assert all(same.values()) and b["trips"] == 0, label


def squares_agree(path, n_frames, indice):
    """pow(U, 2.0) == U * U in float32 for the dataset frames a whole-step test sends (see the module docstring)."""
    for t in range(n_frames):
        d = formats.read_dataset(path, 0, t)[0][0, 0, :indice]
        U = np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2])))
        assert isinstance(U, np.float32) and pow(U, 2.0) == U * U and U ** 2 == U * U, (path, t, U)


def still_dataset(ds, name="still_rows.hdf5"):
    """The dataset with a middle frame whose velocity hardly changed (the variant of the evaluators' own tests)."""
    import h5write
    sim2 = ds["sim"].copy()
    sim2[0, 1, :ds["N"], 5:7] *= 1e-7
    p2 = os.path.join(ds["dir"], name)
    tb, ob = formats.read_dataset(ds["dataset_path"], 0, 0)[1:]
    h5write.write_h5(p2, {"sim_data": sim2, "top_bound": np.repeat(tb, 3, axis=1), "obst_bound": np.repeat(ob, 3, axis=1)})
    return p2


@pytest.fixture(scope="module")
def ds_deltas(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rows_deltas"))
    c = cases.build_dataset_case(d)
    c["dir"] = d
    return c


@pytest.fixture(scope="module")
def ds_poisson(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rows_poisson"))
    c = cases.build_dataset_case(d, poisson=True)
    c["dir"] = d
    return c


@pytest.fixture(scope="module")
def ds_gradp(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rows_gradp"))
    c = cases.build_gradp_dataset_case(d)
    c["dir"] = d
    return c


@pytest.mark.gpu
def test_gpu_deltas_time_steps_device_prep(ds_deltas):
    ds = ds_deltas
    ev = tdf.evaluator(ds, max_frames=3)
    assert ev.computeOnlyOnce(0) == 0
    squares_agree(ds["dataset_path"], 3, ev.indice)
    ref = {}
    for fields in (False, True):
        ref[fields] = run("deltas", ev, [0, 1, 2], fields, False)
        got = run("deltas", ev, [0, 1, 2], fields, True)
        assert len(got["out"]) == 3 and not any(isinstance(o, int) for o in got["out"])
        compare(ref[fields], got, f"deltas fields={fields}")
    # frame independence: frame 2 of the batch of three is frame 2 sent alone
    for fields in (False, True):
        alone = run("deltas", ev, [2], fields, True)
        print(f"deltas fields={fields}: frame 2 alone equals frame 2 of the batch: {equal(alone['out'][0], ref[fields]['out'][2])}")
        assert equal(alone["out"][0], ref[fields]["out"][2]) and alone["trips"] == 0
    # an irrelevant frame in the middle keeps its slot, returns 0 and changes no other frame's bits
    ev.dataset_path = still_dataset(ds)
    squares_agree(ev.dataset_path, 3, ev.indice)
    for fields in (False, True):
        off = run("deltas", ev, [0, 1, 2], fields, False)                      # the default mode sends frames 0 and 2 only
        on = run("deltas", ev, [0, 1, 2], fields, True)
        assert isinstance(on["out"][1], int) and on["out"][1] == 0 and isinstance(off["out"][1], int)
        compare(off, on, f"deltas fields={fields}, middle frame irrelevant")
        assert equal(on["out"][0], ref[fields]["out"][0]) and equal(on["out"][2], ref[fields]["out"][2]), "the frames beside the irrelevant one changed"
        assert len(on["lists"]["pred_minus_true"]) == 2 and len(on["lists"]["pred_minus_true_block"]) == 2
    assert ev.timeSteps(0, [1], fields=False, device_prep=True) == [0] and ev._sur.guard_trips == 0


@pytest.mark.gpu
def test_gpu_poisson_time_steps_device_prep(ds_poisson):
    ds = ds_poisson
    ev = tpf.evaluator(ds, max_frames=3)
    assert ev.computeOnlyOnce(0) == 0
    squares_agree(ds["dataset_path"], 3, ev.indice)
    ref = {}
    for fields in (False, True):
        ref[fields] = run("poisson", ev, [0, 1, 2], fields, False, phi=PHI)
        got = run("poisson", ev, [0, 1, 2], fields, True, phi=PHI)
        assert len(got["out"]) == 3 and not any(isinstance(o, int) for o in got["out"]) and ev._sur.geometry_bound
        compare(ref[fields], got, f"Poisson fields={fields}")
        assert equal(ref[fields]["labels"], got["labels"])
    # an irrelevant frame in the middle keeps its slot (the call still holds three frames: the bound route, as above), returns 0
    # and changes no other frame's bits
    good, ev.dataset_path = ev.dataset_path, still_dataset(ds)
    squares_agree(ev.dataset_path, 3, ev.indice)
    for fields in (False, True):
        on = run("poisson", ev, [0, 1, 2], fields, True, phi=PHI)
        assert isinstance(on["out"][1], int) and on["out"][1] == 0 and on["trips"] == 0
        same = [equal(on["out"][i], ref[fields]["out"][i]) for i in (0, 2)]
        print(f"Poisson fields={fields}, middle frame irrelevant: frames 0 and 2 equal the run without it: {same}; lists {len(on['lists']['pred_minus_true'])}")
        assert all(same) and len(on["lists"]["pred_minus_true"]) == 2 and len(on["lists"]["pred_minus_true_p"]) == 2
        assert equal(on["lists"]["pred_minus_true"], [ref[fields]["lists"]["pred_minus_true"][i] for i in (0, 2)])
        if fields:
            assert on["labels"][1] is None and equal(on["labels"][0], ref[True]["labels"][0]) and equal(on["labels"][2], ref[True]["labels"][2])
    assert ev.timeSteps(0, [1], False, PHI, device_prep=True) == [0] and ev._sur.guard_trips == 0
    # frame independence: frame 2 of a batch of three is frame 2 sent alone -- on the general route, which a call of any frame count
    # takes (the geometry is bound for exactly three)
    ev.dataset_path = good
    ev._sur.unbind_geometry()
    for fields in (False, True):
        batch = run("poisson", ev, [0, 1, 2], fields, True, phi=PHI)
        alone = run("poisson", ev, [2], fields, True, phi=PHI)
        print(f"Poisson fields={fields}: frame 2 alone equals frame 2 of the batch (general route): {equal(alone['out'][0], batch['out'][2])}")
        assert equal(alone["out"][0], batch["out"][2])


@pytest.mark.gpu
def test_gpu_gradp_time_steps_device_prep(ds_gradp):
    ds = ds_gradp
    ev = tgf.evaluator(ds, max_frames=3)
    assert ev.computeOnlyOnce(0) == 0
    assert isinstance(ev.max_x - ev.min_x, np.float32) and isinstance(ev.max_y - ev.min_y, np.float32)     # what the kernel's ex / ey reproduce
    squares_agree(ds["dataset_path"], 2, ev.indice)
    times = [0, 1, 1, 0, 1]                                       # calls of 3 and 2 frames
    ref = {}
    for fields in (False, True):
        ref[fields] = run("gradp", ev, times, fields, False)
        got = run("gradp", ev, times, fields, True)
        compare(ref[fields], got, f"gradP fields={fields}")
        assert equal(ev.frame_metrics, [ref[fields]["out"][i] for i in range(5)]) if not fields else len(ev.frame_metrics) == 5
    for fields in (False, True):
        alone = run("gradp", ev, [1], fields, True)
        print(f"gradP fields={fields}: frame 1 alone equals frame 1 of the batch: {equal(alone['out'][0], ref[fields]['out'][1])}")
        assert equal(alone["out"][0], ref[fields]["out"][1]) and alone["trips"] == 0
