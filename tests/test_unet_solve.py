"""The convolutional path at the solver boundary (psm_unet_mesh_*, psm_unet_solve*): K meshes, cells [sum n_i, 5] -> p [sum n_i]
through the U-Net, on the device.  The step is checked end by end on what it leaves behind (psm_unet_mesh_read): the HEAD against
the NumPy oracle's ``mesh_to_grid`` on the same tables, the NETWORK against ``psm_unet_forward`` on the read-back canvas (its own
accuracy is tests/test_unet.py's), the TAIL against the oracle's ``grid_to_mesh`` on the read-back field; then end to end against the
full NumPy composition, the delta step, the device entry, the errors and the Python mirrors.

Inputs: the four ``synthetic.channel_mesh`` cases of tests/test_mesh_cases.py (138 x 300 grid, about 16 k cells each, native
tables, two time steps) behind three small networks -- none of the grid's axes, one or both need padding:

  L = 4, widths (16, 16, 32, 32): canvas 144 x 304      L = 3, (16, 16, 32): canvas 140 x 300      L = 2, (16, 16): canvas 138 x 300

A (network, precision) pair is solved once per module (``runs``) and its read-backs are shared by the tests; the NumPy references
are computed once and never modified."""
import ctypes as C
import warnings

import numpy as np
import pytest

import hipmem
from oracle import psm_oracle as orc
from oracle import unet_oracle as uo
from psm_amd import UNetSolverEnsemble, UNetSolverModule, UNetSurrogate, _lib
from test_mesh_cases import CELLS, SHAPE, Ensemble, check_against_oracle, pack, split

pytestmark = pytest.mark.gpu

NETS = {4: (16, 16, 32, 32), 3: (16, 16, 32), 2: (16, 16)}
CANVAS = {4: (144, 304), 3: (140, 300), 2: (138, 300)}
DELTA_MAXS = (0.01, 0.01, 0.35, 0.5)     # tests/test_delta_step.py: the image channels of a velocity difference are O(1)
BOUND = 2e-4                              # of max|p_ref|: what tests/test_mesh_cases.py holds the PCA path's boundary to
_dp = C.POINTER(C.c_double)
_COLS = (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32), ("sdfunct", np.float64), ("vtx_g2m", np.int32), ("wts_g2m", np.float64))


def weights(L, c_in=3):
    return uo.he_weights(uo.unet_specs(c_in, NETS[L], 1), seed=40 + L)


class Binding:
    """A planned network and a mesh binding on it, through the C entries."""

    def __init__(self, L, precision="f32", max_cases=3, step="absolute", canvas=None):
        self.lib, self.L = _lib.load(), L
        self.ny_c, self.nx_c = canvas or CANVAS[L]
        self.net = UNetSurrogate(weights(L), self.ny_c, self.nx_c, widths=NETS[L], max_cases=max_cases, precision=precision)
        self.h = C.c_void_p()
        rc = self.lib.psm_unet_mesh_create(self.net.h, 0, self.ny_c, self.nx_c, max_cases, _lib.UNET_STEPS[step], C.byref(self.h))
        assert rc == 0, self.lib.psm_unet_mesh_last_error(None)
        self.K = 0

    def error(self):
        return (self.lib.psm_unet_mesh_last_error(self.h) or b"").decode()

    def set_geometry(self, ens, order, maxs=None, flags=0, expect=0):
        tabs = [ens.tabs[k] for k in order]
        cols = [[np.ascontiguousarray(getattr(g, f), dt) for g in tabs] for f, dt in _COLS]
        mx = np.asarray(maxs or ens.maxs, np.float64)
        rc = self.lib.psm_unet_mesh_set_geometry(self.h, len(order), (C.c_int64 * len(order))(*[CELLS[k] for k in order]), *SHAPE,
                                                 *[(C.c_void_p * len(order))(*[a.ctypes.data for a in c]) for c in cols], mx.ctypes.data_as(_dp),
                                                 flags, flags, 0.05)
        assert rc == expect, (rc, self.error())
        if rc == 0:
            self.K = len(order)
        return self

    def solve(self, cells):
        p = np.full(cells.shape[0], -7.0)
        rc = self.lib.psm_unet_solve(self.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp))
        assert rc == 0, self.error()
        return p

    def read(self, what):
        out = {"canvas": np.empty((self.K, self.ny_c, self.nx_c, 3), np.float32), "field": np.empty((self.K, self.ny_c, self.nx_c), np.float32),
               "umax": np.empty(self.K)}[what]
        rc = self.lib.psm_unet_mesh_read(self.h, _lib.UNET_READ[what], out.ctypes.data, out.nbytes)
        assert rc == 0, self.error()
        return out

    def state(self):
        primed, steps = C.c_int32(-1), C.c_int64(-1)
        assert self.lib.psm_unet_mesh_state(self.h, C.byref(primed), C.byref(steps)) == 0
        return bool(primed.value), steps.value

    def close(self):
        self.lib.psm_unet_mesh_destroy(self.h)
        self.net.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


ORDER = (0, 1, 2)


class Shared:
    """The ensemble, and per (L, precision) one run of two consecutive steps of cases (0, 1, 2) with everything read back."""

    def __init__(self):
        self.ens = Ensemble()
        self._runs, self._grids = {}, {}

    def grid(self, k, step):
        """The oracle's image and U_max of case k (float64, computed once)."""
        if (k, step) not in self._grids:
            e = self.ens
            self._grids[(k, step)] = orc.mesh_to_grid(e.array(k, step), e.geo[k], e.maxs[0], e.maxs[1])
        return self._grids[(k, step)]

    def run(self, L, precision="f32"):
        if (L, precision) not in self._runs:
            out = []
            with Binding(L, precision).set_geometry(self.ens, ORDER) as b:
                for step in (0, 1):
                    p = b.solve(pack(self.ens, ORDER, step))
                    r = dict(p=split(p, ORDER), canvas=b.read("canvas"), field=b.read("field"), umax=b.read("umax"))
                    r["forward"] = b.net.forward(r["canvas"])[..., 0]            # the same handle, the same n_cases
                    out.append(r)
            self._runs[(L, precision)] = out
        return self._runs[(L, precision)]


@pytest.fixture(scope="module")
def shared():
    return Shared()


# ---- head ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 3, 2])
def test_head_image_padding_and_umax_against_the_oracle(shared, L):
    """Image region: at most one float32 ulp of the oracle's value per element (both are float32 roundings of float64 values a few
    float64 ulps apart: fma contraction, a multiplication by 1 / max_abs_dist in the place of a division).  Padding: +0.0 bit for
    bit after two consecutive solves.  U_max: 1e-15 relative.
    Measured on an MI355X: 0 of 124 200 image elements differ from the oracle's float32 value, in every case, step and network."""
    ny, nx = SHAPE
    for step, r in enumerate(shared.run(L)):
        pad = np.ones(CANVAS[L], bool)
        pad[:ny, :nx] = False
        assert pad.sum() == CANVAS[L][0] * CANVAS[L][1] - ny * nx
        assert (r["canvas"].view(np.uint32)[:, pad] == 0).all()
        for i, k in enumerate(ORDER):
            grid, umax = shared.grid(k, step)
            want = grid.astype(np.float32)
            got = r["canvas"][i, :ny, :nx]
            differ = int((got != want).sum())
            worst = float((np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)).max())
            print(f"L={L} step {step} case {k}: {differ} of {want.size} image elements differ, worst {worst:.2f} ulp")
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()
            assert np.count_nonzero(got[..., :2]) > 0.5 * ny * nx
            assert abs(r["umax"][i] - umax) <= 1e-15 * umax


def test_a_case_does_not_care_about_its_slot_or_its_neighbours(shared):
    ens = shared.ens
    first = dict(zip(ORDER, shared.run(4)[0]["canvas"]))
    other = (2, 0, 1)
    with Binding(4).set_geometry(ens, other) as b:
        b.solve(pack(ens, other))
        for k, c in zip(other, b.read("canvas")):
            np.testing.assert_array_equal(c, first[k])
        b.set_geometry(ens, (1,))                            # K = 1 on the same binding
        p = b.solve(pack(ens, (1,)))
        np.testing.assert_array_equal(b.read("canvas")[0], first[1])
        assert b.read("umax")[0] == shared.run(4)[0]["umax"][1]
        assert np.isfinite(p).all()


def test_a_nan_velocity_stays_in_its_case(shared):
    """One NaN velocity in case 1: its U_max is NaN like np.max's, its image is zero but for the SDF; cases 0 and 2 are bit for bit
    what they were, canvas and p."""
    ens, clean = shared.ens, shared.run(4)[0]
    bad = pack(ens, ORDER).copy()
    bad[CELLS[0] + 1234, 0] = np.nan
    with Binding(4).set_geometry(ens, ORDER) as b:
        p = split(b.solve(bad), ORDER)
        canvas, umax = b.read("canvas"), b.read("umax")
    assert np.isnan(umax[1]) and np.isfinite(umax[[0, 2]]).all()
    assert not canvas[1, ..., :2].any()
    np.testing.assert_array_equal(canvas[1, ..., 2], clean["canvas"][1, ..., 2])
    for i in (0, 2):
        np.testing.assert_array_equal(canvas[i], clean["canvas"][i])
        np.testing.assert_array_equal(p[i], clean["p"][i])


# ---- network --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("L", [4, 3, 2])
def test_field_is_the_forward_pass_of_the_canvas(shared, L, precision):
    for r in shared.run(L, precision):
        assert np.isfinite(r["field"]).all() and r["field"].any()
        np.testing.assert_array_equal(r["field"], r["forward"])


# ---- tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 3, 2])
def test_tail_against_the_oracle_on_the_read_back_field(shared, L):
    """p against grid_to_mesh of the read-back field (cropped, as float64) with the read-back U_max: float64 over three terms and two
    scalings, 1e-12 of max|p|; the cells where the oracle keeps cells[:,4] bit for bit."""
    ens = shared.ens
    ny, nx = SHAPE
    for step, r in enumerate(shared.run(L)):
        for i, k in enumerate(ORDER):
            array = ens.array(k, step)
            ref = orc.grid_to_mesh(r["field"][i, :ny, :nx].astype(np.float64), array, ens.geo[k], ens.maxs[3], r["umax"][i])
            kept = ref == array[:, 4]
            assert 0 < kept.sum() < len(ref)
            np.testing.assert_array_equal(r["p"][i][kept], array[kept, 4])
            err, bound = np.abs(r["p"][i] - ref).max(), 1e-12 * np.abs(ref).max()
            print(f"L={L} step {step} case {k}: max|p - ref| = {err:.3e}, bound {bound:.3e}, kept {int(kept.sum())}")
            assert err <= bound


# ---- end to end -----------------------------------------------------------------------------------------------------------
def numpy_step(ens, k, step, L, grid, umax):
    """mesh -> grid (given), np.pad to the canvas, unet_forward, crop, grid -> mesh."""
    ny, nx = SHAPE
    canvas = np.pad(grid.astype(np.float32), ((0, CANVAS[L][0] - ny), (0, CANVAS[L][1] - nx), (0, 0)))
    field = uo.unet_forward(canvas, weights(L), NETS[L])[:ny, :nx, 0]
    return orc.grid_to_mesh(field.astype(np.float64), ens.array(k, step), ens.geo[k], ens.maxs[3], umax)


@pytest.mark.parametrize("L", [4, 3, 2])
def test_end_to_end_against_the_numpy_composition(shared, L):
    """float32, two time steps, cases 0 and 2 of the three solved: 2e-4 of max|p_ref| (the network's own bound is 1e-4 of max|field|).
    Measured on an MI355X, max|p - ref| / max|p_ref|: 1.6e-6 .. 2.0e-6 (L = 4), 0.8e-6 .. 1.1e-6 (L = 3), 0.8e-6 .. 1.0e-6 (L = 2)."""
    ens = shared.ens
    for step, r in enumerate(shared.run(L)):
        for i, k in ((0, 0), (2, 2)):
            ref = numpy_step(ens, k, step, L, *shared.grid(k, step))
            check_against_oracle(r["p"][i], ens.array(k, step), ref)


def delta_reference(ens, k, L):
    """dp_ref of the step from time step 0 to time step 1 (NaN on the oracle's fallback cells), formed the way
    tests/test_delta_step.py forms its own, the network in the place of solve_grid."""
    prev, array, geo = ens.array(k, 0), ens.array(k, 1), ens.geo[k]
    ny, nx = SHAPE
    U_max = np.max(np.sqrt(np.square(array[:, 0]) + np.square(array[:, 1])))
    grid = np.zeros((ny, nx, 3))
    idx = tuple(geo.indices.T)
    for c in (0, 1):
        grid[:, :, c][idx] = orc.interpolate_fill((array[:, c] - prev[:, c]) / U_max, geo.vert_m2g, geo.wts_m2g) / DELTA_MAXS[c]
    grid[:, :, 2] = geo.sdfunct / DELTA_MAXS[2]
    grid[np.isnan(grid)] = 0
    canvas = np.pad(grid.astype(np.float32), ((0, CANVAS[L][0] - ny), (0, CANVAS[L][1] - nx), (0, 0)))
    field = uo.unet_forward(canvas, weights(L), NETS[L])[:ny, :nx, 0]
    marked = array.copy()
    marked[:, 4] = np.nan                                   # grid_to_mesh puts the previous p on its fallback cells: NaN marks them
    return orc.grid_to_mesh(field.astype(np.float64), marked, geo, DELTA_MAXS[3], U_max)


def test_delta_step_priming_reference_and_reset(shared):
    """The priming step, one real step against the composed reference (2e-4 of max|dp_ref|, the bound of tests/test_delta_step.py;
    measured on an MI355X: 1.4e-6 for both cases), the explicit prime, and reset."""
    ens, order = shared.ens, (0, 1)
    c0, c1 = pack(ens, order, 0), pack(ens, order, 1)
    with Binding(4, max_cases=2, step="delta").set_geometry(ens, order, DELTA_MAXS, flags=1) as b:
        assert b.state() == (False, 0)
        np.testing.assert_array_equal(b.solve(c0), c0[:, 4])            # the priming step
        assert b.state() == (True, 0)
        p = split(b.solve(c1), order)
        assert b.state() == (True, 1)
        for i, k in enumerate(order):
            array, dp_ref = ens.array(k, 1), delta_reference(ens, k, 4)
            fb = np.isnan(dp_ref)
            assert 0.0 < fb.mean() < 0.5, fb.mean()
            np.testing.assert_array_equal(p[i][fb], array[fb, 4])
            dp = p[i][~fb] - array[~fb, 4]
            scale = np.abs(dp_ref[~fb]).max()
            err = np.abs(dp - dp_ref[~fb]).max() / scale
            print(f"case {k}: max|dp - dp_ref| / max|dp_ref| = {err:.3e} (max|dp_ref| = {scale:.3e}, fallback share {fb.mean():.3f})")
            assert err <= BOUND
        # the image holds the difference: the explicit prime with time step 0 gives the same step again, bit for bit
        assert b.lib.psm_unet_mesh_prime(b.h, c0.ctypes.data_as(_dp)) == 0, b.error()
        assert b.state() == (True, 1)
        again = b.solve(c1)
        np.testing.assert_array_equal(again, np.concatenate(p))
        assert b.state() == (True, 2)
        assert b.lib.psm_unet_mesh_reset(b.h) == 0
        assert b.state() == (False, 0)
        np.testing.assert_array_equal(b.solve(c1), c1[:, 4])            # a priming step again
        assert b.state() == (True, 0)


def test_device_entry_equals_the_host_entry(shared):
    ens = shared.ens
    cells = pack(ens, ORDER)
    with Binding(4).set_geometry(ens, ORDER) as b:
        d_cells, d_p = hipmem.DeviceArray(cells), hipmem.DeviceArray(shape=(len(cells),), dtype=np.float64)
        assert b.lib.psm_unet_solve_device(b.h, d_cells.ptr, d_p.ptr, None) == 0, b.error()
        got = d_p.numpy()
        d_cells.free(); d_p.free()
    np.testing.assert_array_equal(got, np.concatenate(shared.run(4)[0]["p"]))


def test_errors_are_reported_and_leave_the_handles_usable(shared):
    ens, lib = shared.ens, _lib.load()
    out = C.c_void_p()
    cells = pack(ens, (0, 1))
    with Binding(4, max_cases=2).set_geometry(ens, (0, 1)) as b:
        ref = b.solve(cells)
        # K > max_cases, and a null table: refused before the binding is touched
        b.set_geometry(ens, (0, 1, 2), expect=-1)
        assert "max_cases" in b.error()
        assert lib.psm_unet_mesh_set_geometry(b.h, 1, (C.c_int64 * 1)(CELLS[0]), *SHAPE, *[None] * 6, None, 0, 0, 0.05) == -1
        np.testing.assert_array_equal(b.solve(cells), ref)
        # the network is planned for 144 x 304: a binding for another canvas, or for a shape that is no canvas, is refused
        assert lib.psm_unet_mesh_create(b.net.h, 0, 160, 304, 2, 0, C.byref(out)) == -1 and not out.value
        assert "another image size" in lib.psm_unet_mesh_last_error(None).decode()
        assert lib.psm_unet_mesh_create(b.net.h, 0, 138, 300, 2, 0, C.byref(out)) == -1 and not out.value
        assert lib.psm_unet_mesh_create(b.net.h, 0, 144, 304, 2, 7, C.byref(out)) == -1 and not out.value
        # the state entries of an absolute binding
        assert lib.psm_unet_mesh_prime(b.h, cells.ctypes.data_as(_dp)) == -2 and lib.psm_unet_mesh_reset(b.h) == -2
        assert b.state() == (False, 0)
        assert lib.psm_unet_mesh_read(b.h, 9, cells.ctypes.data, cells.nbytes) == -1
        assert lib.psm_unet_mesh_read(b.h, 0, cells.ctypes.data, 16) == -1 and "too small" in b.error()
        np.testing.assert_array_equal(b.solve(cells), ref)
    # a geometry whose canvas is not the binding's: 138 x 300 under four levels is 144 x 304, the binding holds 160 x 304
    with Binding(4, max_cases=1, canvas=(160, 304)) as b:
        assert lib.psm_unet_solve(b.h, cells.ctypes.data_as(_dp), cells.ctypes.data_as(_dp)) == -2       # no geometry yet
        assert lib.psm_unet_mesh_read(b.h, 0, cells.ctypes.data, cells.nbytes) == -2
        b.set_geometry(ens, (0,), expect=-1)
        assert "144 x 304" in b.error() and "160 x 304" in b.error()
    # an unplanned network; a four-channel stem
    w = np.asarray(NETS[2], np.int32)
    u = C.c_void_p()
    assert lib.psm_unet_create(3, 1, 2, w.ctypes.data_as(C.POINTER(C.c_int32)), 0, C.byref(u)) == 0
    assert lib.psm_unet_mesh_create(u, 0, 138, 300, 1, 0, C.byref(out)) == -2 and not out.value
    assert "not planned" in lib.psm_unet_mesh_last_error(None).decode()
    lib.psm_unet_destroy(u)
    with UNetSurrogate(weights(2, c_in=4), 138, 300, c_in=4, widths=NETS[2]) as net:
        assert lib.psm_unet_mesh_create(net.h, 0, 138, 300, 1, 0, C.byref(out)) == -5 and not out.value
        assert "c_in == 3" in lib.psm_unet_mesh_last_error(None).decode()
        g = np.zeros((138, 300, 4), np.float32)
        assert np.isfinite(net.forward(g)).all()            # the network is as usable as before


# ---- the Python mirrors -------------------------------------------------------------------------------------------------
def test_solver_module_and_ensemble_return_what_the_c_entries_return(shared):
    ens = shared.ens
    run = shared.run(4)
    with UNetSolverEnsemble(weights(4), ens.maxs, NETS[4], geometry="native", max_cases=3) as se:
        assert se.init_func(*zip(*[ens.mesh[k] for k in ORDER])) == 0
        assert se.cell_off == [0, 16021, 32186, 48024] and (se.ny_c, se.nx_c) == CANVAS[4]
        for step in (0, 1):
            for a, b in zip(se.py_func([ens.array(k, step) for k in ORDER]), run[step]["p"]):
                np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(se.read("canvas"), run[1]["canvas"])
        np.testing.assert_array_equal(se.read("umax"), run[1]["umax"])
    with UNetSolverModule(weights(2), ens.maxs, NETS[2], geometry="native") as sm:
        assert sm.init_func(*ens.mesh[0]) == 0
        out = np.empty(CELLS[0])
        assert sm.py_func(ens.array(0), out=out) is out
        np.testing.assert_array_equal(out, shared.run(2)[0]["p"][0])
        with pytest.raises(ValueError):
            sm.py_func(ens.array(1))                        # the cell count of init_func
    # step='delta': init_func primes with its own array; the first py_func is a real step
    with Binding(4, max_cases=1, step="delta").set_geometry(ens, (0,), DELTA_MAXS, flags=1) as b:
        assert b.lib.psm_unet_mesh_prime(b.h, pack(ens, (0,)).ctypes.data_as(_dp)) == 0
        want = b.solve(pack(ens, (0,), 1))
    with UNetSolverModule(weights(4), DELTA_MAXS, NETS[4], step="delta", geometry="native") as sm:
        sm.init_func(*ens.mesh[0])
        assert sm.state == (True, 0)
        np.testing.assert_array_equal(sm.py_func(ens.array(0, 1)), want)
        assert sm.state == (True, 1)
        sm.reset_state()
        assert sm.state == (False, 0)
        np.testing.assert_array_equal(sm.py_func(ens.array(0, 1)), ens.array(0, 1)[:, 4])


def test_scipy_tables_serve_the_same_entries(shared):
    """geometry='scipy' (geometry.build_geometry): the step on qhull's tables against the NumPy composition on the same tables."""
    ens = shared.ens
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with UNetSolverModule(weights(2), ens.maxs, NETS[2], geometry="scipy") as sm:
            sm.init_func(*ens.mesh[3])
            g = sm.tables
            assert (g.ny, g.nx) == SHAPE
            p = sm.py_func(ens.array(3))
    geo = orc.Geometry(g.ny, g.nx, g.vtx_m2g, g.wts_m2g, g.vtx_g2m, g.wts_g2m, g.indices, g.sdfunct)
    grid, umax = orc.mesh_to_grid(ens.array(3), geo, ens.maxs[0], ens.maxs[1])
    field = uo.unet_forward(grid.astype(np.float32), weights(2), NETS[2])[..., 0]
    check_against_oracle(p, ens.array(3), orc.grid_to_mesh(field.astype(np.float64), ens.array(3), geo, ens.maxs[3], umax))
