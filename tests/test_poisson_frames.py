"""Frames of cell columns on the device (psm_bind_frames, psm_frames_to_grid_device, psm_poisson_frames_device / psm_poisson_frames)
and the evaluator on top of them (EvaluationPoisson.timeSteps, call_SM_main_Poisson(frames_per_call=...)): the mesh -> grid step of
pressureSM_Poisson/SM_call.py:577-600 for K frames in one launch, every column into a plane of its own, and behind it the Poisson
time step of test_poisson_step_device.py as one graph replay.

Table sets of the kernel tests: (a) the evaluator's tables of cases.build_dataset_case(poisson=True) -- 138 x 300 = 161 full
workgroups + 184 cells, IDW fallback, out-of-domain points colliding in cell (0, 0); (b) a hand-made set on 130 x 131 (66 workgroups
+ 134 cells, 200 mesh cells, random simplices) with negative weights, cells written by several grid points and cells written by
none -- (a) can hold no negative weight.

References: psm_mesh_to_grid on the same frame (bit for bit: same statements, same order), the oracle's interpolate_fill + NumPy
scatter in float64 (1e-12 * max|plane|, the bound of test_dataset_evaluator.py for this step), psm_poisson_step_device fed with the
planes of psm_mesh_to_grid (bit for bit: same kernels, inputs and route) and the float64 chain of
test_poisson_evaluation_from_files_end_to_end (NaN pattern equal, 2e-4 * max(|want|, |field|): the project's SOLVE_TOL).
Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import cases
from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import EvaluationPoisson, GridSurrogate, _lib, call_SM_main_Poisson, error_metrics, formats, geometry, surrogate, synthetic
from test_oracle_golden import oracle_model
from test_poisson_step_device import MAX_ABS, P_SCALE, S_FIELD, S_WEIGHT, SOLVE_TOL, error, free, model4
from test_poisson_step_device import K as K_ARCSINH

NEW_ENTRIES = ("psm_bind_frames", "psm_unbind_frames", "psm_frames_to_grid_device", "psm_poisson_frames_device", "psm_poisson_frames")
NEW_METHODS = ("bind_frames", "unbind_frames", "frames_to_grid_device", "poisson_frames_device", "poisson_frames")
GRID_TOL = 1e-12
NF = 3                                   # frames per batch
PAD, CANARY = 37, -7.5                   # canary elements on either side of every plane
PHI = 0.16
_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------------------------- tables, computed once
@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("poisson_frames"))
    c = cases.build_dataset_case(d, poisson=True)
    cells = np.asarray(c["sim"][0, 0, :c["N"]], np.float64)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    c["dir"] = d
    c["tables"] = geometry.build_geometry_evaluator(cells[:, 3:5], cells[:, 2], f32(c["top"]), f32(c["obst"]), 5e-3, idw_fallback=True)
    return c


class Tables:
    def __init__(self, ny, nx, n_cells, vtx, wts, indices, sdfunct):
        self.ny, self.nx, self.n_cells = ny, nx, n_cells
        self.vtx, self.wts, self.indices, self.sdfunct = vtx, wts, indices, sdfunct


def eval_tables(c):
    t = c["tables"]
    return Tables(t.ny, t.nx, c["N"], np.ascontiguousarray(t.vtx_m2g, np.int32), np.ascontiguousarray(t.wts_m2g, np.float64),
                  np.ascontiguousarray(t.indices, np.int32), np.ascontiguousarray(t.sdfunct, np.float64))


@functools.lru_cache(maxsize=None)
def hand_tables():
    """130 x 131, 200 mesh cells: random simplices, a quarter of the grid points with one negative weight, 15 % of the points
    redirected to another cell (that cell gets several writers, the point's own cell possibly none)."""
    ny, nx, n_cells = 130, 131, 200
    ng = ny * nx
    rng = np.random.default_rng(1301)
    vtx = rng.integers(0, n_cells, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    wts = np.c_[w, 1.0 - w.sum(axis=1)]
    neg = rng.random(ng) < 0.25
    wts[neg, 0] = -wts[neg, 0]
    wts[neg, 2] = 1.0 - wts[neg, 0] - wts[neg, 1]
    cell = np.arange(ng)
    moved = rng.random(ng) < 0.15
    cell[moved] = rng.integers(0, ng, int(moved.sum()))
    indices = np.c_[cell // nx, cell % nx].astype(np.int32)
    return Tables(ny, nx, n_cells, vtx, np.ascontiguousarray(wts), indices, np.ones((ny, nx)))


def cell_kinds(t):
    """(cells nobody writes, cells several points write, cells whose last writer has a negative weight), from the tables."""
    ng = t.ny * t.nx
    flat = t.indices[:, 0].astype(np.int64) * t.nx + t.indices[:, 1]
    writers = np.bincount(flat, minlength=ng)
    last = np.full(ng, -1)
    last[flat] = np.arange(ng)                                   # NumPy fancy assignment: the last writer stays
    neg = (t.wts < 0).any(axis=1)
    return int((writers == 0).sum()), int((writers > 1).sum()), int(neg[last[last >= 0]].sum())


def frame_columns(t, k, seed):
    """[NF][n_cells][k] float64, other values per frame; NaNs in (up to) two columns of the last frame."""
    rng = np.random.default_rng(seed)
    cols = rng.standard_normal((NF, t.n_cells, k)) * (1.0 + np.arange(NF))[:, None, None]
    cols[NF - 1, 3 % t.n_cells, 0] = np.nan
    cols[NF - 1, t.n_cells // 2, k - 1] = np.nan
    return np.ascontiguousarray(cols)


def surrogate_on(t, max_cases=NF):
    sur = GridSurrogate(model4(), t.ny, t.nx, max_cases=max_cases)
    sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
    return sur


def mesh_to_grid(sur, values, fill):
    """psm_mesh_to_grid of one frame [n_cells][k] -> planes [k][Ny][Nx] float64."""
    v = np.ascontiguousarray(values, np.float64)
    out = np.empty((sur.ny, sur.nx, v.shape[1]), np.float64)
    sur._chk(sur.lib.psm_mesh_to_grid(sur.h, v.ctypes.data_as(_dp), v.shape[0], v.shape[1], int(fill), out.ctypes.data_as(_dp)))
    return np.ascontiguousarray(np.moveaxis(out, 2, 0))


def oracle_plane(t, col):
    g = np.zeros((t.ny, t.nx))
    g[tuple(t.indices.T)] = orc.interpolate_fill(np.asarray(col, np.float64).reshape(-1), t.vtx, t.wts)
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# plan A / plan B of the destinations: between them every column is stored as float64 and as float32 once, and left out once
KINDS = (("f64", "f32", None), ("f32", None, "f64"))


def launch(sur, d_cols_ptr, n_frames, k, plan, fill):
    """One psm_frames_to_grid_device: all float64 columns share one array [n][k][PAD + npix + PAD], all float32 columns
    another; column c uses plane slot c of its array.  -> (float64 array, float32 array) as NumPy, canaries included."""
    npix = sur.ny * sur.nx
    plane = npix + 2 * PAD + 1                                   # odd plane pitch: a float32 plane starts 4-, not 8-byte aligned
    d64 = DeviceArray(np.full((n_frames, k, plane), CANARY, np.float64))
    d32 = DeviceArray(np.full((n_frames, k, plane), CANARY, np.float32))
    outs = []
    for c in range(k):
        kind = KINDS[plan][c % 3]
        if kind is None:
            outs.append((0, 0, 0))
        else:
            d, size = (d64, 8) if kind == "f64" else (d32, 4)
            outs.append((d.ptr + (c * plane + PAD) * size, k * plane, kind == "f32"))
    sur.frames_to_grid_device(d_cols_ptr, n_frames, k, outs, fill=fill)
    sur.synchronize()
    got = d64.numpy(), d32.numpy()
    free(d64, d32)
    return got


def check_launch(sur, got, want, k, plan, label):
    """got of launch(); want [n][k][npix] float64 from psm_mesh_to_grid.  -> planes compared."""
    npix = sur.ny * sur.nx
    n = want.shape[0]
    stats = dict(f64=0, f32=0, null=0)
    for c in range(k):
        kind = KINDS[plan][c % 3]
        for arr, name in ((got[0], "f64"), (got[1], "f32")):
            slot = arr[:, c]
            if kind == name:
                body = np.ascontiguousarray(slot[:, PAD:PAD + npix])
                ref = want[:, c] if name == "f64" else want[:, c].astype(np.float32)
                assert same_bits(body, np.ascontiguousarray(ref)), f"{label}: column {c} as {name} differs from psm_mesh_to_grid"
                assert (slot[:, :PAD] == CANARY).all() and (slot[:, PAD + npix:] == CANARY).all(), f"{label}: canary of column {c} ({name})"
                stats[name] += n
            else:
                assert (slot == CANARY).all(), f"{label}: column {c} wrote into a plane that is not its own ({name})"
        stats["null"] += n if kind is None else 0
    return stats


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_entries_are_declared_bound_and_exported():
    """Every new name is in psm.h, in _lib.SIGNATURES and exported by the built library; the mirrors exist."""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(psm_[a-z_0-9]+)\s*\(", txt))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "psm_frame_col" in txt and C.sizeof(_lib.psm_frame_col) == 24
    for name in NEW_METHODS:
        assert callable(getattr(GridSurrogate, name, None)), name
    assert callable(getattr(EvaluationPoisson, "timeSteps", None))


def test_python_argument_checks_come_before_any_library_call():
    """poisson_frames / poisson_frames_device / frames_to_grid_device / timeSteps refuse bad shapes on a surrogate whose library
    and handle do not exist: any call into the library would raise AttributeError instead."""
    sur = GridSurrogate.__new__(GridSurrogate)
    sur.lib = sur.h = None
    sur.ny, sur.nx, sur.model, sur.mesh_cells = 6, 7, model4(), 11
    ok = np.zeros((2, 11, 8))
    lu = [[0.2, 1.0], [0.2, 1.1]]
    with pytest.raises(ValueError, match="at least the 4 columns"):
        sur.poisson_frames(ok[..., :3], lu, weighting=False)
    with pytest.raises(ValueError, match="at least 6 columns"):
        sur.poisson_frames(ok[..., :5], lu)
    with pytest.raises(ValueError, match="at most 16"):
        sur.poisson_frames(np.zeros((2, 11, 17)), lu)
    with pytest.raises(ValueError, match=r"\[n,n_cells,k\]"):
        sur.poisson_frames(np.zeros((2, 3, 11, 8)), lu)
    with pytest.raises(ValueError, match="11 cells"):
        sur.poisson_frames(np.zeros((2, 12, 8)), lu)
    with pytest.raises(ValueError, match="LU"):
        sur.poisson_frames(ok, lu[:1])
    with pytest.raises(ValueError, match="out_scale"):
        sur.poisson_frames(ok, lu, out_scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="at least 6 columns"):
        sur.poisson_frames_device(4096, 2, 5, lu, 4096)
    with pytest.raises(ValueError, match="LU"):
        sur.poisson_frames_device(4096, 2, 8, lu[:1], 4096)
    with pytest.raises(ValueError, match="one .* per column"):
        sur.frames_to_grid_device(4096, 2, 3, [(4096, 42, 0)])
    sur.mesh_cells = None
    with pytest.raises(RuntimeError, match="no mesh"):
        sur.poisson_frames(ok, lu)
    sur.h = None                                                   # nothing for __del__ to destroy
    make = lambda **kw: EvaluationPoisson(5e-3, 128, 32, 0.95, 0.95, "no.hdf5", "no.h5", 128, "std", 0.5, None, model=model4(), **kw)
    with pytest.raises(ValueError, match="max_frames"):
        make(max_frames=0)
    ev = make(max_frames=3)
    assert ev.max_frames == 3 and make().max_frames == 1
    with pytest.raises(RuntimeError, match="computeOnlyOnce"):
        ev.timeSteps(0, [0, 1])


def test_the_hand_made_tables_hold_what_they_were_made_for(ds):
    """Set (b): at least 100 cells nobody writes, 100 that several points write and 100 whose last writer has a negative weight;
    both sets end in a partly idle workgroup; set (a) has no negative weight and its out-of-domain points collide in cell (0, 0)."""
    b, a = hand_tables(), eval_tables(ds)
    none_b, many_b, neg_b = cell_kinds(b)
    none_a, many_a, neg_a = cell_kinds(a)
    print(f"set (b): {none_b} unwritten, {many_b} written by several points, {neg_b} ending on a negative weight; "
          f"set (a): {none_a} / {many_a} / {neg_a}")
    assert min(none_b, many_b, neg_b) >= 100
    assert neg_a == 0 and many_a >= 1 and ((a.indices == 0).all(axis=1)).sum() > 1
    assert (b.ny * b.nx, a.ny * a.nx) == (66 * 256 + 134, 161 * 256 + 184)


# ------------------------------------------------------------------------------------------------------- GPU, the kernel alone
@pytest.mark.gpu
@pytest.mark.parametrize("which,k", [("eval", 1), ("eval", 8), ("hand", 1), ("hand", 8), ("hand", 16)])
def test_gpu_frames_to_grid_is_psm_mesh_to_grid_per_column(ds, which, k):
    """Three frames in one launch, fill 0 and 1, two destination plans: every float64 plane is psm_mesh_to_grid's column bit for
    bit (NaN pattern included), every float32 plane its np.float32, frame i of the batch is frame i sent alone, canaries and the
    planes of NULL columns stay untouched; with fill, every plane is within 1e-12 * max of the oracle."""
    t = eval_tables(ds) if which == "eval" else hand_tables()
    cols = frame_columns(t, k, seed=100 + k)
    npix = t.ny * t.nx
    with surrogate_on(t) as sur:
        sur.bind_frames(NF, k)
        d_cols = DeviceArray(cols)
        frame_bytes = t.n_cells * k * 8
        total = dict(f64=0, f32=0, null=0)
        for fill in (0, 1):
            want = np.stack([mesh_to_grid(sur, cols[i], fill).reshape(k, npix) for i in range(NF)])
            for plan in (0, 1):
                label = f"{which} k={k} fill={fill} plan {'AB'[plan]}"
                got = launch(sur, d_cols.ptr, NF, k, plan, fill)
                st = check_launch(sur, got, want, k, plan, label)
                alone = 0
                for i in range(NF):
                    one = launch(sur, d_cols.ptr + i * frame_bytes, 1, k, plan, fill)
                    assert same_bits(one[0][0], got[0][i]) and same_bits(one[1][0], got[1][i]), f"{label}: frame {i} alone differs from the batch"
                    alone += 1
                for key in total:
                    total[key] += st[key]
                print(f"{label}: {st['f64']} float64 and {st['f32']} float32 planes identical to psm_mesh_to_grid, {st['null']} NULL planes and "
                      f"all canaries untouched, {alone} frames identical when sent alone")
            if fill:
                worst, nan_cells = 0.0, 0
                for i in range(NF):
                    for c in range(k):
                        ref, g = oracle_plane(t, cols[i, :, c]).reshape(-1), want[i, c]
                        assert np.array_equal(np.isnan(ref), np.isnan(g)), f"{which} k={k}: NaN pattern of frame {i} column {c}"
                        ok = ~np.isnan(ref)
                        nan_cells += int((~ok).sum())
                        worst = max(worst, float(np.abs(g[ok] - ref[ok]).max() / np.abs(ref[ok]).max()))
                print(f"{which} k={k}: against interpolate_fill + scatter {worst:.2e} (bound {GRID_TOL}), {nan_cells} NaN cells in all planes")
                assert worst <= GRID_TOL and (which == "eval" or nan_cells >= 100)
        assert total["f64"] > 0 and total["f32"] > 0 and (k == 1 or total["null"] > 0)
        free(d_cols)


# ------------------------------------------------------------------------------------------------------- GPU, the whole step
def dataset_columns(c, t, scale=1.0):
    """The evaluator's eight columns of frame t (as timeSteps builds them) and U_max_norm."""
    d = c["sim"][0, t, :c["N"]] * np.float32(scale)
    dU, dUp = d[:, 5:7], d[:, 8:10]
    changed = np.abs(dU - dUp).sum(axis=-1)
    changed = changed / changed.max()
    U = float(np.max(np.sqrt(np.square(d[:, 0:1]) + np.square(d[:, 1:2]))))
    cols = np.concatenate([d[:, 0:2], dU, d[:, 7:8], d[:, 2:3], changed[:, None], d[:, 10:11]], axis=1).astype(np.float64)
    return cols, U


def oracle_frame(t, cols, U, phi, model, max_abs4, p_scale):
    """Float64 chain of test_poisson_evaluation_from_files_end_to_end on one frame's columns -> (field_deltap, assembled field)."""
    g = [oracle_plane(t, cols[:, q]) for q in (0, 1, 2, 3, 6, 7)]
    grid, _ = orc.poisson_features(g[0], g[1], g[2], g[3], t.sdfunct, phi, U, K_ARCSINH, max_abs4)
    om = oracle_model(model)
    om.out_scale = p_scale * U ** 2
    field = orc.solve_grid(grid, om).fields[..., 0]
    prev, w = g[5], ndi.gaussian_filter(g[4], sigma=S_WEIGHT, order=0)
    return prev + ndi.gaussian_filter((field - prev) * w, sigma=S_FIELD, order=0), field


def check_against_chain(got, want, field, label):
    ok = ~np.isnan(want)
    same_nan = np.array_equal(np.isnan(got), ~ok)
    err = float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), np.abs(field).max()))
    print(f"{label}: NaN pattern equal {same_nan} ({ok.mean():.2f} of the cells finite), chain {err:.2e} (bound {SOLVE_TOL})")
    assert ok.mean() > 0.1 and same_nan and err <= SOLVE_TOL


def by_hand(sur, planes, lu, sc, af):
    """psm_poisson_step_device fed with planes [n][8][Ny][Nx] of psm_mesh_to_grid -> (result, change, next)."""
    n = planes.shape[0]
    d_vel = DeviceArray(np.ascontiguousarray(planes[:, 0:4]))
    d_u, d_p = (DeviceArray(np.ascontiguousarray(planes[:, q], np.float32)) for q in (6, 7))
    outs = [DeviceArray(shape=(n, sur.ny, sur.nx)) for _ in range(3)]
    sur.poisson_step_device(d_vel.ptr, n, lu, outs[0].ptr, af, d_u.ptr, d_p.ptr, outs[1].ptr, outs[2].ptr, out_scale=sc)
    sur.synchronize()
    got = tuple(o.numpy() for o in outs)
    free(d_vel, d_u, d_p, *outs)
    return got


def frames_device(sur, d_cols, n, k, lu, sc, af, d_extra=None):
    outs = [DeviceArray(shape=(n, sur.ny, sur.nx)) for _ in range(3)]
    sur.poisson_frames_device(d_cols.ptr, n, k, lu, outs[0].ptr, af, True, d_extra.ptr if d_extra else 0, outs[1].ptr, outs[2].ptr, out_scale=sc)
    sur.synchronize()
    got = tuple(o.numpy() for o in outs)
    free(*outs)
    return got


def bind_step(sur, t, n=NF, k=8):
    sur.bind_features(np.repeat(t.sdfunct[None], n, axis=0), K_ARCSINH, MAX_ABS)
    sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_frames(n, k)


@pytest.mark.gpu
def test_gpu_poisson_frames_is_the_step_fed_by_psm_mesh_to_grid(ds):
    """Three dataset frames as one psm_poisson_frames_device: result / change / next and the extra planes are those of
    psm_poisson_step_device on planes psm_mesh_to_grid made, bit for bit, on the general and on the bound route; a second replay
    with other columns in the same buffer and other (L, U) sees them; the host entry gives the device entry's bits; every frame
    is within 2e-4 of the float64 chain."""
    t = eval_tables(ds)
    frames = [dataset_columns(ds, i) for i in range(NF)]
    cols = np.stack([f[0] for f in frames])
    lu = np.array([[PHI, f[1]] for f in frames])
    sc = [P_SCALE * f[1] ** 2 for f in frames]
    cols2 = np.stack([dataset_columns(ds, i, scale=1.0 + 0.25 * (i + 1))[0] for i in (2, 0, 1)])
    lu2 = lu[[2, 0, 1]] * np.array([1.3, 1.0 + 0.25])
    with surrogate_on(t) as sur:
        bind_step(sur, t)
        d_cols, d_extra = DeviceArray(cols), DeviceArray(np.full((NF, 2, t.ny, t.nx), CANARY, np.float64))
        planes = np.stack([mesh_to_grid(sur, cols[i], 1) for i in range(NF)])
        for route in ("general", "bound"):
            if route == "bound":
                g = np.zeros((NF, t.ny, t.nx, 4), np.float32)
                g[..., 3] = (t.sdfunct / MAX_ABS[3]).astype(np.float32)[None]
                assert sur.bind_geometry(g) and sur.geometry_bound
            for af in (False, True):
                want = by_hand(sur, planes, lu, sc, af)
                got = frames_device(sur, d_cols, NF, 8, lu, sc, af, d_extra)
                same = [same_bits(a, b) for a, b in zip(got, want)]
                extra_same = same_bits(d_extra.numpy(), np.ascontiguousarray(planes[:, 4:6]))
                print(f"frames step {route} apply_filter={af}: identical to mesh_to_grid -> poisson_step_device {same}, extra planes identical {extra_same}, "
                      f"{int(np.isnan(got[2]).sum())} NaN cells in next")
                assert all(same) and extra_same
        assert sur.guard_trips == 0 and sur.geometry_bound
        first = frames_device(sur, d_cols, NF, 8, lu, sc, False, d_extra)
        # the same buffers, other columns and scalars: the second call has the first one's graph key
        assert sur.lib.psm_debug_copy_to_device(d_cols.ptr, cols2.ctypes.data, cols2.nbytes) == 0
        planes2 = np.stack([mesh_to_grid(sur, cols2[i], 1) for i in range(NF)])
        sc2 = [1.7 * s for s in sc]
        got2, want2 = frames_device(sur, d_cols, NF, 8, lu2, sc2, False, d_extra), by_hand(sur, planes2, lu2, sc2, False)
        same2 = [same_bits(a, b) for a, b in zip(got2, want2)]
        ok = ~np.isnan(first[0]) & ~np.isnan(got2[0])
        moved = float(np.abs(got2[0][ok] - first[0][ok]).max())
        print(f"second replay with other columns and (L, U): identical to the composition by hand {same2}, result moved by {moved:.3e}")
        assert all(same2) and moved > 0 and same_bits(d_extra.numpy(), np.ascontiguousarray(planes2[:, 4:6]))
        # host entry
        for af in (False, True):
            dev = frames_device(sur, d_cols, NF, 8, lu2, sc2, af, d_extra)
            res, chg, nxt, extra = sur.poisson_frames(cols2, lu2, out_scale=sc2, apply_filter=af)
            same = [same_bits(res[..., 0], dev[0]), same_bits(chg, dev[1]), same_bits(nxt, dev[2]), same_bits(extra, np.ascontiguousarray(planes2[:, 4:6]))]
            print(f"host entry apply_filter={af}: result / change / next identical to the device entry, extra to psm_mesh_to_grid {same}")
            assert all(same)
        res, chg, nxt, extra = sur.poisson_frames(cols[:2, :, :4], lu[:2], out_scale=sc[:2], weighting=False, want_extra=True)
        assert chg is None and nxt is None and extra is None and res.shape == (2, t.ny, t.nx, 1)
        # the float64 chain, frame by frame
        _, _, nxt, _ = sur.poisson_frames(cols, lu, out_scale=sc)
        for i in range(NF):
            want, field = oracle_frame(t, cols[i], frames[i][1], PHI, model4(), MAX_ABS, P_SCALE)
            check_against_chain(nxt[i], want, field, f"frame {i} of the batch")
        assert sur.guard_trips == 0
        free(d_cols, d_extra)


# ------------------------------------------------------------------------------------------------------- GPU, errors
@pytest.mark.gpu
def test_gpu_frame_errors_enqueue_nothing_and_leave_the_handle_usable(ds):
    """Every state and argument error of the five entries returns its code and enqueues nothing (the outputs keep their
    sentinel); the handle then performs a correct step; a new mesh, a new plan and an unbind drop the binding."""
    t = eval_tables(ds)
    cols = np.stack([dataset_columns(ds, i)[0] for i in range(2)])
    lu = np.array([[PHI, dataset_columns(ds, i)[1]] for i in range(2)])
    npix = t.ny * t.nx
    with GridSurrogate(model4(), t.ny, t.nx, max_cases=NF) as sur:
        d_cols = DeviceArray(cols)
        d_out = DeviceArray(np.full((2, 3, npix + 1), CANARY, np.float64))
        d_res = DeviceArray(np.full((2, t.ny, t.nx), CANARY, np.float32))
        plane = lambda n=2, k=8, outs=None, ptr=None: sur.frames_to_grid_device(
            ptr if ptr is not None else d_cols.ptr, n, k, outs if outs is not None else [(d_out.ptr, 3 * (npix + 1), 0)] + [(0, 0, 0)] * (k - 1))
        lu3 = np.vstack([lu, lu[:1]])
        step = lambda n=2, k=8: sur.poisson_frames_device(d_cols.ptr, n, k, lu3[:n], d_res.ptr, False, True)
        raw = lambda n, k, w: sur.lib.psm_poisson_frames_device(sur.h, d_cols.ptr, n, k, lu.ctypes.data_as(_dp), None, 0, w, None, d_res.ptr, None, None, None)
        assert "psm_set_geometry" in error(-2, lambda: sur.bind_frames(2, 8))                      # no mesh
        assert "psm_set_geometry" in error(-2, plane)
        assert "psm_set_geometry" in error(-2, step)
        sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        assert "psm_bind_frames" in error(-2, plane)                                               # a mesh, no binding
        assert "psm_bind_frames" in error(-2, step)
        for n, k in ((0, 8), (NF + 1, 8), (2, 0), (2, 17)):
            error(-1, lambda: sur.bind_frames(n, k))
        assert "psm_bind_frames" in error(-2, plane)                                               # a refused bind binds nothing
        sur.bind_frames(2, 8)
        assert "psm_bind_features" in error(-2, step)
        sur.bind_features(np.repeat(t.sdfunct[None], 2, axis=0), K_ARCSINH, MAX_ABS)
        assert "psm_bind_poststeps" in error(-2, step)
        assert "psm_bind_poststeps" in error(-2, lambda: sur.poisson_frames(cols, lu))
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        for k in (0, 17):
            error(-1, lambda: plane(2, k, [(d_out.ptr, 0, 0)] * k))
        error(-1, lambda: plane(0))
        error(-1, lambda: plane(3))                                                                # three frames, two bound
        error(-1, lambda: plane(2, 8, [(d_out.ptr + 4, 3 * (npix + 1), 0)] + [(0, 0, 0)] * 7))     # float64 plane on a 4-byte boundary
        error(-1, lambda: plane(2, 8, [(d_out.ptr + 2, 6 * (npix + 1), 1)] + [(0, 0, 0)] * 7))     # float32 plane on a 2-byte boundary
        error(-1, lambda: plane(2, 8, [(0, 0, 0)] * 8))                                            # nothing to store
        error(-1, lambda: plane(2, 8, None, 0))                                                    # no columns
        error(-1, lambda: step(3))
        error(-1, lambda: step(0))
        assert raw(2, 3, 0) == -1 and raw(2, 5, 1) == -1 and raw(2, 17, 1) == -1                   # k below 4 / below 6 with the weighting / above 16
        error(-1, lambda: sur.poisson_frames(np.zeros((1, t.n_cells, 9)), lu[:1]))                 # more columns than bound
        bad = lu.copy()
        bad[1, 1] = 0.0
        error(-1, lambda: sur.poisson_frames_device(d_cols.ptr, 2, 8, bad, d_res.ptr, False, True))
        sur.synchronize()
        assert (d_out.numpy() == CANARY).all() and (d_res.numpy() == CANARY).all()                 # nothing was enqueued
        # the handle still works: the stage alone and the whole step, against psm_mesh_to_grid / the composition by hand
        plane()
        sur.synchronize()
        planes = np.stack([mesh_to_grid(sur, cols[i], 1) for i in range(2)])
        out = d_out.numpy()
        assert same_bits(np.ascontiguousarray(out[:, 0, :npix]), planes[:, 0].reshape(2, npix)) and (out[:, 1:] == CANARY).all() and (out[:, 0, npix] == CANARY).all()
        got = frames_device(sur, d_cols, 2, 8, lu, None, False)
        want = by_hand(sur, planes, lu, None, False)
        same = [same_bits(a, b) for a, b in zip(got, want)]
        print(f"after the refused calls: stage identical to psm_mesh_to_grid, step identical to the composition by hand {same}")
        assert all(same)
        # what drops the binding
        sur.unbind_frames()
        assert "psm_bind_frames" in error(-2, plane)
        sur.bind_frames(2, 8)
        assert sur.lib.psm_plan_grid(sur.h, t.ny, t.nx) == 0                                       # a new plan drops the mesh with it
        assert "psm_set_geometry" in error(-2, plane)
        sur.set_mesh(t.vtx, t.wts, t.indices, t.sdfunct, t.n_cells)
        assert "psm_bind_frames" in error(-2, plane)                                               # a new mesh: bind again
        free(d_cols, d_out, d_res)


@pytest.mark.gpu
def test_gpu_frames_are_refused_on_a_case_set():
    """A handle that holds the case set of psm_set_geometry_cases has no single mesh: PSM_ERR_STATE."""
    from test_mesh_cases import set_cases
    _, _, _, model, maxs = cases.build_mesh_case()
    array, top, obst = synthetic.channel_mesh()
    tab = geometry.build_geometry_native(array, top, obst)
    with GridSurrogate(model, tab.ny, tab.nx, 2) as sur:
        rc, msg = set_cases(sur, [tab], [array.shape[0]], maxs)
        assert rc == 0, msg
        assert "case set" in error(-2, lambda: sur.bind_frames(1, 4))
        assert "case set" in error(-2, lambda: sur.frames_to_grid_device(4096, 1, 1, [(4096, 0, 0)]))


# ------------------------------------------------------------------------------------------------------- GPU, the evaluator
def evaluator(c, path=None, **kw):
    return EvaluationPoisson(5e-3, 128, 32, 0.95, 0.95, path or c["dataset_path"], c["model_path"], 128, "std", K_ARCSINH, None,
                             artifact_dir=c["dir"], **kw)


def recompute(ev, field, labels, U):
    """The three error blocks of one frame from the returned field and label planes (delta_p, p), as timeStep states them."""
    cfd = np.nan_to_num(labels[0] / pow(U, 2.0), nan=0.0) / ev.max_abs_delta_p * ev.max_abs_delta_p * pow(U, 2.0)
    p_grid = np.nan_to_num(labels[1], nan=0.0)
    no_flow = np.nan_to_num(ev.sdfunct[..., 0], nan=0.0) / ev.max_abs_dist == 0
    return error_metrics(field, cfd, no_flow), error_metrics((p_grid - cfd) + field, p_grid, no_flow), cfd, no_flow


@pytest.mark.gpu
def test_gpu_evaluator_time_steps(ds):
    """EvaluationPoisson(max_frames=3).timeSteps on the three frames of the dataset: every field within 2e-4 of the float64 chain,
    one metric entry per frame in order, each equal to error_metrics recomputed from the returned field and label planes; a batch
    whose middle frame is irrelevant returns 0 there, records nothing for it and sends two frames."""
    t = eval_tables(ds)
    ev = evaluator(ds, max_frames=NF)
    assert ev.computeOnlyOnce(0) == 0
    fields = ev.timeSteps(0, [0, 1, 2], False, PHI)
    assert len(fields) == 3 and len(ev.label_planes) == 3 and ev._sur.geometry_bound and ev._sur.guard_trips == 0
    assert [len(getattr(ev, "pred_minus_true" + s)) for s in ("", "_deltap_crude", "_p")] == [3, 3, 3]
    chain = []
    for i in range(3):
        cols, U = dataset_columns(ds, i)
        chain.append(oracle_frame(t, cols, U, PHI, ds["model"], cases.POISSON_MAXS[:4], cases.POISSON_MAXS[4]))
        check_against_chain(fields[i], *chain[i], f"timeSteps frame {i}")
        m, mp, cfd, no_flow = recompute(ev, fields[i], ev.label_planes[i], U)
        got = (ev.pred_minus_true[i], ev.pred_minus_true_squared[i], ev.pred_minus_true_p[i], ev.pred_minus_true_squared_p[i])
        print(f"frame {i}: recorded (mean_err, mean_sq_err) of delta_p and p {got}, recomputed {(m['mean_err'], m['mean_sq_err'], mp['mean_err'], mp['mean_sq_err'])}")
        assert got == (m["mean_err"], m["mean_sq_err"], mp["mean_err"], mp["mean_sq_err"])
    # the attributes are those of the last frame
    assert ev.U_max_norm == U and ev.last_metrics["delta_p"] == m and ev.last_metrics["p"] == mp
    assert ev.last_metrics["deltap_crude"] == error_metrics(ev.deltap_res, cfd, no_flow)
    assert np.array_equal(ev.cfd_results, cfd) and np.array_equal(ev.no_flow_bool, no_flow)
    assert np.array_equal(ev.p_pred, (np.nan_to_num(ev.label_planes[2][1], nan=0.0) - cfd) + fields[2], equal_nan=True)
    # a middle frame whose velocity hardly changed (SM_call.py:562-567)
    import h5write
    sim2 = ds["sim"].copy()
    sim2[0, 1, :ds["N"], 5:7] *= 1e-7
    p2 = os.path.join(ds["dir"], "still.hdf5")
    tb, ob = formats.read_dataset(ds["dataset_path"], 0, 0)[1:]
    h5write.write_h5(p2, {"sim_data": sim2, "top_bound": np.repeat(tb, 3, axis=1), "obst_bound": np.repeat(ob, 3, axis=1)})
    ev.dataset_path = p2
    sent = []
    inner = ev._sur.poisson_frames
    ev._sur.poisson_frames = lambda cols, *a, **kw: (sent.append(np.shape(cols)[0]), inner(cols, *a, **kw))[1]
    again = ev.timeSteps(0, [0, 1, 2], False, PHI)
    print(f"middle frame irrelevant: frames sent per call {sent}, entries recorded {len(ev.pred_minus_true) - 3}")
    assert isinstance(again[1], int) and again[1] == 0 and ev.label_planes[1] is None
    assert sent == [2] and len(ev.pred_minus_true) == 5 and len(ev.pred_minus_true_p) == 5
    for i in (0, 2):                                       # two frames on three bound slots take the general route: the same chain
        check_against_chain(again[i], *chain[i], f"frame {i} beside the irrelevant one")
    assert ev.timeSteps(0, [1], False, PHI) == [0] and len(ev.pred_minus_true) == 5


@pytest.mark.gpu
def test_gpu_poisson_main_with_frames_per_call(ds):
    """call_SM_main_Poisson(frames_per_call=2): the keys of the default call, the summaries of timeSteps' own lists."""
    phis = os.path.join(ds["dir"], "phis.txt")
    np.savetxt(phis, np.array([PHI, 0.2]))
    args = (5e-3, ds["model_path"], 128, 0.25, 0.95, 0.95, 128, ds["dataset_path"], False, "std", K_ARCSINH, False, False, False, False, 1, 3, phis)
    kw = dict(artifact_dir=ds["dir"], sim_offset=0, time_offset=0)
    default = call_SM_main_Poisson(*args, **kw)
    out = call_SM_main_Poisson(*args, frames_per_call=2, **kw)
    assert set(out) == set(default) and set(out["overall"]) == set(default["overall"]) and set(out["sims"][0]) == set(default["sims"][0])
    ev = evaluator(ds, max_frames=2)
    ev.computeOnlyOnce(0)
    ev.timeSteps(0, [0, 1, 2], False, PHI)
    want = {"delta_p": surrogate._summary(ev.pred_minus_true, ev.pred_minus_true_squared),
            "delta_p_no_weighting": surrogate._summary(ev.pred_minus_true_deltap_crude, ev.pred_minus_true_squared_deltap_crude),
            "p": surrogate._summary(ev.pred_minus_true_p, ev.pred_minus_true_squared_p)}
    print(f"frames_per_call=2 overall {out['overall']}\ndefault call      overall {default['overall']}")
    assert out["overall"] == want and out["sims"][0]["delta_p"] == want["delta_p"]
    assert out["sims"][0]["sim"] == 0 and out["sims"][0]["phi"] == PHI
