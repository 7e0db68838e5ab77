"""The gradient-model step at the solver boundary (psm_solve_gradp*, psm_solve_cases_gradp*): cells [N,5] -> p [N] through the
U_to_gradP model, the integration and the outlet level, on the single mesh and on a case set.

Shapes: the hand tables of test_poisson_solve.hand_tabs(), restated here with the size, seed, obstacle and cut as arguments -- 130 x 131
(four gradP blocks; nx = 131 leaves partial 64-pixel chunks on both row sides of the integration and an unaligned plane stride), 257
cells (more than one tail workgroup), pixels with several writers and with none, a fifth of the cells with a negative grid -> mesh
weight, obstacle sdf[40:60, 30:50] = 0 with cut (50, 40).  The case set is K = 3 on that grid with max_cases = 4 and (257, 64, 300)
cells: 300 is more than one tail workgroup, 64 less than one; three obstacle rectangles and cuts.

Reference, composed here in float64 from functions the oracle pins and never modified: orc.mesh_to_grid(sdf_div = max_abs_dist,
fill) -> orc.solve_grid (-> scipy's gaussian_filter per component) -> orc.integrate_gradp(sx, sy, cut) -> the outlet shift ->
orc.grid_to_mesh(q - s, cells, geo, 1.0, U), with column 4 set to NaN to mark the fallback cells.  Bound: CHAIN_TOL = 2e-4 of
max|p_ref|, the project's own for solve + integration against the oracle chain (test_gradp_pressure.py); the float64 ends add
nothing to it.  Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib, solver, synthetic
from test_gradp_pressure import CHAIN_TOL, oracle_model

pytestmark = pytest.mark.gpu

NY, NX = 130, 131
MAXS4 = (1.2, 0.5, 0.35, 1.0)             # max_abs_Ux, max_abs_Uy, max_abs_dist, unused
MAX_GRAD = (40.0, 25.0)                   # max_abs_dPdx, max_abs_dPdy
DX, DY, EXTENTS = 0.005, 0.005, (0.655, 0.65)
SX, SY = DX * MAX_GRAD[0] / EXTENTS[0], DY * MAX_GRAD[1] / EXTENTS[1]
S_FIELD, S_WEIGHT = (2.0, 3.0), (2.0, 2.0)
CASES = ((257, 1302, (40, 60, 30, 50), (50, 40)), (64, 1303, (70, 90, 60, 90), (80, 75)), (300, 1304, (20, 50, 80, 100), (35, 90)))
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class Tabs:
    """One mesh's six tables on its grid, as psm_set_geometry takes them, its cut and one frame of cells."""

    def __init__(self, n, seed, rect, cut):
        ng = NY * NX
        rng = np.random.default_rng(seed)
        self.ny, self.nx, self.n_cells, self.cut = NY, NX, n, cut
        self.v1 = rng.integers(0, n, (ng, 3)).astype(np.int32)
        w = rng.random((ng, 2)) * 0.5
        self.w1 = np.ascontiguousarray(np.c_[w, 1.0 - w.sum(axis=1)])
        pix = np.arange(ng)
        moved = rng.random(ng) < 0.15
        pix[moved] = rng.integers(0, ng, int(moved.sum()))
        self.idx = np.ascontiguousarray(np.c_[pix // NX, pix % NX].astype(np.int32))
        self.sdf = 0.02 + 0.3 * rng.random((NY, NX))
        self.sdf[rect[0]:rect[1], rect[2]:rect[3]] = 0.0
        self.v2 = rng.integers(0, ng, (n, 3)).astype(np.int32)
        w = rng.random((n, 2)) * 0.5
        w2 = np.c_[w, 1.0 - w.sum(axis=1)]
        neg = rng.random(n) < 0.2
        w2[neg, 0] = -w2[neg, 0]
        w2[neg, 2] = 1.0 - w2[neg, 0] - w2[neg, 1]
        self.w2 = np.ascontiguousarray(w2)
        self.cells = np.ascontiguousarray(np.c_[1.5 + 0.3 * rng.standard_normal(n), 0.2 * rng.standard_normal(n), rng.random(n), rng.random(n),
                                                0.4 * rng.standard_normal(n)])
        writers = np.bincount(pix, minlength=ng)
        assert (writers == 0).any() and (writers > 1).any()
        self.geo = orc.Geometry(NY, NX, self.v1, self.w1, self.v2, self.w2, self.idx, self.sdf)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def outlet_level(q):
    """s = mean_y(3 q[y, nx-1] - q[y, nx-2]) / 3 in float64 (python_module.py:472 on the integrated plane)."""
    q = np.asarray(q, np.float64)
    return float(np.mean(3.0 * q[:, -1] - q[:, -2]) / 3.0)


class Case:
    """Models, tables and references, built once per module and left unchanged."""

    def __init__(self):
        self.model = synthetic.make_model("gradp", p_in=8, p_out=8)
        self.tabs = [Tabs(*c) for c in CASES]
        self._ref = {}

    def ref(self, k, reference, af):
        """-> (p_ref [N] with NaN on the oracle's fallback cells, q_ref [ny][nx], s_ref, U)."""
        key = (k, reference, af)
        if key not in self._ref:
            t = self.tabs[k]
            grid, U = orc.mesh_to_grid(t.cells, t.geo, MAXS4[0], MAXS4[1], sdf_div=MAXS4[2], fill=True)
            fields = orc.solve_grid(grid.astype(np.float32).astype(np.float64), oracle_model(self.model)).fields
            if af:
                fields = np.stack([ndi.gaussian_filter(fields[..., c], sigma=S_FIELD, order=0) for c in range(2)], axis=-1)
            q = orc.integrate_gradp(fields, t.sdf, SX, SY, t.cut[0], t.cut[1])
            s = outlet_level(q) if reference == "outlet" else 0.0
            marked = np.array(t.cells)
            marked[:, 4] = np.nan
            p = orc.grid_to_mesh(q - s, marked, t.geo, 1.0, U)
            assert np.isfinite(grid).all() and np.isfinite(fields).all() and np.isfinite(q).all() and np.isfinite(s)
            self._ref[key] = (p, q, s, float(U))
        return self._ref[key]


@functools.lru_cache(maxsize=None)
def _case():
    return Case()


@pytest.fixture(scope="module")
def case():
    return _case()


# ------------------------------------------------------------------------------------------------------- handles and calls
def set_geometry(sur, t, g2m=True):
    mx = np.asarray(MAXS4, np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, t.n_cells, t.ny, t.nx, t.v1.ctypes.data_as(_ip), t.w1.ctypes.data_as(_dp), t.idx.ctypes.data_as(_ip),
                                  t.sdf.ctypes.data_as(_dp), t.v2.ctypes.data_as(_ip) if g2m else None, t.w2.ctypes.data_as(_dp) if g2m else None,
                                  mx.ctypes.data_as(_dp), 1, 1, 0.05)
    assert rc == 0, _lib.last_error(sur.h)
    sur.mesh_cells = t.n_cells


def set_geometry_cases(sur, tabs):
    ptrs = lambda name: (C.c_void_p * len(tabs))(*[getattr(t, name).ctypes.data for t in tabs])
    mx = np.asarray(MAXS4, np.float64)
    return sur.lib.psm_set_geometry_cases(sur.h, len(tabs), (C.c_int64 * len(tabs))(*[t.n_cells for t in tabs]), NY, NX, ptrs("v1"), ptrs("w1"), ptrs("idx"),
                                          ptrs("sdf"), ptrs("v2"), ptrs("w2"), mx.ctypes.data_as(_dp), 1, 1, 0.05)


def bind(sur, t, af=0, reference="outlet"):
    if af:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_gradp_solve(t.cut, DX, DY, EXTENTS, MAX_GRAD, af, reference)


def handle(model, t, af=0, reference="outlet"):
    sur = GridSurrogate(model, NY, NX, 1)
    set_geometry(sur, t)
    bind(sur, t, af, reference)
    return sur


def cases_handle(model, tabs, af=0, reference="outlet"):
    sur = GridSurrogate(model, NY, NX, 4)
    assert set_geometry_cases(sur, tabs) == 0, _lib.last_error(sur.h)
    if af:
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
    sur.bind_gradp_solve_cases([t.cut for t in tabs], DX, DY, EXTENTS, MAX_GRAD, af, reference)
    return sur


def device_step(sur, cells, K=0):
    """psm_solve_gradp_device (K = 0) or psm_solve_cases_gradp_device on buffers of its own -> (p, image, gradp, q, scalars)."""
    shape = (lambda *s: s) if K == 0 else (lambda *s: (K,) + s)
    bufs = [DeviceArray(cells), DeviceArray(np.full(len(cells), -7.0)), DeviceArray(np.full(shape(NY, NX, 3), -7.0, np.float32)),
            DeviceArray(np.full(shape(NY, NX, 2), -7.0, np.float32)), DeviceArray(np.full(shape(NY, NX), -7.0, np.float32)),
            DeviceArray(np.full(shape(8), -7.0))]
    try:
        (sur.solve_cases_gradp_device if K else sur.solve_gradp_device)(*[b.ptr for b in bufs])
        sur.synchronize()                                    # the entry is asynchronous on the handle's stream
        return tuple(b.numpy() for b in bufs[1:])
    finally:
        for b in bufs:
            b.free()


def near_wall(t):
    """The near-wall flags as psm_set_geometry derives them: interpolate(sdfunct.flatten()) < 0.05 (PM:492-494)."""
    sdf_mesh = np.zeros(t.n_cells)
    for j in range(3):
        sdf_mesh += t.sdf.reshape(-1)[t.v2[:, j]] * t.w2[:, j]
    return sdf_mesh < 0.05


def numpy_tail(t, q, s, U, scale=None):
    """The tail restated in NumPy float64 on the returned q and s: sequential acc += (q - s) * w over j, one multiply by U * U
    (``scale``: psm_to_mesh_kernel's statements instead, acc * max_abs_p * (U * U)); cells[:,4] on fallback."""
    f = q.reshape(-1).astype(np.float64)[(t.idx[:, 0].astype(np.int64) * t.nx + t.idx[:, 1])]
    acc = np.zeros(t.n_cells)
    for j in range(3):
        acc += (f[t.v2[:, j]] - s) * t.w2[:, j]
    p = acc * (U * U) if scale is None else acc * scale * (U * U)
    fb = near_wall(t) | (t.w2 < 0).any(axis=1) | np.isnan(acc)
    p[fb] = t.cells[fb, 4]
    return p, fb


def check_against_reference(p, t, ref, what):
    """Fallback cells hold cells[:,4] bit for bit, the others p within CHAIN_TOL of max|p_ref|; -> the measured ratio."""
    p_ref = ref[0]
    fb = np.isnan(p_ref)
    assert 0.0 < fb.mean() < 0.5, fb.mean()                 # asserted on the oracle before the device is looked at
    unchanged = bits(p) == bits(np.ascontiguousarray(t.cells[:, 4]))
    scale = float(np.abs(p_ref[~fb]).max())
    err = float(np.abs(p[~fb] - p_ref[~fb]).max() / scale)
    print(f"{what}: max|p - p_ref| / max|p_ref| = {err:.3e} (max|p_ref| {scale:.3e}, s_ref {ref[2]:.4e}, U {ref[3]:.4f}, fallback share {fb.mean():.3f})")
    assert np.array_equal(unchanged, fb)                    # the fallback set equals the oracle's exactly
    assert err <= CHAIN_TOL, (what, err)
    return err


def expect_error(code, words, call):
    with pytest.raises(_lib.PsmError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("reference", ("none", "outlet"))
@pytest.mark.parametrize("af", (0, 1))
def test_oracle_parity(case, reference, af):
    """psm_solve_gradp on the hand tables against the composed float64 reference: fallback cells equal cells[:,4] bit for bit and are
    exactly the oracle's (their share lies in (0, 0.5)), elsewhere |p - p_ref| <= 2e-4 * max|p_ref|.
    Measured on an MI355X, max|p - p_ref| / max|p_ref|: 3.6e-7 (reference none) and 3.1e-7 (outlet) without the filter, 3.4e-7 and
    3.1e-7 with it; fallback share 0.237 (61 of 257 cells).  DESIGN.md section 0.3 carries the same figures."""
    t = case.tabs[0]
    ref = case.ref(0, reference, af)
    sur = handle(case.model, t, af, reference)
    try:
        p = sur.solve_gradp(t.cells)
    finally:
        sur.close()
    check_against_reference(p, t, ref, f"reference={reference} apply_filter={af}")


@pytest.mark.parametrize("reference", ("outlet", "none"))
def test_bit_identity_with_the_existing_chain(case, reference):
    """The step's solve and integration ARE the existing chain: on the same handle and the same solve route, d_pgrid and d_gradp of the
    step equal, bit for bit, psm_solve_pressure_device fed the step's own d_image (psm_bind_integration with (sx, sy)), which returns
    the same bits again afterwards.  The route: the step takes the geometry binding psm_set_geometry makes for psm_solve, which no
    grid entry of a two-channel handle can take (it is scoped to the mesh entries, and its bits differ from the general path's in the
    last place: measured here, printed below); so the comparison runs after psm_bind_geometry on the step's image, the binding both
    entries take.  On either route: a step is reproducible, d_scalars holds U and U^2 as NumPy computes them, s is within
    1e-12 * max|q| of the NumPy float64 mean, and p equals the tail restated in NumPy float64 on the returned q and s; with
    reference = none p also equals the statements of psm_to_mesh_kernel's body for max_abs_p = 1 (restated in NumPy: the device
    body of that kernel is compiled with fused multiply-adds, this one rounds every operation)."""
    t = case.tabs[0]
    sur = handle(case.model, t, 0, reference)
    try:
        own = device_step(sur, t.cells)                      # on the binding of psm_set_geometry
        own_again = device_step(sur, t.cells)
        assert sur.bind_geometry(own[1]) and sur.geometry_bound
        assert sur.bind_integration(t.sdf, t.cut[0], t.cut[1], SX, SY)
        step = device_step(sur, t.cells)                     # on the binding every single-case solve takes
        d_img, d_q, d_g = DeviceArray(step[1]), DeviceArray(np.full((NY, NX), -7.0, np.float32)), DeviceArray(np.full((NY, NX, 2), -7.0, np.float32))
        try:
            chain = []
            for _ in range(2):
                sur.solve_pressure_device(d_img.ptr, 1, d_q.ptr, d_g.ptr)
                sur.synchronize()
                chain.append((d_q.numpy(), d_g.numpy()))
            behind = device_step(sur, t.cells)
            sur.solve_pressure_device(d_img.ptr, 1, d_q.ptr, d_g.ptr)
            sur.synchronize()
            chain.append((d_q.numpy(), d_g.numpy()))
        finally:
            for d in (d_img, d_q, d_g):
                d.free()
    finally:
        sur.close()
    same_q, same_g = [same_bits(step[3], c[0]) for c in chain], [same_bits(step[2], c[1]) for c in chain]
    routes = float(np.abs(own[3].astype(np.float64) - step[3]).max() / np.abs(step[3]).max())
    print(f"reference={reference}: q identical to psm_solve_pressure_device on the step's image {same_q}, the gradient {same_g}; "
          f"the two bindings' q differ by {routes:.3e} of max|q|, their images are identical: {same_bits(own[1], step[1])}")
    assert all(same_bits(x, y) for x, y in zip(own_again, own))          # a step is reproducible,
    assert all(same_bits(x, y) for x, y in zip(behind, step))            # also behind the other entry
    assert all(same_q) and all(same_g) and same_bits(own[1], step[1])
    assert routes <= 2 * CHAIN_TOL                                        # each route is within CHAIN_TOL of the oracle chain
    U = float(np.max(np.sqrt(np.square(t.cells[:, 0]) + np.square(t.cells[:, 1]))))
    for what, (p, image, gradp, q, scalars) in (("psm_set_geometry's binding", own), ("psm_bind_geometry", step)):
        s_np = outlet_level(q) if reference == "outlet" else 0.0
        print(f"reference={reference}, {what}: scalars {scalars}; |s - s_np| = {abs(scalars[2] - s_np):.3e} (max|q| {np.abs(q).max():.3e})")
        assert np.isfinite(q).all() and np.isfinite(image).all() and np.isfinite(gradp).all()
        assert same_bits(scalars[[0, 1, 3, 4, 5, 6, 7]], np.array([U, U * U, SX, SY, 0.0, 0.0, 0.0]))
        assert abs(scalars[2] - s_np) <= 1e-12 * np.abs(q).max() and (reference == "outlet" or same_bits(scalars[2:3], np.zeros(1)))
        p_np, fb = numpy_tail(t, q, scalars[2], U)
        print(f"reference={reference}, {what}: p identical to the NumPy tail {same_bits(p, p_np)}, fallback share {fb.mean():.3f}, max|p| {np.abs(p).max():.3e}")
        assert 0.0 < fb.mean() < 1.0 and same_bits(p, p_np)
        if reference == "none":
            assert same_bits(p, numpy_tail(t, q, 0.0, U, scale=1.0)[0])


def test_case_set(case):
    """K = 3 on one handle (max_cases = 4): for every case p, q and s are bit-identical to a single-mesh handle with that case's
    tables; changing another case's cells changes no bit of this case; the host entry equals the device entry; oracle parity per case
    (measured on an MI355X: 3.1e-7, 5.1e-7 and 4.5e-7 of max|p_ref| for the 257-, 64- and 300-cell case)."""
    tabs = case.tabs
    off = np.cumsum([0] + [t.n_cells for t in tabs])
    cells = np.ascontiguousarray(np.concatenate([t.cells for t in tabs]))
    sur = cases_handle(case.model, tabs)
    try:
        p, image, gradp, q, scalars = device_step(sur, cells, K=3)
        host = sur.solve_cases_gradp(cells)
        other = cells.copy()
        other[off[1]:off[2], 0] *= 1.7                       # case 1 gets another velocity field (and another U)
        other[off[1]:off[2], 4] += 0.3
        p2, _, _, q2, scalars2 = device_step(sur, other, K=3)
    finally:
        sur.close()
    assert same_bits(host, p)
    for k, t in enumerate(tabs):
        one = handle(case.model, t)
        try:
            p1, image1, gradp1, q1, scalars1 = device_step(one, t.cells)
        finally:
            one.close()
        pk = p[off[k]:off[k + 1]]
        same = [same_bits(pk, p1), same_bits(image[k], image1), same_bits(gradp[k], gradp1), same_bits(q[k], q1), same_bits(scalars[k], scalars1)]
        print(f"case {k} ({t.n_cells} cells): (p, image, gradient, q, scalars) identical to the single mesh {same}")
        assert all(same)
        check_against_reference(pk, t, case.ref(k, "outlet", 0), f"case {k}")
        if k != 1:
            assert same_bits(p2[off[k]:off[k + 1]], pk) and same_bits(q2[k], q[k]) and same_bits(scalars2[k], scalars[k])
    assert not same_bits(q2[1], q[1]) and scalars2[1][0] != scalars[1][0]


def test_errors_and_lifetime(case):
    t, m = case.tabs[0], case.model
    args = (DX, DY, EXTENTS, MAX_GRAD)
    sur = GridSurrogate(m, NY, NX, 4)
    try:
        expect_error(-2, ["psm_set_geometry has not", "psm_bind_gradp_solve_cases"], lambda: sur.bind_gradp_solve(t.cut, *args))
        expect_error(-2, ["psm_set_geometry_cases has not", "psm_bind_gradp_solve"], lambda: sur.bind_gradp_solve_cases([t.cut], *args))
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        set_geometry(sur, t)
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        expect_error(-2, ["single mesh", "psm_bind_gradp_solve"], lambda: sur.bind_gradp_solve_cases([t.cut], *args))
        expect_error(-2, ["psm_bind_poststeps"], lambda: sur.bind_gradp_solve(t.cut, *args, apply_filter=True))
        for bad in ((0.0, DY, EXTENTS, MAX_GRAD), (DX, np.nan, EXTENTS, MAX_GRAD), (DX, DY, (0.0, 0.65), MAX_GRAD), (DX, DY, (0.655, np.inf), MAX_GRAD),
                    (DX, DY, EXTENTS, (0.0, 25.0)), (DX, DY, EXTENTS, (40.0, np.nan))):
            expect_error(-1, ["finite and non-zero"], lambda: sur.bind_gradp_solve(t.cut, *bad))
        assert sur.lib.psm_bind_gradp_solve(sur.h, t.cut[0], t.cut[1], DX, DY, EXTENTS[0], EXTENTS[1], np.asarray(MAX_GRAD).ctypes.data_as(_dp), 0, 2) == -1
        assert "reference" in _lib.last_error(sur.h)
        expect_error(-1, ["cut outside the grid"], lambda: sur.bind_gradp_solve((0, 40), *args))
        expect_error(-5, ["flow-cell counts"], lambda: sur.bind_gradp_solve((50, 30), *args))    # column 29 is flow, column 30 solid
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))     # a refused bind binds nothing
        sur.bind_gradp_solve(t.cut, *args)
        first = sur.solve_gradp(t.cells)
        expect_error(-1, ["cell count"], lambda: sur.solve_gradp(t.cells[:-1]))
        expect_error(-2, ["single mesh", "psm_solve_gradp"], lambda: sur.solve_cases_gradp(t.cells))
        d = DeviceArray(np.zeros(8 * t.n_cells + 1))
        try:
            expect_error(-1, ["misaligned"], lambda: sur.solve_gradp_device(d.ptr + 4, d.ptr + 8 * 5 * t.n_cells))
            expect_error(-1, ["misaligned"], lambda: sur.solve_gradp_device(d.ptr, d.ptr + 8 * 5 * t.n_cells, d_gradp=d.ptr + 4))
            expect_error(-1, ["misaligned"], lambda: sur.solve_gradp_device(d.ptr, d.ptr + 8 * 5 * t.n_cells, d_pgrid=d.ptr + 2))
        finally:
            d.free()
        p = np.empty(t.n_cells)                              # psm_solve itself keeps refusing the two-channel model
        assert sur.lib.psm_solve(sur.h, t.cells.ctypes.data_as(_dp), t.n_cells, 0, p.ctypes.data_as(_dp)) == -5
        assert same_bits(sur.solve_gradp(t.cells), first)
        # the binding goes with the plan, the model, the mesh and its own unbind; a step after rebinding gives the first step's bits
        sur._chk(sur.lib.psm_plan_grid(sur.h, 160, 200))
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        set_geometry(sur, t)
        sur.bind_gradp_solve(t.cut, *args)
        assert same_bits(sur.solve_gradp(t.cells), first)
        sc = [np.ascontiguousarray(getattr(m, f), np.float64) for f in ("in_a", "in_b", "out_a", "out_b")]
        sur._chk(sur.lib.psm_set_scaler(sur.h, *[a.ctypes.data_as(_dp) for a in sc]))
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        set_geometry(sur, t)                                 # (a model setter also drops the geometry binding of the solve: set it again)
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        sur.bind_gradp_solve(t.cut, *args)
        assert same_bits(sur.solve_gradp(t.cells), first)
        sur.unbind_gradp_solve()
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        # with apply_filter the post-steps carry the binding; without it they do not
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        sur.bind_gradp_solve(t.cut, *args, apply_filter=True)
        filtered = sur.solve_gradp(t.cells)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        expect_error(-2, ["psm_bind_gradp_solve has not"], lambda: sur.solve_gradp(t.cells))
        sur.bind_gradp_solve(t.cut, *args, apply_filter=True)
        assert same_bits(sur.solve_gradp(t.cells), filtered) and not same_bits(filtered, first)
        sur.bind_gradp_solve(t.cut, *args)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        assert same_bits(sur.solve_gradp(t.cells), first)
        # no grid -> mesh tables
        set_geometry(sur, t, g2m=False)
        expect_error(-1, ["grid->mesh tables"], lambda: sur.bind_gradp_solve(t.cut, *args))
        # a case set: the single-mesh entries name the other form; the set serves the gradient step alone
        assert set_geometry_cases(sur, case.tabs[:2]) == 0, _lib.last_error(sur.h)
        expect_error(-2, ["case set", "psm_bind_gradp_solve_cases"], lambda: sur.bind_gradp_solve(t.cut, *args))
        expect_error(-5, ["case 1", "flow-cell counts"], lambda: sur.bind_gradp_solve_cases([t.cut, (80, 60)], *args))
        sur.bind_gradp_solve_cases([x.cut for x in case.tabs[:2]], *args)
        expect_error(-2, ["case set", "psm_solve_cases_gradp"], lambda: sur.solve_gradp(t.cells))
        both = np.ascontiguousarray(np.concatenate([x.cells for x in case.tabs[:2]]))
        assert same_bits(sur.solve_cases_gradp(both)[:t.n_cells], first)
        out = np.empty(len(both))
        for entry in (sur.lib.psm_solve_cases, sur.lib.psm_solve_cases_delta):
            assert entry(sur.h, both.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == -5
        assert sur.lib.psm_delta_prime_cases(sur.h, both.ctypes.data_as(_dp)) == -5
    finally:
        sur.close()
    three = synthetic.make_model("deltas", p_in=32, p_out=32)    # c_in == 3, c_out == 1
    sur = GridSurrogate(three, NY, NX, 1)
    try:
        set_geometry(sur, t)
        expect_error(-5, ["c_out == 2"], lambda: sur.bind_gradp_solve(t.cut, *args))
        expect_error(-5, ["c_out == 2"], lambda: sur.bind_gradp_solve_cases([t.cut], *args))
    finally:
        sur.close()


def channel_case(k):
    a, top, obst = synthetic.channel_mesh(step=k)
    return np.ascontiguousarray(a), top, obst


def test_solver_module_and_ensemble(case):
    """SolverModule(step="gradp").py_func equals solve_gradp on its own tables bit for bit, SolverEnsemble(step="gradp").py_func
    equals solve_cases_gradp; the default cut is the stated rule; the state entries raise."""
    maxs5 = (2.5, 0.6, 0.35) + MAX_GRAD
    a0, top, obst = channel_case(0)
    a3 = channel_case(3)[0]
    sm = SolverModule(case.model, maxs5, step="gradp")
    assert sm.init_func(a0, top, obst) == 0
    try:
        g = sm.tables
        got = [sm.py_func(a0), sm.py_func(a3)]
        cut, (ny, nx) = sm.cut_used, (g.ny, g.nx)
        with pytest.raises(RuntimeError, match="no state"):
            sm.prime(a0)
        with pytest.raises(RuntimeError, match="begin / end"):
            sm.py_func_begin(a0)
    finally:
        sm._sur.close()
    sd = np.asarray(g.sdfunct, np.float64).reshape(ny, nx)
    rows = 1 + np.flatnonzero((sd[1:-1, 1:-1] == 0).any(axis=1))
    cy = int((rows.min() + rows.max() + 1) // 2)
    dx, dy, extents, x_min = solver.gradp_grid_metrics(a0, ny, nx)
    xl = np.linspace(x_min, x_min + extents[0], nx)
    cx = int(((xl[sd[cy] == 0].max() + xl[sd[cy] == 0].min()) / 2 - g.x0) / 5e-3)
    print(f"SolverModule(step='gradp'): grid {ny} x {nx}, default cut {cut}, the rule gives {(cy, cx)}; dx {dx:.6f} dy {dy:.6f} extents {extents}")
    assert cut == (cy, cx) and extents == (round(a0[:, 2].max(), 2) - round(a0[:, 2].min(), 2), round(a0[:, 3].max(), 2) - round(a0[:, 3].min(), 2))
    sur = GridSurrogate(case.model, ny, nx, 1)
    try:
        mx = np.asarray(maxs5[:3] + (1.0,), np.float64)
        v1, w1 = np.ascontiguousarray(g.vtx_m2g, np.int32), np.ascontiguousarray(g.wts_m2g, np.float64)
        v2, w2 = np.ascontiguousarray(g.vtx_g2m, np.int32), np.ascontiguousarray(g.wts_g2m, np.float64)
        idx = np.ascontiguousarray(g.indices, np.int32)
        sur._chk(sur.lib.psm_set_geometry(sur.h, len(a0), ny, nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                          sd.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05))
        sur.bind_gradp_solve(cut, dx, dy, extents, MAX_GRAD, False, "outlet")
        want = [sur.solve_gradp(a0), sur.solve_gradp(a3)]
    finally:
        sur.close()
    same = [same_bits(x, y) for x, y in zip(got, want)]
    moved = float(np.abs(got[0] - a0[:, 4]).max())
    print(f"SolverModule(step='gradp') identical to solve_gradp {same}; max|p - p_prev| {moved:.3e}, cells that keep p_prev {np.mean(got[0] == a0[:, 4]):.3f}")
    assert all(same) and moved > 0 and np.isfinite(got[0]).all()
    ens = SolverEnsemble(case.model, maxs5, max_cases=2, step="gradp")      # the library's own table builder
    assert ens.init_func([a0, a3], [top, top], [obst, obst]) == 0
    try:
        p = ens.py_func([a0, a3])
        cells = np.ascontiguousarray(np.concatenate([a0, a3]))
        direct = ens._sur.solve_cases_gradp(cells)
        with pytest.raises(RuntimeError, match="no state"):
            ens.reset_state()
        cuts = ens.cuts_used
    finally:
        ens._sur.close()
    print(f"SolverEnsemble(step='gradp'): cuts {cuts}; identical to solve_cases_gradp {same_bits(np.concatenate(p), direct)}")
    assert same_bits(np.concatenate(p), direct) and len(cuts) == 2 and np.isfinite(direct).all() and np.abs(p[1] - a3[:, 4]).max() > 0
