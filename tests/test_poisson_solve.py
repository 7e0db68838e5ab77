"""The Poisson-model step at the solver boundary (psm_solve_poisson*): cells [N,5] -> p [N] with U(t-1), dU(t-1) and p(t-2) kept on the
device.  Every check is on dp = p_out - cells[:,4], never on p: the previous pressure is of the size of p and would hide any error.

The case is test_delta_step.py's: ``synthetic.channel_mesh(step=k)`` for k in {0, 3, 5, 6} -- 16 021 cells (15 * 1024 + 661 for the
partial launch, 62 * 256 + 149 for the tail), a 138 x 300 grid, tables from ``orc.init_geometry`` -- behind ``model4()`` of
test_poisson_step_device.py (c_in = 4, p_in = 48, p_out = 40), phi = 0.16 and max_abs = (2.7, 0.004, 0.004, 0.35, 0.005): on this case
U ~ 2.16, max|dU| ~ 0.005-0.010 and max|dp_prev| ~ 0.015-0.030, so the image channels are O(0.1-1) and the field is of the size of
dp_prev.  The reference of a step is composed here in float64, once per frame triple, from functions the oracle pins (NumPy columns,
interpolate_fill + scatter with NaN -> 0 on the two weighting planes, poisson_features, solve_grid, scipy's gaussian_filter as in
test_poisson_step_device.chain, grid_to_mesh with column 4 set to NaN to mark the fallback cells) and never modified.
Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverModule, _lib, geometry, synthetic
from test_oracle_golden import oracle_model
from test_poisson_step_device import K, S_FIELD, S_WEIGHT, SOLVE_TOL, chain, model4

pytestmark = pytest.mark.gpu

PHI = 0.16
MAXS5 = (2.7, 0.004, 0.004, 0.35, 0.005)  # max_abs_Poisson_term_1, max_abs_delta_Ux, max_abs_delta_Uy, max_abs_dist, max_abs_delta_p
CONFIGS = ((1, 1), (1, 0), (0, 0))       # (weighting, apply_filter)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


class Tabs:
    """One mesh's six tables on its grid, as psm_set_geometry takes them."""

    def __init__(self, ny, nx, n_cells, v1, w1, idx, sdf, v2, w2):
        self.ny, self.nx, self.n_cells = int(ny), int(nx), int(n_cells)
        self.v1, self.w1 = np.ascontiguousarray(v1, np.int32), np.ascontiguousarray(w1, np.float64)
        self.idx, self.sdf = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(sdf, np.float64).reshape(ny, nx)
        self.v2 = None if v2 is None else np.ascontiguousarray(v2, np.int32)
        self.w2 = None if w2 is None else np.ascontiguousarray(w2, np.float64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------------- the float64 reference
def columns(a0, a1, a2):
    """The six cell columns of a step on frames (t-2, t-1, t) and its scalars, in the statements of the header comment."""
    U = np.max(np.sqrt(np.square(a2[:, 0]) + np.square(a2[:, 1])))
    dU, dU_prev = a2[:, 0:2] - a1[:, 0:2], a1[:, 0:2] - a0[:, 0:2]
    cc = np.abs(dU - dU_prev).sum(axis=-1)
    c = cc.max()
    w = cc / c if c != 0 else np.zeros_like(cc)
    cols = np.ascontiguousarray(np.c_[a2[:, 0], a2[:, 1], dU[:, 0], dU[:, 1], w, a2[:, 4] - a1[:, 4]])
    return cols, float(U), float(c)


def plane(t, col):
    g = np.zeros((t.ny, t.nx))
    g[tuple(t.idx.T)] = orc.interpolate_fill(np.asarray(col, np.float64).reshape(-1), t.v1, t.w1)
    return g


def g2m(t, field, cells):
    """grid -> mesh of the dimensional field: dp [N], NaN on the oracle's fallback cells (PM:481-496 applied to dp)."""
    geo = orc.Geometry(t.ny, t.nx, t.v1, t.w1, t.v2, t.w2, t.idx, t.sdf)
    marked = np.array(cells, np.float64)
    marked[:, 4] = np.nan
    return orc.grid_to_mesh(field, marked, geo, 1.0, 1.0)


class Case:
    """Inputs and references, built once per module and left unchanged."""

    def __init__(self):
        self.model = model4()
        self.arrays = {k: np.ascontiguousarray(synthetic.channel_mesh(step=k)[0]) for k in (0, 3, 5, 6)}
        still = self.arrays[5].copy()
        still[:, 0:2] = 0.0
        self.arrays["still"] = still                         # a frame with all velocities zero: a skipped step
        _, self.top, self.obst = synthetic.channel_mesh()
        geo = orc.init_geometry(self.arrays[0], self.top, self.obst)
        self.tabs = Tabs(geo.ny, geo.nx, len(self.arrays[0]), geo.vert_m2g, geo.wts_m2g, geo.indices, geo.sdfunct, geo.vert_g2m, geo.wts_g2m)
        self._solve, self._ref = {}, {}

    def solve(self, f0, f1, f2):
        """-> (field [ny][nx], weight plane, dp_prev plane): what does not depend on (weighting, apply_filter)."""
        key = (f0, f1, f2)
        if key not in self._solve:
            t = self.tabs
            cols, U, _ = columns(self.arrays[f0], self.arrays[f1], self.arrays[f2])
            g = [plane(t, cols[:, q]) for q in range(6)]
            for q in (4, 5):
                g[q][np.isnan(g[q])] = 0.0                   # the entry's decision on the two weighting planes
            grid, _ = orc.poisson_features(g[0], g[1], g[2], g[3], t.sdf, PHI, U, K, MAXS5[:4])
            om = oracle_model(self.model)
            om.out_scale = MAXS5[4] * U ** 2
            self._solve[key] = (orc.solve_grid(grid, om).fields[..., 0], g[4], g[5])
        return self._solve[key]

    def ref(self, f0, f1, f2, weighting, af):
        """-> (dp_ref [N] with NaN on the fallback cells, the bound's scale max(max|gathered field|, max|solve field|))."""
        key = (f0, f1, f2, weighting, af)
        if key not in self._ref:
            field, w, prev = self.solve(f0, f1, f2)
            res, _, nxt = chain(field, w, prev, af)
            f = nxt if weighting else res
            self._ref[key] = (g2m(self.tabs, f, self.arrays[f2]), float(max(np.abs(f).max(), np.abs(field).max())))
        return self._ref[key]


@pytest.fixture(scope="module")
def case():
    return Case()


# ------------------------------------------------------------------------------------------------------- handles and calls
def set_geometry(sur, t, maxs4=MAXS5[1:]):
    mx = np.asarray(maxs4, np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, t.n_cells, t.ny, t.nx, t.v1.ctypes.data_as(_ip), t.w1.ctypes.data_as(_dp), t.idx.ctypes.data_as(_ip),
                                  t.sdf.ctypes.data_as(_dp), None if t.v2 is None else t.v2.ctypes.data_as(_ip),
                                  None if t.w2 is None else t.w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    assert rc == 0, _lib.last_error(sur.h)
    sur.mesh_cells = t.n_cells


def handle(model, t, weighting=1, af=1, bind=True):
    sur = GridSurrogate(model, t.ny, t.nx, 1)
    set_geometry(sur, t)
    if bind:
        sur.bind_features(t.sdf, K, MAXS5[:4])
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        sur.bind_frames(1, 6)
        sur.bind_poisson_solve(PHI, MAXS5[4], weighting, af)
    return sur


def step(sur, array):
    p = np.full(len(array), -7.0)
    rc = sur.lib.psm_solve_poisson(sur.h, array.ctypes.data_as(_dp), len(array), 0, p.ctypes.data_as(_dp))
    assert rc == 0, _lib.last_error(sur.h)
    return p


def device_step(sur, array):
    """psm_solve_poisson_device on buffers of its own -> (p [N], fields [3][ny][nx] float32, scalars [8])."""
    d_cells, d_p = DeviceArray(array), DeviceArray(np.full(len(array), -7.0))
    d_f, d_s = DeviceArray(np.full((3, sur.ny, sur.nx), -7.0, np.float32)), DeviceArray(np.full(8, -7.0))
    try:
        sur.solve_poisson_device(d_cells.ptr, d_p.ptr, d_f.ptr, d_s.ptr)
        sur.synchronize()                                    # the entry is asynchronous on the handle's stream
        return d_p.numpy(), d_f.numpy(), d_s.numpy()
    finally:
        for d in (d_cells, d_p, d_f, d_s):
            d.free()


def check_against_reference(p, array, ref, what):
    """Fallback cells hold cells[:,4] bit for bit, the others dp within SOLVE_TOL of the grid scale; -> the measured ratio."""
    dp_ref, scale = ref
    fb = np.isnan(dp_ref)
    assert 0.0 < fb.mean() < 0.5, fb.mean()                 # both branches of the last kernel are exercised
    assert same_bits(p[fb], array[fb, 4])
    # p = prev + dp rounds at ulp(p): the recovered dp carries up to one ulp of p (p is O(1): 1e-16 against 2e-4 * 1e-2)
    err = float(np.abs((p[~fb] - array[~fb, 4]) - dp_ref[~fb]).max() / scale)
    print(f"{what}: max|dp - dp_ref| / scale = {err:.3e} (scale {scale:.3e}, max|dp_ref| {np.abs(dp_ref[~fb]).max():.3e}, fallback share {fb.mean():.3f})")
    assert err <= SOLVE_TOL, (what, err)
    return err


@functools.lru_cache(maxsize=None)
def _run_cached(weighting, af):
    return {}


def run(case, weighting, af):
    """push 0, push 3, steps 5 and 6 through the host entry, once per configuration -> {5: p, 6: p, "state": (frames, steps)}."""
    out = _run_cached(weighting, af)
    if not out:
        sur = handle(case.model, case.tabs, weighting, af)
        try:
            sur.poisson_solve_push(case.arrays[0])
            sur.poisson_solve_push(case.arrays[3])
            out[5], out[6] = step(sur, case.arrays[5]), step(sur, case.arrays[6])
            out["state"] = sur.poisson_solve_state
        finally:
            sur.close()
    return out


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("weighting,af", CONFIGS)
def test_oracle_parity(case, weighting, af):
    """Push 0, push 3, then steps 5 and 6, each against its composed float64 reference: fallback cells equal cells[:,4] bit for bit
    (their share lies in (0, 0.5)), elsewhere |dp - dp_ref| <= 2e-4 * max(max|gathered field_ref|, max|solve field_ref|).
    Measured on an MI355X, max|dp - dp_ref| / scale for steps 5 and 6: 1.8e-7 and 1.4e-7 (weighting, filter), 1.9e-7 and 1.4e-7
    (weighting, no filter), 4.0e-7 and 5.2e-7 (neither); fallback share 0.173 (2768 of 16 021 cells)."""
    got = run(case, weighting, af)
    for f0, f1, f2 in ((0, 3, 5), (3, 5, 6)):
        check_against_reference(got[f2], case.arrays[f2], case.ref(f0, f1, f2, weighting, af), f"weighting={weighting} apply_filter={af} step {f1} -> {f2}")
    assert got["state"] == (2, 2)


def test_nan_to_zero_matters(case):
    """The last writer of pixel (0,0) has a negative weight, so without the NaN -> 0 rule on the two weighting planes every pixel
    within the sigma = 50 filter's 200-pixel radius, and every cell under it, would fall back; with it the cells that come back with
    cells[:,4] are exactly the reference's fallback set."""
    t = case.tabs
    flat = t.idx[:, 0].astype(np.int64) * t.nx + t.idx[:, 1]
    last = np.flatnonzero(flat == 0)[-1]
    n_neg = int((t.w1 < 0).any(axis=1).sum())
    print(f"{n_neg} lattice points with a negative weight; the last writer of pixel (0,0) is point {last} with weights {t.w1[last]}")
    assert n_neg > 0 and (t.w1[last] < 0).any()
    got = run(case, 1, 1)
    for f0, f1, f2 in ((0, 3, 5), (3, 5, 6)):
        fb = np.isnan(case.ref(f0, f1, f2, 1, 1)[0])
        unchanged = bits(got[f2]) == bits(case.arrays[f2][:, 4])
        print(f"step {f1} -> {f2}: {int(unchanged.sum())} cells came back with cells[:,4], {int(fb.sum())} fallback cells in the reference")
        assert np.array_equal(unchanged, fb)


def evaluator_tabs(case):
    """The evaluator's mesh -> grid tables of the case (IDW fallback: no negative weight) with random grid -> mesh tables."""
    a = case.arrays[0]
    t = geometry.build_geometry_evaluator(a[:, 2:4], a[:, 4], case.top, case.obst, 5e-3, idw_fallback=True)
    rng = np.random.default_rng(77)
    ng, n = t.ny * t.nx, len(a)
    v2 = rng.integers(0, ng, (n, 3)).astype(np.int32)
    w = rng.random((n, 2)) * 0.5
    w2 = np.c_[w, 1.0 - w.sum(axis=1)]
    neg = rng.random(n) < 0.2
    w2[neg, 0] = -w2[neg, 0]
    w2[neg, 2] = 1.0 - w2[neg, 0] - w2[neg, 1]
    return Tabs(t.ny, t.nx, n, t.vtx_m2g, t.wts_m2g, t.indices, t.sdfunct, v2, w2), [case.arrays[k] for k in (0, 3, 5)]


def hand_tabs():
    """257 mesh cells on 130 x 131: random simplices with positive weights in both directions, 15 % of the lattice points redirected
    to another pixel (pixels with several writers and with none), a fifth of the mesh cells with a negative grid -> mesh weight."""
    ny, nx, n = 130, 131, 257
    ng = ny * nx
    rng = np.random.default_rng(1302)
    v1 = rng.integers(0, n, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    w1 = np.c_[w, 1.0 - w.sum(axis=1)]
    pix = np.arange(ng)
    moved = rng.random(ng) < 0.15
    pix[moved] = rng.integers(0, ng, int(moved.sum()))
    idx = np.c_[pix // nx, pix % nx].astype(np.int32)
    sdf = 0.02 + 0.3 * rng.random((ny, nx))
    sdf[40:60, 30:50] = 0.0
    v2 = rng.integers(0, ng, (n, 3)).astype(np.int32)
    w = rng.random((n, 2)) * 0.5
    w2 = np.c_[w, 1.0 - w.sum(axis=1)]
    neg = rng.random(n) < 0.2
    w2[neg, 0] = -w2[neg, 0]
    w2[neg, 2] = 1.0 - w2[neg, 0] - w2[neg, 1]
    frames = []
    for s in range(3):
        f = np.c_[1.5 + 0.3 * rng.standard_normal(n) + 0.004 * s, 0.2 * rng.standard_normal(n) - 0.003 * s, rng.random(n), rng.random(n),
                  0.4 * rng.standard_normal(n) + 0.02 * s]
        frames.append(np.ascontiguousarray(f if s == 0 else frames[0] + 0.01 * (s + rng.random((n, 5))) * np.array([1, 1, 0, 0, 2.0])))
    writers = np.bincount(pix, minlength=ng)
    assert (writers == 0).any() and (writers > 1).any()
    return Tabs(ny, nx, n, v1, w1, idx, sdf, v2, w2), frames


def numpy_tail(t, nxt, cells, near_wall):
    """The tail restated in NumPy float64 on the returned field: sequential acc += f * w over j, then one add; cells[:,4] on fallback."""
    f = nxt.reshape(-1).astype(np.float64)[(t.idx[:, 0].astype(np.int64) * t.nx + t.idx[:, 1])]
    acc = np.zeros(t.n_cells)
    for j in range(3):
        acc += f[t.v2[:, j]] * t.w2[:, j]
    p = cells[:, 4] + acc
    fb = near_wall | (t.w2 < 0).any(axis=1) | np.isnan(acc)
    p[fb] = cells[fb, 4]
    return p, fb


@pytest.mark.parametrize("which", ("evaluator", "hand"))
def test_bit_identity_with_the_existing_chain(case, which):
    """On tables without a negative mesh -> grid weight, d_fields of psm_solve_poisson_device equals, bit for bit, psm_poisson_frames
    (k = 6, weighting, one frame) fed host-made float64 columns, (L, U) and out_scale; d_scalars equals the NumPy values; p_out equals
    the tail restated in NumPy float64 on the returned `next`."""
    t, (a0, a1, a2) = evaluator_tabs(case) if which == "evaluator" else hand_tabs()
    assert not (t.w1 < 0).any()
    cols, U, c = columns(a0, a1, a2)
    U2 = U * U
    scale = MAXS5[4] * U2
    sur = handle(case.model, t, 1, 1)
    try:
        want = sur.poisson_frames(cols[None], [[PHI, U]], out_scale=[scale], apply_filter=True, weighting=True, want_extra=False)
        sur.poisson_solve_push(a0)
        sur.poisson_solve_push(a1)
        p, fields, scalars = device_step(sur, a2)
        again = sur.poisson_frames(cols[None], [[PHI, U]], out_scale=[scale], apply_filter=True, weighting=True, want_extra=False)
    finally:
        sur.close()
    same = [same_bits(fields[0], want[0][0, ..., 0]), same_bits(fields[1], want[1][0]), same_bits(fields[2], want[2][0])]
    expect = np.array([U, c, U2, scale, 0.0, 2.0, 0.0, 0.0])
    print(f"{which}: (result, change, next) identical to psm_poisson_frames on host-made columns {same}; scalars {scalars} against {expect}")
    assert all(same) and same_bits(scalars, expect)
    assert all(same_bits(x, y) for x, y in zip(want[:3], again[:3]))          # and the frames entry gives its bits behind the step
    # the near-wall flags as psm_set_geometry derives them: interpolate(sdfunct.flatten()) < 0.05 (PM:492-494)
    sdf_mesh = np.zeros(t.n_cells)
    for j in range(3):
        sdf_mesh += t.sdf.reshape(-1)[t.v2[:, j]] * t.w2[:, j]
    p_np, fb = numpy_tail(t, fields[2], a2, sdf_mesh < 0.05)
    print(f"{which}: p identical to the NumPy tail {same_bits(p, p_np)}, fallback share {fb.mean():.3f}, max|dp| {np.abs(p - a2[:, 4]).max():.3e}")
    assert 0.0 < fb.mean() < 1.0 and same_bits(p, p_np)


def test_state(case):
    """(push 0; push 3; 5; 6) ends bit for bit where a fresh handle doing (push 3; push 5; 6) ends; priming steps return cells[:,4]
    bit for bit and leave `steps` at 0; reset gives (0, 0); without the weighting one push suffices."""
    a = run(case, 1, 1)
    b = handle(case.model, case.tabs, 1, 1)
    try:
        b.poisson_solve_push(case.arrays[3])
        b.poisson_solve_push(case.arrays[5])
        assert same_bits(step(b, case.arrays[6]), a[6])
        assert a["state"] == (2, 2) and b.poisson_solve_state == (2, 1)
        b.poisson_solve_reset()
        assert b.poisson_solve_state == (0, 0)
        for k, held in ((0, 1), (3, 2)):                    # two priming steps through the step entry itself
            assert same_bits(step(b, case.arrays[k]), np.ascontiguousarray(case.arrays[k][:, 4]))
            assert b.poisson_solve_state == (held, 0)
        assert same_bits(step(b, case.arrays[5]), a[5]) and b.poisson_solve_state == (2, 1)
    finally:
        b.close()
    w0 = handle(case.model, case.tabs, 0, 0)
    try:
        w0.poisson_solve_push(case.arrays[3])
        assert same_bits(step(w0, case.arrays[5]), run(case, 0, 0)[5]) and w0.poisson_solve_state == (2, 1)
    finally:
        w0.close()


def test_skipped_step(case):
    """A frame with all velocities zero gives p_out == cells[:,4] and skip == 1; the step after it is a normal step, equal to the
    reference built from the same three frames (measured on an MI355X: 4.3e-9 of the scale, which dU = U makes 3.1)."""
    still = case.arrays["still"]
    sur = handle(case.model, case.tabs, 1, 1)
    try:
        sur.poisson_solve_push(case.arrays[0])
        sur.poisson_solve_push(case.arrays[3])
        p, _, scalars = device_step(sur, still)
        print(f"skipped step: scalars {scalars}")
        assert same_bits(p, np.ascontiguousarray(still[:, 4]))
        assert scalars[4] == 1.0 and scalars[0] == 1.0 and scalars[2] == 1.0 and scalars[3] == 0.0 and scalars[5] == 2.0
        assert sur.poisson_solve_state == (2, 1)
        p6 = step(sur, case.arrays[6])
    finally:
        sur.close()
    check_against_reference(p6, case.arrays[6], case.ref(3, "still", 6, 1, 1), "the step behind a skipped step")


def expect_error(code, words, call):
    with pytest.raises(_lib.PsmError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_errors(case):
    t, m = case.tabs, case.model
    bind = lambda s: s.bind_poisson_solve(PHI, MAXS5[4], 1, 1)
    sur = handle(m, t, bind=False)
    try:
        expect_error(-2, ["psm_bind_features has not"], lambda: bind(sur))
        sur.bind_features(t.sdf, K, MAXS5[:4])
        expect_error(-2, ["psm_bind_poststeps has not"], lambda: bind(sur))
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        expect_error(-2, ["psm_bind_frames has not"], lambda: bind(sur))
        sur.bind_frames(1, 4)
        expect_error(-2, ["psm_bind_frames has not", "6 columns"], lambda: bind(sur))
        sur.bind_frames(1, 6)
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.solve_poisson(case.arrays[0]))
        for phi, mp in ((0.0, 0.005), (np.nan, 0.005), (PHI, 0.0), (PHI, np.inf)):
            expect_error(-1, ["finite and non-zero"], lambda: sur.bind_poisson_solve(phi, mp, 1, 1))
        bind(sur)
        assert sur.poisson_solve_state == (0, 0)
        expect_error(-1, ["cell count"], lambda: sur.solve_poisson(case.arrays[0][:-1]))
        expect_error(-1, ["cell count"], lambda: sur.poisson_solve_push(case.arrays[0][:-1]))
        sur.poisson_solve_push(case.arrays[0])
        assert sur.poisson_solve_state == (1, 0)
        sur.bind_features(t.sdf, K, MAXS5[:4])              # re-binding the features drops the step binding
        assert sur.poisson_solve_state == (0, 0)
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.solve_poisson(case.arrays[0]))
        bind(sur)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)               # so do the post-steps,
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.poisson_solve_push(case.arrays[0]))
        bind(sur)
        sur.bind_frames(1, 6)                               # the frames
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.poisson_solve_reset())
        bind(sur)
        sur.unbind_poisson_solve()                          # and its own unbind
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.solve_poisson(case.arrays[0]))
        # no grid -> mesh tables
        no_g2m = Tabs(t.ny, t.nx, t.n_cells, t.v1, t.w1, t.idx, t.sdf, None, None)
        set_geometry(sur, no_g2m)
        sur.bind_features(t.sdf, K, MAXS5[:4]); sur.bind_poststeps(S_FIELD, S_WEIGHT); sur.bind_frames(1, 6)
        expect_error(-1, ["grid->mesh tables"], lambda: bind(sur))
    finally:
        sur.close()
    three = synthetic.make_model("deltas", p_in=32, p_out=32)    # c_in == 3
    sur = GridSurrogate(three, t.ny, t.nx, 1)
    try:
        set_geometry(sur, t)
        expect_error(-5, ["c_in == 4"], lambda: bind(sur))
        # a case set (psm_set_geometry_cases takes the three-channel model only): refused as such, before the model's shape is looked at
        ptr = lambda a: (C.c_void_p * 1)(a.ctypes.data)
        mx = np.asarray(MAXS5[1:], np.float64)
        rc = sur.lib.psm_set_geometry_cases(sur.h, 1, (C.c_int64 * 1)(t.n_cells), t.ny, t.nx, ptr(t.v1), ptr(t.w1), ptr(t.idx), ptr(t.sdf), ptr(t.v2),
                                            ptr(t.w2), mx.ctypes.data_as(_dp), 1, 1, 0.05)
        assert rc == 0, _lib.last_error(sur.h)
        expect_error(-2, ["case set"], lambda: bind(sur))
    finally:
        sur.close()


def test_independence(case):
    """psm_poisson_frames on the handle of a Poisson solver step gives, before and after a step, the bits it gives on a handle that
    never had the binding; psm_solve_delta (a c_in == 3 entry: no handle can run both) gives its bits before and after the refused
    bind on its own handle."""
    t = case.tabs
    cols, U, _ = columns(case.arrays[0], case.arrays[3], case.arrays[5])
    cols = np.nan_to_num(cols)
    frames = lambda s: s.poisson_frames(cols[None], [[PHI, U]], out_scale=[MAXS5[4] * U * U], apply_filter=True, weighting=True, want_extra=False)[:3]
    plain = handle(case.model, t, bind=False)
    try:
        plain.bind_features(t.sdf, K, MAXS5[:4]); plain.bind_poststeps(S_FIELD, S_WEIGHT); plain.bind_frames(1, 6)
        want = frames(plain)
    finally:
        plain.close()
    sur = handle(case.model, t, 1, 1)
    try:
        before = frames(sur)
        sur.poisson_solve_push(case.arrays[0]); sur.poisson_solve_push(case.arrays[3])
        p5 = step(sur, case.arrays[5])
        after = frames(sur)
        p6 = step(sur, case.arrays[6])                      # and the step is not disturbed by the frames call between
    finally:
        sur.close()
    same = [all(same_bits(x, y) for x, y in zip(got, want)) for got in (before, after)]
    print(f"psm_poisson_frames identical to a handle without the binding: before {same[0]}, after {same[1]}")
    assert all(same) and same_bits(p5, run(case, 1, 1)[5]) and same_bits(p6, run(case, 1, 1)[6])
    three = synthetic.make_model("deltas", p_in=32, p_out=32)
    sur = GridSurrogate(three, t.ny, t.nx, 1)
    try:
        set_geometry(sur, t, (0.01, 0.01, 0.35, 0.5))
        delta = lambda: [sur.lib.psm_delta_reset(sur.h), sur.lib.psm_delta_prime(sur.h, case.arrays[0].ctypes.data_as(_dp), t.n_cells), delta_step(sur, case.arrays[3])][2]
        first = delta()
        expect_error(-5, ["c_in == 4"], lambda: sur.bind_poisson_solve(PHI, MAXS5[4], 1, 1))
        assert same_bits(first, delta())
    finally:
        sur.close()


def delta_step(sur, array):
    p = np.full(len(array), -7.0)
    rc = sur.lib.psm_solve_delta(sur.h, array.ctypes.data_as(_dp), len(array), 0, p.ctypes.data_as(_dp))
    assert rc == 0, _lib.last_error(sur.h)
    return p


def test_solver_module(case):
    """SolverModule(step="poisson") over the four arrays equals the C entries on its own tables bit for bit."""
    sm = SolverModule(case.model, MAXS5, step="poisson", phi=PHI, k=K, weighting=True, apply_filter=True, sigma_field=S_FIELD, sigma_weight=S_WEIGHT)
    assert sm.init_func(case.arrays[0], case.top, case.obst) == 0
    try:
        assert sm.state == (1, 0)
        got = [sm.py_func(case.arrays[k]) for k in (3, 5, 6)]
        assert sm.state == (2, 2)
        g = sm.tables
        t = Tabs(g.ny, g.nx, len(case.arrays[0]), g.vtx_m2g, g.wts_m2g, g.indices, g.sdfunct, g.vtx_g2m, g.wts_g2m)
        sm.reset_state()
        assert sm.state == (0, 0)
        sm.prime(case.arrays[3]); sm.prime(case.arrays[5])
        again = sm.py_func(case.arrays[6])
    finally:
        sm._sur.close()
    sur = handle(case.model, t, 1, 1)
    try:
        sur.poisson_solve_push(case.arrays[0])
        want = [step(sur, case.arrays[k]) for k in (3, 5, 6)]
    finally:
        sur.close()
    same = [same_bits(a, b) for a, b in zip(got, want)]
    print(f"SolverModule(step='poisson') identical to the C entries {same}; the first call is a priming step: {same_bits(got[0], np.ascontiguousarray(case.arrays[3][:, 4]))}")
    assert all(same) and same_bits(got[0], np.ascontiguousarray(case.arrays[3][:, 4])) and same_bits(again, want[2])
    assert np.abs(got[2] - case.arrays[6][:, 4]).max() > 0
