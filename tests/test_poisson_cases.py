"""The Poisson-model step at the solver boundary for a case set (psm_bind_poisson_solve_cases, psm_solve_cases_poisson*): K meshes on
one handle, cells [sum n_i,5] -> p [sum n_i], one two-frame state for the set.  Every check is on dp = p_out - cells[:,4], as in
test_poisson_solve.py, whose model, constants, reference functions and tolerance are imported unchanged.

Channel set: the first three meshes of test_mesh_cases.OBSTACLES on their common 138 x 300 grid, 16 021 / 16 165 / 15 838 cells
(62 * 256 + 149, 63 * 256 + 37, 61 * 256 + 222: the tail's launch width and the last part of the partial launch differ from case to
case), tables from ``orc.init_geometry`` once per module, frames ``channel_mesh(step = the obstacle's own + s)`` for s in {0, 3, 5, 6}.
The float64 reference of a step is composed per case exactly as test_poisson_solve.Case.ref composes it, once, and never modified.

Hand set: three meshes of 257 / 1025 / 255 cells on 130 x 131 by the recipe of test_poisson_solve.hand_tabs with a seed per case: one
thread in a second tail workgroup, one cell in a second 1024-cell part (so the two short cases own no cell of part 1), one cell short
of a workgroup; no mesh -> grid weight is negative, a fifth of the grid -> mesh rows carry one, the solid patch differs per case.
Every GPU test prints what it measured before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

from hipmem import DeviceArray
from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverEnsemble, _lib, geometry, synthetic
from test_mesh_cases import OBSTACLES
from test_oracle_golden import oracle_model
from test_poisson_solve import MAXS5, PHI, Tabs, check_against_reference, columns, expect_error, g2m, numpy_tail, plane, same_bits, set_geometry
from test_poisson_solve import handle as single_handle
from test_poisson_solve import step as single_step
from test_poisson_step_device import K, S_FIELD, S_WEIGHT, SOLVE_TOL, chain, model4

pytestmark = pytest.mark.gpu

FRAMES = (0, 3, 5, 6)
CELLS = (16021, 16165, 15838)
HAND_CELLS = (257, 1025, 255)
HAND_SOLID = ((slice(40, 60), slice(30, 50)), (slice(70, 95), slice(60, 80)), (slice(10, 30), slice(90, 120)))
PARITY = ((1, 1, (0, 1, 2)), (0, 0, (0, 1, 2)), (1, 0, (2, 0, 1)))     # (weighting, apply_filter, order of the cases in the set)
_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------------------------- inputs and references
class ChannelSet:
    """Inputs and float64 references of the three channel cases, built once per module and left unchanged."""

    def __init__(self):
        self.model = model4()
        self.arrays, self.bounds, self.tabs = [], [], []
        for kw in OBSTACLES[:3]:
            frames = {s: np.ascontiguousarray(synthetic.channel_mesh(**dict(kw, step=kw.get("step", 0) + s))[0]) for s in FRAMES}
            still = frames[5].copy()
            still[:, 0:2] = 0.0
            frames["still"] = still                              # a frame with all velocities zero: a skipped step of that case
            _, top, obst = synthetic.channel_mesh(**kw)
            geo = orc.init_geometry(frames[0], top, obst)
            self.arrays.append(frames)
            self.bounds.append((top, obst))
            self.tabs.append(Tabs(geo.ny, geo.nx, len(frames[0]), geo.vert_m2g, geo.wts_m2g, geo.indices, geo.sdfunct, geo.vert_g2m, geo.wts_g2m))
        self._solve, self._ref = {}, {}

    def solve(self, k, f0, f1, f2):
        key = (k, f0, f1, f2)
        if key not in self._solve:
            t, a = self.tabs[k], self.arrays[k]
            cols, U, _ = columns(a[f0], a[f1], a[f2])
            g = [plane(t, cols[:, q]) for q in range(6)]
            for q in (4, 5):
                g[q][np.isnan(g[q])] = 0.0
            grid, _ = orc.poisson_features(g[0], g[1], g[2], g[3], t.sdf, PHI, U, K, MAXS5[:4])
            om = oracle_model(self.model)
            om.out_scale = MAXS5[4] * U ** 2
            self._solve[key] = (orc.solve_grid(grid, om).fields[..., 0], g[4], g[5])
        return self._solve[key]

    def ref(self, k, f0, f1, f2, weighting, af):
        """-> (dp_ref [n_k] with NaN on the fallback cells, the bound's scale), as test_poisson_solve.Case.ref."""
        key = (k, f0, f1, f2, weighting, af)
        if key not in self._ref:
            field, w, prev = self.solve(k, f0, f1, f2)
            res, _, nxt = chain(field, w, prev, af)
            f = nxt if weighting else res
            self._ref[key] = (g2m(self.tabs[k], f, self.arrays[k][f2]), float(max(np.abs(f).max(), np.abs(field).max())))
        return self._ref[key]

    def cells(self, order, s, still=()):
        return pack([self.arrays[k]["still" if k in still else s] for k in order])


@pytest.fixture(scope="module")
def cs():
    return ChannelSet()


def hand_case(seed, n, solid):
    """test_poisson_solve.hand_tabs's recipe for one case of the hand set: n cells, its own seed and solid patch, three frames."""
    ny, nx = 130, 131
    ng = ny * nx
    rng = np.random.default_rng(seed)
    v1 = rng.integers(0, n, (ng, 3)).astype(np.int32)
    w = rng.random((ng, 2)) * 0.5
    w1 = np.c_[w, 1.0 - w.sum(axis=1)]
    pix = np.arange(ng)
    moved = rng.random(ng) < 0.15
    pix[moved] = rng.integers(0, ng, int(moved.sum()))
    idx = np.c_[pix // nx, pix % nx].astype(np.int32)
    sdf = 0.02 + 0.3 * rng.random((ny, nx))
    sdf[solid] = 0.0
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
    assert (writers == 0).any() and (writers > 1).any() and not (w1 < 0).any() and 0.1 < neg.mean() < 0.3
    return Tabs(ny, nx, n, v1, w1, idx, sdf, v2, w2), frames


class HandSet:
    def __init__(self):
        self.model = model4()
        made = [hand_case(4100 + 7 * k, n, HAND_SOLID[k]) for k, n in enumerate(HAND_CELLS)]
        self.tabs, self.frames = [m[0] for m in made], [m[1] for m in made]

    def cells(self, s):
        return pack([f[s] for f in self.frames])


@pytest.fixture(scope="module")
def hs():
    return HandSet()


# ------------------------------------------------------------------------------------------------------- handles and calls
def pack(arrays):
    return np.ascontiguousarray(np.concatenate(arrays), np.float64)


def split(p, counts):
    off = np.concatenate([[0], np.cumsum(counts)])
    return [np.ascontiguousarray(p[off[i]:off[i + 1]]) for i in range(len(counts))]


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def set_cases(sur, tabs, maxs4=MAXS5[1:]):
    """psm_set_geometry_cases with the deltas model's two flags, as the single mesh of test_poisson_solve.set_geometry -> status."""
    cols = [[getattr(t, f) for t in tabs] for f in ("v1", "w1", "idx", "sdf", "v2", "w2")]
    mx = np.asarray(maxs4, np.float64)
    return sur.lib.psm_set_geometry_cases(sur.h, len(tabs), (C.c_int64 * len(tabs))(*[t.n_cells for t in tabs]), tabs[0].ny, tabs[0].nx,
                                          *[_ptrs(c) for c in cols], mx.ctypes.data_as(_dp), 1, 1, 0.05)


def bind_under(sur, tabs):
    sur.bind_features(np.stack([t.sdf for t in tabs]), K, MAXS5[:4])
    sur.bind_poststeps(S_FIELD, S_WEIGHT)


def handle(model, tabs, weighting=1, af=1, max_cases=None, bind=True):
    sur = GridSurrogate(model, tabs[0].ny, tabs[0].nx, max_cases or len(tabs))
    rc = set_cases(sur, tabs)
    assert rc == 0, _lib.last_error(sur.h)
    if bind:
        bind_under(sur, tabs)
        sur.bind_poisson_solve_cases(PHI, MAXS5[4], weighting, af)
    return sur


def step(sur, cells):
    p = np.full(len(cells), -7.0)
    rc = sur.lib.psm_solve_cases_poisson(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp))
    assert rc == 0, _lib.last_error(sur.h)
    return p


def device_step(sur, cells, nc, buffers=True):
    """psm_solve_cases_poisson_device on buffers of its own -> (p [sum n_i], fields [3][K][ny][nx] float32, scalars [K][8]); without
    ``buffers`` d_fields and d_scalars are NULL and come back as None."""
    d_cells, d_p = DeviceArray(cells), DeviceArray(np.full(len(cells), -7.0))
    d_f = DeviceArray(np.full((3, nc, sur.ny, sur.nx), -7.0, np.float32)) if buffers else None
    d_s = DeviceArray(np.full((nc, 8), -7.0)) if buffers else None
    try:
        sur.solve_cases_poisson_device(d_cells.ptr, d_p.ptr, d_f.ptr if buffers else 0, d_s.ptr if buffers else 0)
        sur.synchronize()                                    # the entry is asynchronous on the handle's stream
        return d_p.numpy(), d_f.numpy() if buffers else None, d_s.numpy() if buffers else None
    finally:
        for d in (d_cells, d_p, d_f, d_s):
            if d is not None:
                d.free()


@functools.lru_cache(maxsize=None)
def _run_cached(weighting, af, order):
    return {}


def run(cs, weighting, af, order):
    """push 0, push 3, steps 5 and 6 of the set in `order` through the host entry, once per configuration
    -> {5: [p per position], 6: [...], "state": (frames, steps)}."""
    out = _run_cached(weighting, af, order)
    if not out:
        sur = handle(cs.model, [cs.tabs[k] for k in order], weighting, af)
        counts = [CELLS[k] for k in order]
        try:
            sur.poisson_solve_push_cases(cs.cells(order, 0))
            sur.poisson_solve_push_cases(cs.cells(order, 3))
            out[5], out[6] = split(step(sur, cs.cells(order, 5)), counts), split(step(sur, cs.cells(order, 6)), counts)
            out["state"] = sur.poisson_solve_state
        finally:
            sur.close()
    return out


# ------------------------------------------------------------------------------------------------------- the tests
def test_the_sets_are_the_ones_described(cs, hs):
    assert tuple(t.n_cells for t in cs.tabs) == CELLS and all((t.ny, t.nx) == (138, 300) for t in cs.tabs)
    assert [n % 256 for n in CELLS] == [149, 37, 222] and [n // 256 for n in CELLS] == [62, 63, 61]
    assert tuple(t.n_cells for t in hs.tabs) == HAND_CELLS and all((t.ny, t.nx) == (130, 131) for t in hs.tabs)
    assert all(not (t.w1 < 0).any() and 0.1 < (t.w2 < 0).any(axis=1).mean() < 0.3 for t in hs.tabs)
    assert len({int((t.sdf == 0).sum()) for t in hs.tabs}) == 3
    assert hasattr(_lib.load(), "psm_solve_cases_poisson")


@pytest.mark.parametrize("weighting,af,order", PARITY)
def test_oracle_parity_per_case(cs, weighting, af, order):
    """Push 0, push 3, then steps 5 and 6 of the three cases in `order`, each case against its own composed float64 reference:
    fallback cells equal cells[:,4] bit for bit (their share lies in (0, 0.5); on the reference tables 0.173 / 0.166 / 0.180),
    elsewhere |dp - dp_ref| <= 2e-4 * max(max|gathered field_ref|, max|solve field_ref|), the bound of test_poisson_solve.py, where
    the single mesh measured 1.4e-7 to 5.2e-7.  The state ends at (2, 2).
    Measured on an MI355X, max|dp - dp_ref| / scale over the three cases and both steps: 9.1e-8 .. 2.0e-7 (weighting, filter),
    3.4e-7 .. 5.2e-7 (neither), 9.3e-8 .. 2.3e-7 (weighting, no filter, order (2, 0, 1))."""
    got = run(cs, weighting, af, order)
    for f0, f1, f2 in ((0, 3, 5), (3, 5, 6)):
        for i, k in enumerate(order):
            check_against_reference(got[f2][i], cs.arrays[k][f2], cs.ref(k, f0, f1, f2, weighting, af),
                                    f"weighting={weighting} apply_filter={af} order={order} case {k} step {f1} -> {f2}")
    assert got["state"] == (2, 2)


def hand_planes(hs):
    """Per case of the hand set: the six NumPy columns and scalars of the step on its three frames, the columns turned into planes by
    psm_mesh_to_grid (fill = 1) on a single-mesh handle of that case's tables -> (vel [K][4][ny][nx] float64, weight and dp_prev
    planes [K][ny][nx] float32 with NaN -> 0, [(U, c)])."""
    vel, w32, p32, scal = [], [], [], []
    for t, (a0, a1, a2) in zip(hs.tabs, hs.frames):
        cols, U, c = columns(a0, a1, a2)
        sur = GridSurrogate(hs.model, t.ny, t.nx, 1)
        try:
            set_geometry(sur, t)
            out = np.empty((t.ny, t.nx, 6))
            rc = sur.lib.psm_mesh_to_grid(sur.h, cols.ctypes.data_as(_dp), t.n_cells, 6, 1, out.ctypes.data_as(_dp))
            assert rc == 0, _lib.last_error(sur.h)
        finally:
            sur.close()
        vel.append(np.moveaxis(out[..., :4], -1, 0))
        w32.append(np.nan_to_num(out[..., 4], nan=0.0).astype(np.float32))
        p32.append(np.nan_to_num(out[..., 5], nan=0.0).astype(np.float32))
        scal.append((U, c))
    return np.ascontiguousarray(np.stack(vel)), np.stack(w32), np.stack(p32), scal


def hand_chain(hs):
    """psm_poisson_step with n_cases = 3 on a plain handle whose features are bound with the three SDFs, fed the planes above
    -> ((result, change, next) each [K][ny][nx] float32, [(U, c)])."""
    vel, w32, p32, scal = hand_planes(hs)
    plain = GridSurrogate(hs.model, 130, 131, 3)
    try:
        bind_under(plain, hs.tabs)
        res, chg, nxt = plain.poisson_step(vel, [[PHI, U] for U, _ in scal], out_scale=[MAXS5[4] * (U * U) for U, _ in scal], apply_filter=True,
                                           dU=w32, prev=p32)
    finally:
        plain.close()
    return (np.ascontiguousarray(res[..., 0]), chg, nxt), scal


def near_wall_of(t):
    """The near-wall flags as psm_set_geometry_cases derives them: interpolate(sdfunct.flatten()) < 0.05 (PM:492-494)."""
    sdf_mesh = np.zeros(t.n_cells)
    for j in range(3):
        sdf_mesh += t.sdf.reshape(-1)[t.v2[:, j]] * t.w2[:, j]
    return sdf_mesh < 0.05


def test_bit_identity_with_the_batched_chain(hs):
    """Hand set, (weighting, filter): d_fields of psm_solve_cases_poisson_device equals, bit for bit, psm_poisson_step (n_cases = 3) fed
    planes that psm_mesh_to_grid made of host-made float64 columns, (L, U) and out_scale; d_scalars[k] equals the NumPy values; p of
    each case equals the tail restated in NumPy float64 on the returned `next`."""
    want, scal = hand_chain(hs)
    sur = handle(hs.model, hs.tabs, 1, 1)
    try:
        sur.poisson_solve_push_cases(hs.cells(0))
        sur.poisson_solve_push_cases(hs.cells(1))
        p, fields, scalars = device_step(sur, hs.cells(2), 3)
    finally:
        sur.close()
    same = [same_bits(fields[q], want[q]) for q in range(3)]
    expect = np.array([[U, c, U * U, MAXS5[4] * (U * U), 0.0, 2.0, 0.0, 0.0] for U, c in scal])
    print(f"(result, change, next) identical to psm_poisson_step on host-made columns {same}; scalars {scalars.tolist()} against {expect.tolist()}")
    assert all(same) and same_bits(scalars, expect)
    for k, (t, pk) in enumerate(zip(hs.tabs, split(p, HAND_CELLS))):
        p_np, fb = numpy_tail(t, fields[2][k], hs.frames[k][2], near_wall_of(t))
        print(f"case {k} ({t.n_cells} cells): p identical to the NumPy tail {same_bits(pk, p_np)}, fallback share {fb.mean():.3f}, "
              f"max|dp| {np.abs(pk - hs.frames[k][2][:, 4]).max():.3e}")
        assert 0.0 < fb.mean() < 1.0 and same_bits(pk, p_np)


@pytest.mark.parametrize("weighting,af", ((1, 1), (0, 0)))
def test_one_case_is_the_single_mesh_bit_for_bit(cs, weighting, af):
    """K = 1 in a max_cases = 4 handle against psm_solve_poisson on a single-mesh handle with the same tables: push, push, step,
    step; every p is identical."""
    a, t = cs.arrays[0], cs.tabs[0]
    one = handle(cs.model, [t], weighting, af, max_cases=4)
    try:
        one.poisson_solve_push_cases(a[0])
        one.poisson_solve_push_cases(a[3])
        got = [step(one, a[5]), step(one, a[6])]
        state = one.poisson_solve_state
    finally:
        one.close()
    ref = single_handle(cs.model, t, weighting, af)
    try:
        ref.poisson_solve_push(a[0])
        ref.poisson_solve_push(a[3])
        want = [single_step(ref, a[5]), single_step(ref, a[6])]
    finally:
        ref.close()
    same = [same_bits(x, y) for x, y in zip(got, want)]
    print(f"weighting={weighting} apply_filter={af}: one case of a set identical to psm_solve_poisson {same}, max|dp| {np.abs(got[1] - a[6][:, 4]).max():.3e}")
    assert all(same) and state == (2, 2) and np.abs(got[1] - a[6][:, 4]).max() > 0


def test_a_skipped_case_stays_in_its_case(cs):
    """Order (0, 1, 2), case 1's frame 5 with all velocities zero: case 1 returns cells[:,4] bit for bit with scalars[1][4] == 1; cases
    0 and 2 are bit for bit what the same handle sequence gives with case 1 not still; the step after it is within SOLVE_TOL of the
    reference built from the same three frames (case 1: frames 3, still, 6)."""
    order = (0, 1, 2)
    normal = run(cs, 1, 1, order)
    sur = handle(cs.model, cs.tabs, 1, 1)
    try:
        sur.poisson_solve_push_cases(cs.cells(order, 0))
        sur.poisson_solve_push_cases(cs.cells(order, 3))
        p, _, scalars = device_step(sur, cs.cells(order, 5, still=(1,)), 3)
        state = sur.poisson_solve_state
        p6 = split(step(sur, cs.cells(order, 6)), CELLS)
    finally:
        sur.close()
    p5 = split(p, CELLS)
    still = cs.arrays[1]["still"]
    print(f"skipped case: scalars {scalars.tolist()}")
    print(f"case 1 returns cells[:,4]: {same_bits(p5[1], np.ascontiguousarray(still[:, 4]))}; cases 0 and 2 as without the skip: "
          f"{[same_bits(p5[k], normal[5][k]) for k in (0, 2)]}; their next step: {[same_bits(p6[k], normal[6][k]) for k in (0, 2)]}")
    assert same_bits(p5[1], np.ascontiguousarray(still[:, 4]))
    assert scalars[1][4] == 1.0 and scalars[1][0] == 1.0 and scalars[1][2] == 1.0 and scalars[1][3] == 0.0 and scalars[1][5] == 2.0
    assert scalars[0][4] == 0.0 and scalars[2][4] == 0.0 and state == (2, 1)
    assert all(same_bits(p5[k], normal[5][k]) and same_bits(p6[k], normal[6][k]) for k in (0, 2))
    assert np.abs(p5[0] - cs.arrays[0][5][:, 4]).max() > 0
    check_against_reference(p6[1], cs.arrays[1][6], cs.ref(1, 3, "still", 6, 1, 1), "case 1, the step behind its skipped step")
    for k in (0, 2):
        check_against_reference(p6[k], cs.arrays[k][6], cs.ref(k, 3, 5, 6, 1, 1), f"case {k}, the step behind case 1's skipped step")


def test_state(cs):
    """(push 0; push 3; 5; 6) ends bit for bit where a fresh handle doing (push 3; push 5; 6) ends; priming steps through the step
    entry return cells[:,4] bit for bit and leave `steps` at 0; reset gives (0, 0); without the weighting one push suffices."""
    order = (0, 1, 2)
    a = run(cs, 1, 1, order)
    b = handle(cs.model, cs.tabs, 1, 1)
    try:
        b.poisson_solve_push_cases(cs.cells(order, 3))
        b.poisson_solve_push_cases(cs.cells(order, 5))
        last = split(step(b, cs.cells(order, 6)), CELLS)
        print(f"(push 3; push 5; 6) identical to (push 0; push 3; 5; 6): {[same_bits(x, y) for x, y in zip(last, a[6])]}, state {b.poisson_solve_state}")
        assert all(same_bits(x, y) for x, y in zip(last, a[6]))
        assert a["state"] == (2, 2) and b.poisson_solve_state == (2, 1)
        b.poisson_solve_reset()
        assert b.poisson_solve_state == (0, 0)
        for s, held in ((0, 1), (3, 2)):                    # two priming steps through the step entry itself
            cells = cs.cells(order, s)
            assert same_bits(step(b, cells), np.ascontiguousarray(cells[:, 4]))
            assert b.poisson_solve_state == (held, 0)
        again = split(step(b, cs.cells(order, 5)), CELLS)
        assert all(same_bits(x, y) for x, y in zip(again, a[5])) and b.poisson_solve_state == (2, 1)
    finally:
        b.close()
    w0 = handle(cs.model, cs.tabs, 0, 0)
    try:
        w0.poisson_solve_push_cases(cs.cells(order, 3))
        got = split(step(w0, cs.cells(order, 5)), CELLS)
        assert all(same_bits(x, y) for x, y in zip(got, run(cs, 0, 0, order)[5])) and w0.poisson_solve_state == (2, 1)
    finally:
        w0.close()


def test_device_entry_equals_host_entry(hs):
    """Hand set: the device entry with d_fields / d_scalars NULL and non-NULL gives the host entry's p bit for bit, step after step;
    a psm_poisson_step call on the same handle between two steps changes neither the steps nor its own result."""
    seq = (2, 0)                                            # two steps behind push 0, push 1: frames 2 and 0 again
    runs = {}
    for how in ("host", "device", "device_null", "host_with_a_chain_call_between"):
        sur = handle(hs.model, hs.tabs, 1, 1)
        try:
            sur.poisson_solve_push_cases(hs.cells(0))
            sur.poisson_solve_push_cases(hs.cells(1))
            out = []
            for i, s in enumerate(seq):
                if how.startswith("host"):
                    out.append((step(sur, hs.cells(s)), None, None))
                else:
                    out.append(device_step(sur, hs.cells(s), 3, buffers=how == "device"))
                if i == 0 and how.endswith("between"):
                    vel, w32, p32, scal = hand_planes(hs)
                    between = sur.poisson_step(vel, [[PHI, U] for U, _ in scal], out_scale=[MAXS5[4] * (U * U) for U, _ in scal],
                                               apply_filter=True, dU=w32, prev=p32)
            runs[how] = out
            assert sur.poisson_solve_state == (2, 2)
        finally:
            sur.close()
    same = {how: [same_bits(r[0], h[0]) for r, h in zip(runs[how], runs["host"])] for how in runs}
    print(f"p identical to the host entry's: {same}")
    assert all(all(v) for v in same.values())
    assert np.abs(runs["host"][0][0] - hs.cells(2)[:, 4]).max() > 0
    want, _ = hand_chain(hs)
    chain_same = [same_bits(np.ascontiguousarray(between[0][..., 0]), want[0]), same_bits(between[1], want[1]), same_bits(between[2], want[2])]
    fields_same = [same_bits(runs["device"][0][1][q], want[q]) for q in range(3)]
    print(f"psm_poisson_step between two steps gives the plain handle's bits {chain_same}; d_fields of the first step equal them too {fields_same}")
    assert all(chain_same) and all(fields_same)


def test_errors(hs, cs):
    """Every refusal of psm_set_geometry_cases under the four-channel model, of the step entries of the three-channel models on such a
    set, of psm_bind_poisson_solve_cases and of the step; each leaves the handle usable.  Re-binding the features or the post-steps,
    or setting a new case set, drops the binding."""
    tabs, m = hs.tabs, hs.model
    bind = lambda s: s.bind_poisson_solve_cases(PHI, MAXS5[4], 1, 1)
    cells = [hs.cells(s) for s in range(3)]
    total = len(cells[0])
    p = np.empty(total)
    raw = lambda s, name, *args: (getattr(s.lib, name)(s.h, *args), _lib.last_error(s.h))
    cp, pp = cells[0].ctypes.data_as(_dp), p.ctypes.data_as(_dp)
    sur = GridSurrogate(m, 130, 131, 3)
    try:
        expect_error(-2, ["psm_set_geometry_cases has not"], lambda: bind(sur))
        set_geometry(sur, tabs[0])
        expect_error(-2, ["psm_bind_poisson_solve"], lambda: bind(sur))       # a single mesh: the message names the other bind
        assert set_cases(sur, tabs) == 0, _lib.last_error(sur.h)
        # the step entries of the three-channel models on this set
        for name, args in (("psm_solve_cases", (cp, pp)), ("psm_solve_cases_begin", (cp, pp)), ("psm_solve_cases_device", (None, None, None)),
                           ("psm_solve_cases_delta", (cp, pp)), ("psm_solve_cases_delta_begin", (cp, pp)),
                           ("psm_solve_cases_delta_device", (None, None, None)), ("psm_delta_prime_cases", (cp,))):
            rc, msg = raw(sur, name, *args)
            assert rc == -5 and "the mesh entry needs c_in == 3 and c_out == 1" in msg, (name, rc, msg)
        expect_error(-2, ["case set"], lambda: sur.bind_poisson_solve(PHI, MAXS5[4], 1, 1))   # the single-mesh bind stays as it is
        expect_error(-2, ["psm_bind_features has not"], lambda: bind(sur))
        sur.bind_features(tabs[0].sdf, K, MAXS5[:4])
        expect_error(-2, ["psm_bind_features", "fewer cases"], lambda: bind(sur))
        sur.bind_features(np.stack([t.sdf for t in tabs]), K, MAXS5[:4])
        expect_error(-2, ["psm_bind_poststeps has not"], lambda: bind(sur))
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        expect_error(-2, ["psm_bind_poisson_solve_cases has not"], lambda: sur.solve_cases_poisson(cells[0]))
        expect_error(-2, ["psm_bind_poisson_solve_cases has not"], lambda: sur.poisson_solve_push_cases(cells[0]))
        for phi, mp in ((0.0, 0.005), (np.nan, 0.005), (PHI, 0.0), (PHI, np.inf)):
            expect_error(-1, ["finite and non-zero"], lambda: sur.bind_poisson_solve_cases(phi, mp, 1, 1))
        bind(sur)                                           # psm_bind_frames is not needed
        assert sur.poisson_solve_state == (0, 0)
        with pytest.raises(ValueError, match="cells of the case set"):
            sur.solve_cases_poisson(cells[0][:-1])
        with pytest.raises(ValueError, match="cells of the case set"):
            sur.poisson_solve_push_cases(cells[0][:-1])
        assert raw(sur, "psm_solve_cases_poisson", None, pp)[0] == -1 and raw(sur, "psm_solve_cases_poisson", cp, None)[0] == -1
        assert raw(sur, "psm_poisson_solve_push_cases", None)[0] == -1
        # the single-mesh entries on this binding name the _cases entries
        for name, args in (("psm_solve_poisson", (cp, total, 0, pp)), ("psm_poisson_solve_push", (cp, total)),
                           ("psm_solve_poisson_device", (None, None, None, None, None))):
            rc, msg = raw(sur, name, *args)
            assert rc == -2 and "_cases" in msg, (name, rc, msg)
        # the device entry: null and misaligned pointers, before anything is enqueued
        d_cells, d_p = DeviceArray(cells[0]), DeviceArray(p)
        try:
            expect_error(-1, ["null buffer"], lambda: sur.solve_cases_poisson_device(0, d_p.ptr))
            expect_error(-1, ["null buffer"], lambda: sur.solve_cases_poisson_device(d_cells.ptr, 0))
            expect_error(-1, ["misaligned"], lambda: sur.solve_cases_poisson_device(d_cells.ptr + 4, d_p.ptr))
            expect_error(-1, ["misaligned"], lambda: sur.solve_cases_poisson_device(d_cells.ptr, d_p.ptr, d_cells.ptr + 2))
            expect_error(-1, ["misaligned"], lambda: sur.solve_cases_poisson_device(d_cells.ptr, d_p.ptr, 0, d_p.ptr + 4))
        finally:
            d_cells.free(); d_p.free()
        assert sur.poisson_solve_state == (0, 0)
        # the handle is usable: the sequence of the other tests gives its bits
        sur.poisson_solve_push_cases(cells[0])
        sur.poisson_solve_push_cases(cells[1])
        first = step(sur, cells[2])
        assert sur.poisson_solve_state == (2, 1) and np.abs(first - cells[2][:, 4]).max() > 0
        # what drops the binding
        sur.bind_features(np.stack([t.sdf for t in tabs]), K, MAXS5[:4])
        assert sur.poisson_solve_state == (0, 0)
        expect_error(-2, ["psm_bind_poisson_solve_cases has not"], lambda: sur.solve_cases_poisson(cells[0]))
        bind(sur)
        sur.bind_poststeps(S_FIELD, S_WEIGHT)
        assert sur.poisson_solve_state == (0, 0)
        expect_error(-2, ["psm_bind_poisson_solve_cases has not"], lambda: sur.poisson_solve_push_cases(cells[0]))
        bind(sur)
        sur.poisson_solve_push_cases(cells[0])
        assert set_cases(sur, tabs) == 0, _lib.last_error(sur.h)              # a new case set (it drops features and post-steps with the plan or keeps them: the step binding goes either way)
        assert sur.poisson_solve_state == (0, 0)
        expect_error(-2, ["has not"], lambda: sur.solve_cases_poisson(cells[0]))
        bind_under(sur, tabs)
        bind(sur)
        sur.unbind_poisson_solve()
        expect_error(-2, ["psm_bind_poisson_solve_cases has not"], lambda: sur.solve_cases_poisson(cells[0]))
        expect_error(-2, ["psm_bind_poisson_solve has not"], lambda: sur.poisson_solve_reset())
        bind(sur)
        sur.poisson_solve_push_cases(cells[0])
        sur.poisson_solve_push_cases(cells[1])
        again = step(sur, cells[2])
        print(f"after every refusal and re-bind the step gives its bits: {same_bits(again, first)}")
        assert same_bits(again, first)
    finally:
        sur.close()
    # the case-set entries on the single-mesh binding name psm_bind_poisson_solve's entries
    one = single_handle(cs.model, cs.tabs[0], 1, 1)
    try:
        a = cs.arrays[0][0]
        q = np.empty(len(a))
        for name, args in (("psm_solve_cases_poisson", (a.ctypes.data_as(_dp), q.ctypes.data_as(_dp))), ("psm_poisson_solve_push_cases", (a.ctypes.data_as(_dp),)),
                           ("psm_solve_cases_poisson_device", (None, None, None, None, None))):
            rc, msg = raw(one, name, *args)
            assert rc == -2 and "psm_bind_poisson_solve" in msg and "single mesh" in msg, (name, rc, msg)
        one.poisson_solve_push(a)
        assert one.poisson_solve_state == (1, 0)
    finally:
        one.close()
    # the models the entries refuse
    three = synthetic.make_model("deltas", p_in=32, p_out=32)                # c_in == 3: the set is accepted, the bind is not
    sur = GridSurrogate(three, 130, 131, 3)
    try:
        assert set_cases(sur, tabs) == 0, _lib.last_error(sur.h)
        expect_error(-5, ["c_in == 4"], lambda: bind(sur))
    finally:
        sur.close()
    four = synthetic.make_model("deltas", p_in=16, p_out=16, c_in=4)         # c_in == 4 with the SDF in channel 2
    assert four.sdf_ch != 3
    sur = GridSurrogate(four, 130, 131, 3)
    try:
        assert set_cases(sur, tabs) == -5 and "sdf_channel == 3" in _lib.last_error(sur.h)
    finally:
        sur.close()


def test_solver_ensemble(cs):
    """SolverEnsemble(step="poisson") over the four frames equals the C entries on its own tables (the library's builder, which
    geometry.build_geometry_native calls too) bit for bit; the first py_func is a priming step; reset_state + two prime + py_func
    reproduces the last step."""
    order = (0, 1, 2)
    ens = SolverEnsemble(cs.model, MAXS5, 3, step="poisson", phi=PHI, k=K, weighting=True, apply_filter=True, sigma_field=S_FIELD, sigma_weight=S_WEIGHT)
    assert ens.init_func([cs.arrays[k][0] for k in order], [cs.bounds[k][0] for k in order], [cs.bounds[k][1] for k in order]) == 0
    try:
        assert ens.state == (1, 0) and ens.cell_off == [0, 16021, 32186, 48024]
        got = [ens.py_func([cs.arrays[k][s] for k in order]) for s in (3, 5, 6)]
        assert ens.state == (2, 2)
        ens.reset_state()
        assert ens.state == (0, 0)
        ens.prime([cs.arrays[k][3] for k in order]); ens.prime([cs.arrays[k][5] for k in order])
        again = ens.py_func([cs.arrays[k][6] for k in order])
        with pytest.raises(RuntimeError, match="begin / end"):
            ens.py_func_begin([cs.arrays[k][6] for k in order])
    finally:
        ens._sur.close()
    tabs = []
    for k in order:
        g = geometry.build_geometry_native(cs.arrays[k][0], *cs.bounds[k])
        tabs.append(Tabs(g.ny, g.nx, CELLS[k], g.vtx_m2g, g.wts_m2g, g.indices, g.sdfunct, g.vtx_g2m, g.wts_g2m))
    sur = handle(cs.model, tabs, 1, 1)
    try:
        sur.poisson_solve_push_cases(cs.cells(order, 0))
        want = [split(step(sur, cs.cells(order, s)), CELLS) for s in (3, 5, 6)]
    finally:
        sur.close()
    same = [[same_bits(np.ascontiguousarray(x), y) for x, y in zip(g, w)] for g, w in zip(got, want)]
    priming = [same_bits(np.ascontiguousarray(x), np.ascontiguousarray(cs.arrays[k][3][:, 4])) for k, x in zip(order, got[0])]
    print(f"SolverEnsemble(step='poisson') identical to the C entries {same}; the first call is a priming step: {priming}")
    assert all(all(s) for s in same) and all(priming)
    assert all(same_bits(np.ascontiguousarray(x), y) for x, y in zip(again, want[2]))
    assert all(np.abs(x - cs.arrays[k][6][:, 4]).max() > 0 for k, x in zip(order, got[2]))
