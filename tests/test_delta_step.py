"""The delta step at the solver boundary (psm_solve_delta*, psm_solve_cases_delta*): [U(t) - U(t-1)], SDF -> p(t) - p(t-1) with
U(t-1) kept on the device.  Every check is on dp = p_out - cells[:,4], never on p: the previous pressure is of the size of p and
would hide any error.

The case: ``synthetic.channel_mesh(step=k)`` -- 16 021 cells, a 138 x 300 grid, 6 blocks of the deltas layout, the same geometry
for every k with fields that change -- behind ``make_model("deltas", p_in=32, p_out=32)`` with maxs = (0.01, 0.01, 0.35, 0.5), so
that the image channels are O(1).  Tables from ``orc.init_geometry``, handed to psm_set_geometry with normalise_sdf = fill_input = 1:
the oracle and the product hold the same tables.  The reference of a step is composed here from functions the oracle pins to the
reference (interpolate_fill, solve_grid, grid_to_mesh), once per (previous, current) pair, and never modified."""
import ctypes as C

import numpy as np
import pytest

from oracle import psm_oracle as orc
from psm_amd import GridSurrogate, SolverEnsemble, SolverModule, _lib, geometry, synthetic
from test_oracle_golden import oracle_model

pytestmark = pytest.mark.gpu

MAXS = (0.01, 0.01, 0.35, 0.5)
BOUND = 2e-4            # of max|dp_ref|: what tests/test_mesh_path.py holds the same launch chain to against the same float64 oracle
BOUND_ROUTES = 2e-5     # of max|dp|: bound route against the general route, as in tests/test_mesh_path.py
OBSTACLES = (dict(), dict(cx=0.55, cy=0.05, R=0.06), dict(cx=0.9, cy=-0.08, R=0.1, step=2))   # the first three of tests/test_mesh_cases.py
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def compose_reference(prev, array, geo, om):
    """-> (dp_ref [N] with NaN on the oracle's fallback cells, U_max): the statements of SM_call.py:389-391, 404, 418-419, 422-423,
    432-443 on the mesh, the oracle's solve, and PM:481-496 applied to dp."""
    U_max = np.max(np.sqrt(np.square(array[:, 0]) + np.square(array[:, 1])))
    grid = np.zeros((geo.ny, geo.nx, 3))
    idx = tuple(geo.indices.T)
    for c in (0, 1):
        grid[:, :, c][idx] = orc.interpolate_fill((array[:, c] - prev[:, c]) / U_max, geo.vert_m2g, geo.wts_m2g) / MAXS[c]
    grid[:, :, 2] = geo.sdfunct / MAXS[2]
    grid[np.isnan(grid)] = 0
    field = orc.solve_grid(grid, om).fields[..., 0]
    marked = array.copy()
    marked[:, 4] = np.nan                                   # grid_to_mesh puts the previous p on its fallback cells: NaN marks them
    return orc.grid_to_mesh(field, marked, geo, MAXS[3], U_max), U_max


class Case:
    """Inputs and references, built once per module and left unchanged."""

    def __init__(self):
        self.model = synthetic.make_model("deltas", p_in=32, p_out=32)
        self.om = oracle_model(self.model)
        self.arrays = {k: np.ascontiguousarray(synthetic.channel_mesh(step=k)[0]) for k in (0, 3, 5, 6)}
        _, self.top, self.obst = synthetic.channel_mesh()
        self.geo = orc.init_geometry(self.arrays[0], self.top, self.obst)
        self._ref = {}

    def ref(self, prev, cur):
        if (prev, cur) not in self._ref:
            self._ref[(prev, cur)] = compose_reference(self.arrays[prev], self.arrays[cur], self.geo, self.om)[0]
        return self._ref[(prev, cur)]


@pytest.fixture(scope="module")
def case():
    return Case()


def set_geometry(sur, geo, n_cells, maxs=MAXS):
    v1, w1 = np.ascontiguousarray(geo.vert_m2g, np.int32), np.ascontiguousarray(geo.wts_m2g, np.float64)
    v2, w2 = np.ascontiguousarray(geo.vert_g2m, np.int32), np.ascontiguousarray(geo.wts_g2m, np.float64)
    idx, sdf, mx = np.ascontiguousarray(geo.indices, np.int32), np.ascontiguousarray(geo.sdfunct, np.float64), np.asarray(maxs, np.float64)
    rc = sur.lib.psm_set_geometry(sur.h, n_cells, geo.ny, geo.nx, v1.ctypes.data_as(_ip), w1.ctypes.data_as(_dp), idx.ctypes.data_as(_ip),
                                  sdf.ctypes.data_as(_dp), v2.ctypes.data_as(_ip), w2.ctypes.data_as(_dp), mx.ctypes.data_as(_dp), 1, 1, 0.05)
    assert rc == 0, _lib.last_error(sur.h)


def handle(case, geo=None, n_cells=None):
    geo = geo or case.geo
    sur = GridSurrogate(case.model, geo.ny, geo.nx, 1)
    set_geometry(sur, geo, n_cells or len(case.arrays[0]))
    return sur


def prime(sur, array):
    assert sur.lib.psm_delta_prime(sur.h, array.ctypes.data_as(_dp), len(array)) == 0, _lib.last_error(sur.h)


def step(sur, array, entry="psm_solve_delta", out=None):
    p = np.full(len(array), -7.0) if out is None else out
    rc = getattr(sur.lib, entry)(sur.h, array.ctypes.data_as(_dp), len(array), 0, p.ctypes.data_as(_dp))
    assert rc == 0, _lib.last_error(sur.h)
    return p


def state(sur):
    primed, steps = C.c_int32(-1), C.c_int64(-1)
    assert sur.lib.psm_delta_state(sur.h, C.byref(primed), C.byref(steps)) == 0
    return primed.value, steps.value


def check_against_reference(p, array, dp_ref, what):
    """Fallback cells hold cells[:,4] bit for bit, the others dp within BOUND; -> the measured max|dp - dp_ref| / max|dp_ref|."""
    fb = np.isnan(dp_ref)
    assert 0.0 < fb.mean() < 0.5, fb.mean()                 # both branches of the last kernel are exercised
    np.testing.assert_array_equal(p[fb], array[fb, 4])
    dp = p[~fb] - array[~fb, 4]
    scale = np.abs(dp_ref[~fb]).max()
    # p = prev + dp rounds at ulp(p): the recovered dp carries up to one ulp of p, far below the bound (p is O(1), 1e-16 against 1e-4 * scale)
    err = np.abs(dp - dp_ref[~fb]).max() / scale
    print(f"{what}: max|dp - dp_ref| / max|dp_ref| = {err:.3e} (max|dp_ref| = {scale:.3e}, fallback share {fb.mean():.3f})")
    assert err <= BOUND, (what, err)
    return err


def test_oracle_parity_over_three_steps(case):
    """Prime with step 0, then arrays 3, 5, 6 in a row, each against its composed oracle.
    Measured on an MI355X: max|dp - dp_ref| / max|dp_ref| = 6.4e-7, 5.3e-7 and 7.5e-7 for the three steps (bound 2e-4)."""
    fb = np.isnan(case.ref(0, 3))
    assert 0.0 < fb.mean() < 0.5
    sur = handle(case)
    try:
        prime(sur, case.arrays[0])
        for prev, cur in ((0, 3), (3, 5), (5, 6)):
            check_against_reference(step(sur, case.arrays[cur]), case.arrays[cur], case.ref(prev, cur), f"step {prev} -> {cur}")
        assert state(sur) == (1, 3)
    finally:
        sur.close()


def test_state_rotation(case):
    """(prime 0; 3; 5; 6) ends, bit for bit, where a fresh handle doing (prime 5; 6) ends: the state is the last step's velocities."""
    a, b = handle(case), handle(case)
    try:
        prime(a, case.arrays[0])
        for k in (3, 5):
            step(a, case.arrays[k])
        last = step(a, case.arrays[6])
        prime(b, case.arrays[5])
        np.testing.assert_array_equal(last, step(b, case.arrays[6]))
        assert state(a) == (1, 3) and state(b) == (1, 1)
    finally:
        a.close(); b.close()


def test_priming_step(case):
    a, b = handle(case), handle(case)
    try:
        assert state(a) == (0, 0)
        p0 = step(a, case.arrays[3])                        # unprimed: the priming step
        np.testing.assert_array_equal(p0, case.arrays[3][:, 4])
        assert state(a) == (1, 0)
        prime(b, case.arrays[3])
        assert state(b) == (1, 0)
        np.testing.assert_array_equal(step(a, case.arrays[5]), step(b, case.arrays[5]))
        assert state(a) == (1, 1)
        assert a.lib.psm_delta_reset(a.h) == 0 and state(a) == (0, 0)
        np.testing.assert_array_equal(step(a, case.arrays[6]), case.arrays[6][:, 4])
        assert state(a) == (1, 0)
        set_geometry(a, case.geo, len(case.arrays[0]))      # a new geometry drops the state
        assert state(a) == (0, 0)
    finally:
        a.close(); b.close()


def test_umax_comes_from_u_not_from_du(case):
    """Two arrays that differ by a small perturbation: max|dU| < 1e-3 U_max, so a normaliser taken from dU is off by three orders
    of magnitude and cannot pass the bound of the parity test."""
    prev = case.arrays[3]
    cur = prev.copy()
    rng = np.random.default_rng(11)
    cur[:, :2] += 5e-4 * np.sin(6 * prev[:, 2:4] + rng.uniform(0, 6.28, 2))
    dp_ref, U_max = compose_reference(prev, cur, case.geo, case.om)
    assert np.sqrt(((cur - prev)[:, :2] ** 2).sum(axis=1)).max() < 1e-3 * U_max
    sur = handle(case)
    try:
        prime(sur, prev)
        check_against_reference(step(sur, cur), cur, dp_ref, "perturbation")
    finally:
        sur.close()


def test_routes(case, monkeypatch):
    """begin / end and registered buffers (DMA form, direct p store) give the bits of the synchronous staging call; the general
    route (PSM_NO_BIND=1) is within 2e-5 max|dp| of the bound one."""
    a3, a5 = case.arrays[3], case.arrays[5]
    sur = handle(case)
    try:
        assert sur.geometry_bound
        prime(sur, a3)
        ref = step(sur, a5)
        # begin / end
        prime(sur, a3)
        out = np.full(len(a5), -7.0)
        step(sur, a5, "psm_solve_delta_begin", out)
        assert sur.lib.psm_solve_delta_end(sur.h) == 0
        np.testing.assert_array_equal(out, ref)
        # registered input only: DMA from the caller's array, p through the staging copy
        cells, pin_out = a5.copy(), np.full(len(a5), -7.0)
        assert sur.lib.psm_pin_buffers(sur.h, cells.ctypes.data_as(_dp), None) == 0, _lib.last_error(sur.h)
        prime(sur, a3)
        np.testing.assert_array_equal(step(sur, cells), ref)
        # both registered: the last kernel stores p straight into the caller's array
        assert sur.lib.psm_pin_buffers(sur.h, cells.ctypes.data_as(_dp), pin_out.ctypes.data_as(_dp)) == 0, _lib.last_error(sur.h)
        prime(sur, a3)
        assert step(sur, cells, out=pin_out) is pin_out
        np.testing.assert_array_equal(pin_out, ref)
        assert sur.lib.psm_unpin_buffers(sur.h) == 0
    finally:
        sur.close()
    monkeypatch.setenv("PSM_NO_BIND", "1")
    gen = handle(case)
    try:
        assert not gen.geometry_bound
        prime(gen, a3)
        got = step(gen, a5)
        dp = ref - a5[:, 4]
        assert np.abs(got - ref).max() <= BOUND_ROUTES * np.abs(dp).max()
    finally:
        gen.close()


def test_large_mesh_takes_the_device_side_partial_maxima():
    """41 170 cells, above the 32 768 switch to device-side partial maxima (a 140 x 300 grid: the finer cloud reaches a
    centimetre further in y): one primed step.  Tables from the library's host builder, which takes a fraction of the time of
    the oracle's at this size; the oracle gets the same tables."""
    model = synthetic.make_model("deltas", p_in=32, p_out=32)
    a0, top, obst = synthetic.channel_mesh(h=0.005)
    a3 = np.ascontiguousarray(synthetic.channel_mesh(h=0.005, step=3)[0])
    a0 = np.ascontiguousarray(a0)
    assert len(a0) == 41170 and len(a0) > 32768
    g = geometry.build_geometry_native(a0, top, obst)
    geo = orc.Geometry(g.ny, g.nx, g.vtx_m2g, g.wts_m2g, g.vtx_g2m, g.wts_g2m, g.indices, g.sdfunct)
    dp_ref, _ = compose_reference(a0, a3, geo, oracle_model(model))
    sur = GridSurrogate(model, geo.ny, geo.nx, 1)
    try:
        set_geometry(sur, geo, len(a0))
        prime(sur, a0)
        check_against_reference(step(sur, a3), a3, dp_ref, "41 170 cells")
    finally:
        sur.close()


def test_errors(case):
    a3, a5 = case.arrays[3], case.arrays[5]
    out = np.empty(len(a5))
    args = lambda a, o=out: (a.ctypes.data_as(_dp), len(a), 0, o.ctypes.data_as(_dp))
    sur, clean = handle(case), handle(case)
    try:
        prime(sur, a3)
        prime(clean, a3)
        # one step in flight per handle across both kinds
        assert sur.lib.psm_solve_begin(sur.h, *args(a5)) == 0
        assert sur.lib.psm_solve_delta_begin(sur.h, *args(a5)) == -2
        assert sur.lib.psm_solve_end(sur.h) == 0
        assert state(sur) == (1, 0)
        other = np.empty(len(a5))
        assert sur.lib.psm_solve_delta_begin(sur.h, *args(a5, other)) == 0
        assert sur.lib.psm_solve_begin(sur.h, *args(a5)) == -2
        assert sur.lib.psm_solve_end(sur.h) == 0            # either end completes the step that is in flight
        np.testing.assert_array_equal(other, step(clean, a5))
        # a wrong cell count is refused and leaves the state as it was
        short = np.ascontiguousarray(a5[:-5])
        assert sur.lib.psm_solve_delta(sur.h, *args(short)) == -1
        assert sur.lib.psm_delta_prime(sur.h, short.ctypes.data_as(_dp), len(short)) == -1
        assert state(sur) == (1, 1)
        np.testing.assert_array_equal(step(sur, case.arrays[6]), step(clean, case.arrays[6]))
        # the case-set entries on a single mesh
        assert sur.lib.psm_solve_cases_delta(sur.h, a5.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == -2
        assert sur.lib.psm_delta_prime_cases(sur.h, a5.ctypes.data_as(_dp)) == -2
    finally:
        sur.close(); clean.close()


# ---- the case set --------------------------------------------------------------------------------------------------------
class CaseSet:
    def __init__(self):
        self.model = synthetic.make_model("deltas", p_in=32, p_out=32)
        self.om = oracle_model(self.model)
        mesh = [synthetic.channel_mesh(**kw) for kw in OBSTACLES]
        self.steps = [[np.ascontiguousarray(synthetic.channel_mesh(**dict(kw, step=kw.get("step", 0) + s))[0]) for kw in OBSTACLES] for s in (0, 3, 5)]
        self.tabs = [geometry.build_geometry_native(a, t, o) for a, t, o in mesh]
        self.geo = [orc.Geometry(g.ny, g.nx, g.vtx_m2g, g.wts_m2g, g.vtx_g2m, g.wts_g2m, g.indices, g.sdfunct) for g in self.tabs]
        self.n = [len(m[0]) for m in mesh]
        self._ref = {}

    def ref(self, k, s):
        """dp_ref of case k's step s - 1 -> s."""
        if (k, s) not in self._ref:
            self._ref[(k, s)] = compose_reference(self.steps[s - 1][k], self.steps[s][k], self.geo[k], self.om)[0]
        return self._ref[(k, s)]


@pytest.fixture(scope="module")
def cset():
    return CaseSet()


def case_handle(cs, order, max_cases=3):
    sur = GridSurrogate(cs.model, cs.tabs[0].ny, cs.tabs[0].nx, max_cases)
    tabs = [cs.tabs[k] for k in order]
    cols = [[np.ascontiguousarray(getattr(g, f), dt) for g in tabs]
            for f, dt in (("vtx_m2g", np.int32), ("wts_m2g", np.float64), ("indices", np.int32), ("sdfunct", np.float64),
                          ("vtx_g2m", np.int32), ("wts_g2m", np.float64))]
    ptrs = [(C.c_void_p * len(tabs))(*[a.ctypes.data for a in c]) for c in cols]
    mx = np.asarray(MAXS, np.float64)
    rc = sur.lib.psm_set_geometry_cases(sur.h, len(tabs), (C.c_int64 * len(tabs))(*[cs.n[k] for k in order]), tabs[0].ny, tabs[0].nx,
                                        *ptrs, mx.ctypes.data_as(_dp), 1, 1, 0.05)
    assert rc == 0, _lib.last_error(sur.h)
    return sur


def pack(cs, order, s):
    return np.ascontiguousarray(np.concatenate([cs.steps[s][k] for k in order]))


def step_cases(sur, cells, entry="psm_solve_cases_delta"):
    p = np.full(len(cells), -7.0)
    assert getattr(sur.lib, entry)(sur.h, cells.ctypes.data_as(_dp), p.ctypes.data_as(_dp)) == 0, _lib.last_error(sur.h)
    return p


def split(cs, p, order):
    off = np.concatenate([[0], np.cumsum([cs.n[k] for k in order])])
    return [p[off[i]:off[i + 1]] for i in range(len(order))]


def test_case_set_against_the_oracle(cset):
    order = (0, 1, 2)
    sur = case_handle(cset, order)
    try:
        c0 = pack(cset, order, 0)
        assert sur.lib.psm_delta_prime_cases(sur.h, c0.ctypes.data_as(_dp)) == 0, _lib.last_error(sur.h)
        for s in (1, 2):
            for k, p in zip(order, split(cset, step_cases(sur, pack(cset, order, s)), order)):
                check_against_reference(p, cset.steps[s][k], cset.ref(k, s), f"case {k} step {s}")
        assert state(sur) == (1, 2)
        # the single-mesh entries on a case set
        a = cset.steps[0][0]
        out = np.empty(len(a))
        assert sur.lib.psm_solve_delta(sur.h, a.ctypes.data_as(_dp), len(a), 0, out.ctypes.data_as(_dp)) == -2
        assert sur.lib.psm_delta_prime(sur.h, a.ctypes.data_as(_dp), len(a)) == -2
    finally:
        sur.close()


def test_one_case_is_psm_solve_delta_bit_for_bit(cset):
    one, single = case_handle(cset, (1,)), GridSurrogate(cset.model, cset.tabs[1].ny, cset.tabs[1].nx, 1)
    try:
        set_geometry(single, cset.geo[1], cset.n[1])
        a0, a1 = cset.steps[0][1], cset.steps[1][1]
        np.testing.assert_array_equal(step_cases(one, a0), a0[:, 4])          # the priming step of the case entries
        assert state(one) == (1, 0)
        prime(single, a0)
        np.testing.assert_array_equal(step_cases(one, a1), step(single, a1))
    finally:
        one.close(); single.close()


def test_cases_are_isolated_and_the_entries_agree(cset):
    """A case's result does not change when another slot's cells change; begin / end and the device entry give the host call's bits."""
    order = (0, 1, 2)
    sur = case_handle(cset, order)
    try:
        c0, c1 = pack(cset, order, 0), pack(cset, order, 1)
        prime_cases = lambda: sur.lib.psm_delta_prime_cases(sur.h, c0.ctypes.data_as(_dp))
        assert prime_cases() == 0
        ref = step_cases(sur, c1)
        # other cells in slot 1 (state and current): slots 0 and 2 keep their bits
        d0, d1 = c0.copy(), c1.copy()
        lo, hi = cset.n[0], cset.n[0] + cset.n[1]
        d0[lo:hi, :2] *= 1.1
        d1[lo:hi, :2] = cset.steps[2][1][:, :2]
        assert sur.lib.psm_delta_prime_cases(sur.h, d0.ctypes.data_as(_dp)) == 0
        got = step_cases(sur, d1)
        np.testing.assert_array_equal(got[:lo], ref[:lo])
        np.testing.assert_array_equal(got[hi:], ref[hi:])
        assert not np.array_equal(got[lo:hi], ref[lo:hi])
        # begin / end
        assert prime_cases() == 0
        out = np.full(len(c1), -7.0)
        assert sur.lib.psm_solve_cases_delta_begin(sur.h, c1.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == 0
        assert sur.lib.psm_solve_cases_begin(sur.h, c1.ctypes.data_as(_dp), out.ctypes.data_as(_dp)) == -2
        assert sur.lib.psm_solve_cases_delta_end(sur.h) == 0
        np.testing.assert_array_equal(out, ref)
        # device buffers
        assert prime_cases() == 0
        d_cells, d_p = C.c_void_p(), C.c_void_p()
        assert sur.lib.psm_debug_malloc(C.byref(d_cells), c1.nbytes) == 0 and sur.lib.psm_debug_malloc(C.byref(d_p), ref.nbytes) == 0
        try:
            assert sur.lib.psm_debug_copy_to_device(d_cells, c1.ctypes.data, c1.nbytes) == 0
            assert sur.lib.psm_solve_cases_delta_device(sur.h, d_cells, d_p, None) == 0, _lib.last_error(sur.h)
            assert sur.lib.psm_synchronize(sur.h) == 0
            dev = np.full(len(c1), -7.0)
            assert sur.lib.psm_debug_copy_to_host(dev.ctypes.data, d_p, dev.nbytes) == 0
        finally:
            sur.lib.psm_debug_free(d_cells); sur.lib.psm_debug_free(d_p)
        np.testing.assert_array_equal(dev, ref)
    finally:
        sur.close()


def test_psm_solve_on_the_same_handle_is_untouched(case):
    """psm_solve before and after delta steps returns the bits it returns on a handle that never took a delta step, and it
    neither reads nor moves the state."""
    a3, a5 = case.arrays[3], case.arrays[5]
    sur, plain = handle(case), handle(case)
    try:
        ref = step(plain, a5, "psm_solve")
        np.testing.assert_array_equal(step(sur, a5, "psm_solve"), ref)
        assert state(sur) == (0, 0)
        prime(sur, a3)
        step(sur, a5)
        np.testing.assert_array_equal(step(sur, a5, "psm_solve"), ref)
        assert state(sur) == (1, 1)
    finally:
        sur.close(); plain.close()


def test_python_mirror(case):
    """SolverModule(step='delta') and SolverEnsemble(step='delta'): init_func primes with its own array, py_func steps."""
    sm = SolverModule(case.model, MAXS, step="delta")
    assert sm.init_func(case.arrays[0], case.top, case.obst) == 0
    assert sm.state == (True, 0)
    a3 = case.arrays[3]
    p = sm.py_func(a3)
    check_against_reference(p, a3, case.ref(0, 3), "SolverModule 0 -> 3")     # geometry='scipy': the tables are the oracle's
    assert sm.state == (True, 1)
    sm.py_func_begin(case.arrays[5])
    p5 = sm.py_func_end()
    sm.prime(a3)
    np.testing.assert_array_equal(sm.py_func(case.arrays[5]), p5)
    sm.reset_state()
    assert sm.state == (False, 0)
    np.testing.assert_array_equal(sm.py_func(a3), a3[:, 4])
    native = SolverModule(case.model, MAXS, geometry="native", step="delta")
    native.init_func(case.arrays[0], case.top, case.obst)
    assert native.state == (True, 0) and np.isfinite(native.py_func(a3)).all()
    meshes = [synthetic.channel_mesh(**kw) for kw in OBSTACLES[:2]]
    ens = SolverEnsemble(case.model, MAXS, max_cases=2, step="delta")
    ens.init_func([m[0] for m in meshes], [m[1] for m in meshes], [m[2] for m in meshes])
    assert ens.state == (True, 0)
    nxt = [synthetic.channel_mesh(**dict(kw, step=kw.get("step", 0) + 3))[0] for kw in OBSTACLES[:2]]
    ps = ens.py_func(nxt)
    assert ens.state == (True, 1) and all(np.isfinite(q).all() and len(q) == len(a) for q, a in zip(ps, nxt))
    ens.reset_state()
    for q, a in zip(ens.py_func(nxt), nxt):
        np.testing.assert_array_equal(q, a[:, 4])
